/*
 * Host header walk: the frame boundaries of a received byte stream in host memory
 * (include/ws/frame.h, netc_ws_scan_frames_host) -- the CPU counterpart of
 * netc_gpu_scan_frames, with the same outputs and the same strict checks.
 *
 * It hops from header to header (src/ws/common.c:146-296: byte 0 :157-161, byte 1
 * MASK + 7-bit length :180-181, 16 / 64-bit big-endian extended length :223-245,
 * 4 key bytes :273-289), so its cost is O(frames), not O(bytes): for streams of
 * large frames it beats any scan that has to look at every byte, which is why the
 * ingest ring (ws_ingest.hip) uses it for slots whose frames are large.
 */
#include <stdint.h>
#include <string.h>

#include "../../../include/ws/frame.h"
#include "../../../include/ws/mask.h"
#include "ws_header.h"

int netc_ws_scan_frames_host(const void *wire, size_t len, uint64_t start, int flags, uint64_t *hdr,
                             uint32_t *keys, uint8_t *b0, size_t max_frames, uint64_t *result)
{
    if (!result || (len && !wire) || (max_frames && (!hdr || !keys || !b0)) || (flags & ~NETC_WS_SCAN_STRICT))
        return NETC_GPU_EINVAL;
    const uint8_t *w = (const uint8_t *)wire;
    const int strict = (flags & NETC_WS_SCAN_STRICT) != 0;
    uint64_t n = 0, p = start;
    uint64_t error = UINT64_MAX;
    struct ws_header_view h;
    /* judged as soon as byte 1 and the extended length are there: the key may still be missing */
    while (p < len && ws_header_decode(w + p, len - p, &h)) {
        if (strict && ws_header_forbidden(&h)) {
            error = p;
            break;
        }
        const uint64_t room = len - p;
        if (h.hlen > room || h.plen > room - h.hlen) break;   /* the frame is not complete yet */
        if (n < max_frames) {
            hdr[n] = p;
            keys[n] = h.key;
            b0[n] = h.first;
        }
        ++n;
        p += h.hlen + h.plen;
    }
    if (hdr && n <= max_frames) hdr[n] = p;
    result[NETC_WS_SCAN_FRAMES] = n;
    result[NETC_WS_SCAN_CONSUMED] = p;
    result[NETC_WS_SCAN_ERROR] = error;
    return 0;
}
