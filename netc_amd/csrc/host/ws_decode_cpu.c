/*
 * Host frame decode: the frames a scan recorded in a wire stream in host memory as a mask.h
 * batch plus a message table (include/ws/frame.h, netc_ws_decode_frames_host) -- the CPU
 * counterpart of netc_gpu_decode_frames, with the same outputs and the same write bounds.
 *
 * A serial walk: per frame the header length from byte 1 (src/ws/common.c:180-181, :223-245,
 * :273-289), the payload copied and unmasked from phase 0 (:317-323, netc_ws_mask), and the
 * message rule of ws_parse_frame (:163-164 the last non-zero opcode, :303-347 a message ends
 * at the next FIN).
 */
#include <stdint.h>
#include <string.h>

#include "../../../include/ws/frame.h"
#include "../../../include/ws/mask.h"
#include "ws_header.h"

int netc_ws_decode_frames_host(void *payload, size_t payload_capacity, uint64_t *offsets, uint64_t *msg_first,
                               uint8_t *msg_opcode, uint64_t *dresult, const void *wire, size_t len,
                               const uint64_t *hdr, const uint32_t *keys, const uint8_t *b0, size_t max_frames,
                               const uint64_t *result)
{
    if (!offsets || !dresult || !hdr || !result || (max_frames && (!keys || !b0))) return NETC_GPU_EINVAL;
    if ((msg_first == NULL) != (msg_opcode == NULL)) return NETC_GPU_EINVAL;
    if (len && (!wire || !payload)) return NETC_GPU_EINVAL;
    if (payload_capacity < len) return NETC_GPU_EINVAL;
    if (len && payload_capacity) {
        const uintptr_t x = (uintptr_t)payload, y = (uintptr_t)wire;
        if (x < y + len && y < x + payload_capacity) return NETC_GPU_EINVAL;
    }
    const uint8_t *w = (const uint8_t *)wire;
    uint8_t *out = (uint8_t *)payload;
    const uint64_t found = len >= 2 ? result[NETC_WS_SCAN_FRAMES] : 0;
    const uint64_t n = found < max_frames ? found : max_frames;
    uint64_t q = 0, messages = 0;
    uint8_t opcode = 0;
    offsets[0] = 0;
    if (msg_first) msg_first[0] = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t p = hdr[k];
        const uint64_t hl = ws_header_len_of(w[p + 1]);
        uint64_t plen;
        if (k + 1 < n || found <= max_frames) {
            plen = hdr[k + 1] - p - hl;
        } else {   /* max_frames cut the record short: hdr[n] is not there, the length is in the header */
            struct ws_header_view h;
            plen = ws_header_decode(w + p, hl, &h) ? h.plen : 0;   /* (a recorded frame's header is whole) */
        }
        if (plen) {
            const uint32_t key = keys[k];
            const uint8_t kb[4] = {(uint8_t)key, (uint8_t)(key >> 8), (uint8_t)(key >> 16), (uint8_t)(key >> 24)};
            netc_ws_mask(out + q, w + p + hl, (size_t)plen, kb, 0);
        }
        q += plen;
        offsets[k + 1] = q;
        if (b0[k] & 0x0Fu) opcode = b0[k] & 0x0Fu;
        if (b0[k] & 0x80u) {
            if (msg_first) {
                msg_first[messages + 1] = k + 1;
                msg_opcode[messages] = opcode;
            }
            ++messages;
            opcode = 0;
        }
    }
    dresult[NETC_WS_DECODE_FRAMES] = n;
    dresult[NETC_WS_DECODE_BYTES] = q;
    dresult[NETC_WS_DECODE_MESSAGES] = messages;
    return 0;
}
