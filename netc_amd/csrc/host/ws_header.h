/*
 * One WebSocket frame header: its lengths, its key, and what a server must not accept
 * (src/ws/common.c:146-296: byte 0 :157-161, byte 1 MASK + 7-bit length :180-181, 16 / 64-bit
 * big-endian extended length :223-245, 4 key bytes :273-289).  Internal, not installed; C, so
 * the host library's walks and the rings' host code (inside extern "C") read a header the same
 * way.  Only the decoding and the predicate are shared: each walk keeps its own loop and its
 * own order of checks.
 */
#ifndef NETC_WS_HEADER_H
#define NETC_WS_HEADER_H

#include <stdint.h>
#include <string.h>

struct ws_header_view
{
    uint64_t hlen;   /* header bytes: 2 + extended length + key */
    uint64_t plen;   /* payload bytes */
    uint32_t key;    /* packed key32 (0 if MASK is clear, or the key bytes are not there yet) */
    uint8_t first, second;
};

/* extended-length bytes of a payload of this many bytes: the frame's length class (0, 2, 8) */
static inline unsigned ws_header_ext(uint64_t payload_len)
{
    return payload_len <= 125 ? 0u : (payload_len <= 0xFFFF ? 2u : 8u);
}

/* header bytes of a frame to send (src/ws/common.c:55-82; include/ws/frame.h) */
static inline uint64_t ws_header_len(uint64_t payload_len, int masked)
{
    return 2 + ws_header_ext(payload_len) + (masked ? 4 : 0);
}

/* header bytes of a received frame, from its byte 1 */
static inline uint64_t ws_header_len_of(uint8_t second)
{
    const unsigned code = second & 0x7Fu;
    return 2 + (code == 126 ? 2 : code == 127 ? 8 : 0) + ((second & 0x80u) ? 4 : 0);
}

/* 0 when byte 1 or the extended length is not among the `avail` bytes yet.  Else the lengths are
 * known; the whole header, key included, is there when avail >= h->hlen (the key is read then). */
static inline int ws_header_decode(const uint8_t *w, uint64_t avail, struct ws_header_view *h)
{
    if (avail < 2) return 0;
    h->first = w[0];
    h->second = w[1];
    h->hlen = ws_header_len_of(w[1]);
    const uint64_t key_bytes = (w[1] & 0x80u) ? 4 : 0;
    const uint64_t ext = h->hlen - 2 - key_bytes;
    if (avail < 2 + ext) return 0;
    uint64_t plen = w[1] & 0x7Fu;
    if (ext) {
        plen = 0;
        for (uint64_t i = 0; i < ext; ++i) plen = (plen << 8) | w[2 + i];
    }
    h->plen = plen;
    h->key = 0;
    if (key_bytes && avail >= h->hlen) {
        uint32_t k;
        memcpy(&k, w + 2 + ext, 4);   /* wire order k0 k1 k2 k3 -> little-endian key32 */
        h->key = k;
    }
    return 1;
}

/* RFC 6455 §5.1, §5.2, §5.5: what a server must not accept from a client (NETC_WS_SCAN_STRICT,
 * NETC_WS_INGEST_STRICT) */
static inline int ws_header_forbidden(const struct ws_header_view *h)
{
    const unsigned op = h->first & 0x0Fu;
    if (!(h->second & 0x80u)) return 1;               /* MASK clear */
    if (h->first & 0x70u) return 1;                   /* RSV1-3 */
    if ((op >= 3 && op <= 7) || op >= 11) return 1;   /* reserved opcodes */
    if (op >= 8 && (!(h->first & 0x80u) || h->plen > 125)) return 1;   /* control: FIN, <= 125 */
    if ((h->second & 0x7Fu) == 127 && (h->plen >> 63)) return 1;     /* 64-bit length, top bit */
    return 0;
}

#endif
