/* TEST ONLY (tests/test_ring_shared.py): netc_amd/csrc/host/ws_header.h's static inline functions
 * as exported symbols. */
#include "../../netc_amd/csrc/host/ws_header.h"

/* ws_header_decode; out5 = hlen, plen, key, first, second (written when it returns 1) */
int shim_header_decode(const uint8_t *w, uint64_t avail, uint64_t *out5)
{
    struct ws_header_view h;
    if (!ws_header_decode(w, avail, &h)) return 0;
    out5[0] = h.hlen, out5[1] = h.plen, out5[2] = h.key, out5[3] = h.first, out5[4] = h.second;
    return 1;
}

/* ws_header_forbidden of the header decoded from w; -1 when it does not decode yet */
int shim_header_forbidden(const uint8_t *w, uint64_t avail)
{
    struct ws_header_view h;
    return ws_header_decode(w, avail, &h) ? ws_header_forbidden(&h) : -1;
}

uint64_t shim_header_len(uint64_t payload_len, int masked) { return ws_header_len(payload_len, masked); }
uint64_t shim_header_len_of(uint8_t second) { return ws_header_len_of(second); }
