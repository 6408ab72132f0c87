"""Helpers shared by the scan / scan -> unmask parity tests.  Test infrastructure only.

Expected values come from the oracle (oracle_scan_frames, oracle_encode_batch) and numpy,
never from the code under test.
"""

import numpy as np

from oracle import oracle as orc

GUARD = 64
SENTINEL = 0xA5
PAD = 8                      # guard entries on either side of every scan output
HDR_SENTINEL = -7            # int64
KEY_SENTINEL = 0x5A5A5A5A    # int32
RES_SENTINEL = -7            # int64


class ScanOutputs:
    """netc_gpu_scan_frames' outputs for `cap` frames, carved out of larger sentinel-filled
    tensors (hdr and res 8-aligned, keys 4-aligned): `check_guards` proves that nothing outside
    hdr[0, cap], keys[0, cap), b0[0, cap) and res[0, 3) was written."""

    def __init__(self, torch, cap):
        self.cap = cap
        kn = max(cap, 1)   # a one-entry slice for cap 0 (an empty tensor has no address); it is guard too
        self.hdr_buf = torch.full((cap + 1 + 2 * PAD,), HDR_SENTINEL, dtype=torch.int64, device="cuda")
        self.keys_buf = torch.full((kn + 2 * PAD,), KEY_SENTINEL, dtype=torch.int32, device="cuda")
        self.b0_buf = torch.full((kn + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.res_buf = torch.full((3 + 2 * PAD,), RES_SENTINEL, dtype=torch.int64, device="cuda")
        self.hdr = self.hdr_buf[PAD: PAD + cap + 1]
        self.keys = self.keys_buf[PAD: PAD + kn]
        self.b0 = self.b0_buf[PAD: PAD + kn]
        self.res = self.res_buf[PAD: PAD + 3]
        assert self.hdr.data_ptr() % 8 == 0 and self.res.data_ptr() % 8 == 0 and self.keys.data_ptr() % 4 == 0

    def check_guards(self):
        cap = self.cap
        for name, buf, used, sentinel in (("hdr", self.hdr_buf, cap + 1, HDR_SENTINEL),
                                          ("keys", self.keys_buf, cap, KEY_SENTINEL),
                                          ("b0", self.b0_buf, cap, SENTINEL), ("res", self.res_buf, 3, RES_SENTINEL)):
            whole = buf.cpu().numpy()
            outside = np.concatenate([whole[:PAD], whole[PAD + used:]])
            bad = np.nonzero(outside != sentinel)[0]
            assert bad.size == 0, (f"{name}: {bad.size} entries written outside its capacity of {used}, first at "
                                   f"{[int(i) - PAD if i < PAD else int(i) - PAD + used for i in bad[:8]]}")

    def check_scan(self, exp_hdr, exp_keys, exp_b0, exp_consumed, exp_err):
        """the scan outputs equal the oracle's (call after a synchronise)"""
        n, cap = exp_hdr.size, self.cap
        r = self.res.cpu().numpy().view(np.uint64)
        assert int(r[0]) == n, f"frames {int(r[0])} != {n}"
        assert int(r[1]) == exp_consumed, f"consumed {int(r[1])} != {exp_consumed}"
        assert (None if int(r[2]) == (1 << 64) - 1 else int(r[2])) == exp_err
        k = min(n, cap)
        got_hdr = self.hdr.cpu().numpy().view(np.uint64)
        assert np.array_equal(got_hdr[:k], exp_hdr[:k]), \
            f"header offsets differ at {np.nonzero(got_hdr[:k] != exp_hdr[:k])[0][:4]}"
        assert np.array_equal(self.keys.cpu().numpy().view(np.uint32)[:k], exp_keys[:k])
        assert np.array_equal(self.b0.cpu().numpy()[:k], exp_b0[:k])
        if n <= cap:
            assert int(got_hdr[n]) == exp_consumed
        self.check_guards()


def frame_fields(wire, p):
    """(header length, payload length, MASK bit) of the frame whose header starts at wire[p]"""
    second = int(wire[p + 1])
    code = second & 0x7F
    ext = 2 if code == 126 else (8 if code == 127 else 0)
    ln = code if ext == 0 else int.from_bytes(wire[p + 2: p + 2 + ext].tobytes(), "big")
    return 2 + ext + (4 if second & 0x80 else 0), ln, bool(second & 0x80)


def expected_unmasked(wire, length=None, start=0, strict=True, max_frames=None):
    """What scan -> unmask in place must leave in `wire` (all of it, the bytes from `length` on
    included), and the oracle's scan of wire[:length].  Frame k < min(found, max_frames): its
    payload XORed with its key from phase 0 (key 0 when its MASK bit is clear); every other byte --
    headers, bytes before `start`, frames past max_frames, the incomplete frame at the end,
    everything from a strict error on -- as in the input."""
    length = wire.size if length is None else length
    scan = orc.scan_frames(wire[:length], start=start, strict=strict)
    hdr, keys = scan[0], scan[1]
    exp = wire.copy()
    k = hdr.size if max_frames is None else min(hdr.size, max_frames)
    for i in range(k):
        p = int(hdr[i])
        hl, ln, masked = frame_fields(wire, p)
        assert p + hl + ln <= length
        if masked and ln:
            kb = np.frombuffer(int(keys[i]).to_bytes(4, "little"), dtype=np.uint8)
            exp[p + hl: p + hl + ln] ^= np.resize(kb, ln)
    return exp, scan


def stream_of(rng, sizes, masked=True, b0=None):
    """(wire, wire offsets) of random payloads of `sizes` under random keys (oracle_encode_batch)"""
    sizes = np.asarray(sizes, dtype=np.uint64)
    off = np.zeros(sizes.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum(sizes)
    payload = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    keys = rng.integers(0, 2**32, sizes.size, dtype=np.uint64).astype(np.uint32)
    return orc.encode_batch(payload, off, keys, b0, masked)
