"""GPU parity: netc_gpu_scan_frames -> netc_gpu_unmask_frames (the receive route's unmask,
mask_np_kernel<.., ArgsScan> in ws_mask_gpu.hip) vs the oracle.

The kernel builds its frame table from the scan's outputs on the device: two virtual frames
per wire frame (header, key 0; payload), header lengths read from the buffer it rewrites, the
last frame's end decoded from its extended length, the frame count read from the scan result
and clamped to max_frames.  The checker (tests/scanutil.expected_unmasked) is
oracle_scan_frames plus a numpy header decode and XOR; the bar is every byte of the device
buffer, guards and the bytes past `length` included, and scan outputs equal to the oracle's
with nothing written outside their capacity.  The checker itself is proven on the CPU first
(test_checker_against_host_path) against netc_ws_scan_frames_host + netc_ws_mask.
"""

import numpy as np
import pytest

from netc_amd import mask as nm
from oracle import oracle as orc
from tests.scanutil import GUARD, SENTINEL, ScanOutputs, expected_unmasked, frame_fields, stream_of

gpu = pytest.mark.gpu


def run_unmask(torch, wire, shift=0, start=0, strict=True, max_frames=None, length=None, outs=None):
    """scan -> unmask of wire[:length] at buf[GUARD + shift:] on the current stream, no
    synchronisation between the two; checks the whole buffer and the scan outputs.  Returns the
    number of frames the oracle finds."""
    length = wire.size if length is None else length
    exp, scan = expected_unmasked(wire, length, start, strict, max_frames)
    n = scan[0].size
    if outs is None:
        outs = ScanOutputs(torch, n if max_frames is None else max_frames)
    assert max_frames is None or outs.cap == max_frames
    buf = torch.full((wire.size + 2 * GUARD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    lo, hi = GUARD + shift, GUARD + shift + wire.size
    w = buf[lo:hi]
    w.copy_(torch.from_numpy(wire))
    nm.scan_frames(w, outs.hdr, outs.keys, outs.b0, outs.res, start=start, strict=strict, length=length)
    nm.unmask_frames(w, outs.hdr, outs.keys, outs.res, length=length)
    torch.cuda.current_stream().synchronize()
    whole = buf.cpu().numpy()
    outs.check_scan(*scan)
    got = whole[lo:hi]
    if not np.array_equal(got, exp):
        bad = np.nonzero(got != exp)[0]
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[:8].tolist()} (len={wire.size}, length={length}, "
                             f"frames={n}, max_frames={max_frames}, start={start}, strict={strict}, shift={shift})")
    assert (whole[:lo] == SENTINEL).all() and (whole[hi:] == SENTINEL).all(), "write outside the stream"
    return n


# ------------------------------------------------------------------ wires ----

def wire_alignment():
    rng = np.random.default_rng(201)
    sizes = np.array(list(range(0, 40)) + [125, 126, 127, 1023, 1024, 1025, 4095, 4097, 65535, 65536, 70000])
    rng.shuffle(sizes)
    return stream_of(rng, sizes)


def wire_dense():
    """~30,000 frames: runs of 6-byte and 16-byte wire frames, of 0-3 byte payloads, of sizes
    from a small set, a run of 40-200 B, and frames of 3000-9000 B between the runs"""
    rng = np.random.default_rng(202)
    big = lambda: rng.integers(3000, 9001, 3)
    sizes = np.concatenate([np.zeros(6000, dtype=np.int64), big(), np.full(6000, 10), big(),
                            rng.integers(0, 4, 8500), big(),
                            rng.choice(np.array([0, 1, 4, 7, 8, 13, 16, 24]), 8500), big(),
                            rng.integers(40, 201, 1000), big()])
    return stream_of(rng, sizes)


def wire_mixed_masked():
    """blocks of 1-50 frames, masked and unmasked in turn"""
    rng = np.random.default_rng(203)
    parts, masked = [], True
    for _ in range(40):
        sizes = rng.choice(np.array([0, 1, 5, 125, 126, 300, 3000, 66000]), int(rng.integers(1, 51)),
                           p=[.15, .15, .2, .1, .1, .15, .14, .01])
        parts.append(stream_of(rng, sizes, masked=masked)[0])
        masked = not masked
    first_unmasked = parts[0].size
    return np.concatenate(parts), first_unmasked


def wire_strict_error():
    rng = np.random.default_rng(204)
    good, _ = stream_of(rng, rng.integers(0, 6000, 100))
    bad = np.frombuffer(bytes.fromhex("f285") + bytes(9), dtype=np.uint8)   # RSV1-3 set
    return np.concatenate([good, bad, good]), good.size


def spans_by_entries(wire, shift):
    """virtual table entries (header starts and payload starts) per 1 KiB span of the buffer"""
    hdr = orc.scan_frames(wire)[0]
    starts = np.concatenate([hdr, [int(p) + frame_fields(wire, int(p))[0] for p in hdr]]).astype(np.int64)
    return np.bincount((starts + shift) // 1024)


# --------------------------------------------------------------- CPU twin ----

def host_unmasked(wire, start=0, strict=True):
    """the host path on the same stream: netc_ws_scan_frames_host, then netc_ws_mask over each
    recorded frame's payload (from the end of its header to the next header)"""
    n = orc.scan_frames(wire, start=start, strict=strict)[0].size
    hdr, keys, _, res = nm.scan_frames_host(wire, n, start=start, strict=strict)
    assert int(res[0]) == n
    out = wire.copy()
    for k in range(n):
        p, q = int(hdr[k]), int(hdr[k + 1])
        second = int(wire[p + 1])
        hl = 2 + {126: 2, 127: 8}.get(second & 0x7F, 0) + (4 if second & 0x80 else 0)
        if second & 0x80 and q > p + hl:
            out[p + hl:q] = nm.mask_host(wire[p + hl:q], int(keys[k]).to_bytes(4, "little"))
    return out


@pytest.mark.parametrize("case", ["alignment", "dense", "mixed", "mixed_strict", "error"])
def test_checker_against_host_path(case):
    strict, start = True, 0
    if case == "alignment":
        wire = wire_alignment()[0]
    elif case == "dense":
        wire = wire_dense()[0]
    elif case in ("mixed", "mixed_strict"):
        wire, _ = wire_mixed_masked()
        strict = case == "mixed_strict"
    else:
        wire, _ = wire_strict_error()
    exp, scan = expected_unmasked(wire, strict=strict, start=start)
    assert scan[0].size > 0
    assert np.array_equal(exp, host_unmasked(wire, start, strict))
    assert not np.array_equal(exp, wire)


def test_dense_wire_reaches_every_table_case():
    # a condition on the input: spans of >= 64 virtual entries (the 63-entry-window walk), of
    # 3-63 (per lane) and sparse ones
    wire, _ = wire_dense()
    assert 29000 < orc.scan_frames(wire)[0].size < 32000
    for shift in (0, 5):
        per = spans_by_entries(wire, shift)
        assert (per >= 64).sum() > 50 and ((per >= 3) & (per <= 63)).sum() > 50 and (per <= 2).sum() > 5
        assert per.max() >= 300   # 6-byte frames: ~340 entries per span


# -------------------------------------------------------------- GPU cases ----

@gpu
@pytest.mark.parametrize("shift", [0, 1, 7, 8, 15])
def test_alignment(torch_cuda, shift):
    wire, _ = wire_alignment()
    assert run_unmask(torch_cuda, wire, shift=shift) == 51


@gpu
@pytest.mark.parametrize("shift", [0, 5])
def test_dense_tiny_frames(torch_cuda, shift):
    wire, _ = wire_dense()
    assert run_unmask(torch_cuda, wire, shift=shift) > 29000


@gpu
@pytest.mark.parametrize("onepass", ["0", "1"])
def test_max_frames_cap(torch_cuda, gpu_knob, onepass):
    gpu_knob("SCAN_ONEPASS", onepass)
    rng = np.random.default_rng(211)
    wire, _ = stream_of(rng, rng.integers(0, 2000, 400))
    n = 400
    for cap in (0, 1, 100, n - 1, n, n + 5):
        assert run_unmask(torch_cuda, wire, max_frames=cap) == n   # frames past the cap stay masked


@gpu
def test_start_offset(torch_cuda):
    rng = np.random.default_rng(212)
    wire, wo = stream_of(rng, rng.integers(0, 9000, 200))
    for s in (int(wo[1]), int(wo[100]), int(wo[199])):
        assert run_unmask(torch_cuda, wire, start=s, shift=3) > 0   # the frames before stay masked
    assert run_unmask(torch_cuda, wire, start=wire.size) == 0


LENGTH_CLASS = {"7bit": 100, "16bit": 1000, "64bit": 70000}


@gpu
@pytest.mark.parametrize("last", sorted(LENGTH_CLASS))
def test_truncation(torch_cuda, last):
    # the stream cut inside its last frame (and whole): the frame before the cut is the
    # kernel's last, its end decoded from its own extended length -- each length class
    for prev in sorted(LENGTH_CLASS):
        rng = np.random.default_rng(213)
        sizes = np.concatenate([rng.integers(0, 300, 20), [LENGTH_CLASS[prev] + 7, LENGTH_CLASS[last]]])
        wire, wo = stream_of(rng, sizes)
        n = sizes.size
        for d in (0, 1, 2, 3, 5, 7, 9, 13, 14):
            assert run_unmask(torch_cuda, wire, length=int(wo[n - 1]) + d, shift=1) == n - 1
        assert run_unmask(torch_cuda, wire, length=wire.size - 1, shift=1) == n - 1
        assert run_unmask(torch_cuda, wire, shift=1) == n


@gpu
def test_non_strict_with_unmasked_frames(torch_cuda):
    wire, first_unmasked = wire_mixed_masked()
    n = run_unmask(torch_cuda, wire, strict=False)
    second = wire[orc.scan_frames(wire, strict=False)[0].astype(np.int64) + 1]
    assert 100 < ((second & 0x80) == 0).sum() < n - 100    # both kinds of frame
    # strict: the scan stops at the first unmasked header; nothing from there on changes
    exp, scan = expected_unmasked(wire, strict=True)
    assert scan[4] == first_unmasked and np.array_equal(exp[first_unmasked:], wire[first_unmasked:])
    assert run_unmask(torch_cuda, wire, strict=True, shift=9) < n


@gpu
def test_strict_error_mid_stream(torch_cuda):
    wire, at = wire_strict_error()
    exp, scan = expected_unmasked(wire)
    assert scan[4] == at and np.array_equal(exp[at:], wire[at:]) and not np.array_equal(exp[:at], wire[:at])
    for shift in (0, 6):
        assert run_unmask(torch_cuda, wire, shift=shift) == 100


@gpu
@pytest.mark.parametrize("shift", [0, 3])
def test_very_short_streams(torch_cuda, shift):
    # 6-9 byte masked frames (strict), and 2-9 byte frames masked or not (non-strict), at every
    # length 0..48; the tensor stays full size, so the bytes past `length` are guards
    rng = np.random.default_rng(214)
    masked, _ = stream_of(rng, rng.integers(0, 4, 12))
    parts = [stream_of(rng, rng.integers(0, 8, 3), masked=False)[0], stream_of(rng, rng.integers(0, 4, 2))[0]] * 3
    mixed = np.concatenate(parts)
    assert masked.size >= 48 and mixed.size >= 48
    for length in range(0, 49):
        run_unmask(torch_cuda, masked, length=length, shift=shift)
        run_unmask(torch_cuda, mixed, length=length, shift=shift, strict=False)


@gpu
def test_non_default_stream(torch_cuda):
    # two different wires back to back on one stream, the same output tensors; then the
    # stream's scratch is released, as the header asks before a stream is dropped
    torch = torch_cuda
    rng = np.random.default_rng(215)
    a, _ = stream_of(rng, rng.integers(0, 3000, 300))
    b, _ = stream_of(rng, np.concatenate([rng.integers(0, 20, 250), [70000]]))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        outs = ScanOutputs(torch, 300)
        try:
            assert run_unmask(torch, a, max_frames=300, outs=outs) == 300
            assert run_unmask(torch, b, max_frames=300, outs=outs, shift=2) == 251
            assert run_unmask(torch, a, max_frames=300, outs=outs) == 300
        finally:
            nm.stream_release(s)
