"""netc_ws_decode_frames_host (libnetc.so), the host twin of netc_gpu_decode_frames, against the
two oracles of tests/decodeutil.py -- and, oracle only, proof that the wires the decode tests
use contain what they claim (conditions on the input, no code under test involved).

The twin runs on netc_ws_scan_frames_host's outputs, into sentinel-filled arrays: every used
entry must equal the expectation and nothing outside payload[0, BYTES), offsets[0, n],
msg_first[0, M], msg_opcode[0, M) and dresult[0, 3) may change.
"""

import numpy as np
import pytest

from netc_amd import _lib
from netc_amd import mask as nm
from oracle import oracle as orc
from tests import decodeutil as du
from tests.scanutil import GUARD, PAD, SENTINEL, frame_fields

OFF_S, OP_S = np.uint64(0xF9F9F9F9F9F9F9F9), 0xEE


def run_host(wire, length=None, strict=True, max_frames=None, messages=True, exp=None):
    length = wire.size if length is None else length
    if exp is None:
        exp = du.Expected(wire, length, strict=strict, max_frames=max_frames)
    cap = exp.found if max_frames is None else max_frames
    hdr, keys, b0, res = nm.scan_frames_host(wire, cap, strict=strict, length=length)
    assert int(res[0]) == exp.found
    if cap < exp.found:
        hdr[cap] = OFF_S   # the scan leaves hdr[max_frames] alone when it found more: nothing may rely on it
    payload = np.full(length + 2 * GUARD, SENTINEL, dtype=np.uint8)
    off = np.full(cap + 1 + 2 * PAD, OFF_S, dtype=np.uint64)
    first = np.full(cap + 1 + 2 * PAD, OFF_S, dtype=np.uint64)
    op = np.full(max(cap, 1) + 2 * PAD, OP_S, dtype=np.uint8)
    dres = np.full(3 + 2 * PAD, OFF_S, dtype=np.uint64)
    w = np.ascontiguousarray(wire)
    before = w.copy()
    keys_, b0_ = np.ascontiguousarray(keys), np.ascontiguousarray(b0)
    rc = _lib.host().netc_ws_decode_frames_host(
        payload[GUARD:].ctypes.data, length, off[PAD:].ctypes.data, first[PAD:].ctypes.data if messages else None,
        op[PAD:].ctypes.data if messages else None, dres[PAD:].ctypes.data, w.ctypes.data, length, hdr.ctypes.data,
        keys_.ctypes.data if cap else None, b0_.ctypes.data if cap else None, cap, res.ctypes.data)
    assert rc == 0
    assert np.array_equal(w, before), "the wire changed"
    want = np.full(payload.size, SENTINEL, dtype=np.uint8)
    want[GUARD: GUARD + exp.payload.size] = exp.payload
    bad = np.nonzero(payload != want)[0]
    assert bad.size == 0, f"{bad.size} payload bytes differ or were written outside [0, BYTES), first at {bad[:8] - GUARD}"
    for name, arr, used, s in (("offsets", off, exp.n + 1, OFF_S), ("msg_first", first, exp.m + 1 if messages else 0, OFF_S),
                               ("msg_opcode", op, exp.m if messages else 0, OP_S), ("dresult", dres, 3, OFF_S)):
        outside = np.concatenate([arr[:PAD], arr[PAD + used:]])
        assert (outside == s).all(), f"{name}: written outside its {used} used entries"
    exp.check_tables(off[PAD:], first[PAD:] if messages else None, op[PAD:] if messages else None, dres[PAD:])
    return exp


@pytest.mark.parametrize("name", du.WHOLE_WIRES)
def test_host_twin_on_every_wire(name):
    wire, strict, batch, exp = du.case(name)
    assert exp.n > 0
    if batch is not None:
        du.check_round_trip(exp, batch)
    run_host(wire, strict=strict, exp=exp)
    run_host(wire, strict=strict, exp=exp, messages=False)


def test_python_mirror_returns_the_same():
    wire, strict, _, exp = du.case("frag_open")
    hdr, keys, b0, res = nm.scan_frames_host(wire, exp.found, strict=strict)
    payload, off, first, op, dres = nm.decode_frames_host(wire, hdr, keys, b0, res)
    assert np.array_equal(payload, exp.payload)
    exp.check_tables(off, first, op, dres)
    assert first.size == exp.m + 1 and op.size == exp.m and off.size == exp.n + 1
    assert nm.decode_frames_host(wire, hdr, keys, b0, res, messages=False)[2] is None


@pytest.mark.parametrize("at_cap", [None] + sorted(du.LENGTH_CLASS))
def test_max_frames_caps(at_cap):
    wire, _ = du.wire_caps(at_cap)
    n = 400
    for cap in (0, 1, 100, n - 1, n, n + 5):
        exp = run_host(wire, max_frames=cap)
        assert exp.found == n and exp.n == min(cap, n)   # frames past the cap are not decoded
    if at_cap is not None:
        hdr = orc.scan_frames(wire)[0]
        assert frame_fields(wire, int(hdr[99]))[1] == du.LENGTH_CLASS[at_cap]


@pytest.mark.parametrize("last", sorted(du.LENGTH_CLASS))
def test_truncation(last):
    for prev in sorted(du.LENGTH_CLASS):
        wire, wo = du.wire_truncation(prev, last)
        n = wo.size - 1
        for d in (0, 1, 2, 3, 5, 7, 9, 13, 14):
            assert run_host(wire, length=int(wo[n - 1]) + d).n == n - 1
        assert run_host(wire, length=wire.size - 1).n == n - 1
        assert run_host(wire).n == n


def test_strict_error_mid_stream():
    wire, strict, _, exp = du.case("error")
    assert exp.n == 100 and exp.scan[4] is not None and exp.scan[4] < wire.size   # frames before the error only


def test_very_short_streams():
    masked, mixed = du.wires_short()
    for length in range(0, 49):
        run_host(masked, length=length)
        run_host(mixed, length=length, strict=False)


def test_argument_errors():
    wire, strict, _, exp = du.case("alignment")
    hdr, keys, b0, res = nm.scan_frames_host(wire, exp.found)
    payload = np.zeros(wire.size, np.uint8)
    off, first = np.zeros(exp.found + 1, np.uint64), np.zeros(exp.found + 1, np.uint64)
    op, dres = np.zeros(exp.found, np.uint8), np.zeros(3, np.uint64)
    p = lambda a: a.ctypes.data
    good = [p(payload), payload.size, p(off), p(first), p(op), p(dres), p(wire), wire.size, p(hdr), p(keys), p(b0),
            exp.found, p(res)]
    f = _lib.host().netc_ws_decode_frames_host
    assert f(*good) == 0
    for i in (0, 2, 5, 6, 8, 9, 10, 12):          # each required pointer
        bad = list(good)
        bad[i] = None
        assert f(*bad) == nm.NETC_GPU_EINVAL, i
    for i in (3, 4):                              # exactly one of the message arrays
        bad = list(good)
        bad[i] = None
        assert f(*bad) == nm.NETC_GPU_EINVAL, i
    bad = list(good)
    bad[1] = wire.size - 1                        # capacity below the stream length
    assert f(*bad) == nm.NETC_GPU_EINVAL
    both = np.zeros(2 * wire.size, np.uint8)      # payload overlapping the wire
    both[:wire.size] = wire
    for at in (0, wire.size - 1):
        bad = list(good)
        bad[0], bad[6] = p(both[at:]), p(both)
        assert f(*bad) == nm.NETC_GPU_EINVAL
    bad = list(good)
    bad[0], bad[6] = p(both[wire.size:]), p(both)   # adjacent: fine
    assert f(*bad) == 0


# --------------------------------------------- conditions on the input ----

def frames_touched_per_vector(off, shift):
    """non-empty frames touching each 16-byte destination vector (destination misaligned by shift)"""
    ln = np.diff(off.astype(np.int64))
    s, e = off[:-1].astype(np.int64)[ln > 0] + shift, off[1:].astype(np.int64)[ln > 0] + shift
    # frames that start at or before vector v, minus those that end before it
    starts = np.zeros(int(off[-1] + shift) // 16 + 2, dtype=np.int64)
    np.add.at(starts, s // 16, 1)
    ends_before = np.zeros_like(starts)
    np.add.at(ends_before, (e - 1) // 16 + 1, 1)
    return np.cumsum(starts) - np.cumsum(ends_before)


def longest_zero_run(off):
    ln = np.diff(off.astype(np.int64))
    best = run = 0
    for z in (ln == 0).tolist():
        run = run + 1 if z else 0
        best = max(best, run)
    return best


def test_dense_wire_reaches_every_gather_case():
    _, _, _, exp = du.case("dense")
    off = exp.off.astype(np.int64)
    assert 29000 < exp.n < 32000
    for shift in (0, 5):
        per_vec = frames_touched_per_vector(exp.off, shift)
        assert (per_vec >= 3).sum() > 50, "no 16-byte destination vector touches 3 frames"
        # frames (empty ones included: they sit in the table too) starting in each 4 KiB chunk
        per_chunk = np.bincount((off[:-1] + shift) // du.CHUNK)
        assert (per_chunk > 64).sum() >= 5 and per_chunk.max() > 300
        # chunks that 1-2 frames cover: inside or between the 3-9 KiB frames
        first_in = np.searchsorted(off, np.arange(0, int(off[-1]) + shift, du.CHUNK) - shift, side="right") - 1
        last_in = np.searchsorted(off, np.minimum(np.arange(du.CHUNK, int(off[-1]) + shift + du.CHUNK, du.CHUNK)
                                                  - shift, off[-1]) - 1, side="right") - 1
        assert ((last_in - np.maximum(first_in, 0)) <= 1).sum() >= 5
        ln = np.diff(off)
        crosses = ((off[:-1] + shift) // du.CHUNK != (off[1:] + shift - 1) // du.CHUNK) & (ln > 0)
        assert crosses.sum() >= 10, "no frame's payload crosses a chunk boundary"
    assert longest_zero_run(exp.off) >= 64
    assert exp.n > 3 * du.TILE    # the look-back of the offsets scan runs across many blocks


def test_zero_run_wires_hold_their_runs():
    for place in ("whole", "start", "end"):
        _, _, _, exp = du.case("zero_" + place)
        assert longest_zero_run(exp.off) >= 200 and exp.n >= 402
        ln = np.diff(exp.off.astype(np.int64))
        assert (ln == 1).any() and (ln == 5000).any()
    assert du.case("zero_start")[3].n > 2 * du.TILE


def test_fragmented_wires_hold_their_messages():
    _, _, _, strict = du.case("frag_strict")
    per_msg = np.diff(strict.first.astype(np.int64))
    for want in (1, 2, 3, 300, 700):
        assert (per_msg == want).any(), f"no message of {want} frames"
    ln = np.diff(strict.off.astype(np.int64))
    assert any(ln[a:b].sum() == 0 and b - a >= 3 for a, b in zip(strict.first[:-1].astype(int), strict.first[1:].astype(int)))
    assert strict.open_frames == 0 and strict.n > 3 * du.TILE
    assert set(strict.opcode.tolist()) >= {0, 1, 2, 9, 10}
    # a message spanning three scan blocks: its opcode crosses a block with no opcode of its own
    assert (per_msg >= 2 * du.TILE + 2).any()

    _, _, _, open_ = du.case("frag_open")
    assert open_.open_frames == 4 and open_.m == strict.m and int(open_.first[-1]) == open_.n - 4

    _, _, _, nofin = du.case("frag_nofin")
    assert nofin.m == 0 and nofin.open_frames == nofin.n == 600 and nofin.first.tolist() == [0]

    _, _, _, loose = du.case("frag_loose")
    b0 = loose.scan[2]
    inside = [m for m in range(loose.m)
              if int(loose.first[m + 1] - loose.first[m]) >= 4
              and ((b0[int(loose.first[m]) + 1: int(loose.first[m + 1]) - 1] & 0x0F) >= 8).any()
              and ((b0[int(loose.first[m]): int(loose.first[m + 1])] & 0x0F) < 8).sum() >= 3]
    assert inside, "no message of >= 3 fragments with a control frame inside it"
    assert loose.opcode[inside[0]] in (9, 10)          # the last non-zero opcode: the control frame's
    cont_only = [m for m in range(loose.m) if not (b0[int(loose.first[m]): int(loose.first[m + 1])] & 0x0F).any()]
    assert cont_only and all(loose.opcode[m] == 0 for m in cont_only)
    assert any(int(loose.first[m + 1] - loose.first[m]) == 300 for m in cont_only)


def test_mixed_and_text_wires():
    wire, _, _, mixed = du.case("mixed")
    second = wire[mixed.scan[0].astype(np.int64) + 1]
    assert 100 < ((second & 0x80) == 0).sum() < mixed.n - 100        # both kinds of frame
    assert du.case("mixed_strict")[3].n < mixed.n
    _, _, batch, text = du.case("text")
    verdicts = orc.validate_batch(batch[0], batch[1], batch[3])
    fin_text = (batch[3] & 0x80) != 0
    assert 50 < (verdicts[fin_text] == 0).sum() < fin_text.sum() - 50   # valid and invalid messages
