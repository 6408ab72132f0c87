"""GPU parity: netc_gpu_scan_frames -> netc_gpu_decode_frames (ws_decode_gpu.hip) against the
two oracles of tests/decodeutil.py.

Every case queues the scan and the decode on one stream with no synchronisation between them,
then compares the whole payload tensor (guards on both sides included: not a byte outside
[0, BYTES) may change), offsets / msg_first / msg_opcode / dresult carved out of sentinel-filled
tensors (decodeutil.DecodeOutputs), the scan outputs (ScanOutputs.check_scan) and the wire
itself, which the out-of-place decode must leave unchanged.  The wires are proven to contain
what they claim in tests/test_decode_host.py, on the CPU.
"""

import numpy as np
import pytest

from netc_amd import _lib
from netc_amd import mask as nm
from oracle import oracle as orc
from tests import decodeutil as du
from tests.scanutil import GUARD, SENTINEL, ScanOutputs

pytestmark = pytest.mark.gpu


def run_decode(torch, wire, shift=0, dshift=0, strict=True, max_frames=None, length=None, exp=None, outs=None,
               dec=None, messages=True, place=True):
    """scan -> decode of wire[:length] (wire at a buffer offset of GUARD + shift, payload at
    GUARD + dshift) on the current stream; checks everything.  Returns (Expected, payload tensor,
    offsets tensor, ScanOutputs)."""
    length = wire.size if length is None else length
    if exp is None:
        exp = du.Expected(wire, length, strict=strict, max_frames=max_frames)
    cap = exp.found if max_frames is None else max_frames
    outs = outs or ScanOutputs(torch, cap)
    dec = dec or du.DecodeOutputs(torch, cap, messages)
    assert outs.cap == cap and dec.cap == cap
    dec.reset()
    wbuf = torch.full((wire.size + 2 * GUARD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    w = wbuf[GUARD + shift: GUARD + shift + wire.size]
    w.copy_(torch.from_numpy(wire))
    wire_before = wbuf.cpu().numpy()
    capacity = max(length, 1)
    pbuf = torch.full((capacity + 2 * GUARD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    lo = GUARD + dshift
    payload = pbuf[lo: lo + capacity]
    nm.scan_frames(w, outs.hdr, outs.keys, outs.b0, outs.res, strict=strict, length=length)
    nm.decode_frames(payload, dec.off, dec.first, dec.op, dec.res, w, outs.hdr, outs.keys, outs.b0, outs.res,
                     length=length)
    torch.cuda.current_stream().synchronize()
    outs.check_scan(*exp.scan)
    dec.check(exp)
    got = pbuf.cpu().numpy()
    want = np.full(got.size, SENTINEL, dtype=np.uint8)
    want[lo: lo + exp.payload.size] = exp.payload
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{bad.size} payload bytes differ or were written outside [0, {exp.payload.size}), first at "
                             f"{(bad[:8] - lo).tolist()} (len={wire.size}, length={length}, frames={exp.n}, "
                             f"max_frames={max_frames}, strict={strict}, shift={shift}, dshift={dshift})")
    assert np.array_equal(wbuf.cpu().numpy(), wire_before), "the decode changed the wire"
    return exp, payload, dec, outs


@pytest.mark.parametrize("dshift", [0, 1, 15])
@pytest.mark.parametrize("shift", [0, 1, 7, 8, 15])
def test_alignment(torch_cuda, shift, dshift):
    wire, strict, _, exp = du.case("alignment")
    assert run_decode(torch_cuda, wire, shift=shift, dshift=dshift, exp=exp)[0].n == 51


@pytest.mark.parametrize("dshift", [0, 5])
def test_dense_tiny_frames(torch_cuda, dshift):
    wire, strict, _, exp = du.case("dense")
    assert run_decode(torch_cuda, wire, dshift=dshift, exp=exp)[0].n > 29000


@pytest.mark.parametrize("place", ["whole", "start", "end"])
def test_zero_length_runs(torch_cuda, place):
    wire, strict, batch, exp = du.case("zero_" + place)
    du.check_round_trip(exp, batch)
    for dshift in (0, 3):
        run_decode(torch_cuda, wire, dshift=dshift, exp=exp)


@pytest.mark.parametrize("kind", ["strict", "open", "nofin", "loose"])
def test_fragmentation(torch_cuda, kind):
    wire, strict, batch, exp = du.case("frag_" + kind)
    du.check_round_trip(exp, batch)
    run_decode(torch_cuda, wire, strict=strict, exp=exp, dshift=2)
    run_decode(torch_cuda, wire, strict=strict, exp=exp, messages=False)   # both message arrays NULL


def test_masked_and_unmasked_mixed(torch_cuda):
    wire, strict, _, exp = du.case("mixed")
    assert not strict
    run_decode(torch_cuda, wire, strict=False, exp=exp, dshift=9)
    # strict: the scan stops at the first unmasked header; only the frames before it are decoded
    run_decode(torch_cuda, wire, strict=True, exp=du.case("mixed_strict")[3], shift=9)


@pytest.mark.parametrize("at_cap", sorted(du.LENGTH_CLASS))
@pytest.mark.parametrize("onepass", ["0", "1"])
def test_max_frames_cap(torch_cuda, gpu_knob, onepass, at_cap):
    gpu_knob("SCAN_ONEPASS", onepass)
    wire, _ = du.wire_caps(at_cap)
    n = 400
    for cap in (0, 1, 100, n - 1, n, n + 5):
        exp = run_decode(torch_cuda, wire, max_frames=cap, dshift=1)[0]
        assert exp.found == n and exp.n == min(cap, n)   # frames past the cap are not decoded


@pytest.mark.parametrize("last", sorted(du.LENGTH_CLASS))
def test_truncation(torch_cuda, last):
    for prev in sorted(du.LENGTH_CLASS):
        wire, wo = du.wire_truncation(prev, last)
        n = wo.size - 1
        for d in (0, 1, 2, 3, 5, 7, 9, 13, 14):
            assert run_decode(torch_cuda, wire, length=int(wo[n - 1]) + d, shift=1)[0].n == n - 1
        assert run_decode(torch_cuda, wire, length=wire.size - 1, shift=1)[0].n == n - 1
        assert run_decode(torch_cuda, wire, shift=1)[0].n == n


def test_strict_error_mid_stream(torch_cuda):
    wire, strict, _, exp = du.case("error")
    assert exp.n == 100 and exp.scan[4] is not None
    for dshift in (0, 6):
        run_decode(torch_cuda, wire, exp=exp, dshift=dshift)   # the rest of the payload buffer stays untouched


@pytest.mark.parametrize("dshift", [0, 3])
def test_very_short_streams(torch_cuda, dshift):
    masked, mixed = du.wires_short()
    for length in range(0, 49):
        run_decode(torch_cuda, masked, length=length, dshift=dshift)
        run_decode(torch_cuda, mixed, length=length, shift=dshift, strict=False)


def test_non_default_stream(torch_cuda):
    torch = torch_cuda
    a, b = du.wires_two_streams()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        outs, dec = ScanOutputs(torch, 300), du.DecodeOutputs(torch, 300)
        try:
            assert run_decode(torch, a, max_frames=300, outs=outs, dec=dec)[0].n == 300
            assert run_decode(torch, b, max_frames=300, outs=outs, dec=dec, shift=2, dshift=7)[0].n == 251
            assert run_decode(torch, a, max_frames=300, outs=outs, dec=dec)[0].n == 300
        finally:
            nm.stream_release(s)


def test_decoded_batch_feeds_unmask_validate(torch_cuda):
    torch = torch_cuda
    wire, strict, batch, exp = du.case("text")
    du.check_round_trip(exp, batch)
    _, payload, dec, outs = run_decode(torch, wire, exp=exp)
    n = exp.n
    want = orc.validate_batch(batch[0], batch[1], batch[3])
    dst = torch.empty(exp.payload.size, dtype=torch.uint8, device="cuda")
    valid = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    zero_keys = torch.zeros(n, dtype=torch.int32, device="cuda")
    nm.unmask_validate(dst, payload[:exp.payload.size], dec.off[:n + 1], zero_keys, outs.b0[:n], valid)
    torch.cuda.synchronize()
    assert np.array_equal(valid.cpu().numpy(), want)
    assert np.array_equal(dst.cpu().numpy(), exp.payload)


@pytest.mark.parametrize("name", ["alignment", "frag_strict", "caps"])
def test_encode_of_the_decoded_batch_is_the_wire(torch_cuda, name):
    torch = torch_cuda
    wire, strict, _, exp = du.case(name)
    _, payload, dec, outs = run_decode(torch, wire, strict=strict, exp=exp, dshift=4)
    n = exp.n
    again = torch.full((nm.wire_bound(exp.payload.size, n, True) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    wo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    nm.encode_frames(again, wo, payload[:exp.payload.size], dec.off[:n + 1], outs.keys[:n], outs.b0[:n], masked=True)
    torch.cuda.synchronize()
    start, consumed = int(exp.scan[0][0]), exp.scan[3]
    assert int(wo[n]) == consumed - start
    assert np.array_equal(again[:consumed - start].cpu().numpy(), wire[start:consumed])


def test_argument_errors(torch_cuda):
    torch = torch_cuda
    wire, strict, _, exp = du.case("alignment")
    n = exp.found
    w = torch.from_numpy(wire).cuda()
    outs, dec = ScanOutputs(torch, n), du.DecodeOutputs(torch, n)
    nm.scan_frames(w, outs.hdr, outs.keys, outs.b0, outs.res)
    both = torch.full((2 * wire.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    both[:wire.size].copy_(w)
    payload = torch.full((wire.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    good = [0, p(payload), wire.size, p(dec.off), p(dec.first), p(dec.op), p(dec.res), p(w), wire.size, p(outs.hdr),
            p(outs.keys), p(outs.b0), n, p(outs.res), stream]
    f, err = _lib.gpu().netc_gpu_decode_frames, _lib.gpu().netc_gpu_strerror
    cases = [(i, None) for i in (1, 3, 6, 7, 9, 10, 11, 13)]      # each required pointer
    cases += [(4, None), (5, None)]                                # exactly one of the message arrays
    cases += [(2, wire.size - 1)]                                  # capacity below the stream length
    for i, v in cases:
        bad = list(good)
        bad[i] = v
        assert f(*bad) == nm.NETC_GPU_EINVAL, i
        assert err(), i
    for at in (0, wire.size - 1):                                  # payload overlapping the wire
        bad = list(good)
        bad[1], bad[7] = p(both) + at, p(both)
        assert f(*bad) == nm.NETC_GPU_EINVAL and b"overlap" in err()
    torch.cuda.synchronize()
    # no launch happened: every output still holds its sentinel
    assert bool((payload == SENTINEL).all()) and bool((both[wire.size:] == SENTINEL).all())
    assert bool((dec.off_buf == du.OFF_SENTINEL).all()) and bool((dec.res_buf == du.OFF_SENTINEL).all())
    assert bool((dec.first_buf == du.OFF_SENTINEL).all()) and bool((dec.op_buf == du.OP_SENTINEL).all())
    with pytest.raises(nm.NetcGpuError) as e:                      # the Python mirror raises the same code
        nm.decode_frames(payload[:-1], dec.off, dec.first, dec.op, dec.res, w, outs.hdr, outs.keys, outs.b0, outs.res)
    assert e.value.code == nm.NETC_GPU_EINVAL
    bad = list(good)
    bad[1], bad[7] = p(both) + wire.size, p(both)                  # adjacent buffers are fine
    assert f(*bad) == 0
    torch.cuda.synchronize()
    assert np.array_equal(both[wire.size: wire.size + exp.payload.size].cpu().numpy(), exp.payload)
