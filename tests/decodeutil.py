"""Helpers shared by the frame-decode tests (host twin and GPU).  Test infrastructure only.

Expected values never come from the code under test.  Two independent sources:
  * the batch: oracle_scan_frames plus a numpy header decode and XOR (scanutil.expected_unmasked)
    gives every decoded frame's payload; for wires built with oracle_encode_batch the tests also
    hold the decode to the very payload / offsets / keys / header bytes that went in;
  * the message table: oracle_decode_message called again and again from the consumed offset
    gives each message's bytes and opcode; the frames per message are counted from the FIN bits
    of the oracle's header bytes.
"""

import functools

import numpy as np

from oracle import oracle as orc
from tests.scanutil import PAD, SENTINEL, expected_unmasked, frame_fields, stream_of
from tests.test_gpu_unmask_frames import wire_alignment, wire_dense, wire_mixed_masked, wire_strict_error

TILE = 256                   # frames one block of the offsets scan covers (one frame per thread)
CHUNK = 4096                 # destination bytes one wavefront of the gather covers
OFF_SENTINEL = -7            # int64
OP_SENTINEL = 0xEE


class Expected:
    """What a decode of wire[:length] must give (see the module docstring)."""

    def __init__(self, wire, length=None, start=0, strict=True, max_frames=None):
        length = wire.size if length is None else length
        unmasked, self.scan = expected_unmasked(wire, length, start, strict, max_frames)
        hdr, b0 = self.scan[0], self.scan[2]
        self.found = hdr.size
        self.n = n = self.found if max_frames is None else min(self.found, max_frames)
        self.off = np.zeros(n + 1, dtype=np.uint64)
        pieces, ends = [], np.zeros(n, dtype=np.int64)   # ends: wire offset of the end of frame k
        for k in range(n):
            p = int(hdr[k])
            hl, ln, _ = frame_fields(wire, p)
            pieces.append(unmasked[p + hl: p + hl + ln])
            self.off[k + 1] = self.off[k] + np.uint64(ln)
            ends[k] = p + hl + ln
        self.payload = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
        # messages: the reference's parser from the consumed offset on, over the decoded frames
        first, opcode = [0], []
        p = int(hdr[0]) if n else start
        for f in np.nonzero(b0[:n] & 0x80)[0].tolist():
            lo, hi = int(self.off[first[-1]]), int(self.off[f + 1])
            used, data, op = orc.decode_message(wire[p:int(ends[f])], cap=hi - lo + 1)
            assert used == int(ends[f]) - p, "the FIN bits and oracle_decode_message disagree on a message's end"
            assert data == self.payload[lo:hi].tobytes(), "the two oracles disagree on a message's bytes"
            first.append(f + 1)
            opcode.append(op)
            p = int(ends[f])
        if n and p < int(ends[n - 1]):   # the frames after the last FIN: an open message
            assert orc.decode_message(wire[p:int(ends[n - 1])])[0] == 0
        self.first = np.array(first, dtype=np.uint64)
        self.opcode = np.array(opcode, dtype=np.uint8)
        self.m = len(opcode)
        self.open_frames = n - first[-1]
        self.dresult = np.array([n, int(self.off[n]), self.m], dtype=np.uint64)

    def check_tables(self, off, first, opcode, dresult, what=""):
        """decoded tables (uint64 / uint8 arrays holding at least the used entries) against these"""
        assert np.array_equal(np.asarray(dresult)[:3], self.dresult), f"{what}dresult {dresult} != {self.dresult}"
        assert np.array_equal(off[:self.n + 1], self.off), \
            f"{what}offsets differ at {np.nonzero(off[:self.n + 1] != self.off)[0][:4]}"
        if first is not None:
            assert np.array_equal(first[:self.m + 1], self.first), \
                f"{what}msg_first differs at {np.nonzero(first[:self.m + 1] != self.first)[0][:4]}"
            assert np.array_equal(opcode[:self.m], self.opcode), \
                f"{what}msg_opcode differs at {np.nonzero(opcode[:self.m] != self.opcode)[0][:4]}"


# ------------------------------------------------------------------ wires ----

TEXT, BIN, CONT, FIN, PING, PONG = 0x01, 0x02, 0x00, 0x80, 0x09, 0x0A


def stream_with_b0(rng, frames, masked=True):
    """(wire, (payload, offsets, keys, b0)) of frames = [(header byte 0, payload size), ...]"""
    b0 = np.array([f[0] for f in frames], dtype=np.uint8)
    sizes = np.array([f[1] for f in frames], dtype=np.uint64)
    off = np.zeros(sizes.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum(sizes)
    payload = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    keys = rng.integers(0, 2**32, sizes.size, dtype=np.uint64).astype(np.uint32)
    wire, _ = orc.encode_batch(payload, off, keys, b0, masked)
    return wire, (payload, off, keys if masked else np.zeros(sizes.size, np.uint32), b0)


def zero_run_sizes():
    return [0] * 200 + [1] + [0] * 200 + [5000]


def wire_zero_runs(place):
    """200 empty frames, one 1-byte frame, 200 empty frames, one 5000-byte frame: alone, or at
    the start / the end of a longer stream"""
    rng = np.random.default_rng(301)
    other = rng.integers(0, 2000, 300).tolist()
    sizes = {"whole": zero_run_sizes(), "start": zero_run_sizes() + other, "end": other + zero_run_sizes()}[place]
    return stream_with_b0(rng, [(0x82, s) for s in sizes])


def message(rng, nframes, opcode=TEXT, size=lambda rng: int(rng.integers(0, 300)), between=None):
    """a message of nframes data frames (first `opcode`, then continuations, FIN on the last),
    `between`: a control header byte placed after every fragment but the last"""
    out = []
    for i in range(nframes):
        b = (opcode if i == 0 else CONT) | (FIN if i == nframes - 1 else 0)
        out.append((b, size(rng)))
        if between is not None and i < nframes - 1:
            out.append((between, int(rng.integers(0, 126))))
    return out


def wire_fragmented(kind):
    """streams whose header bytes the test chooses.  "strict": messages of 1, 2, 3, 300 and 700
    frames, one of empty frames only, PING / PONG (FIN set, as RFC 6455 requires) between
    messages and between fragments -- where, by the reference's rule, the control frame's FIN
    ends the message so far.  "open": the same, ending in an open message.  "nofin": no FIN at
    all (M = 0).  "loose" (non-strict scan): control frames WITHOUT FIN between the fragments
    of one message (it stays open across them; its opcode is the last non-zero one), and
    continuation-only messages, whose opcode is 0."""
    rng = np.random.default_rng(302)
    empty = lambda rng: 0
    if kind == "nofin":
        frames = [(TEXT, 10)] + [(CONT, int(rng.integers(0, 200))) for _ in range(599)]
    elif kind == "loose":
        frames = (message(rng, 3, between=PING) + message(rng, 1, CONT) + message(rng, 4, CONT)
                  + message(rng, 5, BIN, between=PONG) + message(rng, 300, CONT) + message(rng, 2, TEXT, between=PING))
    else:
        frames = (message(rng, 1) + [(PING | FIN, 5)] + message(rng, 2) + message(rng, 3, BIN)
                  + message(rng, 3, between=PING | FIN) + [(PONG | FIN, 0)] + message(rng, 300)
                  + message(rng, 4, size=empty) + message(rng, 700, BIN) + message(rng, 1, size=empty)
                  + message(rng, 4, between=PONG | FIN))
        if kind == "open":
            frames += message(rng, 5)[:-1]   # TEXT, 3 continuations, no FIN
    return stream_with_b0(rng, frames)


LENGTH_CLASS = {"7bit": 100, "16bit": 1000, "64bit": 70000}


def wire_caps(at_cap=None, cap=100):
    """400 frames of 0-1999 bytes; at_cap: the length class of frame cap - 1, the last one a
    decode capped at `cap` frames takes (its length comes from its own header)"""
    rng = np.random.default_rng(303)
    sizes = rng.integers(0, 2000, 400)
    if at_cap is not None:
        sizes[cap - 1] = LENGTH_CLASS[at_cap]
    return stream_with_b0(rng, [(0x82, int(s)) for s in sizes])


def wire_truncation(prev, last):
    """20 small frames, one of class `prev`, one of class `last` (tests cut inside the last)"""
    rng = np.random.default_rng(304)
    sizes = np.concatenate([rng.integers(0, 300, 20), [LENGTH_CLASS[prev] + 7, LENGTH_CLASS[last]]])
    return stream_of(rng, sizes)


def wires_short():
    """6-9 byte masked frames (strict), and 2-9 byte frames masked or not (non-strict): >= 48 B each"""
    rng = np.random.default_rng(305)
    masked, _ = stream_of(rng, rng.integers(0, 4, 12))
    parts = [stream_of(rng, rng.integers(0, 8, 3), masked=False)[0], stream_of(rng, rng.integers(0, 4, 2))[0]] * 3
    mixed = np.concatenate(parts)
    assert masked.size >= 48 and mixed.size >= 48
    return masked, mixed


def wires_two_streams():
    rng = np.random.default_rng(306)
    a, _ = stream_of(rng, rng.integers(0, 3000, 300))
    b, _ = stream_of(rng, np.concatenate([rng.integers(0, 20, 250), [70000]]))
    return a, b


def wire_text_messages():
    """valid and invalid TEXT messages, whole and fragmented (cuts inside multi-byte characters),
    with BINARY frames of arbitrary bytes between them"""
    rng = np.random.default_rng(307)
    good = "héllo wörld ✓ 𝄞 ".encode()
    bad = [b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"abc\xff", b"\xe2\x9c", b"\x80"]
    frames, payloads = [], []
    for i in range(240):
        body = good * int(rng.integers(1, 9))
        if i % 3 == 1:
            at = int(rng.integers(0, len(body)))
            body = body[:at] + bad[i % len(bad)] + body[at:]
        if i % 5 == 4:
            frames.append((BIN | FIN, 0))
            payloads.append(bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)))
        cuts = sorted(rng.integers(0, len(body) + 1, int(rng.integers(0, 4))).tolist())
        parts = [body[a:b] for a, b in zip([0] + cuts, cuts + [len(body)])]
        for j, part in enumerate(parts):
            frames.append(((TEXT if j == 0 else CONT) | (FIN if j == len(parts) - 1 else 0), 0))
            payloads.append(part)
    b0 = np.array([f[0] for f in frames], dtype=np.uint8)
    off = np.zeros(len(frames) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in payloads])
    payload = np.frombuffer(b"".join(payloads), dtype=np.uint8)
    keys = rng.integers(0, 2**32, b0.size, dtype=np.uint64).astype(np.uint32)
    wire, _ = orc.encode_batch(payload, off, keys, b0, True)
    return wire, (payload, off, keys, b0)


@functools.lru_cache(maxsize=None)
def case(name):
    """(wire, strict, the batch that went into oracle_encode_batch or None, Expected) of a named
    wire, built once and shared by the tests (callers must not modify the arrays)"""
    strict, batch = True, None
    if name == "alignment":
        wire = wire_alignment()[0]
    elif name == "dense":
        wire = wire_dense()[0]
    elif name.startswith("zero_"):
        wire, batch = wire_zero_runs(name[5:])
    elif name.startswith("frag_"):
        wire, batch = wire_fragmented(name[5:])
        strict = name != "frag_loose"
    elif name in ("mixed", "mixed_strict"):
        wire = wire_mixed_masked()[0]
        strict = name == "mixed_strict"
    elif name == "error":
        wire = wire_strict_error()[0]
    elif name == "caps":
        wire, batch = wire_caps()
    elif name == "text":
        wire, batch = wire_text_messages()
    else:
        raise KeyError(name)
    return wire, strict, batch, Expected(wire, strict=strict)


WHOLE_WIRES = ["alignment", "dense", "zero_whole", "zero_start", "zero_end", "frag_strict", "frag_open", "frag_nofin",
               "frag_loose", "mixed", "mixed_strict", "error", "caps", "text"]


def check_round_trip(exp, batch):
    """the expectation (and so the decode held to it) returns the very batch that was encoded"""
    payload, off, keys, b0 = batch
    assert exp.n == keys.size and np.array_equal(exp.payload, payload) and np.array_equal(exp.off, off)
    assert np.array_equal(exp.scan[1], keys) and np.array_equal(exp.scan[2], b0)


class DecodeOutputs:
    """netc_gpu_decode_frames' table outputs for `cap` frames carved out of sentinel-filled device
    tensors, as scanutil.ScanOutputs: `check` proves the used entries equal the expectation and
    that nothing outside offsets[0, n], msg_first[0, M], msg_opcode[0, M), dresult[0, 3) was written."""

    def __init__(self, torch, cap, messages=True):
        self.cap, self.messages = cap, messages
        kn = max(cap, 1)
        self.off_buf = torch.full((cap + 1 + 2 * PAD,), OFF_SENTINEL, dtype=torch.int64, device="cuda")
        self.first_buf = torch.full((cap + 1 + 2 * PAD,), OFF_SENTINEL, dtype=torch.int64, device="cuda")
        self.op_buf = torch.full((kn + 2 * PAD,), OP_SENTINEL, dtype=torch.uint8, device="cuda")
        self.res_buf = torch.full((3 + 2 * PAD,), OFF_SENTINEL, dtype=torch.int64, device="cuda")
        self.off = self.off_buf[PAD: PAD + cap + 1]
        self.first = self.first_buf[PAD: PAD + cap + 1] if messages else None
        self.op = self.op_buf[PAD: PAD + kn] if messages else None
        self.res = self.res_buf[PAD: PAD + 3]

    def reset(self):
        self.off_buf.fill_(OFF_SENTINEL)
        self.first_buf.fill_(OFF_SENTINEL)
        self.op_buf.fill_(OP_SENTINEL)
        self.res_buf.fill_(OFF_SENTINEL)

    def check(self, exp):
        m = exp.m if self.messages else -1
        want_first = exp.first.view(np.int64) if self.messages else np.zeros(0, np.int64)
        want_op = exp.opcode if self.messages else np.zeros(0, np.uint8)
        for name, buf, want, sentinel in (("offsets", self.off_buf, exp.off.view(np.int64), OFF_SENTINEL),
                                          ("msg_first", self.first_buf, want_first, OFF_SENTINEL),
                                          ("msg_opcode", self.op_buf, want_op, OP_SENTINEL),
                                          ("dresult", self.res_buf, exp.dresult.view(np.int64), OFF_SENTINEL)):
            whole = buf.cpu().numpy()
            full = np.full(whole.size, sentinel, dtype=whole.dtype)
            full[PAD: PAD + want.size] = want
            bad = np.nonzero(whole != full)[0]
            assert bad.size == 0, (f"{name}: {bad.size} entries wrong or written outside the used range "
                                   f"(n={exp.n}, M={m}), first at {(bad[:8] - PAD).tolist()}: "
                                   f"got {whole[bad[:8]].tolist()}, want {full[bad[:8]].tolist()}")


__all__ = ["Expected", "DecodeOutputs", "case", "check_round_trip", "WHOLE_WIRES", "SENTINEL"]
