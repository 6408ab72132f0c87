"""GPU parity: netc_gpu_unmask_validate (fused unmask + UTF-8 check of TEXT messages) vs the oracle.

Checkers: oracle_mask_batch (the reference's unmask expression, src/ws/common.c:321)
for the bytes, oracle_validate_batch (RFC 3629 decoder pinned by
tests/test_utf8_oracle.py) for the per-frame verdicts.  The bar: identical bytes,
identical verdicts.
"""

import functools

import numpy as np
import pytest

from netc_amd import mask as nm
from oracle import oracle as orc
from tests.utf8util import MESSAGE_STRUCTURE, batch_arrays, structure_counts, sweep_frames

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def text_bytes(rng, n):
    """~n bytes of UTF-8 text: mostly ASCII, code points near every encoding boundary."""
    pool = [0x7F, 0x80, 0xE9, 0x7FF, 0x800, 0x20AC, 0xD7FF, 0xE000, 0xFFFD, 0xFFFF, 0x10000, 0x1F600, 0x10FFFF]
    out = bytearray()
    while len(out) < n:
        c = int(rng.choice(pool)) if rng.random() < 0.15 else int(rng.integers(0x20, 0x7F))
        out += chr(c).encode("utf-8")
    return bytes(out)


def corrupt(rng, b: bytes) -> bytes:
    b = bytearray(b)
    kind = rng.integers(0, 5)
    if not b:
        return bytes([0xC3])
    i = int(rng.integers(0, len(b)))
    if kind == 0:
        b[i] = 0xFF
    elif kind == 1:
        b.insert(i, 0x80)                    # stray continuation
    elif kind == 2:
        b[i:i] = b"\xed\xa0\x80"             # surrogate
    elif kind == 3:
        b[i:i] = b"\xe0\x80\xaf"             # overlong
    else:
        b += b"\xf0\x9f\x98"                 # truncated at the end
    return bytes(b)


def build_batch(rng, n_msgs, max_len, bad_frac=0.3, control_frac=0.1, binary_frac=0.1):
    """Frames (header byte, payload) of whole messages, fragments split at random byte offsets."""
    frames = []
    for _ in range(n_msgs):
        r = rng.random()
        if r < binary_frac:
            body = rng.integers(0, 256, int(rng.integers(0, max_len)), dtype=np.uint8).tobytes()
            op = 2
        else:
            body = text_bytes(rng, int(rng.integers(0, max_len)))
            if rng.random() < bad_frac:
                body = corrupt(rng, body)
            op = 1
        parts = int(rng.integers(1, 5))
        cuts = sorted(int(x) for x in rng.integers(0, len(body) + 1, parts - 1))
        pieces = [body[a:b] for a, b in zip([0] + cuts, cuts + [len(body)])]
        for i, piece in enumerate(pieces):
            frames.append(((0x80 if i == len(pieces) - 1 else 0) | (op if i == 0 else 0), piece))
            if rng.random() < control_frac:
                frames.append((0x89, rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8).tobytes()))
    return frames


# where dst lies: in place; out of place 3 bytes off src's alignment (the SRC_ALIGNED = false
# kernels); out of place 16 bytes on, co-aligned with src (SRC_ALIGNED = true: with one-step
# windows each window checks its own first bytes from src -- seam_raw<true> -- ADVICE r3)
PLACES = {"inplace": None, "oop_misaligned": 3, "oop_coaligned": 16}


class Batch:
    """A frame batch on the host: payload, offsets, header bytes, keys, the masked (wire)
    payload and the oracle's verdicts -- computed once, reused (unchanged) by every run of it."""

    def __init__(self, payload, off, h0):
        self.payload = np.ascontiguousarray(payload, dtype=np.uint8)
        self.off = np.ascontiguousarray(off, dtype=np.uint64)
        self.h0 = np.ascontiguousarray(h0, dtype=np.uint8)
        n = self.n = self.h0.size
        assert self.off.size == n + 1 and int(self.off[-1]) == self.payload.size
        self.keys = np.random.default_rng(n).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        self.masked = orc.mask_batch(self.payload, self.off, self.keys)   # the wire payload (masking is an involution)
        self.exp = orc.validate_batch(self.payload, self.off, self.h0)


def run_batch(torch, b: Batch, shift=0, inplace=True, dshift=3):
    """unmask_validate of the batch with src at buf[GUARD + shift:] and dst in place or at
    dbuf[GUARD + shift + dshift:]; every buffer sentinel-filled, `valid` a slice of a larger
    tensor: identical bytes, identical verdicts, guards intact, src unchanged out of place."""
    n, total = b.n, b.masked.size
    buf = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    lo, hi = GUARD + shift, GUARD + shift + total
    src = buf[lo:hi]
    src.copy_(torch.from_numpy(b.masked))
    if inplace:
        dbuf, dst, dlo, dhi = buf, src, lo, hi
    else:
        dbuf = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        dlo, dhi = lo + dshift, hi + dshift
        dst = dbuf[dlo:dhi]
    vbuf = torch.full((n + 2 * GUARD,), 7, dtype=torch.uint8, device="cuda")
    valid = vbuf[GUARD: GUARD + n]
    nm.unmask_validate(dst, src, _dev(torch, b.off), _dev(torch, b.keys), torch.from_numpy(b.h0).cuda(), valid)
    torch.cuda.current_stream().synchronize()
    whole = dbuf.cpu().numpy()
    assert np.array_equal(whole[dlo:dhi], b.payload), "unmasked bytes differ"
    assert (whole[:dlo] == SENTINEL).all() and (whole[dhi:] == SENTINEL).all(), "write outside the destination"
    if not inplace:
        swhole = buf.cpu().numpy()
        assert np.array_equal(swhole[lo:hi], b.masked), "the source changed"
        assert (swhole[:lo] == SENTINEL).all() and (swhole[hi:] == SENTINEL).all(), "write around the source"
    vwhole = vbuf.cpu().numpy()
    got = vwhole[GUARD: GUARD + n]
    bad = np.nonzero(got != b.exp)[0]
    assert bad.size == 0, (f"verdicts differ at frames {bad[:8].tolist()} of {n} (got {got[bad[:8]].tolist()}; "
                           f"{bad.size} in all)")
    assert (vwhole[:GUARD] == 7).all() and (vwhole[GUARD + n:] == 7).all(), "write outside the verdicts"
    return b.exp


def run_validate(torch, frames, shift=0, inplace=True, dshift=3):
    return run_batch(torch, Batch(*batch_arrays(frames)), shift, inplace, dshift)


@pytest.mark.parametrize("steps", [None, 1, 2, 4])
@pytest.mark.parametrize("seed", range(4))
def test_mixed_messages(torch_cuda, gpu_knob, seed, steps):
    gpu_knob("VAL_STEPS", steps)   # the 4 KiB window as 1, 2 or 4 steps (None: by batch size)
    rng = np.random.default_rng(seed)
    exp = run_validate(torch_cuda, build_batch(rng, 300, 3000))
    assert 0 < (exp == 0).sum()   # some messages are invalid


@pytest.mark.parametrize("shift", [1, 7, 13])
def test_alignments_and_out_of_place(torch_cuda, shift):
    rng = np.random.default_rng(40 + shift)
    run_validate(torch_cuda, build_batch(rng, 200, 2000), shift=shift)
    run_validate(torch_cuda, build_batch(rng, 200, 2000), shift=shift, inplace=False)


def test_tiny_fragments(torch_cuda):
    # fragments of 0-3 bytes: every code point split across frames
    rng = np.random.default_rng(50)
    frames = []
    for _ in range(200):
        body = text_bytes(rng, int(rng.integers(0, 40)))
        if rng.random() < 0.3:
            body = corrupt(rng, body)
        pieces, i = [], 0
        while i < len(body):
            k = int(rng.integers(0, 4))
            pieces.append(body[i:i + k])
            i += k
        pieces = pieces or [b""]
        for j, p in enumerate(pieces):
            frames.append(((0x80 if j == len(pieces) - 1 else 0) | (1 if j == 0 else 0), p))
    run_validate(torch_cuda, frames)


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("steps", [None, 1, 2, 4])
def test_errors_at_every_boundary(torch_cuda, gpu_knob, steps, place):
    # one long valid TEXT frame per case with an error at a vector / span / chunk edge
    gpu_knob("VAL_STEPS", steps)
    rng = np.random.default_rng(60)
    base = text_bytes(rng, 20000)
    base = base[: base.rfind(b" ") if b" " in base else len(base)]
    frames = []
    for pos in (0, 1, 2, 3, 15, 16, 17, 1023, 1024, 1025, 4093, 4094, 4095, 4096, 4097, 8191, 8192):
        for bad in (b"\x80", b"\xff", b"\xc3\x28", b"\xed\xa0\x80", b"\xe0\x80\xaf"):
            cut = base[:pos]
            while cut and (cut[-1] & 0xC0) == 0x80:   # keep the prefix itself valid
                cut = cut[:-1]
            if cut and cut[-1] >= 0xC0:
                cut = cut[:-1]
            frames.append((0x81, cut + bad + b"tail"))
    frames.append((0x81, base))   # and a valid one
    exp = run_validate(torch_cuda, frames, inplace=PLACES[place] is None, dshift=PLACES[place] or 0)
    assert (exp[:-1] == 0).all() and exp[-1] == 1


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("steps", [None, 1, 2, 4])
@pytest.mark.parametrize("shift", [0, 5])
def test_errors_at_chunk_seams(torch_cuda, gpu_knob, shift, steps, place):
    gpu_knob("VAL_STEPS", steps)
    frames = chunk_seam_frames(shift)
    run_validate(torch_cuda, frames, shift=shift, inplace=PLACES[place] is None, dshift=PLACES[place] or 0)


def chunk_seam_frames(shift):
    # long frames (many 4 KiB chunks each) with one broken byte among the first 3 bytes
    # of a chunk -- the bytes phase B checks in place; out of place each window checks its
    # own first bytes (the 4 before it unmasked from src) -- or just before / after them
    rng = np.random.default_rng(70 + shift)
    flen, win, mis = 70000, 4096, shift & 15   # torch allocations are 256-B aligned
    frames, o = [], 0
    for i in range(30):
        body = bytearray(text_bytes(rng, flen)[:flen]) if i % 3 else bytearray(rng.integers(0x20, 0x7F, flen, dtype=np.uint8).tobytes())
        if i % 6 != 5:
            c = ((o + mis + 3 + win - 1) // win + int(rng.integers(0, 12))) * win   # a chunk start inside the frame
            p = c - mis - o + (-1, 0, 1, 2, 3)[i % 5]
            if 3 <= p < flen:
                body[p] = (0xFF, 0x80, 0xC0)[i % 3]
        frames.append((0x81, bytes(body)))
        o += flen
    return frames


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("steps", [2, 4])
@pytest.mark.parametrize("shift", [0, 7])
def test_errors_at_step_starts_of_the_last_window(torch_cuda, gpu_knob, steps, shift, inplace):
    # a window of several steps that holds a partial vector (the batch's last) runs its steps
    # one by one; the first 3 bytes of each later step are checked with the carry from the
    # step before (they are no 4 KiB seam that phase B would check)
    gpu_knob("VAL_STEPS", steps)
    rng = np.random.default_rng(90 + steps + shift)
    win, mis = 4096, shift & 15
    total = 5 * win + 3000 - mis                     # the last window is partial
    last = (mis + total) // win * win                # its first byte (P coordinates)
    step = win // steps
    for k in range(1, steps):
        for d in range(3):
            # an overlong 2-byte sequence C0 80 whose second byte is byte d of the step: the
            # rule flags that byte and no other (ASCII around it)
            q = last + k * step + d - mis            # payload offset of the flagged byte
            if q + 6 >= total:
                continue
            body = bytearray(b"a" * 1000) + bytearray(text_bytes(rng, total)[:total - 1000])
            body[q - 5:q + 6] = b"a" * 11
            body[-4:] = b"tail"                      # no code point cut at the end
            body[q - 1], body[q] = 0xC0, 0x80
            frames = [(0x81, bytes(body[:1000])), (0x81, bytes(body[1000:]))]
            exp = run_validate(torch_cuda, frames, shift=shift, inplace=inplace)
            assert exp.tolist() == [1, 0]


def test_large_text_batch(torch_cuda):
    # ~64 MiB of 1 KiB TEXT frames (config 2 shape), 1 % corrupted
    rng = np.random.default_rng(70)
    chunk = text_bytes(rng, 1 << 20)
    frames = []
    pos = 0
    for i in range(65536):
        p = chunk[pos: pos + 1024]
        pos = (pos + 1024) % (len(chunk) - 1024)
        if i % 100 == 7:
            p = corrupt(rng, p)
        frames.append((0x81, p))
    exp = run_validate(torch_cuda, frames)
    assert (exp == 0).sum() > 300


def edge_text(rng, n, bad):
    """n bytes of text whose first and last 3 bytes are multi-byte sequences (or, bad: a stray
    continuation first / a truncated sequence last)"""
    if n < 8:
        return corrupt(rng, text_bytes(rng, n)) if bad else text_bytes(rng, n)
    head, tail = "\u20ac".encode(), "\U0001F600".encode()
    mid = bytearray(text_bytes(rng, max(0, n - 7)))
    body = head + bytes(mid) + tail
    if bad:
        body = (b"\x80" + body[1:]) if rng.random() < 0.5 else body[:-1]
    return body


@pytest.mark.parametrize("steps", [None, 1, 2, 4])
@pytest.mark.parametrize("place", sorted(PLACES))
def test_message_edges(torch_cuda, gpu_knob, steps, place):
    """single-frame TEXT messages starting and ending at every offset around span (1 KiB) and
    window (4 KiB) edges, with multi-byte first and last bytes, half of them broken at the start
    or end (the bytes the per-message launch checks), short ones among them"""
    gpu_knob("VAL_STEPS", steps)
    frames = message_edge_frames()
    shift = PLACES[place]
    exp = run_validate(torch_cuda, frames, shift=0 if shift is None else 0, inplace=shift is None,
                       dshift=shift or 3)
    assert 100 < (exp == 0).sum() < len(frames)


def message_edge_frames():
    rng = np.random.default_rng(171)
    frames = []
    for _ in range(600):
        r = rng.random()
        n = int(rng.integers(0, 12)) if r < 0.2 else (int(rng.integers(1015, 1034)) if r < 0.7 else int(rng.integers(30, 3000)))
        bad = rng.random() < 0.5
        frames.append((0x81, edge_text(rng, n, bad)))
        if rng.random() < 0.05:
            frames.append((0x82, rng.integers(0, 256, int(rng.integers(0, 50)), dtype=np.uint8).tobytes()))
    return frames


# ------------------------------------------------------- the rule, swept ----

@functools.lru_cache(maxsize=None)
def sweep_batch(layout, lead):
    """every sequence of tests/utf8util.sweep_sequences as one single-frame TEXT message
    ("bare": 4-byte frames, phase B's utf8_rule sees bytes 0-2 and the end-of-message rule;
    "padded": b"abcd" + seq + b"wxyz", phase A's utf8_err_word sees the whole sequence) after
    a BINARY frame of `lead` bytes, which moves every sequence to another residue mod 16"""
    fr = sweep_frames(layout)
    n, w = fr.shape
    payload = np.concatenate([np.full(lead, 0xFF, dtype=np.uint8), fr.reshape(-1)])
    off = np.zeros(n + 2, dtype=np.uint64)
    off[1:] = lead + w * np.arange(n + 1, dtype=np.uint64)
    h0 = np.full(n + 1, 0x81, dtype=np.uint8)
    h0[0] = 0x82
    return Batch(payload, off, h0)


@pytest.mark.parametrize("steps", [None, 1])
@pytest.mark.parametrize("place", ["inplace", "oop_coaligned"])
def test_every_sequence_prefix(torch_cuda, gpu_knob, place, steps):
    """both copies of the rule against the oracle (pinned on this very set by
    tests/test_utf8_oracle.py) on all 1,048,576 sequences (b0, b1, b2, b3) with (b0, b1) any
    and (b2, b3) from {24, 80, BF, C3}, at every residue mod 16 and across span and window edges"""
    gpu_knob("VAL_STEPS", steps)
    for layout in ("bare", "padded"):
        for lead in range(4):
            b = sweep_batch(layout, lead)
            assert b.n == (1 << 20) + 1 and 0 < int((b.exp == 0).sum()) < b.n - 1
            run_batch(torch_cuda, b, inplace=PLACES[place] is None, dshift=PLACES[place] or 0)


# ------------------------------------------------------ message structure ----

def test_message_structure_known_answers(torch_cuda):
    """hand-written batches with hand-written verdicts (tests/utf8util.MESSAGE_STRUCTURE):
    orphan continuations, abandoned and unfinished messages, reserved opcodes, RSV bits, empty
    continuation frames, control frames inside a message -- the kernel and the oracle both"""
    wrong = []
    for frames, expect in MESSAGE_STRUCTURE:
        b = Batch(*batch_arrays(frames))
        assert b.exp.tolist() == expect, frames
        for inplace in (True, False):
            try:
                run_batch(torch_cuda, b, inplace=inplace)
            except AssertionError as e:
                wrong.append(f"{[(hex(h), p) for h, p in frames]} inplace={inplace}: {e}")
    assert not wrong, f"{len(wrong)} runs differ:\n" + "\n".join(wrong)


DIRTY_POOL = np.array([0x01, 0x81, 0x00, 0x80, 0x02, 0x82, 0x89, 0x8A, 0x03, 0x83, 0xC1], dtype=np.uint8)


def dirty_frames(seed, n=3000):
    """header bytes drawn freely (no message discipline), payloads of 0-40 B, half of them broken"""
    rng = np.random.default_rng(300 + seed)
    frames = []
    for h in rng.choice(DIRTY_POOL, n).tolist():
        body = text_bytes(rng, int(rng.integers(0, 35)))
        frames.append((h, corrupt(rng, body) if rng.random() < 0.5 else body))
    return frames


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("seed", range(4))
def test_dirty_message_streams(torch_cuda, seed, inplace):
    b = Batch(*batch_arrays(dirty_frames(seed)))
    c = structure_counts(b.h0)
    assert c["orphans"] >= 50 and c["abandoned"] >= 50, c
    assert 50 < int((b.exp == 0).sum()) and 50 < int((b.exp[(b.h0 & 0x8F) == 0x80] == 1).sum())
    run_batch(torch_cuda, b, shift=seed, inplace=inplace)


def test_long_walks(torch_cuda):
    # phase B walks back from a FIN continuation frame and forward again: 5,000 control frames
    # between two fragments (valid and not), and messages of 3,000 continuation frames
    euro = "€".encode()
    pings = [(0x89, b"\xff\x80")] * 5000
    text = ("€éa" * 1000).encode()
    pieces = [text[i:i + 2] for i in range(0, len(text), 2)]
    assert len(pieces) == 3000
    chain = [(0x01, pieces[0])] + [(0x00, p) for p in pieces[1:-1]] + [(0x80, pieces[-1])]
    broken = list(chain)
    broken[1500] = (0x00, b"\xa9\xa9")
    frames = ([(0x01, euro[:2])] + pings + [(0x80, euro[2:])] + [(0x01, euro[:2])] + pings + [(0x80, b"!")]
              + chain + broken + [(0x80, b"\xff")])
    exp = run_validate(torch_cuda, frames)
    assert (exp == 0).sum() == 2 and exp[2 * 5002 - 1] == 0 and exp[-2] == 0
    run_validate(torch_cuda, frames, shift=5, inplace=False)


# ------------------------------------------------ zero frames, zero bytes ----

def test_no_frames_out_of_place_is_a_copy(torch_cuda):
    # nframes == 0: the bytes are unframed and pass through, as with netc_gpu_mask_batch
    # (tests/test_gpu_parity.py::test_no_frames_is_a_copy)
    torch = torch_cuda
    total = 100003
    payload = np.random.default_rng(400).integers(0, 256, total, dtype=np.uint8)
    sbuf = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    dbuf = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    src, dst = sbuf[GUARD + 1: GUARD + 1 + total], dbuf[GUARD + 4: GUARD + 4 + total]
    src.copy_(torch.from_numpy(payload))
    empty8 = torch.zeros(0, dtype=torch.uint8, device="cuda")
    nm.unmask_validate(dst, src, torch.zeros(1, dtype=torch.int64, device="cuda"),
                       torch.zeros(0, dtype=torch.int32, device="cuda"), empty8, empty8)
    torch.cuda.synchronize()
    whole = dbuf.cpu().numpy()
    assert np.array_equal(whole[GUARD + 4: GUARD + 4 + total], payload), "dst is not a copy of src"
    assert (whole[:GUARD + 4] == SENTINEL).all() and (whole[GUARD + 4 + total:] == SENTINEL).all()
    swhole = sbuf.cpu().numpy()
    assert np.array_equal(swhole[GUARD + 1: GUARD + 1 + total], payload)
    assert (swhole[:GUARD + 1] == SENTINEL).all() and (swhole[GUARD + 1 + total:] == SENTINEL).all()
    nm.unmask_validate(src, src, torch.zeros(1, dtype=torch.int64, device="cuda"),
                       torch.zeros(0, dtype=torch.int32, device="cuda"), empty8, empty8)   # in place: nothing to do
    torch.cuda.synchronize()
    assert np.array_equal(sbuf.cpu().numpy(), swhole)


def test_empty_frames_only(torch_cuda):
    # total == 0: 50 empty frames of mixed opcodes; an empty TEXT message is valid
    rng = np.random.default_rng(401)
    frames = [(int(h), b"") for h in rng.choice(DIRTY_POOL, 50)]
    exp = run_validate(torch_cuda, frames)
    assert (exp == 1).all()
    run_validate(torch_cuda, frames, inplace=False)


# -------------------------------------------------- the persistent walk ----

@functools.lru_cache(maxsize=None)
def persistent_walk_batches():
    # test_mixed_messages' batch (seed 0), test_errors_at_chunk_seams' (shift 5), test_message_edges'
    return [Batch(*batch_arrays(f)) for f in (build_batch(np.random.default_rng(0), 300, 3000),
                                              chunk_seam_frames(5), message_edge_frames())]


@pytest.mark.parametrize("max_blocks", [0, 1, 3])
@pytest.mark.parametrize("flags", [4, 7])
def test_persistent_walk(torch_cuda, flags, max_blocks):
    """NETC_GPU_TUNE_PERSISTENT (alone, and with non-temporal loads and stores): the VAL
    instantiation of the grid-stride kernel, mask_frames_kernel<4, AL, true, true>"""
    nm.tune(4, max_blocks, flags)
    try:
        for i, b in enumerate(persistent_walk_batches()):
            assert 0 < int((b.exp == 0).sum())
            for place in sorted(PLACES):
                run_batch(torch_cuda, b, shift=5 if i == 1 else 0, inplace=PLACES[place] is None,
                          dshift=PLACES[place] or 0)
    finally:
        nm.tune()


# ---------------------------------------- dense frames over many windows ----

def fast_text(rng, nchars) -> str:
    """text_bytes' mix of code points, drawn with numpy"""
    pool = np.array([0x7F, 0x80, 0xE9, 0x7FF, 0x800, 0x20AC, 0xD7FF, 0xE000, 0xFFFD, 0xFFFF, 0x10000, 0x1F600,
                     0x10FFFF])
    cps = np.where(rng.random(nchars) < 0.15, rng.choice(pool, nchars), rng.integers(0x20, 0x7F, nchars))
    return "".join(map(chr, cps.tolist()))


@functools.lru_cache(maxsize=None)
def dense_batch():
    """~200,000 TEXT fragments of 0-24 B (tests/test_tiny_fragments' rule: every code point may be
    split), 30 % of the messages broken; then a stretch of 20-300 B fragments (3-63 frame starts
    per 1 KiB span) and a few frames of several KiB"""
    rng = np.random.default_rng(500)
    frames = []

    def message(body, lo, hi):
        if rng.random() < 0.3:
            body = corrupt(rng, body)
        cuts = np.cumsum(rng.integers(lo, hi, len(body) // max(1, lo) + 2)).tolist()
        pieces, i = [], 0
        for c in cuts:
            if i >= len(body):
                break
            pieces.append(body[i:c])
            i = c
        pieces = pieces or [b""]
        for j, p in enumerate(pieces):
            frames.append(((0x80 if j == len(pieces) - 1 else 0) | (1 if j == 0 else 0), p))

    text = fast_text(rng, 3_000_000)
    pos = 0
    while len(frames) < 200_000:
        k = int(rng.integers(0, 300))
        message(text[pos:pos + k].encode(), 0, 25)
        pos += k
    for _ in range(300):
        k = int(rng.integers(100, 2000))
        message(text[pos:pos + k].encode(), 20, 301)
        pos += k
    for _ in range(6):
        k = int(rng.integers(3000, 9000))
        message(text[pos:pos + k].encode(), 20000, 20001)
        pos += k
    assert pos < len(text)
    return Batch(*batch_arrays(frames))


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("shift", [0, 7])
def test_dense_fragments_many_windows(torch_cuda, shift, inplace):
    b = dense_batch()
    assert b.n > 200_000 and 2 << 20 < b.payload.size < 4 << 20
    per = np.bincount((b.off[:-1].astype(np.int64) + shift) // 1024)   # frame starts per 1 KiB span
    assert (per >= 64).sum() > 500 and ((per >= 3) & (per <= 63)).sum() > 200 and (per <= 2).sum() > 10
    assert 1000 < int((b.exp == 0).sum())
    run_batch(torch_cuda, b, shift=shift, inplace=inplace)


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("steps", [None, 1])
@pytest.mark.parametrize("shift", [0, 7])
def test_errors_behind_a_frame_start_at_a_window_seam(torch_cuda, gpu_knob, shift, steps, place):
    """TEXT frames that start 0-4 bytes before a 4 KiB window start, with one stray continuation
    byte at frame offset 0-6 (or none): phase A leaves a window's first 3 bytes and a frame's
    first 3 bytes to phase B, which must cover every byte of both sets -- a window starting 1 or
    2 bytes into a frame leaves it frame bytes 3 and 4 (found by
    test_dense_fragments_many_windows: E0 80 AF with E0 the first byte of a window, 2 bytes
    into its frame, went unseen).  Single frames and second fragments."""
    gpu_knob("VAL_STEPS", steps)
    dshift = PLACES[place] or 0
    mis = (GUARD + shift + dshift) & 15            # windows are counted from dst's 16-byte line
    frames, o, w, bad = [], 0, 1, 0
    for fragment in (False, True):
        for delta in range(5):
            for epos in (None, 0, 1, 2, 3, 4, 5, 6):
                lo = w * 4096 - mis - delta        # the frame's first byte: delta bytes before window w
                w += 1
                head = [(0x01, b"\xc3\xa9 first fragment, ")] if fragment else []
                fill = lo - o - sum(len(p) for _, p in head)
                body = bytearray(b"0123456789 the rest of the frame is plain")
                if epos is not None:
                    body[epos] = 0x80
                    bad += 1
                frames += [(0x82, bytes(fill))] + head + [(0x80 if fragment else 0x81, bytes(body))]
                o = lo + len(body)
    exp = run_validate(torch_cuda, frames, shift=shift, inplace=PLACES[place] is None, dshift=dshift)
    assert (exp == 0).sum() == bad == 70


# ------------------------------------------------------ scratch tag epoch ----

def test_flag_scratch_epochs(torch_cuda):
    """the per-stream flag scratch is tagged with an 8-bit epoch (cleared when it wraps after 255
    calls) and reallocated when a batch outgrows its 65,536 entries: 600 calls on one stream
    alternating two batches of one shape whose verdicts are each other's complement, one batch
    of 70,000 frames in the middle; a flag surviving the wrap or the regrowth flips a verdict"""
    torch = torch_cuda
    good, bad = b"valid text \xe2\x82\xac of forty bytes, all fine!", b"valid text \xe2\x82\xac of forty by\xfftes, not fine"
    assert len(good) == len(bad) == 40
    pair = [Batch(*batch_arrays([(0x81, bad if (k + which) % 2 else good) for k in range(128)])) for which in (0, 1)]
    assert np.array_equal(pair[0].exp, 1 - pair[1].exp) and pair[0].exp.sum() == 64
    big = Batch(*batch_arrays([(0x81, b"\xff" if k % 3 == 0 else b"ab") for k in range(70000)]))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        try:
            dev = [(torch.from_numpy(b.masked).cuda(), _dev(torch, b.off), _dev(torch, b.keys),
                    torch.from_numpy(b.h0).cuda()) for b in pair]
            dst = torch.empty_like(dev[0][0])
            valid = torch.empty(128, dtype=torch.uint8, device="cuda")
            for call in range(600):
                if call == 300:
                    run_batch(torch, big)
                b, (src, off, keys, h0) = pair[call % 2], dev[call % 2]
                valid.fill_(7)
                nm.unmask_validate(dst, src, off, keys, h0, valid)
                got = valid.cpu().numpy()
                assert np.array_equal(got, b.exp), f"call {call}: verdicts differ at {np.nonzero(got != b.exp)[0][:8]}"
            assert np.array_equal(dst.cpu().numpy(), pair[1].payload)
        finally:
            nm.stream_release(s)
