"""The two helpers the rings and hubs share and that had no direct test (CPU only).

* netc_amd/csrc/host/ws_header.h -- the header decode and the strict predicate that the host walk
  (ws_scan_cpu.c), the host decode and the receive hub read headers with -- through a C shim
  (tests/drivers/ws_header_shim.c), against the oracle's scan and tests/scanutil.py's model.
* the message assembler of netc_amd/csrc/ws_ring_host.h, through its two users in the mock
  library (tests/mockhip): the ingest ring (write + next_message) and a receive hub over a
  socketpair are fed the same frames and must deliver the same messages and the same error.
"""

import ctypes
import os
import select

import numpy as np
import pytest

from netc_amd import _lib
from netc_amd import hub as nh
from netc_amd import ingest as ni
from oracle import oracle as orc
from tests.scanutil import frame_fields
from tests.wsutil import Endpoint, ParseState, libc, pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "bin", "libws_header_shim.so")
MOCK = os.path.join(ROOT, "tests", "bin", "libnetc_ingest_mock.so")

CONT, TEXT, BINARY, PING = 0, 1, 2, 9
TOO_BIG = ni.WS_FRAME_PARSE_ERROR_PAYLOAD_TOO_BIG


# ------------------------------------------------------------------------ ws_header.h --

@pytest.fixture(scope="module")
def shim():
    assert os.path.exists(SHIM), "tests/bin/libws_header_shim.so missing: run make"
    lib = ctypes.CDLL(SHIM)
    u8p, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint64
    lib.shim_header_decode.argtypes = [u8p, u64, ctypes.POINTER(u64)]
    lib.shim_header_forbidden.argtypes = [u8p, u64]
    lib.shim_header_len.argtypes = [u64, ctypes.c_int]
    lib.shim_header_len.restype = u64
    lib.shim_header_len_of.argtypes = [ctypes.c_uint8]
    lib.shim_header_len_of.restype = u64
    return lib


# (7-bit code, extended-length value): the length codes with the extended lengths at their
# boundaries -- 125 / 126, 65535 / 65536, the 64-bit top bit -- non-minimal encodings included
LENGTHS = [(0, None), (125, None), (126, 0), (126, 125), (126, 126), (126, 65535), (127, 65535), (127, 65536),
           (127, (1 << 63) - 1), (127, 1 << 63), (127, (1 << 64) - 1)]
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])


def header_bytes(first, masked, code, extval):
    ext = b"" if extval is None else extval.to_bytes(2 if code == 126 else 8, "big")
    return bytes([first, (0x80 if masked else 0) | code]) + ext + (KEY if masked else b"")


def test_header_decode_and_strict_predicate(shim):
    """every first byte x {MASK set, clear} x the length cases, each header truncated at every
    length from 0 to its full size: the decode against scanutil.frame_fields (the lengths are
    known once byte 1 and the extended length are there, the key once the header is whole), the
    predicate against the oracle's strict scan of the same bytes (error at offset 0 or not)"""
    o = orc.lib()
    out5 = (ctypes.c_uint64 * 5)()
    hdr, keys, b0 = (ctypes.c_uint64 * 1)(), (ctypes.c_uint32 * 1)(), (ctypes.c_uint8 * 1)()
    consumed, error = ctypes.c_uint64(0), ctypes.c_uint64(0)
    checked = 0
    for masked in (False, True):
        for code, extval in LENGTHS:
            for first in range(256):
                h = header_bytes(first, masked, code, extval)
                hl, ln, m = frame_fields(np.frombuffer(h, dtype=np.uint8), 0)
                assert hl == len(h) and m == masked and ln == (code if extval is None else extval)
                assert shim.shim_header_len_of(h[1]) == hl
                buf = (ctypes.c_uint8 * len(h)).from_buffer_copy(h)
                lengths_at = hl - (4 if masked else 0)   # byte 1 and the extended length
                for avail in range(hl + 1):
                    got = shim.shim_header_decode(buf, avail, out5)
                    assert got == (1 if avail >= lengths_at else 0), (h.hex(), avail)
                    o.oracle_scan_frames(buf, avail, 0, 1, hdr, keys, b0, 1, ctypes.byref(consumed), ctypes.byref(error))
                    rejected = error.value == 0
                    f = shim.shim_header_forbidden(buf, avail)
                    if not got:
                        assert f == -1 and not rejected, (h.hex(), avail)
                        continue
                    key = int.from_bytes(KEY, "little") if masked and avail >= hl else 0
                    assert list(out5) == [hl, ln, key, first, h[1]], (h.hex(), avail)
                    assert f == (1 if rejected else 0), (h.hex(), avail)
                    checked += 1
    assert checked > 256 * 2 * len(LENGTHS)


@pytest.mark.parametrize("masked", [False, True])
def test_header_of_a_complete_frame_and_header_len(shim, masked):
    """frames the oracle encodes at the length-class boundaries: ws_header_len is the oracle's
    header size, and the decode of the oracle's header gives the lengths and key its scan gives"""
    out5 = (ctypes.c_uint64 * 5)()
    for ln in (0, 1, 125, 126, 65535, 65536):
        wire = frames_wire([(0x80 | BINARY, bytes(ln))], masked)
        hl = len(wire) - ln
        assert shim.shim_header_len(ln, 1 if masked else 0) == hl
        buf = (ctypes.c_uint8 * hl).from_buffer_copy(wire[:hl])
        assert shim.shim_header_decode(buf, hl, out5) == 1
        shdr, skeys, sb0, consumed, err = orc.scan_frames(np.frombuffer(wire, dtype=np.uint8), strict=False)
        assert shdr.size == 1 and err is None and consumed == len(wire)
        assert list(out5) == [hl, consumed - hl, int(skeys[0]), int(sb0[0]), wire[1]]


def frames_wire(frames, masked=True):
    """the wire of frames (byte 0, payload), one key each: oracle_encode_batch, which gives a
    masked empty frame its key (RFC 6455 §5.2)"""
    off = np.cumsum([0] + [len(p) for _, p in frames]).astype(np.uint64)
    keys = np.array([0x0B090700 + i + 1 for i in range(len(frames))], dtype=np.uint32)
    wire, _ = orc.encode_batch(np.frombuffer(b"".join(p for _, p in frames), dtype=np.uint8), off,
                               keys if masked else None, np.array([b0 for b0, _ in frames], dtype=np.uint8), masked)
    return wire.tobytes()


# ------------------------------------------------------------------- message reassembly --


def model(frames, limit):
    """the reference's reassembly (src/ws/common.c:163-164, 210-211, 340-346): the last non-zero
    opcode, the payloads joined, a TEXT message's NUL; PAYLOAD_TOO_BIG once a frame would pass
    the limit"""
    msgs, buf, op = [], b"", 0
    for b0, p in frames:
        if b0 & 0x0F:
            op = b0 & 0x0F
        if len(p) + len(buf) > limit:
            return msgs, TOO_BIG
        buf += p
        if b0 & 0x80:
            if op == TEXT:
                buf += b"\0"
            msgs.append((op, buf, len(buf)))
            buf = b""
    return msgs, 1


FIN = 0x80
CASES = {
    "messages": ([(TEXT, b"frag"), (CONT, b"men"), (FIN | CONT, b"ted"),          # a TEXT of three frames
                  (FIN | BINARY, b""), (FIN | TEXT, b""),                          # empty BINARY, empty TEXT
                  (BINARY, b"abc"), (FIN | PING, b"p"), (FIN | CONT, b"def"),      # a control frame between fragments
                  (FIN | BINARY, bytes(range(200)))], 1 << 20),
    "one_byte_over_on_the_second_frame": ([(FIN | TEXT, b"ok"), (BINARY, b"123456"), (FIN | CONT, b"78901"),
                                           (FIN | BINARY, b"never")], 10),
}


def ingest_messages(mock, wire, limit):
    got = []
    with ni.Ingest(slot_bytes=1 << 16, nslots=2, lib=mock) as ing:
        assert ing.write(wire) == len(wire)
        while True:
            rc, op, data = ing.next_message(limit)
            if rc != 0:
                return got, rc
            got.append((op, data, len(data)))


def hub_messages(mock, wire, limit):
    lib = _lib.host()
    a, b = pair()
    b.setblocking(False)
    ep, st, got = Endpoint(b), ParseState(), []
    with nh.Hub(slot_bytes=1 << 17, nslots=2, lib=mock) as hub:
        hub.attach(b.fileno())
        try:
            a.sendall(wire)
            for _ in range(100):
                rc = lib.ws_parse_frame(ctypes.byref(ep.client), ctypes.byref(st), limit)
                if rc == 0:
                    m = st.message
                    got.append((m.opcode, ctypes.string_at(m.buffer, m.payload_length), m.payload_length))
                    libc.free(m.buffer)
                    ctypes.memset(ctypes.byref(st), 0, ctypes.sizeof(st))
                elif rc != 1 or not select.select([b], [], [], 0)[0]:
                    break
        finally:
            hub.detach(b.fileno())
    a.close()
    b.close()
    return got, rc


@pytest.mark.parametrize("case", sorted(CASES))
def test_ring_and_hub_assemble_the_same_messages(case):
    assert os.path.exists(MOCK), "tests/bin/libnetc_ingest_mock.so missing: run make"
    mock = ctypes.CDLL(MOCK)
    frames, limit = CASES[case]
    wire = frames_wire(frames)
    ring = ingest_messages(mock, wire, limit)
    hub = hub_messages(mock, wire, limit)
    assert ring == hub
    assert ring == model(frames, limit)
    if case != "messages":
        assert ring[1] == TOO_BIG and len(ring[0]) == 1
