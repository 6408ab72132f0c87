"""Inputs shared by the UTF-8 oracle tests (CPU) and the GPU verdict tests: the oracle is pinned
on exactly the sets the kernel is then judged by.  Test infrastructure only."""

import numpy as np


def sweep_sequences() -> np.ndarray:
    """(1048576, 4) uint8: every (b0, b1) in 256^2 crossed with (b2, b3) in {24, 80, BF, C3}^2 --
    every lead byte with every second byte (F4 90, F0 8F, E0 9F, ED A0, C0 / C1 xx, F5..FF, a
    lead after a lead, ...), followed by ASCII, the lowest and highest continuation, or a lead."""
    tail = np.array([0x24, 0x80, 0xBF, 0xC3], dtype=np.uint8)
    b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), tail, tail, indexing="ij")
    return np.stack(b, axis=-1).reshape(-1, 4)


def sweep_frames(layout: str) -> np.ndarray:
    """(1048576, 4 or 12) uint8 payloads: "bare" the sequences alone, "padded" each as
    b"abcd" + seq + b"wxyz" """
    seq = sweep_sequences()
    if layout == "bare":
        return seq
    out = np.empty((seq.shape[0], 12), dtype=np.uint8)
    out[:, :4] = np.frombuffer(b"abcd", dtype=np.uint8)
    out[:, 4:8] = seq
    out[:, 8:] = np.frombuffer(b"wxyz", dtype=np.uint8)
    return out


# Message structure, by the text of include/ws/mask.h: verdict 0 only on the FIN frame of a TEXT
# message (opcode 1, then opcode 0 up to the first FIN; control frames apart) whose bytes are
# not UTF-8; 1 everywhere else.  (frames as (header byte 0, payload), expected verdicts), each
# list a batch of its own, the verdicts written by hand.
MESSAGE_STRUCTURE = [
    # a FIN continuation after a finished message belongs to no message: an orphan
    ([(0x81, b"ok"), (0x80, b"\x80")], [1, 1]),
    ([(0x01, b"a"), (0x80, b"b"), (0x80, b"\xff")], [1, 1, 1]),              # after a finished fragmented TEXT
    ([(0x01, b"a\xc3"), (0x80, b"\xa9"), (0x80, b"\xa9")], [1, 1, 1]),
    ([(0x01, b"a"), (0x80, b"\xff"), (0x80, b"b")], [1, 0, 1]),
    ([(0x82, b"\xff"), (0x80, b"\xff")], [1, 1]),                             # after a BINARY
    ([(0x80, b"\xff"), (0x81, b"ok")], [1, 1]),                               # as the batch's first frame
    ([(0x80, b"\xff")], [1]),
    ([(0x81, b"ok"), (0x00, b"\xff"), (0x80, b"\xff")], [1, 1, 1]),           # a non-FIN orphan, then a FIN one
    ([(0x00, b"\xff"), (0x00, b"\xff"), (0x80, b"\xff"), (0x81, b"\xff")], [1, 1, 1, 0]),
    ([(0x81, b"ok"), (0x89, b"\xff"), (0x80, b"\x80")], [1, 1, 1]),           # a control frame before the orphan
    # a TEXT abandoned before its FIN by a new TEXT: only the new message is judged
    ([(0x01, b"\xff"), (0x81, b"ok")], [1, 1]),
    ([(0x01, b"\xff"), (0x01, b"o"), (0x80, b"k")], [1, 1, 1]),
    ([(0x01, b"ok"), (0x81, b"\xff")], [1, 0]),
    ([(0x01, b"ok"), (0x01, b"\xff"), (0x80, b"k")], [1, 1, 0]),
    ([(0x01, b"\xc3"), (0x01, b"\xa9"), (0x80, b"k")], [1, 1, 0]),            # the abandoned bytes are not carried over
    # ... and by a BINARY: its continuation frames are BINARY
    ([(0x01, b"\xff"), (0x02, b"x"), (0x80, b"y")], [1, 1, 1]),
    ([(0x01, b"ok"), (0x02, b"\xff"), (0x80, b"\xff")], [1, 1, 1]),
    ([(0x01, b"\xff"), (0x82, b"x"), (0x80, b"\xff")], [1, 1, 1]),
    ([(0x02, b"\xff"), (0x01, b"\xc3"), (0x80, b"\xa9")], [1, 1, 1]),         # a BINARY abandoned by a TEXT
    ([(0x02, b"x"), (0x01, b"\xc3"), (0x80, b"(")], [1, 1, 0]),
    # a TEXT still open at the end of the batch
    ([(0x01, b"\xff"), (0x00, b"\xfe")], [1, 1]),
    ([(0x81, b"\xff"), (0x01, b"\xff")], [0, 1]),
    # reserved opcodes 3-7 start messages that are not TEXT
    ([(0x83, b"\xff"), (0x03, b"\xff"), (0x80, b"\xff"), (0x84, b"\xff"), (0x05, b"\xff"), (0x00, b"\xff"),
      (0x80, b"\xff"), (0x86, b"\xff"), (0x07, b"\xff"), (0x80, b"\xff")], [1] * 10),
    ([(0x01, b"\xff"), (0x87, b"x"), (0x80, b"\xff")], [1, 1, 1]),
    ([(0x01, b"\xff"), (0x04, b"x"), (0x80, b"\xff"), (0x81, b"\xc3\xa9")], [1, 1, 1, 1]),
    # RSV bits on the header byte change neither the opcode nor FIN
    ([(0xC1, b"\xff")], [0]),
    ([(0xC1, b"ok"), (0x91, b"\xc3"), (0xF1, b"\xc3\xa9")], [1, 0, 1]),
    ([(0x11, b"\xc3"), (0xB0, b"\xa9")], [1, 1]),
    ([(0x41, b"ab"), (0x30, b"c"), (0x90, b"\x80")], [1, 1, 0]),
    ([(0xC1, b"ok"), (0xB0, b"\x80")], [1, 1]),                                # an orphan with RSV bits
    # a TEXT whose continuation frames are all empty; an empty TEXT is valid
    ([(0x01, b"\xc3\xa9"), (0x00, b""), (0x00, b""), (0x80, b"")], [1, 1, 1, 1]),
    ([(0x01, b"\xc3"), (0x00, b""), (0x80, b"")], [1, 1, 0]),
    ([(0x01, b""), (0x80, b"")], [1, 1]),
    ([(0x81, b""), (0x01, b""), (0x00, b""), (0x80, b"\x80")], [1, 1, 1, 0]),
    # control frames between fragments are not part of the message, whatever they hold
    ([(0x01, b"\xe2\x82"), (0x89, b"\xff\xff"), (0x8A, b"\x80"), (0x80, b"\xac")], [1, 1, 1, 1]),
    ([(0x01, b"\xe2\x82"), (0x89, b"\xac"), (0x80, b"!")], [1, 1, 0]),
    ([(0x01, b"\xe2"), (0x88, b"\x82\xac"), (0x00, b"\x82"), (0x8A, b""), (0x80, b"\xac")], [1, 1, 1, 1, 1]),
]


def batch_arrays(frames):
    """(payload uint8, offsets uint64 [n + 1], header bytes uint8 [n]) of a frame list"""
    payload = np.frombuffer(b"".join(p for _, p in frames), dtype=np.uint8)
    off = np.zeros(len(frames) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for _, p in frames], dtype=np.uint64)
    h0 = np.array([h for h, _ in frames], dtype=np.uint8)
    return payload, off, h0


def structure_counts(h0) -> dict:
    """How many frames of a batch are orphan continuations (opcode 0, no message open) and how
    many data messages are abandoned (a new data frame with a non-zero opcode before the FIN)."""
    open_, orphans, abandoned = False, 0, 0
    for h in np.asarray(h0).tolist():
        op, fin = h & 0x0F, h >> 7
        if op >= 8:
            continue
        if op == 0 and not open_:
            orphans += 1
            continue
        if op != 0 and open_:
            abandoned += 1
        open_ = not fin
    return {"orphans": orphans, "abandoned": abandoned}
