#!/usr/bin/env python3
"""Device frame decode (netc_gpu_decode_frames) beside the frame assembly and the in-place
unmask, one GPU.

Wire streams of configs 2 and 4 shape (masked client frames, built on the host by the oracle
encoder; c4 is 256 MiB of the config-4 size mix), scanned once before the timing.  Three legs,
in the same process, interleaved over --rounds rounds:
  decode   netc_gpu_decode_frames on the scan's outputs (both launches, message table included)
  encode   netc_gpu_encode_frames (general entry) on the same batch: the yardstick -- it moves
           the same algorithmic bytes the other way, payload in and wire out
  unmask   netc_gpu_unmask_frames on (a copy of) the same wire, in place
Every leg rotates through enough buffer sets that a step never finds its data in the 256 MiB
MALL.  GPU time from two events around --steps calls on the launch stream.  The decode's
outputs of the last step are compared with the batch that was encoded.  One JSON line per
workload; --out appends them to a file as a JSON list.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MALL = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="c2,c4", help="c2, c4 (256 MiB of the config-4 mix), tiny16")
    ap.add_argument("--legs", default="decode,encode,unmask")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from netc_amd import _lib, synth
    from netc_amd import mask as nm
    from oracle import oracle as orc

    dev = torch.device("cuda", 0)
    g = _lib.gpu()
    s = torch.cuda.Stream(dev)
    sh = s.cuda_stream
    results = []
    for wl in args.workloads.split(","):
        if wl == "tiny16":   # 64 MiB of uniform 16-byte frames (README "small frames"): the gather's compose path
            off = synth.uniform_offsets((64 << 20) // 16, 16)
            keys = synth.random_keys(off.size - 1)
        else:
            off, keys, _ = synth.config(wl)
        if wl == "c4":
            cut = int(np.searchsorted(off, 256 << 20))
            off, keys = off[: cut + 1], keys[:cut]
        n, total = keys.size, int(off[-1])
        payload = np.random.default_rng(5).integers(0, 256, total, dtype=np.uint8)
        wire, _ = orc.encode_batch(payload, off, keys, None, True)
        sets = max(2, -(-2 * MALL // (wire.size + total)))   # wire + payload of all sets: twice the MALL
        d_payload = torch.from_numpy(payload).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_keys = torch.from_numpy(keys.view(np.int32)).to(dev)
        S = []
        for _ in range(sets):
            S.append(dict(
                wire=torch.from_numpy(wire).to(dev), wire_um=torch.from_numpy(wire).to(dev),
                wire_out=torch.empty(nm.wire_bound(total, n, True), dtype=torch.uint8, device=dev),
                src=d_payload.clone(), out=torch.empty(wire.size, dtype=torch.uint8, device=dev),
                off=torch.empty(n + 1, dtype=torch.int64, device=dev), wo=torch.empty(n + 1, dtype=torch.int64, device=dev),
                first=torch.empty(n + 1, dtype=torch.int64, device=dev), op=torch.empty(n, dtype=torch.uint8, device=dev),
                dres=torch.empty(3, dtype=torch.int64, device=dev)))
        hdr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        kk = torch.empty(n, dtype=torch.int32, device=dev)
        b0 = torch.empty(n, dtype=torch.uint8, device=dev)
        res = torch.empty(3, dtype=torch.int64, device=dev)
        with torch.cuda.stream(s):
            nm.scan_frames(S[0]["wire"], hdr, kk, b0, res, stream=s)   # the same offsets hold for every copy
        torch.cuda.synchronize()
        assert int(res[0]) == n and int(res[1]) == wire.size

        def check(rc):
            if rc:
                raise RuntimeError(g.netc_gpu_strerror())

        def decode(b):
            check(g.netc_gpu_decode_frames(0, b["out"].data_ptr(), wire.size, b["off"].data_ptr(), b["first"].data_ptr(),
                                           b["op"].data_ptr(), b["dres"].data_ptr(), b["wire"].data_ptr(), wire.size,
                                           hdr.data_ptr(), kk.data_ptr(), b0.data_ptr(), n, res.data_ptr(), sh))

        def encode(b):
            check(g.netc_gpu_encode_frames(0, b["wire_out"].data_ptr(), b["wire_out"].numel(), b["wo"].data_ptr(),
                                           b["src"].data_ptr(), total, d_off.data_ptr(), d_keys.data_ptr(), 0, n, 1, sh))

        def unmask(b):   # in place: every call toggles its own copy of the wire
            check(g.netc_gpu_unmask_frames(0, b["wire_um"].data_ptr(), wire.size, hdr.data_ptr(), kk.data_ptr(), n,
                                           res.data_ptr(), sh))

        legs = {"decode": decode, "encode": encode, "unmask": unmask}
        us = {k: [] for k in args.legs.split(",")}
        for _ in range(args.rounds):
            for name in us:
                f = legs[name]
                for i in range(args.warmup):
                    f(S[i % sets])
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for i in range(args.steps):
                    f(S[i % sets])
                b.record(s)
                torch.cuda.synchronize()
                us[name].append(round(a.elapsed_time(b) / args.steps * 1e3, 2))
        rec = {"workload": wl, "frames": int(n), "payload_bytes": total, "wire_bytes": int(wire.size),
               "algorithmic_bytes": total + int(wire.size), "buffer_sets": sets, "steps": args.steps,
               "us_rounds": us, "us_median": {k: float(np.median(v)) for k, v in us.items()}}
        if "decode" in us:
            last = S[(args.steps - 1) % sets]
            rec["decode_matches_batch"] = bool(
                torch.equal(last["out"][:total], d_payload) and torch.equal(last["off"], d_off)
                and last["dres"].tolist() == [n, total, n] and int(last["first"][n]) == n and bool((last["op"] == 2).all()))
            rec["decode_GBps"] = round(rec["algorithmic_bytes"] / rec["us_median"]["decode"] / 1e3, 1)
            if "encode" in us:
                rec["decode_over_encode"] = round(rec["us_median"]["decode"] / rec["us_median"]["encode"], 3)
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del S, d_payload
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
