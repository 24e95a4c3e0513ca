#!/usr/bin/env python3
"""ugo_fec_stream_deliver / ugo_fec_stream_read on the packet codec's workload
(DESIGN.md §3.7): 851,968 received packets with one 1400-B segment each, slot
1488, the RC4 pad, into a 2-GiB receive window.  Not product code.

Three arrival orders: in order; shuffled within runs of 64 packets; in order
with 1 % of the packets repeated inside the batch (the ordered pass).  For each,
a fresh window takes the batch once and every window byte, the record and the
statuses are checked.  Then the batch is delivered `reps` times, each followed by
a read that discards it and by moving the segments' stream offsets on by the
batch's bytes, so the ring laps; every launch is timed with the launch-timing
ABI (kernel classes stream_deliver -- seven launches per call, reported one by
one -- and stream_read).  An nt copy of the same byte count, ring -> window, is
timed in the same run as the ceiling.  Algorithmic bytes = segment bytes read +
window bytes written.  Prints one JSON line per case.

  python3 tools/stream_deliver_probe.py [--reps 10] [--packets 851968] [--label TEXT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (probe_nt_copy_ms)
from ugo_amd import fec  # noqa: E402

SLOT, SEG = 1488, 1400
NL = 8  # launches per deliver + read
KERNELS = ("classify", "resolve", "apply", "ordered", "copy", "scan", "finish")


def uvarint_len(v):
    return np.maximum(1, (np.floor(np.log2(np.maximum(v, 1))).astype(np.int64) + 7) // 7)


def arrival(case, npk, rng):
    """chunk[i] = which 1400-B piece of the stream packet i carries; n_unique pieces in all."""
    if case == "in_order":
        return np.arange(npk), npk
    if case == "shuffled_64":
        c = np.arange(npk)
        for k in range(0, npk, 64):
            rng.shuffle(c[k:k + 64])
        return c, npk
    ndup = npk // 100
    uniq = npk - ndup
    # a repeat follows its original by 1..32 packets
    src = np.sort(rng.choice(uniq, ndup, replace=False))
    key = np.concatenate([np.arange(uniq) * 2, (src + rng.integers(1, 33, ndup)) * 2 + 1])
    order = np.argsort(key, kind="stable")
    return np.concatenate([np.arange(uniq), src])[order], uniq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--packets", type=int, default=851968)
    ap.add_argument("--window", type=int, default=1 << 31)
    ap.add_argument("--label", default="")
    ap.add_argument("--cases", default="in_order,shuffled_64,repeat_1pct")
    ap.add_argument("--no-pad", action="store_true", help="packets in the clear, no keystream (what the pad XOR costs)")
    args = ap.parse_args()
    npk = args.packets
    dev = torch.device("cuda", 0)
    cur = torch.cuda.current_stream(dev)
    enc = fec.New(10, 3)
    rng = np.random.default_rng(23)
    ks = np.frombuffer(fec.rc4_keystream(b"1234567890123456", SLOT), np.uint8)
    pad = None if args.no_pad else torch.from_numpy(ks.copy()).to(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    stream = torch.randint(0, 256, (npk, SEG), dtype=torch.uint8, device=dev, generator=gen)

    for case in args.cases.split(","):
        chunk, uniq = arrival(case, npk, rng)
        total = uniq * SEG
        assert total <= args.window
        offs = chunk.astype(np.uint64) * np.uint64(SEG)
        doff = 1 + 3 + uvarint_len(offs) + 2              # flags, packet number, offset, length
        info = np.zeros(npk, fec.PKT_INFO_DTYPE)
        info["n_segments"] = 1
        segs = np.zeros((npk, 1), fec.PKT_SEGMENT_DTYPE)
        segs["offset"][:, 0] = offs
        segs["data_off"][:, 0] = doff
        segs["len"][:, 0] = SEG
        segs["avail"][:, 0] = SEG
        wire = torch.randint(0, 256, (npk, SLOT), dtype=torch.uint8, device=dev, generator=gen)
        d_chunk = torch.from_numpy(chunk).to(dev)
        for d in np.unique(doff):
            rows = torch.from_numpy(np.nonzero(doff == d)[0]).to(dev)
            wire[rows, d:d + SEG] = stream[d_chunk[rows]] if pad is None else stream[d_chunk[rows]] ^ pad[d:d + SEG]
        d_info = torch.from_numpy(info.view(np.uint8).reshape(npk, 64).copy()).to(dev)
        d_segs = torch.from_numpy(segs.view(np.uint8).reshape(npk, 1, 16).copy()).to(dev)
        seg_off = d_segs.view(torch.int64)[:, :, 0]       # the offset field of every descriptor
        status = torch.empty((npk, 1), dtype=torch.uint8, device=dev)

        # ---- once into a fresh window: every byte, the record, the statuses
        rx = fec.StreamRx(enc, args.window)
        rx.deliver(wire, d_info, d_segs, pad=pad, out=status)
        rec = rx.state()
        win = rx.window()
        ok_bytes = bool(torch.equal(win[:total], stream[:uniq].reshape(-1))) and not bool(win[total:].any())
        counts = torch.bincount(status.reshape(-1).to(torch.int64), minlength=6).cpu().numpy()
        ok_rec = (int(rec["accepted"]) == uniq and int(rec["duplicate"]) == npk - uniq and int(rec["err"]) == 0 and
                  int(rec["readable"]) == total and int(rec["ngaps"]) == 1 and int(rec["hi"]) == total and
                  counts[1] == uniq and counts[2] == npk - uniq and counts.sum() == npk)
        ordered = int(rec["ordered_segments"])
        del win

        # ---- timed: deliver, read(discard), move the offsets on; the ring laps
        reps = args.reps if case != "repeat_1pct" else min(args.reps, 4)
        per = {k: [] for k in KERNELS}
        read_ms = []

        def step():
            rx.deliver(wire, d_info, d_segs, pad=pad, out=status)
            rx.read(total, discard=True)
            seg_off.add_(total)

        rx.read(total, discard=True)
        seg_off.add_(total)
        step()
        torch.cuda.synchronize()
        enc.timing_begin(NL * reps)
        for _ in range(reps):
            step()
        recs, untimed = enc.timing_end()
        assert untimed == 0 and len(recs) == NL * reps
        for r in range(reps):
            blk = recs[NL * r:NL * r + NL]
            assert (blk["kernel"][:NL - 1] == fec.KERNEL_IDS["stream_deliver"]).all() and \
                blk["kernel"][NL - 1] == fec.KERNEL_IDS["stream_read"]
            for k, name in enumerate(KERNELS):
                per[name].append(float(blk["ms"][k]))
            read_ms.append(float(blk["ms"][NL - 1]))
        end = rx.state()
        ok_laps = int(end["err"]) == 0 and int(end["read_pos"]) == (reps + 2) * total and \
            int(end["accepted"]) == (reps + 2) * uniq
        alg = 2 * total
        wptr = rx.window().data_ptr()
        cb = min(total, wire.numel()) // 16 * 16
        copy_ms = bench.probe_nt_copy_ms([wire.data_ptr()], [wptr], cb, max(reps, 4), cur.cuda_stream) * total / cb
        med = {k: float(np.median(v)) for k, v in per.items()}
        deliver = float(np.median(np.sum([per[k] for k in KERNELS], axis=0)))
        print(json.dumps({
            "probe": "stream_deliver", "label": args.label, "case": case, "pad": pad is not None, "packets": npk, "slot": SLOT,
            "segment_bytes": SEG, "window_bytes": args.window, "stream_bytes": total,
            "verify_every_window_byte": ok_bytes, "verify_record_and_statuses": bool(ok_rec),
            "verify_laps": bool(ok_laps), "ordered_segments_first_call": ordered, "reps": reps,
            "kernel_ms": {k: round(v, 4) for k, v in med.items()}, "deliver_ms": round(deliver, 4),
            "read_discard_ms": round(float(np.median(read_ms)), 4), "algorithmic_bytes": alg,
            "copy_kernel_GBps": round(alg / (med["copy"] * 1e-3) / 1e9, 1),
            "nt_copy_same_bytes_ms": round(copy_ms, 4),
            "copy_kernel_frac_of_nt_copy": round(copy_ms / med["copy"], 4),
            "deliver_frac_of_nt_copy": round(copy_ms / deliver, 4),
            "note": "kernel ms = median over reps of each launch's own duration (hipExtLaunchKernel events); "
                    "deliver_ms = median of the seven launches' sum (gaps between launches not included); nt copy = "
                    "libugoprobe's one-chunk-per-thread nt copy of stream_bytes, ring -> window"}), flush=True)
        rx.close()
        del wire, d_info, d_segs, status
    enc.close()


if __name__ == "__main__":
    main()
