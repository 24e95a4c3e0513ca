#!/usr/bin/env python3
"""ugo_fec_stream_set_deliver / ugo_fec_stream_set_read against the single
entry points: 851,968 received packets with one 1400-B segment
each, slot 1488, the RC4 pad, spread round-robin over nconn connections.  Not
product code.

Per case (nconn, window bytes, arrival) the batch goes once through a set into
fresh windows and every window byte, every record and every status is checked.
Then two forms alternate, rep by rep, in this process and on the same windows
(set calls and single calls on a member may be mixed):

  set     one ugo_fec_stream_set_deliver over the interleaved batch, one
          ugo_fec_stream_set_read that drains (discards) every member;
  looped  nconn ugo_fec_stream_deliver calls over the same packets pre-sorted by
          connection (the sort is not timed) and nconn ugo_fec_stream_read
          calls -- all there was before the set entry points.  With nconn = 1 it
          is the single call itself.

After each form the segments' stream offsets move on by what a connection
received, so the rings lap.  wall ms: device events around the deliver and the
read of a form, launch gaps included.  kernel ms (launch-timing ABI): each
launch's own duration; for the set form always, for the looped form up to
--hooked-loop-max connections.  An nt copy of the same bytes is timed in the
same run.  Prints one JSON line per case.

  python3 tools/stream_set_probe.py [--reps 6] [--cases n1,n1024,n16384,n1024_repeat_1pct]
"""
import argparse
import ctypes
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
KERNELS = ("classify", "resolve", "apply", "ordered", "copy", "scan", "finish")
CASES = {  # name: (nconn, window bytes, 1 % of each connection's packets repeated inside the batch)
    "n1": (1, 1 << 31, False),
    "n1024": (1024, 2 << 20, False),
    "n16384": (16384, 128 << 10, False),
    "n1024_repeat_1pct": (1024, 2 << 20, True),
}


def uvarint_len(v):
    return np.maximum(1, (np.floor(np.log2(np.maximum(v, 1))).astype(np.int64) + 7) // 7)


def local_arrival(per, repeat, rng):
    """piece[k] = which 1400-B piece of its connection's stream a connection's
    k-th packet carries; n_unique pieces per connection."""
    if not repeat:
        return np.arange(per), per
    ndup = max(1, per // 100)
    uniq = per - ndup
    src = np.sort(rng.choice(uniq, ndup, replace=False))   # a repeat follows its original by 1..32 packets
    key = np.concatenate([np.arange(uniq) * 2, (src + rng.integers(1, 33, ndup)) * 2 + 1])
    order = np.argsort(key, kind="stable")
    return np.concatenate([np.arange(uniq), src])[order], uniq


def spread(v):
    return {"min": round(float(np.min(v)), 4), "median": round(float(np.median(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--packets", type=int, default=851968)
    ap.add_argument("--cases", default="n1,n1024,n16384,n1024_repeat_1pct")
    ap.add_argument("--hooked-loop-max", type=int, default=1024)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    lib = fec.load_library()
    dev = torch.device("cuda", 0)
    cur = torch.cuda.current_stream(dev)
    sh = cur.cuda_stream or None
    enc = fec.New(10, 3)
    rng = np.random.default_rng(23)
    ks = np.frombuffer(fec.rc4_keystream(b"1234567890123456", SLOT), np.uint8)
    pad = torch.from_numpy(ks.copy()).to(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    npk = args.packets
    stream = torch.randint(0, 256, (npk, SEG), dtype=torch.uint8, device=dev, generator=gen)
    scratch = torch.empty(npk * SEG, dtype=torch.uint8, device=dev)      # the nt copy's destination

    for case in args.cases.split(","):
        nconn, window, repeat = CASES[case]
        assert npk % nconn == 0
        per = npk // nconn
        piece, uniq = local_arrival(per, repeat, rng)
        per_total = uniq * SEG
        assert per_total <= window
        # packet i = k * nconn + c: connection c's k-th packet, its piece `piece[k]`
        k_of = np.arange(npk) // nconn
        c_of = (np.arange(npk) % nconn).astype(np.uint32)
        offs = piece[k_of].astype(np.uint64) * np.uint64(SEG)
        src_row = piece[k_of] * nconn + c_of                             # row of `stream` it carries
        doff = 1 + 3 + uvarint_len(offs) + 2
        info = np.zeros(npk, fec.PKT_INFO_DTYPE)
        info["n_segments"] = 1
        segs = np.zeros((npk, 1), fec.PKT_SEGMENT_DTYPE)
        segs["offset"][:, 0] = offs
        segs["data_off"][:, 0] = doff
        segs["len"][:, 0] = SEG
        segs["avail"][:, 0] = SEG
        wire = torch.randint(0, 256, (npk, SLOT), dtype=torch.uint8, device=dev, generator=gen)
        d_src = torch.from_numpy(src_row).to(dev)
        for d in np.unique(doff):
            rows = torch.from_numpy(np.nonzero(doff == d)[0]).to(dev)
            wire[rows, d:d + SEG] = stream[d_src[rows]] ^ pad[d:d + SEG]
        d_info = torch.from_numpy(info.view(np.uint8).reshape(npk, 64).copy()).to(dev)
        d_segs = torch.from_numpy(segs.view(np.uint8).reshape(npk, 1, 16).copy()).to(dev)
        d_conn = torch.from_numpy(c_of.view(np.int32).copy()).to(dev)
        status = torch.empty((npk, 1), dtype=torch.uint8, device=dev)
        if nconn == 1:
            wire_s, segs_s, status_s = wire, d_segs, status
        else:  # the looped form's input: the same packets, sorted by connection (not timed)
            wire_s = wire.view(per, nconn, SLOT).transpose(0, 1).contiguous()
            segs_s = d_segs.view(per, nconn, 16).transpose(0, 1).contiguous()
            status_s = torch.empty((npk, 1), dtype=torch.uint8, device=dev)
        seg_offs = [t.view(torch.int64).view(-1, 2)[:, 0] for t in ({id(d_segs): d_segs, id(segs_s): segs_s}).values()]

        rxs = [fec.StreamRx(enc, window) for _ in range(nconn)]
        rset = fec.StreamRxSet(enc, rxs)
        d_n = torch.full((nconn,), per_total, dtype=torch.int64, device=dev)
        d_nread = torch.zeros(nconn, dtype=torch.int64, device=dev)
        d_eof = torch.zeros(nconn, dtype=torch.uint8, device=dev)

        # ---- once into fresh windows: every byte, every record, every status
        rset.deliver(wire, d_info, d_segs, d_conn, pad=pad, out=status)
        recs = rset.states()
        ok_bytes = True
        by_conn = stream.view(per, nconn, SEG)
        for c in range(nconn):
            win = rxs[c].window()
            ok_bytes &= bool(torch.equal(win[:per_total], by_conn[:uniq, c].reshape(-1))) and not bool(win[per_total:].any())
        first = piece[k_of] >= 0
        if repeat:  # a connection's repeat comes after its original: the later one is the duplicate
            seen = np.zeros(per, bool)
            dup_k = np.zeros(per, bool)
            for k, p in enumerate(piece):
                dup_k[k] = seen[p]
                seen[p] = True
            first = ~dup_k[k_of]
        want_status = torch.from_numpy(np.where(first, 1, 2).astype(np.uint8)).to(dev)
        ok_status = bool(torch.equal(status[:, 0], want_status))
        ok_rec = all(int(r["accepted"]) == uniq and int(r["duplicate"]) == per - uniq and int(r["err"]) == 0 and
                     int(r["readable"]) == per_total and int(r["ngaps"]) == 1 and int(r["hi"]) == per_total and
                     int(r["skipped_packets"]) == 0 and int(r["out_of_window"]) == 0 for r in recs)
        ordered_first = int(recs["ordered_segments"].sum())

        # ---- the two forms
        p_wire, p_info, p_segs, p_stat, p_pad = (t.data_ptr() for t in (wire_s, d_info, segs_s, status_s, pad))
        handles = [rx._h for rx in rxs]
        nread1 = torch.zeros(1, dtype=torch.int64, device=dev)
        p_nread1 = nread1.data_ptr()

        def advance():
            for o in seg_offs:
                o.add_(per_total)

        def set_deliver():
            rset.deliver(wire, d_info, d_segs, d_conn, pad=pad, out=status)

        def set_read():
            rset.read(d_n, n_read=d_nread, eof=d_eof)

        def loop_deliver():
            for c, h in enumerate(handles):
                rc = lib.ugo_fec_stream_deliver(h, p_wire + c * per * SLOT, SLOT, p_pad, p_info + c * per * 64,
                                                p_segs + c * per * 16, 1, per, p_stat + c * per, sh)
                assert rc == 0

        def loop_read():
            for h in handles:
                rc = lib.ugo_fec_stream_read(h, None, per_total, p_nread1, None, sh)
                assert rc == 0

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            return a, b

        set_read()
        advance()
        for fn in (set_deliver, set_read, advance, loop_deliver, loop_read, advance):   # warm both forms
            fn()
        torch.cuda.synchronize()
        reps = args.reps if nconn < 16384 else min(args.reps, 3)
        ev = {"set_deliver": [], "set_read": [], "loop_deliver": [], "loop_read": []}
        for _ in range(reps):
            ev["set_deliver"].append(timed(set_deliver))
            ev["set_read"].append(timed(set_read))
            advance()
            ev["loop_deliver"].append(timed(loop_deliver))
            ev["loop_read"].append(timed(loop_read))
            advance()
        torch.cuda.synchronize()
        wall = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}

        # per-launch durations, the forms alternating again
        hook_loop = nconn <= args.hooked_loop_max
        per_k = {k: [] for k in KERNELS}
        set_sum, set_read_k, loop_sum, loop_read_k, loop_copy = [], [], [], [], []
        for _ in range(reps):
            enc.timing_begin(8)
            set_deliver()
            set_read()
            r, untimed = enc.timing_end()
            assert untimed == 0 and len(r) == 8 and (r["kernel"][:7] == fec.KERNEL_IDS["stream_deliver"]).all()
            for k, name in enumerate(KERNELS):
                per_k[name].append(float(r["ms"][k]))
            set_sum.append(float(r["ms"][:7].sum()))
            set_read_k.append(float(r["ms"][7]))
            advance()
            if hook_loop:
                enc.timing_begin(8 * nconn)
                loop_deliver()
                loop_read()
                r, untimed = enc.timing_end()
                assert untimed == 0 and len(r) == 8 * nconn
                loop_sum.append(float(r["ms"][:7 * nconn].sum()))
                loop_copy.append(float(r["ms"][:7 * nconn].reshape(nconn, 7)[:, 4].sum()))
                loop_read_k.append(float(r["ms"][7 * nconn:].sum()))
            else:
                loop_deliver()
                loop_read()
            advance()
        end = rset.states()
        calls = 2 + 4 * reps + 1
        ok_laps = bool((end["err"] == 0).all() and (end["read_pos"] == calls * per_total).all() and
                       (end["accepted"] == calls * uniq).all() and (end["readable"] == 0).all())
        total = nconn * per_total
        cb = total // 16 * 16
        copy_ms = bench.probe_nt_copy_ms([wire.data_ptr()], [scratch.data_ptr()], cb, max(reps, 4), cur.cuda_stream)
        med = {k: float(np.median(v)) for k, v in per_k.items()}
        out = {
            "probe": "stream_set", "label": args.label, "case": case, "nconn": nconn, "window_bytes": window,
            "packets": npk, "packets_per_conn": per, "slot": SLOT, "segment_bytes": SEG, "stream_bytes": total,
            "repeat_1pct": repeat, "verify_every_window_byte": bool(ok_bytes), "verify_every_record": bool(ok_rec),
            "verify_every_status": ok_status, "verify_laps": ok_laps, "ordered_segments_first_call": ordered_first,
            "reps": reps,
            "set_kernel_ms": {k: round(v, 4) for k, v in med.items()},
            "set_deliver_kernel_sum_ms": spread(set_sum), "set_read_kernel_ms": spread(set_read_k),
            "set_deliver_wall_ms": spread(wall["set_deliver"]), "set_read_wall_ms": spread(wall["set_read"]),
            "loop_deliver_wall_ms": spread(wall["loop_deliver"]), "loop_read_wall_ms": spread(wall["loop_read"]),
            "loop_deliver_kernel_sum_ms": spread(loop_sum) if hook_loop else "not measured",
            "loop_copy_kernel_sum_ms": spread(loop_copy) if hook_loop else "not measured",
            "loop_read_kernel_sum_ms": spread(loop_read_k) if hook_loop else "not measured",
            "ratio_set_to_loop_deliver_wall": round(float(np.median(wall["set_deliver"]) / np.median(wall["loop_deliver"])), 4),
            "ratio_set_to_loop_read_wall": round(float(np.median(wall["set_read"]) / np.median(wall["loop_read"])), 4),
            "ratio_set_to_loop_deliver_kernel_sum": round(float(np.median(set_sum) / np.median(loop_sum)), 4) if hook_loop else "not measured",
            "nt_copy_same_bytes_ms": round(copy_ms, 4),
            "set_copy_kernel_frac_of_nt_copy": round(copy_ms / med["copy"], 4),
            "note": "wall = device events around the calls of one form (launch gaps and the host's launch rate "
                    "included); kernel sums = each launch's own duration (hipExtLaunchKernel events), gaps excluded; "
                    "set and looped forms alternate rep by rep on the same windows; looped = nconn single calls "
                    "on packets pre-sorted by connection, the sort not timed"}
        print(json.dumps(out), flush=True)
        rset.close()
        for rx in rxs:
            rx.close()
        del wire, wire_s, d_info, d_segs, segs_s, status, status_s, rxs
    enc.close()


if __name__ == "__main__":
    main()
