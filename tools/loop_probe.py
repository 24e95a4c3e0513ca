#!/usr/bin/env python3
"""The connection loop on the device (ugo_fec_loop_*) on the
README's ring: 851,968 decoded packets spread over 1, 1,024 and 16,384
connections, 1 % of the members closing and 1 % ending (peer RST, ACK|FIN or a
corrupt packet) per call.  Not product code.

Per number of connections, on a fresh loop set per repetition:
  receive        ugo_fec_loop_set_receive (3 launches)
  close, check, append, sent   the four per-member calls (1, 1, 2, 2 launches)
Timed: the summed kernel durations of a call (the launch-timing ABI) and the
elapsed time between two events around it, launch gaps included; median of the
repetitions.  conn_of, the records and the outputs of the first repetition are
compared with the RuleLoop of tests/loop_ref.py.

Comparators, in the same run:
  nt copy        libugoprobe's nt copy scaled to the bytes receive reads (the
                 64-byte record once, conn_of twice)
  read-back      what the calls replace: the pinned read-back of one flags and
                 one status byte per packet (gathered on the device first) and of
                 rto_count / err per member, the pinned upload of may_ack_only
  ack receive,   ugo_fec_ack_set_receive and ugo_fec_stream_set_deliver on the
  deliver        conn_of receive has passed over and on the one it has not, same
                 repetitions, taking turns to go first
  FIN / RST      the pinned upload of hand-written FIN / RST records

  python3 tools/loop_probe.py [--reps 8] [--packets 851968] [--conns 1,1024,16384] [--label TEXT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (probe_nt_copy_ms)
import loop_ref as lf  # noqa: E402
from ugo_amd import fec  # noqa: E402

NOW = 1_000_000
SLOT, SEG = 64, 32                                              # set_deliver's packets: one segment of SEG bytes at 16


def timed(enc, call, n_launches, kernel="loop"):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    enc.timing_begin(n_launches or 16)
    e0.record()
    call()
    e1.record()
    recs, untimed = enc.timing_end()
    torch.cuda.synchronize()
    assert untimed == 0 and (kernel is None or (recs["kernel"] == fec.KERNEL_IDS[kernel]).all()), recs
    assert n_launches is None or len(recs) == n_launches, recs
    return float(recs["ms"].sum()), float(e0.elapsed_time(e1))


def wall(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return float(e0.elapsed_time(e1))


def run(enc, nconn, npk, reps, label):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(nconn)
    per = (npk + nconn - 1) // nconn                            # packets of a member: SEG stream bytes each, in order
    window = max(4096, 1 << (per * SEG - 1).bit_length())
    rxs = [fec.StreamRx(enc, window) for _ in range(nconn)]
    acks = [fec.AckRx(enc, 1024) for _ in range(nconn)]
    txs = [fec.StreamTx(enc, 4096, 4) for _ in range(nconn)]
    sents = [fec.SentTx(enc, 1024, 1) for _ in range(nconn)]
    rset, aset = fec.StreamRxSet(enc, rxs), fec.AckRxSet(enc, acks)
    tset, sset = fec.StreamTxSet(enc, txs), fec.SentTxSet(enc, sents)
    # the batch: data packets, 1 % of the members end somewhere in it
    who = (np.arange(npk) % nconn).astype(np.uint32)
    raw = np.zeros((npk, 64), np.uint8)
    iv = raw.view(fec.PKT_INFO_DTYPE).reshape(-1)
    iv["flags"], iv["packet_number"], iv["n_segments"] = 0x20, 1 + np.arange(npk) // nconn, 1
    n_end = max(1, nconn // 100)
    for k, c in enumerate(rng.choice(nconn, n_end, replace=False)):
        i = int(c) + nconn * int(rng.integers(0, npk // nconn))
        if k % 3 == 2:
            iv["status"][i] = 3
        else:
            iv["flags"][i] = (0x08, 0x90)[k % 3]
    info = torch.from_numpy(raw).to(dev)
    segs_np = np.zeros((npk, 1, 16), np.uint8)
    sv = segs_np.view(fec.PKT_SEGMENT_DTYPE).reshape(npk, 1)
    sv["offset"][:, 0], sv["data_off"][:, 0] = SEG * (np.arange(npk) // nconn), 16
    sv["len"][:, 0] = sv["avail"][:, 0] = SEG
    segs = torch.from_numpy(segs_np).to(dev)
    wire = torch.from_numpy(rng.integers(0, 256, (npk, SLOT), dtype=np.uint8)).to(dev)
    seg_status = torch.zeros((npk, 1), dtype=torch.uint8, device=dev)
    conn0 = torch.from_numpy(who.view(np.int32)).to(dev)
    how_np = np.zeros(nconn, np.uint8)
    how_np[rng.choice(nconn, n_end, replace=False)] = 1
    how = torch.from_numpy(how_np).to(dev)
    conn = conn0.clone()
    budget = torch.zeros(nconn, dtype=torch.int32, device=dev)
    may = torch.zeros(nconn, dtype=torch.uint8, device=dev)
    cap = 2 * n_end + 8
    pinfo = torch.zeros((cap, 64), dtype=torch.uint8, device=dev)
    psegs = torch.zeros((cap, 2, 16), dtype=torch.uint8, device=dev)
    pconn = torch.zeros(cap, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    appended = torch.zeros(nconn, dtype=torch.uint8, device=dev)
    zeros32, zeros8 = torch.zeros(nconn, dtype=torch.int32, device=dev), torch.zeros(nconn, dtype=torch.uint8, device=dev)
    out = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(nconn, dtype=torch.int32, device=dev),
           torch.zeros(nconn, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
           torch.zeros(nconn, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    # what the calls replace
    pin_bytes = torch.zeros((npk, 2), dtype=torch.uint8).pin_memory()
    pin_member = torch.zeros((nconn, 2), dtype=torch.int32).pin_memory()
    pin_may = torch.ones(nconn, dtype=torch.uint8).pin_memory()
    dev_member = torch.zeros((nconn, 2), dtype=torch.int32, device=dev)
    may_up = torch.zeros(nconn, dtype=torch.uint8, device=dev)
    pin_info, pin_segs = torch.zeros((cap, 64), dtype=torch.uint8).pin_memory(), \
        torch.zeros((cap, 2, 16), dtype=torch.uint8).pin_memory()
    pin_conn = torch.zeros(cap, dtype=torch.int32).pin_memory()
    up_info, up_segs, up_conn = torch.zeros_like(pinfo), torch.zeros_like(psegs), torch.zeros_like(pconn)
    rset.deliver(wire, info, segs, conn0, out=seg_status)       # every timed deliver finds the bytes there already
    t = {}
    ok = True
    for r in range(reps + 2):                                   # two warm-up rounds, the first one verified
        loop = fec.LoopSet(enc, rset, aset, tset, sset, now_us=NOW)
        conn.copy_(conn0)
        budget.fill_(8)
        total.zero_()
        res = {"receive": timed(enc, lambda: loop.receive(info, conn, NOW + 10), 3)}
        res["close"] = timed(enc, lambda: loop.close_members(how, NOW + 20), 1)
        res["check"] = timed(enc, lambda: loop.check(NOW + 30, budget, may_ack_only=may), 1)
        res["append"] = timed(enc, lambda: loop.append(total, pinfo, psegs, pconn, appended=appended), 2)
        res["sent"] = timed(enc, lambda: loop.sent(zeros32, zeros8, NOW + 40, out=out), 2)
        # ugo_fec_ack_set_receive behind receive, and on the conn_of it has not passed over
        # (the history is not fresh the second time: the two take turns to go first)
        for name in (("ack_receive_masked", "ack_receive_plain") if r % 2 else ("ack_receive_plain", "ack_receive_masked")):
            res[name] = timed(enc, lambda: aset.receive(info, conn if name.endswith("masked") else conn0, NOW + 50),
                              None, "ack")
        # ugo_fec_stream_set_deliver likewise (the windows hold the batch: both forms see duplicates)
        for name in (("deliver_masked", "deliver_plain") if r % 2 else ("deliver_plain", "deliver_masked")):
            res[name] = timed(enc, lambda: rset.deliver(wire, info, segs, conn if name.endswith("masked") else conn0,
                                                        out=seg_status), None, None)
        # the FIN / RST records a caller wrote by hand: 2 % of the members' records, segment rows and conn_of, uploaded
        res["fin_rst_upload"] = (0.0, wall(lambda: (up_info.copy_(pin_info, non_blocking=True),
                                                      up_segs.copy_(pin_segs, non_blocking=True),
                                                      up_conn.copy_(pin_conn, non_blocking=True))))
        res["readback"] = (0.0, wall(lambda: (pin_bytes.copy_(info[:, 40:54:12], non_blocking=True),
                                                pin_member.copy_(dev_member, non_blocking=True),
                                                may_up.copy_(pin_may, non_blocking=True))))
        if r == 0:
            rules = [lf.RuleLoop(NOW) for _ in range(nconn)]
            want = lf.receive_set(rules, iv["status"], iv["flags"], iv["packet_number"], who.tolist(), NOW + 10)
            ok = ok and np.array_equal(conn.cpu().numpy().view(np.uint32), np.asarray(want, np.uint32))
            lf.close_set(rules, how_np, None, NOW + 20)
            nbs = [lf.NB_IDLE] * nconn
            wb, wm = lf.check_set(rules, nbs, NOW + 30, [8] * nconn)
            ok = ok and budget.cpu().numpy().tolist() == wb and may.cpu().numpy().tolist() == wm
            writes, wa, wt = lf.append_set(rules, nbs, 0, cap)
            ok = ok and appended.cpu().numpy().tolist() == wa and int(total.item()) == wt
            ws = lf.sent_set(rules, nbs, [0] * nconn, [0] * nconn, None, NOW + 40, nconn)
            ok = ok and int(out[3].item()) == ws[3] and out[1][:ws[3]].cpu().numpy().tolist() == ws[1]
            ok = ok and int(out[0].cpu().numpy().view(np.uint64)[0]) == ws[0] and int(out[5].item()) == ws[5]
            st = loop.states()
            for k in lf.RuleLoop.FIELDS:
                ok = ok and np.array_equal(st[k].astype(np.uint64), np.array([getattr(x, k) for x in rules], np.uint64))
        loop.close()
        if r >= 2:
            for k, (ms, w) in res.items():
                t.setdefault(k, []).append(ms)
                t.setdefault(k + "_wall", []).append(w)
    stream = torch.cuda.current_stream()
    src, dst = torch.zeros(npk * 64, dtype=torch.uint8, device=dev), torch.zeros(npk * 64, dtype=torch.uint8, device=dev)
    copy_ms = bench.probe_nt_copy_ms([src.data_ptr()], [dst.data_ptr()], npk * 64, reps, stream.cuda_stream)
    read = npk * (64 + 8)
    ack0, rx_states = aset.states(), rset.states()
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"probe": "loop", "label": label, "connections": nconn, "packets": npk, "ending_members": n_end,
           "closing_members": n_end, "reps": reps, "verify_every_output_of_the_first_repetition": bool(ok)}
    for k in ("receive", "close", "check", "append", "sent", "ack_receive_masked", "ack_receive_plain", "deliver_masked",
              "deliver_plain"):
        res[k + "_ms"] = round(med[k], 4)
        res[k + "_wall_ms"] = round(med[k + "_wall"], 4)
    res["receive_min_max"] = [round(min(t["receive"]), 4), round(max(t["receive"]), 4)]
    res["receive_bytes_read"] = read
    res["nt_copy_same_bytes_ms"] = round(copy_ms * read / (npk * 64), 4)    # as tools/ack_probe.py scales it
    res["receive_over_nt_copy"] = round(med["receive"] / res["nt_copy_same_bytes_ms"], 2)
    res["member_calls_wall_ms"] = round(sum(med[k + "_wall"] for k in ("close", "check", "append", "sent")), 4)
    res["replaced_readback_upload_wall_ms"] = round(med["readback_wall"], 4)
    res["replaced_fin_rst_upload_wall_ms"] = round(med["fin_rst_upload_wall"], 4)
    res["ack_histories_in_err"] = int((ack0["err"] != 0).sum())
    res["ack_member0"] = {k: int(ack0[k][0]) for k in ("fresh", "old", "out_of_window", "largest_in_order")}
    res["stream_windows_in_err"] = int((rx_states["err"] != 0).sum())
    res["stream_window_bytes"] = window
    res["note"] = ("ms = median over reps of the summed kernel durations of one call; wall = elapsed between events "
                   "around the call, launch gaps included; nt copy = libugoprobe's nt copy (read + write) scaled to the "
                   "bytes receive reads, the copy's time taken for the bytes it reads as tools/ack_probe.py does; deliver = "
                   "ugo_fec_stream_set_deliver of one 32-byte segment per packet into windows that hold the batch "
                   "already, masked = on the conn_of receive passed over, the two forms taking turns to go first; "
                   "fin_rst_upload = the pinned upload of the records, segment rows and conn_of a caller wrote by hand; "
                   "replaced = a strided device-to-pinned copy of the status and flags bytes of "
                   "every packet, of two words per member, and the pinned upload of may_ack_only, synchronised; the "
                   "host loop over them is not timed")
    print(json.dumps(res), flush=True)
    for x in (rset, aset, tset, sset):
        x.close()
    for x in rxs + acks + txs + sents:
        x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--packets", type=int, default=851968)
    ap.add_argument("--conns", default="1,1024,16384")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    enc = fec.New(10, 3)
    for nconn in [int(c) for c in args.conns.split(",")]:
        run(enc, nconn, args.packets, args.reps, args.label)
    enc.close()


if __name__ == "__main__":
    main()
