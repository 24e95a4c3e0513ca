#!/usr/bin/env python3
"""The receive histories (ugo_fec_ack_set_*) on the README's
workload: 851,968 decoded packets of 1, 1,024 and 16,384 connections,
interleaved packet by packet as a listener receives them.  Not product code.

Per connection the batch carries consecutive packet numbers.  5 % of them are
missing at their place; a missing number arrives 512 of the connection's
packets later (its retransmission) or, if the batch ends first, not at all.
1 % of the packets arrive twice.  The first packet of a connection carries the
stop-waiting that gives up what the batch before left open, so a repetition
starts from where the last one ended and the histories stay below the
reference's limit of 1,000 outstanding packets.

Per connection count, in one process with interleaved repetitions:
  receive   THE RULE for every member (four launches)
  attach    buildSack for every member onto a plan in which every second member
            has a packet and the others get an ACK-only record (three launches)
  plan      ugo_fec_stream_tx_set_plan for as many connections and packets: the
            launch-bound sibling
  nt copy   of the bytes receive reads (info and conn_of)
  D2H       info copied to pinned host memory: the read-back the host needed
            when it kept this state itself
Times are sums of the calls' kernel durations (hipExtLaunchKernel events, the
launch-timing ABI) and, beside them, the elapsed time between two events around
the call, launch gaps included.

After each of the first two batches (the second begins with a floor) every
record and every attached row is compared with one RuleAck (tests/ack_ref.py)
per member.  Prints one JSON line per connection count.

  python3 tools/ack_probe.py [--reps 8] [--packets 851968] [--conns 1,1024,16384] [--label TEXT]
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
import ack_ref as ar  # noqa: E402
import bench  # noqa: E402  (probe_nt_copy_ms)
from ugo_amd import fec  # noqa: E402

SEG, MAX_RANGES, LATE = 1400, 32, 512
M = SEG + fec.STREAM_TX_HEADER


def connection_numbers(rng, k):
    """k arrivals of one connection, numbers from 1: 1 % repeats, 5 % of the
    numbers late by LATE arrivals or missing.  Returns (numbers, top)."""
    dup = int(round(0.01 * k))
    out, late, n = [], {}, 0
    while len(out) < k - dup:
        at = len(out)
        if at in late:
            out.append(late.pop(at))
            continue
        n += 1
        if rng.random() < 0.05 and at + LATE not in late:       # one late arrival per place
            late[at + LATE] = n
        else:
            out.append(n)
    for _ in range(dup):
        at = int(rng.integers(0, len(out)))
        out.insert(at + 1, out[at])
    return np.asarray(out[:k], np.uint64), n


def batch(nconn, per_pk, seed):
    """(number [nconn, per_pk] relative to the repetition's base, top per connection)."""
    rng = np.random.default_rng(seed)
    nums = np.zeros((nconn, per_pk), np.uint64)
    tops = np.zeros(nconn, np.uint64)
    for c in range(nconn):
        nums[c], tops[c] = connection_numbers(rng, per_pk)
    return nums, tops


def timed(enc, call, n_launches, kernel):
    """(sum of the call's kernel durations, elapsed between events around it), ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    enc.timing_begin(n_launches)
    e0.record()
    call()
    e1.record()
    recs, untimed = enc.timing_end()
    torch.cuda.synchronize()
    assert untimed == 0 and len(recs) == n_launches and (recs["kernel"] == fec.KERNEL_IDS[kernel]).all(), recs
    return float(recs["ms"].sum()), float(e0.elapsed_time(e1))


def same_records(states, rules):
    want = [r.record() for r in rules]
    return all(np.array_equal(states[k].astype(np.uint64), np.array([w[k] for w in want], np.uint64))
               for k in ar.RuleAck.FIELDS)


def run(enc, nconn, npk, reps, label, stream):
    dev = torch.device("cuda", 0)
    per_pk = npk // nconn
    assert per_pk * nconn == npk, "packets must divide among the connections"
    nums, tops = batch(nconn, per_pk, seed=nconn)
    span = int(tops.max()) + 1                     # a repetition's numbers are base + 1 .. base + top
    wp = max(fec.ACK_MIN_WINDOW, 1 << (span - 1).bit_length())
    rxs = [fec.AckRx(enc, wp) for _ in range(nconn)]
    aset = fec.AckRxSet(enc, rxs)
    rules = [ar.RuleAck(wp) for _ in range(nconn)]
    # packet i of the batch is arrival i // nconn of connection i % nconn
    conn_np = (np.arange(npk, dtype=np.int64) % nconn).astype(np.int32)
    rel = nums.T.reshape(npk)
    info_np = np.zeros(npk, fec.PKT_INFO_DTYPE)
    info_np["n_segments"], info_np["flags"], info_np["payload_off"] = 1, 0x20, 6
    info = torch.zeros((npk, 64), dtype=torch.uint8, device=dev)
    conn_of = torch.from_numpy(conn_np).to(dev)
    # the plan attach writes onto: every second member has one packet, the others may send an ACK alone
    counts = (np.arange(nconn) % 2 == 0).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    total_n = int(counts.sum())
    max_packets = total_n + nconn
    d_first, d_count = torch.from_numpy(first).to(dev), torch.from_numpy(counts).to(dev)
    d_total = torch.tensor([total_n], dtype=torch.int64, device=dev)
    d_may = torch.ones(nconn, dtype=torch.uint8, device=dev)
    plan_info = torch.zeros((max_packets, 64), dtype=torch.uint8, device=dev)
    plan_ranges = torch.zeros((max_packets, MAX_RANGES, 2), dtype=torch.int64, device=dev)
    plan_conn = torch.zeros(max_packets, dtype=torch.int32, device=dev)
    total_out = torch.zeros(1, dtype=torch.int64, device=dev)
    attached = torch.zeros(nconn, dtype=torch.uint8, device=dev)
    # the sibling: set_plan for as many connections and packets
    per = per_pk * SEG
    cap = max(fec.STREAM_MIN_WINDOW, 1 << (per - 1).bit_length())
    txs = [fec.StreamTx(enc, cap, 4) for _ in range(nconn)]
    tset = fec.StreamTxSet(enc, txs)
    i64 = dict(dtype=torch.int64, device=dev)
    src = torch.zeros(per * nconn, dtype=torch.uint8, device=dev)
    src_off, n_bytes, n_written = torch.arange(nconn, **i64) * per, torch.full((nconn,), per, **i64), torch.zeros(nconn, **i64)
    budget = torch.full((nconn,), per_pk, dtype=torch.int32, device=dev)
    upto = torch.full((nconn,), 1 << 62, **i64)
    plan_out = (torch.zeros((npk, 64), dtype=torch.uint8, device=dev), torch.zeros((npk, 1, 16), dtype=torch.uint8, device=dev),
                torch.zeros(npk, dtype=torch.int32, device=dev), torch.zeros(nconn, **i64),
                torch.zeros(nconn, dtype=torch.int32, device=dev), torch.zeros(1, **i64))
    pinned = torch.zeros((npk, 64), dtype=torch.uint8).pin_memory()
    t = {k: [] for k in ("receive", "receive_wall", "attach", "attach_wall", "plan", "plan_wall", "d2h_wall")}
    ok_records = ok_rows = None
    for r in range(reps + 2):                      # two warm-up rounds, the first one verified
        base = r * span
        info_np["packet_number"] = rel + np.uint64(base)
        info_np["stop_waiting"] = 0
        info_np["stop_waiting"][:nconn] = base + 1  # each connection's first arrival
        info.copy_(torch.from_numpy(info_np.view(np.uint8).reshape(npk, 64)))
        now = 1000 * (r + 1)
        rc = timed(enc, lambda: aset.receive(info, conn_of, now), 4, "ack")
        if r < 2:                                  # the first batch, and the first one that begins with a floor
            for c in range(nconn):
                rules[c].receive([(int(x) + base, base + 1 if k == 0 else 0) for k, x in enumerate(nums[c])], now)
            ok = same_records(aset.states(), rules)
            ok_records = ok if ok_records is None else (ok_records and ok)
        at = timed(enc, lambda: aset.attach(now + 250, d_first, d_count, d_total, plan_info, plan_ranges, plan_conn,
                                            may_ack_only=d_may, total_out=total_out, attached=attached), 3, "ack")
        if r < 2:
            writes, want_total, want_att = ar.attach_set(rules, now + 250, first.tolist(), counts.tolist(), total_n,
                                                         [1] * nconn, max_packets, MAX_RANGES)
            iv = plan_info.cpu().numpy().reshape(-1).view(fec.PKT_INFO_DTYPE)
            rg = plan_ranges.cpu().numpy().view(np.uint64)
            pc = plan_conn.cpu().numpy()
            ok = int(total_out.item()) == want_total and attached.cpu().numpy().tolist() == want_att
            for tt, c, ack_only, la, lio, delay, nr, rows in writes:
                ok = ok and (int(iv["largest_acked"][tt]), int(iv["largest_in_order"][tt]), int(iv["delay_us"][tt]),
                             int(iv["n_ranges"][tt]), int(iv["flags"][tt]) & 0x80) == (la, lio, delay, nr, 0x80)
                ok = ok and [tuple(x) for x in rg[tt, :nr].tolist()] == rows and (not ack_only or pc[tt] == c)
            ok_rows = ok if ok_rows is None else (ok_rows and ok)
            runs = [len(w[7]) for w in writes]
        tset.write(src, src_off, n_bytes, n_written=n_written)
        pl = timed(enc, lambda: tset.plan(budget, npk, max_payload=M, max_segments=1, out=plan_out), 6, "stream_tx")
        tset.release(upto)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pinned.copy_(info, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            for k, v in (("receive", rc), ("attach", at), ("plan", pl)):
                t[k].append(v[0])
                t[k + "_wall"].append(v[1])
            t["d2h_wall"].append(float(e0.elapsed_time(e1)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    read_bytes = npk * 64 + npk * 4
    dst = torch.empty(npk * 64, dtype=torch.uint8, device=dev)
    cb = npk * 64 // 16 * 16
    copy_ms = bench.probe_nt_copy_ms([info.data_ptr()], [dst.data_ptr()], cb, reps, stream.cuda_stream) * read_bytes / cb
    st = aset.states()
    print(json.dumps({
        "probe": "ack", "label": label, "connections": nconn, "packets": npk, "packets_per_connection": per_pk,
        "window_packets": wp, "max_ranges": MAX_RANGES, "reps": reps,
        "verify_every_record": bool(ok_records), "verify_every_attached_row": bool(ok_rows),
        "ranges_per_sack_max": max(runs), "outstanding_max": int(st["outstanding"].max()), "errors": int(st["err"].sum()),
        "fresh": int(st["fresh"].sum()), "old": int(st["old"].sum()), "out_of_window": int(st["out_of_window"].sum()),
        "receive_ms": round(med["receive"], 4), "receive_wall_ms": round(med["receive_wall"], 4),
        "receive_min_max": [round(min(t["receive"]), 4), round(max(t["receive"]), 4)],
        "receive_ns_per_packet": round(med["receive"] * 1e6 / npk, 3),
        "attach_ms": round(med["attach"], 4), "attach_wall_ms": round(med["attach_wall"], 4),
        "attach_min_max": [round(min(t["attach"]), 4), round(max(t["attach"]), 4)],
        "set_plan_ms": round(med["plan"], 4), "set_plan_wall_ms": round(med["plan_wall"], 4),
        "receive_read_bytes": read_bytes, "nt_copy_same_bytes_ms": round(copy_ms, 4),
        "receive_frac_of_copy": round(copy_ms / med["receive"], 4),
        "pinned_d2h_of_info_ms": round(med["d2h_wall"], 4),
        "note": "ms = median over reps of the summed kernel durations of one call (hipExtLaunchKernel events); "
                "wall = elapsed between events around the call, launch gaps included; nt copy = libugoprobe's nt copy "
                "of info scaled to info + conn_of; pinned_d2h = info copied to pinned host memory, event to event"}),
          flush=True)
    aset.close()
    tset.close()
    for x in rxs + txs:
        x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--packets", type=int, default=851968)
    ap.add_argument("--conns", default="1,1024,16384")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    stream = torch.cuda.current_stream(torch.device("cuda", 0))
    enc = fec.New(10, 3)
    for nconn in [int(c) for c in args.conns.split(",")]:
        run(enc, nconn, args.packets, args.reps, args.label, stream)
    enc.close()


if __name__ == "__main__":
    main()
