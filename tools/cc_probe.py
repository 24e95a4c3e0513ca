#!/usr/bin/env python3
"""Congestion control on the device (ugo_fec_cc_*) on the
README's workload: 851,968 planned and 851,968 decoded packets of 1, 1,024 and
16,384 connections, one SACK per connection per batch with 5 % of the numbers
missing, as tools/sent_probe.py builds it.  Not product code.

Two identical sets of sent histories record the same batch in every
repetition; one is acknowledged through ugo_fec_sent_set_ack, the other through
ugo_fec_cc_sent_ack, so the two are timed beside each other on the same state.
Then ugo_fec_cc_set_ack, ugo_fec_sent_set_rto and ugo_fec_cc_set_rto on the
second.  Timed: the summed kernel durations of a call (the launch-timing ABI)
and the elapsed time between two events around it, launch gaps included.
Beside them what the two controller calls replace: the event rows copied to
pinned host memory and budget and delay_us uploaded from it, event to event,
and the same with the host's wait in between by the host's clock.

In the first repetition the event rows of the two sets are compared, the rows
with what the events say, and every controller record with a RuleCc
(tests/cc_ref.py) fed the same rows.

--plain-only times ugo_fec_sent_set_ack alone; with --tree DIR the package is
imported from a checkout of another commit built there (the parent), so that
its set_ack is timed by the same script on the same machine.

  python3 tools/cc_probe.py [--reps 8] [--packets 851968] [--conns 1,1024,16384] [--label TEXT]
                            [--plain-only] [--tree DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_RANGES, WIRE = 32, 1446


def sack_rows(per_pk, missing):
    """(lio, rows) for one connection that lacks the numbers in `missing`: the
    highest MAX_RANGES - 1 runs and {lio, lio} (tools/sent_probe.py)."""
    have = np.ones(per_pk + 2, bool)
    have[0] = have[per_pk + 1] = False
    have[missing] = False
    lio = int(missing[0]) - 1 if len(missing) else per_pk
    starts = np.flatnonzero(have[1:] & ~have[:-1]) + 1
    ends = np.flatnonzero(have[:-1] & ~have[1:])
    runs = [(int(a), int(b)) for a, b in zip(starts, ends) if a > lio][::-1]
    if not runs:
        return lio, []
    return lio, runs[:MAX_RANGES - 1] + [(lio, lio)]


def timed(enc, call, n_launches, kernel):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    enc.timing_begin(n_launches)
    e0.record()
    call()
    e1.record()
    recs, untimed = enc.timing_end()
    torch.cuda.synchronize()
    assert untimed == 0 and len(recs) == n_launches and (recs["kernel"] == kernel).all(), recs
    return float(recs["ms"].sum()), float(e0.elapsed_time(e1))


def run(fec, cr, enc, nconn, npk, reps, label, plain_only):
    dev = torch.device("cuda", 0)
    per_pk = npk // nconn
    assert per_pk * nconn == npk and per_pk >= 3
    ws = max(fec.SENT_MIN_WINDOW, 1 << (per_pk - 1).bit_length())
    nsets = 1 if plain_only else 2
    txs = [[fec.SentTx(enc, ws, 1) for _ in range(nconn)] for _ in range(nsets)]
    ssets = [fec.SentTxSet(enc, t) for t in txs]
    cc = None if plain_only else fec.CcSet(enc, ssets[1])
    rng = np.random.default_rng(nconn)
    conn_np = (np.arange(npk, dtype=np.int64) % nconn).astype(np.int32)
    rel = (np.arange(npk, dtype=np.uint64) // np.uint64(nconn)) + np.uint64(1)
    top = per_pk - 1
    sacks = [sack_rows(top, np.sort(rng.choice(np.arange(1, top), int(0.05 * top), replace=False)))
             for _ in range(nconn)]
    pinfo_np = np.zeros(npk, fec.PKT_INFO_DTYPE)
    pinfo_np["n_segments"], pinfo_np["flags"] = 1, 0x20
    segs_np = np.zeros((npk, 1), fec.PKT_SEGMENT_DTYPE)
    segs_np["len"] = 1400
    lens = torch.full((npk,), WIRE, dtype=torch.int16, device=dev)
    status = torch.zeros(npk, dtype=torch.uint8, device=dev)
    conn_of = torch.from_numpy(conn_np).to(dev)
    pinfo = torch.zeros((npk, 64), dtype=torch.uint8, device=dev)
    psegs = torch.zeros((npk, 1, 16), dtype=torch.uint8, device=dev)
    dinfo_np = np.zeros(npk, fec.PKT_INFO_DTYPE)
    dinfo_np["n_segments"] = 1
    dranges_np = np.zeros((npk, MAX_RANGES, 2), np.uint64)
    dinfo = torch.zeros((npk, 64), dtype=torch.uint8, device=dev)
    dranges = torch.zeros((npk, MAX_RANGES, 2), dtype=torch.int64, device=dev)
    events = [torch.zeros((nconn, 64), dtype=torch.uint8, device=dev) for _ in range(nsets)]
    rows = torch.zeros((nconn, 32), dtype=torch.uint8, device=dev)
    delays = torch.zeros(nconn, dtype=torch.int64, device=dev)
    budget = torch.zeros(nconn, dtype=torch.int32, device=dev)
    fired = torch.zeros(nconn, dtype=torch.uint8, device=dev)
    drain_out = (torch.zeros(npk, dtype=torch.int32, device=dev), torch.zeros(npk, dtype=torch.int64, device=dev),
                 torch.zeros(npk, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                 torch.zeros(nconn, dtype=torch.uint8, device=dev), torch.zeros(nconn, dtype=torch.int64, device=dev))
    pin_events = torch.zeros((nconn, 64), dtype=torch.uint8).pin_memory()
    pin_budget = torch.zeros(nconn, dtype=torch.int32).pin_memory()
    pin_delay = torch.zeros(nconn, dtype=torch.int64).pin_memory()
    clear_info = torch.zeros((nconn, 64), dtype=torch.uint8, device=dev)
    clear_conn = torch.arange(nconn, dtype=torch.int32, device=dev)
    clear_ranges = torch.zeros((nconn, 0, 2), dtype=torch.int64, device=dev)
    k_sent = fec.KERNEL_IDS["sent"]
    names = ("set_ack",) if plain_only else ("set_ack", "cc_sent_ack", "cc_set_ack", "sent_set_rto", "cc_set_rto")
    t = {k: [] for n in names for k in (n, n + "_wall")}
    for k in ("d2h_events", "h2d_budget_delay", "host_step"):
        t[k + "_wall"] = []
    verified = None
    rules = None if plain_only else [cr.RuleCc() for _ in range(nconn)]
    for r in range(reps + 2):                                   # two warm-up rounds, the first one verified
        base = r * per_pk
        now = 1_000_000 * (r + 1)
        if r:                                                   # everything of the last repetition is acknowledged
            ci = np.zeros(nconn, fec.PKT_INFO_DTYPE)
            ci["flags"], ci["largest_acked"], ci["largest_in_order"] = 0x80, base, base
            clear_info.copy_(torch.from_numpy(ci.view(np.uint8).reshape(nconn, 64)))
            for s, ev in zip(ssets, events):
                s.ack(clear_info, clear_ranges, clear_conn, now - 10, events=ev)
                s.drain(npk, out=drain_out)
        pinfo_np["packet_number"] = rel + np.uint64(base)
        segs_np["offset"][:, 0] = (rel + np.uint64(base)) * np.uint64(1400)
        pinfo.copy_(torch.from_numpy(pinfo_np.view(np.uint8).reshape(npk, 64)))
        psegs.copy_(torch.from_numpy(segs_np.view(np.uint8).reshape(npk, 1, 16)))
        dinfo_np["flags"], dinfo_np["n_ranges"] = 0x20, 0
        dinfo_np["packet_number"] = rel + np.uint64(base)
        for c in range(nconn):
            i = npk - nconn + c                                 # the SACK rides on the connection's last packet
            lio, rws = sacks[c]
            dinfo_np["flags"][i] = 0xA0
            dinfo_np["largest_acked"][i], dinfo_np["largest_in_order"][i] = base + top, base + lio
            dinfo_np["n_ranges"][i], dinfo_np["delay_us"][i] = len(rws), 24
            for k, (a, b) in enumerate(rws):
                dranges_np[i, k] = (a + base, b + base)
        dinfo.copy_(torch.from_numpy(dinfo_np.view(np.uint8).reshape(npk, 64)))
        dranges.copy_(torch.from_numpy(dranges_np.view(np.int64)))
        for s in ssets:
            s.record(pinfo, psegs, conn_of, lens, status, now)
        res = {}
        res["set_ack"] = timed(enc, lambda: ssets[0].ack(dinfo, dranges, conn_of, now + 500, events=events[0]), 5, k_sent)
        if not plain_only:
            k_cc = fec.KERNEL_IDS["cc"]
            split = cc.cutback()
            res["cc_sent_ack"] = timed(enc, lambda: cc.sent_ack(dinfo, dranges, conn_of, now + 500, events=events[1],
                                                                 split=split, rows=rows), 5, k_cc)
            if r == 0:
                before = ssets[1].states()
            res["cc_set_ack"] = timed(enc, lambda: cc.ack(events[1], rows, now + 500, delay_us=delays), 1, k_cc)
            res["sent_set_rto"] = timed(enc, lambda: ssets[1].rto(delays, now + 1000, fired=fired), 1, k_sent)
            res["cc_set_rto"] = timed(enc, lambda: cc.rto(fired, WIRE, 64, budget=budget), 1, k_cc)
            if r == 0:
                ev0 = events[0].cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)
                ev1 = events[1].cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)
                rw = rows.cpu().numpy().view(fec.CC_ROW_DTYPE).reshape(-1)
                ok = bool(np.array_equal(ev0, ev1) and (rw["max_acked"] == base + top).all() and
                          (rw["acked_le"] == 0).all() and ((rw["max_lost"] != 0) == (ev1["lost_packets"] != 0)).all())
                after = ssets[1].states()
                f = fired.cpu().numpy()
                want_d = [x.ack(ev1[c], rw[c], now + 500, int(before["last_sent"][c]), int(before["lio"][c]), 0)
                          for c, x in enumerate(rules)]
                want_b = [x.rto(int(f[c]), int(after["last_sent"][c]), int(after["bytes_in_flight"][c]), WIRE, 64, 0)
                          for c, x in enumerate(rules)]
                st = cc.states()
                ok = ok and delays.cpu().numpy().tolist() == want_d and budget.cpu().numpy().tolist() == want_b
                ok = ok and all(np.array_equal(st[k].astype(np.uint64), np.array([x.view()[k] for x in rules], np.uint64))
                                for k in cr.RuleCc.FIELDS)
                verified = bool(ok)
        # what the controller calls replace: events to the host, budget and delay_us back
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        e[0].record()
        pin_events.copy_(events[-1], non_blocking=True)
        e[1].record()
        torch.cuda.synchronize()                                # the host reads the rows here
        e[2].record()
        budget.copy_(pin_budget, non_blocking=True)
        delays.copy_(pin_delay, non_blocking=True)
        e[3].record()
        torch.cuda.synchronize()
        h1 = time.perf_counter()
        if r >= 2:
            for k in names:
                t[k].append(res[k][0])
                t[k + "_wall"].append(res[k][1])
            t["d2h_events_wall"].append(float(e[0].elapsed_time(e[1])))
            t["h2d_budget_delay_wall"].append(float(e[2].elapsed_time(e[3])))
            t["host_step_wall"].append((h1 - h0) * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"probe": "cc", "label": label, "connections": nconn, "packets": npk, "packets_per_connection": per_pk,
           "window_packets": ws, "max_ranges": MAX_RANGES, "reps": reps, "plain_only": plain_only,
           "verify_events_rows_and_controller_records": verified,
           "errors": int(sum(int(s.states()["err"].sum()) for s in ssets))}
    assert out["errors"] == 0, "a member left its window: the timings would be of inert members"
    for k in names:
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_wall_ms"] = round(med[k + "_wall"], 4)
        out[k + "_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
    if not plain_only:
        out["cc_calls_wall_ms"] = round(med["cc_set_ack_wall"] + med["cc_set_rto_wall"], 4)
    for k in ("d2h_events", "h2d_budget_delay", "host_step"):
        out[k + "_wall_ms"] = round(med[k + "_wall"], 4)
    out["note"] = ("ms = median over reps of the summed kernel durations of one call; wall = elapsed between events "
                   "around the call, launch gaps included; d2h_events = the event rows copied to pinned host memory, "
                   "h2d_budget_delay = budget and delay_us uploaded from it, event to event; host_step = the two with "
                   "the host's wait between them, by the host's clock (no per-connection work on the host counted)")
    print(json.dumps(out), flush=True)
    if cc is not None:
        cc.close()
    for s in ssets:
        s.close()
    for tx in txs:
        for x in tx:
            x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--packets", type=int, default=851968)
    ap.add_argument("--conns", default="1,1024,16384")
    ap.add_argument("--label", default="")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose ugo_amd package is timed")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from ugo_amd import fec
    cr = None
    if not args.plain_only:
        import cc_ref as cr
    enc = fec.New(10, 3)
    for nconn in [int(c) for c in args.conns.split(",")]:
        run(fec, cr, enc, nconn, args.packets, args.reps, args.label, args.plain_only)
    enc.close()


if __name__ == "__main__":
    main()
