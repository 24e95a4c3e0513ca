#!/usr/bin/env python3
"""The sent histories (ugo_fec_sent_set_*) on the README's
workload: 851,968 planned and 851,968 decoded packets of 1, 1,024 and 16,384
connections, interleaved packet by packet.  Not product code.

Per repetition every connection sends consecutive numbers (one segment each)
and gets one SACK back, on its last decoded packet, for all but the last
number: 5 % of the numbers are
missing in it (the highest MAX_RANGES - 1 runs and {lio, lio}, as
ugo_fec_ack_set_attach writes a truncated SACK), and 1 % of the connections get
that SACK a second time.  This is the leg "one SACK per connection per batch",
what this project's own attach produces.  The second leg (run_every) is a
reference peer: every arriving packet carries a SACK with up to four rows, 1 %
of them the SACK of the arrival before; it is verified against a numpy
difference-array model of THE RULE (every_packet_model, itself checked against
RuleSent at small sizes) and times record, ack and drain.  Before a repetition (not timed) one ACK for everything
clears the histories, so every repetition does the same work.

Timed, per connection count, in one process: record, ack, rto, drain, attach --
sums of the calls' kernel durations (the launch-timing ABI) and the elapsed
time between two events around the call, launch gaps included.  Beside them an
nt copy of the bytes record reads, and the pinned D2H of what the host needed
when it kept this state itself: decoded info, planned info, segs and wire_lens
(the range rows left out, since the host needed only the rows of the packets
that carry a SACK, and with the whole ranges array: both are reported).

In the first repetition every record, event row and drained entry is compared
with one RuleSent (tests/sent_ref.py) per member.  Prints one JSON line per
connection count.

  python3 tools/sent_probe.py [--reps 8] [--packets 851968] [--conns 1,1024,16384] [--label TEXT]
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
import sent_ref as sr  # noqa: E402
from ugo_amd import fec  # noqa: E402

MAX_RANGES, WIRE = 32, 1446


def timed(enc, call, n_launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    enc.timing_begin(n_launches)
    e0.record()
    call()
    e1.record()
    recs, untimed = enc.timing_end()
    torch.cuda.synchronize()
    assert untimed == 0 and len(recs) == n_launches and (recs["kernel"] == fec.KERNEL_IDS["sent"]).all(), recs
    return float(recs["ms"].sum()), float(e0.elapsed_time(e1))


def sack_rows(per_pk, missing):
    """(lio, rows) relative to the repetition's base for one connection that
    lacks the numbers in `missing` (sorted, none of them per_pk)."""
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


def run(enc, nconn, npk, reps, label, stream):
    dev = torch.device("cuda", 0)
    per_pk = npk // nconn
    assert per_pk * nconn == npk
    ws = max(fec.SENT_MIN_WINDOW, 1 << (per_pk - 1).bit_length())
    txs = [fec.SentTx(enc, ws, 1) for _ in range(nconn)]
    sset = fec.SentTxSet(enc, txs)
    rules = [sr.RuleSent(ws, 1) for _ in range(nconn)]
    rng = np.random.default_rng(nconn)
    conn_np = (np.arange(npk, dtype=np.int64) % nconn).astype(np.int32)      # packet i: arrival i // nconn of i % nconn
    rel = (np.arange(npk, dtype=np.uint64) // np.uint64(nconn)) + np.uint64(1)
    top = per_pk - 1                   # the SACK's largest_acked: the last number is still on its way
    assert top >= 2
    missing = [np.sort(rng.choice(np.arange(1, top), int(0.05 * top), replace=False)) for _ in range(nconn)]
    sacks = [sack_rows(top, m) for m in missing]
    repeated = rng.choice(nconn, max(1, nconn // 100), replace=False) if nconn > 1 else np.array([0])
    # the planned batch
    pinfo_np = np.zeros(npk, fec.PKT_INFO_DTYPE)
    pinfo_np["n_segments"], pinfo_np["flags"] = 1, 0x20
    segs_np = np.zeros((npk, 1), fec.PKT_SEGMENT_DTYPE)
    segs_np["len"] = 1400
    lens = torch.full((npk,), WIRE, dtype=torch.int16, device=dev)
    status = torch.zeros(npk, dtype=torch.uint8, device=dev)
    conn_of = torch.from_numpy(conn_np).to(dev)
    pinfo = torch.zeros((npk, 64), dtype=torch.uint8, device=dev)
    psegs = torch.zeros((npk, 1, 16), dtype=torch.uint8, device=dev)
    # the decoded batch: data packets, the SACK on each connection's last one
    dinfo_np = np.zeros(npk, fec.PKT_INFO_DTYPE)
    dinfo_np["flags"], dinfo_np["n_segments"] = 0x20, 1
    dranges_np = np.zeros((npk, MAX_RANGES, 2), np.uint64)
    dinfo = torch.zeros((npk, 64), dtype=torch.uint8, device=dev)
    dranges = torch.zeros((npk, MAX_RANGES, 2), dtype=torch.int64, device=dev)
    events = torch.zeros((nconn, 64), dtype=torch.uint8, device=dev)
    delays = torch.zeros(nconn, dtype=torch.int64, device=dev)
    fired = torch.zeros(nconn, dtype=torch.uint8, device=dev)
    drain_out = (torch.zeros(npk, dtype=torch.int32, device=dev), torch.zeros(npk, dtype=torch.int64, device=dev),
                 torch.zeros(npk, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                 torch.zeros(nconn, dtype=torch.uint8, device=dev), torch.zeros(nconn, dtype=torch.int64, device=dev))
    first = torch.arange(nconn, dtype=torch.int64, device=dev)
    counts = torch.ones(nconn, dtype=torch.int32, device=dev)
    attached = torch.zeros(nconn, dtype=torch.uint8, device=dev)
    plan_info = torch.zeros((nconn, 64), dtype=torch.uint8, device=dev)
    pin = [torch.zeros(n, dtype=torch.uint8).pin_memory() for n in (npk * 64, npk * 64, npk * 16, npk * 2)]
    pin_ranges = torch.zeros(npk * MAX_RANGES * 16, dtype=torch.uint8).pin_memory()
    clear_info = torch.zeros((nconn, 64), dtype=torch.uint8, device=dev)
    clear_conn = torch.arange(nconn, dtype=torch.int32, device=dev)
    clear_ranges = torch.zeros((nconn, 0, 2), dtype=torch.int64, device=dev)
    names = ("record", "ack", "rto", "drain", "attach")
    t = {k: [] for n in names for k in (n, n + "_wall")}
    t["d2h_wall"], t["d2h_ranges_wall"] = [], []
    verified = None
    w = 0
    for r in range(reps + 2):                                   # two warm-up rounds, the first one verified
        base = r * per_pk
        now = 1_000_000 * (r + 1)
        if r:                                                   # everything of the last repetition is acknowledged
            ci = np.zeros(nconn, fec.PKT_INFO_DTYPE)
            ci["flags"], ci["largest_acked"], ci["largest_in_order"] = 0x80, base, base
            clear_info.copy_(torch.from_numpy(ci.view(np.uint8).reshape(nconn, 64)))
            sset.ack(clear_info, clear_ranges, clear_conn, now - 10, events=events)
            sset.drain(npk, out=drain_out)
        pinfo_np["packet_number"] = rel + np.uint64(base)
        segs_np["offset"][:, 0] = (rel + np.uint64(base)) * np.uint64(1400)
        pinfo.copy_(torch.from_numpy(pinfo_np.view(np.uint8).reshape(npk, 64)))
        psegs.copy_(torch.from_numpy(segs_np.view(np.uint8).reshape(npk, 1, 16)))
        dinfo_np["flags"], dinfo_np["n_ranges"] = 0x20, 0
        dinfo_np["packet_number"] = rel + np.uint64(base)
        model = [[] for _ in range(nconn)]
        slots = [(c, npk - nconn + c) for c in range(nconn)] + [(int(c), npk - 2 * nconn + int(c) if per_pk > 1 else int(c))
                                                                for c in repeated]
        for c, i in slots:
            lio, rows = sacks[c]
            w += 1
            dinfo_np["flags"][i] = 0xA0
            dinfo_np["largest_acked"][i], dinfo_np["largest_in_order"][i] = base + top, base + lio
            dinfo_np["n_ranges"][i], dinfo_np["delay_us"][i] = len(rows), 25
            for k, (a, b) in enumerate(rows):
                dranges_np[i, k] = (a + base, b + base)
            model[c].append((i, sr.Ack(base + top, base + lio, [(a + base, b + base) for a, b in rows],
                                       int(dinfo_np["packet_number"][i]), 25)))
        dinfo.copy_(torch.from_numpy(dinfo_np.view(np.uint8).reshape(npk, 64)))
        dranges.copy_(torch.from_numpy(dranges_np.view(np.int64)))
        res = {}
        res["record"] = timed(enc, lambda: sset.record(pinfo, psegs, conn_of, lens, status, now), 5)
        res["ack"] = timed(enc, lambda: sset.ack(dinfo, dranges, conn_of, now + 500, events=events), 5)
        res["rto"] = timed(enc, lambda: sset.rto(delays, now + 1000, fired=fired), 1)
        res["drain"] = timed(enc, lambda: sset.drain(npk, out=drain_out), 6)
        res["attach"] = timed(enc, lambda: sset.attach(first, counts, plan_info, attached=attached), 1)
        if r == 0:
            evs = []
            for c in range(nconn):
                rules[c].record([(base + k, WIRE, 0x20, 0, [((base + k) * 1400, 1400)]) for k in range(1, per_pk + 1)], now)
                evs.append(rules[c].ack([a for _, a in sorted(model[c], key=lambda x: x[0])], now + 500))
            got_ev = events.cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)
            ok = all(np.array_equal(got_ev[k].astype(np.uint64), np.array([e[k] for e in evs], np.uint64))
                     for k in sr.RuleSent.EVENT_FIELDS)
            ok = ok and sr.rto_set(rules, [0] * nconn, now + 1000) == fired.cpu().numpy().tolist()
            conn, off, ln, touch, upto = sr.drain_set(rules, npk)
            n = int(drain_out[3].item())
            ok = ok and n == len(conn) and drain_out[0][:n].cpu().numpy().tolist() == conn and \
                drain_out[1][:n].cpu().numpy().tolist() == off and drain_out[4].cpu().numpy().tolist() == touch and \
                drain_out[5].cpu().numpy().view(np.uint64).tolist() == upto
            _, att = sr.attach_set(rules, list(range(nconn)), [1] * nconn, nconn)
            ok = ok and attached.cpu().numpy().tolist() == att
            st = sset.states()
            want = [x.record_fields() for x in rules]
            ok = ok and all(np.array_equal(st[k].astype(np.uint64), np.array([x[k] for x in want], np.uint64))
                            for k in sr.RuleSent.FIELDS)
            verified = bool(ok)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pin[0].copy_(dinfo.view(-1), non_blocking=True)
        pin[1].copy_(pinfo.view(-1), non_blocking=True)
        pin[2].copy_(psegs.view(-1), non_blocking=True)
        pin[3].copy_(lens.view(torch.uint8), non_blocking=True)
        e1.record()
        pin_ranges.copy_(dranges.view(-1).view(torch.uint8), non_blocking=True)
        e2 = torch.cuda.Event(enable_timing=True)
        e2.record()
        torch.cuda.synchronize()
        if r >= 2:
            for k in names:
                t[k].append(res[k][0])
                t[k + "_wall"].append(res[k][1])
            t["d2h_wall"].append(float(e0.elapsed_time(e1)))
            t["d2h_ranges_wall"].append(float(e0.elapsed_time(e2)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    read_bytes = npk * (64 + 16 + 4 + 2 + 1)
    dst = torch.empty(npk * 64, dtype=torch.uint8, device=dev)
    cb = npk * 64 // 16 * 16
    copy_ms = bench.probe_nt_copy_ms([pinfo.data_ptr()], [dst.data_ptr()], cb, reps, stream.cuda_stream) * read_bytes / cb
    st = sset.states()
    total_wall = sum(med[k + "_wall"] for k in names)
    out = {"probe": "sent", "leg": "one SACK per connection per batch", "label": label, "connections": nconn,
           "packets": npk, "packets_per_connection": per_pk, "window_packets": ws, "max_ranges": MAX_RANGES,
           "reps": reps, "verify_records_events_drain_attach": verified, "errors": int(st["err"].sum()),
           "tracked_after": int(st["tracked"].sum()), "lost_packets": int(st["lost_packets"].sum())}
    assert out["errors"] == 0, "a member left its window: the timings would be of inert members"
    for k in names:
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_wall_ms"] = round(med[k + "_wall"], 4)
        out[k + "_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
    out.update({"five_calls_wall_ms": round(total_wall, 4), "pinned_d2h_ms": round(med["d2h_wall"], 4),
                "pinned_d2h_min_max": [round(min(t["d2h_wall"]), 4), round(max(t["d2h_wall"]), 4)],
                "pinned_d2h_bytes": npk * (64 + 64 + 16 + 2),
                "pinned_d2h_with_ranges_ms": round(med["d2h_ranges_wall"], 4),
                "pinned_d2h_with_ranges_bytes": npk * (64 + 64 + 16 + 2 + MAX_RANGES * 16), "below_read_back": bool(total_wall < med["d2h_wall"]),
                "record_read_bytes": read_bytes, "nt_copy_same_bytes_ms": round(copy_ms, 4),
                "note": "ms = median over reps of the summed kernel durations of one call; wall = elapsed between "
                        "events around the call, launch gaps included; pinned_d2h = decoded info, planned info, segs "
                        "and wire_lens copied to pinned host memory, event to event, range rows left out; with_ranges = the same "
                        "with the decoded batch's whole ranges array, the quantity as the issue of this probe states it"})
    print(json.dumps(out), flush=True)
    sset.close()
    for x in txs:
        x.close()


def every_packet_model(per_pk, miss, again):
    """The second leg for one connection, relative numbers 1 .. per_pk all in
    flight, lio 0: arrival j (if j is not missing) carries the SACK of a
    reference peer -- la = j, lio_a = miss[0] - 1, the three highest runs below
    la and {lio_a, lio_a} -- and every ACK is accepted; an arrival in `again`
    repeats the SACK of the arrival before it instead (not accepted: the same la).  A numpy difference
    array gives acked(n) and nacks(n).  Returns (la, lio_a, rows [per_pk, 4, 2],
    n_rows, acked bool [per_pk + 1], lost bool [per_pk + 1])."""
    j = np.arange(1, per_pk + 1, dtype=np.int64)
    arrives = np.ones(per_pk + 1, bool)
    arrives[miss] = False
    lio_a = int(miss[0]) - 1
    i = np.searchsorted(miss, j, side="right")            # missing numbers <= j
    rows = np.zeros((per_pk, 4, 2), np.int64)
    n_rows = np.zeros(per_pk, np.int64)
    m = np.concatenate([[0], miss])                       # m[i] = the i-th missing number, m[0] a floor
    has = (i > 0) & arrives[1:]
    top_f = m[i] + 1                                      # run 0: (m_i, j]
    rows[:, 0, 0], rows[:, 0, 1] = top_f, j
    k = np.ones(per_pk, np.int64)
    for r in (1, 2):                                      # run r: (m_{i-r}, m_{i-r+1})
        ok = has & (i - r >= 1)
        f = m[np.maximum(i - r, 0)] + 1
        l = m[np.maximum(i - r + 1, 0)] - 1
        at = np.flatnonzero(ok)
        rows[at, k[at], 0], rows[at, k[at], 1] = f[at], l[at]
        k[at] += 1
    at = np.flatnonzero(has)
    rows[at, k[at], 0] = rows[at, k[at], 1] = lio_a
    n_rows[at] = k[at] + 1                                # i == 0: no rows, everything up to j acknowledged
    # the difference array over 1 .. per_pk of the accepted ACKs (every arriving j: distinct la)
    d_ack = np.zeros(per_pk + 2, np.int64)
    d_le = np.zeros(per_pk + 2, np.int64)
    acc = np.flatnonzero(arrives[1:] & ~again[1:]) + 1
    np.add.at(d_le, 1, len(acc))
    np.add.at(d_le, acc + 1, -1)                          # ACK la covers n <= la
    plain = acc[i[acc - 1] == 0]
    np.add.at(d_ack, 1, len(plain))
    np.add.at(d_ack, plain + 1, -1)
    ranged = acc[i[acc - 1] > 0]
    np.add.at(d_ack, 1, len(ranged))                      # the part n <= lio_a
    np.add.at(d_ack, lio_a + 1, -len(ranged))
    for r in range(3):
        sel = ranged[n_rows[ranged - 1] - 1 > r]
        np.add.at(d_ack, rows[sel - 1, r, 0], 1)
        np.add.at(d_ack, rows[sel - 1, r, 1] + 1, -1)
    cnt_ack, cnt_le = np.cumsum(d_ack)[:per_pk + 1], np.cumsum(d_le)[:per_pk + 1]
    lam = int(acc.max())
    n = np.arange(per_pk + 1)
    acked = (cnt_ack > 0) & (n >= 1) & (n <= lam)
    lost = ~acked & (cnt_le - cnt_ack > 3) & (n >= 1) & (n <= lam)
    return lio_a, rows, n_rows, arrives, acked, lost, lam


def run_every(enc, nconn, npk, reps, label):
    """The leg of a reference peer: a SACK with up to four rows on every packet."""
    dev = torch.device("cuda", 0)
    per_pk = npk // nconn
    ws = max(fec.SENT_MIN_WINDOW, 1 << (per_pk - 1).bit_length())
    rng = np.random.default_rng(7 + nconn)
    cand = np.arange(3, per_pk - 1, 2)                    # never adjacent, never the first two or the last
    miss = np.sort(rng.choice(cand, max(1, int(0.05 * per_pk)), replace=False))
    again1 = np.zeros(per_pk + 1, bool)                   # 1 % of the arrivals repeat the SACK before them
    pick = rng.choice(np.arange(2, per_pk + 1), max(1, per_pk // 100), replace=False)
    again1[pick] = True
    gone = np.zeros(per_pk + 2, bool)
    gone[miss] = True
    again1[1:] &= ~gone[1:per_pk + 1] & ~gone[0:per_pk] & ~np.concatenate([[False], again1[1:per_pk]])
    lio_a, rows, n_rows, arrives, acked, lost, lam = every_packet_model(per_pk, miss, again1)
    txs = [fec.SentTx(enc, ws, 1) for _ in range(nconn)]
    sset = fec.SentTxSet(enc, txs)
    conn_np = (np.arange(npk, dtype=np.int64) % nconn).astype(np.int32)
    rel = (np.arange(npk, dtype=np.int64) // nconn) + 1  # packet i is arrival rel[i] of connection i % nconn
    pinfo_np = np.zeros(npk, fec.PKT_INFO_DTYPE)
    pinfo_np["n_segments"], pinfo_np["flags"] = 1, 0x20
    segs_np = np.zeros((npk, 1), fec.PKT_SEGMENT_DTYPE)
    segs_np["len"] = 1400
    dinfo_np = np.zeros(npk, fec.PKT_INFO_DTYPE)
    dinfo_np["n_segments"] = 1
    rep_of = rel - again1[rel]                            # the arrival whose SACK packet i carries
    dinfo_np["status"] = np.where(arrives[rel], 0, 1)     # a missing number does not arrive
    dinfo_np["flags"] = 0xA0
    dinfo_np["n_ranges"] = n_rows[rep_of - 1]
    rows_rel = rows[rep_of - 1]
    lens = torch.full((npk,), WIRE, dtype=torch.int16, device=dev)
    status = torch.zeros(npk, dtype=torch.uint8, device=dev)
    conn_of = torch.from_numpy(conn_np).to(dev)
    pinfo = torch.zeros((npk, 64), dtype=torch.uint8, device=dev)
    psegs = torch.zeros((npk, 1, 16), dtype=torch.uint8, device=dev)
    dinfo = torch.zeros((npk, 64), dtype=torch.uint8, device=dev)
    dranges = torch.zeros((npk, 4, 2), dtype=torch.int64, device=dev)
    events = torch.zeros((nconn, 64), dtype=torch.uint8, device=dev)
    drain_out = (torch.zeros(npk, dtype=torch.int32, device=dev), torch.zeros(npk, dtype=torch.int64, device=dev),
                 torch.zeros(npk, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                 torch.zeros(nconn, dtype=torch.uint8, device=dev), torch.zeros(nconn, dtype=torch.int64, device=dev))
    clear_info = torch.zeros((nconn, 64), dtype=torch.uint8, device=dev)
    clear_conn = torch.arange(nconn, dtype=torch.int32, device=dev)
    clear_ranges = torch.zeros((nconn, 0, 2), dtype=torch.int64, device=dev)
    names = ("record", "ack", "drain")
    t = {k: [] for nme in names for k in (nme, nme + "_wall")}
    verified = None
    for r in range(reps + 2):
        base = r * per_pk
        now = 1_000_000 * (r + 1)
        if r:
            ci = np.zeros(nconn, fec.PKT_INFO_DTYPE)
            ci["flags"], ci["largest_acked"], ci["largest_in_order"] = 0x80, base, base
            clear_info.copy_(torch.from_numpy(ci.view(np.uint8).reshape(nconn, 64)))
            sset.ack(clear_info, clear_ranges, clear_conn, now - 10, events=events)
            sset.drain(npk, out=drain_out)
        pinfo_np["packet_number"] = (rel + base).astype(np.uint64)
        segs_np["offset"][:, 0] = ((rel + base) * 1400).astype(np.uint64)
        pinfo.copy_(torch.from_numpy(pinfo_np.view(np.uint8).reshape(npk, 64)))
        psegs.copy_(torch.from_numpy(segs_np.view(np.uint8).reshape(npk, 1, 16)))
        dinfo_np["packet_number"] = (rel + base).astype(np.uint64)
        dinfo_np["largest_acked"] = (rep_of + base).astype(np.uint64)
        dinfo_np["largest_in_order"] = np.where(n_rows[rep_of - 1] > 0, lio_a + base, rep_of + base).astype(np.uint64)
        dinfo.copy_(torch.from_numpy(dinfo_np.view(np.uint8).reshape(npk, 64)))
        dranges.copy_(torch.from_numpy(rows_rel + base))
        res = {}
        res["record"] = timed(enc, lambda: sset.record(pinfo, psegs, conn_of, lens, status, now), 5)
        res["ack"] = timed(enc, lambda: sset.ack(dinfo, dranges, conn_of, now + 500, events=events), 5)
        res["drain"] = timed(enc, lambda: sset.drain(npk, out=drain_out), 6)
        if r == 0:                                        # every member against the model
            ev = events.cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)
            n_ack, n_lost = int(acked.sum()), int(lost.sum())
            left = per_pk - n_ack - n_lost
            ok = bool((ev["acked_packets"] == n_ack).all() and (ev["lost_packets"] == n_lost).all() and
                      (ev["acked_bytes"] == n_ack * WIRE).all() and (ev["bytes_in_flight"] == left * WIRE).all() and
                      (ev["largest_acked"] == lam).all() and (ev["accepted"] == 1).all())
            st = sset.states()
            still = ~acked & ~lost
            still[0] = False
            flying = np.flatnonzero(still)
            want_lio = int(flying[0]) - 1 if len(flying) else per_pk
            ok = ok and bool((st["tracked"] == left).all() and (st["queued"] == 0).all() and
                             (st["lio"] == want_lio).all() and (st["lost_packets"] == n_lost).all() and
                             not st["err"].any())
            n_e = int(drain_out[3].item())
            lost_off = np.flatnonzero(lost) * 1400
            got_c = drain_out[0][:n_e].cpu().numpy()
            got_o = drain_out[1][:n_e].cpu().numpy()
            ok = ok and n_e == n_lost * nconn and np.array_equal(got_c, np.repeat(np.arange(nconn), n_lost)) and \
                np.array_equal(got_o, np.tile(lost_off, nconn))
            want_upto = int(flying[0]) * 1400 if len(flying) else (1 << 64) - 1
            ok = ok and bool((drain_out[5].cpu().numpy().view(np.uint64) == np.uint64(want_upto)).all())
            verified = bool(ok)
        if r >= 2:
            for k in names:
                t[k].append(res[k][0])
                t[k + "_wall"].append(res[k][1])
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"probe": "sent", "leg": "a SACK with up to four rows on every packet", "label": label,
           "connections": nconn, "packets": npk, "packets_per_connection": per_pk, "window_packets": ws,
           "max_ranges": 4, "reps": reps, "verify_events_records_drain_against_numpy_model": verified,
           "accepted_acks_per_connection": int((arrives[1:] & ~again1[1:]).sum()), "acked_per_connection": int(acked.sum()),
           "lost_per_connection": int(lost.sum())}
    for k in names:
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_wall_ms"] = round(med[k + "_wall"], 4)
        out[k + "_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
    print(json.dumps(out), flush=True)
    sset.close()
    for x in txs:
        x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--packets", type=int, default=851968)
    ap.add_argument("--conns", default="1,1024,16384")
    ap.add_argument("--label", default="")
    ap.add_argument("--leg", default="both", choices=("one", "every", "both"))
    args = ap.parse_args()
    stream = torch.cuda.current_stream(torch.device("cuda", 0))
    enc = fec.New(10, 3)
    for nconn in [int(c) for c in args.conns.split(",")]:
        if args.leg in ("one", "both"):
            run(enc, nconn, args.packets, args.reps, args.label, stream)
        if args.leg in ("every", "both"):
            run_every(enc, nconn, args.packets, args.reps, args.label)
    enc.close()


if __name__ == "__main__":
    main()
