#!/usr/bin/env python3
"""The connection table on the device (ugo_fec_listen_*) on the
README's ring: 851,968 datagrams in 1,488-byte slots, spread over 1, 1,024 and
16,384 known connections (v4 and v6 names alternating).  Not product code.

Per number of connections:
  route          the ring of known connections (nothing to accept)
  route_accept   the same ring in which 1,024 new connections send their INIT
                 and two packets after it (the table is remapped back between
                 repetitions, untimed)
  names          ugo_fec_listen_names for 851,968 planned packets
  remap          an identity remap of the members (with 16,384 connections: the
                 remap of 16,384 members)
Timed: the summed kernel durations of a call (the launch-timing ABI) and the
elapsed time between two events around it, launch gaps included; median of the
repetitions.  Every output of the first repetition is compared with the
RuleListener of tests/listen_ref.py (which sees the first 32 bytes of a slot).

Comparators, in the same run:
  nt copy        libugoprobe's nt copy scaled to the bytes route reads and
                 writes (names, lens, conn_of twice -- it is the call's scratch
                 -- and cls)
  connOf upload  the pinned upload of conn_of (npackets x 4 B) the call replaces
  host loop      one core walking the same names through a string-keyed hash
                 map: a Python dict keyed by the name row's address bytes.  A
                 stand-in for what INTEGRATION.md asked of the caller, not the
                 Go reference.

  python3 tools/listen_probe.py [--reps 8] [--packets 851968] [--conns 1,1024,16384] [--label TEXT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (probe_nt_copy_ms)
import listen_ref as lr  # noqa: E402
from ugo_amd import fec  # noqa: E402

SLOT, WIRE, NEW = 1488, 1446, 1024


def timed(enc, call, n_launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    enc.timing_begin(n_launches)
    e0.record()
    call()
    e1.record()
    recs, untimed = enc.timing_end()
    torch.cuda.synchronize()
    assert untimed == 0 and len(recs) == n_launches and (recs["kernel"] == fec.KERNEL_IDS["listen"]).all(), recs
    return float(recs["ms"].sum()), float(e0.elapsed_time(e1))


def key_rows(rng, n, first):
    rows = np.zeros((n, 32), np.uint8)
    for k in range(n):
        port = 1024 + (first + k) % 60000
        if k % 2:
            row = lr.name_v6(bytes([0x20, 1]) + bytes(rng.integers(0, 256, 10, dtype=np.uint8)) +
                             int(first + k).to_bytes(4, "big"), port, flowinfo=int(rng.integers(0, 1 << 20)))
        else:
            row = lr.name_v4(int(0x0a000000 + first + k).to_bytes(4, "big"), port)
        rows[k] = np.frombuffer(row, np.uint8)
    return rows


def verify(rule, names, head, lens, got):
    """The call's outputs against the rule; head = the first 32 bytes of every slot."""
    conn_of, cls, acc, n_acc = got
    w_conn, w_cls, w_acc = rule.route(names, head, np.where(lens == 22, 22, 23), 32)
    ok = np.array_equal(conn_of.cpu().numpy().view(np.uint32), np.asarray(w_conn, np.uint32))
    ok = ok and np.array_equal(cls.cpu().numpy(), np.asarray(w_cls, np.uint8)) and int(n_acc.item()) == len(w_acc)
    rows = acc.cpu().numpy()[:len(w_acc)].view(fec.LISTEN_ACCEPT_DTYPE).reshape(-1)
    ok = ok and rows["packet"].tolist() == [a[0] for a in w_acc] and rows["member"].tolist() == [a[1] for a in w_acc]
    ok = ok and rows["client_id"].tolist() == [a[2] for a in w_acc]
    return bool(ok and rows["name"].tobytes() == b"".join(a[3] for a in w_acc))


def run(enc, nconn, npk, reps, label):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(nconn)
    table = fec.ListenTable(enc, nconn + NEW)
    rule = lr.RuleListener(nconn + NEW)
    known, fresh = key_rows(rng, nconn, 0), key_rows(rng, NEW, 1 << 20)
    # the connections of the ring, accepted before anything is timed
    head0 = np.zeros((nconn, 32), np.uint8)
    head0[:, :22] = np.frombuffer(lr.init_packet(7), np.uint8)
    pk0 = torch.zeros((nconn, SLOT), dtype=torch.uint8, device=dev)
    pk0[:, :32] = torch.from_numpy(head0).to(dev)
    l0 = np.full(nconn, 22, np.uint16)
    ok = verify(rule, known, head0, l0, table.route(torch.from_numpy(known).to(dev), pk0,
                                                    torch.from_numpy(l0.view(np.int16)).to(dev)))
    del pk0
    # the ring
    who = np.arange(npk) % nconn
    names_np = known[who]
    lens_np = np.full(npk, WIRE, np.uint16)
    head = rng.integers(0, 256, (npk, 32), dtype=np.uint8)
    pkts = torch.zeros((npk, SLOT), dtype=torch.uint8, device=dev)
    pkts[:, :32] = torch.from_numpy(head).to(dev)
    names, lens = torch.from_numpy(names_np).to(dev), torch.from_numpy(lens_np.view(np.int16)).to(dev)
    # the ring with NEW connections arriving: INIT, then two packets, at places spread over the ring
    at = np.sort(rng.choice(npk // 3, NEW, replace=False)) * 3
    names2_np, lens2_np, head2 = names_np.copy(), lens_np.copy(), head.copy()
    for k, i in enumerate(at):
        names2_np[i:i + 3] = fresh[k]
        head2[i, :22] = np.frombuffer(lr.init_packet(int(i)), np.uint8)
        lens2_np[i] = 22
    pkts2 = pkts.clone()
    pkts2[:, :32] = torch.from_numpy(head2).to(dev)
    names2, lens2 = torch.from_numpy(names2_np).to(dev), torch.from_numpy(lens2_np.view(np.int16)).to(dev)
    conn_of = torch.zeros(npk, dtype=torch.int32, device=dev)
    cls = torch.zeros(npk, dtype=torch.uint8, device=dev)
    acc = torch.zeros((NEW, 48), dtype=torch.uint8, device=dev)
    n_acc = torch.zeros(1, dtype=torch.int32, device=dev)
    names_out = torch.zeros((npk, 32), dtype=torch.uint8, device=dev)
    name_lens = torch.zeros(npk, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    planned = torch.from_numpy(who.astype(np.int32)).to(dev)
    back = torch.from_numpy(np.concatenate([np.arange(nconn), np.full(NEW, lr.NO_CONN)]).astype(np.uint32)
                            .view(np.int32)).to(dev)
    same = torch.arange(nconn, dtype=torch.int32, device=dev)
    pin_conn = torch.zeros(npk, dtype=torch.int32).pin_memory()
    out = dict(conn_of=conn_of, cls=cls, accepted=acc, n_accepted=n_acc)
    t = {k: [] for k in ("route", "route_wall", "route_accept", "route_accept_wall", "names", "names_wall", "remap",
                         "remap_wall", "upload_wall")}
    for r in range(reps + 2):                                   # two warm-up rounds, the first one verified
        res = {"route": timed(enc, lambda: table.route(names, pkts, lens, **out), 4)}
        if r == 0:
            ok = ok and verify(rule, names_np, head, lens_np, (conn_of, cls, acc, n_acc))
        res["route_accept"] = timed(enc, lambda: table.route(names2, pkts2, lens2, **out), 4)
        if r == 0:
            ok = ok and verify(rule, names2_np, head2, lens2_np, (conn_of, cls, acc, n_acc))
            ok = ok and int(n_acc.item()) == NEW
        res["names"] = timed(enc, lambda: table.names(planned, names_out=names_out, name_lens=name_lens), 1)
        if r == 0:
            w_rows, w_lens = rule.names(who[:65536].tolist())
            ok = ok and names_out[:65536].cpu().numpy().tobytes() == b"".join(w_rows)
            ok = ok and name_lens[:65536].cpu().numpy().tolist() == w_lens
            ok = ok and bool((names_out.view(-1, nconn, 32) == names_out[:nconn]).all().item()) if npk % nconn == 0 \
                else ok
        table.remap(back, nconn, status=status)                 # the NEW connections close again
        if r == 0:
            ok = ok and rule.remap(list(range(nconn)) + [lr.NO_CONN] * NEW, nconn) == 0 and int(status.item()) == 0
        res["remap"] = timed(enc, lambda: table.remap(same, nconn, status=status), 4)
        if r == 0:
            ok = ok and rule.remap(list(range(nconn)), nconn) == 0 and int(status.item()) == 0
            st = table.state()
            ok = ok and (int(st["nconn"]), int(st["n_dead"]), int(st["err"])) == (rule.nconn, 0, 0)
            ok = ok and st["counts"].tolist() == rule.counts
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        conn_of.copy_(pin_conn, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            for k, (ms, wall) in res.items():
                t[k].append(ms)
                t[k + "_wall"].append(wall)
            t["upload_wall"].append(float(e0.elapsed_time(e1)))
    # one core, a string-keyed hash map: what the caller did per datagram
    book = {bytes(row[:28]): m for m, row in enumerate(known)}
    h0 = time.perf_counter()
    host_conn = [book.get(bytes(row[:28]), lr.NO_CONN) for row in names_np]
    host_ms = (time.perf_counter() - h0) * 1e3
    ok = ok and host_conn[:4096] == (who[:4096] if nconn > 1 else [0] * 4096).tolist() if nconn > 1 else ok
    stream = torch.cuda.current_stream()
    moved = npk * (32 + 2 + 4 + 4 + 1)
    cb = npk * 32
    copy_ms = bench.probe_nt_copy_ms([names.data_ptr()], [names_out.data_ptr()], cb, reps, stream.cuda_stream)
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"probe": "listen", "label": label, "connections": nconn, "packets": npk, "slot": SLOT, "new": NEW,
           "n_slots": int(table.state()["n_slots"]), "reps": reps, "verify_every_output_of_the_first_repetition": bool(ok)}
    for k in ("route", "route_accept", "names", "remap"):
        res[k + "_ms"] = round(med[k], 4)
        res[k + "_wall_ms"] = round(med[k + "_wall"], 4)
        res[k + "_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
    res["route_bytes"] = moved
    res["nt_copy_same_bytes_ms"] = round(copy_ms * moved / (2 * cb), 4)
    res["conn_of_upload_wall_ms"] = round(med["upload_wall"], 4)
    res["host_dict_loop_ms"] = round(host_ms, 1)
    res["route_over_nt_copy"] = round(med["route"] / res["nt_copy_same_bytes_ms"], 2)
    res["route_wall_over_upload"] = round(med["route_wall"] / med["upload_wall"], 2)
    res["host_loop_over_route_wall"] = round(host_ms / med["route_wall"], 1)
    res["note"] = ("ms = median over reps of the summed kernel durations of one call; wall = elapsed between events "
                   "around the call, launch gaps included; nt copy = libugoprobe's nt copy (read + write) scaled to the "
                   "bytes route reads and writes, slot lookups not counted; host_dict_loop = one pass of one core over "
                   "the names through a Python dict, a stand-in for the caller's map lookup, not the Go reference")
    print(json.dumps(res), flush=True)
    table.close()


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
