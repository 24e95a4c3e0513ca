#!/usr/bin/env python3
"""The send windows (ugo_fec_stream_tx_set_*) on the README's
packet-encode workload: 851,968 packets with one 1400-B segment each, a quarter
with a short SACK patched in by the caller, 3-byte packet numbers, slot 1488,
FEC-framed -- planned from and encoded out of the windows of 1, 1,024 and 16,384
connections.  Not product code.

Per connection count, in one process with interleaved repetitions:
  write       the whole batch's stream bytes into the windows (two launches)
  plan        THE RULE for every member (six launches)
  set_encode  the packets out of the windows
  flat        ugo_fec_packet_encode on the identical records from one flat
              buffer (the bytes write took): the parent's entry point, the
              yardstick
  release     everything, so that the next repetition starts from empty windows
Times are sums of the calls' kernel durations (hipExtLaunchKernel events, the
launch-timing ABI); write, plan and set_encode are also given as the elapsed
time between two events around the call, launch gaps included.  An nt copy of
the same bytes (libugoprobe's, as in tools/pkt_encode_probe.py) is the ceiling
of write and of set_encode.

Every wire byte of set_encode's first batch is compared with an expectation
built on the host with numpy (pkt_encode_probe.expectation) and with the flat
encoder's output.  Prints one JSON line per connection count.

  python3 tools/stream_tx_probe.py [--reps 10] [--packets 851968] [--conns 1,1024,16384] [--label TEXT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402  (probe_nt_copy_ms)
from pkt_encode_probe import SEG, SLOT, expectation  # noqa: E402
from ugo_amd import fec  # noqa: E402

M = SEG + fec.STREAM_TX_HEADER   # max_payload: a packet of new data carries M - H bytes
PN0 = (1 << 15) - 1              # 3-byte packet numbers, as in the README's workload


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


def run(enc, nconn, npk, reps, label, src, outs, stream):
    dev = src.device
    per_pk = npk // nconn
    assert per_pk * nconn == npk, "packets must divide among the connections"
    per = per_pk * SEG
    cap = max(fec.STREAM_MIN_WINDOW, 1 << (per - 1).bit_length())
    txs = [fec.StreamTx(enc, cap, 4, 0, PN0) for _ in range(nconn)]
    tset = fec.StreamTxSet(enc, txs)
    i64 = dict(dtype=torch.int64, device=dev)
    src_off = torch.arange(nconn, **i64) * per
    n = torch.full((nconn,), per, **i64)
    n_written = torch.zeros(nconn, **i64)
    budget = torch.full((nconn,), per_pk, dtype=torch.int32, device=dev)
    upto = torch.full((nconn,), 1 << 62, **i64)
    plan_out = (torch.zeros((npk, 64), dtype=torch.uint8, device=dev),
                torch.zeros((npk, 1, 16), dtype=torch.uint8, device=dev),
                torch.zeros(npk, dtype=torch.int32, device=dev), torch.zeros(nconn, **i64),
                torch.zeros(nconn, dtype=torch.int32, device=dev), torch.zeros(1, **i64))
    info, segs, conn_of, first_packet, n_packets, total = plan_out
    ranges = torch.zeros((npk, 1, 2), dtype=torch.int64, device=dev)
    rng = np.random.default_rng(11)
    ack = rng.random(npk) < 0.25
    ack_rows = torch.from_numpy(np.nonzero(ack)[0]).to(dev)
    t = {k: [] for k in ("write", "write_wall", "plan", "plan_wall", "set_encode", "set_encode_wall", "flat")}
    ok = None
    for r in range(reps + 2):                      # two warm-up rounds, the first one verified
        w = timed(enc, lambda: tset.write(src, src_off, n, n_written=n_written), 2, "stream_tx")
        p = timed(enc, lambda: tset.plan(budget, npk, max_payload=M, max_segments=1, out=plan_out), 6, "stream_tx")
        # the caller's patch between plan and encode: a short SACK in a quarter of the packets
        iv = info.view(torch.int64)
        pn = iv[ack_rows, 0]
        iv[ack_rows, 2] = pn                       # largest_acked
        iv[ack_rows, 3] = pn - 4                   # largest_in_order: first block length 5
        iv[ack_rows, 4] = 7                        # delay_us
        info[ack_rows, 52] = 0x80                  # flags: this packet carries a SACK
        e = timed(enc, lambda: tset.encode(info, ranges, segs, conn_of, SLOT, framed=True, out=outs[0]), 1,
                  "packet_encode")
        # the identical records for the flat encoder: data_off into the buffer write took (every
        # connection's stream is at r * per in round r)
        flat_segs = segs.clone()
        flat_segs.view(torch.int32).view(npk, 4)[:, 2] = \
            (conn_of.to(torch.int64) * per + segs.view(torch.int64).view(npk, 2)[:, 0] - r * per).to(torch.int32)
        if r == 0:
            assert int(total.item()) == npk and n_written.tolist() == [per] * nconn
            sv = flat_segs.cpu().numpy().reshape(npk, 16).view(fec.PKT_SEGMENT_DTYPE).reshape(npk, 1)
        f = timed(enc, lambda: enc.packet_encode(info, ranges, flat_segs, src, SLOT, framed=True, out=outs[1]), 1,
                  "packet_encode")
        if r == 0:
            hv = info.cpu().numpy().reshape(npk * 64).view(fec.PKT_INFO_DTYPE)
            want, want_len = expectation(hv, sv, ack, src.cpu().numpy(), True, None)
            same = bool(torch.equal(outs[0][0], outs[1][0])) and bool(torch.equal(outs[0][1], outs[1][1]))
            ok = same and bool(torch.equal(outs[0][0], torch.from_numpy(want).to(dev))) and \
                bool((outs[0][1].cpu().numpy().view(np.uint16) == want_len).all()) and \
                not bool(outs[0][2].any()) and not bool(outs[1][2].any())
            wire_bytes = int(want_len.astype(np.int64).sum())
            del want, hv
        tset.release(upto)
        if r >= 2:
            for k, v in (("write", w), ("plan", p), ("set_encode", e)):
                t[k].append(v[0])
                t[k + "_wall"].append(v[1])
            t["flat"].append(f[0])
    st = tset.states()
    assert (st["base"] == st["tail"]).all() and int(st["packets"].sum()) == (reps + 2) * npk
    med = {k: float(np.median(v)) for k, v in t.items()}
    stream_bytes = npk * SEG
    alg = stream_bytes + wire_bytes
    cb = min(alg // 2, src.numel()) // 16 * 16
    copy_ms = bench.probe_nt_copy_ms([src.data_ptr()], [outs[0][0].data_ptr()], cb, reps, stream.cuda_stream)
    enc_copy = copy_ms * (alg / 2) / cb
    write_copy = copy_ms * stream_bytes / cb
    ratios = sorted(a / b for a, b in zip(t["set_encode"], t["flat"]))
    print(json.dumps({
        "probe": "stream_tx", "label": label, "connections": nconn, "packets": npk, "window_bytes": cap,
        "slot": SLOT, "max_payload": M, "reps": reps, "verify_all_wire_bytes": ok,
        "write_ms": round(med["write"], 4), "write_wall_ms": round(med["write_wall"], 4),
        "write_frac_of_copy": round(write_copy / med["write"], 4), "nt_copy_of_write_bytes_ms": round(write_copy, 4),
        "plan_ms": round(med["plan"], 4), "plan_wall_ms": round(med["plan_wall"], 4),
        "plan_ns_per_packet": round(med["plan"] * 1e6 / npk, 3),
        "set_encode_ms": round(med["set_encode"], 4), "set_encode_wall_ms": round(med["set_encode_wall"], 4),
        "set_encode_min_max": [round(min(t["set_encode"]), 4), round(max(t["set_encode"]), 4)],
        "flat_encode_ms": round(med["flat"], 4), "flat_min_max": [round(min(t["flat"]), 4), round(max(t["flat"]), 4)],
        "set_over_flat": round(med["set_encode"] / med["flat"], 4),
        "set_over_flat_per_rep_min_median_max": [round(ratios[0], 4), round(float(np.median(ratios)), 4),
                                                 round(ratios[-1], 4)],
        "algorithmic_bytes": alg, "nt_copy_same_bytes_ms": round(enc_copy, 4),
        "set_encode_frac_of_copy": round(enc_copy / med["set_encode"], 4),
        "note": "ms = median over reps of the summed kernel durations of one call (hipExtLaunchKernel events); "
                "wall = elapsed between events around the call, launch gaps included; set and flat encode run "
                "back to back in every repetition on identical records; algorithmic bytes = segment bytes read + "
                "wire bytes written; nt copy = libugoprobe's nt copy scaled to the same bytes"}), flush=True)
    tset.close()
    for tx in txs:
        tx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--packets", type=int, default=851968)
    ap.add_argument("--conns", default="1,1024,16384")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    npk = args.packets
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    enc = fec.New(10, 3)
    gen = torch.Generator(device=dev).manual_seed(5)
    src = torch.randint(0, 256, (npk * SEG,), dtype=torch.uint8, device=dev, generator=gen)
    outs = [(torch.zeros((npk, SLOT), dtype=torch.uint8, device=dev), torch.zeros(npk, dtype=torch.int16, device=dev),
             torch.zeros(npk, dtype=torch.uint8, device=dev)) for _ in range(2)]
    for nconn in [int(c) for c in args.conns.split(",")]:
        for o in outs:
            o[0].zero_()
        run(enc, nconn, npk, args.reps, args.label, src, outs, stream)
    enc.close()


if __name__ == "__main__":
    main()
