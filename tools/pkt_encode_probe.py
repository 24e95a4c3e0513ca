#!/usr/bin/env python3
"""ugo_fec_packet_encode on bench.py's packet-decode workload, reversed
(DESIGN.md §4.3): 851,968 packets, a quarter with a short SACK, a 3-byte packet
number, one 1400-B segment each taken from a flat stream buffer, slot 1488 --
once FEC-framed without a pad (tx_assemble's input) and once unframed with the
RC4 pad (FEC off).  Not product code.

Every packet of the batch is first compared with an expectation built on the
host with numpy (headers byte by byte, independent of the kernel).  Then the
kernel is timed with the launch-timing ABI (kernel class packet_encode) on two
cold buffer sets used in turn, and a device nt copy of the same byte count on
the same buffers is timed as the ceiling.  Algorithmic bytes = segment bytes
read + wire bytes written.  Prints one JSON line per mode.

  python3 tools/pkt_encode_probe.py [--reps 20] [--packets 851968] [--label TEXT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (probe_nt_copy_ms, HBM_PEAK_GBS)
from ugo_amd import fec  # noqa: E402

SLOT, SEG = 1488, 1400


def put_uvarint(hdr, pos, v, rows):
    """binary.PutUvarint of v[rows] at hdr[row, pos[row]...], vectorised."""
    v = v.copy()
    live = rows.copy()
    for _ in range(10):
        more = (v >> np.uint64(7)) != 0
        r = np.nonzero(live)[0]
        hdr[r, pos[r]] = ((v[r] & np.uint64(0x7F)) | (more[r].astype(np.uint64) << np.uint64(7))).astype(np.uint8)
        pos[r] += 1
        live &= more
        v >>= np.uint64(7)


def workload(npk, rng):
    seq = np.arange(npk, dtype=np.uint64)
    ack = rng.random(npk) < 0.25
    info = np.zeros(npk, fec.PKT_INFO_DTYPE)
    info["flags"] = np.where(ack, 0x80, 0)
    info["packet_number"] = seq + np.uint64(1 << 15)
    info["largest_acked"] = np.where(ack, seq + np.uint64(1 << 15), 0)
    info["largest_in_order"] = np.where(ack, seq + np.uint64((1 << 15) - 4), 0)  # first block length 5
    info["delay_us"] = np.where(ack, 7, 0)
    info["n_segments"] = 1
    segs = np.zeros((npk, 1), fec.PKT_SEGMENT_DTYPE)
    segs["offset"][:, 0] = seq * np.uint64(SEG)
    segs["data_off"][:, 0] = np.arange(npk, dtype=np.uint64) * SEG  # a contiguous stream window
    segs["len"][:, 0] = SEG
    return info, segs, ack


def expectation(info, segs, ack, stream, framed, ks):
    """The batch on the host: [npk, SLOT] with zeros past each packet, and the lengths."""
    npk = len(info)
    hdr = np.zeros((npk, 32), np.uint8)
    pos = np.full(npk, 6 if framed else 0)
    everyone = np.ones(npk, bool)
    hdr[np.arange(npk), pos] = np.where(ack, 0xA0, 0x20)  # PSH, ACK for a quarter
    pos += 1
    r = np.nonzero(ack)[0]
    pos[r] += 1  # type byte 0: no missing ranges
    put_uvarint(hdr, pos, info["largest_acked"], ack)
    hdr[r, pos[r]] = 7  # ufloat16(7), little endian
    pos[r] += 2
    hdr[r, pos[r]] = 5  # first block length
    pos[r] += 1
    put_uvarint(hdr, pos, info["packet_number"], everyone)
    put_uvarint(hdr, pos, segs["offset"][:, 0], everyone)
    hdr[np.arange(npk), pos] = SEG >> 8
    hdr[np.arange(npk), pos + 1] = SEG & 0xFF
    pos += 2
    out = np.zeros((npk, SLOT), np.uint8)
    data = stream.reshape(npk, SEG)
    for h in np.unique(pos):
        rows = np.nonzero(pos == h)[0]
        out[rows, :h] = hdr[rows, :h]
        out[rows, h:h + SEG] = data[rows]
        if ks is not None:
            out[rows, :h + SEG] ^= ks[None, :h + SEG]
    return out, (pos + SEG).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--packets", type=int, default=851968)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    npk = args.packets
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    enc = fec.New(10, 3)
    rng = np.random.default_rng(11)
    info, segs, ack = workload(npk, rng)
    ks = np.frombuffer(fec.rc4_keystream(b"1234567890123456", SLOT), np.uint8)
    pad = torch.from_numpy(ks.copy()).to(dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    streams = [torch.randint(0, 256, (npk * SEG,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(2)]
    d_info = torch.from_numpy(info.view(np.uint8).reshape(npk, 64).copy()).to(dev)
    d_segs = torch.from_numpy(segs.view(np.uint8).reshape(npk, 1, 16).copy()).to(dev)
    d_ranges = torch.zeros((npk, 1, 2), dtype=torch.int64, device=dev)
    outs = [(torch.zeros((npk, SLOT), dtype=torch.uint8, device=dev), torch.zeros(npk, dtype=torch.int16, device=dev),
             torch.zeros(npk, dtype=torch.uint8, device=dev)) for _ in range(2)]
    host_stream = streams[0].cpu().numpy()

    for mode, framed, p in (("framed", True, None), ("unframed_rc4", False, pad)):
        def run(r):
            enc.packet_encode(d_info, d_ranges, d_segs, streams[r % 2], SLOT, pad=p, framed=framed, out=outs[r % 2])

        for o in outs:
            o[0].zero_()
        run(0)
        torch.cuda.synchronize()
        want, want_len = expectation(info, segs, ack, host_stream, framed, None if p is None else ks)
        ok = bool(torch.equal(outs[0][0], torch.from_numpy(want).to(dev))) and \
            bool((outs[0][1].cpu().numpy().view(np.uint16) == want_len).all()) and not bool(outs[0][2].any())
        del want
        for r in range(4):
            run(r)
        torch.cuda.synchronize()
        enc.timing_begin(2 * args.reps)
        for r in range(args.reps):
            run(r)
        recs, _ = enc.timing_end()
        ms = recs["ms"][recs["kernel"] == fec.KERNEL_IDS["packet_encode"]]
        assert len(ms) == args.reps
        alg = npk * SEG + int(want_len.astype(np.int64).sum())
        cb = min(alg // 2, streams[0].numel()) // 16 * 16
        copy_ms = bench.probe_nt_copy_ms([s.data_ptr() for s in streams], [o[0].data_ptr() for o in outs], cb,
                                         args.reps, stream.cuda_stream) * (alg / 2) / cb
        k = float(np.median(ms))
        print(json.dumps({
            "probe": "pkt_encode", "label": args.label, "mode": mode, "packets": npk, "slot": SLOT,
            "verify_all_packets": ok, "packet_encode_ms": round(k, 4),
            "ms_min_max": [round(float(ms.min()), 4), round(float(ms.max()), 4)], "algorithmic_bytes": alg,
            "GBps": round(alg / (k * 1e-3) / 1e9, 1), "frac_of_8TBps": round(alg / (k * 1e-3) / 1e9 / 8000.0, 4),
            "Mpkt_per_s": round(npk / (k * 1e-3) / 1e6, 1), "nt_copy_same_bytes_ms": round(copy_ms, 4),
            "frac_of_copy": round(copy_ms / k, 4),
            "note": "kernel ms = median of the timed launches (hipExtLaunchKernel events) on 2 cold buffer sets "
                    "used in turn; algorithmic bytes = segment bytes read + wire bytes written; nt copy = "
                    "libugoprobe's one-chunk-per-thread nt copy of half that many bytes, stream -> wire buffers"}),
            flush=True)
    enc.close()


if __name__ == "__main__":
    main()
