"""Stream delivery on the GPU (include/ugo_stream.h): ugo_fec_stream_deliver is
batch Conn.handleSegment / segmentSorter.push, ugo_fec_stream_read is Conn.Read.

The checker is tests/stream_ref.py: LiteralConn restates the reference (gap list,
map of queued segments, the Read loop), RuleRx the header's rule over bitmaps.
The CPU tests hold the rule against the literal reference; the GPU tests hold
the device against the rule -- seg_status, every field of the record, every
read, and the whole window, which is pre-filled with a sentinel so that a byte
written outside an accepted segment shows -- and, where the history lies inside
the common domain, against the literal reference as well.

Argument checks that need a context (window size, slot and pad alignment) are
made on the Python side without a device and against the C entry points in a
GPU test: no context can be created on a host without a GPU.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import stream_ref as sr
from stream_harness import SENTINEL, Harness, enc, pad_bytes  # noqa: F401  (fixtures)
from stream_harness import rand_bytes as _bytes
from stream_ref import Packet, Seg
from ugo_amd import fec


# ------------------------------------------------------------------ CPU tests
def _run_both(steps, cap):
    """The history through the rule and the literal reference; every status,
    every read and every EOF must agree."""
    rule, lit = sr.RuleRx(cap), sr.LiteralConn()
    got = bytearray()
    for op, arg in steps:
        if op == "deliver":
            assert rule.deliver(arg) == lit.deliver(arg)
            assert rule.ngaps == len(lit.gaps)
        else:
            a, b = rule.read(arg), lit.read(arg)
            assert a == b
            got += a[0]
    assert rule.err == sr.NONE and lit.err == sr.NONE
    assert not lit.hit_start_eq_gap_end
    return bytes(got), rule, lit


def test_rule_matches_literal_reference_over_seeded_histories():
    n_eof = 0
    for seed in range(2500):
        rng = np.random.default_rng(seed)
        steps, data = sr.gen_history(rng, total_max=1500, in_batch_dups=seed % 2 == 1)
        got, rule, lit = _run_both(steps, 4096)
        assert got == data, seed           # the whole stream came out, in order
        assert rule.eof and lit.read(1) == (b"", True), seed
        n_eof += 1
    assert n_eof == 2500


def test_deviation_a_window_bound():
    s = Seg(4090, bytes(range(10)))
    rule, lit = sr.RuleRx(4096), sr.LiteralConn()
    assert rule.deliver([Packet([s])]) == [[sr.OUT_OF_WINDOW]]
    assert rule.hi == 0 and not rule.C.any() and rule.out_of_window == 1   # not applied
    assert lit.deliver([Packet([s])]) == [[sr.ACCEPTED]]                   # the reference buffers without bound
    # one byte less fits
    assert sr.RuleRx(4096).deliver([Packet([Seg(4086, bytes(10))])]) == [[sr.ACCEPTED]]


def test_deviation_b_gap_limit_after_the_call():
    # 50 isolated segments make 51 gaps; the batch's last segment closes one again
    segs = [Seg(10 + 20 * k, bytes(10)) for k in range(50)] + [Seg(0, bytes(10))]
    batch = [Packet([s]) for s in segs]
    rule, lit = sr.RuleRx(4096), sr.LiteralConn()
    assert rule.deliver(batch) == [[sr.ACCEPTED]] * 51
    assert rule.ngaps == 50 and rule.err == sr.NONE
    want = [[sr.ACCEPTED]] * 49 + [[sr.TOO_MANY_GAPS], [sr.NONE]]          # the reference trips on the transient
    assert lit.deliver(batch) == want and lit.err == sr.TOO_MANY_GAPS
    # without the closing segment both trip
    rule = sr.RuleRx(4096)
    rule.deliver(batch[:50])
    assert rule.ngaps == 51 and rule.err == sr.TOO_MANY_GAPS


def test_deviation_c_passed_empty_segment_is_forgotten():
    rule, lit = sr.RuleRx(4096), sr.LiteralConn()
    first = [Packet([Seg(10)]), Packet([Seg(0, bytes(range(20)))])]        # an empty segment, then data over it
    assert rule.deliver(first) == lit.deliver(first) == [[sr.ACCEPTED], [sr.ACCEPTED]]
    assert rule.read(20) == lit.read(20) == (bytes(range(20)), False)
    again = [Packet([Seg(10)])]
    assert lit.deliver(again) == [[sr.DUPLICATE]]                          # the map entry lives for ever
    assert rule.deliver(again) == [[sr.OUT_OF_WINDOW]]                     # below read_pos, forgotten
    longer = [Packet([Seg(10, bytes(15))])]
    assert lit.deliver(longer) == [[sr.DUPLICATE]] and lit.err == sr.NONE
    assert rule.deliver(longer) == [[sr.OVERLAP]] and rule.err == sr.OVERLAP


def test_symbols_constants_and_null_arguments():
    lib = fec.load_library()
    syms = fec.header_symbols()
    for name in ("ugo_fec_stream_rx_create", "ugo_fec_stream_rx_destroy", "ugo_fec_stream_deliver",
                 "ugo_fec_stream_read", "ugo_fec_stream_rx_state", "ugo_fec_stream_rx_window"):
        assert name in syms and hasattr(lib, name)
    hdr = open(fec.STREAM_HEADER_PATH).read()
    for name, val in [("NONE", fec.STREAM_NONE), ("ACCEPTED", fec.STREAM_ACCEPTED),
                      ("DUPLICATE", fec.STREAM_DUPLICATE), ("OUT_OF_WINDOW", fec.STREAM_OUT_OF_WINDOW),
                      ("OVERLAP", fec.STREAM_OVERLAP), ("TOO_MANY_GAPS", fec.STREAM_TOO_MANY_GAPS)]:
        assert re.search(rf"UGO_STREAM_{name} = {val}\b", hdr), name
        assert getattr(sr, name) == val
    assert f"#define UGO_STREAM_MAX_GAPS {fec.STREAM_MAX_GAPS}u" in hdr and sr.MAX_GAPS == fec.STREAM_MAX_GAPS
    assert f"#define UGO_STREAM_MIN_WINDOW {fec.STREAM_MIN_WINDOW}u" in hdr
    # the record's fields, in the header's order
    body = hdr[hdr.index("typedef struct ugo_stream_rx_state {"):hdr.index("} ugo_stream_rx_state;")]
    fields = re.findall(r"^\s*u?int\d+_t (\w+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    assert fields == list(fec.STREAM_STATE_DTYPE.names)
    main = open(fec.HEADER_PATH).read()
    assert "#define UGO_FEC_KERNEL_STREAM_DELIVER 9" in main and "#define UGO_FEC_KERNEL_STREAM_READ 10" in main
    assert fec.KERNEL_NAMES[9] == "stream_deliver" and fec.KERNEL_NAMES[10] == "stream_read"
    assert lib.ugo_fec_abi_version() == 9
    # no context, no window
    h = ctypes.c_void_p()
    for wb in (4096, 4095, 2048, 0):
        assert lib.ugo_fec_stream_rx_create(None, wb, ctypes.byref(h)) == 6 and not h.value
    assert lib.ugo_fec_stream_rx_create(None, 4096, None) == 6
    assert lib.ugo_fec_stream_deliver(None, None, 16, None, None, None, 1, 1, None, None) == 6
    assert lib.ugo_fec_stream_read(None, None, 0, None, None, None) == 6
    assert lib.ugo_fec_stream_rx_state(None, None) == 6
    assert lib.ugo_fec_stream_rx_window(None, None, None) == 6
    lib.ugo_fec_stream_rx_destroy(None)


def test_python_argument_checks():
    for wb in (0, 2048, 4095, 4097, 3 * 4096):
        with pytest.raises(ValueError):
            fec.StreamRx.check_window(wb)
    fec.StreamRx.check_window(4096)
    fec.StreamRx.check_window(1 << 31)
    for slot, pk, pad in [(1480, 0, None), (0, 0, None), (0x10000, 0, None), (1488, 8, None), (1488, 0, 4)]:
        with pytest.raises(ValueError):
            fec.StreamRx.check_batch(slot, pk, pad)
    fec.StreamRx.check_batch(1488, 4096, 256)


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
def test_argument_checks_against_a_context(enc):
    lib = fec.load_library()
    h = ctypes.c_void_p()
    for wb in (0, 2048, 4095, 4097, 3 * 4096):
        assert lib.ugo_fec_stream_rx_create(enc._h, wb, ctypes.byref(h)) == 6 and not h.value
    rx = fec.StreamRx(enc, 4096)
    pk = torch.zeros(4 * 64 + 16, dtype=torch.uint8, device="cuda")
    info = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    segs = torch.zeros((4, 1, 16), dtype=torch.uint8, device="cuda")
    st = torch.zeros((4, 1), dtype=torch.uint8, device="cuda")
    pad = torch.zeros(80, dtype=torch.uint8, device="cuda")
    base = pk.data_ptr()
    assert base % 16 == 0 and pad.data_ptr() % 16 == 0

    def call(pkts=base, slot=64, padp=None, npk=4, infop=info.data_ptr(), stp=st.data_ptr()):
        return lib.ugo_fec_stream_deliver(rx._h, pkts, slot, padp, infop, segs.data_ptr(), 1, npk, stp, None)

    assert call(slot=60) == 6 and call(slot=0) == 6 and call(slot=0x10000) == 6
    assert call(pkts=base + 8) == 6
    assert call(padp=pad.data_ptr() + 4) == 6
    assert call(pkts=None) == 6 and call(infop=None) == 6 and call(stp=None) == 6
    pageable = np.zeros(256, np.uint8)
    assert call(infop=pageable.ctypes.data) == 6                # pageable host memory
    assert call(npk=0, pkts=None) == 0                           # an empty batch is a no-op
    assert lib.ugo_fec_stream_read(rx._h, None, 16, None, None, None) == 6
    assert call(padp=pad.data_ptr()) == 0                        # and a well-formed call goes through
    assert int(rx.state()["accepted"]) == 0 and int(rx.state()["out_of_window"]) == 0
    rx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_pad", [False, True])
def test_alignment_sweep(enc, pad_bytes, with_pad):
    """All 16 x 16 residues of (data_off mod 16, stream offset mod 16) for six
    lengths.  The stream is tiled without gaps -- filler segments set the next
    offset's residue -- so neighbours share 16-B chunks, and the ring laps."""
    rng = np.random.default_rng(11)
    h = Harness(enc, 4096, slot=128, max_segments=1, pad=pad_bytes[:128] if with_pad else None)
    seen = set()
    for L in (1, 15, 16, 17, 33, 64):
        x = h.rule.read_pos + h.rule.readable
        packets, offs = [], []
        for k in range(256):
            r_doff, r_off = k % 16, k // 16
            fill = (r_off - x) % 16
            if fill:
                packets.append(Packet([Seg(x, _bytes(rng, fill))]))
                offs.append(7)
                x += fill
            packets.append(Packet([Seg(x, _bytes(rng, L))]))
            offs.append(16 + r_doff)
            seen.add((L, r_doff, x % 16))
            x += L
        # as many packets per call as the window holds
        k = 0
        while k < len(packets):
            room = h.cap - h.rule.readable
            n = 0
            while k + n < len(packets) and packets[k + n].segs[0].length <= room:
                room -= packets[k + n].segs[0].length
                n += 1
            chunk_offs = offs[k:k + n]
            got = h.deliver(packets[k:k + n], data_off=lambda i, j: chunk_offs[i], ordered=0)
            assert (got[:, 0] == sr.ACCEPTED).all()
            h.read(h.cap)
            k += n
    assert len(seen) == 6 * 256
    h.close()


@pytest.mark.gpu
def test_shared_chunks(enc, pad_bytes):
    """Adjacent accepted segments of one batch that share 16-B chunks at both
    ends, delivered in an order that is not the stream's."""
    rng = np.random.default_rng(12)
    h = Harness(enc, 4096, slot=256, max_segments=4, pad=pad_bytes[:256])
    cuts = [0, 5, 9, 13, 14, 37, 60, 61, 75, 80, 99, 131, 150]     # several boundaries inside one chunk
    segs = [Seg(a, _bytes(rng, b - a)) for a, b in zip(cuts, cuts[1:])]
    order = [7, 2, 11, 0, 5, 9, 1, 10, 3, 8, 6, 4]
    packets = [Packet([segs[i] for i in order[k:k + 3]]) for k in range(0, 12, 3)]
    got = h.deliver(packets, ordered=0)
    assert (got[:, :3] == sr.ACCEPTED).all()
    assert h.rule.readable == 150 and h.rule.ngaps == 1
    h.read(150)
    h.close()


@pytest.mark.gpu
def test_wrap(enc, pad_bytes):
    rng = np.random.default_rng(13)
    cap = 4096
    h = Harness(enc, cap, slot=1488, max_segments=2, pad=pad_bytes)
    # advance read_pos to 3000: the ring's physical end (4096) now lies inside the window [3000, 7096)
    h.deliver([Packet([Seg(o, _bytes(rng, 300))]) for o in range(0, 3000, 300)], ordered=0)
    h.read(3000)
    assert h.rule.read_pos == 3000
    lim = 3000 + cap
    batch = [
        Packet([Seg(4000, _bytes(rng, 96))]),                     # ends exactly at the physical end
        Packet([Seg(4096, _bytes(rng, 33))]),                     # starts exactly at it
        Packet([Seg(4200, _bytes(rng, 50)), Seg(lim - 40, _bytes(rng, 40))]),   # ...; ends exactly at read_pos + cap
        Packet([Seg(lim - 39, _bytes(rng, 40))]),                 # one byte too far: out of window
        Packet([Seg(lim, _bytes(rng, 8))]),                       # starts at read_pos + cap
        Packet([Seg(lim)]),                                       # an empty segment there is outside too
        Packet([Seg(lim - 100, _bytes(rng, 101))]),               # straddles read_pos + cap
    ]
    got = h.deliver(batch, ordered=0)
    assert got[:, 0].tolist() == [1, 1, 1, 3, 3, 3, 3] and got[2, 1] == 1
    # a segment that straddles the physical end, and the bytes up to it
    h.deliver([Packet([Seg(3000, _bytes(rng, 1000))]), Packet([Seg(4129, _bytes(rng, 71))]),
               Packet([Seg(4250, _bytes(rng, 1400))])], ordered=0)
    assert h.rule.readable == 2650
    h.read(500)
    h.read(1000)                                                  # across the physical end
    # the window moved: what was out of window now fits, over ring positions that were read
    got = h.deliver([Packet([Seg(lim, _bytes(rng, 8)), Seg(lim + 8)])], ordered=0)
    assert got[0].tolist() == [1, 1]
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("npk", [64, 93])
@pytest.mark.parametrize("reverse", [False, True])
def test_long_interior(enc, pad_bytes, reverse, npk):
    """64 packets x one 1400-B segment, slot 1488, cap 131072: four blocks of the
    classify kernels and one of the copy kernel's, which takes 64 packets per
    block; 93 packets, all that this window holds, are two of those."""
    rng = np.random.default_rng(14)
    h = Harness(enc, 131072, slot=1488, max_segments=1, pad=pad_bytes, literal=True)
    packets = [Packet([Seg(1400 * k, _bytes(rng, 1400))]) for k in range(npk)]
    if reverse:
        packets.reverse()
    got = h.deliver(packets, data_off=lambda i, j: 21 + i % 17, ordered=0)
    assert (got == sr.ACCEPTED).all()
    assert h.rule.readable == npk * 1400
    h.read(npk * 1400 - 7)
    h.read(100)
    h.close()


@pytest.mark.gpu
def test_multi_segment_packets(enc, pad_bytes):
    rng = np.random.default_rng(15)
    h = Harness(enc, 8192, slot=512, max_segments=4, pad=pad_bytes[:512])
    x = 0
    packets = []
    for i in range(9):
        segs = []
        for j in range(1 + i % 4):
            n = int(rng.integers(1, 90))
            segs.append(Seg(x, _bytes(rng, n)))
            x += n
        packets.append(Packet(segs))
    packets[4].status = fec.PKT_CAPACITY                          # dropped whole: a hole in the stream
    # the last segment of the last packet is truncated: 30 of its 75 bytes arrived
    packets[8].segs[-1] = Seg(packets[8].segs[-1].offset, _bytes(rng, 30), length=75)
    got = h.deliver(packets, ordered=0)
    assert (got[4] == 0).all() and h.rule.skipped_packets == 1 and h.rule.ngaps == 2
    o = packets[8].segs[-1].offset
    assert not h.rule.W[o + 30:o + 75].any() and h.rule.W[o + 75] == SENTINEL   # the tail reads as zeros
    h.read(8192)
    # the dropped packet again, now decoded: the stream closes up
    packets[4].status = 0
    h.deliver([packets[4]], ordered=0)
    assert h.rule.ngaps == 1
    h.read(8192)
    h.close()


@pytest.mark.gpu
def test_clean_batches_skip_the_ordered_pass(enc, pad_bytes):
    rng = np.random.default_rng(16)
    h = Harness(enc, 8192, slot=256, max_segments=2, pad=pad_bytes[:256], literal=True)
    fresh = [Packet([Seg(100 * k, _bytes(rng, 60)), Seg(100 * k + 60, _bytes(rng, 40))]) for k in range(40)]
    fresh.append(Packet([Seg(4000)]))
    got = h.deliver(fresh, ordered=0)
    assert (got[:40] == sr.ACCEPTED).all()
    got = h.deliver(fresh, ordered=0)                              # the whole batch again: duplicates by C / S
    assert (got[:40] == sr.DUPLICATE).all() and got[40, 0] == sr.DUPLICATE
    h.read(1000)
    got = h.deliver(fresh, ordered=0)                              # and again, partly below read_pos
    assert (got[:40] == sr.DUPLICATE).all()
    assert int(h.rx.state()["ordered_segments"]) == 0
    h.close()


@pytest.mark.gpu
def test_contested_batches(enc, pad_bytes):
    rng = np.random.default_rng(17)
    h = Harness(enc, 8192, slot=256, max_segments=2, pad=pad_bytes[:256], literal=True)
    a = Packet([Seg(0, _bytes(rng, 50)), Seg(50, _bytes(rng, 30))])
    got = h.deliver([a, Packet([Seg(200, _bytes(rng, 10))]), a])           # the same packet twice
    assert got.tolist() == [[1, 1], [1, 0], [2, 2]] and h.rule.contested == 4
    long_, short = Seg(300, _bytes(rng, 40)), None
    short = Seg(300, long_.data[:25])
    got = h.deliver([Packet([long_]), Packet([short])])                    # same offset, the longer first
    assert got[:, 0].tolist() == [1, 2] and h.rule.contested == 2
    long2 = Seg(400, _bytes(rng, 40))
    short2 = Seg(400, long2.data[:25])
    rest2 = Seg(425, long2.data[25:])
    got = h.deliver([Packet([short2]), Packet([long2]), Packet([rest2])])  # the shorter first wins, its rest follows
    assert got[:, 0].tolist() == [1, 2, 1] and h.rule.contested == 3   # the rest lies in the longer one's claim
    assert h.rule.W[400:440].tobytes() == long2.data
    got = h.deliver([Packet([Seg(500)]), Packet([Seg(500, _bytes(rng, 9))])])   # empty, then data at its offset
    assert got[:, 0].tolist() == [1, 2] and h.rule.contested == 2
    assert h.rule.W[500] == SENTINEL
    got = h.deliver([Packet([Seg(600, _bytes(rng, 9))]), Packet([Seg(600)])])   # and the reverse
    assert got[:, 0].tolist() == [1, 2] and h.rule.contested == 2
    # an empty segment inside another segment's range is contested with it, and both are accepted
    got = h.deliver([Packet([Seg(700, _bytes(rng, 20))]), Packet([Seg(710)])], ordered=2)
    assert got[:, 0].tolist() == [1, 1]
    assert h.ordered == 15
    h.finish()                                                     # no claim or contested bit stayed behind
    h.close()


def _fatal_case(enc, pad, first_call, batch, want, err_at, sentinel_at):
    h = Harness(enc, 4096, slot=256, max_segments=2, pad=pad)
    if first_call:
        h.deliver(first_call, ordered=0)
    got = h.deliver(batch, ordered=None)
    assert got[:, 0].tolist() == want
    st = h.rx.state()
    assert int(st["err"]) == fec.STREAM_OVERLAP and (int(st["err_packet"]), int(st["err_segment"])) == err_at
    assert int(st["ordered_segments"]) >= 1
    win = h.rx.window().cpu().numpy()
    assert (win[sentinel_at[0]:sentinel_at[1]] == SENTINEL).all()     # the later fresh segment went nowhere
    before = dict(h.rule.record())
    got = h.deliver(batch, ordered=0)                               # the next call is inert
    assert not got.any() and h.rule.record() == before
    h.close()


@pytest.mark.gpu
def test_fatal_overlap(enc, pad_bytes):
    rng = np.random.default_rng(18)
    pad = pad_bytes[:256]
    fresh = Packet([Seg(1000, _bytes(rng, 64))])
    ok = Packet([Seg(500, _bytes(rng, 20))])
    # partial overlap with an earlier call's data
    _fatal_case(enc, pad, [Packet([Seg(0, _bytes(rng, 100))])],
                [ok, Packet([Seg(90, _bytes(rng, 20))]), fresh], [1, 4, 0], (1, 0), (1000, 1064))
    # ... reaching below read_pos is no different
    a, b = Seg(100, _bytes(rng, 30)), Seg(120, _bytes(rng, 30))
    # partial overlap between two segments of one batch, both arrival orders
    _fatal_case(enc, pad, None, [ok, Packet([a]), Packet([b]), fresh], [1, 1, 4, 0], (2, 0), (1000, 1064))
    _fatal_case(enc, pad, None, [ok, Packet([b]), Packet([a]), fresh], [1, 1, 4, 0], (2, 0), (1000, 1064))
    # the fatal segment second in its packet; a clean duplicate after it is not reported either
    h = Harness(enc, 4096, slot=256, max_segments=2, pad=pad)
    h.deliver([Packet([Seg(0, _bytes(rng, 100))])], ordered=0)
    got = h.deliver([Packet([Seg(100, _bytes(rng, 10)), Seg(95, _bytes(rng, 20))]), Packet([Seg(0, bytes(100))]),
                     fresh], ordered=None)
    assert got.tolist() == [[1, 4], [0, 0], [0, 0]] and h.rule.err_segment == 1
    assert h.rule.duplicate == 0 and h.rule.accepted == 2
    h.read(4096)                                                    # what was readable can still be read
    h.close()


@pytest.mark.gpu
def test_too_many_gaps(enc, pad_bytes):
    rng = np.random.default_rng(19)
    iso = [Packet([Seg(10 + 20 * k, _bytes(rng, 10))]) for k in range(51)]
    h = Harness(enc, 4096, slot=64, max_segments=1, pad=pad_bytes[:64])
    h.deliver(iso, ordered=0)
    assert h.rule.err == sr.TOO_MANY_GAPS and h.rule.ngaps == 52
    got = h.deliver([Packet([Seg(0, _bytes(rng, 10))])], ordered=0)
    assert not got.any()
    h.close()
    h = Harness(enc, 4096, slot=64, max_segments=1, pad=pad_bytes[:64], literal=True)
    h.deliver(iso[:49], ordered=0)
    assert h.rule.err == sr.NONE and h.rule.ngaps == 50
    h.deliver([Packet([Seg(20 * k, _bytes(rng, 10))]) for k in range(49)], ordered=0)   # fills the gaps
    assert h.rule.err == sr.NONE and h.rule.ngaps == 1 and h.rule.readable == 49 * 20
    h.read(49 * 20)
    h.close()


@pytest.mark.gpu
def test_read(enc, pad_bytes):
    rng = np.random.default_rng(20)
    cap = 4096
    h = Harness(enc, cap, slot=1488, max_segments=1, pad=pad_bytes, literal=True)
    segs = [Seg(0, _bytes(rng, 700)), Seg(700, _bytes(rng, 1300)), Seg(2000, _bytes(rng, 1000))]
    h.deliver([Packet([s]) for s in segs], ordered=0)
    assert h.read(0) == (b"", False)
    h.read(300)                                                     # below readable, inside the first segment
    st = h.rx.state()
    assert st["head_valid"] == 1 and st["head_off"] == 0
    got = h.deliver([Packet([segs[0]])], ordered=0)                 # its retransmission: duplicate through head_off
    assert got[0, 0] == sr.DUPLICATE
    h.read(400)                                                     # up to the segment's end exactly
    assert h.rx.state()["head_valid"] == 0
    h.read(1301)                                                    # one byte into the third
    assert int(h.rx.state()["head_off"]) == 2000
    h.read(10, discard=True)                                        # dst = NULL
    data, eof = h.read(5000)                                        # above readable
    assert len(data) == 989 and not eof
    assert h.read(16) == (b"", False)
    # one lap later the same ring positions hold new data: the bits were cleared
    more = [Seg(3000, _bytes(rng, 1400)), Seg(4400, _bytes(rng, 1400)), Seg(5800, _bytes(rng, 1296))]
    got = h.deliver([Packet([s]) for s in more], ordered=0)
    assert got[:, 0].tolist() == [1, 1, 1] and h.rule.hi == h.rule.read_pos + cap
    h.read(1000)
    h.read(2000)                                                    # across the physical end (4096)
    got = h.deliver([Packet([Seg(7096)])], ordered=0)
    assert got[0, 0] == sr.ACCEPTED and h.rule.eof
    data, eof = h.read(1095)
    assert len(data) == 1095 and not eof                            # one byte short of the empty segment
    data, eof = h.read(1)
    assert len(data) == 1 and eof                                   # EOF with the last byte in front of it
    assert h.read(10) == (b"", True)
    h.close()


@pytest.mark.gpu
def test_random_histories(enc, pad_bytes):
    """200 seeded histories from the CPU test's in-domain generator, plus
    packets repeated inside their batch; device = rule = literal reference."""
    streams = ordered = 0
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        cap = (4096, 8192)[seed % 2]
        steps, data = sr.gen_history(rng, total_max=cap - 100, in_batch_dups=True)
        h = Harness(enc, cap, slot=256, max_segments=3, pad=pad_bytes[:256] if seed % 4 else None, literal=True)
        got = bytearray()
        for op, arg in steps:
            if op == "deliver":
                h.deliver(arg)
            else:
                got += h.read(arg)[0]
        assert bytes(got) == data and h.rule.eof, seed
        ordered += h.ordered
        h.finish(seed)                               # the ring holds no stale bit of the history
        streams += 1
        h.close()
    assert streams == 200 and ordered > 200          # the ordered pass had its share


@pytest.mark.gpu
@pytest.mark.parametrize("framed", [False, True])
def test_chain_encode_decode_deliver_read(enc, pad_bytes, framed):
    """packet_encode -> packet_decode -> deliver -> read returns the sender's
    stream window byte for byte."""
    rng = np.random.default_rng(21)
    npk, slot, max_segments = 100, 1488, 2
    stream = torch.from_numpy(rng.integers(0, 256, 120000, dtype=np.uint8)).cuda()
    info = np.zeros(npk, fec.PKT_INFO_DTYPE)
    segs = np.zeros((npk, max_segments), fec.PKT_SEGMENT_DTYPE)
    x = 0
    for i in range(npk):
        info[i]["packet_number"] = i + 1
        info[i]["n_segments"] = 1 + i % 2
        for j in range(1 + i % 2):
            n = int(rng.integers(1, 650))
            segs[i, j] = (x, x, n, n)            # the sender's window: data_off = stream offset
            x += n
    order = rng.permutation(npk)                # the network reorders
    info, segs = info[order], segs[order]
    di = torch.from_numpy(info.view(np.uint8).reshape(npk, 64)).cuda()
    ds = torch.from_numpy(segs.view(np.uint8).reshape(npk, max_segments, 16)).cuda()
    ranges = torch.zeros((npk, 1, 2), dtype=torch.int64, device="cuda")
    dpad = torch.from_numpy(pad_bytes[:slot]).cuda()
    wire, wire_lens, status = enc.packet_encode(di, ranges, ds, stream, slot, pad=None if framed else dpad,
                                                framed=framed)
    assert not status.any().item()
    if framed:   # what tx_assemble's markData would put in front: a typeData FEC header
        wire[:, 4] = 0xF1
    oinfo, _, osegs = enc.packet_decode(wire, wire_lens, pad=None if framed else dpad, framed=framed,
                                        max_ranges=1, max_segments=max_segments)
    rx = fec.StreamRx(enc, 131072)
    st = rx.deliver(wire, oinfo, osegs, pad=None if framed else dpad)
    buf, n_read, eof = rx.read(x + 5)
    assert int(n_read.item()) == x and not eof.item()
    assert torch.equal(buf[:x], stream[:x])
    rec = rx.state()
    assert int(rec["accepted"]) == int(info["n_segments"].sum()) and int(rec["ordered_segments"]) == 0
    assert int((st == sr.ACCEPTED).sum().item()) == int(rec["accepted"])
    rx.close()
