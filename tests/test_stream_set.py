"""Stream delivery for a set of receive windows (ugo_fec_stream_set_*,
include/ugo_stream.h): one batch holds the packets of many connections.

The statement of what a set call means is stream_set_harness.demux_deliver:
every member's rule (tests/stream_ref.py) sees its subsequence of the batch.
The CPU tests hold that demultiplexing against hand-split batches; the GPU
tests hold the device against it -- every status, every field of every
member's record, ordered_segments and every window byte after every call --
at the smallest shapes where kernels written for one connection go wrong once
a block holds packets of several: one past the 16-packet classify block and
the 64-packet copy block, a fatal segment in one connection between another's
packets, contested segments of two connections in different tiles of the
ordered pass, a read of many members with one ticket each.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import stream_ref as sr
from stream_harness import SENTINEL, Harness, enc, pad_bytes  # noqa: F401  (fixtures)
from stream_harness import build_batch
from stream_harness import rand_bytes as _bytes
from stream_ref import Packet, Seg
from stream_set_harness import NO_CONN, SetHarness, conn_tensor, demux_deliver, interleave
from ugo_amd import fec

SET_SYMBOLS = ("ugo_fec_stream_set_create", "ugo_fec_stream_set_destroy", "ugo_fec_stream_set_deliver",
               "ugo_fec_stream_set_read", "ugo_fec_stream_set_state")


def P(o, data, status=0):
    return Packet([Seg(o, data)], status=status)


# ------------------------------------------------------------------ CPU tests
def test_set_symbols_constants_and_null_arguments():
    lib = fec.load_library()
    syms = fec.header_symbols()
    for name in SET_SYMBOLS:
        assert name in syms and hasattr(lib, name)
    hdr = open(fec.STREAM_HEADER_PATH).read()
    assert re.search(r"#define UGO_STREAM_NO_CONN 0xffffffffu\b", hdr) and fec.STREAM_NO_CONN == 0xffffffff
    assert lib.ugo_fec_abi_version() == 9      # added within version 9: the symbols are the feature test
    h = ctypes.c_void_p()
    fake = (ctypes.c_uint8 * 64)()             # a non-NULL context that must never be looked into
    ctx = ctypes.addressof(fake)
    one = (ctypes.c_void_p * 1)(None)          # a list with a NULL member
    rxs = ctypes.addressof(one)
    assert lib.ugo_fec_stream_set_create(None, rxs, 1, ctypes.byref(h)) == 6 and not h.value
    assert lib.ugo_fec_stream_set_create(ctx, None, 1, ctypes.byref(h)) == 6 and not h.value
    assert lib.ugo_fec_stream_set_create(ctx, rxs, 1, None) == 6
    assert lib.ugo_fec_stream_set_create(ctx, rxs, 0, ctypes.byref(h)) == 6 and not h.value
    assert lib.ugo_fec_stream_set_create(ctx, rxs, (1 << 20) + 1, ctypes.byref(h)) == 6 and not h.value
    assert lib.ugo_fec_stream_set_create(ctx, rxs, 1, ctypes.byref(h)) == 6 and not h.value     # NULL member
    assert lib.ugo_fec_stream_set_deliver(None, None, 16, None, None, None, 1, 1, None, None, None) == 6
    assert lib.ugo_fec_stream_set_read(None, None, None, None, None, None, None) == 6
    assert lib.ugo_fec_stream_set_state(None, None) == 6
    lib.ugo_fec_stream_set_destroy(None)


def test_set_python_argument_checks():
    def fake_rx(ctx):
        rx = object.__new__(fec.StreamRx)
        rx._h, rx._enc = None, ctx            # _h None: close() / __del__ do nothing
        return rx

    ctx_a, ctx_b = object(), object()
    a, b = fake_rx(ctx_a), fake_rx(ctx_a)
    for bad in ([], [a, b]):                   # empty; members that are not open
        with pytest.raises(ValueError):
            fec.StreamRxSet.check_members(ctx_a, bad)
    other = fake_rx(ctx_b)
    try:
        a._h, b._h, other._h = ctypes.c_void_p(16), ctypes.c_void_p(32), ctypes.c_void_p(48)   # "open"
        fec.StreamRxSet.check_members(ctx_a, [a, b])
        for bad in ([a, a], [a, b, a], [a, other], [a, object()]):
            with pytest.raises(ValueError):
                fec.StreamRxSet.check_members(ctx_a, bad)
    finally:
        a._h = b._h = other._h = None          # nothing to destroy
    fec.StreamRxSet.check_conn_of(torch.zeros(5, dtype=torch.int32), 5)
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros(4, dtype=torch.int32),
                torch.zeros(5, dtype=torch.float32), torch.zeros(10, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError):
            fec.StreamRxSet.check_conn_of(bad, 5)


def test_demultiplexing_agrees_with_hand_split_batches():
    for seed in range(40):
        rng = np.random.default_rng(seed)
        nconn = int(rng.integers(2, 6))
        lists = []
        for c in range(nconn):
            steps, _ = sr.gen_history(rng, total_max=600, in_batch_dups=True, calls=(1, 1), max_packets=10_000)
            lists.append(steps[0][1])
        packets, conn_of = interleave(rng, lists)
        for c in range(nconn):                 # the merge keeps every connection's own order
            assert [p for p, k in zip(packets, conn_of) if k == c] == lists[c]
        # strangers in between: they belong to nobody
        for at, who in ((0, NO_CONN), (len(packets) // 2, nconn), (len(packets), 0x7fffffff)):
            packets.insert(at, P(0, b"xyz"))
            conn_of.insert(at, who)
        rules = [sr.RuleRx(4096) for _ in range(nconn)]
        rows, contested = demux_deliver(rules, packets, conn_of)
        for c in range(nconn):
            alone = sr.RuleRx(4096)
            want = alone.deliver(lists[c], count_contested=True)
            assert [rows[i] for i, k in enumerate(conn_of) if k == c] == want
            assert alone.record() == rules[c].record() and contested[c] == alone.contested
            assert np.array_equal(alone.W, rules[c].W)
        assert all(rows[i] == [sr.NONE] for i, k in enumerate(conn_of) if not 0 <= k < nconn)


def test_demultiplexing_reports_the_fatal_packet_by_batch_index():
    a = [P(0, bytes(100)), P(50, bytes(100)), P(300, bytes(10))]        # the second overlaps the first
    b = [P(0, bytes(10)), P(10, bytes(10)), P(20, bytes(10)), P(30, bytes(10))]
    packets = [b[0], a[0], b[1], b[2], a[1], b[3], a[2]]
    conn_of = [1, 0, 1, 1, 0, 1, 0]
    rules = [sr.RuleRx(4096), sr.RuleRx(4096)]
    rows, _ = demux_deliver(rules, packets, conn_of)
    assert rows == [[1], [1], [1], [1], [sr.OVERLAP], [1], [sr.NONE]]
    assert rules[0].err == sr.OVERLAP and rules[0].err_packet == 4      # 1 in its own subsequence
    assert rules[1].err == sr.NONE and rules[1].accepted == 4
    # an inert member keeps its record, err_packet included
    rows, _ = demux_deliver(rules, [P(500, bytes(5)), P(40, bytes(5))], [0, 1])
    assert rows == [[sr.NONE], [1]] and rules[0].err_packet == 4 and rules[0].accepted == 1


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
def test_same_offsets_in_two_connections(enc, pad_bytes):
    rng = np.random.default_rng(21)
    h = SetHarness(enc, [4096, 8192], slot=256, max_segments=2, pad=pad_bytes)
    packets, conn_of = [], []
    for o in (0, 100, 200, 300, 400):
        for c in (0, 1):
            packets.append(P(o, _bytes(rng, 100)))
            conn_of.append(c)
    got = h.deliver(packets, conn_of, ordered=[0, 0])
    assert (got[:, 0] == sr.ACCEPTED).all()
    for c in (0, 1):
        assert h.rules[c].accepted == 5 and h.rules[c].readable == 500
    w0, w1 = (h.rxs[c].window().cpu().numpy()[:500] for c in (0, 1))
    mine = [np.concatenate([np.frombuffer(p.segs[0].data, np.uint8) for p, k in zip(packets, conn_of) if k == c])
            for c in (0, 1)]
    assert np.array_equal(w0, mine[0]) and np.array_equal(w1, mine[1]) and not np.array_equal(w0, w1)
    out = h.read([500, 500])
    assert out[0][0] == mine[0].tobytes() and out[1][0] == mine[1].tobytes()
    h.finish()
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("npk", [17, 65])
def test_blocks_that_mix_connections_keep_their_counters_apart(enc, pad_bytes, npk):
    """Round-robin over three connections, one packet more than a classify block
    (16) or a copy block (64) holds: connection 1 receives only duplicates,
    connection 2 one segment beyond its window."""
    rng = np.random.default_rng(npk)
    h = SetHarness(enc, [4096, 4096, 8192], slot=256, max_segments=2, pad=pad_bytes)
    h.deliver([P(0, _bytes(rng, 2000))], [1], slot=2048, ordered=[0, 0, 0])    # what connection 1 will see again
    packets, conn_of = [], []
    seen = [0, 0, 0]
    for i in range(npk):
        c = i % 3
        k = seen[c]
        seen[c] += 1
        if c == 0:
            p = P(64 * k, _bytes(rng, 50))                             # fresh, with gaps
        elif c == 1:
            p = P(0 if k == 0 else 37 * k, _bytes(rng, 30))            # its start bit, then covered bytes
        elif k == 3:
            p = P(8192 - 10, _bytes(rng, 20))                          # ends beyond read_pos + cap
        else:
            p = Packet([Seg(100 * k, _bytes(rng, 100)), Seg(5000 + 10 * k, _bytes(rng, 10))])
        packets.append(p)
        conn_of.append(c)
    h.deliver(packets, conn_of, ordered=[0, 0, 0])
    r0, r1, r2 = h.rules
    assert (r0.accepted, r0.duplicate, r0.out_of_window) == (seen[0], 0, 0)
    assert r0.hi == 64 * (seen[0] - 1) + 50 and r0.readable == 50
    assert (r1.accepted, r1.duplicate, r1.out_of_window) == (1, seen[1], 0) and r1.hi == 2000 and r1.readable == 2000
    assert (r2.accepted, r2.duplicate, r2.out_of_window) == (2 * (seen[2] - 1), 0, 1)
    assert r2.hi == 5000 + 10 * (seen[2] - 1) + 10 and r2.readable == 300
    h.read([50, 2000, 0])
    h.finish()
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nconn", [2, 3, 7])
def test_random_histories_interleaved(enc, pad_bytes, nconn):
    """A history of stream_ref.gen_history per connection, merged call by call
    with a seeded interleave that keeps every connection's order; reads go
    through set_read.  Every call is compared, and finish() closes each run."""
    ordered_seen = 0
    for seed in range(17):
        rng = np.random.default_rng(1000 * nconn + seed)
        caps = [4096 << (c % 2) for c in range(nconn)]
        h = SetHarness(enc, caps, slot=256, max_segments=3, pad=pad_bytes)
        todo = [list(sr.gen_history(rng, total_max=1500, in_batch_dups=True)[0]) for _ in range(nconn)]
        while any(todo):
            lists, ns = [[] for _ in range(nconn)], [0] * nconn
            for c in range(nconn):
                if not todo[c]:
                    continue
                op, arg = todo[c].pop(0)
                if op == "deliver":
                    lists[c] = arg
                else:
                    ns[c] = arg
            if any(lists):
                packets, conn_of = interleave(rng, lists)
                h.deliver(packets, conn_of)
            if any(ns):
                h.read(ns, shifts=[int(rng.integers(0, 16)) for _ in range(nconn)])
        assert all(r.eof and r.err == sr.NONE for r in h.rules), seed
        h.finish(seed)
        ordered_seen += sum(h.ordered)
        h.close()
    assert ordered_seen > 0                    # the ordered pass was entered


@pytest.mark.gpu
def test_a_fatal_overlap_stops_its_own_connection_only(enc, pad_bytes):
    rng = np.random.default_rng(41)
    h = SetHarness(enc, [4096, 4096], slot=256, max_segments=1, pad=pad_bytes)
    h.deliver([P(0, _bytes(rng, 100)), P(200, _bytes(rng, 100))], [0, 0])
    batch = [(1, P(0, _bytes(rng, 50))), (0, P(300, _bytes(rng, 50))),
             (0, P(50, _bytes(rng, 100))),                             # [50, 100) covered, [100, 150) not: fatal
             (1, P(50, _bytes(rng, 50))), (0, P(400, _bytes(rng, 50))), (1, P(100, _bytes(rng, 50)))]
    got = h.deliver([p for _, p in batch], [c for c, _ in batch], ordered=[1, 0])
    assert got[:, 0].tolist() == [1, 1, sr.OVERLAP, 1, 0, 1]           # A's later accept is undone and reads 0
    a, b = h.rules
    assert (a.err, a.err_packet, a.err_segment, a.accepted) == (sr.OVERLAP, 2, 0, 3)
    assert (b.err, b.accepted, b.readable) == (sr.NONE, 3, 150)
    # the next call: A is inert, B is live
    got = h.deliver([P(500, _bytes(rng, 20)), P(150, _bytes(rng, 20)), P(600, _bytes(rng, 20))], [0, 1, 0],
                    ordered=[0, 0])
    assert got[:, 0].tolist() == [0, 1, 0] and b.readable == 170 and a.accepted == 3
    h.read([0, 170])
    h.finish()                                 # B's bitmaps are clean; A stays as it is
    h.close()


@pytest.mark.gpu
def test_too_many_gaps_in_one_member_only(enc, pad_bytes):
    rng = np.random.default_rng(42)
    h = SetHarness(enc, [4096, 4096], slot=64, max_segments=1, pad=pad_bytes)
    lists = [[P(1 + 2 * k, _bytes(rng, 1)) for k in range(51)], [P(10 * k, _bytes(rng, 10)) for k in range(30)]]
    packets, conn_of = interleave(rng, lists)
    got = h.deliver(packets, conn_of, ordered=[0, 0])
    assert (got == sr.ACCEPTED).all()
    a, b = h.rules
    assert a.err == sr.TOO_MANY_GAPS and a.ngaps == 52 and b.err == sr.NONE and b.readable == 300
    got = h.deliver([P(0, _bytes(rng, 1)), P(300, _bytes(rng, 10))], [0, 1], ordered=[0, 0])
    assert got[:, 0].tolist() == [0, 1]
    h.finish()
    h.close()


@pytest.mark.gpu
def test_packets_of_no_connection_and_skipped_packets(enc, pad_bytes):
    rng = np.random.default_rng(51)
    h = SetHarness(enc, [4096, 4096], slot=256, max_segments=2, pad=pad_bytes)
    two = lambda o: Packet([Seg(o, _bytes(rng, 20)), Seg(o + 20, _bytes(rng, 20))])  # noqa: E731
    batch = [(NO_CONN, two(0)), (0, two(0)), (2, two(0)), (1, two(0)), (0x7fffffff, two(40)),
             (1, Packet(two(40).segs, status=fec.PKT_CAPACITY)), (0, two(40)), (NO_CONN, two(80)), (1, two(80)),
             (0, Packet(two(80).segs, status=3)), (2, Packet(two(0).segs, status=3))]
    got = h.deliver([p for _, p in batch], [c for c, _ in batch], ordered=[0, 0])
    for i, (c, p) in enumerate(batch):
        want = [1, 1] if c in (0, 1) and p.status == 0 else [0, 0]
        assert got[i].tolist() == want, i
    a, b = h.rules
    assert (a.accepted, a.skipped_packets, a.readable) == (4, 1, 80)
    assert (b.accepted, b.skipped_packets, b.readable, b.hi) == (4, 1, 40, 120)
    h.finish()
    h.close()


@pytest.mark.gpu
def test_a_set_of_one_equals_the_single_entry_points(enc, pad_bytes):
    for seed in range(6):
        rng = np.random.default_rng(600 + seed)
        steps, _ = sr.gen_history(rng, total_max=2500, in_batch_dups=True)
        single = Harness(enc, 4096, slot=256, max_segments=3, pad=pad_bytes)
        one = SetHarness(enc, [4096], slot=256, max_segments=3, pad=pad_bytes)
        for op, arg in steps:
            if op == "deliver":
                a = single.deliver(arg)
                b = one.deliver(arg, [0] * len(arg))
                assert np.array_equal(a, b)
            else:
                a = single.read(arg)
                b = one.read([arg])
                assert arg == 0 or a == b[0]
            assert single.rx.state().tobytes() == one.set.states()[0].tobytes()       # every field, reserved too
            assert torch.equal(single.rx.window(), one.rxs[0].window())
        single.close()
        one.close()


@pytest.mark.gpu
def test_set_calls_and_single_calls_mix(enc, pad_bytes):
    rng = np.random.default_rng(71)
    h = SetHarness(enc, [4096, 4096], slot=256, max_segments=1, pad=pad_bytes)
    h.deliver([P(0, _bytes(rng, 100)), P(0, _bytes(rng, 60)), P(100, _bytes(rng, 100))], [0, 1, 0])
    # member 0 through the single entry points, from the state the set left
    s = Harness(enc, 4096, slot=256, max_segments=1, pad=pad_bytes, rx=h.rxs[0], rule=h.rules[0], ordered=h.ordered[0])
    s.deliver([P(200, _bytes(rng, 50)), P(200, _bytes(rng, 50)), P(300, _bytes(rng, 10))])     # a repeat: ordered pass
    s.read(130)
    h.ordered[0] = s.ordered
    assert h.ordered[0] == 2
    h.check()                                  # set_state sees the single calls
    # a set call, then the member's own state at once: it waits for the set's stream
    packets, conn_of = [P(250, _bytes(rng, 50)), P(60, _bytes(rng, 40)), P(310, _bytes(rng, 10))], [0, 1, 0]
    pkts, info, segs = build_batch(packets, 256, 1, pad_bytes[:256], seed=9)

    def dev(x, *shape):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(shape)).cuda()

    h.set.deliver(dev(pkts, 3, 256), dev(info, 3, 64), dev(segs, 3, 1, 16), conn_tensor(conn_of),
                  pad=dev(pad_bytes[:256], 256))
    demux_deliver(h.rules, packets, conn_of)
    for c in (1, 0):
        st = h.rxs[c].state()
        want = h.rules[c].record()
        assert {k: int(st[k]) for k in want} == want
    h.check()
    s.read(1000)                               # and the single read after the set call
    h.read([0, 100])
    h.finish()
    h.close()


@pytest.mark.gpu
def test_1024_members(enc, pad_bytes):
    rng = np.random.default_rng(81)
    n = 1024
    h = SetHarness(enc, [4096] * n, slot=128, max_segments=1, pad=pad_bytes)
    h.deliver([P(0, _bytes(rng, 40)) for _ in range(n)], list(rng.permutation(n)), ordered=[0] * n)
    before = h.set.states()
    lists = [[P(100 * (k + 1), _bytes(rng, 30)) for k in range(c % 3)] for c in range(n)]
    packets, conn_of = interleave(rng, lists)
    assert len(packets) == sum(c % 3 for c in range(n))
    h.deliver(packets, conn_of, ordered=[0] * n)
    after = h.set.states()
    assert after.shape == (n,)
    for c in range(n):
        assert int(after[c]["accepted"]) == 1 + c % 3 and int(after[c]["readable"]) == 40
        if c % 3 == 0:
            assert before[c].tobytes() == after[c].tobytes()           # no packet: bit for bit
    out = h.read([40 if c % 2 else 0 for c in range(n)])
    assert all(len(d) == (40 if c % 2 else 0) for c, (d, _) in enumerate(out))
    h.finish(slot=1488)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement", ["apart", "together"])
def test_ordered_pass_across_tiles(enc, arrangement):
    """36,000 one-segment packets of two connections: three tiles (16,384
    entries each) of the ordered pass.  A packet repeated inside the batch makes
    two contested segments.  apart: connection 0's only in tile 0, connection
    1's only in tile 2; together: both in every tile."""
    npk, tile = 36000, 16384
    rng = np.random.default_rng(91)
    packets = [P(16 * (i // 2), _bytes(rng, 16)) for i in range(npk)]
    conn_of = [i % 2 for i in range(npk)]
    if arrangement == "apart":
        repeats = [1000, 5000, tile - 2, 2 * tile + 301, 2 * tile + 1001, npk - 1]
    else:
        repeats = [t * tile + k for t in range(3) for k in (500, 501, 3000, 3001)]
    for i in repeats:
        packets[i] = packets[i - 200]          # the same connection's earlier packet, again
    h = SetHarness(enc, [1 << 19, 1 << 19], slot=64, max_segments=1)
    got = h.deliver(packets, conn_of)
    assert (got[repeats, 0] == sr.DUPLICATE).all() and (np.delete(got[:, 0], repeats) == sr.ACCEPTED).all()
    per = [2 * sum(1 for i in repeats if i % 2 == c) for c in (0, 1)]
    assert h.ordered == per and min(per) > 0
    h.finish(slot=4096)
    h.close()


@pytest.mark.gpu
def test_set_read_in_one_call(enc, pad_bytes):
    rng = np.random.default_rng(101)
    h = SetHarness(enc, [4096] * 6, slot=2048, max_segments=2, pad=pad_bytes)
    # member 4 reads across its ring's end: read_pos to 3000 first
    h.deliver([P(0, _bytes(rng, 1500)), P(1500, _bytes(rng, 1500))], [4, 4])
    h.read([0, 0, 0, 0, 3000, 0])
    batch = [(0, P(0, _bytes(rng, 200))),                              # n = 0: skipped
             (1, P(0, _bytes(rng, 300))), (1, P(300, _bytes(rng, 300))),          # n < readable, inside a segment
             (2, P(0, _bytes(rng, 700))),                              # n == readable
             (3, P(0, _bytes(rng, 90))),                               # n > readable
             (4, P(3000, _bytes(rng, 1000))), (4, P(4000, _bytes(rng, 1000))),    # across the physical end (4096)
             (5, Packet([Seg(0, _bytes(rng, 100)), Seg(100)]))]        # ends at an empty segment: eof
    h.deliver([p for _, p in batch], [c for c, _ in batch])
    before = h.set.states()[0].tobytes()
    out = h.read([0, 450, 700, 5000, 1500, 200], shifts=[0, 1, 7, 15, 3, 9])
    assert [len(d) for d, _ in out] == [0, 450, 700, 90, 1500, 100]
    assert [e for _, e in out] == [False, False, False, False, False, True]
    assert h.set.states()[0].tobytes() == before and h.rules[0].readable == 200
    r1 = h.rules[1]
    assert r1.head_valid and r1.head_off == 300 and r1.read_pos == 450
    assert h.rules[4].read_pos == 4500
    # discard mode: the same bookkeeping, no destination
    h.deliver([P(90, _bytes(rng, 60)), P(5000, _bytes(rng, 96))], [3, 4])
    out = h.read([200, 150, 0, 10, 700, 5], discard=True)
    assert [len(d) for d, _ in out] == [200, 150, 0, 10, 596, 0] and out[5][1]
    h.finish()
    h.close()


@pytest.mark.gpu
def test_a_zero_length_read_at_the_end_of_stream_single_and_set(enc, pad_bytes):
    """readable == 0 with the empty segment at read_pos.  The two entry points
    differ on purpose: ugo_fec_stream_read with n == 0 still reports end of
    stream, as RuleRx.read(0) does; ugo_fec_stream_set_read skips a member with
    n[c] == 0 -- n_read 0, eof 0 -- and leaves its record bit for bit."""
    rng = np.random.default_rng(111)
    h = SetHarness(enc, [4096], slot=256, max_segments=2, pad=pad_bytes)
    h.deliver([Packet([Seg(0, _bytes(rng, 100)), Seg(100)])], [0])
    assert h.read([100])[0][1]                                         # everything read: end of stream
    rule = h.rules[0]
    assert rule.readable == 0 and rule.eof and rule.read(0) == (b"", True)
    before = h.set.states()[0].tobytes()
    s = Harness(enc, 4096, slot=256, max_segments=2, pad=pad_bytes, rx=h.rxs[0], rule=rule, ordered=h.ordered[0])
    assert s.read(0) == (b"", True)            # Harness.read holds n_read and eof against the rule's
    assert h.read([0])[0] == (b"", False)      # SetHarness.read holds them against the skip: 0 and 0
    assert h.set.states()[0].tobytes() == before
    h.close()


@pytest.mark.gpu
def test_set_argument_checks_against_a_context(enc):
    lib = fec.load_library()
    other = fec.New(4, 2, device=0)
    a, b, foreign = fec.StreamRx(enc, 4096), fec.StreamRx(enc, 8192), fec.StreamRx(other, 4096)

    def create(ctx, rxs, n=None):
        arr = (ctypes.c_void_p * max(len(rxs), 1))(*[r._h.value if r is not None else None for r in rxs])
        h = ctypes.c_void_p()
        rc = lib.ugo_fec_stream_set_create(ctx._h, ctypes.addressof(arr), len(rxs) if n is None else n, ctypes.byref(h))
        return rc, h

    for rxs, n in (([a, b, a], None), ([a, a], None), ([a, foreign], None), ([foreign], None), ([a, None], None),
                   ([a, b], 0)):
        rc, h = create(enc, rxs, n)
        assert rc == 6 and not h.value
    for bad in ([a, a], [a, foreign]):
        with pytest.raises(ValueError):
            fec.StreamRxSet(enc, bad)
    s = fec.StreamRxSet(enc, [a, b])
    pk = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    one_seg = np.zeros(4, fec.PKT_INFO_DTYPE)
    one_seg["n_segments"] = 1                  # an empty segment at offset 0 per packet
    info = torch.from_numpy(one_seg.view(np.uint8).reshape(4, 64)).cuda()
    segs = torch.zeros((4, 1, 16), dtype=torch.uint8, device="cuda")
    st = torch.full((4, 1), 0x77, dtype=torch.uint8, device="cuda")
    conn = conn_tensor([0, 1, 0, NO_CONN])
    before = s.states().tobytes()

    def call(pkts=pk.data_ptr(), slot=64, npk=4, connp=conn.data_ptr(), stp=st.data_ptr()):
        return lib.ugo_fec_stream_set_deliver(s._h, pkts, slot, None, info.data_ptr(), segs.data_ptr(), 1, npk, connp,
                                              stp, None)

    pageable = np.zeros(16, np.uint32)
    assert call(connp=pageable.ctypes.data) == 6                 # pageable conn_of
    assert call(connp=None) == 6 and call(stp=None) == 6 and call(slot=60) == 6 and call(pkts=pk.data_ptr() + 8) == 6
    assert call(npk=0, pkts=None, connp=None) == 0               # an empty batch is a no-op, not an error
    n = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert lib.ugo_fec_stream_set_read(s._h, None, None, n.data_ptr(), None, None, None) == 6      # no n_read
    assert lib.ugo_fec_stream_set_read(s._h, st.data_ptr(), None, n.data_ptr(), n.data_ptr(), None, None) == 6
    assert lib.ugo_fec_stream_set_read(s._h, None, None, pageable.ctypes.data, n.data_ptr(), None, None) == 6
    assert lib.ugo_fec_stream_set_state(s._h, None) == 6
    assert s.states().tobytes() == before and (st == 0x77).all().item()       # no output was written
    assert call() == 0                                           # and a well-formed call goes through
    got = s.states()
    assert st[:, 0].tolist() == [1, 1, 2, 0]                     # empty segments at offset 0: queued, queued, again
    assert [int(g["accepted"]) for g in got] == [1, 1] and int(got[0]["duplicate"]) == 1
    s.close()
    for rx in (a, b, foreign):
        rx.close()
    other.close()


@pytest.mark.gpu
def test_set_pinned_operands(enc, pad_bytes):
    rng = np.random.default_rng(121)
    h = SetHarness(enc, [4096, 8192, 4096], slot=256, max_segments=2, pad=pad_bytes)
    lists = [[P(70 * k, _bytes(rng, 70)) for k in range(9)], [P(33 * k, _bytes(rng, 33)) for k in range(14)],
             [P(0, _bytes(rng, 10)), P(0, _bytes(rng, 10))]]
    packets, conn_of = interleave(rng, lists)
    h.deliver(packets, conn_of, conn_where="pinned")
    h.deliver([P(700, _bytes(rng, 5))], [0], inputs="pinned", outputs="pinned")
    h.read([300, 462, 0], shifts=[5, 11, 0], where="pinned")
    h.read([1000, 5, 10], where="pinned", discard=True)
    h.finish()
    h.close()
