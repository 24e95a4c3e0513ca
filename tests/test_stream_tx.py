"""Send windows (ugo_fec_stream_tx_*, include/ugo_stream.h).

CPU: THE RULE against a literal restatement of the Go send loop
(tests/stream_tx_ref.py) -- the property of deviation (a) and a directed case
per deviation --, the record's layout, and the argument errors that need no
launch.  GPU: the set calls against one rule per member
(tests/stream_tx_harness.py), at the shapes where these kernels can go wrong.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import packet_ref as pr
import stream_ref as sr
import stream_tx_ref as tr
from stream_tx_harness import NO_CONN, SENTINEL, TxHarness, _put
from ugo_amd import fec

KEY = b"ugo-test-key"
MS = (16, 17, 21, 40, 64, 100, 1436)


# ---------------------------------------------------------------- CPU: the rule against the reference
def _strip(go_packets):
    """The reference's packets with their empty segments removed."""
    out = []
    for pn, segs in go_packets:
        kept = [(o, d) for o, d in segs if len(d) > 0]
        assert kept, "a packet of empty segments only"
        out.append((pn, kept))
    return out


def _both(stream, queue, wp, pending, pn, budget, M):
    """The same state through the reference and through the rule.  Returns
    (reference packets, rule packets with their bytes, reference, rule state)."""
    go = tr.GoSender(wp, pn)
    for o, l in queue:
        go.AddSegmentForRetransmission(tr.Segment(o, stream[o:o + l]))
    if pending:
        go.Write(stream[wp:wp + pending])
    got_go = go.sendPackets(budget, M)
    q = [list(e) for e in queue]
    pk, wp2, pn2, _ = tr.rule_packets(q, wp, wp + pending, pn, budget, M, 1 << 30)
    got_rule = [(n, [(o, stream[o:o + l]) for o, l, _ in segs]) for n, segs in pk]
    return got_go, got_rule, go, (q, wp2, pn2)


@pytest.mark.parametrize("M", MS)
def test_rule_is_reference_minus_empty_segments(M):
    rng = np.random.default_rng(1000 + M)
    stream = rng.integers(0, 256, 8 * 1436 + 64, dtype=np.uint8).tobytes()
    empties = 0
    for case in range(3000):
        wp = int(rng.integers(1, 4 * M))
        lens = [1, 2, 3, 4, 5, max(1, M - 8), max(1, M - 9), max(1, M - 12), M - 4, M - 3, M, 2 * M + 1]
        queue = []
        for _ in range(int(rng.integers(0, 5))):
            l = int(rng.choice(lens)) if rng.random() < 0.6 else int(rng.integers(1, 2 * M))
            l = min(l, wp)
            o = int(rng.integers(0, wp - l + 1))
            queue.append((o, l))
        pending = int(rng.choice([0, 1, M - 4, M - 5, 2 * (M - 4), int(rng.integers(0, 3 * M))]))
        budget = int(rng.integers(0, 7))
        pn = int(rng.integers(0, 1000))
        got_go, got_rule, go, (q, wp2, pn2) = _both(stream, queue, wp, pending, pn, budget, M)
        empties += any(len(d) == 0 for _, segs in got_go for _, d in segs)
        assert _strip(got_go) == got_rule, (case, queue, wp, pending, budget)
        assert [(s.offset, s.dataLen()) for s in go.retransmissionQueue] == [tuple(e) for e in q], case
        assert (go.writeOffset, go.lastPacketNumber) == (wp2, pn2), case
        assert go.lenOfDataForWriting() == wp + pending - wp2, case
    assert empties > 30, empties          # the reference did emit empty segments in this sample


def test_deviation_a_retransmission_site():
    """Exactly 4 bytes of room behind a retransmitted segment: the reference
    splits an empty segment off the next queue entry, the rule does not."""
    M, stream = 40, bytes(range(200))
    queue = [(0, M - 8), (50, 10)]
    got_go, got_rule, go, (q, wp, pn) = _both(stream, queue, 100, 0, 7, 1, M)
    assert got_go == [(8, [(0, stream[0:32]), (50, b"")])]
    assert got_rule == [(8, [(0, stream[0:32])])]
    assert [(s.offset, s.dataLen()) for s in go.retransmissionQueue] == [(50, 10)] == [tuple(e) for e in q]


def test_deviation_a_new_data_site():
    """Exactly 4 bytes of room for new data: the reference sends an empty
    segment at writeOffset (a FIN to the receiver), the rule nothing."""
    M, stream = 40, bytes(range(200))
    got_go, got_rule, go, (q, wp, pn) = _both(stream, [(0, M - 8)], 100, 20, 0, 2, M)
    assert got_go == [(1, [(0, stream[0:32]), (100, b"")]), (2, [(100, stream[100:120])])]
    assert got_rule == [(1, [(0, stream[0:32])]), (2, [(100, stream[100:120])])]
    assert go.writeOffset == wp == 120


def test_deviation_c_segment_cap():
    """A packet of 1-byte retransmissions: the reference has no cap (287 fit
    1436 bytes), the rule closes the packet at max_segments."""
    M, stream = 1436, bytes(300)
    queue = [(i, 1) for i in range(300)]
    go = tr.GoSender(300, 0)
    for o, l in queue:
        go.AddSegmentForRetransmission(tr.Segment(o, stream[o:o + l]))
    assert len(go.sendPackets(1, M)[0][1]) == 287      # 287 * 5 = 1435; a 288th header: 1439 > 1436
    q = [list(e) for e in queue]
    pk, _, _, popped = tr.rule_packets(q, 300, 300, 0, 2, M, 8)
    assert [len(s) for _, s in pk] == [8, 8] and popped == 16 and len(q) == 284


def test_deviation_d_empty_write():
    """Write([]byte{}): the reference sends an empty segment, the rule's
    zero-length write is a no-op."""
    go = tr.GoSender(10, 0)
    go.Write(b"")
    assert go.sendPackets(3, 1436) == [(1, [(10, b"")])]
    r = tr.RuleTx(4096, start_offset=10)
    before = r.record()
    assert r.write(b"") == 0 and r.plan(3, 1436, 8) == [] and r.record() == before


def test_rule_window_model_and_release():
    r = tr.RuleTx(4096, rq_cap=2, start_offset=4000, fill=SENTINEL)
    data = bytes(range(1, 201))
    assert r.write(data) == 200 and r.tail == 4200
    assert r.W[4000:4096].tobytes() == data[:96] and r.W[:104].tobytes() == data[96:] and r.W[104] == SENTINEL
    assert r.write(bytes(5000)) == 4096 - 200          # deviation (b): partial, never waits
    assert r.plan(1, 1436, 8) == [(1, [(4000, 1432)])]
    assert r.retransmit([(4000, 10), (3999, 5), (4000, 0), (5400, 40), (4100, 70000), (4010, 5), (4020, 5)]) == \
        [tr.RQ_QUEUED, tr.RQ_REJECTED, tr.RQ_REJECTED, tr.RQ_REJECTED, tr.RQ_REJECTED, tr.RQ_QUEUED, tr.RQ_FULL]
    r.release(6000)
    assert r.base == 4000                               # held back by the queued entry at 4000
    r.queue.clear()
    r.release(6000)
    assert r.base == r.write_pos == 5432                # and by write_pos


# ---------------------------------------------------------------- CPU: layout and arguments
def test_record_size_and_offsets():
    dt = fec.STREAM_TX_STATE_DTYPE
    assert dt.itemsize == 80
    want = [("base", 0), ("write_pos", 8), ("tail", 16), ("last_packet_number", 24), ("packets", 32),
            ("segments", 40), ("bytes_new", 48), ("bytes_retransmitted", 56), ("rq_rejected", 64), ("rq_len", 72),
            ("rq_head", 76)]
    assert [(n, dt.fields[n][1]) for n in dt.names] == want
    src = open(fec.STREAM_HEADER_PATH).read()
    body = re.search(r"typedef struct ugo_stream_tx_state \{(.*?)\} ugo_stream_tx_state;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint64_t|uint32_t)\s+(\w+);", body)
    assert [f for _, f in fields] == [n for n, _ in want]
    assert [8 if t == "uint64_t" else 4 for t, _ in fields] == [dt.fields[n][0].itemsize for n in dt.names]
    assert "(80 bytes)" in src and fec.STREAM_TX_RQ_DTYPE.itemsize == 16
    assert re.search(r"#define UGO_FEC_KERNEL_STREAM_TX 11\b", open(fec.HEADER_PATH).read())
    assert re.search(r"UGO_PKT_OUT_OF_WINDOW = 10\b", open(fec.PKT_HEADER_PATH).read())
    assert fec.PKT_OUT_OF_WINDOW == 10 and fec.KERNEL_NAMES[11] == "stream_tx"
    for word in ("THE RULE", "(a) no empty segment", "(b) the window bound", "(c) the segment cap",
                 "(d) the empty write"):
        assert word in src, word


def test_argument_errors_without_a_launch():
    lib = fec.load_library()
    bad = fec.ErrInvalidArg.code
    h = ctypes.c_void_p(1)
    assert lib.ugo_fec_stream_tx_create(None, 4096, 4, 0, 0, ctypes.byref(h)) == bad and h.value is None
    assert lib.ugo_fec_stream_tx_create(None, 4096, 4, 0, 0, None) == bad
    assert lib.ugo_fec_stream_tx_set_create(None, None, 1, ctypes.byref(h)) == bad
    assert lib.ugo_fec_stream_tx_set_write(None, None, None, None, None, None) == bad
    assert lib.ugo_fec_stream_tx_set_release(None, None, None) == bad
    assert lib.ugo_fec_stream_tx_set_retransmit(None, None, None, None, 1, None, None) == bad
    assert lib.ugo_fec_stream_tx_set_plan(None, None, 1436, 8, 0, None, None, None, None, None, None, None) == bad
    assert lib.ugo_fec_stream_tx_set_encode(None, None, None, 0, None, 0, None, 1, None, 0, None, 16, None, None,
                                            None) == bad
    assert lib.ugo_fec_stream_tx_set_state(None, None) == bad
    assert lib.ugo_fec_stream_tx_window(None, None, None) == bad and lib.ugo_fec_stream_tx_queue(None, None, None) == bad
    lib.ugo_fec_stream_tx_destroy(None)
    lib.ugo_fec_stream_tx_set_destroy(None)
    assert lib.ugo_fec_abi_version() == 9               # the symbols are the feature test
    for window, rq in ((4095, 4), (2048, 4), (1 << 32, 4), (12288, 4), (4096, 0), (4096, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            fec.StreamTx.check_create(window, rq)
    fec.StreamTx.check_create(1 << 31, 1)
    for args in ((15, 8, 10), (0x10000, 8, 10), (1436, 0, 10), (1436, 0x10000, 10), (1436, 8, (1 << 31) + 1)):
        with pytest.raises(ValueError):
            fec.StreamTxSet.check_plan(*args)
    with pytest.raises(ValueError):
        fec.StreamTxSet.check_members(None, [])


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def enc(gpu):
    return fec.New(10, 3)


@pytest.fixture(scope="module")
def pad_bytes():
    return fec.rc4_keystream(KEY, 1488)


def _data(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _flat_encode(enc, p, payload, data_offs, slot, framed, pad):
    """The parent's encoder on plan's records, reading one flat buffer:
    data_offs None keeps plan's data_off, else segment (i, j) reads there."""
    n = len(p["packets"])
    segs = p["segs_np"][:n].copy()
    if data_offs is not None:
        for (i, j), off in data_offs.items():
            segs[i, j]["data_off"] = off
    buf = torch.full((n + 1, slot), SENTINEL, dtype=torch.uint8, device="cuda")
    lens = torch.full((n,), -1, dtype=torch.int16, device="cuda")
    status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    enc.packet_encode(_put(p["info_np"][:n].view(np.uint8).reshape(n, 64)), torch.zeros((n, 1, 2), dtype=torch.int64,
                      device="cuda"), _put(segs.view(np.uint8).reshape(n, -1, 16)), payload, slot,
                      pad=None if pad is None else _put(np.frombuffer(pad, np.uint8)[:slot].copy()), framed=framed,
                      out=(buf[:n], lens, status))
    return buf, lens, status


@pytest.mark.gpu
@pytest.mark.parametrize("framed", [True, False])
def test_wire_equals_the_flat_encoder(enc, pad_bytes, framed):
    """One member, no wrap yet: set_encode of plan's output is
    ugo_fec_packet_encode(payload = the window, payload_stride = 0) on the same
    records, byte for byte over the whole wire buffer -- and the oracle's
    packets (compared inside the harness)."""
    rng = np.random.default_rng(3)
    pad = None if framed else pad_bytes
    h = TxHarness(enc, [65536], rq_caps=4)
    assert h.write([_data(rng, 40000)]) == [40000]
    first = h.plan_encode([5], 8, pad=pad, framed=framed)
    assert [s for _, _, s in first["packets"]] == [[(1432 * k, 1432)] for k in range(5)]
    assert h.retransmit([(0, 100, 700), (0, 3000, 17)]) == [tr.RQ_QUEUED] * 2
    p = h.plan_encode([40], 40, pad=pad, framed=framed)
    assert p["packets"][0][2] == [(100, 700), (3000, 17), (7160, 1436 - 8 - 717 - 4)]
    assert len(p["packets"]) == 24 and p["packets"][-1][2][0][1] < 1432
    n = len(p["packets"])
    buf, lens, status = _flat_encode(enc, p, h.txs[0].window(), None, 1488, framed, pad)
    assert torch.equal(buf[:n], p["wire"]) and torch.equal(lens, p["wire_lens"]) and not status.any().item()
    assert (buf[n] == SENTINEL).all().item()
    h.close()


@pytest.mark.gpu
def test_wrap_placements_one_packet_each(enc):
    """Window 4,096, M = 1436: one member per placement of the wrap point in
    its packet -- in the segment's head (before the packet's first 16-B
    boundary), in an interior chunk at each of the 16 byte phases, in the tail
    -- written in two pieces from sources at odd alignments, then planned and
    encoded.  The wire equals the flat encoder's on a linearised copy."""
    rng = np.random.default_rng(5)
    data_at = 6 + 1 + 1 + 2 + 2                    # framed, pn < 128, offset in [128, 16384): the data's packet byte
    ks = [1, 2, 3] + [4 + ph + 16 * (3 + ph) for ph in range(16)] + [1429, 1431]   # segment byte at the wrap point
    assert sorted({(data_at + k) % 16 for k in ks[3:19]}) == list(range(16))
    assert all(data_at + k < 16 for k in ks[:3]) and all(data_at + k >= (data_at + 1432) & ~15 for k in ks[19:])
    starts = [4096 - k for k in ks]
    h = TxHarness(enc, [4096] * len(ks), rq_caps=2, starts=starts)
    datas = [_data(rng, 1432 + c) for c in range(len(ks))]
    assert h.write(datas) == [len(d) for d in datas]           # every write is two pieces; src shifts 1, 3, 5 ...
    p = h.plan_encode([1] * len(ks), len(ks))
    assert [s for _, _, s in p["packets"]] == [[(s, 1432)] for s in starts]
    flat = np.concatenate([np.frombuffer(d, np.uint8) for d in datas] + [np.zeros(16, np.uint8)])
    offs = np.cumsum([0] + [len(d) for d in datas])
    buf, lens, status = _flat_encode(enc, p, _put(flat), {(i, 0): int(offs[i]) for i in range(len(ks))}, 1488, True,
                                     None)
    assert torch.equal(buf[:len(ks)], p["wire"]) and torch.equal(lens, p["wire_lens"]) and not status.any().item()
    h.close()


@pytest.mark.gpu
def test_wrap_rounds_write_plan_encode_release(enc, pad_bytes):
    """Several write / plan / encode / release rounds in a 4,096-B window:
    tail, write_pos and base lap the ring, writes go partial and two-piece,
    segments straddle the wrap."""
    rng = np.random.default_rng(6)
    h = TxHarness(enc, [4096], rq_caps=4)
    r = h.rules[0]
    straddles = partial = 0
    for rnd in range(9):
        n = int(rng.integers(900, 3500))
        got = h.write([_data(rng, n)], shifts=[int(rng.integers(0, 16))])
        partial += got[0] < n
        p = h.plan_encode([int(rng.integers(1, 4))], 4, pad=pad_bytes if rnd % 2 else None, framed=rnd % 2 == 0)
        for _, _, segs in p["packets"]:
            straddles += any((o & 4095) + l > 4096 for o, l in segs)
        if rnd == 4:
            o, l = p["packets"][0][2][0]
            assert h.retransmit([(0, o + 3, l - 3)]) == [tr.RQ_QUEUED]
        h.release([r.write_pos - int(rng.integers(0, 300))])
    assert straddles >= 3 and partial >= 1 and r.tail > 3 * 4096 and r.bytes_retransmitted > 0
    h.close()


@pytest.mark.gpu
def test_rule_boundaries(enc):
    """rem == H and H + 1; a queue entry that exactly fills a packet and one
    byte more; an entry over three packets (M = 64); pending an exact multiple
    of M - H; the max_segments closure; budget 0."""
    rng = np.random.default_rng(7)
    M = 1436
    h = TxHarness(enc, [16384] * 7, rq_caps=8)
    h.write([_data(rng, 9000)] * 6 + [_data(rng, 2 * (M - 4))])
    h.plan_encode([3] * 6 + [0], 32)
    assert [r.write_pos for r in h.rules] == [3 * 1432] * 6 + [0]
    st = h.retransmit([(0, 0, M - 8), (1, 0, M - 9), (2, 5, M - 4), (3, 5, M - 3), (4, 7, 150)] +
                      [(5, 10 * k, 1) for k in range(7)])
    assert st == [tr.RQ_QUEUED] * 12
    p = h.plan_encode([1, 1, 1, 2, 0, 0, 9], 32)
    by = {}
    for c, _, segs in p["packets"]:
        by.setdefault(c, []).append(segs)
    assert by[0] == [[(0, M - 8)]]                                     # rem == H: no new data
    assert by[1] == [[(0, M - 9), (3 * 1432, 1)]]                      # rem == H + 1: one byte
    assert by[2] == [[(5, M - 4)]]                                     # exactly fills the packet
    assert by[3] == [[(5, M - 4)], [(5 + M - 4, 1), (3 * 1432, M - 4 - 1 - 4)]]   # one byte more
    assert 4 not in by and 5 not in by                                 # budget 0
    assert by[6] == [[(0, M - 4)], [(M - 4, M - 4)]] and p["count_np"][6] == 2   # an exact multiple: no third packet
    p = h.plan_encode([0, 0, 0, 0, 4, 0, 0], 8, M=64, slot=96)
    assert [s for _, _, s in p["packets"]] == [[(7, 60)], [(67, 60)], [(127, 30), (3 * 1432, 26)], [(3 * 1432 + 26, 60)]]
    p = h.plan_encode([0, 0, 0, 0, 0, 3, 0], 8, max_segments=3)
    assert [len(s) for _, _, s in p["packets"]] == [3, 3, 2] and p["packets"][2][2][0] == (60, 1)
    h.close()


@pytest.mark.gpu
def test_budget_clamp_by_max_packets(enc):
    """budget_eff cut in the middle of a member and exactly between two
    members; the clamp counts budgets, not packets."""
    rng = np.random.default_rng(8)
    h = TxHarness(enc, [8192] * 3, rq_caps=2)
    h.write([_data(rng, 8000), _data(rng, 8000), _data(rng, 8000)])
    p = h.plan([3, 3, 3], 4)                       # eff 3, 1, 0
    assert p["count_np"] == [3, 1, 0] and p["first_np"] == [0, 3, 4]
    p = h.plan([2, 5, 5], 2)                       # exactly between two members: eff 2, 0, 0
    assert p["count_np"] == [2, 0, 0] and p["first_np"] == [0, 2, 2]
    p = h.plan([4, 2, 1], 5)                       # member 0 has one packet left: its budget still counts 4
    assert p["count_np"] == [1, 1, 0] and p["first_np"] == [0, 1, 2]
    p = h.plan([0xFFFFFFFF, 1, 7], 3)              # the budgets before member 2 sum to 2^32, not to 0
    assert p["count_np"] == [0, 0, 0] and h.rules[2].write_pos == 0
    p = h.plan([1, 1, 1], 0)                       # no room at all: nothing written, total 0
    assert p["count_np"] == [0, 0, 0]
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nconn", [3, 1025, 32769])
def test_many_connections(enc, nconn):
    """The scans cross a block (1,025) and a second level (32,769): unequal
    windows (4 KiB to 4 MiB), unequal budgets and pending sizes, idle members
    between busy ones.  All records and outputs compared; the windows of a
    chosen subset copied out."""
    rng = np.random.default_rng(nconn)
    caps = [4096] * nconn
    big = sorted({0, nconn // 2, nconn - 1})
    for c, cap in zip(big, (1 << 22, 65536, 16384)):
        caps[c] = cap
    watch = sorted(set(big) | {1 % nconn, nconn - 2, min(1023, nconn - 1), min(1024, nconn - 1)})
    h = TxHarness(enc, caps, rq_caps=4, watch=watch, starts=[int(rng.integers(0, 1 << 20)) for _ in range(nconn)])
    busy = rng.random(nconn) < (1.0 if nconn == 3 else 0.15)
    busy[big] = True
    busy[1 % nconn] = False                                  # an idle member between busy ones
    blob = _data(rng, 70000)
    datas = [blob[:int(rng.integers(1, 5000))] if busy[c] else b"" for c in range(nconn)]
    datas[0] = blob[:70000]                                  # the 4 MiB window: many packets from one member
    nw = h.write(datas)
    assert nw[big[-1]] == len(datas[big[-1]]) and max(nw[1:]) <= 4999
    budgets = [int(rng.integers(0, 5)) for _ in range(nconn)]
    budgets[0] = 30
    total_max = sum(min(b, -(-n // 1432)) for b, n in zip(budgets, nw))
    p = h.plan_encode(budgets, sum(budgets) + 37)            # the tail of conn_of is NO_CONN (compared in plan)
    assert len(p["packets"]) == total_max and p["count_np"][0] == 30 and p["count_np"][1 % nconn] == 0
    idle = [c for c in range(nconn) if p["count_np"][c] == 0]
    assert len(idle) >= 1 and all(h.rules[c].packets == 0 for c in idle)
    # a second batch: retransmissions in some members, the rest goes on; max_packets cuts the set short
    ent = [(c, h.rules[c].base, min(200, h.rules[c].write_pos - h.rules[c].base))
           for c in range(nconn) if h.rules[c].write_pos > h.rules[c].base and c % 3 == 0]
    assert set(h.retransmit(ent)) == {tr.RQ_QUEUED}
    p2 = h.plan_encode([3] * nconn, 2 * nconn + 5 if nconn > 3 else 7)
    assert 0 in p2["count_np"][:-1] and len(p2["packets"]) > 0
    h.release([r.write_pos for r in h.rules])
    h.close()


@pytest.mark.gpu
def test_across_2_32(enc, pad_bytes):
    """A member that starts at 2^32 - 4500 beside one at 0 (and one below
    2^35, where the offset's uvarint does grow a byte and the segment data
    shifts phase): segments that end at the power of two, start there and
    straddle it."""
    rng = np.random.default_rng(9)
    for top in (1 << 32, 1 << 35):
        s = top - 4500
        h = TxHarness(enc, [16384, 16384], rq_caps=4, starts=[s, 0], pns=[(1 << 32) - 2, 0])
        h.write([_data(rng, 9000), _data(rng, 9000)])
        p = h.plan_encode([4, 2], 8, pad=pad_bytes, framed=False)
        offs = [segs[0][0] for c, _, segs in p["packets"] if c == 0]
        assert offs == [s + 1432 * k for k in range(4)] and offs[3] < top < offs[3] + 1432     # one straddles
        assert [pn for c, pn, _ in p["packets"] if c == 0] == [(1 << 32) - 1 + k for k in range(4)]
        assert h.retransmit([(0, top - 100, 100), (0, top, 50), (0, top - 7, 14)]) == [tr.RQ_QUEUED] * 3
        p = h.plan_encode([2, 2], 8)
        assert p["packets"][0][2][:3] == [(top - 100, 100), (top, 50), (top - 7, 14)]
        if top == 1 << 35:
            assert len(pr.put_uvarint(top - 1)) + 1 == len(pr.put_uvarint(top))
        h.release([top + 10, 0])
        assert h.rules[0].base == top + 10
        h.close()


@pytest.mark.gpu
def test_encode_lying_descriptors(enc):
    """A segment below base, past tail, with offset + len wrapping 2^64;
    conn_of >= nconn between valid packets of other members; n_segments >
    max_segments: the stated status, an untouched slot, wire_lens 0, the
    neighbours bit-exact (all compared inside the harness)."""
    rng = np.random.default_rng(10)
    h = TxHarness(enc, [8192, 4096], rq_caps=2, starts=[5000, 100])
    h.write([_data(rng, 6000), _data(rng, 3000)])
    p = h.plan([4, 2], 16, max_segments=2)
    h.release([5000 + 1432, 0])                     # member 0: base 6432, tail 11000
    n = len(p["packets"])
    assert n == 6
    good_i, good_s, good_c = p["info_np"][:n].copy(), p["segs_np"][:n].copy(), p["conn_np"][:n].copy()
    info, segs, conn = [], [], []

    def add(i, patch=None, c=None):
        I, S = good_i[i].copy(), good_s[i].copy()
        if patch:
            patch(I, S)
        info.append(I)
        segs.append(S)
        conn.append(good_c[i] if c is None else c)

    def seg(j, off, ln):
        def f(I, S):
            S[j]["offset"], S[j]["len"] = off & tr.M64, ln
            I["n_segments"] = max(int(I["n_segments"]), j + 1)
        return f

    def nseg(k):
        def f(I, S):
            I["n_segments"] = k
        return f

    lies = [(0, None, None, fec.PKT_OUT_OF_WINDOW),                     # released: below base
            (1, seg(0, 6431, 10), None, fec.PKT_OUT_OF_WINDOW),         # starts one byte below base
            (2, seg(0, 10990, 11), None, fec.PKT_OUT_OF_WINDOW),        # ends one byte past tail
            (2, seg(1, 11001, 0), None, fec.PKT_OUT_OF_WINDOW),         # an empty segment past tail
            (3, seg(0, tr.M64 - 3, 8), None, fec.PKT_OUT_OF_WINDOW),    # offset + len wraps 2^64
            (3, seg(0, 9000, 0xFFFF), None, fec.PKT_OUT_OF_WINDOW),
            (1, None, 2, 0), (1, None, NO_CONN, 0), (4, None, 0x80000000, 0),   # no member: status 0, nothing written
            (2, nseg(3), None, fec.PKT_CAPACITY), (5, nseg(0xFFFF), None, fec.PKT_CAPACITY),
            (4, seg(0, 100, 3000), None, 0),                            # member 1, whole window: a valid packet
            (4, seg(0, 100, 3001), None, fec.PKT_OUT_OF_WINDOW),
            (2, seg(1, 11000, 0), None, 0)]                             # an empty segment at tail is the caller's FIN
    want = []
    for i, patch, c, st in lies:                   # every case between two good neighbours of another member
        add(4 if good_c[i] == 0 else 1)
        add(i, patch, c)
        want += [0, st]
    add(2)
    want.append(0)
    info, segs, conn = np.array(info), np.array(segs), np.array(conn, np.uint32)
    _, lens, st = h.encode(info, segs, conn, len(info), slot=3072)
    assert st.tolist() == want
    h.close()


@pytest.mark.gpu
def test_retransmit_and_release(enc):
    """Order kept within a connection, every reject reason, queue full in
    mid-list, an unsorted list applies nothing; release held back by a queued
    entry and by write_pos."""
    rng = np.random.default_rng(11)
    h = TxHarness(enc, [8192, 8192, 4096], rq_caps=[3, 5, 2], starts=[1000, 0, 50])
    h.write([_data(rng, 5000), _data(rng, 5000), _data(rng, 100)])
    h.plan_encode([2, 3, 1], 8)                    # write_pos: 3864, 4296, 150
    before = [r.record() for r in h.rules]
    assert set(h.retransmit([(0, 1000, 10), (1, 0, 10), (0, 1100, 10)])) == {tr.RQ_UNSORTED}
    assert [r.record() for r in h.rules] == before
    st = h.retransmit([(0, 2000, 30), (0, 1000, 40), (0, 999, 5), (0, 3860, 5), (0, 3000, 0), (0, 3000, 0x10000),
                       (0, 1 << 63, 9), (0, 3863, 1), (0, 1500, 1), (0, 1500, 0), (1, 4000, 296), (1, 5, 5),
                       (2, 60, 5), (2, 50, 100), (2, 70, 1), (3, 0, 1), (7, 0, 1), (NO_CONN, 0, 1)])
    Q, R, F = tr.RQ_QUEUED, tr.RQ_REJECTED, tr.RQ_FULL
    assert st == [Q, Q, R, R, R, R, R, Q, F, F, Q, Q, Q, Q, F, R, R, R]
    assert [tuple(q) for q in h.rules[0].queue] == [(2000, 30), (1000, 40), (3863, 1)]      # list order kept
    assert [r.rq_rejected for r in h.rules] == [7, 0, 1]
    h.release([1 << 40, 4200, 0])
    assert [r.base for r in h.rules] == [1000, 5, 50]        # held by the lowest queued entry; member 2 asked for 0
    p = h.plan_encode([1, 1, 1], 4)
    assert p["packets"][0][2][:3] == [(2000, 30), (1000, 40), (3863, 1)] and p["packets"][1][2][:2] == [(4000, 296), (5, 5)]
    h.release([1 << 40, 1 << 40, 1 << 40])
    assert [r.base for r in h.rules] == [r.write_pos for r in h.rules]          # and by write_pos
    st = h.retransmit([(2, 50, 10)])
    assert st == [R]                                          # released bytes cannot be retransmitted
    h.close()


@pytest.mark.gpu
def test_argument_errors_on_the_device(enc):
    """INVALID_ARG before any launch, with nothing written: pageable operands,
    a max_payload below 16, max_segments 0, a framed encode with a pad, a
    duplicate member."""
    lib = fec.load_library()
    bad = fec.ErrInvalidArg.code
    h = TxHarness(enc, [4096, 4096], rq_caps=2)
    out_set = ctypes.c_void_p(1)
    twice = (ctypes.c_void_p * 2)(h.txs[0]._h.value, h.txs[0]._h.value)
    assert lib.ugo_fec_stream_tx_set_create(enc._h, ctypes.addressof(twice), 2, ctypes.byref(out_set)) == bad
    assert out_set.value is None
    with pytest.raises(ValueError):
        fec.StreamTxSet(enc, [h.txs[0], h.txs[0]])
    out = {k: torch.full((8 * w,), 0x11, dtype=torch.uint8, device="cuda")
           for k, w in (("info", 64), ("segs", 32), ("conn", 4), ("first", 8), ("count", 4), ("total", 8))}
    budget = torch.ones(2, dtype=torch.int32, device="cuda")
    host = torch.ones(2, dtype=torch.int32)                   # pageable

    def plan(b, M, ms, mp=8):
        return lib.ugo_fec_stream_tx_set_plan(h.set._h, b.data_ptr(), M, ms, mp, out["info"].data_ptr(),
                                              out["segs"].data_ptr(), out["conn"].data_ptr(), out["first"].data_ptr(),
                                              out["count"].data_ptr(), out["total"].data_ptr(), None)
    assert plan(budget, 15, 2) == bad and plan(budget, 0x10000, 2) == bad and plan(budget, 1436, 0) == bad
    assert plan(host, 1436, 2) == bad and plan(budget, 1436, 2, (1 << 31) + 1) == bad
    n64 = torch.zeros(2, dtype=torch.int64, device="cuda")
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.ugo_fec_stream_tx_set_write(h.set._h, torch.zeros(64, dtype=torch.uint8).data_ptr(), n64.data_ptr(),
                                           n64.data_ptr(), n64.data_ptr(), None) == bad
    assert lib.ugo_fec_stream_tx_set_write(h.set._h, src.data_ptr(), None, n64.data_ptr(), n64.data_ptr(), None) == bad
    assert lib.ugo_fec_stream_tx_set_release(h.set._h, torch.zeros(2, dtype=torch.int64).data_ptr(), None) == bad
    wire = torch.full((2, 64), 0x11, dtype=torch.uint8, device="cuda")
    pad = torch.zeros(64, dtype=torch.uint8, device="cuda")
    z = torch.zeros(256, dtype=torch.uint8, device="cuda")
    args = lambda slot, flags, p: (h.set._h, z.data_ptr(), None, 0, z.data_ptr(), 1, z.data_ptr(), 2, p, flags,  # noqa: E731
                                   wire.data_ptr(), slot, z.data_ptr(), z.data_ptr(), None)
    assert lib.ugo_fec_stream_tx_set_encode(*args(64, fec.PKT_FEC_FRAMED, pad.data_ptr())) == bad
    assert lib.ugo_fec_stream_tx_set_encode(*args(60, 0, None)) == bad
    assert lib.ugo_fec_stream_tx_set_encode(*args(64, 2, None)) == bad
    torch.cuda.synchronize()
    assert all(bool((t == 0x11).all()) for t in out.values()) and bool((wire == 0x11).all())
    h.check()
    h.close()


@pytest.mark.gpu
def test_pinned_operands_and_kernel_classes(enc, pad_bytes):
    """Every operand array in pinned host memory (the windows stay on the
    device), and what the launches report as: write, release, retransmit and
    plan as UGO_FEC_KERNEL_STREAM_TX, set_encode as UGO_FEC_KERNEL_PACKET_ENCODE."""
    rng = np.random.default_rng(13)
    h = TxHarness(enc, [8192, 4096], rq_caps=2, starts=[7000, 0])
    enc.timing_begin(64)
    try:
        assert h.write([_data(rng, 5000), _data(rng, 4500)], where="pinned") == [5000, 4096]
        h.plan_encode([2, 1], 6, pad=pad_bytes, framed=False, where="pinned")
        assert h.retransmit([(0, 7100, 300), (1, 8, 90)], where="pinned") == [tr.RQ_QUEUED] * 2
        h.release([7050, 1432], where="pinned")
        assert [r.base for r in h.rules] == [7050, 8]
        p = h.plan_encode([3, 3], 8, where="pinned")
    finally:
        recs, untimed = enc.timing_end()
    assert len(p["packets"]) == 4 and untimed == 0
    tx, pe = fec.KERNEL_IDS["stream_tx"], fec.KERNEL_IDS["packet_encode"]
    assert (tx, pe) == (11, 8)
    assert recs["kernel"].tolist() == [tx] * 2 + [tx] * 6 + [pe] + [tx] * 2 + [tx] + [tx] * 6 + [pe]
    h.close()


@pytest.mark.gpu
def test_round_trip_write_to_read(enc, pad_bytes):
    """write -> plan -> set_encode (framed) -> tx_assemble -> rx_assemble (no
    loss) -> packet_decode -> stream_set_deliver -> set_read returns, for three
    connections, the bytes written, with one retransmitted segment delivered as
    a duplicate."""
    rng = np.random.default_rng(12)
    d, p_, n, S, slot = 10, 3, 13, 1470, 1488
    h = TxHarness(enc, [16384, 16384, 16384], rq_caps=4)
    first = [_data(rng, 500), _data(rng, 700), _data(rng, 900)]
    h.write(first)
    a = h.plan_encode([1, 1, 1], 3, max_segments=2)
    rest = [_data(rng, 8092), _data(rng, 7000), _data(rng, 6500)]
    h.write(rest)
    assert h.retransmit([(1, 0, 700)]) == [tr.RQ_QUEUED]       # as if member 1's first packet had been lost
    b = h.plan_encode([9, 9, 9], 27, max_segments=2)
    assert b["packets"][b["first_np"][1]][2] == [(0, 700), (700, 1436 - 704 - 4)]
    assert len(b["packets"]) == 17 and all(r.write_pos == r.tail for r in h.rules)
    pkts = torch.cat([a["wire"], b["wire"]])
    lens = torch.cat([a["wire_lens"], b["wire_lens"]])
    conn = np.concatenate([a["conn_np"][:3], b["conn_np"][:17]]).astype(np.int64)
    G = 2
    dpad = _put(np.frombuffer(pad_bytes, np.uint8)[:slot].copy())
    wire = torch.zeros((G * n, slot), dtype=torch.uint8, device="cuda")
    wl = torch.zeros(G * n, dtype=torch.int16, device="cuda")
    st = torch.full((G,), -1, dtype=torch.int8, device="cuda")
    enc.tx_assemble(pkts.contiguous(), lens, wire, wl, first_seq=0, pad=dpad, status=st)
    assert st.tolist() == [0, 0]
    frames = torch.zeros((n, G, slot), dtype=torch.uint8, device="cuda")
    present = torch.zeros(G, dtype=torch.int64, device="cuda")
    enc.rx_assemble(wire, wl, frames, present, shard_size=S, pad=dpad, frames=True)
    assert present.tolist() == [(1 << n) - 1] * G
    rows = frames[:d].reshape(d * G, slot)                      # row k * G + g is data packet g * d + k
    order = np.array([g * d + k for k in range(d) for g in range(G)])
    rl = wl.view(G, n)[:, :d].t().contiguous().view(-1)
    info, _, segs = enc.packet_decode(rows, rl, framed=True, max_ranges=1, max_segments=2)
    I = info.cpu().numpy().view(fec.PKT_INFO_DTYPE).reshape(-1)
    assert not I["status"].any() and (I["payload_off"] == 6).all()
    rxs = [fec.StreamRx(enc, 16384) for _ in range(3)]
    rset = fec.StreamRxSet(enc, rxs)
    # the receiver sees the packets in sending order (the rows, read group by group)
    back = torch.from_numpy(np.argsort(order)).cuda()
    status = rset.deliver(rows[back].contiguous(), info[back].contiguous(), segs[back].contiguous(),
                          _put(conn.astype(np.uint32).view(np.int32)))
    st = status.cpu().numpy()
    dup = 3 + b["first_np"][1]
    assert st[dup, 0] == sr.DUPLICATE and (np.delete(st, dup, 0)[np.delete(st, dup, 0) != 0] == sr.ACCEPTED).all()
    want = [x + y for x, y in zip(first, rest)]
    sizes = torch.tensor([len(w) + 5 for w in want], dtype=torch.int64, device="cuda")
    offs = torch.tensor([0, 10000, 20000], dtype=torch.int64, device="cuda")
    dst = torch.zeros(30000, dtype=torch.uint8, device="cuda")
    n_read, _ = rset.read(sizes, dst=dst, dst_off=offs)
    assert n_read.tolist() == [len(w) for w in want]
    got = dst.cpu().numpy()
    for c, w in enumerate(want):
        assert got[10000 * c:10000 * c + len(w)].tobytes() == w, c
    rset.close()
    for rx in rxs:
        rx.close()
    h.close()
