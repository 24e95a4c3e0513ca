"""Sent histories (include/ugo_sent.h): THE RULE against a restatement of
packetSender on the CPU, and the device against one rule per member."""
import ctypes
import random
import re

import numpy as np
import pytest

import ack_ref as ar
import sent_ref as sr
from sent_ref import Ack
from ugo_amd import fec


# ---------------------------------------------------------------- CPU: the rule against the reference
def _sack(peer, w, delay=0):
    la, lio, rows, _ = peer.view()
    return Ack(la, lio, rows, w, delay)


def run_family(seed, shuffle=False, rto=False, one_per_call=False):
    """One seeded sequence: bursts sent, 0-20 % lost, a SACK on 60 % of the
    arrivals (RuleAck is the peer), 1-4 ACKs a call, a drain after every call.
    Returns (compared states, states that differ)."""
    rng = random.Random(seed)
    loss = rng.uniform(0.0, 0.2)
    go, rule, peer = sr.GoSender(), sr.RuleSent(1024, 1), ar.RuleAck(1024)
    nxt, w, now = 1, 0, 1000
    compared = differ = 0
    for _ in range(rng.randint(4, 30)):
        burst = list(range(nxt, nxt + rng.randint(1, 12)))
        nxt = burst[-1] + 1
        now += 1000
        sw = rule.attach(True)[1]
        go.GetStopWaitingFrame()
        for n in burst:
            go.sentPacket(sr._GoPacket(n, 100), now)
        rule.record([(n, 100, 0, 0, [(10 * n, 10)]) for n in burst], now)
        acks = []
        for k, n in enumerate(burst):
            if rng.random() >= loss:
                peer.receive([(n, sw if k == 0 else 0)])
                if rng.random() < 0.6:
                    w += 1
                    acks.append(_sack(peer, w))
        while acks:
            k = 1 if one_per_call else rng.randint(1, 4)
            call, acks = acks[:k], acks[k:]
            if shuffle:
                rng.shuffle(call)
            now += 10
            rule.ack(call, now)
            for a in (sorted(call, key=lambda a: a.la) if shuffle and not one_per_call else call):
                go.receivedAck(a, a.w)
            if rto and rng.random() < 0.1:
                now += 600_000
                fired = rule.rto(0, now)
                assert bool(go.checkRTO(0, now)) == bool(fired)
            assert go.drain_all() == rule.drain()[0]
            compared += 1
            differ += go.view() != rule.view()
    return compared, differ


def test_in_order_family_equals_the_reference():
    total = bad = 0
    for seed in range(400):
        c, d = run_family(seed)
        total, bad = total + c, bad + d
    assert total > 5000 and bad == 0, (total, bad)


def test_shuffled_family_equals_the_reference_on_sorted_acks():
    total = bad = 0
    for seed in range(400):
        c, d = run_family(10_000 + seed, shuffle=True)
        total, bad = total + c, bad + d
    assert total > 5000 and bad == 0, (total, bad)


def test_one_ack_per_call_equals_the_acceptance_chain_in_any_order():
    total = bad = 0
    for seed in range(200):
        c, d = run_family(20_000 + seed, shuffle=True, one_per_call=True)
        total, bad = total + c, bad + d
    assert total > 2000 and bad == 0, (total, bad)


def test_rto_family_equals_the_reference():
    """With an RTO after every tenth call.  Every call is followed by a drain, so
    no queued packet is left under lio for a later ACK and deviation (b) cannot
    arise; checkRTO then picks the same packet and leaves the same state."""
    total = bad = 0
    for seed in range(300):
        c, d = run_family(30_000 + seed, rto=True)
        total, bad = total + c, bad + d
    assert total > 5000 and bad == 0, (total, bad)


def _pair(numbers, length=100):
    go, rule = sr.GoSender(), sr.RuleSent(1024, 2)
    for n in numbers:
        go.sentPacket(sr._GoPacket(n, length), 5)
    rule.record([(n, length, 0, 0, [(10 * n, 10)]) for n in numbers], 5)
    return go, rule


def test_deviation_a_an_overtaken_ack_counts():
    go, rule = _pair(range(1, 9))
    a6, a8 = Ack(6, 0, [(2, 6), (0, 0)], 1), Ack(8, 0, [(2, 8), (0, 0)], 2)
    go.receivedAck(a8, 2), go.receivedAck(a6, 1)
    rule.ack([a8, a6], 9)
    assert go.packetHistory[1].missingCount == 1 and rule.slots[1]["missing"] == 2


def test_deviation_b_a_queued_packet_under_lio_is_freed():
    go, rule = _pair(range(1, 4))
    assert go.checkRTO(0, 600_000) == 1 and rule.rto(0, 600_000) == 1
    a = Ack(2, 0, [(2, 2), (0, 0)], 1)
    go.receivedAck(a, 1), rule.ack([a], 650_000)
    assert go.largestInOrderAcked == rule.lio == 2                   # past the queued packet 1
    go.receivedAck(Ack(3, 3, [], 2), 2)
    rule.ack([Ack(3, 3, [], 2)], 700_000)
    assert go.drain_all() == [1] and rule.drain()[0] == []           # the reference sends it again
    assert rule.tracked == 0 and rule.bytes_in_flight == 0


def test_deviation_c_window_bound_and_collision():
    rule = sr.RuleSent(1024, 1)
    rule.record([(n, 10, 0, 0, []) for n in (1, 1024)], 1)
    assert not rule.err and rule.tracked == 2
    rule.record([(1025, 10, 0, 0, []), (1000, 10, 0, 0, [])], 2)     # lio + Ws + 1; 1000 did fit
    assert rule.err == sr.TOO_MANY_TRACKED and 1000 in rule.slots and 1025 not in rule.slots
    before = rule.record_fields()
    rule.record([(2, 10, 0, 0, [])], 3)
    assert rule.ack([Ack(1, 1)], 4)["accepted"] == 0 and rule.rto(0, 10 ** 9) == 0
    assert rule.record_fields() == before                            # inert


def test_deviation_d_one_rtt_sample_and_lost_then_acked():
    go, rule = _pair(range(1, 10))
    acks = [Ack(la, 0, [(2, la), (0, 0)], la) for la in (5, 6, 7, 8)] + [Ack(9, 9, [], 9, delay=77)]
    go_acked, go_lost = [], []
    for a in acks:
        _, ak, lo = go.receivedAck(a, a.w)
        go_acked, go_lost = go_acked + ak, go_lost + lo
    assert go_lost == [1] and go.drain_all() == [1]                  # the reference reports it lost and resends it
    ev = rule.ack(acks, 105)
    assert (ev["has_rtt"], ev["rtt_us"], ev["delay_us"]) == (1, 100, 77)
    assert (ev["acked_packets"], ev["lost_packets"]) == (9, 0) and rule.tracked == 0 and not rule.sw_pending
    assert rule.drain()[0] == []


def test_deviation_i_acked_counts_a_freed_retransmission():
    go, rule = _pair(range(1, 10))
    first = [Ack(la, 0, [(2, la), (0, 0)], la) for la in (5, 6, 7, 8)]
    for a in first:
        go.receivedAck(a, a.w)
    rule.ack(first, 50)                                              # packet 1 is queued in both
    last = Ack(9, 9, [], 9)
    go.receivedAck(last, 9)
    ev = rule.ack([last], 60)                                        # ... and acknowledged before the drain
    assert go.totalAcked == 800 and rule.acked_bytes == 900 and ev["acked_packets"] == 2
    assert go.bytesInFlight == rule.bytes_in_flight == 0


def test_deviation_e_missing_saturates():
    rule = sr.RuleSent(1024, 1)
    rule.record([(n, 10, 0, 0, []) for n in range(1, 301)], 1)
    for la in range(2, 301):
        rule.ack([Ack(la, 0, [(2, la), (0, 0)])], 2)
    assert rule.slots[1]["missing"] == 255 and rule.slots[1]["state"] == sr.QUEUED


def test_deviation_f_ascending_drain_and_g_pending_without_a_packet():
    go, rule = _pair(range(1, 12))
    acks = [Ack(la, 0, [(4, la), (2, 2), (0, 0)], la) for la in (8, 9, 10, 11)]
    rule.ack(acks, 9)
    for a in acks:
        go.receivedAck(a, a.w)
    assert rule.drain()[0] == [1, 3]
    assert [go.dequeuePacketForRetransmission().packetNumber for _ in range(2)] == [3, 1]   # a stack
    assert rule.sw_pending and rule.attach(False) == (0, 0) and rule.sw_pending
    assert rule.attach(True) == (1, rule.lio + 1) and not rule.sw_pending


def test_deviation_h_lio_passes_what_is_no_longer_in_flight():
    go, rule = _pair([1, 2, 4, 5])                                   # 3 was never sent
    a = Ack(2, 2, [], 1)
    go.receivedAck(a, 1), rule.ack([a], 9)
    assert go.largestInOrderAcked == 2 and rule.lio == 3


def test_rto_arithmetic():
    rule = sr.RuleSent(1024, 1)
    assert rule.rto_us(0) == 500_000 and rule.rto_us(1) == 200_000 and rule.rto_us(10 ** 12) == 60_000_000
    rule.rto_count = 1
    assert rule.rto_us(0) == 1_000_000
    rule.rto_count = 9
    assert rule.rto_us(0) == 60_000_000 and rule.rto_us(1) == 60_000_000
    rule.rto_count = 8
    assert rule.rto_us(1) == 51_200_000


def test_layouts_and_constants():
    d = fec.SENT_STATE_DTYPE
    assert d.itemsize == 160 and d.names[:21] == sr.RuleSent.FIELDS
    assert [d.fields[n][1] for n in d.names] == list(range(0, 120, 8)) + [120, 124, 128, 132, 136, 137, 138]
    e = fec.SENT_EVENT_DTYPE
    assert e.itemsize == 64 and e.names[:10] == sr.RuleSent.EVENT_FIELDS
    assert [e.fields[n][1] for n in e.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 57, 58]
    s = fec.SENT_SLOT_DTYPE
    assert s.itemsize == 32 and [s.fields[n][1] for n in s.names] == [0, 8, 16, 24, 28, 29, 30, 31]
    assert fec.SENT_SEG_DTYPE.itemsize == 16
    src = open(fec.SENT_HEADER_PATH).read()
    assert re.search(r"#define UGO_FEC_KERNEL_SENT 13\b", src)
    assert "(160 bytes)" in src and "(32 bytes)" in src and "(64 bytes)" in src
    assert fec.KERNEL_NAMES[13] == "sent" and fec.KERNEL_IDS["sent"] == 13
    assert "UGO_FEC_KERNEL_SENT" in open(fec.HEADER_PATH).read()
    assert (fec.SENT_RTO_DEFAULT_US, fec.SENT_RTO_MIN_US, fec.SENT_RTO_MAX_US) == \
        (sr.RTO_DEFAULT_US, sr.RTO_MIN_US, sr.RTO_MAX_US)


def test_symbols_are_exported_within_abi_9():
    lib = fec.load_library()
    names = [s for s in fec.header_symbols() if s.startswith("ugo_fec_sent_")]
    assert sorted(names) == ["ugo_fec_sent_set_ack", "ugo_fec_sent_set_attach", "ugo_fec_sent_set_create",
                             "ugo_fec_sent_set_destroy", "ugo_fec_sent_set_drain", "ugo_fec_sent_set_record",
                             "ugo_fec_sent_set_rto", "ugo_fec_sent_set_state", "ugo_fec_sent_tx_create",
                             "ugo_fec_sent_tx_destroy", "ugo_fec_sent_tx_scratch", "ugo_fec_sent_tx_segments",
                             "ugo_fec_sent_tx_slots"]
    for s in names:
        assert hasattr(lib, s), s
    assert lib.ugo_fec_abi_version() == 9


def test_argument_errors_that_need_no_launch():
    lib = fec.load_library()
    h = ctypes.c_void_p(1)
    assert lib.ugo_fec_sent_tx_create(None, 1024, 4, ctypes.byref(h)) == 6 and h.value is None
    assert lib.ugo_fec_sent_tx_create(None, 1024, 4, None) == 6
    assert lib.ugo_fec_sent_tx_slots(None, None, None) == 6
    assert lib.ugo_fec_sent_tx_segments(None, None, None, None) == 6
    assert lib.ugo_fec_sent_tx_scratch(None, None, None) == 6
    h = ctypes.c_void_p(1)
    assert lib.ugo_fec_sent_set_create(None, None, 1, ctypes.byref(h)) == 6 and h.value is None
    assert lib.ugo_fec_sent_set_record(None, None, None, 1, None, None, None, 1, 0, None) == 6
    assert lib.ugo_fec_sent_set_ack(None, None, None, 0, None, 1, 0, None, None) == 6
    assert lib.ugo_fec_sent_set_rto(None, None, 0, None, None) == 6
    assert lib.ugo_fec_sent_set_drain(None, 0, None, None, None, None, None, None, None) == 6
    assert lib.ugo_fec_sent_set_attach(None, None, None, 0, None, None, None) == 6
    assert lib.ugo_fec_sent_set_state(None, None) == 6
    lib.ugo_fec_sent_tx_destroy(None)
    lib.ugo_fec_sent_set_destroy(None)
    for ws, cap in ((0, 1), (512, 1), (1536, 1), ((1 << 20) + 1, 1), (1 << 21, 1), (1024, 0), (1024, 17)):
        with pytest.raises(ValueError):
            fec.SentTx.check_create(ws, cap)
    for ws, cap in ((1024, 1), (4096, 16), (1 << 20, 8)):
        fec.SentTx.check_create(ws, cap)
    with pytest.raises(ValueError):
        fec.SentTxSet.check_members(None, [])


# ---------------------------------------------------------------- CPU: undrained runs and truncated SACKs
from sent_ref_b import GoSenderB  # noqa: E402


def run_family_b(seed, p_drain, p_rto, shuffle, make_go=GoSenderB, max_ranges=None, truncated=None):
    """run_family's loop with three changes: the drain after a call happens with
    probability p_drain, an RTO with probability p_rto, and the reference is
    make_go().  With max_ranges the peer's SACK is RuleAck.sack(max_ranges), and
    truncated[0] counts the truncated ones.  Compares view() after every call,
    the drained numbers at every drain and whether the RTO fired.  Returns
    (compared states, states that differ)."""
    rng = random.Random(seed)
    loss = rng.uniform(0.0, 0.2)
    go, rule, peer = make_go(), sr.RuleSent(1024, 1), ar.RuleAck(1024)
    nxt, w, now = 1, 0, 1000
    compared = differ = 0

    def sack(w):
        if max_ranges is None:
            return _sack(peer, w)
        la, _, rows, how = peer.sack(max_ranges)
        truncated[0] += how == ar.TRUNCATED
        return Ack(la, peer.lio, rows, w, 0)

    for _ in range(rng.randint(4, 30)):
        burst = list(range(nxt, nxt + rng.randint(1, 12)))
        nxt = burst[-1] + 1
        now += 1000
        sw = rule.attach(True)[1]
        go.GetStopWaitingFrame()
        for n in burst:
            go.sentPacket(sr._GoPacket(n, 100), now)
        rule.record([(n, 100, 0, 0, [(10 * n, 10)]) for n in burst], now)
        acks = []
        for k, n in enumerate(burst):
            if rng.random() >= loss:
                peer.receive([(n, sw if k == 0 else 0)])
                if rng.random() < 0.6:
                    w += 1
                    acks.append(sack(w))
        while acks:
            k = rng.randint(1, 4)
            call, acks = acks[:k], acks[k:]
            now += 10
            if shuffle:
                rng.shuffle(call)
            rule.ack(call, now)
            for a in (sorted(call, key=lambda a: a.la) if shuffle else call):
                go.receivedAck(a, a.w)
            bad = False
            if rng.random() < p_rto:
                now += 600_000
                fired = rule.rto(0, now)
                bad |= bool(go.checkRTO(0, now)) != bool(fired)
            if rng.random() < p_drain:
                bad |= go.drain_all() != rule.drain()[0]
            compared += 1
            differ += bad or go.view() != rule.view()
    return compared, differ


UNDRAINED = [(p, q, sh) for p in (1, 0.5, 0.1, 0) for q in (0.1, 0) for sh in (False, True)]


@pytest.mark.parametrize("p_drain,p_rto,shuffle", UNDRAINED)
def test_undrained_families_equal_the_reference_with_deviation_b(p_drain, p_rto, shuffle):
    """Queued packets stay under lio for later ACKs.  The rule equals the
    reference that carries deviation (b) and nothing else, in every state; the
    plain reference differs wherever a drain is left out, so the comparison is
    not empty."""
    total = bad = plain = 0
    for seed in range(300):
        c, d = run_family_b(30_000 + seed, p_drain, p_rto, shuffle)
        total, bad = total + c, bad + d
        if p_drain < 1:
            plain += run_family_b(30_000 + seed, p_drain, p_rto, shuffle, make_go=sr.GoSender)[1] > 0
    assert total > 5000 and bad == 0, (total, bad)
    assert p_drain == 1 or plain > 0, plain


@pytest.mark.parametrize("max_ranges,p_drain", [(3, 1), (3, 0), (2, 0)])
@pytest.mark.parametrize("p_rto", [0.1, 0])
@pytest.mark.parametrize("shuffle", [False, True])
def test_truncated_sacks_equal_the_reference_with_deviation_b(max_ranges, p_drain, p_rto, shuffle):
    """The same family with the peer's SACK cut to max_ranges rows by
    RuleAck.sack: deviation (h) against a truncated SACK."""
    total = bad = 0
    truncated = [0]
    for seed in range(300):
        c, d = run_family_b(30_000 + seed, p_drain, p_rto, shuffle, max_ranges=max_ranges, truncated=truncated)
        total, bad = total + c, bad + d
    assert truncated[0] > 0 and total > 5000 and bad == 0, (truncated[0], total, bad)


# ---------------------------------------------------------------- GPU
import torch  # noqa: E402

from sent_harness import NO_CONN, SentHarness, _put  # noqa: E402

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def enc(gpu):
    return fec.New(10, 3)


def A(c, la, lio, ranges=(), w=0, delay=0, status=0, flags=0x80, nr=None):
    return (status, c, flags, Ack(la, lio, ranges, w, delay), nr)


def holes(la, missing):
    """The rows a receiver that has everything up to la but `missing` sends."""
    rows, n = [], la
    have = [x for x in range(1, la + 1) if x not in missing]
    lio = 0
    while lio + 1 in have:
        lio += 1
    runs = []
    for x in sorted((x for x in have if x > lio), reverse=True):
        if runs and runs[-1][0] == x + 1:
            runs[-1][0] = x
        else:
            runs.append([x, x])
    rows = [tuple(r) for r in runs] + ([(lio, lio)] if runs else [])
    return lio, rows


@pytest.mark.gpu
def test_rings_window_bound_collision_and_2_32(enc):
    h = SentHarness(enc, [1024, 1024, 1024], 1)
    h.send(0, [1, 1024])                                  # lio + Ws fits
    st = h.send(0, [1025, 1000])                          # lio + Ws + 1 does not; 1000 did fit
    assert st["err"].tolist() == [1, 0, 0] and st["tracked"][0] == 3
    h.send(0, [5])                                        # inert
    # a collision: packet 1 of member 1 is queued and stays while lio moves on
    h.send(1, range(1, 9))
    h.ack([A(1, la, 0, [(2, la), (0, 0)], w=la) for la in (5, 6, 7, 8)], max_ranges=2)
    assert h.rules[1].slots[1]["state"] == sr.QUEUED and h.rules[1].lio == 8
    st = h.send(1, [1025])                                # <= lio + Ws, but slot 1 holds packet 1
    assert st["err"].tolist() == [1, 1, 0]
    # numbers on both sides of 2^32: member 2 starts at 2^32 - 300
    base = (1 << 32) - 300
    h.send(2, range(base, base + 600))
    lio, rows = base + 399, [(base + 450, base + 599), (base + 399, base + 399)]
    h.ack([A(2, base + 599, lio, rows, w=1)], max_ranges=2)
    st = h.set.states()
    assert st["lio"][2] == base + 399 and st["tracked"][2] == 50 and st["largest_acked"][2] == base + 599
    h.close()
    # seg_cap 4 with a 4-segment packet, a descriptor that says 9, and one without segments
    h = SentHarness(enc, [1024, 2048], 4)
    h.record([(0, 1, 200, 0, 0x80, 7, [(0, 5), (5, 6), (11, 7), (18, 8)], None),
              (1, 1, 300, 0, 0, 0, [(100, 1), (50, 2), (70, 3), (60, 4)], 9),
              (1, 2, 60, 0, 0, 0, [], None)])
    assert h.rules[0].slots[1]["bits"] == 0xC0 and len(h.rules[1].slots[1]["segs"]) == 4
    h.record([(0, 2, 10, 0, 0, 0, [(1, 1)], None), (0, 2, 20, 0, 0, 0, [(2, 2)], None),   # two copies: the first
              (0, 1, 10, 0, 0, 0, [(1, 1)], None),                                        # a duplicate
              (0, 3, 0, 0, 0, 0, [(1, 1)], None), (0, 4, 10, 7, 0, 0, [(1, 1)], None),    # wire_lens 0; status
              (0, 0, 10, 0, 0, 0, [(1, 1)], None), (2, 5, 10, 0, 0, 0, [(1, 1)], None),   # number 0; no member
              (NO_CONN, 6, 10, 0, 0, 0, [(1, 1)], None)], max_segments=1)
    assert h.rules[0].slots[2]["len"] == 10 and h.rules[0].duplicates == 2 and h.rules[0].tracked == 2
    h.close()


@pytest.mark.gpu
def test_threshold_and_deviation_b(enc):
    h = SentHarness(enc, [1024, 1024], 2)
    h.send(0, range(1, 13))
    h.send(1, range(1, 13))
    # three nacks in one call: missing 3 stays in flight
    h.ack([A(0, la, 0, [(2, la), (0, 0)], w=la) for la in (5, 6, 7)], max_ranges=3)
    assert h.rules[0].slots[1]["missing"] == 3 and h.rules[0].slots[1]["state"] == sr.IN_FLIGHT
    ev = h.ack([A(0, 8, 0, [(2, 8), (0, 0)], w=8)])               # and one in the next: queued
    assert h.rules[0].slots[1]["state"] == sr.QUEUED and ev["lost_packets"][0] == 1 and h.rules[0].sw_pending
    assert h.rules[0].lio == 8
    # acked and nacked in the same call: acknowledged wins
    ev = h.ack([A(1, 5, 0, [(2, 5), (0, 0)], w=1), A(1, 6, 6, [], w=2)])
    assert ev["acked_packets"][1] == 6 and 1 not in h.rules[1].slots
    # queued, then acknowledged before the drain, by an ACK whose lio_a is under the sender's lio (b)
    ev = h.ack([A(0, 9, 1, [(3, 9), (1, 1)], w=9)])
    assert 1 not in h.rules[0].slots and h.rules[0].queued == 0 and ev["acked_packets"][0] == 2
    conn, off, ln, touch, upto = h.drain(16)
    assert conn == [] and upto[0] == 100
    # an ACK at a queued number under lio that does not cover it leaves it queued
    h.send(0, range(13, 20))
    h.ack([A(0, la, 9, [(11, la), (9, 9)], w=la) for la in (14, 15, 16, 17)], max_ranges=2)
    assert h.rules[0].slots[10]["state"] == sr.QUEUED and h.rules[0].lio == 17
    h.ack([A(0, 18, 9, [(11, 18), (9, 9)], w=18)], max_ranges=2)
    assert h.rules[0].slots[10]["missing"] == 5
    assert h.drain(16)[0] == [0]
    h.close()


@pytest.mark.gpu
def test_ranges_at_word_bounds_the_wrap_none_and_a_lying_count(enc):
    h = SentHarness(enc, [1024, 1024], 1)
    h.send(0, range(1, 1001))
    rows = [(960, 1000), (768, 895), (640, 704), (128, 191), (64, 64)]      # begin / end at multiples of 64
    h.ack([A(0, 1000, 64, rows, w=1)], max_ranges=8)
    assert h.rules[0].tracked == 1000 - (41 + 128 + 65 + 64 + 64)
    h.ack([A(0, 1000, 64, rows, w=2)], max_ranges=8)                       # the same la again: not accepted
    h.send(0, range(1001, 1089))                                            # across the ring's wrap
    h.ack([A(0, 1088, 64, [(1020, 1030), (64, 64)], w=3, nr=7)], max_ranges=2)   # n_ranges > max_ranges
    assert 1024 not in h.rules[0].slots and 1031 in h.rules[0].slots
    h.send(1, range(1, 200))
    ev = h.ack([A(1, 150, 150, (), w=1)], max_ranges=0)                     # no ranges, no rows at all
    assert ev["acked_packets"][1] == 150 and h.rules[1].lio == 150
    # rows out of order and overlapping are clamped, not followed
    h.ack([A(1, 190, 150, [(170, 180), (175, 190), (160, 172), (150, 150)], w=2)], max_ranges=4)
    h.close()


@pytest.mark.gpu
def test_same_la_in_a_wave_in_two_waves_and_in_two_blocks(enc):
    h = SentHarness(enc, [4096], 1)
    h.send(0, range(1, 41))
    pk = [A(0, 0, 0, (), w=0)] * 3000                                       # filler: valid, never a candidate
    pk[7] = A(0, 30, 0, [(2, 30), (0, 0)], delay=1)                         # the lowest index wins
    pk[9] = A(0, 30, 30, (), delay=2)                                       # the same wave
    pk[200] = A(0, 30, 30, (), delay=3)                                     # another wave
    pk[2500] = A(0, 30, 30, (), delay=4)                                    # another block of 1,024
    pk[2501] = A(0, 31, 31, (), delay=5)
    pk[1100] = A(0, 31, 0, [(3, 31), (0, 0)], delay=6)
    ev = h.ack(pk, max_ranges=2)
    assert h.rules[0].slots[1]["missing"] == 2 and 2 not in h.rules[0].slots and ev["delay_us"][0] == 6
    h.close()


@pytest.mark.gpu
def test_filters_unsent_status_and_conn_of(enc):
    h = SentHarness(enc, [1024, 1024, 2048], 1)
    for c in range(3):
        h.send(c, range(1, 31))
    pk = [A(0, 31, 31, w=1),                                                # la > last_sent
          A(0, 10, 10, w=2), A(0, 20, 20, w=3, status=3), A(0, 12, 12, w=4),      # a non-OK status between
          A(7, 25, 25, w=5), A(NO_CONN, 25, 25, w=6),                       # conn_of >= nconn
          A(1, 9, 9, w=0, flags=0x20)]                                      # no ACK flag
    pk += [A(i % 3, 13 + i // 3, 13 + i // 3, w=10 + i) for i in range(30)]      # alternating over three members
    h.ack(pk)
    st = h.set.states()
    assert st["unsent_acks"].tolist() == [1, 0, 0] and st["largest_acked"].tolist() == [22, 22, 22]
    ev = h.ack([A(0, 25, 25, w=5), A(1, 25, 25, w=0)])                      # w not above largest_with_ack
    assert ev["accepted"].tolist() == [0, 1, 0]
    h.ack([])                                                               # an empty batch writes the rows
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nconn", [3, 1025, 32769])
def test_many_members(enc, nconn):
    wss = [(1024, 2048, 4096)[c % 3] for c in range(nconn)]
    h = SentHarness(enc, wss, 2, watch=[0, 1, 2, nconn // 2, nconn - 1])
    rng = random.Random(nconn)
    pk = [(c, n, 100 + c % 7, 0, 0x80 if c % 4 == 0 else 0, 0, [(10 * n, 10)], None)
          for c in range(nconn) for n in range(1, 9) if c % 5 != 4]
    pk.append((1, 5000, 10, 0, 0, 0, [], None))                             # member 1 becomes inert
    rng.shuffle(pk)
    h.record(pk)
    acks = [A(c, la, 0, [(2, la), (0, 0)], w=la) for c in range(nconn) if c % 5 != 4 for la in (5, 6, 7, 8)]
    rng.shuffle(acks)
    ev = h.ack(acks, max_ranges=2)
    assert ev["lost_packets"][0] == 1 and ev["accepted"][1] == 0 and ev["accepted"][min(4, nconn - 1) if nconn > 4 else 1] == 0
    h.rto([0] * nconn, 10 ** 9)
    live = sum(1 for c in range(nconn) if c % 5 != 4 and c != 1)
    conn, off, ln, touch, upto = h.drain(live - live // 3)                  # the last third does not fit
    assert len(conn) == live - live // 3 and touch[0] == 1 and touch[2] == 0
    h.attach([c % 50 for c in range(nconn)], [c % 2 for c in range(nconn)], 40)
    h.close()


@pytest.mark.gpu
def test_rto_deadline_backoff_and_cap(enc):
    h = SentHarness(enc, [1024] * 4, 1)
    for c in range(4):
        h.send(c, range(1, 40), now_us=1_000_000)
    assert h.rto([0, 300_000, 100_000, 0], 1_000_000 + 299_999) == [0, 0, 1, 0]    # floor 200 ms fired
    assert h.rto([0, 300_000, 0, 0], 1_000_000 + 300_000) == [0, 1, 0, 0]           # at the deadline
    assert h.rto([0, 0, 0, 0], 1_000_000 + 500_001) == [1, 0, 0, 1]                 # after it; default 500 ms
    assert h.rules[0].rto_count == 1 and h.rules[0].lio == 1
    t = h.rules[0].last_sent_us
    assert h.rto([0, 0, 0, 0], t + 999_999)[0] == 0 and h.rto([0, 0, 0, 0], t + 1_000_000)[0] == 1   # << 1
    for k in range(2, 9):
        t = h.rules[0].last_sent_us
        assert h.rto([0, 0, 0, 0], t + 60_000_000)[0] == 1
    assert h.rules[0].rto_count == 9
    t = h.rules[0].last_sent_us
    assert h.rto([200_000] + [0] * 3, t + 59_999_999)[0] == 0                       # 200 ms << 9 is capped
    assert h.rto([200_000] + [0] * 3, t + 60_000_000)[0] == 1
    h.ack([A(0, 39, 39, w=1)])                                                      # an RTT sample resets it
    assert h.rules[0].rto_count == 0
    assert h.rto([0] * 4, 10 ** 12)[0] == 0                                         # nothing in flight
    assert 0 not in h.drain(64)[0]                                                  # all freed by the ACK
    h.close()


@pytest.mark.gpu
def test_a_deadline_past_2_64_never_comes(enc):
    """The RTO is at most 60 s, so last_sent_us + rto passes 2^64 only in the
    last minute of the clock: member 0 sent 30 s before 2^64, member 1 70 s
    before it, both wait the capped 60 s.  At the last clock there is, member
    1's deadline has passed and member 0's never comes; a sum that wrapped
    would have it due since long."""
    top = 1 << 64
    h = SentHarness(enc, [1024] * 2, 1)
    h.send(1, range(1, 5), now_us=top - 70_000_000)
    h.send(0, range(1, 5), now_us=top - 30_000_000)
    assert h.rto([60_000_000] * 2, top - 10_000_001) == [0, 0]
    assert h.rto([60_000_000] * 2, top - 10_000_000) == [0, 1]                      # at member 1's deadline
    assert h.rto([60_000_000] * 2, top - 1) == [0, 0]                               # member 1 backs off: 60 s again
    assert h.rto([10 ** 9, 200_000], top - 1) == [0, 1]                             # 400 ms: due; 0 is capped at 60 s
    assert h.rto([0, 0], top - 1) == [1, 0]                                         # 500 ms: due since 29.5 s; 1's 2 s wrap
    h.close()


@pytest.mark.gpu
def test_drain_order_tail_clamp_touch_and_upto(enc):
    h = SentHarness(enc, [1024] * 3, 2)
    h.record([(c, n, 100, 0, 0x80 if (c, n) == (1, 3) else 0, 5 if (c, n) == (0, 1) else 0,
               [(1000 * c + 10 * n, 4), (1000 * c + 10 * n + 4, 6)], None) for c in range(3) for n in range(1, 13)])
    def lose(c, missing):
        out = []
        for la in (9, 10, 11, 12):
            lio, rows = holes(la, missing)
            out.append(A(c, la, lio, rows, w=la))
        return out
    h.ack(lose(0, {1, 3}) + lose(1, {3}) + lose(2, {2, 5, 6}), max_ranges=5)
    assert [r.queued_segments for r in h.rules] == [4, 2, 6]
    assert h.drain(0)[0] == []                                              # max_entries 0
    conn, off, ln, touch, upto = h.drain(5)                                 # the clamp inside member 1
    assert conn == [0] * 4 and off == [10, 14, 30, 34] and touch == [0, 0, 0] and h.rules[0].sw_pending
    assert upto == [M64, 1030, 2020] and h.rules[1].queued == 1            # member 0 holds nothing any more
    conn, off, ln, touch, upto = h.drain(7)                                 # member 1 fits, member 2 not
    assert conn == [1, 1] and touch == [0, 1, 0]
    conn, off, ln, touch, upto = h.drain(6)
    assert conn == [2] * 6 and off[:2] == [2020, 2024]
    for c in range(3):
        h.ack([A(c, 12, 12, w=20)])
    assert h.drain(4)[4] == [M64] * 3                                       # nothing occupied
    h.close()


@pytest.mark.gpu
def test_attach_cases(enc):
    h = SentHarness(enc, [1024] * 4, 1)
    for c in range(4):
        h.send(c, range(1, 10))
        h.ack([A(c, la, 0, [(2, la), (0, 0)], w=la) for la in (5, 6, 7, 8)], max_ranges=2)
    assert [r.sw_pending for r in h.rules] == [1] * 4
    w, att = h.attach([0, 3, 9, 2], [2, 0, 1, 1], 8)                        # no packet; first_packet past the end
    assert att == [1, 0, 0, 1] and w == [(0, 9), (2, 9)]
    w, att = h.attach([0, 3, 7, 2], [1, 1, 1, 1], 8)
    assert att == [0, 1, 1, 0]
    h.close()


@pytest.mark.gpu
def test_pinned_operands_and_kernel_class(enc):
    h = SentHarness(enc, [1024, 4096], 2)
    enc.timing_begin(64)
    try:
        h.record([(c, n, 50, 0, 0, 0, [(n, 1)], None) for c in range(2) for n in range(1, 9)], where="pinned")
        h.ack([A(c, la, 0, [(2, la), (0, 0)], w=la) for c in range(2) for la in (5, 6, 7, 8)], where="pinned")
        h.rto([0, 0], 10 ** 9, where="pinned")
        h.drain(8, where="pinned")
        h.attach([0, 1], [1, 1], 2, where="pinned")
    finally:
        recs, untimed = enc.timing_end()
    assert untimed == 0
    # record 5 launches, ack 5, rto 1, drain 6, attach 1 (the state gather is not a timed call)
    assert recs["kernel"].tolist() == [13] * (5 + 5 + 1 + 6 + 1)
    h.close()


@pytest.mark.gpu
def test_argument_errors_on_the_device(enc):
    lib = fec.load_library()
    bad = fec.ErrInvalidArg.code
    h = SentHarness(enc, [1024, 1024], [2, 4])
    h.send(0, [1, 2])
    out = ctypes.c_void_p(1)
    twice = (ctypes.c_void_p * 2)(h.txs[0]._h.value, h.txs[0]._h.value)
    assert lib.ugo_fec_sent_set_create(enc._h, ctypes.addressof(twice), 2, ctypes.byref(out)) == bad
    assert out.value is None
    assert lib.ugo_fec_sent_tx_create(enc._h, 1000, 4, ctypes.byref(out)) == bad
    assert lib.ugo_fec_sent_tx_create(enc._h, 1024, 17, ctypes.byref(out)) == bad
    buf = {k: torch.full((n,), 0x11, dtype=torch.uint8, device="cuda")
           for k, n in (("info", 256), ("segs", 256), ("conn", 16), ("lens", 8), ("st", 4), ("ranges", 256),
                        ("ev", 128), ("u64", 16), ("u8", 2), ("off", 32), ("len", 16), ("n", 8))}
    p = {k: v.data_ptr() for k, v in buf.items()}
    host = torch.zeros(256, dtype=torch.uint8).data_ptr()                   # pageable
    rec = lambda **k: lib.ugo_fec_sent_set_record(  # noqa: E731
        h.set._h, k.get("info", p["info"]), k.get("segs", p["segs"]), k.get("ms", 2), k.get("conn", p["conn"]),
        k.get("lens", p["lens"]), k.get("st", p["st"]), k.get("n", 4), 5, None)
    assert rec(ms=3) == bad and rec(ms=0) == bad                            # above the smallest seg_cap
    assert rec(info=None) == bad and rec(segs=None) == bad and rec(conn=None) == bad and rec(lens=None) == bad
    assert rec(st=None) == bad and rec(info=p["info"] + 8) == bad and rec(info=host) == bad and rec(st=host) == bad
    assert rec(n=(1 << 31) + 1) == bad and rec(n=0) == 0
    ack = lambda **k: lib.ugo_fec_sent_set_ack(  # noqa: E731
        h.set._h, k.get("info", p["info"]), k.get("ranges", p["ranges"]), k.get("mr", 4), k.get("conn", p["conn"]),
        k.get("n", 4), 5, k.get("ev", p["ev"]), None)
    assert ack(info=None) == bad and ack(ranges=None) == bad and ack(conn=None) == bad and ack(ev=None) == bad
    assert ack(mr=0x10000) == bad and ack(ev=host) == bad and ack(info=p["info"] + 4) == bad
    assert lib.ugo_fec_sent_set_rto(h.set._h, None, 5, p["u8"], None) == bad
    assert lib.ugo_fec_sent_set_rto(h.set._h, p["u64"], 5, None, None) == bad
    assert lib.ugo_fec_sent_set_rto(h.set._h, host, 5, p["u8"], None) == bad
    dr = lambda **k: lib.ugo_fec_sent_set_drain(  # noqa: E731
        h.set._h, k.get("m", 4), k.get("conn", p["conn"]), k.get("off", p["off"]), k.get("len", p["len"]),
        k.get("n", p["n"]), k.get("touch", p["u8"]), k.get("upto", p["u64"]), None)
    assert dr(conn=None) == bad and dr(off=None) == bad and dr(len=None) == bad and dr(n=None) == bad
    assert dr(touch=None) == bad and dr(upto=None) == bad and dr(m=(1 << 31) + 1) == bad and dr(off=host) == bad
    at = lambda **k: lib.ugo_fec_sent_set_attach(  # noqa: E731
        h.set._h, k.get("first", p["u64"]), k.get("count", p["conn"]), k.get("m", 4), k.get("info", p["info"]),
        k.get("att", p["u8"]), None)
    assert at(first=None) == bad and at(count=None) == bad and at(info=None) == bad and at(att=None) == bad
    assert at(m=(1 << 31) + 1) == bad and at(first=host) == bad
    torch.cuda.synchronize()
    assert all(bool((t == 0x11).all()) for t in buf.values())
    h.check()
    h.close()


@pytest.mark.gpu
def test_one_member_with_a_long_span(enc):
    """One connection, 5,000 numbers outstanding over five chunks, a SACK on
    every arrival: the chunk sums and the scan across them."""
    h = SentHarness(enc, [8192], 1)
    h.send(0, range(1, 5001))
    missing = set(range(7, 5000, 97))
    acks = []
    for la in range(4000, 5001, 50):
        lio, rows = holes(la, {m for m in missing if m < la})
        acks.append(A(0, la, lio, rows[:3] + rows[-1:], w=la))
    h.ack(acks, max_ranges=4)
    h.drain(4096)
    h.close()


@pytest.mark.gpu
def test_an_accepted_la_in_a_gap_below_scan_from_leaves_no_claim(enc):
    """Number 3 failed to encode, so 4 and 5 are stored above a gap and the drain
    moves scan_from to 4.  An ACK for 3 is accepted all the same; its claim lies
    below scan_from and must be cleared (the harness checks both scratch rings
    after every call), or number 3 + Ws would later lose its slot to it."""
    h = SentHarness(enc, [1024], 1)
    h.send(0, [1, 2])
    h.ack([A(0, 2, 2, w=1)])
    h.record([(0, 3, 100, 7, 0, 0, [(30, 10)], None), (0, 4, 100, 0, 0, 0, [(40, 10)], None),
              (0, 5, 100, 0, 0, 0, [(50, 10)], None)])
    h.drain(8)
    assert h.rules[0].scan_from == 4 and h.rules[0].lio == 2
    ev = h.ack([A(0, 0, 0, w=0)] * 70 + [A(0, 3, 3, w=2)])                  # a high batch index holds the claim
    assert ev["accepted"][0] == 1 and h.rules[0].lio == 3
    h.ack([A(0, 5, 5, w=3)])
    st = h.record([(0, 3 + 1024, 100, 0, 0, 0, [(99, 1)], None)])           # batch index 0: would lose to a stale ~70
    assert st["tracked"][0] == 1 and st["duplicates"][0] == 0 and 3 + 1024 in h.rules[0].slots
    h.close()


KEY = b"\x0f\x1e\x2d\x3c\x4b\x5a\x69\x78"


@pytest.mark.gpu
def test_round_trip_of_two_peers_heals_a_lossy_link(enc):
    """Three connections from A to B, a fixed 5 % of the wire packets dropped in
    every round: write, plan, both attaches, set_encode, record, tx_assemble |
    rx_assemble, packet_decode, set_deliver, ack_set_receive, B's ACK-only
    packets back | set_ack, set_rto, drain, set_retransmit, ack_set_touch,
    set_release, until set_read has returned every written byte.  The host
    reads only sizes (total, total_out, n_read) and the event rows."""
    rng = np.random.default_rng(5)
    d, n, S, slot, MR, MS, G = 10, 13, 1470, 1488, 8, 2, 3
    NP = G * d
    dev = torch.device("cuda")
    pad = _put(np.frombuffer(fec.rc4_keystream(KEY, slot), np.uint8)[:slot].copy())
    sizes = [30_000, 45_000, 20_011]
    data = [rng.integers(0, 256, k, dtype=np.uint8) for k in sizes]
    i64 = dict(dtype=torch.int64, device=dev)
    # side A: send windows, its sent histories, its (idle) receive histories
    txA = [fec.StreamTx(enc, 65536, 64, 0, 1000 * c) for c in range(3)]      # packet numbers start anywhere
    tsetA = fec.StreamTxSet(enc, txA)
    sentA = [fec.SentTx(enc, 1024, MS) for _ in range(3)]
    ssetA = fec.SentTxSet(enc, sentA)
    ackA = [fec.AckRx(enc, 1024) for _ in range(3)]
    asetA = fec.AckRxSet(enc, ackA)
    # side B: receive windows, receive histories, empty send windows for its ACK-only packets
    rxB = [fec.StreamRx(enc, 65536) for _ in range(3)]
    rsetB = fec.StreamRxSet(enc, rxB)
    ackB = [fec.AckRx(enc, 1024) for _ in range(3)]
    asetB = fec.AckRxSet(enc, ackB)
    txB = [fec.StreamTx(enc, 4096, 4) for _ in range(3)]
    tsetB = fec.StreamTxSet(enc, txB)
    src = torch.from_numpy(np.concatenate(data)).to(dev)
    off = torch.tensor([0, sizes[0], sizes[0] + sizes[1]], **i64)
    written = tsetA.write(src, off, torch.tensor(sizes, **i64))
    assert written.tolist() == sizes
    budget = torch.full((3,), 8, dtype=torch.int32, device=dev)
    zero_budget = torch.zeros(3, dtype=torch.int32, device=dev)
    may = torch.ones(3, dtype=torch.uint8, device=dev)
    delays = torch.zeros(3, **i64)
    want_all = torch.full((3,), 1 << 20, **i64)
    dst = torch.zeros(3 << 20, dtype=torch.uint8, device=dev)
    dst_off = torch.arange(3, **i64) << 20
    got = [bytearray() for _ in range(3)]
    planA = planB = None
    rangesA = torch.zeros((NP, MR, 2), **i64)
    rangesB = torch.zeros((8, MR, 2), **i64)
    lost_total = stop_waitings = rounds = 0
    now = 1_000_000
    while any(len(g) < s for g, s in zip(got, sizes)):
        rounds += 1
        assert rounds <= 80, ([len(g) for g in got], ssetA.states())
        now += 150_000
        # ---- A sends
        planA = tsetA.plan(budget, NP, max_segments=MS, out=planA)
        info, segs, conn, first, count, total = planA
        asetA.attach(now, first, count, total, info, rangesA, conn)
        att = ssetA.attach(first, count, info)
        npk = int(total.item())                                             # a size
        wire_in = torch.zeros((NP, slot), dtype=torch.uint8, device=dev)
        lens_in = torch.full((NP,), 16, dtype=torch.int16, device=dev)      # the groups are filled up with 16 zero
                                                                            # bytes of no connection (conn_of NO_CONN)
        if npk:
            w, l, st = tsetA.encode(info, rangesA, segs, conn, slot, npackets=npk, framed=True)
            ssetA.record(info, segs, conn, l, st, now, npackets=npk)
            wire_in[:npk], lens_in[:npk] = w, l
            iv = info[:npk].cpu().numpy().view(fec.PKT_INFO_DTYPE).reshape(-1)   # the test's own look, not the host path's
            stop_waitings += int((iv["stop_waiting"] != 0).sum())
            assert int(att.sum()) == int((iv["stop_waiting"] != 0).sum()) and not st.any()
        wire = torch.zeros((G * n, slot), dtype=torch.uint8, device=dev)
        wl = torch.zeros(G * n, dtype=torch.int16, device=dev)
        gst = torch.full((G,), -1, dtype=torch.int8, device=dev)
        enc.tx_assemble(wire_in, lens_in, wire, wl, first_seq=0, pad=pad, status=gst)
        assert gst.tolist() == [0] * G
        # ---- the link: a fixed 5 % of the wire packets is lost
        wl_rx = wl.clone()
        wl_rx[torch.arange(G * n, device=dev) % 20 == (7 * rounds) % 20] = 0
        frames = torch.zeros((n, G, slot), dtype=torch.uint8, device=dev)
        present = torch.zeros(G, **i64)
        enc.rx_assemble(wire, wl_rx, frames, present, shard_size=S, pad=pad, frames=True)
        rows = frames[:d].reshape(d * G, slot)                              # row k * G + g is data packet g * d + k
        order = np.array([g * d + k for k in range(d) for g in range(G)])
        back = torch.from_numpy(np.argsort(order)).to(dev)
        rows = rows[back].contiguous()
        rl = wl_rx.view(G, n)[:, :d].contiguous().view(-1)
        dinfo, dranges, dsegs = enc.packet_decode(rows, rl, framed=True, max_ranges=MR, max_segments=MS)
        # ---- B receives and acknowledges
        seg_status = rsetB.deliver(rows, dinfo, dsegs, conn)
        asetB.receive(dinfo, conn, now + 1000, seg_status=seg_status)
        n_read, _ = rsetB.read(want_all, dst, dst_off)
        for c, k in enumerate(n_read.tolist()):                             # sizes
            got[c] += dst[(c << 20):(c << 20) + k].cpu().numpy().tobytes()
        planB = tsetB.plan(zero_budget, 8, max_segments=MS, out=planB)
        binfo, bsegs, bconn, bfirst, bcount, btotal = planB
        total_out, _ = asetB.attach(now + 2000, bfirst, bcount, btotal, binfo, rangesB, bconn, may_ack_only=may)
        nb = int(total_out.item())                                          # a size
        if nb:
            bw, bl, bst = tsetB.encode(binfo, rangesB, bsegs, bconn, slot, npackets=nb, pad=pad)
            assert not bst.any()
            ainfo, aranges, _ = enc.packet_decode(bw, bl, pad=pad, max_ranges=MR, max_segments=MS)
            # ---- A hears of it
            events = ssetA.ack(ainfo, aranges, bconn, now + 3000, npackets=nb)
            ev = events.cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)    # the event rows: the host's input
            lost_total += int(ev["lost_packets"].sum())
        ssetA.rto(delays, now + 4000)
        rc, ro, rlen, n_entries, touch, upto = ssetA.drain(64)
        tsetA.retransmit(rc, ro, rlen)
        asetA.touch(touch)
        tsetA.release(upto)
    for c in range(3):
        assert bytes(got[c]) == data[c].tobytes(), c
    st = ssetA.states()
    assert not st["err"].any() and lost_total + int(st["rto_count"].sum()) > 0 and stop_waitings > 0
    assert int(st["lost_packets"].sum()) > 0
    for x in (tsetA, ssetA, asetA, rsetB, asetB, tsetB):
        x.close()
    for x in txA + sentA + ackA + rxB + ackB + txB:
        x.close()
