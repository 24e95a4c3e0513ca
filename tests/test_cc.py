"""Congestion control (include/ugo_cc.h): THE RULE against a restatement of
ugo/congestion/ on the CPU, and the device against one rule per member."""
import ctypes
import random
import re
import time
from collections import Counter

import numpy as np
import pytest

import ack_ref as ar
import cc_ref as cr
import sent_ref as sr
from cc_harness import CcHarness, CcRulesOnly, event_array, row_array
from sent_ref import Ack
from ugo_amd import fec


# ---------------------------------------------------------------- CPU: the rule against the reference
def _sack(peer, w, delay=0):
    la, lio, rows, _ = peer.view()
    return Ack(la, lio, rows, w, delay)


def _differs(go, rule):
    g, r = go.cc.view(), rule.cc.view()
    keys = [k for k in g if k != "started" or (g["cwnd"] < g["ssthresh"] and r["cwnd"] < r["ssthresh"])]
    return any(g[k] != r[k] for k in keys) or go.go.view() != rule.sent.view()


def run_family(seed, length=1400, rto=True, **params):
    """One seeded sequence: bursts as large as the budget allows, 0-20 % lost,
    a SACK on 60 % of the arrivals, one accepted ACK per member and call, an
    RTO now and then, a drain after every call.  Every clock value and ACK
    delay is an even number of us, so that no RTT sample is odd (deviation
    (c)).  Returns (compared states, states that differ)."""
    rng = random.Random(seed)
    loss = rng.uniform(0.0, 0.2)
    go, rule, peer = cr.GoPair(**params), cr.RulePair(1024, 1, **params), ar.RuleAck(1024)
    nxt, w, now = 1, 0, 1000
    compared = differ = 0
    budget = rule.cc.rto(0, 0, 0, length, 64)
    assert budget == go.budget(length, 64)
    for _ in range(rng.randint(4, 30)):
        k = min(budget, rng.randint(1, 40))
        if k == 0:                                         # nothing may be sent: time passes until the RTO
            now += 600_000
        burst = list(range(nxt, nxt + k))
        nxt += k
        now += 2 * rng.randint(100, 30_000)
        sw = rule.sent.attach(True)[1]
        go.go.GetStopWaitingFrame()
        go.send(burst, length, now)
        rule.send(burst, length, now)
        acks = []
        for j, n in enumerate(burst):
            if rng.random() >= loss:
                peer.receive([(n, sw if j == 0 else 0)])
                if rng.random() < 0.6:
                    w += 1
                    acks.append(_sack(peer, w, delay=2 * rng.randint(0, 3000)))
        for a in acks + [None]:                            # the last call of a round carries no ACK
            now += 2 * rng.randint(1, 20_000)
            go_acked, go_lost = go.ack(a, now) if a else ([], [])
            ev, row, delay = rule.ack([a] if a else [], now)
            assert (len(go_acked), len(go_lost)) == (ev["acked_packets"], ev["lost_packets"])
            assert max(go_lost, default=0) == row["max_lost"] and max(go_acked, default=0) == row["max_acked"]
            assert delay == go.cc.RetransmissionDelay() // cr.US
            if rto and rng.random() < 0.1:
                now += 600_000
            fired, budget = rule.rto(now, length, 64)
            assert bool(go.rto(now)) == bool(fired)
            assert budget == go.budget(length, 64)
            assert go.go.drain_all() == rule.sent.drain()[0]
            compared += 1
            differ += _differs(go, rule)
    return compared, differ, rule.cc


def _families(seeds, **kw):
    total = bad = cutbacks = rtos = 0
    modes = set()
    for seed in seeds:
        c, d, cc = run_family(seed, **kw)
        total, bad, cutbacks, rtos = total + c, bad + d, cutbacks + cc.cutbacks, rtos + cc.rtos
        modes.add("slow start" if cc.in_slow_start() else "avoidance")
        modes.add("app-limited" if cc.app_limited_us else "busy")
    return total, bad, cutbacks, rtos, modes


def test_family_equals_the_reference():
    total, bad, cutbacks, rtos, modes = _families(range(300))
    assert total > 5000 and bad == 0, (total, bad)
    assert cutbacks > 100 and rtos > 100 and modes == {"slow start", "avoidance", "app-limited", "busy"}


def test_family_of_small_packets_equals_the_reference():
    """Packets of 100 bytes never fill the window: the app-limited side."""
    total, bad, _, _, _ = _families(range(1000, 1150), length=100)
    assert total > 2000 and bad == 0, (total, bad)


def test_family_with_other_parameters_equals_the_reference():
    total, bad, cutbacks, _, _ = _families(range(2000, 2150), initial_cwnd=10, max_cwnd=60, min_cwnd=3,
                                           num_connections=1, mss=1000)
    assert total > 2000 and bad == 0 and cutbacks > 0, (total, bad)


def test_family_without_rto_equals_the_reference():
    total, bad, _, _, _ = _families(range(3000, 3150), rto=False)
    assert total > 2000 and bad == 0, (total, bad)


def _pair(numbers, length=1400, now=1000, **params):
    go, rule = cr.GoPair(**params), cr.RulePair(1024, 1, **params)
    go.send(numbers, length, now)
    rule.send(numbers, length, now)
    return go, rule


def test_deviation_a_two_accepted_acks_in_one_call_are_one_event():
    """The reference runs UpdateRTT and OnCongestionEvent per ACK: two RTT
    samples, ShouldExitSlowStart twice, and the ten packets of the first ACK
    judged with 42,000 bytes in flight (ten increments, then 28,000 bytes are
    too few for a window of 42).  The rule takes the later sample, asks once,
    and judges all twenty with the 28,000 bytes the call leaves in flight: the
    window stops at 39, the first with 39 * 1460 >= 2 * 28,000."""
    go, rule = _pair(range(1, 41))
    a10, a20 = Ack(10, 10, [], 1, delay=0), Ack(20, 20, [], 2, delay=0)
    go.ack(a10, 5000), go.ack(a20, 5000)
    ev, row, _ = rule.ack([a10, a20], 5000)
    assert ev["acked_packets"] == 20 and row["max_acked"] == 20 and ev["bytes_in_flight"] == 28_000
    g, r = go.cc.view(), rule.cc.view()
    assert (g["cwnd"], r["cwnd"]) == (42, 39) and g["app_limited_us"] == r["app_limited_us"] == 5000
    assert g["sample_count"] == 2 and r["sample_count"] == 1             # ShouldExitSlowStart ran twice / once
    assert g["srtt_us"] == r["srtt_us"] == 4000 and g["mean_dev_us"] == 1500 and r["mean_dev_us"] == 2000
    # ... and equals the reference run on them in turn when each call carries one
    go, rule = _pair(range(1, 41))
    go.ack(a10, 5000), go.ack(a20, 5000)
    rule.ack([a10], 5000), rule.ack([a20], 5000)
    assert not _differs(go, rule)


def test_deviation_c_whole_microseconds():
    go, rule = _pair([1])
    a = Ack(1, 1, [], 1)
    go.ack(a, 1000 + 4001), rule.ack([a], 1000 + 4001)                  # an odd sample
    assert go.cc.meanDeviation == 2_000_500 and rule.cc.mean_dev_us == 2000      # ns / us
    assert go.cc.RetransmissionDelay() // cr.US == 4001 + 8002 and rule.delay_us == 4001 + 8000
    go, rule = _pair([1])
    go.ack(a, 1000 + 4000), rule.ack([a], 1000 + 4000)                  # an even one: the same
    assert go.cc.RetransmissionDelay() // cr.US == rule.delay_us == 12000 and not _differs(go, rule)


def test_deviation_e_started_is_judged_after_the_calls_increments():
    """ssthresh 40: the call's eighth increment leaves slow start.  The
    reference cleared started at the first packet above end_packet_number, while
    still in slow start; the rule looks once, after the increments, and is no
    longer in slow start.  Nothing reads started outside slow start, and the
    next round in slow start starts anew either way."""
    go, rule = _pair(range(1, 71))                                       # 56,000 bytes stay in flight: cwnd-limited
    go.cc.slowstartThreshold = rule.cc.ssthresh = 40
    go.cc.started = rule.cc.started = 1                                  # a round that ends at packet 3
    go.cc.endPacketNumber = rule.cc.end_packet_number = 3
    a = Ack(30, 30, [], 1)
    go.ack(a, 5000), rule.ack([a], 5000)
    g, r = go.cc.view(), rule.cc.view()
    assert g["cwnd"] == r["cwnd"] >= 40 and g["ssthresh"] == r["ssthresh"] == 40       # 8 increments, then CUBIC
    assert (g["started"], r["started"]) == (0, 1)
    assert {k: v for k, v in g.items() if k != "started"} == {k: v for k, v in r.items() if k not in
                                                              ("started", "rto_candidate")}


def test_deviation_g_a_budget_counts_whole_packets():
    go, rule = _pair(range(1, 31), length=1400)                          # 42,000 of 46,720 bytes in flight
    assert rule.rto(1001, 1400, 64)[1] == go.budget(1400, 64) == 4       # 4,720 / 1,400 + 1
    assert rule.rto(1001, 1400, 3)[1] == 3 and rule.rto(1001, 1400, 0)[1] == 0
    # the reference sends short packets while bytes_in_flight <= W: five of 1,000; the budget of 1,400-byte
    # packets lets four through, whatever their length
    assert go.budget(1000, 64) == 5
    go, rule = _pair(range(1, 34), length=1460)                          # 48,180 > 46,720
    assert rule.rto(1001, 1460, 64)[1] == go.budget(1460, 64) == 0
    go, rule = _pair(range(1, 33), length=1460)                          # bif == W: one more
    assert rule.rto(1001, 1460, 64)[1] == go.budget(1460, 64) == 1


def test_deviation_i_the_rto_takes_the_candidate_cc_set_ack_saw():
    go, rule = _pair(range(1, 11))
    a = Ack(10, 10, [], 1)
    go.ack(a, 3000), rule.ack([a], 3000)                                 # nothing outstanding: candidate 0
    assert rule.cc.rto_candidate == 0
    go.send(range(11, 21), 1400, 4000), rule.send(range(11, 21), 1400, 4000)
    assert bool(go.rto(10 ** 7)) and rule.rto(10 ** 7, 1400, 64)[0] == 1      # no ugo_fec_cc_set_ack between
    assert go.cc.cutbacks == 1 and rule.cc.cutbacks == 0                 # the reference lost packet 11 first
    assert go.cc.congestionWindow == rule.cc.cwnd == 2 and (go.cc.slowstartThreshold, rule.cc.ssthresh) == (13, 16)
    # in THE ORDER ugo_fec_cc_set_ack runs in every batch, with or without ACKs, and the two agree
    go, rule = _pair(range(1, 11))
    go.ack(a, 3000), rule.ack([a], 3000)
    go.send(range(11, 21), 1400, 4000), rule.send(range(11, 21), 1400, 4000)
    rule.ack([], 5000)
    assert rule.cc.rto_candidate == 11
    assert bool(go.rto(10 ** 7)) and rule.rto(10 ** 7, 1400, 64)[0] == 1
    assert not _differs(go, rule)


def test_the_integer_cube_root_is_the_references_up_to_its_default_window():
    """... and up to the largest window the header permits: every difference
    last_max_cwnd - cwnd of 1 .. 2^20, against the restatement's root, which is
    numpy.cbrt on float64 (Go's own math.Cbrt is not what this compares with)."""
    for d in range(1, 200):
        x = cr.CUBE_FACTOR * d
        t = cr.icbrt(x)
        assert t ** 3 <= x < (t + 1) ** 3 and t == cr.cbrt_go(x), d
    assert cr.icbrt(0) == 0 and cr.icbrt(7) == 1 and cr.icbrt(8) == 2 and cr.icbrt((1 << 64) - 1) == 2642245
    x = np.uint64(cr.CUBE_FACTOR) * np.arange(1, (1 << 20) + 1, dtype=np.uint64)      # below 2^52: exact as float64
    t = np.zeros_like(x)
    for b in range(21, -1, -1):                            # cr.icbrt, every difference at once
        cand = t | np.uint64(1 << b)
        t = np.where(cand * cand * cand <= x, cand, t)     # cand < 2^21.4: the cube stays below 2^64
    assert int(t[-1]) == cr.icbrt(int(x[-1])) == 141_147 and int(t[198]) == cr.icbrt(int(x[198]))
    assert bool((t * t * t <= x).all()) and bool((x < (t + np.uint64(1)) ** np.uint64(3)).all())
    bad = np.flatnonzero(t != np.cbrt(x.astype(np.float64)).astype(np.uint64))
    assert bad.size == 0, (bad[:8] + 1, t[bad[:8]])


# ---------------------------------------------------------------- CPU: off the defaults, event by event
# (initial_cwnd, max_cwnd, min_cwnd, num_connections, mss)
PARAM_SETS = {
    "defaults": dict(cr.DEFAULTS),
    "window_2_20": dict(initial_cwnd=32, max_cwnd=1 << 20, min_cwnd=2, num_connections=1, mss=1460),
    "jumbo": dict(initial_cwnd=1000, max_cwnd=100_000, min_cwnd=1, num_connections=8, mss=9000),
    "floor_2_19": dict(initial_cwnd=1 << 20, max_cwnd=1 << 20, min_cwnd=1 << 19, num_connections=1000, mss=1),
}
# floor_2_19 is never in slow start: its window starts at ssthresh = max_cwnd, a cutback sets ssthresh = cwnd,
# and an RTO leaves ssthresh = cwnd / 2 <= 2^19 = min_cwnd = cwnd.  The tests below hold that instead.
NEVER_IN_SLOW_START = ("floor_2_19",)
CLOCK_STEPS = (1000, 20_000, 30_000, 30_001, 200_000, 5 * 10 ** 6, 4 * 10 ** 8, 36 * 10 ** 8, 10 ** 13)
STEP_WEIGHTS = (4, 6, 3, 3, 4, 3, 3, 1, 1)
SHORT_STEPS = CLOCK_STEPS[:6]                              # each twice: 12 rounds stay below 10^8 us
ACKED = (0, 1, 3, 40, 300, 5000, 60_000)
ACKED_WEIGHTS = (2, 4, 4, 5, 4, 3, 2)
WRAP_OFFSET = 282_000                                     # 410 * offset^3 passes 2^63 from here on


def _wide_fields(rng, rule):
    """What of an event row does not depend on packet numbers: an even RTT
    sample and ACK delay (deviation (c)), bytes in flight around the member's
    own window and far above it."""
    mss = rule.p["mss"]
    w = rule.cwnd * mss
    bif = rng.choice((0, w // 2, w // 2 + 1, w - 3 * mss - 1, w - 3 * mss, w - 1, w, w + 1, 2 * w, 10 ** 12, 1 << 62))
    return dict(accepted=int(rng.random() < 0.9), has_rtt=int(rng.random() < 0.8),
                rtt_us=2 * (rng.choice((0, 450, 2000, 10_000, 10_500, 30_000, 1_250_000)) + rng.randrange(25)),
                delay_us=rng.choice((0, 10, 3000, 10 ** 7)), bytes_in_flight=max(bif, 0),
                acked_packets=rng.choices(ACKED, ACKED_WEIGHTS)[0], lost_packets=rng.choice((0, 0, 0, 0, 0, 1, 3)))


def _cubic_offset(rule, now):
    """time_to_origin - elapsed of the call's CUBIC step, if it took one past
    the 30-ms return (the fields are as that step left them)."""
    if rule.last_update_us != now or rule.epoch_us == 0:
        return 0
    return rule.time_to_origin - cr.go_div(cr.s64((now + rule.min_rtt_us - rule.epoch_us) << 10), 1000000)


def _go_budget(go, bif, packet_bytes, max_budget):
    k = 0
    while k < max_budget and bif <= go.GetCongestionWindow():
        k, bif = k + 1, bif + packet_bytes
    return k


def _views_differ(go, rule):
    g, r = go.view(), rule.view()
    return [k for k in g if g[k] != r[k] and (k != "started" or (g["cwnd"] < g["ssthresh"] and
                                                                   r["cwnd"] < r["ssthresh"]))]


def run_events(seed, reach, **params):
    """One seeded sequence of synthetic event and cc rows into RuleCc.ack beside
    GoCubicSender.UpdateRTT / OnCongestionEvent, and RTOs as checkRTO makes
    them beside RuleCc.rto.  The numbers a call acknowledges and loses are
    n_from + 1 .. hi, acknowledged in rising order.  Returns the calls compared."""
    rng = random.Random(seed)
    now = [2 * rng.randrange(500, 500_000)]
    go, rule = cr.GoCubicSender(lambda: now[0] * cr.US, **params), cr.RuleCc(**params)
    n_from = last_sent = compared = 0
    for _ in range(rng.randint(10, 24)):
        now[0] += rng.choices(CLOCK_STEPS, STEP_WEIGHTS)[0]
        ev = _wide_fields(rng, rule)
        acked, nlost = ev["acked_packets"], ev["lost_packets"]
        hi = n_from + acked + nlost
        lost = sorted(rng.sample(range(n_from + 1, hi + 1), nlost)) if acked + nlost else []
        nlost = ev["lost_packets"] = len(lost)
        last_sent = max(last_sent, hi + rng.choice((0, 3, 40)))
        lio = rng.choice((last_sent, hi, max(n_from - 5, 0)))
        below = max(0, min(rule.cutback, hi) - n_from)    # numbers of this call at or below the cutback
        row = dict(max_lost=max(lost, default=0), max_acked=max((n for n in (hi, hi - 1, hi - 2, hi - 3)
                                                                 if n > n_from and n not in lost), default=0),
                   acked_le=below - sum(1 for n in lost if n <= rule.cutback))
        ev["largest_acked"] = row["max_acked"]
        go.OnPacketSent(last_sent)
        if ev["accepted"]:
            if ev["has_rtt"]:
                go.UpdateRTT(ev["rtt_us"] * cr.US, ev["delay_us"] * cr.US)
            gone = set(lost)
            go.OnCongestionEvent(bool(ev["has_rtt"]), ev["bytes_in_flight"],
                                 [n for n in range(n_from + 1, hi + 1) if n not in gone], lost)
            n_from = hi
        delay = rule.ack(ev, row, now[0], last_sent, lio)
        assert delay == go.RetransmissionDelay() // cr.US
        assert not _views_differ(go, rule), (seed, params, compared, "ack", _views_differ(go, rule))
        reach["slow start" if rule.in_slow_start() else "avoidance"] += 1
        reach["max_cwnd"] = max(reach["max_cwnd"], rule.cwnd)
        reach["max_time_to_origin"] = max(reach["max_time_to_origin"], rule.time_to_origin)
        reach["wrapped_cubes"] += abs(_cubic_offset(rule, now[0])) >= WRAP_OFFSET
        fired = int(rng.random() < 0.12)
        if fired:
            if rule.rto_candidate != 0 and rule.rto_candidate > go.largestSentAtLastCutback:
                go.onPacketLost(rule.rto_candidate)
            go.OnRetransmissionTimeout(True)
        bif, pb, mb = rng.choice((0, 1400, rule.cwnd * rule.p["mss"], 10 ** 12)), rng.choice((1, 1400, 9000)), \
            rng.choice((0, 8, 64))
        assert rule.rto(fired, last_sent, bif, pb, mb) == _go_budget(go, bif, pb, mb)
        assert not _views_differ(go, rule), (seed, params, compared, "rto", _views_differ(go, rule))
        compared += 1
    reach["cutbacks"] += rule.cutbacks
    reach["rtos"] += rule.rtos
    return compared


EVENT_SEEDS = range(40)


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_events_off_the_defaults_equal_the_reference(name):
    """Conditions on the generator, not measurements: what its seeds reach on
    the rules alone.  Printed, then held."""
    reach = Counter()
    total = sum(run_events(seed, reach, **PARAM_SETS[name]) for seed in EVENT_SEEDS)
    print(name, "calls compared", total, dict(reach))
    assert reach["avoidance"] > 0 and reach["cutbacks"] > 0 and reach["rtos"] > 0
    assert (reach["slow start"] > 0) != (name in NEVER_IN_SLOW_START)
    assert reach["wrapped_cubes"] > 0
    if name == "window_2_20":
        assert reach["max_cwnd"] >= 1 << 19
    # defaults: at most icbrt(cubeFactor * 199) = 8,108; floor_2_19: beta is 0.9997, a cutback takes 314 at the most
    if name in ("window_2_20", "jumbo"):
        assert reach["max_time_to_origin"] >= 1 << 14


# ---------------------------------------------------------------- every mode at once, off the defaults
# The driver of the device tests; CcRulesOnly runs it without a device, so that what the seeds reach is held
# here first.  T1 crosses 2^32 us in mid-run; T4 ends 10^8 us short of 2^64 and takes the short steps only.
EVERY_MODE_MEMBERS, EVERY_MODE_ROUNDS = 257, 12            # two blocks, the second with one lane
T1, T4 = (1 << 32) - (sum(SHORT_STEPS) + 2500), (1 << 64) - 10 ** 8    # T1: the seventh call is the first past 2^32
EVERY_MODE = [(name, 0, "long") for name in PARAM_SETS] + [("defaults", T1, "short"), ("defaults", T4, "short")]
EVERY_MODE_IDS = [f"{name}-{'0' if not base else 'T1' if base == T1 else 'T4'}" for name, base, _ in EVERY_MODE]
BUDGET_BYTES, BUDGET_MAX = (1, 1400, 9000), (0, 8, 64, 1 << 31)


def _wide_event(rng, rule, n_from):
    """An event row and a cc row as ugo_fec_cc_sent_ack could write them, off
    the generator of run_events."""
    ev = _wide_fields(rng, rule)
    acked, lost, mss = ev["acked_packets"], ev["lost_packets"], rule.p["mss"]
    hi = n_from + acked + lost
    ev.update(acked_bytes=mss * acked, lost_bytes=mss * lost, largest_acked=hi)
    row = dict(max_lost=rng.randrange(n_from, hi + 1) if lost else 0, max_acked=hi if acked else 0,
               acked_le=rng.randrange(0, acked + 1))
    return ev, row


def drive_every_mode(h, name, base, steps):
    """The body of test_controller_equals_the_rule_in_every_mode_at_once with
    the wide generator, every clock above base.  h: a CcHarness or a
    CcRulesOnly.  Returns the clocks of the calls and the wrapped cubes met."""
    nconn = h.nconn
    rng = random.Random(f"{name} {base}")
    pk = [(c, n, 1000 + 100 * (c % 5), 0, 0, 0, [(10 * n, 10)], None) for c in range(nconn) if c % 7 != 6
          for n in range(1, 2 + c % 4)]
    pk.append((1, 5000, 10, 0, 0, 0, [], None))                             # member 1 becomes inert
    h.h.record(pk, now_us=base + 1000)
    n_from = [1] * nconn
    now, clocks, wrapped = base + 2000, [], 0
    if steps == "long":                                                    # every step once, three of them twice
        schedule = list(CLOCK_STEPS) + rng.choices(CLOCK_STEPS, STEP_WEIGHTS, k=EVERY_MODE_ROUNDS - len(CLOCK_STEPS))
        rng.shuffle(schedule)
    else:
        schedule = list(SHORT_STEPS) * 2
    for step in schedule:
        now += step
        clocks.append(now)
        evs, rows = [], []
        for c in range(nconn):
            ev, row = _wide_event(rng, h.rules[c], n_from[c])
            n_from[c] = max(n_from[c], ev["largest_acked"])
            evs.append(ev), rows.append(row)
        h.ack(event_array(evs), row_array(rows), now)
        wrapped += sum(abs(_cubic_offset(x, now)) >= WRAP_OFFSET for x in h.rules)
        h.rto([int(rng.random() < 0.15) for _ in range(nconn)], rng.choice(BUDGET_BYTES), rng.choice(BUDGET_MAX))
    return clocks, wrapped


def hold_every_mode(st, name, base, clocks, where):
    """What the records of a run show at its end; the same of the rules alone
    and of ugo_fec_cc_set_state."""
    p = PARAM_SETS[name]
    live = st[np.arange(len(st)) != 1]
    slow = live["cwnd"] < live["ssthresh"]
    reach = dict(slow_start=int(slow.sum()), avoidance=int((~slow).sum()),
                 cutbacks=int(live["cutbacks"].sum()), rtos=int(live["rtos"].sum()),
                 app_limited=int(np.count_nonzero(live["app_limited_us"])),
                 epochs=int(np.count_nonzero(live["epoch_us"])), max_cwnd=int(live["cwnd"].max()),
                 max_time_to_origin=int(live["time_to_origin"].max()))
    print(where, name, "base", base, "clocks", clocks[0], "..", clocks[-1], reach)
    assert reach["avoidance"] and reach["cutbacks"] and reach["rtos"] and reach["app_limited"] and reach["epochs"]
    assert bool(reach["slow_start"]) != (name in NEVER_IN_SLOW_START)
    if name == "window_2_20":
        assert reach["max_cwnd"] >= 1 << 19 and reach["max_time_to_origin"] >= 1 << 14
    assert st["cwnd"][1] == p["initial_cwnd"] and st["cutbacks"][1] == 0 and st["rtos"][1] == 0          # inert
    assert base + 2000 < clocks[0] and clocks[-1] < 1 << 64
    if base == T1:
        below = sum(1 for t in clocks if t < 1 << 32)
        assert 3 <= below <= len(clocks) - 3, clocks                         # 2^32 falls in mid-run
    if base == T4:
        assert min(int(x) for x in live["epoch_us"] if x) > T4               # no clock wrapped to a small one


@pytest.mark.parametrize("name,base,steps", EVERY_MODE, ids=EVERY_MODE_IDS)
def test_every_mode_runs_reach_what_they_are_for(name, base, steps):
    """The rules alone through the generator and seeds of the device tests."""
    h = CcRulesOnly([1024] * EVERY_MODE_MEMBERS, 1, **PARAM_SETS[name])
    clocks, wrapped = drive_every_mode(h, name, base, steps)
    hold_every_mode(h.states(), name, base, clocks, "rules alone:")
    print("   wrapped cubes", wrapped)
    assert wrapped > 0 or steps == "short"


def _closed_form(setup, calls):
    """RuleCc with its shortcuts against the per-packet loop of the same rule.
    calls: [(G, bytes_in_flight, now_us)].  Returns the rounds the short form took."""
    fast, slow = cr.RuleCc(), cr.RuleCc(per_packet=True)
    for r in (fast, slow):
        setup(r)
    n = 0
    for g, bif, now in calls:
        ev = dict(accepted=1, has_rtt=0, rtt_us=0, delay_us=0, acked_packets=g, lost_packets=0, bytes_in_flight=bif)
        row = dict(max_lost=0, max_acked=n + g, acked_le=0)
        n += g
        for r in (fast, slow):
            r.steps = 0
            r.ack(ev, row, now, n + 10, n)
        assert fast.view() == slow.view(), (g, bif, now)
        assert slow.steps == g and fast.steps <= 8, fast.steps
    return fast


def test_closed_form_slow_start_hits_ssthresh_max_cwnd_and_the_cwnd_limit():
    def low_ssthresh(r):
        r.ssthresh, r.largest_acked = 120, 1
    r = _closed_form(low_ssthresh, [(100_000, 10 ** 9, 5000)])           # 88 increments, then CUBIC's first instant
    assert r.cwnd == 120 and r.epoch_us == 5000 and r.acked_count > 90_000
    r = _closed_form(lambda r: None, [(100_000, 10 ** 9, 5000)])          # ssthresh == max_cwnd: 168 increments
    assert r.cwnd == 200 and r.app_limited_us == 0
    # 100,000 bytes in flight: limited up to the first window with c mss >= 2 bif, 137
    r = _closed_form(lambda r: None, [(100_000, 100_000, 5000)])
    assert r.cwnd == 137 and r.app_limited_us == 5000
    for bif in (0, 1, 1459, 1460, 46_719, 46_720, 46_721, 60_000, 99_999, 145_999, 146_000, 146_001, 292_000):
        for g in (1, 2, 50, 1000):
            _closed_form(lambda r: None, [(g, bif, 7000)])


def _avoidance(r):
    r.cwnd, r.ssthresh, r.largest_acked, r.min_rtt_us = 50, 50, 1, 20_000
    r.last_max_cwnd = 80


def test_closed_form_congestion_avoidance_reaches_its_fixed_point():
    r = _closed_form(_avoidance, [(100_000, 10 ** 9, 1_000_000), (100_000, 10 ** 9, 1_010_000),
                                  (3, 10 ** 9, 1_020_000), (100_000, 10 ** 9, 9_000_000)])
    assert r.cwnd == 200 and r.epoch_us == 1_000_000


def test_closed_form_the_30_ms_boundary():
    calls = [(1000, 10 ** 9, 1_000_000), (1000, 10 ** 9, 1_030_000), (1000, 10 ** 9, 1_060_001),
             (100_000, 10 ** 9, 1_090_001), (5, 10 ** 9, 1_090_002)]
    r = _closed_form(_avoidance, calls)
    assert r.last_update_us == 1_060_001 or r.last_update_us >= 1_090_001


def test_closed_form_an_app_limited_epoch_shift():
    calls = [(1000, 10 ** 9, 1_000_000), (1000, 0, 1_500_000), (100_000, 10 ** 9, 2_000_000),
             (100_000, 70_000, 2_100_000)]
    r = _closed_form(_avoidance, calls)
    assert r.epoch_us == 1_500_000 and r.app_limited_us in (0, 2_100_000)


def test_rtt_filter_and_loss_arithmetic():
    r = cr.RuleCc()
    r._update_rtt(4000, 1000)
    assert (r.min_rtt_us, r.latest_rtt_us, r.srtt_us, r.mean_dev_us) == (4000, 3000, 3000, 1500)
    r._update_rtt(1000, 1000)                                            # sample not above the delay: kept whole
    assert r.latest_rtt_us == 1000 and r.srtt_us == 2750 and r.mean_dev_us == 1625
    r = cr.RuleCc()
    r._loss_reaction(77)
    assert (r.cwnd, r.ssthresh, r.cutback, r.last_max_cwnd, r.last_cutback_exited_slowstart) == (27, 27, 77, 32, 1)
    r._loss_reaction(99)                                                 # below the old max: betaLastMax
    assert (r.cwnd, r.last_max_cwnd, r.last_cutback_exited_slowstart) == (22, 22, 0)
    r = cr.RuleCc(min_cwnd=30)
    r._loss_reaction(1)
    assert r.cwnd == 30


def test_layouts_and_constants():
    d = fec.CC_STATE_DTYPE
    assert d.itemsize == 192 and d.names[:27] == cr.RuleCc.FIELDS
    assert [d.fields[n][1] for n in d.names] == list(range(0, 168, 8)) + [168, 172, 176, 180, 181, 182, 183]
    r = fec.CC_ROW_DTYPE
    assert r.itemsize == 32 and r.names[:3] == cr.RuleCc.ROW_FIELDS
    assert [r.fields[n][1] for n in r.names] == [0, 8, 16, 20]
    p = fec.CC_PARAMS_DTYPE
    assert p.itemsize == 20 and list(p.names) == list(cr.DEFAULTS) and fec.CC_DEFAULTS == cr.DEFAULTS
    src = open(fec.CC_HEADER_PATH).read()
    assert re.search(r"#define UGO_FEC_KERNEL_CC 14\b", src)
    assert "(192 bytes)" in src and "(32 bytes)" in src
    assert fec.KERNEL_NAMES[14] == "cc" and fec.KERNEL_IDS["cc"] == 14
    assert "UGO_FEC_KERNEL_CC" in open(fec.HEADER_PATH).read()
    go = open(fec.CC_HEADER_PATH).read()
    for letter in "abcdefghij":
        assert f"({letter})" in go


def test_symbols_are_exported_within_abi_9():
    lib = fec.load_library()
    names = [s for s in fec.header_symbols() if s.startswith("ugo_fec_cc_")]
    assert sorted(names) == ["ugo_fec_cc_sent_ack", "ugo_fec_cc_set_ack", "ugo_fec_cc_set_create",
                             "ugo_fec_cc_set_cutback", "ugo_fec_cc_set_destroy", "ugo_fec_cc_set_rto",
                             "ugo_fec_cc_set_state"]
    for s in names:
        assert hasattr(lib, s), s
    assert set(fec.header_symbols((fec.CC_HEADER_PATH,))) == set(names)  # every new symbol starts with ugo_fec_cc_
    assert lib.ugo_fec_abi_version() == 9


def test_argument_errors_that_need_no_launch():
    lib = fec.load_library()
    h = ctypes.c_void_p(1)
    assert lib.ugo_fec_cc_set_create(None, None, None, ctypes.byref(h)) == 6 and h.value is None
    assert lib.ugo_fec_cc_set_create(None, None, None, None) == 6
    assert lib.ugo_fec_cc_set_cutback(None, None) == 6
    assert lib.ugo_fec_cc_sent_ack(None, None, None, 0, None, 1, 0, None, None, None, None) == 6
    assert lib.ugo_fec_cc_set_ack(None, None, None, 0, None, None) == 6
    assert lib.ugo_fec_cc_set_rto(None, None, 1, 1, None, None) == 6
    assert lib.ugo_fec_cc_set_state(None, None) == 6
    lib.ugo_fec_cc_set_destroy(None)
    for bad in (dict(min_cwnd=0), dict(min_cwnd=33), dict(initial_cwnd=201), dict(max_cwnd=(1 << 20) + 1),
                dict(num_connections=0), dict(mss=0), dict(cwnd=1), dict(mss=1.5)):
        with pytest.raises(ValueError):
            fec.CcSet.check_params(**bad)
    assert fec.CcSet.check_params() == cr.DEFAULTS
    assert fec.CcSet.check_params(max_cwnd=1 << 20, initial_cwnd=1 << 20, min_cwnd=1)["max_cwnd"] == 1 << 20


# ---------------------------------------------------------------- GPU
import torch  # noqa: E402

from sent_harness import NO_CONN, _put  # noqa: E402

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def enc(gpu):
    return fec.New(10, 3)


def A(c, la, lio, ranges=(), w=0, delay=0, status=0, flags=0x80, nr=None):
    return (status, c, flags, Ack(la, lio, ranges, w, delay), nr)


def _lose(c, las, lio, first_after):
    """Accepted ACKs at las that have everything but (lio, first_after)."""
    return [A(c, la, lio, [(first_after, la), (lio, lio)], w=la) for la in las]


@pytest.mark.gpu
def test_sent_ack_rows_across_three_chunks_and_every_split(enc):
    """Members 0-4: window 4096, numbers 1..3000 outstanding (chunks 1..1024,
    1025..2048, 2049..3072), four ACKs that lose 1500..1510 (the second chunk)
    and free the rest up to 3000 (all three).  split 0, on a chunk boundary,
    inside a wave of the second chunk, inside the lost run, above the span.
    Member 5 across 2^32, member 6 with no accepted ACK, member 7 with err."""
    h = CcHarness(enc, [4096] * 5 + [1024] * 3, 1)
    for c in range(5):
        h.h.send(c, range(1, 3001))
    base = (1 << 32) - 300
    h.h.send(5, range(base, base + 600))
    h.h.send(6, range(1, 20))
    h.h.send(7, [1, 5000])                                                  # past the window: err
    assert h.h.rules[7].err
    acks = [a for c in range(5) for a in _lose(c, (2997, 2998, 2999, 3000), 1499, 1511)]
    acks += _lose(5, [base + k for k in (596, 597, 598, 599)], base + 99, base + 110)
    acks += [A(6, 19, 19, w=0, flags=0x20), A(7, 1, 1, w=1)]                # no ACK flag; inert
    random.Random(1).shuffle(acks)
    split = [0, 1024, 1030, 1505, 5000, 1 << 32, 7, 7]
    ev, rows = h.sent_ack(acks, max_ranges=2, split=split)
    assert rows["max_lost"].tolist() == [1510] * 5 + [base + 109, 0, 0]
    assert rows["max_acked"].tolist() == [3000] * 5 + [base + 599, 0, 0]
    assert rows["acked_le"].tolist() == [0, 1024, 1030, 1499, 2989, 300 - 9, 0, 0]
    assert ev["accepted"].tolist() == [1] * 6 + [0, 0] and ev["lost_packets"].tolist() == [11] * 5 + [10, 0, 0]
    # a second round: the span now starts at 1500; split below it, and the queued run freed by a later ACK
    for c in range(5):
        h.h.send(c, range(3001, 3200))
    ev, rows = h.sent_ack([A(c, 3199, 3199, w=4000) for c in range(5)], split=[100, 1499, 1500, 1510, 3199, 0, 0, 0])
    assert rows["acked_le"].tolist() == [0, 0, 1, 11, 11 + 199, 0, 0, 0] and not rows["max_lost"].any()
    ev, rows = h.sent_ack([])                                               # an empty batch writes the rows
    assert not rows["max_acked"].any() and not ev["accepted"].any()
    h.close()


@pytest.mark.gpu
def test_sent_ack_is_set_ack_for_the_sent_histories(enc):
    """The cases of tests/test_sent.py that pin what set_ack does to the
    histories, through the new entry point, split being the set's own array."""
    h = CcHarness(enc, [1024, 1024, 2048], 2)
    for c in range(3):
        h.h.send(c, range(1, 31))
    # three nacks in one call leave packet 1 in flight; the fourth queues it
    h.sent_ack([A(0, la, 0, [(2, la), (0, 0)], w=la) for la in (5, 6, 7)], max_ranges=3)
    assert h.h.rules[0].slots[1]["missing"] == 3
    ev, rows = h.sent_ack([A(0, 8, 0, [(2, 8), (0, 0)], w=8)])
    assert ev["lost_packets"][0] == 1 and rows["max_lost"][0] == 1 and rows["max_acked"][0] == 8
    # the same la in a wave, in two waves and in two blocks: the lowest index wins
    pk = [A(1, 0, 0, (), w=0)] * 3000
    pk[7], pk[9], pk[200], pk[2500] = (A(1, 20, 0, [(2, 20), (0, 0)], delay=1), A(1, 20, 20, (), delay=2),
                                       A(1, 20, 20, (), delay=3), A(1, 20, 20, (), delay=4))
    pk[2501], pk[1100] = A(1, 21, 21, (), delay=5), A(1, 21, 0, [(3, 21), (0, 0)], delay=6)
    ev, rows = h.sent_ack(pk, max_ranges=2)
    assert ev["delay_us"][1] == 6 and rows["max_acked"][1] == 21
    # filters: la > last_sent, a bad status, conn_of past the set, pinned operands
    ev, rows = h.sent_ack([A(2, 31, 31, w=1), A(2, 10, 10, w=2, status=3), A(7, 9, 9, w=3), A(NO_CONN, 9, 9, w=4),
                           A(2, 12, 12, w=5)], where="pinned")
    assert rows["max_acked"][2] == 12 and h.h.rules[2].unsent_acks == 1
    h.close()


def _random_event(rng, rule, sent, n_from):
    """An event row and a cc row as ugo_fec_cc_sent_ack could write them."""
    acked = rng.choice([0, 1, 2, 5, 40, 300])
    lost = rng.choice([0, 0, 0, 1, 3])
    hi = n_from + acked + lost
    ev = dict(accepted=int(rng.random() < 0.85), has_rtt=int(rng.random() < 0.8),
              rtt_us=rng.choice([0, 900, 4000, 20_000, 21_000, 60_000, 2_500_000]) + rng.randrange(0, 50),
              delay_us=rng.choice([0, 10, 3000, 10 ** 7]), acked_packets=acked, lost_packets=lost,
              acked_bytes=1400 * acked, lost_bytes=1400 * lost,
              bytes_in_flight=rng.choice([0, 3000, 40_000, 46_720, 100_000, 290_000, 10 ** 9]), largest_acked=hi)
    row = dict(max_lost=rng.randrange(n_from, hi + 1) if lost else 0, max_acked=hi if acked else 0,
               acked_le=rng.randrange(0, acked + 1))
    return ev, row


@pytest.mark.gpu
@pytest.mark.parametrize("nconn", [3, 1025, 32769])
def test_controller_equals_the_rule_in_every_mode_at_once(enc, nconn):
    """Every member gets its own random sequence of event and cc rows, so that
    the lanes of one wave are in slow start, in recovery, in congestion
    avoidance, app-limited and past an RTO at once."""
    rng = random.Random(nconn)
    h = CcHarness(enc, [1024] * nconn, 1, watch=[0, nconn - 1])
    pk = [(c, n, 1000 + 100 * (c % 5), 0, 0, 0, [(10 * n, 10)], None) for c in range(nconn) if c % 7 != 6
          for n in range(1, 2 + c % 4)]
    pk.append((1, 5000, 10, 0, 0, 0, [], None))                             # member 1 becomes inert
    h.h.record(pk)
    n_from = [1] * nconn
    rounds = 12 if nconn < 2000 else 3
    now = 1_000_000
    for r in range(rounds):
        now += rng.choice([1000, 20_000, 31_000, 200_000])
        evs, rows = [], []
        for c in range(nconn):
            ev, row = _random_event(rng, h.rules[c], h.h.rules[c], n_from[c])
            n_from[c] = max(n_from[c], ev["largest_acked"])
            evs.append(ev), rows.append(row)
        h.ack(event_array(evs), row_array(rows), now)
        h.rto([int(rng.random() < 0.15) for _ in range(nconn)], rng.choice([1, 1400, 1460]), rng.choice([0, 8, 64]))
    if nconn >= 1025:
        st = h.cc.states()
        live = st[np.arange(nconn) != 1]
        assert (live["cwnd"] < live["ssthresh"]).any() and (live["cwnd"] >= live["ssthresh"]).any()
        assert live["cutbacks"].any() and live["rtos"].any() and live["app_limited_us"].any() and live["epoch_us"].any()
        assert st["cwnd"][1] == 32 and st["cutbacks"][1] == 0 and st["rtos"][1] == 0          # inert
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,base,steps", EVERY_MODE, ids=EVERY_MODE_IDS)
def test_controller_equals_the_rule_in_every_mode_at_once_off_the_defaults(enc, name, base, steps):
    """257 members (two blocks, the second with one lane) through
    drive_every_mode: large counts, bytes in flight around each member's own
    window, idle times up to 10^13 us, budgets up to 2^31 -- per parameter set,
    and at the defaults across 2^32 us and just below 2^64."""
    n = EVERY_MODE_MEMBERS
    h = CcHarness(enc, [1024] * n, 1, watch=[0, n - 1], **PARAM_SETS[name])
    try:
        clocks, _ = drive_every_mode(h, name, base, steps)
        hold_every_mode(h.states(), name, base, clocks, "device:")
    finally:
        h.close()


BOUNDARY_SETS = {"defaults": PARAM_SETS["defaults"], "jumbo": PARAM_SETS["jumbo"],
                 "small": dict(initial_cwnd=10, max_cwnd=60, min_cwnd=3, num_connections=1, mss=1000)}


def _boundary_table(cwnd, mss):
    """(bytes_in_flight, acked_packets) around every edge of isCwndLimited for
    a window of cwnd packets, and around half of cwnd + 5 packets: there the
    closed form's ceil(2 bif / mss) decides where slow start stops."""
    w, k = cwnd * mss, cwnd + 5
    bifs = [w - 3 * mss - 1, w - 3 * mss, w - 3 * mss + 1, w // 2 - 1, w // 2, w // 2 + 1, w - 1, w, w + 1, 0,
            k * mss // 2 - 1, k * mss // 2, k * mss // 2 + 1]
    return [(b, g) for b in bifs for g in (1, 2, 50, 1000)]


def _table_call(h, table, now):
    evs = event_array([dict(accepted=1, acked_packets=g, bytes_in_flight=b) for b, g in table])
    rows = np.zeros(len(table), fec.CC_ROW_DTYPE)
    rows["max_acked"] = now
    h.ack(evs, rows, now)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BOUNDARY_SETS))
def test_the_window_limit_boundaries_off_the_defaults(enc, name):
    p = BOUNDARY_SETS[name]
    table = _boundary_table(p["initial_cwnd"], p["mss"])
    h = CcHarness(enc, [1024] * len(table), 1, watch=[0], **p)             # slow start
    _table_call(h, table, 1_000_000)
    grown = [r.cwnd - p["initial_cwnd"] for r in h.rules]
    assert 0 in grown and max(grown) >= 5 and any(r.app_limited_us for r in h.rules), grown
    assert len({g for g in grown if 0 < g < 50}) >= 3                      # stops at ssthresh aside, the stops differ
    h.close()
    # cut back once: cwnd == ssthresh.  The table of the first window and that of the window the cut left
    h = CcHarness(enc, [1024] * 2 * len(table), 1, watch=[0], **p)
    rows = np.zeros(h.nconn, fec.CC_ROW_DTYPE)
    rows["max_lost"] = 1
    h.ack(event_array([dict(accepted=1, lost_packets=1)] * h.nconn), rows, 1_000_000)
    cut = h.rules[0].cwnd
    assert all(r.cwnd == r.ssthresh == cut and r.cutbacks == 1 for r in h.rules) and cut < p["initial_cwnd"]
    both = table + _boundary_table(cut, p["mss"])
    for now in (1_050_000, 1_070_000, 1_101_000):                           # a new epoch, the 30-ms return, past it
        _table_call(h, both, now)
    assert any(r.cwnd > cut for r in h.rules) and any(r.cwnd == cut and r.app_limited_us for r in h.rules)
    assert any(r.last_update_us == 1_101_000 for r in h.rules)
    h.close()


HYSTART_MIN_RTTS = (31_992, 32_000, 32_008, 64_000, 127_992, 128_000, 128_008, 10 ** 6)


@pytest.mark.gpu
@pytest.mark.parametrize("initial_cwnd", [15, 16])
def test_hybrid_slow_starts_threshold_at_both_clamps_and_the_low_window(enc, initial_cwnd):
    """min_rtt >> 3 is 3,999, 4,000, 4,001, 8,000, 15,999, 16,000, 16,001 and
    125,000: below, at and above both clamps.  Members 0-7 see a round of eight
    samples whose minimum is min_rtt + thr (not found), members 8-15 one whose
    minimum is min_rtt + thr + 1 (found).  No event acknowledges a packet but
    the first, which is app-limited, so the window never grows: at 15 the low
    window holds the exit back in the round that finds it, at 16 it does not."""
    thr = [max(min(m >> 3, 16_000), 4000) for m in HYSTART_MIN_RTTS]
    assert thr == [4000, 4000, 4001, 8000, 15_999, 16_000, 16_000, 16_000]
    mins, thrs = HYSTART_MIN_RTTS * 2, thr * 2
    h = CcHarness(enc, [1024] * 16, 1, watch=[0], initial_cwnd=initial_cwnd)
    # the sample that sets min_rtt; its packet is past end_packet_number (0), so the round it began ends with it
    rows = np.zeros(16, fec.CC_ROW_DTYPE)
    rows["max_acked"] = 1
    h.ack(event_array([dict(accepted=1, has_rtt=1, rtt_us=m, acked_packets=1) for m in mins]), rows, 1_000_000)
    assert all(r.started == 0 and r.cwnd == initial_cwnd and r.min_rtt_us == m for r, m in zip(h.rules, mins))
    none = np.zeros(16, fec.CC_ROW_DTYPE)
    for k in range(8):                                                      # the minimum comes as the sixth sample
        extra = [(c >= 8) + (0 if k == 5 else 100 * (1 + (3 * k + c) % 7)) for c in range(16)]
        evs = event_array([dict(accepted=1, has_rtt=1, rtt_us=m + t + x) for m, t, x in zip(mins, thrs, extra)])
        h.ack(evs, none, 1_010_000 + 10_000 * k)
    assert [r.found for r in h.rules] == [0] * 8 + [1] * 8 and all(r.sample_count == 8 for r in h.rules)
    assert [r.current_min_rtt_us - r.min_rtt_us for r in h.rules] == thr + [t + 1 for t in thr]
    low = initial_cwnd < 16
    assert [r.ssthresh for r in h.rules] == [200] * 8 + [200 if low else 16] * 8
    # the next sample of a round that found it leaves slow start whatever the window (the reference's own order)
    h.ack(event_array([dict(accepted=1, has_rtt=1, rtt_us=m + 1) for m in mins]), none, 1_100_000)
    assert [r.ssthresh for r in h.rules] == [200] * 8 + [initial_cwnd] * 8
    h.close()


@pytest.mark.gpu
def test_rtt_filter_magnitudes(enc):
    """Samples from 2^10 to 2^40 us, delays above the sample (kept whole) and
    one below it (a sample of 1): the float32 lines of the rule, whose operands
    stay below 2^53 and so reach float32 in one rounding."""
    cases = []
    for m in (1 << 10, (1 << 24) + 1, 1 << 27, (1 << 32) + 12_345, (1 << 40) + 3):
        up = m + m // 3 + 1
        cases += [((m, 0), (up, 0), (m, 0)), ((up, 0), (m, 0), (up, 1)), ((m, m + 5), (m // 2 + 7, m // 2 + 6), (m, 0)),
                  ((m, m - 1), (m, 0), (m, m)), ((m, 0), (m, m - 1), (up, up + 1))]
    h = CcHarness(enc, [1024] * len(cases), 1, watch=[0])
    for k in range(3):
        h.ack(event_array([dict(accepted=1, has_rtt=1, rtt_us=c[k][0], delay_us=c[k][1]) for c in cases]),
              np.zeros(len(cases), fec.CC_ROW_DTYPE), 1_000_000 * (k + 1))
        if k == 0:                                                          # after (m, m + 5); after (m, m - 1)
            assert h.rules[2].latest_rtt_us == 1 << 10 and h.rules[3].srtt_us == 1 and h.rules[3].min_rtt_us == 1 << 10
    assert max(r.srtt_us for r in h.rules) > 1 << 40 and h.rules[-1].latest_rtt_us == cases[-1][2][0] > 1 << 40
    h.close()


@pytest.mark.gpu
def test_acked_count_wraps_as_a_uint32(enc):
    """acked_packets is a uint32 of the event row, so one call adds 2^32 - 1 at
    the most.  Member 0 takes that twice within 30 ms of a CUBIC step: the second
    wraps acked_count.  Member 1 takes it once and then a step past the 30-ms
    return, which turns a count of almost 2^32 into est_tcp_cwnd."""
    big = (1 << 32) - 1
    h = CcHarness(enc, [1024] * 2, 1)
    rows = np.zeros(2, fec.CC_ROW_DTYPE)
    rows["max_lost"] = 1
    h.ack(event_array([dict(accepted=1, lost_packets=1)] * 2), rows, 1_000_000)      # avoidance at 27
    rows = np.zeros(2, fec.CC_ROW_DTYPE)
    rows["max_acked"] = 5

    def call(g0, g1, now):
        h.ack(event_array([dict(accepted=1, acked_packets=g, bytes_in_flight=1 << 62) for g in (g0, g1)]), rows, now)

    call(big, big - 10, 1_050_000)
    before = [r.acked_count for r in h.rules]
    assert before == [big, big - 10] and all(r.cwnd < 200 for r in h.rules), before
    call(big, 0, 1_060_000)                                                 # the 30-ms return
    assert h.rules[0].acked_count == (before[0] + big) & 0xffffffff == before[0] - 1
    call(3, 3, 1_100_000)
    assert h.rules[1].est_tcp_cwnd > 50_000 and h.rules[1].cwnd == 200 and h.rules[1].acked_count < 1 << 20
    h.close()


def _fused(s1, s2):
    """(srtt, mean_dev) after samples s1 then s2 if a * b + c were one fused
    operation: 0.75 m and 0.875 s exact, one rounding.  The other two products
    are exact in float32 either way (powers of two).  All of it is exact in
    float64 up to the one rounding to float32."""
    as_f32 = lambda x: float(np.float32(x))                # noqa: E731  (the operands are float32 either way)
    md = int(np.float32(0.75 * as_f32(s1 // 2) + 0.25 * as_f32(abs(s1 - s2))))
    srtt = int(np.float32(0.875 * as_f32(s1) + 0.125 * as_f32(s2)))
    return srtt, md


def _fma_sensitive_samples(n):
    """Pairs of RTT samples whose smoothed RTT and mean deviation both come out
    different with a fused multiply-add than with the float32 lines as written."""
    rng, out = random.Random(99), []
    while len(out) < n:
        s1, s2 = rng.randrange(1 << 24, 1 << 27), rng.randrange(1 << 24, 1 << 27)
        r = cr.RuleCc()
        r._update_rtt(s1, 0), r._update_rtt(s2, 0)
        f = _fused(s1, s2)
        if f[0] != r.srtt_us and f[1] != r.mean_dev_us:
            out.append((s1, s2))
    return out


@pytest.mark.gpu
def test_rtt_filters_are_not_contracted(enc):
    samples = _fma_sensitive_samples(64)
    h = CcHarness(enc, [1024] * 64, 1, watch=[0])
    for k in (0, 1):
        evs = event_array([dict(accepted=1, has_rtt=1, rtt_us=s[k]) for s in samples])
        h.ack(evs, np.zeros(64, fec.CC_ROW_DTYPE), 1000 * (k + 1))
    st = h.cc.states()
    for c, s in enumerate(samples):
        fused = _fused(*s)
        assert st["srtt_us"][c] != fused[0] and st["mean_dev_us"][c] != fused[1], c
    h.close()


@pytest.mark.gpu
def test_a_hundred_thousand_packets_in_one_call_return_promptly(enc):
    """Member 0 acknowledges 100,000 packets in one call, in slow start and then
    in congestion avoidance; the others a handful.  The call may take ten times
    the longest of the calls in which every member acknowledges a handful: a
    lane that stepped through its packets one by one would take a thousand
    times as long."""
    h = CcHarness(enc, [1024] * 4, 1)
    big = 10 ** 9

    def call(g0, now):
        evs = event_array([dict(accepted=1, acked_packets=g0 if c == 0 else 3, bytes_in_flight=big) for c in range(4)])
        rows = np.zeros(4, fec.CC_ROW_DTYPE)
        rows["max_acked"] = now
        dev, drows = _put(evs.view(np.uint8).reshape(4, 64)), _put(rows.view(np.uint8).reshape(4, 32))
        out = torch.zeros(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.cc.ack(dev, drows, now, delay_us=out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for c, r in enumerate(h.rules):
            r.ack(evs[c], rows[c], now, 0, 0, 0)
        h.check()
        return dt

    call(3, 900_000)                                                        # the first launch loads the code
    small = max(call(3, 1_000_000 + 40_000 * k) for k in range(4))
    assert call(100_000, 2_000_000) < 10 * small                             # slow start to max_cwnd ...
    assert h.rules[0].cwnd == 200
    h.rto([1, 0, 0, 0], 1400, 8)                                            # ... an RTO: ssthresh 100
    assert call(100_000, 3_000_000) < 10 * small                             # slow start, then avoidance
    assert h.rules[0].cwnd == h.rules[0].ssthresh == 100 and h.rules[0].acked_count > 90_000
    assert call(100_000, 3_040_000) < 10 * small                             # avoidance from the first step: the
    assert h.rules[0].cwnd == 200 and h.rules[0].est_tcp_cwnd > 400          # count raises est_tcp_cwnd at once
    h.close()


@pytest.mark.gpu
def test_rto_candidates_and_budgets(enc):
    h = CcHarness(enc, [1024] * 6, 1)
    for c in range(6):
        h.h.send(c, range(1, 34), length=1460)                              # 33 * 1460 = W + 1460
    # members 0-2 lose packet 2 and cut back at last_sent 33; all free 1 and 3..8
    lose = [a for c in range(3) for a in [A(c, la, 1, [(3, la), (1, 1)], w=la) for la in (5, 6, 7, 8)]]
    ev, rows, fired, budget = h.batch(lose + [A(c, 8, 8, w=1) for c in range(3, 6)], 500_000, packet_bytes=1460)
    assert [r.cutbacks for r in h.rules] == [1, 1, 1, 0, 0, 0] and h.rules[0].cutback == 33
    assert [r.rto_candidate for r in h.rules] == [9] * 6 and fired == [0] * 6
    # fired with the candidate at or below cutback (0, 1: no second cut), above it (3, 4), and not fired (2, 5)
    fired = h.h.rto([0] * 6, 10 ** 7)
    assert fired == [1] * 6
    h.rto([1, 1, 0, 1, 1, 0], 1460, 64)
    assert [r.cutbacks for r in h.rules] == [1, 1, 1, 1, 1, 0] and [r.rtos for r in h.rules] == [1, 1, 0, 1, 1, 0]
    assert [r.cwnd for r in h.rules] == [2, 2, 27, 2, 2, 40] and h.rules[3].ssthresh == 17
    # candidate 0: nothing outstanding when ugo_fec_cc_set_ack looked
    g = CcHarness(enc, [1024] * 2, 1)
    g.h.send(0, range(1, 5), length=1460)
    g.batch([A(0, 4, 4, w=1)], 300_000)
    assert g.rules[0].rto_candidate == 0
    g.rto([1, 1], 1460, 64)
    assert [r.cutbacks for r in g.rules] == [0, 0] and [r.rtos for r in g.rules] == [1, 1]
    g.close()
    # budgets: bif == W, bif == W + 1, max_budget 0 and clamping
    b = CcHarness(enc, [1024] * 4, 1)
    b.h.send(0, range(1, 33), length=1460)                                  # bif == W = 46,720
    b.h.record([(1, n, 1460 + (n == 1), 0, 0, 0, [(n, 1)], None) for n in range(1, 33)])      # W + 1
    b.h.send(2, [1], length=20)
    assert b.rto([0] * 4, 1460, 64) == [1, 0, 32, 33]                       # (46,720 - 20) / 1460 + 1 = 32
    assert b.rto([0] * 4, 1460, 0) == [0] * 4 and b.rto([0] * 4, 1460, 5) == [1, 0, 5, 5]
    assert b.rto([0] * 4, 1, 1 << 31) == [1, 0, 46_701, 46_721]
    b.close()
    h.close()


@pytest.mark.gpu
def test_pinned_operands_and_kernel_class(enc):
    h = CcHarness(enc, [1024, 4096], 1)
    h.h.send(0, range(1, 9)), h.h.send(1, range(1, 9))
    enc.timing_begin(64)
    try:
        ev, rows = h.sent_ack([A(c, la, 0, [(2, la), (0, 0)], w=la) for c in range(2) for la in (5, 6, 7, 8)],
                              where="pinned")
        h.ack(ev, rows, 9000, where="pinned")
        h.rto([0, 1], 1400, 8, where="pinned")
    finally:
        recs, untimed = enc.timing_end()
    assert untimed == 0
    # ugo_fec_cc_sent_ack 5 launches, ugo_fec_cc_set_ack 1, ugo_fec_cc_set_rto 1 (the state gathers are not timed)
    assert recs["kernel"].tolist() == [14] * 7
    h.close()


@pytest.mark.gpu
def test_argument_errors_on_the_device(enc):
    lib = fec.load_library()
    bad = fec.ErrInvalidArg.code
    h = CcHarness(enc, [1024, 1024], 1)
    h.h.send(0, [1, 2])
    out = ctypes.c_void_p(1)
    other = fec.New(4, 2)
    assert lib.ugo_fec_cc_set_create(other._h, h.h.set._h, None, ctypes.byref(out)) == bad and out.value is None
    for p in ((0, 200, 2, 2, 1460), (32, 200, 0, 2, 1460), (32, 31, 2, 2, 1460), (32, (1 << 20) + 1, 2, 2, 1460),
              (32, 200, 33, 2, 1460), (32, 200, 2, 0, 1460), (32, 200, 2, 2, 0)):
        arr = np.array([p], fec.CC_PARAMS_DTYPE)
        assert lib.ugo_fec_cc_set_create(enc._h, h.h.set._h, arr.ctypes.data, ctypes.byref(out)) == bad
        assert out.value is None
    buf = {k: torch.full((n,), 0x11, dtype=torch.uint8, device="cuda")
           for k, n in (("info", 256), ("ranges", 256), ("conn", 16), ("ev", 128), ("rows", 64), ("u64", 16),
                        ("u8", 2), ("u32", 8))}
    p = {k: v.data_ptr() for k, v in buf.items()}
    host = torch.zeros(256, dtype=torch.uint8).data_ptr()                   # pageable
    sa = lambda **k: lib.ugo_fec_cc_sent_ack(  # noqa: E731
        h.h.set._h, k.get("info", p["info"]), k.get("ranges", p["ranges"]), k.get("mr", 4), k.get("conn", p["conn"]),
        k.get("n", 4), 5, k.get("ev", p["ev"]), k.get("split", p["u64"]), k.get("rows", p["rows"]), None)
    assert sa(info=None) == bad and sa(ranges=None) == bad and sa(conn=None) == bad and sa(ev=None) == bad
    assert sa(split=None) == bad and sa(rows=None) == bad and sa(rows=p["rows"] + 8) == bad
    assert sa(split=p["u64"] + 4) == bad and sa(mr=0x10000) == bad and sa(rows=host) == bad and sa(split=host) == bad
    assert sa(n=(1 << 31) + 1) == bad
    ca = lambda **k: lib.ugo_fec_cc_set_ack(  # noqa: E731
        h.cc._h, k.get("ev", p["ev"]), k.get("rows", p["rows"]), 5, k.get("delay", p["u64"]), None)
    assert ca(ev=None) == bad and ca(rows=None) == bad and ca(delay=None) == bad and ca(ev=p["ev"] + 8) == bad
    assert ca(rows=p["rows"] + 8) == bad and ca(delay=p["u64"] + 4) == bad and ca(ev=host) == bad
    assert ca(delay=host) == bad
    cr_ = lambda **k: lib.ugo_fec_cc_set_rto(  # noqa: E731
        h.cc._h, k.get("fired", p["u8"]), k.get("pb", 1400), k.get("mb", 8), k.get("budget", p["u32"]), None)
    assert cr_(fired=None) == bad and cr_(budget=None) == bad and cr_(pb=0) == bad and cr_(mb=(1 << 31) + 1) == bad
    assert cr_(budget=p["u32"] + 2) == bad and cr_(fired=host) == bad and cr_(budget=host) == bad
    torch.cuda.synchronize()
    assert all(bool((t == 0x11).all()) for t in buf.values())
    h.check(sent=True)
    # a controller set whose sent set is gone refuses every call
    g = CcHarness(enc, [1024], 1)
    g.h.set.close()                                                         # closes the controller set first
    assert g.cc._h is None
    g.h.close()
    other.close()
    h.close()


KEY = b"\x0f\x1e\x2d\x3c\x4b\x5a\x69\x78"


def _trace(log, cc, last=24):
    """The last rounds of the round trip, for a failure's message: per round
    fired, budget, delay_us, and per member (accepted, acked, lost, bytes in
    flight, rto_count, lio, last_sent)."""
    out = []
    for events, crows, delays, fired, budget, st_ack, st_rto, t in log[-last:]:
        ev = events.cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)
        out.append((t, fired.tolist(), budget.tolist(), delays.tolist(),
                    [(int(e["accepted"]), int(e["acked_packets"]), int(e["lost_packets"]), int(s["bytes_in_flight"]),
                      int(s["rto_count"]), int(s["lio"]), int(s["last_sent"])) for e, s in zip(ev, st_rto)]))
    st = cc.states()
    return out, [(int(x["cwnd"]), int(x["ssthresh"]), int(x["cutback"]), int(x["rtos"])) for x in st]


@pytest.mark.gpu
def test_round_trip_of_two_peers_with_congestion_control_on_the_device(enc):
    """The two-peer lossy round trip of tests/test_sent.py with the controllers
    in the chain: budget is the array ugo_fec_cc_set_rto wrote, delays the array
    ugo_fec_cc_set_ack wrote, split the set's own cutback array, all passed on
    as device tensors.  The host reads only sizes (total, total_out, n_read).
    At the end every member's controller equals a RuleCc fed the same rows.

    The peer's receive histories hold 4,096 numbers, not the 1,024 of
    tests/test_sent.py: member 2 starts at packet 2,001, which a history of
    1,024 numbers that starts at 0 drops as out of window until a stop-waiting
    raises it.  There a fixed budget lets the retransmission that carries the
    stop-waiting out after the first RTO; here, as in the reference, the window
    is 2 after an RTO and the 13 packets still in flight keep the budget at 0,
    so the stop-waiting would never leave and the peer never acknowledge."""
    rng = np.random.default_rng(5)
    d, n, S, slot, MR, MS, G = 10, 13, 1470, 1488, 8, 2, 3
    NP = G * d
    dev = torch.device("cuda")
    pad = _put(np.frombuffer(fec.rc4_keystream(KEY, slot), np.uint8)[:slot].copy())
    sizes = [30_000, 45_000, 20_011]
    data = [rng.integers(0, 256, k, dtype=np.uint8) for k in sizes]
    i64 = dict(dtype=torch.int64, device=dev)
    txA = [fec.StreamTx(enc, 65536, 64, 0, 1000 * c) for c in range(3)]
    tsetA = fec.StreamTxSet(enc, txA)
    sentA = [fec.SentTx(enc, 1024, MS) for _ in range(3)]
    ssetA = fec.SentTxSet(enc, sentA)
    ccA = fec.CcSet(enc, ssetA)
    ackA = [fec.AckRx(enc, 1024) for _ in range(3)]
    asetA = fec.AckRxSet(enc, ackA)
    rxB = [fec.StreamRx(enc, 65536) for _ in range(3)]
    rsetB = fec.StreamRxSet(enc, rxB)
    ackB = [fec.AckRx(enc, 4096) for _ in range(3)]
    asetB = fec.AckRxSet(enc, ackB)
    txB = [fec.StreamTx(enc, 4096, 4) for _ in range(3)]
    tsetB = fec.StreamTxSet(enc, txB)
    src = torch.from_numpy(np.concatenate(data)).to(dev)
    off = torch.tensor([0, sizes[0], sizes[0] + sizes[1]], **i64)
    written = tsetA.write(src, off, torch.tensor(sizes, **i64))
    assert written.tolist() == sizes
    zero_budget = torch.zeros(3, dtype=torch.int32, device=dev)
    may = torch.ones(3, dtype=torch.uint8, device=dev)
    want_all = torch.full((3,), 1 << 20, **i64)
    dst = torch.zeros(3 << 20, dtype=torch.uint8, device=dev)
    dst_off = torch.arange(3, **i64) << 20
    got = [bytearray() for _ in range(3)]
    planA = planB = None
    rangesA = torch.zeros((NP, MR, 2), **i64)
    rangesB = torch.zeros((8, MR, 2), **i64)
    budget = ccA.rto(torch.zeros(3, dtype=torch.uint8, device=dev), S, 8)   # the first budget: nothing in flight
    split = ccA.cutback()
    log = []                                                                # what the rules are fed, read at the end
    rounds = 0
    now = 1_000_000
    while any(len(g) < s for g, s in zip(got, sizes)):
        rounds += 1
        if rounds > 200:
            for line in _trace(log, ccA, last=200)[0]:
                print(line)
        assert rounds <= 200, ([len(g) for g in got], _trace(log, ccA, last=2))
        now += 150_000
        # ---- A sends what the budget allows
        planA = tsetA.plan(budget, NP, max_segments=MS, out=planA)
        info, segs, conn, first, count, total = planA
        asetA.attach(now, first, count, total, info, rangesA, conn)
        ssetA.attach(first, count, info)
        npk = int(total.item())                                             # a size
        wire_in = torch.zeros((NP, slot), dtype=torch.uint8, device=dev)
        lens_in = torch.full((NP,), 16, dtype=torch.int16, device=dev)
        if npk:
            w, l, st = tsetA.encode(info, rangesA, segs, conn, slot, npackets=npk, framed=True)
            ssetA.record(info, segs, conn, l, st, now, npackets=npk)
            wire_in[:npk], lens_in[:npk] = w, l
        wire = torch.zeros((G * n, slot), dtype=torch.uint8, device=dev)
        wl = torch.zeros(G * n, dtype=torch.int16, device=dev)
        gst = torch.full((G,), -1, dtype=torch.int8, device=dev)
        enc.tx_assemble(wire_in, lens_in, wire, wl, first_seq=0, pad=pad, status=gst)
        # ---- the link: a fixed 5 % of the wire packets is lost
        wl_rx = wl.clone()
        wl_rx[torch.arange(G * n, device=dev) % 20 == (7 * rounds) % 20] = 0
        frames = torch.zeros((n, G, slot), dtype=torch.uint8, device=dev)
        present = torch.zeros(G, **i64)
        enc.rx_assemble(wire, wl_rx, frames, present, shard_size=S, pad=pad, frames=True)
        rows = frames[:d].reshape(d * G, slot)
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
        ainfo, aranges = binfo, rangesB
        if nb:
            bw, bl, bst = tsetB.encode(binfo, rangesB, bsegs, bconn, slot, npackets=nb, pad=pad)
            ainfo, aranges, _ = enc.packet_decode(bw, bl, pad=pad, max_ranges=MR, max_segments=MS)
        # ---- A hears of it: every link of this chain reads what the one before wrote on the device
        events, crows = ccA.sent_ack(ainfo, aranges, bconn, now + 3000, npackets=nb, split=split)
        before_ack = ssetA.states()                                         # the test's own look, for the rules
        delays = ccA.ack(events, crows, now + 3000)
        fired = ssetA.rto(delays, now + 4000)
        budget = ccA.rto(fired, S, 8)
        log.append((events.clone(), crows.clone(), delays.clone(), fired.clone(), budget.clone(), before_ack,
                    ssetA.states(), now + 3000))
        rc, ro, rlen, n_entries, touch, upto = ssetA.drain(64)
        tsetA.retransmit(rc, ro, rlen)
        asetA.touch(touch)
        tsetA.release(upto)
    for c in range(3):
        assert bytes(got[c]) == data[c].tobytes(), c
    rules = [cr.RuleCc() for _ in range(3)]
    assert [r.rto(0, 0, 0, S, 8) for r in rules] == [8, 8, 8]
    for events, crows, delays, fired, budget, st_ack, st_rto, t in log:
        ev = events.cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)
        rw = crows.cpu().numpy().view(fec.CC_ROW_DTYPE).reshape(-1)
        f = fired.cpu().numpy()
        for c, r in enumerate(rules):
            want = r.ack(ev[c], rw[c], t, int(st_ack["last_sent"][c]), int(st_ack["lio"][c]), int(st_ack["err"][c]))
            assert int(delays[c]) == want
            want = r.rto(int(f[c]), int(st_rto["last_sent"][c]), int(st_rto["bytes_in_flight"][c]), S, 8,
                         int(st_rto["err"][c]))
            assert int(budget[c]) == want
    st = ccA.states()
    for c, r in enumerate(rules):
        for k, v in r.view().items():
            assert int(st[k][c]) == v, (c, k, int(st[k][c]), v)
    assert int(st["cutbacks"].sum()) > 0 and not ssetA.states()["err"].any()
    assert np.array_equal(split.cpu().numpy().view(np.uint64), st["cutback"])
    for x in (ccA, tsetA, ssetA, asetA, rsetB, asetB, tsetB):
        x.close()
    for x in txA + sentA + ackA + rxB + ackB + txB:
        x.close()
