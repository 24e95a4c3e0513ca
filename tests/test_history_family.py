"""Seeded traffic families (tests/history_family.py) for the sent and the
receive histories: on the CPU the rules alone, to hold what the families reach;
on the device one family per test, call by call, under the harnesses' own
checks (tests/sent_harness.py, tests/cc_harness.py, tests/ack_harness.py)."""
import pytest

import history_family as hf
from ugo_amd import fec

# (seed, max_ranges) of every family the GPU tests run; the CPU test below
# drives the rules alone through each of them.
SENT = [(5, 4), (2, 4), (3, 8)]
CC = [7]
CC_MAX_RANGES = 4
ACK = [(2, 2), (6, 4)]
PINNED = (25, 4)
PINNED_ROUNDS = 10
ACK_ROUNDS = 12

# The floors of a family: conditions on the inputs, not measurements.  The rules
# alone reach, over the sent and cc seeds above (20 rounds): 1-4 live members
# three windows past their first number, 4-10 across 2^32, 5-10 long spans,
# 549-622 ACKs of one member in a call, 226-264 pairs with two ACKs of one la,
# 646-725 mixed stretches, 44-104 pairs with a queued slot present, 35-81 RTOs,
# 8-10 clamped drains, 36,000 truncated SACKs and more.
# The last three are what an arithmetic slip in the ack kernels needs in order
# to show, counted by history_family.run from the rules' records:
#   accepting_waves  64-packet stretches of an ACK batch in which five members or
#                    more have an accepted ACK: wave_add's lane-by-lane tail.
#                    They are the mixed stretches that matter, and get their floor.
#   carried_ends     (member, call) pairs with an accepted la in an earlier quarter
#                    of a 1,024-number chunk and a slot that stays in a later one:
#                    run_e carried from round to round in k_sent_ack_apply.
#   queued_freed     (member, call) pairs in which an ACK frees a queued slot:
#                    lost_pk - qfreed in k_sent_ack_finish.
#                    Both need a queued slot or a loss present, and get the floor
#                    of the pairs with a queued slot present.
FLOORS = dict(lapped=1, across_2_32=1, long_spans=5, most_acks=200, same_la_pairs=50, mixed_stretches=100,
              queued_present=20, rtos=10, clamped_drains=3, truncated=1, accepting_waves=100, carried_ends=20,
              queued_freed=20)
# The family on pinned operands has 10 rounds and the same floors but one: its
# bursts are at most a quarter of a window, so in 10 rounds no member can pass
# three windows, and a member once round its ring stands in for that.
SHORT_FLOORS = dict(FLOORS, lapped=0, lapped_once=1)
# What the receiving side of a family must have been given: attaches whose SACK
# was cut at max_ranges, numbers that were repeats or below the floor (counted
# old), 64-packet stretches of a receive batch naming five members or more, and
# members attached.  Its families have 12 rounds: the sending side is only their
# source, on the rules alone.
RX_FLOORS = dict(rx_truncated=1, rx_old=500, rx_mixed_stretches=100, rx_attached=100)


# The same families from real clocks, 8 rounds each (the floors above are for 20 rounds and do not apply).
# T1 starts 6,750 or 8,750 us below 2^32 us (71.6 minutes of uptime), so that the boundary falls between the record
# and the ack of the round whose RTO step follows: the third round of the sent family, the fourth of the others.
# T2 is a wall clock in us, T3 is no double, T4 ends 10^8 us short of 2^64 (a clock of 0 means unset, and no call
# may pass 2^64).
CLOCK_ROUNDS = 8
T2, T3, T4 = 1_760_000_000_000_000, (1 << 53) + 1, (1 << 64) - 10 ** 8
CLOCK_SENT, CLOCK_CC, CLOCK_ACK = (2, 4), 7, (6, 4)
T1_SENT, T1_CC, T1_ACK = hf.EDGE - 6750, hf.EDGE - 8750, hf.EDGE - 8750
SENT_BASES = [T1_SENT, T2, T3, T4]
CC_BASES = [T1_CC, T2, T3, T4]
ACK_BASES = [T1_ACK, T2, T3]


def _clock_family(kind, start_us):
    if kind == "cc":
        return hf.Family(CLOCK_CC, CC_MAX_RANGES, rounds=CLOCK_ROUNDS, start_us=start_us)
    return hf.Family(*(CLOCK_SENT if kind == "sent" else CLOCK_ACK), rounds=CLOCK_ROUNDS, start_us=start_us)


def _hold(fam, st, floors):
    print(fam, {k: st[k] for k in floors}, "inert", st["inert"], "inert peers", st["inert_peers"])
    for k, v in floors.items():
        assert st[k] >= v, f"{fam}: {k} is {st[k]}, below {v}: {dict(st)}"
    quarter = fam.nconn // 4
    assert st["inert"] <= quarter and st["inert_peers"] <= quarter, f"{fam}: {dict(st)}"


def test_the_families_reach_what_they_are_for():
    """The rules alone through every (seed, parameters) of the GPU tests."""
    inert = 0
    for seed, mr in SENT:
        fam = hf.Family(seed, mr)
        st = hf.run(fam, hf.RuleOps(fam))
        _hold(fam, st, FLOORS)
        inert += st["inert"]
    for seed in CC:
        fam = hf.Family(seed, CC_MAX_RANGES)
        st = hf.run(fam, hf.RuleCcOps(fam))
        _hold(fam, st, FLOORS)
        inert += st["inert"]
    for seed, mr in ACK:
        fam = hf.Family(seed, mr, rounds=ACK_ROUNDS)
        st = hf.run(fam, hf.RuleOps(fam), hf.RuleRx(fam))
        _hold(fam, st, RX_FLOORS)
        assert st["rx_inert"] <= fam.nconn // 4, dict(st)
    fam = hf.Family(*PINNED, rounds=PINNED_ROUNDS)
    st = hf.run(fam, hf.RuleOps(fam))
    _hold(fam, st, SHORT_FLOORS)
    inert += st["inert"]
    assert inert >= 1, "no sent family on the device keeps an inert member beside live ones"


def test_the_families_at_real_clocks_reach_what_they_are_for():
    """The rules alone through every (family, base) of the GPU tests: no run is
    idle, and the runs from T1 carry an RTT sample, an RTO and a lo_time_us
    across 2^32 us."""
    for kind, bases in (("sent", SENT_BASES), ("cc", CC_BASES), ("ack", ACK_BASES)):
        for base in bases:
            fam = _clock_family(kind, base)
            ops = hf.RuleCcOps(fam) if kind == "cc" else hf.RuleOps(fam)
            st = hf.run(fam, ops, hf.RuleRx(fam) if kind == "ack" else None)
            keys = ("first_clock", "last_clock", "rtos", "cutbacks", "clamped_drains", "queued_present", "rtt_across",
                    "rto_across", "lo_time_across", "rx_attached", "inert", "inert_peers", "rx_inert")
            print(kind, fam, {k: st[k] for k in keys})
            assert base == st["first_clock"] < st["last_clock"] < 1 << 64
            assert st["rtos"] >= 1 and st["clamped_drains"] + st["queued_present"] >= 1, dict(st)
            assert kind != "cc" or st["cutbacks"] >= 1, dict(st)
            quarter = fam.nconn // 4
            assert st["inert"] <= quarter and st["inert_peers"] <= quarter and st["rx_inert"] <= quarter, dict(st)
            if base in (T1_SENT, T1_CC, T1_ACK):
                assert st["first_clock"] < hf.EDGE < st["last_clock"]
                if kind == "ack":                          # its sending side is the rules alone, only a source
                    assert st["lo_time_across"] >= 1 and st["rx_attached"] >= 1, dict(st)
                else:
                    assert st["rtt_across"] >= 1 and st["rto_across"] >= 1, dict(st)
            else:
                assert st["rtt_across"] == st["rto_across"] == st["lo_time_across"] == 0
                assert (st["first_clock"] < hf.EDGE) == (st["last_clock"] < hf.EDGE)


def test_a_failing_call_is_named_and_can_be_replayed_without_a_gpu():
    fam = hf.Family(11, 4, nconn=5, rounds=3)

    class Failing(hf.RuleOps):
        def ack(self, packets, max_ranges, now_us):
            ev = hf.RuleOps.ack(self, packets, max_ranges, now_us)
            assert now_us < hf.START_US + 5000, "record field lio differs"       # the second round's call
            return ev

    with pytest.raises(hf.FamilyFailure) as e:
        hf.run(fam, Failing(fam))
    text = str(e.value)
    assert "seed 11" in text and "round 1, call ack" in text and "record field lio differs" in text
    assert "describe(11, 4, 5, 3, 1, 'ack', cc=False, rx=False)" in text

    class Broken(hf.RuleOps):                          # not an assertion: an error of the binding or the runtime
        def drain(self, max_entries):
            raise RuntimeError("hipErrorInvalidValue")

    with pytest.raises(hf.FamilyFailure, match="round 0, call drain: RuntimeError: hipErrorInvalidValue"):
        hf.run(hf.Family(11, 4, nconn=5, rounds=3), Broken(fam))
    out = []
    hf.describe(11, 4, 5, 3, 1, "ack", out=out)
    assert "round 1, call ack" in out[0] and sum(1 for line in out if line.startswith("member ")) == 5
    assert any("Ack(la=" in line for line in out)
    out = []
    hf.describe(11, 2, 5, 3, 2, "ack_attach", rx=True, out=out)
    assert any("may_ack_only" in line for line in out) and "largest_in_order" in out[-2] + out[-1]


# ---------------------------------------------------------------- GPU
from ack_harness import AckHarness  # noqa: E402
from cc_harness import CcHarness  # noqa: E402
from sent_harness import SentHarness  # noqa: E402


@pytest.fixture(scope="module")
def enc(gpu):
    return fec.New(10, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,max_ranges", SENT)
def test_sent_family_on_the_device(enc, seed, max_ranges):
    """attach, record, ack, rto, drain of one family; every member watched."""
    fam = hf.Family(seed, max_ranges)
    h = SentHarness(enc, fam.wss, fam.seg_cap)
    try:
        hf.run(fam, hf.DeviceOps(h))
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", CC)
def test_sent_family_through_cc_sent_ack(enc, seed):
    """The ack / rto step is CcHarness.batch: ugo_fec_cc_sent_ack with the set's
    own cutback array as split, cc_set_ack, sent_set_rto with the delays just
    written, cc_set_rto.  The script's clock and ACK delays are even."""
    fam = hf.Family(seed, CC_MAX_RANGES)
    ch = CcHarness(enc, fam.wss, fam.seg_cap)
    try:
        hf.run(fam, hf.DeviceCcOps(ch, fam.max_ranges))
    finally:
        ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,max_ranges", ACK)
def test_ack_family_on_the_device(enc, seed, max_ranges):
    """receive, then attach with may_ack_only, from the arrivals of a family
    whose sending side runs on the rules alone."""
    fam = hf.Family(seed, max_ranges, rounds=ACK_ROUNDS)
    h = AckHarness(enc, fam.wss)
    try:
        hf.run(fam, hf.RuleOps(fam), hf.DeviceRx(h))
    finally:
        h.close()


@pytest.mark.gpu
def test_sent_family_on_pinned_operands(enc):
    fam = hf.Family(*PINNED, rounds=PINNED_ROUNDS)
    h = SentHarness(enc, fam.wss, fam.seg_cap)
    try:
        hf.run(fam, hf.DeviceOps(h, where="pinned"))
    finally:
        h.close()


def _base_id(base):
    return "T1" if base < 1 << 33 else "T2" if base == T2 else "T3" if base == T3 else "T4"


@pytest.mark.gpu
@pytest.mark.parametrize("base", SENT_BASES, ids=_base_id)
def test_sent_family_at_real_clocks(enc, base):
    fam = _clock_family("sent", base)
    h = SentHarness(enc, fam.wss, fam.seg_cap)
    try:
        hf.run(fam, hf.DeviceOps(h))
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("base", CC_BASES, ids=_base_id)
def test_cc_family_at_real_clocks(enc, base):
    fam = _clock_family("cc", base)
    ch = CcHarness(enc, fam.wss, fam.seg_cap)
    try:
        hf.run(fam, hf.DeviceCcOps(ch, fam.max_ranges))
    finally:
        ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("base", ACK_BASES, ids=_base_id)
def test_ack_family_at_real_clocks(enc, base):
    fam = _clock_family("ack", base)
    h = AckHarness(enc, fam.wss)
    try:
        hf.run(fam, hf.RuleOps(fam), hf.DeviceRx(h))
    finally:
        h.close()
