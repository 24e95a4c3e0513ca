"""The whole device chain against its composed rules, call by call
(tests/chain_ref.py, tests/chain_harness.py): two endpoints live through a
seeded script, and every output of every call of every batch is compared whole
with what the rules of the stages, run in THE ORDER of include/ugo_loop.h, say
it must be."""
import pytest

import chain_ref as ch
import listen_ref as lr
import loop_ref as lf
from ugo_amd import fec

# The runs of this module: the script's seed, the size, and the per-call capacities.  The seeds are chosen so
# that test_the_script_reaches_what_it_is_for holds; nothing else distinguishes them.
RUNS = {
    "n3": dict(seed=6, n=3, max_ranges=8, max_packets=16, max_exits=3, max_entries=64),
    "n257": dict(seed=1, n=257, max_ranges=8, max_packets=512, max_exits=257, max_entries=512),
    "mr2": dict(seed=11, n=70, max_ranges=2, max_packets=128, max_exits=70, max_entries=128),
    "mr3": dict(seed=18, n=70, max_ranges=3, max_packets=128, max_exits=70, max_entries=128),
    "clamp": dict(seed=2, n=70, max_ranges=8, max_packets=24, max_exits=4, max_entries=16),
}
SERVER = dict(seed=4, n=40, max_conn=64, max_ranges=8, max_packets=96, max_exits=40, max_entries=96)
ROUND_CAP = 200


# The n = 3 run once more with other congestion parameters (the family of tests/test_cc.py) from a wall clock.
OTHER_CC = dict(initial_cwnd=10, max_cwnd=60, min_cwnd=3, num_connections=1, mss=1000)
WALL_CLOCK_US = 1_760_000_000_000_000


def run(name, make, start_us=ch.START_US, **more):
    """The run `name` with make(n, now, **capacities) as both endpoints.  Returns (script, A, B, stats)."""
    kw = dict(RUNS[name], **more)
    scr = ch.script(kw.pop("seed"), kw["n"])
    n = kw.pop("n")
    A, B = make(n, start_us, idle_us=scr.idle_us, **kw), make(n, start_us, idle_us=scr.idle_us, **kw)
    return scr, A, B, ch.run_pair(scr, A, B, round_cap=ROUND_CAP, start_us=start_us)


def lives_hold(scr, A, B, st):
    """What must be true of every run, whatever the script drew."""
    assert st["done"] and st["rounds"] <= ROUND_CAP, (st["rounds"], len(A.exits), len(B.exits))
    for c, m in enumerate(scr.members):
        if st["reasons"][0][c] == lf.CLOSED and st["reasons"][1][c] == lf.CLOSED:
            assert bytes(B.got[c]) == m.data[0] and bytes(A.got[c]) == m.data[1], c
        for side in (0, 1):
            fin, data = st["fin_round"][side].get(c), st["data_round"][side].get(c)
            assert fin is None or data is None or fin > data, (side, c, fin, data)


def run_server(make_server, device):
    """The server run: make_server(max_conn, now, **capacities) against scripted rule clients."""
    kw = dict(SERVER)
    scr = ch.script(kw.pop("seed"), kw["n"])
    n, max_conn = kw.pop("n"), kw.pop("max_conn")
    C = ch.RuleEndpoint(n, ch.START_US, idle_us=scr.idle_us, **kw)
    S = make_server(max_conn, ch.START_US, idle_us=scr.idle_us, **kw)
    return S, ch.run_server(scr, S, C, device, round_cap=ROUND_CAP)


def server_holds(st):
    n = SERVER["n"]
    assert st["done"] and st["rounds"] <= ROUND_CAP, st["rounds"]
    assert st["classes"] >= {lr.FED, lr.FED_NEW, lr.DUP_INIT, lr.ACCEPT, lr.STRANGER}, st["classes"]
    assert st["accepted"] == n + 1 and st["remaps"] > 1
    before, member = st["again"]                                                  # accepted again: the next number
    assert 0 < before == member < SERVER["max_conn"], st["again"]
    assert len(st["reasons"][0]) == n and len(st["reasons"][1]) == n
    assert st["late"] > 0                         # packets arrived for members that had exited and were still listed


def test_the_script_reaches_what_it_is_for():
    """The rule pair alone through every run of this module: conditions on the
    inputs of the GPU tests, checked where no GPU is."""
    reasons, total = set(), dict.fromkeys(("lost_fin", "ack_only", "fired", "retx_delivered"), 0)
    stats = {}
    for name in RUNS:
        scr, A, B, st = run(name, ch.RuleEndpoint)
        lives_hold(scr, A, B, st)
        stats[name] = st
        reasons |= set(st["reasons"][0].values()) | set(st["reasons"][1].values())
        for k in total:
            total[k] += st[k]
    every = set(range(1, 12)) - {lf.STREAM_ERR, lf.ACK_ERR, lf.SENT_ERR}
    assert reasons >= every, sorted(every - reasons)
    assert stats["mr2"]["trunc_acks"] > 0 and stats["mr3"]["trunc_acks"] > 0      # a truncated SACK reached set_ack
    assert stats["n257"]["trunc_acks"] == 0                                       # and none where max_ranges is 8
    assert stats["clamp"]["pending_rounds"] > 0                                   # a member stayed pending in append
    assert stats["clamp"]["over_exits"] > 0                                       # more exits than max_exits in a round
    assert all(v > 0 for v in total.values()), total
    assert stats["n257"]["lost_fin"] > 0
    for name in ("n3", "n257", "mr2", "mr3", "clamp"):                             # packets arrive for exited members
        assert stats[name]["late"] > 0, name
    server_holds(run_server(ch.RuleServer, False)[1])
    scr, A, B, st = run("n3", ch.RuleEndpoint, WALL_CLOCK_US, cc_params=OTHER_CC)
    lives_hold(scr, A, B, st)
    print("n3 with", OTHER_CC, "from", WALL_CLOCK_US, {k: st[k] for k in ("rounds", "fired", "retx_delivered", "late")},
          "cutbacks", sum(k.cutbacks for E in (A, B) for k in E.cc), "rtos", sum(k.rtos for E in (A, B) for k in E.cc))
    assert st["fired"] > 0 and all(k.p == dict(OTHER_CC) for k in A.cc) and max(k.cwnd for k in A.cc + B.cc) <= 60


# ---------------------------------------------------------------- GPU
from chain_harness import ChainHarness, ServerHarness  # noqa: E402


@pytest.fixture(scope="module")
def enc(gpu):
    return fec.New(10, 3)


def run_on_device(enc, name, where="device", **more):
    made = []

    def make(n, now, **kw):
        made.append(ChainHarness(enc, n, now, kw.pop("max_ranges"), kw.pop("max_packets"), where=where, **kw))
        return made[-1]

    try:
        scr, A, B, st = run(name, make, **more)
        lives_hold(scr, A, B, st)
        return st
    finally:
        for h in made:
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 257])
def test_chain_equals_the_rules_call_by_call(enc, n):
    """257 is the smallest size at which the one-lane-per-member kernels cross
    a block, and one wave holds live, closing, lingering, failing and exited
    lanes together."""
    run_on_device(enc, f"n{n}")


@pytest.mark.gpu
def test_chain_with_other_congestion_parameters_from_a_wall_clock(enc):
    """The controllers of both endpoints at (10, 60, 3, 1, 1000), every clock
    above 2^50 us."""
    st = run_on_device(enc, "n3", start_us=WALL_CLOCK_US, cc_params=OTHER_CC)
    assert st["fired"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("max_ranges", [2, 3])
def test_chain_with_truncated_sacks(enc, max_ranges):
    """attach truncates the runs, decode clamps with the same max_ranges and
    cc_sent_ack is fed them: the rule says which ACKs were truncated."""
    st = run_on_device(enc, f"mr{max_ranges}")
    assert st["trunc_acks"] > 0


@pytest.mark.gpu
def test_chain_when_the_capacities_clamp(enc):
    """max_packets below what plan, append and attach ask for and max_exits
    below the exits of a round: the pending FIN or RST goes out later, n_exits
    counts past max_exits, the rest is listed by the next call and new_index
    is whole every time."""
    st = run_on_device(enc, "clamp")
    assert st["pending_rounds"] > 0 and st["over_exits"] > 0


@pytest.mark.gpu
def test_server_accepts_serves_remaps_and_accepts_again(enc):
    """A connection table in front of the chain, 40 scripted rule clients behind
    the link.  The INITs and the first data arrive in one ring, interleaved, so
    FED_NEW packets lie behind ACCEPT, with two v4-mapped names, a dup-INIT and
    a stranger among them; the sets are created from accepted[] before deliver;
    when a round lists exits and three or more wait, new_index goes to
    listen_remap and the sets are rebuilt over the survivors, whose windows and
    histories carry on -- until then the exited members stay listed, and what
    arrives for them is masked; then a closed address sends an INIT again and
    is accepted under the next number."""
    made = []

    def make(max_conn, now, **kw):
        made.append(ServerHarness(enc, max_conn, now, kw.pop("max_ranges"), kw.pop("max_packets"), **kw))
        return made[-1]

    try:
        server_holds(run_server(make, True)[1])
    finally:
        for s in made:
            s.close()


@pytest.mark.gpu
def test_chain_on_pinned_operands(enc):
    """The arrays a host reads -- conn_of, the sizes, deadline_us, n_exits -- in pinned memory."""
    run_on_device(enc, "n3", where="pinned")
