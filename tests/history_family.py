"""Seeded traffic for the sent and the receive histories; test infrastructure
only.

A Family is a script of rounds for nconn members that knows nothing of what
consumes it.  run() plays it into a consumer round by round, in THE ORDER of
include/ugo_sent.h: attach, record, [link], ack, maybe rto, maybe drain.  The
consumer is a small adapter with attach / record / ack / rto / drain and the
list of its RuleSent (`rules`):

  RuleOps     the rules of tests/sent_ref.py alone
  RuleCcOps   the same with one RuleCc of tests/cc_ref.py per member: the ack
              step is ugo_fec_cc_sent_ack, cc_set_ack, sent_set_rto with the
              delays just written, cc_set_rto
  DeviceOps   a SentHarness      DeviceCcOps   a CcHarness

The link is one RuleAck of tests/ack_ref.py per member (the peer): it loses
packets, receives every arrival on its own and answers 60 % of them with a
SACK snapshot cut to max_ranges.  The same arrivals, with repeats and numbers
below the floor, go as one shuffled batch to an optional receiving consumer
(RuleRx, DeviceRx), followed by one attach whose first / counts / total are as
set_plan would leave them.

What the script decides depends on the seed alone, but for two values it reads
from the consumer's rules: the stop-waiting attach handed out, and the number
of queued segments a drain is sized by.  run() counts what the traffic reached
(Family.stats); describe() replays a family on the rules alone up to one call
and prints that call's inputs per member.

Every clock of a run is start_us plus what the script adds.  EDGE is 2^32 us:
run() counts the RTT samples, the RTOs and the receive side's lo_time_us that
reach across it, for the runs that start just below it.
"""
import random
from collections import Counter

import ack_ref as ar
import cc_ref as cr
import sent_ref as sr
from sent_ref import Ack

M64 = (1 << 64) - 1
NO_CONN = 0xffffffff
WINDOWS = (1024, 2048, 4096)
FIRSTS = (1, 5000, (1 << 32) - 700)
P_NONE = 0.15                          # no burst; else a long one of ws/8 .. ws/4, else 1 .. 12 packets
P_LONG = {1024: 0.7, 2048: 0.3, 4096: 0.3}   # the short windows talk most: they are the ones that lap their ring
P_ROUND_LOST, P_SWAP, P_SACK, P_AGAIN = 0.07, 0.05, 0.6, 0.03
P_RTO, P_DRAIN, P_HALF = 0.15, 0.85, 0.5
RTO_STEP_US = 600_000
START_US = 1_000_000
EDGE = 1 << 32


class Family:
    def __init__(self, seed, max_ranges, nconn=24, rounds=20, seg_cap=2, start_us=START_US):
        self.seed, self.max_ranges, self.nconn, self.rounds, self.seg_cap = seed, max_ranges, nconn, rounds, seg_cap
        self.start_us = start_us
        rng = self.rng = random.Random(seed)
        self.wss = [rng.choice(WINDOWS) for _ in range(nconn)]
        self.first = [rng.choice(FIRSTS) for _ in range(nconn)]
        self.loss = [rng.uniform(0.0, 0.2) for _ in range(nconn)]
        self.peers = [ar.RuleAck(ws) for ws in self.wss]
        for peer, n in zip(self.peers, self.first):    # the handshake told the peer where the numbers start
            peer.receive([(0, n)])
        self.nxt = list(self.first)                    # the next number of every member
        self.off = [0] * nconn                         # ... and its next stream offset
        self.w = [0] * nconn                           # the peer's own packet numbers
        self.flight = [[] for _ in range(nconn)]       # this round's packets on the wire
        self.spent = []                                # ACKs of earlier rounds, to be replayed
        self.stats = Counter()

    def __repr__(self):
        at = "" if self.start_us == START_US else f", from {self.start_us} us"
        return f"family seed {self.seed}, max_ranges {self.max_ranges}, {self.nconn} members, {self.rounds} rounds{at}"

    # ---------------------------------------------------------------- attach
    def plan(self):
        """The bursts of a round -> (n_packets, first_packet, total)."""
        rng, counts = self.rng, []
        for ws in self.wss:
            x = rng.random()
            counts.append(0 if x < P_NONE else rng.randint(ws // 8, ws // 4) if x < P_NONE + P_LONG[ws]
                          else rng.randint(1, 12))
        first, cur = [], 0
        for k in counts:
            first.append(cur)
            cur += k
        return counts, first, cur

    # ---------------------------------------------------------------- record
    def record_batch(self, counts, sw_of):
        """[(conn, n, wire_len, status, flags, stop_waiting, segments, None)],
        all members shuffled together.  sw_of: {member: the stop-waiting attach
        wrote}; it rides on the burst's first packet."""
        rng, pk = self.rng, []
        for c, k in enumerate(counts):
            self.flight[c] = []
            for j in range(k):
                n = self.nxt[c]
                self.nxt[c] += 1
                segs = []
                for _ in range(rng.randint(1, self.seg_cap)):
                    ln = rng.randint(1, 700)
                    segs.append((self.off[c], ln))
                    self.off[c] += ln
                length = rng.randint(40, 1400)
                flags = rng.choice((0x20, 0x20, 0x20, 0x00, 0xA0, 0x80))
                sw = sw_of.get(c, 0) if j == 0 else 0
                fate = rng.random() if j else 1.0
                if fate < 0.003:                       # failed to encode: the number is spent, nothing is stored
                    pk.append((c, n, length, rng.choice((1, 3, 7)), flags, sw, segs, None))
                    continue
                if fate < 0.006:                       # nothing on the wire
                    pk.append((c, n, 0, 0, flags, sw, segs, None))
                    continue
                pk.append((c, n, length, 0, flags, sw, segs, None))
                self.flight[c].append((n, sw, len(segs)))
                if rng.random() < 0.01:                # a second copy of the number: the lower index is stored
                    pk.append((c, n, length + 1, 0, flags ^ 0x80, 0, segs[:1], None))
        for _ in range(rng.randint(2, 6)):             # packets of no member, and without a number
            c = rng.randrange(self.nconn)
            kind = rng.randrange(3)
            conn = (self.nconn + rng.randrange(40), NO_CONN, c)[kind]
            n = (self.nxt[c] + 3, self.nxt[c], 0)[kind]
            pk.append((conn, n, 100, 0, 0x20, 0, [(7, 7)], None))
        rng.shuffle(pk)
        return pk

    # ---------------------------------------------------------------- link
    def _snapshot(self, c):
        peer = self.peers[c]
        la, _, rows, how = peer.sack(self.max_ranges)
        self.stats["truncated"] += how == ar.TRUNCATED
        self.w[c] += 1
        return (0, c, self.rng.choice((0x80, 0xA0)), Ack(la, peer.lio, rows, self.w[c], 2 * self.rng.randrange(1500)),
                None)

    def link(self):
        """What the peers make of the round -> (ack batch, receive batch):
        [(status, conn, flags, Ack, None)] and [(status, conn, n, stop_waiting,
        n_segments)], each shuffled over the members."""
        rng, acks, arrivals = self.rng, [], []
        for c, sent in enumerate(self.flight):
            peer = self.peers[c]
            if not sent:
                continue
            if rng.random() < P_ROUND_LOST:
                self.stats["rounds_lost"] += 1
                continue
            got = [p for p in sent if rng.random() >= self.loss[c]]
            i = 0
            while i + 1 < len(got):                    # a neighbour overtakes now and then
                if rng.random() < P_SWAP:
                    got[i], got[i + 1] = got[i + 1], got[i]
                    i += 1
                i += 1
            for n, sw, nseg in got:
                peer.receive([(n, sw)])
                arrivals.append((0, c, n, sw, nseg))
                if rng.random() < P_AGAIN:
                    arrivals.append((0, c, n, 0, nseg))
                if rng.random() < P_SACK:
                    acks.append(self._snapshot(c))
                    if rng.random() < P_AGAIN:         # the same snapshot under a fresh w
                        acks.append(self._snapshot(c))
            for _ in range(rng.randrange(3)):          # numbers below the floor
                n = peer.lio - rng.randrange(40)
                if n > 0:
                    arrivals.append((0, c, n, 0, 1))
        for _ in range(rng.randint(2, 6)):             # ACKs that take no part, or are not valid
            c = rng.randrange(self.nconn)
            kind = rng.randrange(5)
            a = Ack(self.nxt[c] - 1, self.nxt[c] - 1, [], 0, 0)
            if kind == 0 and self.spent:               # an old w again
                acks.append(rng.choice(self.spent))
            elif kind == 1:                            # for a number never sent
                self.w[c] += 1
                acks.append((0, c, 0x80, Ack(self.nxt[c] + 2, self.nxt[c] + 2, [], self.w[c], 0), None))
            elif kind == 2:
                acks.append((rng.choice((1, 3)), c, 0x80, a, None))
            elif kind == 3:
                acks.append((0, c, 0x20, a, None))
            else:
                acks.append((0, rng.choice((self.nconn + rng.randrange(40), NO_CONN)), 0x80, a, None))
            arrivals.append((rng.choice((0, 3)), rng.choice((c, self.nconn + 1, NO_CONN)), self.nxt[c] + 1, 0, 1))
        if acks:
            self.spent = rng.sample(acks, min(4, len(acks)))
        rng.shuffle(acks)
        rng.shuffle(arrivals)
        return acks, arrivals

    # ---------------------------------------------------------------- the receiving side's attach
    def rx_plan(self, rx_rules):
        """first / counts / total as set_plan would leave them for the reverse
        direction, may_ack_only and a max_packets that now and then leaves the
        last third of the ACK-only slots out."""
        rng = self.rng
        counts = [int(rng.random() < 0.3) for _ in range(self.nconn)]
        may = [int(rng.random() < 0.9) for _ in range(self.nconn)]
        clamp = rng.random() < 0.2
        first, cur = [], 0
        for k in counts:
            first.append(cur)
            cur += k
        want = sum(1 for c, r in enumerate(rx_rules) if r.changed and not r.err and not counts[c] and may[c])
        return first, counts, cur, max(1, cur + want - (want // 3 if clamp else 0)), may


# -------------------------------------------------------------------- consumers
class RuleOps:
    """The rules alone."""

    def __init__(self, fam):
        self.rules = [sr.RuleSent(ws, fam.seg_cap) for ws in fam.wss]

    def attach(self, first, counts, max_packets):
        return sr.attach_set(self.rules, first, counts, max_packets)[0]

    def record(self, packets, max_segments, now_us):
        sr.record_set(self.rules, [(p[0], p[1] & M64, p[2], p[3], p[4], p[5], p[6][:max_segments]) for p in packets],
                      now_us)

    def ack(self, packets, max_ranges, now_us):
        return sr.ack_set(self.rules, [(st, c, fl, a, len(a.ranges)) for st, c, fl, a, _ in packets], now_us,
                          max_ranges)

    def rto(self, delays, now_us):
        return sr.rto_set(self.rules, delays, now_us)

    def drain(self, max_entries):
        sr.drain_set(self.rules, max_entries)


class RuleCcOps(RuleOps):
    """CcHarness.batch on the rules alone."""

    def __init__(self, fam, packet_bytes=1400, max_budget=64):
        RuleOps.__init__(self, fam)
        self.cc = [cr.RuleCc() for _ in self.rules]
        self.packet_bytes, self.max_budget = packet_bytes, max_budget
        self.fired, self.max_ranges = [], fam.max_ranges

    def ack(self, packets, max_ranges, now_us):
        before = [{n: s["state"] for n, s in r.slots.items()} for r in self.rules]
        splits = [k.cutback for k in self.cc]
        ev = RuleOps.ack(self, packets, max_ranges, now_us)
        delays = []
        for c, (s, k) in enumerate(zip(self.rules, self.cc)):
            row = cr.cc_row(before[c], s, ev[c], splits[c])
            delays.append(k.ack(ev[c], row, now_us, s.last_sent, s.lio, s.err))
        self.fired = sr.rto_set(self.rules, delays, now_us)
        for f, s, k in zip(self.fired, self.rules, self.cc):
            k.rto(f, s.last_sent, s.bytes_in_flight, self.packet_bytes, self.max_budget, s.err)
        return ev

    def rto(self, delays, now_us):                     # an empty batch; the controller's own delays, not the script's
        self.ack([], self.max_ranges, now_us)
        return self.fired


class DeviceOps:
    """A SentHarness: every check is the harness's own, after every call."""

    def __init__(self, h, where="device"):
        self.h, self.rules, self.where = h, h.rules, where

    def attach(self, first, counts, max_packets):
        return self.h.attach(first, counts, max_packets, where=self.where)[0]

    def record(self, packets, max_segments, now_us):
        self.h.record(packets, max_segments=max_segments, now_us=now_us, where=self.where)

    def ack(self, packets, max_ranges, now_us):
        return self.h.ack(packets, max_ranges=max_ranges, now_us=now_us, where=self.where)

    def rto(self, delays, now_us):
        return self.h.rto(delays, now_us, where=self.where)

    def drain(self, max_entries):
        self.h.drain(max_entries, where=self.where)


class DeviceCcOps(DeviceOps):
    """A CcHarness: the ack and the rto step are CcHarness.batch, the rest goes
    to its SentHarness."""

    def __init__(self, ch, max_ranges):
        DeviceOps.__init__(self, ch.h)
        self.ch, self.cc = ch, ch.rules
        self.fired, self.max_ranges = [], max_ranges

    def ack(self, packets, max_ranges, now_us):
        ev, _, self.fired, _ = self.ch.batch(packets, now_us, max_ranges=max_ranges)
        return ev

    def rto(self, delays, now_us):
        self.ack([], self.max_ranges, now_us)
        return self.fired


class RuleRx:
    """The receiving side on the rules alone."""

    def __init__(self, fam):
        self.rules = [ar.RuleAck(ws) for ws in fam.wss]

    def receive(self, packets, now_us):
        ar.receive_set(self.rules, [(st, c, n & M64, sw & M64, nseg, None) for st, c, n, sw, nseg in packets], now_us)

    def attach(self, first, counts, total, max_packets, max_ranges, may, now_us):
        return ar.attach_set(self.rules, now_us, first, counts, total, may, max_packets, max_ranges)[2]


class DeviceRx:
    """An AckHarness."""

    def __init__(self, h, where="device"):
        self.h, self.rules, self.where = h, h.rules, where

    def receive(self, packets, now_us):
        self.h.receive(packets, now_us=now_us, where=self.where)

    def attach(self, first, counts, total, max_packets, max_ranges, may, now_us):
        return self.h.attach(first, counts, total, max_packets, max_ranges, may=may, now_us=now_us,
                             where=self.where)[5]


# -------------------------------------------------------------------- the rounds
class FamilyFailure(AssertionError):
    pass


class _Stop(Exception):
    pass


def _note_acks(fam, acks, rules):
    """What an ACK batch is, before it is applied."""
    st = fam.stats
    per = [Counter() for _ in rules]
    for status, c, flags, a, _ in acks:
        if status == 0 and flags & 0x80 and c < fam.nconn:
            per[c][a.la] += 1
    for c, las in enumerate(per):
        n = sum(las.values())
        st["most_acks"] = max(st["most_acks"], n)
        st["same_la_pairs"] += any(v > 1 for v in las.values())
        st["queued_present"] += bool(n and not rules[c].err and rules[c].queued)
    for i in range(0, len(acks), 64):
        st["mixed_stretches"] += len({p[1] for p in acks[i:i + 64]}) >= 5
    # The accepted ACKs, from the records as they stand (steps 1 and 3 of set_ack): a wave of the batch in
    # which five members or more have one is a wave whose adds to the difference rings go past wave_add's
    # four shared addresses.
    accepted = [{} for _ in rules]                     # member -> {la: batch index}
    for i, (status, c, flags, a, _) in enumerate(acks):
        if status or not flags & 0x80 or c >= fam.nconn or rules[c].err:
            continue
        x = rules[c]
        if a.la <= x.last_sent and (a.w == 0 or a.w > x.largest_with_ack) and a.la > max(x.largest_acked, x.lio):
            accepted[c].setdefault(a.la, i)
    waves = Counter()
    for c, las in enumerate(accepted):
        for i in set(i // 64 for i in las.values()):
            waves[i] += 1
    st["accepting_waves"] += sum(1 for v in waves.values() if v >= 5)
    return accepted


def _note_ack_result(fam, rules, accepted, pre):
    """What an ACK call met, after it: per (member, call) pair, whether it freed
    a slot that was queued, and whether an accepted la lay in an earlier quarter
    of a chunk of 1,024 numbers in which a later quarter keeps an occupied slot
    at or below the highest accepted la -- there the count of the accepted ACKs
    with n <= la depends on what the quarters before handed on."""
    st = fam.stats
    for c, x in enumerate(rules):
        las = accepted[c]
        if not las or x.err:
            continue
        n0, queued = pre[c]
        st["queued_freed"] += any(n not in x.slots for n in queued)
        lam = max(las)
        ends = {}                                      # chunk -> the earliest quarter holding an accepted la
        for la in las:
            k, q = divmod(la - n0, 1024)
            ends[k] = min(ends.get(k, 4), q // 256)
        st["carried_ends"] += any(n <= lam and (n - n0) % 1024 // 256 > ends.get((n - n0) // 1024, 4)
                                  for n in x.slots if n >= n0)


def run(fam, ops, rx=None, stop=None, out=None):
    """Plays the family into ops (and the arrivals into rx).  A failing call is
    re-raised as FamilyFailure naming seed, round and call.  stop = (round,
    call name): return before that call, after describing it to out."""
    rng, st, rules = fam.rng, fam.stats, ops.rules
    now = fam.start_us
    st["first_clock"] = now

    def across(pre_sent_us, fired, t):
        """RTOs that fired at t >= EDGE on a last_sent_us from below it."""
        st["rto_across"] += sum(1 for f, u in zip(fired, pre_sent_us) if f and 0 < u < EDGE <= t)

    def call(r, name, fn, *args):
        if stop == (r, name):
            _describe(fam, r, name, args, ops, rx, out)
            raise _Stop
        try:
            return fn(*args)
        except FamilyFailure:
            raise
        except Exception as e:                         # a harness assertion, or an error of the binding or the runtime
            raise FamilyFailure(f"{fam}: round {r}, call {name}: {type(e).__name__}: {e}\n"
                                f"replay without a GPU: history_family.describe({fam.seed}, {fam.max_ranges}, "
                                f"{fam.nconn}, {fam.rounds}, {r}, {name!r}, cc={isinstance(ops, (RuleCcOps, DeviceCcOps))}, "
                                f"rx={rx is not None}" + ("" if fam.start_us == START_US else f", start_us={fam.start_us}")
                                + ")"
                                ) from e

    try:
        if rx is not None:                             # the peers' start, as Family gave it to its own
            call(-1, "receive", rx.receive, [(0, c, 0, n, 0) for c, n in enumerate(fam.first)], now)
        for r in range(fam.rounds):
            now += 2000
            counts, first, total = fam.plan()
            writes = call(r, "attach", ops.attach, first, counts, max(1, total))
            member = {first[c]: c for c in range(fam.nconn) if counts[c]}
            pk = fam.record_batch(counts, {member[t]: sw for t, sw in writes})
            st["stop_waitings"] += len(writes)
            st["largest_batch"] = max(st["largest_batch"], len(pk))
            call(r, "record", ops.record, pk, fam.seg_cap, now)
            acks, arrivals = fam.link()
            if rx is not None:
                call(r, "receive", rx.receive, arrivals, now + 500)
                for i in range(0, len(arrivals), 64):
                    st["rx_mixed_stretches"] += len({p[1] for p in arrivals[i:i + 64]}) >= 5
                plan = fam.rx_plan(rx.rules)
                lo_times = [x.lo_time_us for x in rx.rules]
                att = call(r, "ack_attach", rx.attach, *plan[:4], fam.max_ranges, plan[4], now + 1500)
                st["lo_time_across"] += sum(1 for a, u in zip(att, lo_times) if a and 0 < u < EDGE <= now + 1500)
                st["rx_truncated"] += sum(1 for a in att if a == ar.TRUNCATED)
                st["rx_attached"] += sum(1 for a in att if a)
            accepted = _note_acks(fam, acks, rules)
            pre = [(min(x.scan_from, x.lio + 1), x.last_sent) for x in rules]
            # the first number set_ack scans (never more than a window below last_sent), and what is queued
            pre2 = [(max(lo, hi - x.ws + 1, 1), [n for n, s in x.slots.items() if s["state"] == sr.QUEUED])
                    for x, (lo, hi) in zip(rules, pre)]
            sent_us = [x.last_sent_us for x in rules]
            ev = call(r, "ack", ops.ack, acks, fam.max_ranges, now + 1000)
            st["rtt_across"] += sum(1 for e in ev if e["has_rtt"] and now + 1000 - int(e["rtt_us"]) < EDGE <= now + 1000)
            across(sent_us, getattr(ops, "fired", []), now + 1000)
            for c, (lo, hi) in enumerate(pre):
                st["long_spans"] += bool(ev[c]["accepted"] and hi - lo + 1 > 1024)
                assert bool(ev[c]["accepted"]) == bool(accepted[c]), (c, "the script's own reading of set_ack is off")
            _note_ack_result(fam, rules, accepted, pre2)
            fired = getattr(ops, "fired", [])
            if rng.random() < P_RTO:
                delays = [rng.choice((0, 0, 100_000, 300_000)) for _ in rules]
                now += RTO_STEP_US
                sent_us = [x.last_sent_us for x in rules]
                again = call(r, "rto", ops.rto, delays, now + 1000)
                across(sent_us, again, now + 1000)
                fired = [a or b for a, b in zip(again, fired or [0] * fam.nconn)]
            st["rtos"] += sum(fired)
            if rng.random() < P_DRAIN:
                m = sum(x.queued_segments for x in rules if not x.err)
                if rng.random() < P_HALF:
                    m //= 2
                call(r, "drain", ops.drain, max(1, m))
                st["clamped_drains"] += any(x.queued for x in rules if not x.err)
    except _Stop:
        return st
    st["last_clock"] = now + 1000
    st["cutbacks"] = sum(k.cutbacks for k in getattr(ops, "cc", []))
    live = [c for c, x in enumerate(rules) if not x.err]
    st["inert"] = fam.nconn - len(live)
    st["inert_peers"] = sum(1 for p in fam.peers if p.err)
    st["lapped"] = sum(1 for c in live if rules[c].last_sent - fam.first[c] >= 3 * fam.wss[c])
    st["lapped_once"] = sum(1 for c in live if rules[c].last_sent - fam.first[c] >= fam.wss[c])
    st["across_2_32"] = sum(1 for c in live if fam.first[c] < 1 << 32 <= rules[c].last_sent)
    if rx is not None:
        st["rx_inert"] = sum(1 for x in rx.rules if x.err)
        st["rx_old"] = sum(x.old for x in rx.rules)
    return st


# -------------------------------------------------------------------- reading a failure without a GPU
def _describe(fam, r, name, args, ops, rx, out):
    p = (lambda *a: print(*a)) if out is None else (lambda *a: out.append(" ".join(str(x) for x in a)))
    p(f"{fam}: the inputs of round {r}, call {name}")
    rules = rx.rules if name in ("receive", "ack_attach") else ops.rules
    per = [[] for _ in range(fam.nconn)]
    other = []
    if name == "record":
        for i, (c, n, length, status, flags, sw, segs, _) in enumerate(args[0]):
            (per[c] if c < fam.nconn else other).append((i, n, length, status, hex(flags), sw, segs))
        p("per packet: (batch index, number, wire_len, status, flags, stop_waiting, segments)")
    elif name == "ack":
        for i, (status, c, flags, a, _) in enumerate(args[0]):
            (per[c] if c < fam.nconn else other).append((i, status, hex(flags), a))
        p(f"per packet: (batch index, status, flags, Ack); max_ranges {args[1]}, now_us {args[2]}")
    elif name == "receive":
        for i, (status, c, n, sw, nseg) in enumerate(args[0]):
            (per[c] if c < fam.nconn else other).append((i, status, n, sw, nseg))
        p(f"per packet: (batch index, status, number, stop_waiting, n_segments); now_us {args[1]}")
    elif name == "attach":
        per = [[("first_packet", f, "n_packets", k)] for f, k in zip(args[0], args[1])]
        p(f"max_packets {args[2]}")
    elif name == "ack_attach":
        per = [[("first_packet", f, "n_packets", k, "may_ack_only", m)] for f, k, m in zip(args[0], args[1], args[5])]
        p(f"total {args[2]}, max_packets {args[3]}, max_ranges {args[4]}, now_us {args[6]}")
    elif name == "rto":
        per = [[("delay_us", d)] for d in args[0]]
        p(f"now_us {args[1]} (a controller's own delays take the place of these)")
    elif name == "drain":
        p(f"max_entries {args[0]}")
    for c, x in enumerate(rules):
        state = x.record() if isinstance(x, ar.RuleAck) else x.record_fields()
        p(f"member {c} (window {fam.wss[c]}, first number {fam.first[c]}) before the call: {state}")
        for item in per[c]:
            p("   ", item)
    if other:
        p("packets of no member:", other)


def describe(seed, max_ranges, nconn, rounds, r, name, cc=False, rx=False, out=None, start_us=START_US):
    """Replays the family on the rules alone up to call `name` of round r and
    prints that call's inputs and every member's record before it.  rx: the
    family also fed a receiving consumer (which draws from the same seed)."""
    fam = Family(seed, max_ranges, nconn, rounds, start_us=start_us)
    run(fam, RuleCcOps(fam) if cc else RuleOps(fam), RuleRx(fam) if rx else None, stop=(r, name), out=out)
