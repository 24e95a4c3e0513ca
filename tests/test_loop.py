"""The connection loop on the GPU (include/ugo_loop.h): THE RULE against a
restatement of ugo/conn.go on the CPU, the device against the rule."""
import ctypes
import random
import re

import numpy as np
import pytest

import loop_ref as lf
import packet_ref as pr
import sent_ref as sr
from ugo_amd import fec

M64 = (1 << 64) - 1


# ================================================================ CPU: layouts, symbols, arguments
def test_layouts_and_constants():
    d = fec.LOOP_STATE_DTYPE
    assert d.itemsize == 64 and d.names[:13] == lf.RuleLoop.FIELDS
    assert [d.fields[n][1] for n in d.names] == [0, 8, 16, 24, 32, 40, 41, 42, 43, 44, 45, 46, 47, 48]
    p = fec.LOOP_PARAMS_DTYPE
    assert p.itemsize == 24 and list(p.names[:3]) == list(lf.DEFAULTS) and fec.LOOP_DEFAULTS == lf.DEFAULTS
    assert [p.fields[n][1] for n in p.names] == [0, 8, 16, 20]
    src = open(fec.LOOP_HEADER_PATH).read()
    for name, value in (("UGO_FEC_KERNEL_LOOP", 16), ("UGO_LOOP_PEER_ACK_FIN", 1), ("UGO_LOOP_PEER_RST", 2),
                        ("UGO_LOOP_BAD_PACKET", 3), ("UGO_LOOP_CLOSED", 4), ("UGO_LOOP_FAILURES", 5),
                        ("UGO_LOOP_SENT_ERR", 6), ("UGO_LOOP_ACK_ERR", 7), ("UGO_LOOP_STREAM_ERR", 8),
                        ("UGO_LOOP_IDLE", 9), ("UGO_LOOP_LINGER", 10), ("UGO_LOOP_ABORT", 11),
                        ("UGO_LOOP_PENDING_FIN", 1), ("UGO_LOOP_PENDING_RST", 2)):
        assert re.search(rf"#define {name} {value}\b", src), name
    assert (fec.LOOP_PEER_ACK_FIN, fec.LOOP_CLOSED, fec.LOOP_FAILURES, fec.LOOP_IDLE, fec.LOOP_LINGER,
            fec.LOOP_ABORT) == (lf.PEER_ACK_FIN, lf.CLOSED, lf.FAILURES, lf.IDLE, lf.LINGER, lf.ABORT) == (1, 4, 5, 9,
                                                                                                        10, 11)
    assert (fec.LOOP_HOW_CLOSE, fec.LOOP_HOW_ABORT, fec.LOOP_HOW_NODELAY_ON, fec.LOOP_HOW_NODELAY_OFF) == (1, 2, 4, 8)
    assert "(64 bytes)" in src
    assert fec.KERNEL_NAMES[16] == "loop" and fec.KERNEL_IDS["loop"] == 16
    assert "UGO_FEC_KERNEL_LOOP" in open(fec.HEADER_PATH).read()
    for letter in "abcdefgh":
        assert f"({letter})" in src
    # the reference's constants
    assert lf.DEFAULTS == dict(ack_delay_us=5000, idle_us=300_000_000, max_retries=10)


def test_symbols_are_exported_within_abi_9():
    lib = fec.load_library()
    names = [s for s in fec.header_symbols() if s.startswith("ugo_fec_loop_")]
    assert sorted(names) == ["ugo_fec_loop_set_" + s for s in ("append", "check", "close", "create", "destroy",
                                                              "receive", "sent", "state")]
    for s in names:
        assert hasattr(lib, s), s
    assert set(fec.header_symbols((fec.LOOP_HEADER_PATH,))) == set(names)
    assert lib.ugo_fec_abi_version() == 9


def test_argument_errors_that_need_no_launch():
    lib = fec.load_library()
    h = ctypes.c_void_p(1)
    assert lib.ugo_fec_loop_set_create(None, None, None, None, None, None, 0, ctypes.byref(h)) == 6
    assert h.value is None
    assert lib.ugo_fec_loop_set_create(None, None, None, None, None, None, 0, None) == 6
    assert lib.ugo_fec_loop_set_receive(None, None, None, 1, 0, None) == 6
    assert lib.ugo_fec_loop_set_receive(None, None, None, 0, 0, None) == 6
    assert lib.ugo_fec_loop_set_close(None, None, None, 0, None) == 6
    assert lib.ugo_fec_loop_set_check(None, 0, None, None, None) == 6
    assert lib.ugo_fec_loop_set_append(None, None, 0, None, None, 1, None, None, None, None) == 6
    assert lib.ugo_fec_loop_set_sent(None, None, None, None, 0, None, None, None, 0, None, None, None, None) == 6
    assert lib.ugo_fec_loop_set_state(None, None) == 6
    lib.ugo_fec_loop_set_destroy(None)
    for bad in (dict(idle_us=0), dict(max_retries=1 << 32), dict(ack_delay_us=-1), dict(idle=1),
                dict(ack_delay_us=1.5)):
        with pytest.raises(ValueError):
            fec.LoopSet.check_params(**bad)
    assert fec.LoopSet.check_params() == lf.DEFAULTS
    assert fec.LoopSet.check_params(max_retries=0, idle_us=1)["idle_us"] == 1


# ================================================================ CPU: closed forms of the rule
def _closed(now=0, **kw):
    r = lf.RuleLoop(now)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_closed_form_the_delayed_ack_boundary():
    r = _closed()
    assert r.receive([(0, 0x20, 7)], 1000) == 1 and r.origin_ack_us == 1000
    assert r.check(1000 + 5000, lf.NB_IDLE) == (False, 0)             # now - origin == ack_delay_us: not yet
    assert r.check(1000 + 5001, lf.NB_IDLE) == (False, 1)
    r.ack_no_delay = 1
    assert r.check(1000, lf.NB_IDLE) == (False, 1)
    r.ack_no_delay = 0
    assert r.sent(True, 0, 1000, lf.NB_IDLE) == 1000 + 300_000_000 and r.origin_ack_us == 0
    assert r.check(1001, lf.NB_IDLE) == (False, 1)                    # unset reads as long ago
    r.receive([(0, 0x80, 0)], 2000)                                   # a pure ACK carries no number
    assert r.origin_ack_us == 0


def test_closed_form_the_idle_boundary():
    r = _closed(50)
    assert r.check(50 + 300_000_000 - 1, lf.NB_IDLE) == (False, 1) and not r.exited
    assert r.check(50 + 300_000_000, lf.NB_IDLE) == (True, 0)
    assert (r.exited, r.reason, r.pending, r.exit_us) == (1, lf.IDLE, lf.RST, 50 + 300_000_000)


def test_closed_form_the_failure_boundary():
    r = _closed()
    assert r.check(1, dict(lf.NB_IDLE, rto_count=10)) == (False, 1) and not r.exited
    assert r.check(1, dict(lf.NB_IDLE, rto_count=11)) == (True, 0) and r.reason == lf.FAILURES and r.pending == lf.RST


def test_closed_form_the_order_of_the_exit_tests():
    nb = dict(lf.NB_IDLE, stream_err=4, ack_err=1, sent_err=1, rto_count=99)
    want = [lf.STREAM_ERR, lf.ACK_ERR, lf.SENT_ERR, lf.FAILURES, lf.LINGER, lf.IDLE]
    for k, key in enumerate(("stream_err", "ack_err", "sent_err", "rto_count", None, None)):
        r = _closed(closed=1, linger_deadline_us=5)
        if k == 5:
            r.linger_deadline_us = 0
        r.check(300_000_000, nb)
        assert r.reason == want[k], (k, r.reason)
        if key:
            nb[key] = 0


def test_closed_form_the_fin_conditions_one_at_a_time():
    ready = dict(lf.NB_IDLE, tail=700, write_pos=700)
    for nb in (dict(ready, tail=701), dict(ready, rq_len=1), dict(ready, tracked=1)):
        r = _closed(closed=1)
        assert r.check(1, nb) == (False, 1) and r.pending == lf.NONE
    r = _closed()
    assert r.check(1, ready) == (False, 1) and r.pending == lf.NONE                  # not closed
    r = _closed(closed=1, fin_sent=1)
    assert r.check(1, ready) == (True, 1) and r.pending == lf.NONE                   # sent already
    r = _closed(closed=1)
    assert r.check(1, ready) == (True, 1) and r.pending == lf.FIN and not r.exited
    rules = [r]
    writes, appended, total = lf.append_set(rules, [ready], 3, 4)
    assert writes == [(3, 0, lf.FIN, 700, 700)] and appended == [1] and total == 4
    assert (r.fin_sent, r.pending, r.linger_deadline_us) == (1, 0, 0)
    r.receive([(0, 0x30, 0)], 9)                                                     # the peer's FIN
    assert r.fin_rcvd and r.check(10, ready) == (True, 0) and r.reason == lf.CLOSED and r.pending == lf.NONE
    r = _closed(closed=1, fin_rcvd=1)                                                # FIN and exit in one check
    assert r.check(1, ready) == (True, 0) and (r.reason, r.pending) == (lf.CLOSED, lf.FIN)


def test_closed_form_receive_ends_where_the_loop_returns():
    r = _closed()
    pk = [(0, 0x20, 1), (0, 0x30, 0), (0, 0x90, 0), (0, 0x20, 2), (0, 0x08, 0)]
    assert r.receive(pk, 5) == 2 and (r.reason, r.fin_rcvd, r.dropped, r.pending) == (lf.PEER_ACK_FIN, 1, 3, 0)
    assert r.receive(pk, 6) == 0 and r.dropped == 8 and r.last_activity_us == 5
    r = _closed()
    assert r.receive([(0, 0x08, 0)], 5) == 0 and (r.reason, r.fin_rcvd, r.origin_ack_us) == (lf.PEER_RST, 0, 0)
    for status in (1, 2, 3, 4, 5):
        r = _closed()
        assert r.receive([(status, 0x30, 9), (0, 0x20, 1)], 5) == 0
        assert (r.reason, r.pending, r.fin_rcvd, r.origin_ack_us, r.last_activity_us) == (lf.BAD_PACKET, lf.RST, 0, 0,
                                                                                         5)
    r = _closed()
    assert r.receive([(6, 0x28, 1), (6, 0x08, 0)], 5) == 1 and r.reason == lf.PEER_RST   # CAPACITY decoded
    r = _closed()
    assert r.receive([(7, 0x08, 1)], 5) == 1 and not r.exited                            # not a decode status


def test_closed_form_close_linger_and_abort():
    r = _closed()
    r.close(lf.HOW_CLOSE, 7, 100)
    assert (r.closed, r.linger_deadline_us) == (1, 107)
    r.close(lf.HOW_CLOSE, 9, 200)                                                    # closing a closed member
    assert r.linger_deadline_us == 107
    assert r.check(106, dict(lf.NB_IDLE, tracked=1)) == (False, 1)
    assert r.check(107, dict(lf.NB_IDLE, tracked=1)) == (True, 0) and r.reason == lf.LINGER
    r = _closed()
    r.close(lf.HOW_CLOSE, 0, 100)                                                    # linger < 0: no deadline
    assert (r.closed, r.linger_deadline_us) == (1, 0)
    r = _closed()
    r.close(lf.HOW_ABORT | lf.HOW_CLOSE | lf.HOW_NODELAY_ON, 5, 100)
    assert (r.exited, r.reason, r.pending, r.closed, r.ack_no_delay) == (1, lf.ABORT, lf.RST, 0, 1)
    r.close(lf.HOW_NODELAY_OFF, 0, 101)                                              # inert
    assert r.ack_no_delay == 1
    r = _closed()
    r.close(lf.HOW_NODELAY_ON | lf.HOW_NODELAY_OFF, 0, 1)
    assert r.ack_no_delay == 0


def test_closed_form_the_deadline_and_the_rto_it_shares():
    assert [lf.rto_us(0, k) for k in (0, 1, 6, 7, 16, 40)] == [500_000, 1_000_000, 32_000_000, 60_000_000, 60_000_000,
                                                              60_000_000]
    assert lf.rto_us(100, 0) == 200_000 and lf.rto_us(10 ** 9, 0) == 60_000_000 and lf.rto_us(300_000, 2) == 1_200_000
    r = _closed(1000)
    nb = dict(lf.NB_IDLE, last_sent_us=2000, rto_count=1)
    assert r.sent(False, 0, 2500, nb) == 2000 + 1_000_000
    assert r.sent(False, 0, 2000 + 1_000_000, nb) == 1000 + 300_000_000              # an RTO time not after now
    r.origin_ack_us = 1500
    assert r.sent(False, 0, 2500, nb) == 6500
    r.linger_deadline_us = 6000
    assert r.sent(False, 0, 2500, nb) == 6000
    rules = [r, _closed(exited=1, reason=lf.IDLE), _closed(exited=1, reason=lf.ABORT, reported=1), _closed(7)]
    out = lf.sent_set(rules, [nb] * 4, [0, 0, 0, 1], [0] * 4, None, 2500, 0)
    assert out == (6000, [], [], 1, [0, lf.NO_CONN, lf.NO_CONN, 1], 2)
    out = lf.sent_set(rules, [nb] * 4, [0] * 4, [0] * 4, None, 2500, 4)
    assert out[1:4] == ([1], [lf.IDLE], 1) and rules[1].reported == 1
    assert lf.sent_set([_closed(exited=1)], [nb], [0], [0], None, 1, 0)[0] == lf.NEVER


# ================================================================ CPU: the rule against the restatement
PLOTS = ("transfer", "close_both", "peer_rst", "ackfin", "corrupt", "silence", "failures", "linger", "abort",
         "sent_err", "ack_err", "stream_err")
PARAMS = dict(ack_delay_us=5000, idle_us=3_000_000, max_retries=10)


class _Peer:
    """The other end, scripted: what it has of the subject's packets (a fixed
    share is lost on the way, by packet number) and the SACK it would send."""

    def __init__(self, seed, loss):
        self.seed, self.loss, self.got, self.next_pn = seed, loss, set(), 1

    def hears(self, packets):
        for pn, _, _, _ in packets:
            if pn and random.Random(self.seed * 100003 + pn).random() >= self.loss:
                self.got.add(pn)

    def sack(self):
        if not self.got:
            return None
        lio = 0
        while lio + 1 in self.got:
            lio += 1
        runs = []
        for n in sorted((x for x in self.got if x > lio), reverse=True):
            if runs and runs[-1][0] == n + 1:
                runs[-1][0] = n
            else:
                runs.append([n, n])
        rows = [tuple(r) for r in runs] + [(lio, lio)] if runs else []
        return sr.Ack(max(self.got), lio, rows)


def _life(seed, params=PARAMS):
    """One connection's life under both statements, each beside its own
    neighbours: GoConn with sent_ref.GoSender, ack_ref.GoReceiver and
    stream_tx_ref.GoSender, RuleConn with RuleSent, RuleAck and RuleTx.  What
    the loops read of tracked, rq_len, tail / write_pos, err, rto_count and
    last_sent_us is what those hold.  Returns (states compared, [(step,
    letter)] of the states excluded, the reason it ended with)."""
    rng = random.Random(seed)
    plot = PLOTS[seed % len(PLOTS)]
    if plot == "failures":                                   # eleven backed-off RTOs take 303.5 s: longer than idle
        params = dict(params, idle_us=10 ** 9)
    now = 1000
    rule, go = lf.RuleConn(now, **params), lf.GoConn(now, **params)
    peer = _Peer(seed, rng.choice([0.0, 0.05, 0.2]))
    compared, excluded = 0, []
    deadline = rule.loop.sent(False, 0, now, rule.nb())
    for step in range(60):
        was_exited = rule.loop.exited
        kinds = ["write", "ack", "data", "data", "ack", "rto", "nodelay"]
        if step > 4:
            kinds += {"transfer": [], "close_both": ["close", "peer_fin"], "peer_rst": ["peer_rst"],
                      "ackfin": ["close", "ackfin"], "corrupt": ["corrupt"], "silence": ["silence"] * 6,
                      "failures": ["rto"] * 12, "linger": ["close_linger"] * 2, "abort": ["abort", "close"],
                      "sent_err": ["sent_err"], "ack_err": ["ack_err"], "stream_err": ["stream_err"]}[plot]
        kind = rng.choice(kinds)
        if was_exited:
            kind = "data"                                    # what arrives after the exit is dropped
        if plot == "failures" and step > 4 and rule.sent.tracked:
            kind = "rto"
        now += rng.choice([1, 100, 4999, 5000, 5001, 20_000])
        packets, how, linger = [], 0, 0
        if kind == "write":
            data = bytes(lf.SEGMENT * rng.randint(1, 4))
            go.Write(data), rule.write(data)
        elif kind == "ack" and peer.sack() is not None:
            packets = [(0, 0x80, 0, peer.sack(), 0, 0)]
        elif kind == "data":
            peer.next_pn += rng.choice([1, 1, 1, 2])         # now and then one of the peer's is lost
            packets = [(0, rng.choice([0x20, 0x20, 0xa0, 0x60]), peer.next_pn, None, 0, 0)]   # one: deviation (a)
        elif kind == "rto" and rule.sent.tracked:
            now = max(now, rule.sent.last_sent_us + lf.rto_us(0, rule.sent.rto_count))
        elif kind == "silence":
            now = max(now, deadline if deadline != lf.NEVER else now)
        elif kind == "nodelay":
            how = rng.choice([lf.HOW_NODELAY_ON, lf.HOW_NODELAY_OFF])
        elif kind in ("close", "close_linger"):
            how, linger = lf.HOW_CLOSE, 0 if kind == "close" else rng.choice([1, 30_000, 200_000])
        elif kind == "abort":
            how = lf.HOW_ABORT
        elif kind == "peer_fin":
            packets = [(0, 0x30, 0, None, 0, 0)]
        elif kind == "peer_rst":
            packets = [(0, 0x80, 0, None, 0, 0), (0, 0x08, 0, None, 0, 0), (0, 0x20, 6, None, 0, 0)]
        elif kind == "ackfin":
            packets = [(0, 0x90, 0, None, 0, 0), (0, 0x20, 6, None, 0, 0)]
        elif kind == "corrupt":
            packets = [(0, 0x80, 0, None, 0, 0), (rng.randint(1, 5), rng.randrange(256), rng.randrange(99), None, 0, 0)]
        elif kind == "sent_err":
            go.tooManyTracked, rule.sent_err = True, 1
        elif kind == "ack_err":                              # 1,001 numbers outstanding, in one batch
            packets = [(0, 0x20, peer.next_pn + 2 * k + 2, None, 0, 0) for k in range(1001)]
            peer.next_pn += 2004
        elif kind == "stream_err":
            peer.next_pn += 1
            packets = [(0, 0x20, peer.next_pn, None, 0, 1)]
        # ---- the application, both ways
        wire_before = len(go.wire)
        if how & (lf.HOW_NODELAY_ON | lf.HOW_NODELAY_OFF):
            go.SetACKNoDelay(how & lf.HOW_NODELAY_ON)
        if how & lf.HOW_ABORT and not go.loopExited:
            go.SetLinger(0), go.Close(now)
        elif how & lf.HOW_CLOSE and not go.loopExited:
            go.SetLinger(linger if linger > 0 else -1), go.Close(now)
        rule.loop.close(how, linger, now)
        # ---- the reference packet by packet and send loop by send loop; the rule one batch in THE ORDER
        queued = len(go.ss.retransmissionQueue) + len(go.ps.retransmissionQueue)
        handled_go = go.event(now, None, packets)
        handled = rule.batch(packets, now)
        deadline = rule.deadline
        peer.hears(rule.packets)
        # ---- compare
        compared += 1
        gv, rv = go.view(), rule.loop.view()
        diff = [k for k in gv if gv[k] != rv[k]]
        if handled_go != handled:
            diff.append("handled")
        if go.wire[wire_before:] != rule.emitted:
            diff.append("wire")
        if go.onlyAck is not None and not go.loopExited and not rule.loop.exited and int(go.onlyAck) != rule.may:
            diff.append("may_ack_only")
        go_deadline = min(go.resetTimer(now), go.lingerTimer or lf.NEVER) if not go.loopExited else lf.NEVER
        if go_deadline != deadline:
            diff.append("deadline")
        if sorted(p[0] for p in go.packets if p[0]) != sorted(p[0] for p in rule.packets if p[0]):
            diff.append("numbers sent")
        if diff:
            d, both = set(diff), {go.reason, rule.loop.reason}
            letter = None
            if (was_exited or any(lf.end_kind(p[0], p[1]) for p in packets)) and \
                    d <= {"wire", "fin_sent", "origin_ack_us", "deadline", "linger_deadline_us", "numbers sent"}:
                letter = "l"                                 # the send loop behind the packet that ended the loop
            elif len(packets) > 1 and both <= {lf.ACK_ERR, lf.STREAM_ERR} and d <= {"handled", "origin_ack_us",
                                                                                    "fin_rcvd"}:
                letter = "m"                                 # a neighbour's error is found behind the batch
            elif len(packets) > 1 and d <= {"origin_ack_us", "deadline", "may_ack_only", "numbers sent"}:
                letter = "a"                                 # one send loop per batch, not one per packet
            elif both == {lf.IDLE} and d <= {"wire", "fin_sent", "origin_ack_us", "linger_deadline_us",
                                             "numbers sent"}:
                letter = "b"                                 # the idle test before the send loop: nothing leaves first
            elif both == {lf.LINGER} and d <= {"exit_us", "linger_deadline_us", "handled", "origin_ack_us",
                                               "last_activity_us", "fin_rcvd"}:
                letter = "e"                                 # the linger timer is judged at check, behind the batch
            elif both <= {lf.FAILURES, lf.SENT_ERR} and d <= {"origin_ack_us", "numbers sent"}:
                letter = "c"                                 # the exit takes this batch's budget
            elif rule.loop.closed and queued and d <= {"wire", "fin_sent", "linger_deadline_us", "deadline"}:
                letter = "d"                                 # FIN waits for the retransmission queue
            assert letter, (seed, plot, step, kind, diff, gv, rv, go.wire, go.packets, rule.packets)
            excluded.append((step, letter, bool(go.loopExited or rule.loop.exited)))
            break                                            # the two have parted: the life ends here
        if was_exited:
            break
    return compared, excluded, rule.loop.reason


def test_families_of_whole_lives_equal_the_reference():
    """360 seeded lives: write, exchange with 0-20 % loss, an RTO now and then,
    Close from either side or both, linger 0 / > 0 / < 0, a peer RST, an
    ACK|FIN, a corrupt packet, silence until idle, eleven RTOs in a row.  After
    every call the rule and the restatement agree on every state field, the
    packets handled, the FIN / RST emitted, may_ack_only and the deadline.
    Two conditions: the families reach every reason 1-11, and at most 2 % of the
    compared states are excluded for meeting a deviation, each one attributed
    to its letter in include/ugo_loop.h."""
    compared, excluded, reasons = 0, [], set()
    for seed in range(360):
        n, ex, reason = _life(seed)
        compared += n
        excluded += [(seed,) + e for e in ex]
        reasons.add(reason)
    print(f"lives 360, states compared {compared}, excluded {len(excluded)}: "
          f"{sorted((l, sum(1 for e in excluded if e[2] == l)) for l in {e[2] for e in excluded})}")
    assert reasons >= set(range(1, 12)), sorted(reasons)
    assert len(excluded) <= 0.02 * compared, (len(excluded), compared, excluded[:10])
    # A life ends at the state it is excluded for.  That hides no later state where the member exits in that
    # very step (nothing but the drop of late packets follows an exit); a life that parts while both are live
    # does hide the rest of it, so those are capped as well: 2 % of the lives.
    midlife = [e for e in excluded if not e[3]]
    assert len(midlife) <= 0.02 * 360, midlife
    assert {e[2] for e in excluded} <= set("abcdelm")


# ================================================================ CPU: one directed test per deviation
def _env(**kw):
    return dict(dict(unsent=0, tracked=0, sent_err=0, rto_count=0, rto_fires=False, n_data=0, last_sent_us=0,
                     delay_us=0), **kw)


def test_deviation_a_one_clock_and_one_send_loop_per_batch():
    go, rule = lf.GoLoop(0), lf.RuleLoop(0)
    first = [(0, 0x20, 1, 0, 0)]
    go.event(1, _env(), first), rule.receive([p[:3] for p in first], 1)
    assert rule.check(1, lf.NB_IDLE) == (False, 0) and go.originAckTime == rule.origin_ack_us == 1
    pk = [(0, 0x20, 2, 0, 0), (0, 0x20, 3, 0, 0)]
    assert go.event(6002, _env(), pk) == 2
    assert go.originAckTime == 6002 and go.ackPending   # the ACK left behind packet 2; packet 3 started the delay again
    assert rule.receive([p[:3] for p in pk], 6002) == 2 and rule.check(6002, lf.NB_IDLE) == (False, 1)
    rule.sent(True, 0, 6002, lf.NB_IDLE)                # one send loop behind the batch: the ACK covers both
    assert rule.origin_ack_us == 0


def test_deviation_b_the_idle_test_runs_before_the_send_loop():
    go, rule = lf.GoLoop(0, idle_us=1000), lf.RuleLoop(0, idle_us=1000)
    go.event(1000, _env(unsent=500, n_data=1))
    assert go.sentAny and (go.reason, go.wire) == (lf.IDLE, ["RST"])      # the data left first
    assert rule.check(1000, dict(lf.NB_IDLE, tail=500)) == (True, 0) and rule.reason == lf.IDLE


def test_deviation_c_an_exit_found_by_check_takes_the_budget_of_this_batch():
    go, rule = lf.GoLoop(0), lf.RuleLoop(0)
    go.event(50, _env(tracked=3, rto_count=10, rto_fires=True, n_data=1))
    assert go.sentAny and (go.reason, go.wire) == (lf.FAILURES, ["RST"])  # the retransmission left first
    assert rule.check(50, dict(lf.NB_IDLE, tracked=2, rq_len=1, rto_count=11)) == (True, 0)
    assert (rule.reason, rule.pending) == (lf.FAILURES, lf.RST)


def test_deviation_d_fin_waits_for_the_retransmission_queue():
    go, rule = lf.GoLoop(0), lf.RuleLoop(0)
    go.Close(10), rule.close(lf.HOW_CLOSE, 0, 10)
    go.event(20, _env(tracked=0, n_data=1))     # dequeued: the history is empty, its segment waits to be popped
    assert go.wire == ["FIN"]                   # in front of the segment
    assert rule.check(20, dict(lf.NB_IDLE, rq_len=1)) == (False, 1) and rule.pending == lf.NONE
    assert rule.check(30, lf.NB_IDLE) == (True, 1) and rule.pending == lf.FIN


def test_deviation_e_the_linger_timer_is_a_deadline_judged_at_check():
    go, rule = lf.GoLoop(0), lf.RuleLoop(0)
    go.SetLinger(500), go.Close(10), rule.close(lf.HOW_CLOSE, 500, 10)
    assert go.lingerTimer == rule.linger_deadline_us == 510
    go.event(700, _env(tracked=1)), rule.check(700, dict(lf.NB_IDLE, tracked=1))
    assert go.reason == rule.reason == lf.LINGER and go.wire == ["RST"] and rule.pending == lf.RST
    assert (go.exitTime, rule.exit_us) == (510, 700)


def test_deviation_j_close_and_abort_change_nothing_on_a_closed_member():
    go, rule = lf.GoLoop(0), lf.RuleLoop(0)
    go.SetLinger(500), go.Close(10), rule.close(lf.HOW_CLOSE, 500, 10)
    go.SetLinger(0)
    assert go.Close(20) == "close closed connection" and not go.loopExited and go.wire == []
    rule.close(lf.HOW_ABORT, 0, 20)
    assert not rule.exited and rule.pending == lf.NONE and rule.linger_deadline_us == 510
    rule.close(lf.HOW_CLOSE | lf.HOW_NODELAY_ON, 900, 30)
    assert rule.linger_deadline_us == 510 and rule.ack_no_delay == 1        # the option still applies


def test_deviation_m_a_neighbours_error_is_found_behind_the_batch():
    go, rule = lf.GoConn(0), lf.RuleConn(0)
    pk = [(0, 0x20, 1, None, 0, 1), (0, 0x30, 2, None, 0, 0)]               # handleSegment fails on the first
    assert go.event(10, None, pk) == 1 and (go.reason, go.finRcvd, go.wire) == (lf.STREAM_ERR, False, ["RST"])
    assert rule.batch(pk, 10) == 2 and (rule.loop.reason, rule.loop.fin_rcvd, rule.emitted) == (lf.STREAM_ERR, 1,
                                                                                                 ["RST"])


def test_deviation_n_the_error_tests_come_before_the_fin_test():
    go, rule = lf.GoConn(0), lf.RuleConn(0)
    fin = [(0, 0x30, 0, None, 0, 0)]
    go.event(5, None, fin), rule.batch(fin, 5)
    go.Close(10), rule.loop.close(lf.HOW_CLOSE, 0, 10)
    go.tooManyTracked, rule.sent_err = True, 1
    go.event(20, None), rule.batch([], 20)
    assert (go.reason, go.wire) == (lf.CLOSED, ["FIN"])                     # FIN and exitLoop before CheckForError
    assert (rule.loop.reason, rule.emitted) == (lf.SENT_ERR, ["RST"])


def test_deviation_h_an_rst_that_never_fits_stays_pending():
    rule = lf.RuleLoop(0)
    rule.close(lf.HOW_ABORT, 0, 5)
    for _ in range(3):
        assert lf.append_set([rule], [lf.NB_IDLE], 8, 8) == ([], [0], 8) and rule.pending == lf.RST
    assert lf.sent_set([rule], [lf.NB_IDLE], [0], [0], None, 9, 4)[1:4] == ([0], [lf.ABORT], 1)
    assert rule.reported and rule.pending == lf.RST
    assert lf.append_set([rule], [lf.NB_IDLE], 7, 8) == ([(7, 0, lf.RST, 0, 0)], [2], 8) and rule.pending == lf.NONE


# ================================================================ GPU
import torch  # noqa: E402

import listen_ref as lr  # noqa: E402
from listen_harness import _put  # noqa: E402
from loop_harness import NO_CONN, LoopHarness, make_info  # noqa: E402

KEY = b"\x0f\x1e\x2d\x3c\x4b\x5a\x69\x78"
DATA, ACKFIN, RSTF = 0x20, 0x90, 0x08


@pytest.fixture(scope="module")
def enc(gpu):
    return fec.New(10, 3)


def _batch(n, conn, ends=()):
    """n data packets of member conn (a number, or an array); ends: [(index, status, flags)]."""
    status, flags, pn = np.zeros(n, np.uint32), np.full(n, DATA, np.uint8), np.arange(1, n + 1, dtype=np.uint64)
    for i, st, fl in ends:
        status[i], flags[i] = st, fl
    conn_of = np.full(n, conn, np.uint32) if np.isscalar(conn) else np.asarray(conn, np.uint32)
    return status, flags, pn, conn_of


@pytest.mark.gpu
def test_receive_tie_breaks_the_lowest_ending_packet_wins(enc):
    h = LoopHarness(enc, 5, now_us=10)
    # two ending packets of one member in one wave, in two waves of a block, in two blocks
    for k, (a, b) in enumerate(((40, 9), (200, 70), (3000, 700))):
        st, fl, pn, conn = _batch(4096, k, [(a, 0, RSTF), (b, 0, ACKFIN)])
        got = h.receive(st, fl, pn, conn, 100 + k)
        assert (got[:b] == k).all() and (got[b:] == NO_CONN).all()
        assert (h.rules[k].reason, h.rules[k].dropped) == (lf.PEER_ACK_FIN, 4096 - b)
    # the ending packet at index 0 and at the last index; entries >= nconn and NO_CONN are untouched
    st, fl, pn, conn = _batch(1000, 3, [(0, 3, DATA)])
    conn[5], conn[6], conn[7] = NO_CONN, 5, 0x7fffffff
    conn[999] = 4
    st[999], fl[999] = 0, RSTF
    got = h.receive(st, fl, pn, conn, 200)
    assert got[5] == NO_CONN and got[6] == 5 and got[7] == 0x7fffffff and (got[[0, 1, 998, 999]] == NO_CONN).all()
    assert (h.rules[3].reason, h.rules[3].pending, h.rules[4].reason) == (lf.BAD_PACKET, lf.RST, lf.PEER_RST)
    # every member has exited: the whole batch is dropped, an ending packet changes nothing
    st, fl, pn, conn = _batch(300, np.arange(300) % 5, [(17, 0, ACKFIN)])
    assert (h.receive(st, fl, pn, conn, 300) == NO_CONN).all()
    h.close()


@pytest.mark.gpu
def test_receive_a_thousand_ending_packets_among_a_hundred_thousand_of_one_member(enc):
    h = LoopHarness(enc, 2, now_us=10)
    rng = np.random.default_rng(11)
    n = 100_000
    ends = np.sort(rng.choice(np.arange(50_000, n), 1000, replace=False))
    st, fl, pn, conn = _batch(n, 1)
    fl[ends] = rng.choice([RSTF, ACKFIN], 1000)
    st[ends[::7]] = 2
    got = h.receive(st, fl, pn, conn, 50)
    assert (got[:ends[0]] == 1).all() and (got[ends[0]:] == NO_CONN).all() and h.rules[1].dropped == n - ends[0]
    # the scratch words are idle again: a second call with no ending packet masks nothing
    st, fl, pn, conn = _batch(n, 0)
    assert (h.receive(st, fl, pn, conn, 60) == 0).all()
    assert not h.rules[0].exited and h.rules[0].origin_ack_us == 60
    h.close()


def _inject_members(nconn):
    if nconn < 16:                                                        # the errors share members 0 and 1
        return dict(sent_err=0, ack_err=1, stream_err=1, failures=2, tracked=2, unsent=2)
    return {k: 3 + 5 * j for j, k in enumerate(("sent_err", "ack_err", "stream_err", "failures", "tracked", "unsent"))}


def _inject(h, nconn, base=0):
    """Errors and progress in the neighbouring sets, through their own calls.
    Returns the members touched, by what.  The eleven RTOs take 671 s, which
    do not fit between the highest base and 2^64: above base 0 the neighbours'
    clocks start 700 s below base and so end below it."""
    m = _inject_members(nconn)
    at = base - 700_000_000 if base else 0
    h.sent_record([(m["sent_err"], 1), (m["tracked"], 20)] + [(m["failures"], k) for k in range(1, 14)], at + 1000)
    h.sent_record([(m["sent_err"], 5000)], at + 1001)                     # past the window: TOO_MANY_TRACKED
    now = at + 1000
    for _ in range(11):                                                   # eleven RTOs in a row
        now += 61_000_000
        h.sent_rto(now)
    h.ack_receive([(m["ack_err"], 2 * k + 2) for k in range(1001)], at + 5)    # 1,001 outstanding
    h.stream_deliver([(m["stream_err"], 10, 10)])
    h.stream_deliver([(m["stream_err"], 5, 10)])                          # overlaps
    counts = [0] * nconn
    counts[m["unsent"]] = 100
    h.tx_write(counts)
    nb = h.nbs()
    assert nb[m["sent_err"]]["sent_err"] and nb[m["ack_err"]]["ack_err"] and nb[m["stream_err"]]["stream_err"]
    assert nb[m["failures"]]["rto_count"] == 11 and nb[m["tracked"]]["tracked"] >= 1
    assert nb[m["unsent"]]["tail"] == 100 and nb[m["unsent"]]["write_pos"] == 0
    return m


class _DryLoop:
    """Takes the calls of _every_mode and does nothing: what the script draws
    does not depend on what the device answers, so its clocks can be had
    without one."""
    rules = ()

    def __getattr__(self, name):
        return lambda *a, **k: (0, [], [], 0, [], 0)


EVERY_MODE_IDLE = 40_000


def _every_mode(h, nconn, base, who):
    """The body of test_the_loop_equals_the_rule_in_every_mode_at_once, every
    clock above base.  Returns the clocks of the loop calls."""
    rng = np.random.default_rng(nconn)
    idle = EVERY_MODE_IDLE
    now = base + 1000
    seen = set()
    clocks = []
    for rnd in range(6):
        now += int(rng.choice([0, 1, 4999, 5000, 5001, 7000, idle - 5001]))
        clocks.append(now)
        npk = int(rng.integers(4096, 20001))
        conn = rng.integers(0, nconn, npk).astype(np.uint32)
        conn[rng.random(npk) < 0.02] = NO_CONN
        conn[rng.random(npk) < 0.01] = nconn + int(rng.integers(0, 1000))
        if nconn > 100:                                                   # some members hear nothing: they go idle
            conn[conn % 11 == 3] = NO_CONN
        flags = rng.choice([DATA, 0x80, 0xa0, 0x60, 0x30, 0x10], npk, p=[.6, .2, .1, .05, .03, .02]).astype(np.uint8)
        status = np.where(rng.random(npk) < 0.05, 6, 0).astype(np.uint32)
        pn = np.where(flags == 0x80, 0, rng.integers(1, 1 << 40, npk)).astype(np.uint64)
        n_end = max(2, nconn // 100)                                      # about 1 % of the members end per call
        at = rng.choice(npk, 3 * n_end, replace=False)
        flags[at[:n_end]], flags[at[n_end:2 * n_end]] = ACKFIN, RSTF
        status[at[2 * n_end:]] = rng.integers(1, 6, n_end)
        h.receive(status, flags, pn, conn, now)
        how = rng.choice([0, 1, 2, 4, 8, 5, 3], nconn, p=[.9, .05, .01, .01, .01, .01, .01]).astype(np.uint8)
        linger = rng.choice([0, 1, 5000, 5001, idle], nconn)
        if rnd == 1:                                                      # two that cannot send their FIN linger
            how[[who["tracked"], who["unsent"]]], linger[[who["tracked"], who["unsent"]]] = 1, (1, 5001)
        h.close_members(how, now, None if rnd == 0 else linger)
        now += int(rng.choice([0, 1, 5000, 5001]))
        clocks.append(now)
        budget = rng.integers(0, 9, nconn)
        h.check_call(now, budget)
        total = int(rng.integers(0, 50))
        pending = sum(1 for r in h.rules if r.pending)
        room = int(rng.choice([pending, max(pending - 1, 0), pending + 3, 0]))
        h.append(total, total + room, max_segments=int(rng.integers(1, 4)), alias=bool(rnd % 2))
        delay = rng.choice([0, 100, 300_000, 10 ** 9], nconn)
        out = h.sent(rng.integers(0, 2, nconn), rng.integers(0, 2, nconn), now, None if rnd == 2 else delay,
                     max_exits=int(rng.choice([0, 1, 7, nconn])), remap=rnd != 3)
        seen |= set(out[2])
    return clocks


def _loop_in_every_mode(enc, nconn, base):
    h = LoopHarness(enc, nconn, now_us=base + 1000, idle_us=EVERY_MODE_IDLE, ack_delay_us=5000)
    who = _inject(h, nconn, base)
    clocks = _every_mode(h, nconn, base, who)
    reasons = {r.reason for r in h.rules}
    if nconn >= 1025:
        assert reasons >= set(range(1, 12)), sorted(reasons)
        assert {who[k] for k in who} and all(h.rules[who[k]].exited for k in ("sent_err", "ack_err", "stream_err",
                                                                             "failures"))
        assert any(r.fin_sent for r in h.rules) and any(r.dropped for r in h.rules)
    rules = h.rules
    h.close()
    return clocks, rules


@pytest.mark.gpu
@pytest.mark.parametrize("nconn", [3, 1025, 32769])
def test_the_loop_equals_the_rule_in_every_mode_at_once(enc, nconn):
    """Six batches through receive, close, check, append and sent.  Every member
    draws its own packets, closes and clocks, so the lanes of one wave are live,
    closing, lingering, failing and exited at once; the clocks step by the
    boundaries of the delayed ACK, the linger and the idle tests."""
    _loop_in_every_mode(enc, nconn, 0)


# Real clocks.  T1 is placed by the script's own clocks (had without a device) so that the fourth batch is the
# first at or past 2^32 us; T2 is a wall clock in us; T4 ends 10^8 us short of 2^64.
_DRY_CLOCKS = _every_mode(_DryLoop(), 1025, 0, _inject_members(1025))
T1 = (1 << 32) - _DRY_CLOCKS[6]
T2, T4 = 1_760_000_000_000_000, (1 << 64) - 10 ** 8
BASE_IDS = {T1: "T1", T2: "T2", T4: "T4"}


def test_the_clocks_of_the_every_mode_script_cross_2_32_in_mid_run():
    clocks = _every_mode(_DryLoop(), 1025, T1, _inject_members(1025))
    print("loop clocks from T1, less 2^32:", [t - (1 << 32) for t in clocks])
    assert len(clocks) == 12 and clocks == sorted(clocks)
    assert clocks[0] < clocks[5] < 1 << 32 == clocks[6] and clocks[-1] > clocks[6]


@pytest.mark.gpu
@pytest.mark.parametrize("base", [T1, T2, T4], ids=BASE_IDS.get)
def test_the_loop_equals_the_rule_in_every_mode_at_once_at_real_clocks(enc, base):
    clocks, rules = _loop_in_every_mode(enc, 1025, base)
    assert base < clocks[0] and clocks[-1] < 1 << 64 and clocks == [base + t for t in _DRY_CLOCKS]
    assert all(r.exited or r.origin_ack_us == 0 or r.origin_ack_us > base for r in rules)


def _pad(slot):
    return np.frombuffer(fec.rc4_keystream(KEY, slot), np.uint8)[:slot].copy()


@pytest.mark.gpu
def test_append_interleaves_fins_and_rsts_and_clamps_at_max_packets(enc):
    h = LoopHarness(enc, 6, now_us=0)
    counts = [0, 300, 0, 0, 50, 0]
    h.tx_write(counts)
    budget = torch.tensor([0, 4, 0, 0, 0, 0], dtype=torch.int32, device="cuda")
    h.tx_set.plan(budget, 8)                                              # member 1 packetises its 300 bytes
    h._nbs = None
    assert h.nbs()[1]["write_pos"] == 300 and h.nbs()[4]["tail"] == 50
    h.close_members([1, 1, 2, 0, 1, 3], 10)
    zero, may = h.check_call(20, [5] * 6)
    assert zero == [0, 0, 0, 5, 5, 0] and may == [1, 1, 0, 1, 1, 0]
    assert [r.pending for r in h.rules] == [lf.FIN, lf.FIN, lf.RST, 0, 0, lf.RST]
    *_, appended, writes = h.append(2, 2, alias=False)                    # *total == max_packets: no target
    assert appended == [0] * 6 and writes == []
    *_, total, appended, writes = h.append(0, 3)                          # one short: member 5 stays pending
    assert appended == [1, 1, 2, 0, 0, 0] and total == 3 and h.rules[5].pending == lf.RST
    assert [(t, c, off) for t, c, _, off, _ in writes] == [(0, 0, 0), (1, 1, 300), (2, 2, 0)]
    *_, total, appended, writes = h.append(1, 2, max_segments=1)          # exactly fits
    assert appended == [0, 0, 0, 0, 0, 2] and total == 2
    *_, total, appended, writes = h.append(1 << 40, 8, alias=False)  # a *total past every target
    assert appended == [0] * 6 and total == 1 << 40
    h.close()


@pytest.mark.gpu
def test_appended_records_encode_as_the_references_fin_and_rst(enc):
    slot = 64
    pad = _pad(slot)
    h = LoopHarness(enc, 4, now_us=0)
    h.tx_write([0, 5000 - 904, 0, 200])                                   # the window holds 4,096: 4,096 written
    budget = torch.tensor([0, 8, 0, 1], dtype=torch.int32, device="cuda")
    h.tx_set.plan(budget, 16)
    h._nbs = None
    offs = [h.nbs()[c]["write_pos"] for c in range(4)]
    assert offs == [0, 4096, 0, 200]
    h.close_members([1, 1, 2, 1], 10)
    h.check_call(20, [0] * 4)
    info, segs, conn, total, appended, _ = h.append(0, 8, max_segments=2)
    assert total == 4 and appended == [1, 1, 2, 1]
    ranges = torch.zeros((8, 1, 2), dtype=torch.int64, device="cuda")
    wire, lens, status = h.tx_set.encode(_put(info), ranges, _put(segs), _put(conn.view(np.int32)), slot,
                                         npackets=total, pad=_put(pad))
    assert status.cpu().numpy().tolist() == [0] * 4
    wire, lens = wire.cpu().numpy(), lens.cpu().numpy()
    for t, off in ((0, 0), (1, 4096), (3, 200)):
        want = pr.encode(flags=0x10, packet_number=0, segments=[(off, b"")])      # sendFin
        assert want[0] == 0x30
        assert lens[t] == len(want) and bytes(wire[t, :lens[t]] ^ pad[:lens[t]]) == want, t
    want = pr.encode(flags=0x08, packet_number=0)                                 # sendRst
    assert lens[2] == len(want) and bytes(wire[2, :lens[2]] ^ pad[:lens[2]]) == want
    h.close()


def _deadline_terms(enc, base):
    """Each term of the deadline the minimum in turn, every clock above base.
    Returns the deadlines less base, in the order asked, and the last output."""
    idle = 10 ** 9
    h = LoopHarness(enc, 4, now_us=base + 1000, idle_us=idle)
    none = [0] * 4
    got = [h.sent(none, none, base + 1000)[0]]                            # the idle term
    st, fl, pn, conn = _batch(1, 1)
    h.receive(st, fl, pn, conn, base + 2000)
    got.append(h.sent(none, none, base + 2000)[0])                        # the delayed ACK
    h.sent_record([(2, 1), (3, 1)], base + 1)                             # last_sent_us = 1: an RTO at 500,001
    h.close_members([0, 0, 1, 0], base + 2500, [0, 0, 3000, 0])
    got.append(h.sent(none, none, base + 2500)[0])                        # the linger deadline
    got.append(h.sent([0, 1, 0, 0], none, base + 2600)[0])
    assert h.rules[1].origin_ack_us == 0
    h.check_call(base + 5500, none)
    assert h.rules[2].reason == lf.LINGER
    got.append(h.sent(none, none, base + 5500)[0])                        # the RTO, default delay
    got.append(h.sent(none, none, base + 5500, delay_us=[0, 0, 0, 300_000])[0])
    got.append(h.sent(none, none, base + 300_001, delay_us=[0, 0, 0, 300_000])[0])            # not after now
    h.close_members([2] * 4, base + 6000)
    out = h.sent(none, none, base + 6000, remap=True)
    h.close()
    return [lf.NEVER if t == lf.NEVER else t - base for t in got], out


@pytest.mark.gpu
def test_sent_deadline_each_term_the_minimum_in_turn(enc):
    idle = 10 ** 9
    got, out = _deadline_terms(enc, 0)
    assert got == [1000 + idle, 2000 + 5000, 5500, 5500, 500_001, 300_001, min(1000, 2000) + idle]
    assert out[0] == lf.NEVER and out[4] == [NO_CONN] * 4 and out[5] == 0  # no live member


@pytest.mark.gpu
@pytest.mark.parametrize("base", [T1, T2, T4], ids=BASE_IDS.get)
def test_sent_deadline_each_term_the_minimum_in_turn_at_real_clocks(enc, base):
    """The harness holds every deadline to the rule's; what the rule gives is
    the same terms above base, but that at T4 the idle term, 10^9 us ahead,
    passes 2^64 and saturates to NEVER."""
    idle = 10 ** 9
    got, out = _deadline_terms(enc, base)
    far = lf.NEVER if base == T4 else None
    assert base + 1000 + idle >= 1 << 64 if base == T4 else base + 2000 + idle < 1 << 64
    assert got == [far or 1000 + idle, 2000 + 5000, 5500, 5500, 500_001, 300_001, far or min(1000, 2000) + idle]
    assert out[0] == lf.NEVER and out[4] == [NO_CONN] * 4 and out[5] == 0


@pytest.mark.gpu
def test_sent_lists_exits_across_max_exits_and_feeds_listen_remap(enc):
    n = 10
    h = LoopHarness(enc, n, now_us=0)
    table = fec.ListenTable(enc, 16)
    names = np.stack([np.frombuffer(lr.name_v4(bytes([10, 0, 0, k]), 4000 + k), np.uint8) for k in range(n)])
    pkts = np.zeros((n, 32), np.uint8)
    for k in range(n):
        pkts[k, :22] = np.frombuffer(lr.init_packet(k), np.uint8)
    table.route(_put(names), _put(pkts), _put(np.full(n, 22, np.int16)))
    assert int(table.state()["nconn"]) == n
    how = [0] * n
    for c in (1, 3, 4, 7, 9):
        how[c] = 2
    h.close_members(how, 5)
    none = [0] * n
    assert h.sent(none, none, 6, max_exits=0)[1:4] == ([], [], 5)
    assert h.sent(none, none, 7, max_exits=2)[1:4] == ([1, 3], [lf.ABORT] * 2, 5)     # fewer
    assert h.sent(none, none, 8, max_exits=3)[1:4] == ([4, 7, 9], [lf.ABORT] * 3, 3)  # exactly the remainder
    assert h.sent(none, none, 9, max_exits=8)[1:4] == ([], [], 0)                     # more
    # new_index and nconn_new as the device wrote them are the operands of ugo_fec_listen_remap
    zeros = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = h.loop.sent(zeros, zeros.to(torch.uint8), 10, remap=True)
    new_index, nconn_new = out[4], int(out[5].item())
    assert nconn_new == 5
    status = table.remap(new_index, nconn_new)
    assert int(status.item()) == 0
    ent = table.entries()
    assert ent["member"].tolist() == [0, 1, 2, 3, 4] and ent["port"].tolist() == [4000 + k for k in (0, 2, 5, 6, 8)]
    table.close()
    h.close()


@pytest.mark.gpu
def test_pinned_operands_and_kernel_class(enc):
    h = LoopHarness(enc, 3, now_us=0, where="pinned")
    enc.timing_begin(64)
    try:
        st, fl, pn, conn = _batch(100, np.arange(100) % 3, [(50, 0, RSTF)])
        h.receive(st, fl, pn, conn, 10)
        h.close_members([1, 0, 0], 20, [500, 0, 0])
        h.check_call(30, [3, 3, 3])
        h.append(0, 4)
        h.sent([1, 0, 0], [0, 0, 0], 40, delay_us=[0, 0, 0], max_exits=2)
    finally:
        recs, untimed = enc.timing_end()
    assert untimed == 0
    # receive 3 launches, close 1, check 1, append 2, sent 2 (the state gathers are not timed)
    assert recs["kernel"].tolist() == [16] * 9
    assert h.rules[2].reason == lf.PEER_RST and h.rules[0].fin_sent
    h.close()


@pytest.mark.gpu
def test_argument_errors_on_the_device(enc):
    lib = fec.load_library()
    bad = fec.ErrInvalidArg.code
    h = LoopHarness(enc, 2, now_us=0)
    out = ctypes.c_void_p(1)
    other = fec.New(4, 2)
    sets = (h.rx_set._h, h.ack_set._h, h.tx_set._h, h.sent_set._h)
    assert lib.ugo_fec_loop_set_create(other._h, *sets, None, 0, ctypes.byref(out)) == bad and out.value is None
    for k in range(4):                                                    # a NULL set
        a = list(sets)
        a[k] = None
        assert lib.ugo_fec_loop_set_create(enc._h, *a, None, 0, ctypes.byref(out)) == bad and out.value is None
    lone = fec.SentTx(enc, 1024, 1)
    one = fec.SentTxSet(enc, [lone])                                      # another nconn
    assert lib.ugo_fec_loop_set_create(enc._h, sets[0], sets[1], sets[2], one._h, None, 0, ctypes.byref(out)) == bad
    arr = np.array([(5000, 0, 10, 0)], fec.LOOP_PARAMS_DTYPE)             # idle_us == 0
    assert lib.ugo_fec_loop_set_create(enc._h, *sets, arr.ctypes.data, 0, ctypes.byref(out)) == bad
    assert out.value is None
    buf = {k: torch.full((n,), 0x11, dtype=torch.uint8, device="cuda")
           for k, n in (("info", 256), ("segs", 128), ("conn", 16), ("u64", 16), ("u8", 2), ("u32", 8))}
    p = {k: v.data_ptr() for k, v in buf.items()}
    host = torch.zeros(256, dtype=torch.uint8).data_ptr()                 # pageable
    L = h.loop._h
    rc = lambda **k: lib.ugo_fec_loop_set_receive(  # noqa: E731
        L, k.get("info", p["info"]), k.get("conn", p["conn"]), k.get("n", 4), 5, None)
    assert rc(info=None) == bad and rc(conn=None) == bad and rc(info=p["info"] + 8) == bad
    assert rc(conn=p["conn"] + 2) == bad and rc(n=(1 << 31) + 1) == bad and rc(info=host) == bad
    assert rc(conn=host) == bad and rc(n=0, info=None, conn=None) == 0
    cl = lambda **k: lib.ugo_fec_loop_set_close(L, k.get("how", p["u8"]), k.get("lg", p["u64"]), 5, None)  # noqa: E731
    assert cl(how=None) == bad and cl(lg=p["u64"] + 4) == bad and cl(how=host) == bad and cl(lg=host) == bad
    ck = lambda **k: lib.ugo_fec_loop_set_check(L, 5, k.get("b", p["u32"]), k.get("m", p["u8"]), None)  # noqa: E731
    assert ck(b=None) == bad and ck(m=None) == bad and ck(b=p["u32"] + 2) == bad and ck(b=host) == bad
    assert ck(m=host) == bad
    ap = lambda **k: lib.ugo_fec_loop_set_append(  # noqa: E731
        L, k.get("t", p["u64"]), k.get("mp", 2), k.get("info", p["info"]), k.get("segs", p["segs"]), k.get("ms", 2),
        k.get("conn", p["conn"]), k.get("to", p["u64"] + 8), k.get("a", p["u8"]), None)
    assert ap(t=None) == bad and ap(info=None) == bad and ap(segs=None) == bad and ap(conn=None) == bad
    assert ap(to=None) == bad and ap(a=None) == bad and ap(ms=0) == bad and ap(ms=0x10000) == bad
    assert ap(mp=(1 << 31) + 1) == bad and ap(t=p["u64"] + 4) == bad and ap(info=p["info"] + 8) == bad
    assert ap(segs=p["segs"] + 4) == bad and ap(to=p["u64"] + 12) == bad and ap(info=host) == bad
    assert ap(t=host) == bad and ap(a=host) == bad
    sn = lambda **k: lib.ugo_fec_loop_set_sent(  # noqa: E731
        L, k.get("np", p["u32"]), k.get("at", p["u8"]), k.get("d", p["u64"]), 5, k.get("dl", p["info"]),
        k.get("ex", p["conn"]), k.get("rs", p["segs"]), k.get("me", 2), k.get("ne", p["info"] + 8),
        k.get("ni", p["info"] + 16), k.get("nn", p["info"] + 24), None)
    assert sn(np=None) == bad and sn(at=None) == bad and sn(dl=None) == bad and sn(ne=None) == bad
    assert sn(ex=None) == bad and sn(rs=None) == bad and sn(ni=None) == bad and sn(nn=None) == bad
    assert sn(d=p["u64"] + 4) == bad and sn(dl=p["info"] + 4) == bad and sn(ne=p["info"] + 12) == bad
    assert sn(ex=p["conn"] + 2) == bad and sn(ni=p["info"] + 18) == bad and sn(nn=p["info"] + 28) == bad
    assert sn(np=host) == bad and sn(dl=host) == bad and sn(ex=host) == bad and sn(nn=host) == bad
    torch.cuda.synchronize()
    assert all(bool((t == 0x11).all()) for t in buf.values())
    h.check()
    # a loop set one of whose sets is gone refuses every call
    h.ack_set.close()
    assert ck() == bad and rc() == bad and cl() == bad and ap() == bad and sn() == bad
    one.close(), lone.close(), other.close()
    h.close()


# ---------------------------------------------------------------- two peers through the whole chain
SLOT, NP, MR, MS, PKT_BYTES = 1488, 32, 8, 2, 1470


class Endpoint:
    """One side of a link: a member per connection in each of the four sets,
    their controllers and the loop, run in THE ORDER of include/ugo_loop.h.  The
    host hands in now_us and reads sizes and the deadline; budget, delays,
    may_ack_only, attached and the exits pass from call to call on the device."""

    def __init__(self, enc, n, now, **loop_params):
        dev = torch.device("cuda")
        self.enc, self.n = enc, n
        self.pad = _put(_pad(SLOT))
        self.rx = [fec.StreamRx(enc, 65536) for _ in range(n)]
        self.ack = [fec.AckRx(enc, 4096) for _ in range(n)]
        self.tx = [fec.StreamTx(enc, 65536, 64) for _ in range(n)]
        self.sent = [fec.SentTx(enc, 1024, MS) for _ in range(n)]
        self.rset, self.aset = fec.StreamRxSet(enc, self.rx), fec.AckRxSet(enc, self.ack)
        self.tset, self.sset = fec.StreamTxSet(enc, self.tx), fec.SentTxSet(enc, self.sent)
        self.cc = fec.CcSet(enc, self.sset)
        self.loop = fec.LoopSet(enc, self.rset, self.aset, self.tset, self.sset, now_us=now, **loop_params)
        self.budget = self.cc.rto(torch.zeros(n, dtype=torch.uint8, device=dev), PKT_BYTES, 8)
        self.delays = torch.zeros(n, dtype=torch.int64, device=dev)
        self.split = self.cc.cutback()
        self.ranges = torch.zeros((NP, MR, 2), dtype=torch.int64, device=dev)
        self.plan = None
        self.want = torch.full((n,), 1 << 20, dtype=torch.int64, device=dev)
        self.dst = torch.zeros(n << 20, dtype=torch.uint8, device=dev)
        self.dst_off = torch.arange(n, dtype=torch.int64, device=dev) << 20
        self.got = [bytearray() for _ in range(n)]
        self.eof = [False] * n
        self.exits, self.deadline = {}, 0

    def close(self):
        for x in (self.loop, self.cc, self.rset, self.aset, self.tset, self.sset):
            x.close()
        for x in self.rx + self.ack + self.tx + self.sent:
            x.close()

    def write(self, chunks):
        src = torch.from_numpy(np.concatenate(chunks)).cuda()
        sizes = [len(c) for c in chunks]
        off = torch.tensor(np.cumsum([0] + sizes[:-1]), dtype=torch.int64, device="cuda")
        assert self.tset.write(src, off, torch.tensor(sizes, dtype=torch.int64, device="cuda")).tolist() == sizes

    def app_close(self, members, now, how=1):
        flags = torch.zeros(self.n, dtype=torch.uint8, device="cuda")
        flags[list(members)] = how
        self.loop.close_members(flags, now)

    def send(self, now):
        """Returns (wire, lens, conn_of, npackets, the planned records as numpy)."""
        may = self.loop.check(now, self.budget)
        self.plan = self.tset.plan(self.budget, NP, max_segments=MS, out=self.plan)
        info, segs, conn, first, count, total = self.plan
        self.loop.append(total, info, segs, conn)                         # total_out is total itself
        total_out, attached = self.aset.attach(now, first, count, total, info, self.ranges, conn, may_ack_only=may)
        self.sset.attach(first, count, info)
        npk = int(total_out.item())                                       # a size
        wire = lens = None
        if npk:
            wire, lens, st = self.tset.encode(info, self.ranges, segs, conn, SLOT, npackets=npk, pad=self.pad)
            assert not st[:npk].any(), st[:npk].tolist()
            self.sset.record(info, segs, conn, lens, st, now, npackets=npk)
        out = self.loop.sent(count, attached, now, delay_us=self.delays, max_exits=self.n)
        self.deadline = int(out[0].cpu().numpy().view(np.uint64)[0])      # the one deadline
        for k in range(min(int(out[3].item()), self.n)):                  # a size, then the list it counts
            self.exits[int(out[1][k])] = int(out[2][k])
        look = info[:npk].cpu().numpy().view(fec.PKT_INFO_DTYPE).reshape(-1)
        return wire, lens, conn[:npk].clone(), npk, look

    def receive(self, wire, lens, conn, npk, now):
        dev = torch.device("cuda")
        if npk:
            info, ranges, segs = self.enc.packet_decode(wire, lens, pad=self.pad, max_ranges=MR, max_segments=MS)
            self.loop.receive(info, conn, now)
            seg_status = self.rset.deliver(wire, info, segs, conn, pad=self.pad)
            self.aset.receive(info, conn, now, seg_status=seg_status)
            n_read, eof = self.rset.read(self.want, self.dst, self.dst_off)
            for c, k in enumerate(n_read.tolist()):                       # sizes
                self.got[c] += self.dst[(c << 20):(c << 20) + k].cpu().numpy().tobytes()
            self.eof = [a or bool(b) for a, b in zip(self.eof, eof.tolist())]
            events, rows = self.cc.sent_ack(info, ranges, conn, now, npackets=npk, split=self.split)
            self.delays = self.cc.ack(events, rows, now)
        fired = self.sset.rto(self.delays, now)
        self.budget = self.cc.rto(fired, PKT_BYTES, 8)
        rc, ro, rlen, n_entries, touch, upto = self.sset.drain(64)
        self.tset.retransmit(rc, ro, rlen)
        self.aset.touch(touch)
        self.tset.release(upto)
        return conn


def _link(wire, lens, conn, npk, look, counter):
    """The loss applies to the packets ARQ covers only: every twentieth packet
    with no FIN or RST bit is lost, 5 % of those, not 5 % of all wire packets.
    sendFin and sendRst send once and nothing retransmits them, so a lost FIN
    cannot end in reason CLOSED: it ends by the timers."""
    keep = []
    for i in range(npk):
        if look["flags"][i] & 0x18:
            keep.append(i)
            continue
        counter[0] += 1
        if counter[0] % 20 != 0:
            keep.append(i)
    idx = torch.tensor(keep, dtype=torch.int64, device="cuda")
    if not keep:
        return None, None, None, 0
    return wire[idx].contiguous(), lens[idx].contiguous(), conn[idx].contiguous(), len(keep)


@pytest.mark.gpu
def test_two_peers_write_close_read_to_eof_and_close(enc):
    """A writes and closes; B reads to eof and closes.  Both end with reason
    CLOSED, every byte is read, no FIN goes out before the last retransmitted
    segment, and what arrives after the exit is dropped."""
    rng = np.random.default_rng(9)
    sizes = [30_000, 20_011]
    data = [rng.integers(0, 256, k, dtype=np.uint8) for k in sizes]
    now = 1_000_000
    A, B = Endpoint(enc, 2, now), Endpoint(enc, 2, now)
    A.write(data)
    A.app_close([0, 1], now)
    to_b, to_a, fin_round, last_data_round, b_closed = [0], [7], {}, {}, set()
    rounds = 0
    while len(A.exits) < 2 or len(B.exits) < 2:
        rounds += 1
        assert rounds <= 300, (A.exits, B.exits, [len(g) for g in B.got], A.loop.states(), B.loop.states())
        now += 20_000
        wire, lens, conn, npk, look = A.send(now)
        cl = conn.cpu().numpy().view(np.uint32)
        for i in range(npk):
            c = int(cl[i])
            if look["flags"][i] == 0x10:
                fin_round.setdefault(c, rounds)
            elif look["n_segments"][i] and look["packet_number"][i]:
                last_data_round[c] = rounds
        B.receive(*_link(wire, lens, conn, npk, look, to_b), now + 1000)
        ready = [c for c in range(2) if B.eof[c] and c not in b_closed]
        if ready:
            B.app_close(ready, now + 1500)
            b_closed |= set(ready)
        wire, lens, conn, npk, look = B.send(now + 2000)
        A.receive(*_link(wire, lens, conn, npk, look, to_a), now + 3000)
    assert A.exits == {0: lf.CLOSED, 1: lf.CLOSED} and B.exits == {0: lf.CLOSED, 1: lf.CLOSED}
    for c in range(2):
        assert bytes(B.got[c]) == data[c].tobytes(), c
        assert fin_round[c] > last_data_round[c], (c, fin_round, last_data_round)
    assert int(A.sset.states()["lost_packets"].sum()) > 0                 # the link did lose packets
    sa, sb = A.loop.states(), B.loop.states()
    assert sa["fin_sent"].all() and sa["fin_rcvd"].all() and sb["fin_sent"].all() and sb["fin_rcvd"].all()
    # a batch that arrives after the exit
    late = _put(make_info([0, 0, 0], [0x20, 0x30, 0x80], [9, 0, 0], 1))[:3]
    conn = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    assert A.loop.receive(late, conn, now + 5000).cpu().numpy().view(np.uint32).tolist() == [NO_CONN] * 3
    assert A.loop.states()["dropped"].tolist() == [int(sa["dropped"][0]) + 2, int(sa["dropped"][1]) + 1]
    A.close(), B.close()


@pytest.mark.gpu
def test_a_silent_peer_ends_in_failures_and_an_rst_on_the_wire(enc):
    """B never answers.  A's clock is the deadline it read back: the RTO fires
    max_retries + 1 times, the member ends with reason FAILURES and its RST is
    on the wire; the member that wrote nothing stays live."""
    now = 1_000_000
    A = Endpoint(enc, 2, now, max_retries=3)
    A.write([(np.arange(9000) & 0xff).astype(np.uint8), np.zeros(0, np.uint8)])
    rst = bytes(np.frombuffer(pr.encode(flags=0x08, packet_number=0), np.uint8) ^ _pad(SLOT)[:2])
    seen_rst, rounds = [], 0
    while True:
        rounds += 1
        assert rounds <= 12, (A.exits, A.sset.states()["rto_count"], A.loop.states())
        wire, lens, conn, npk, look = A.send(now)
        for i in range(npk):
            if look["flags"][i] == 0x08:
                seen_rst.append((int(conn[i]), bytes(wire[i, :int(lens[i])].cpu().numpy())))
        if 0 in A.exits:
            break
        assert now < A.deadline < 1 << 63
        now = A.deadline                                                  # the host sleeps until then
        A.receive(None, None, None, 0, now)
    st = A.sset.states()
    assert int(st["rto_count"][0]) == 4 and A.exits == {0: lf.FAILURES}
    assert seen_rst == [(0, rst)]
    assert not A.loop.states()["exited"][1]
    A.close()


@pytest.mark.gpu
def test_a_lost_fin_ends_the_peers_by_the_idle_timer(enc):
    """The other half of what the link of the two-peer test spares: A's FIN is
    lost.  Nothing retransmits it, B never reads eof and never closes.  B heard
    of A last before A heard of B (A's last packet against B's last ACK), so B
    goes idle first: reason IDLE with its RST on the wire, and A ends by that
    RST, reason PEER_RST, owing none.  The host's clock is the earlier of the
    two deadlines it read back."""
    now = 1_000_000
    A, B = Endpoint(enc, 1, now, idle_us=2_000_000), Endpoint(enc, 1, now, idle_us=2_000_000)
    data = (np.arange(4000) & 0xff).astype(np.uint8)
    A.write([data])
    A.app_close([0], now)
    none, rsts, fins, rounds = [0], {"A": 0, "B": 0}, 0, 0
    while not (A.exits and B.exits):
        rounds += 1
        assert rounds <= 60, (A.exits, B.exits, A.loop.states(), B.loop.states())
        wire, lens, conn, npk, look = A.send(now)
        fins += int((look["flags"] == 0x10).sum())
        rsts["A"] += int((look["flags"] == 0x08).sum())
        if npk:
            keep = torch.tensor([i for i in range(npk) if look["flags"][i] != 0x10], dtype=torch.int64, device="cuda")
            npk = int(keep.numel())
            wire, lens, conn = (wire[keep].contiguous(), lens[keep].contiguous(), conn[keep].contiguous()) if npk \
                else (None, None, None)
        B.receive(wire, lens, conn, npk, now + 1000)
        wire, lens, conn, npk, look = B.send(now + 2000)
        rsts["B"] += int((look["flags"] == 0x08).sum())
        A.receive(wire, lens, conn, npk, now + 3000)
        live = [e.deadline for e in (A, B) if not e.exits]
        if live:
            now = max(now + 20_000, min(min(live), now + 500_000))
    assert fins == 1 and B.exits == {0: lf.IDLE} and A.exits == {0: lf.PEER_RST} and rsts == {"A": 0, "B": 1}
    assert bytes(B.got[0]) == data.tobytes() and not B.eof[0]
    sa = A.loop.states()
    assert sa["fin_sent"][0] == 1 and sa["fin_rcvd"][0] == 0
    A.close(), B.close()
