"""A set of congestion controllers on the device (ugo_fec_cc_*) beside one
RuleCc of tests/cc_ref.py per member; test infrastructure only.

CcHarness wraps a SentHarness without changing it: ugo_fec_cc_sent_ack goes
through SentHarness.ack, so everything that checks of ugo_fec_sent_set_ack is
checked of the new entry point, and the rows are compared beside.  After every
call every field of every controller record, the dense cutback array and every
output array are compared in whole; the calls write into arrays filled with
arbitrary bytes, and the operand arrays are compared with what went in.
"""
import numpy as np
import torch

import cc_ref as cr
import sent_ref as sr
from sent_harness import M64, SentHarness, _i64, _put
from ugo_amd import fec


def row_array(rows):
    """[dict] -> CC_ROW_DTYPE [n]"""
    out = np.zeros(len(rows), fec.CC_ROW_DTYPE)
    for k in cr.RuleCc.ROW_FIELDS:
        out[k] = [r[k] for r in rows]
    return out


def event_array(events):
    """[dict] -> SENT_EVENT_DTYPE [n]; absent fields are zero."""
    out = np.zeros(len(events), fec.SENT_EVENT_DTYPE)
    for i, e in enumerate(events):
        for k, v in e.items():
            out[k][i] = v
    return out


class _SentRulesOnly:
    def __init__(self, wss, seg_caps):
        self.rules = [sr.RuleSent(ws, seg_caps) for ws in wss]

    def record(self, packets, now_us=None):
        sr.record_set(self.rules, [(p[0], p[1] & M64, p[2], p[3], p[4], p[5] & M64, p[6]) for p in packets], now_us)


class CcRulesOnly:
    """What a driver uses of CcHarness (h.record, ack, rto, states, close) on
    the rules alone: the conditions a device run must meet are held on the CPU
    through the same generator and seeds."""

    def __init__(self, wss, seg_caps=1, **params):
        self.h = _SentRulesOnly(wss, seg_caps)
        self.nconn = len(wss)
        self.rules = [cr.RuleCc(**params) for _ in range(self.nconn)]

    def ack(self, events, rows, now_us):
        sent = self.h.rules
        return [r.ack(events[c], rows[c], now_us, sent[c].last_sent, sent[c].lio, sent[c].err)
                for c, r in enumerate(self.rules)]

    def rto(self, fired, packet_bytes, max_budget):
        sent = self.h.rules
        return [r.rto(int(fired[c]), sent[c].last_sent, sent[c].bytes_in_flight, packet_bytes, max_budget, sent[c].err)
                for c, r in enumerate(self.rules)]

    def states(self):
        out = np.zeros(self.nconn, fec.CC_STATE_DTYPE)
        for k in cr.RuleCc.FIELDS:
            out[k] = [getattr(r, k) & M64 for r in self.rules]
        return out

    def close(self):
        pass


class CcHarness:
    def __init__(self, enc, wss, seg_caps=1, watch=None, **params):
        self.h = SentHarness(enc, wss, seg_caps, watch=watch)
        self.nconn = self.h.nconn
        self.cc = fec.CcSet(enc, self.h.set, **params)
        self.rules = [cr.RuleCc(**params) for _ in range(self.nconn)]
        self.calls = 0
        self.check()

    def close(self):
        self.cc.close()
        self.h.close()

    def states(self):
        return self.cc.states()

    # ---------------------------------------------------------------- state
    def check(self, sent=False):
        states = self.cc.states()                          # waits for the last call
        assert states.shape == (self.nconn,)
        want = [r.view() for r in self.rules]
        for k in cr.RuleCc.FIELDS:
            exp = np.array([w[k] & M64 for w in want], np.uint64)
            got = states[k].astype(np.uint64)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"cc field {k} differs at members {bad[:8]}: {got[bad[:8]]} vs {exp[bad[:8]]}"
        assert not states["reserved"].any()
        cut = self.cc.cutback().cpu().numpy().view(np.uint64)
        assert np.array_equal(cut, states["cutback"]), "the dense cutback array is not the records'"
        if sent:
            self.h.check()                                 # a controller call leaves the sent histories alone
        return states

    # ---------------------------------------------------------------- ugo_fec_cc_sent_ack
    def sent_ack(self, packets, max_ranges=4, now_us=None, split=None, where="device"):
        """SentHarness.ack through ugo_fec_cc_sent_ack.  split: a list, or None
        for the set's own cutback array.  Returns (events, rows) as numpy records."""
        h = self.h
        self.calls += 1
        before = [{n: s["state"] for n, s in r.slots.items()} for r in h.rules]
        splits = [r.cutback for r in self.rules] if split is None else [s & M64 for s in split]
        dsplit = self.cc.cutback() if split is None else _put(_i64(splits), where)
        rows0 = np.random.default_rng(600 + self.calls).integers(0, 256, (self.nconn, 32), dtype=np.uint8)
        drows = _put(rows0, where)

        def through(info, ranges, conn, now, npackets=None, events=None):
            self.cc.sent_ack(info, ranges, conn, now, npackets=npackets, events=events, split=dsplit, rows=drows)
            return events

        h.set.ack = through                                # shadows SentTxSet.ack for this call
        try:
            ev = h.ack(packets, max_ranges=max_ranges, now_us=now_us, where=where)
        finally:
            del h.set.ack
        want = row_array([cr.cc_row(before[c], h.rules[c], ev[c], splits[c]) for c in range(self.nconn)])
        got = drows.cpu().numpy().view(fec.CC_ROW_DTYPE).reshape(-1)
        for k in cr.RuleCc.ROW_FIELDS:
            bad = np.flatnonzero(got[k] != want[k])
            assert bad.size == 0, f"row field {k} differs at members {bad[:8]}: {got[k][bad[:8]]} vs {want[k][bad[:8]]}"
        assert not got["reserved"].any()
        assert np.array_equal(dsplit.cpu().numpy().view(np.uint64), np.asarray(splits, np.uint64))
        self.check()
        return ev, got

    # ---------------------------------------------------------------- ugo_fec_cc_set_ack
    def ack(self, events, rows, now_us, where="device"):
        """events: SENT_EVENT_DTYPE [nconn], rows: CC_ROW_DTYPE [nconn] (numpy).
        Returns delay_us as a list."""
        self.calls += 1
        ev_bytes = np.ascontiguousarray(events).view(np.uint8).reshape(self.nconn, 64)
        row_bytes = np.ascontiguousarray(rows).view(np.uint8).reshape(self.nconn, 32)
        dev, drows = _put(ev_bytes, where), _put(row_bytes, where)
        ddelay = _put(np.full(self.nconn, 0x5555555555555555, np.int64), where)
        self.cc.ack(dev, drows, now_us, delay_us=ddelay)
        sent = self.h.rules
        want = [r.ack(events[c], rows[c], now_us, sent[c].last_sent, sent[c].lio, sent[c].err)
                for c, r in enumerate(self.rules)]
        self.check(sent=True)
        got = ddelay.cpu().numpy().view(np.uint64).tolist()
        assert got == want, [(c, g, w) for c, (g, w) in enumerate(zip(got, want)) if g != w][:8]
        assert np.array_equal(dev.cpu().numpy(), ev_bytes) and np.array_equal(drows.cpu().numpy(), row_bytes)
        return got

    # ---------------------------------------------------------------- ugo_fec_cc_set_rto
    def rto(self, fired, packet_bytes, max_budget, where="device"):
        self.calls += 1
        f0 = np.asarray(fired, np.uint8)
        dfired = _put(f0, where)
        dbudget = _put(np.full(self.nconn, 0x77777777, np.int32), where)
        self.cc.rto(dfired, packet_bytes, max_budget, budget=dbudget)
        sent = self.h.rules
        want = [r.rto(int(f0[c]), sent[c].last_sent, sent[c].bytes_in_flight, packet_bytes, max_budget, sent[c].err)
                for c, r in enumerate(self.rules)]
        self.check(sent=True)
        got = dbudget.cpu().numpy().view(np.uint32).tolist()
        assert got == want, [(c, g, w) for c, (g, w) in enumerate(zip(got, want)) if g != w][:8]
        assert np.array_equal(dfired.cpu().numpy(), f0)
        return got

    # ---------------------------------------------------------------- a batch in THE ORDER
    def batch(self, packets, now_us, packet_bytes=1400, max_budget=64, max_ranges=4):
        """ugo_fec_cc_sent_ack, ugo_fec_cc_set_ack, ugo_fec_sent_set_rto with the
        delays just written, ugo_fec_cc_set_rto.  Returns (events, rows, fired, budget)."""
        ev, rows = self.sent_ack(packets, max_ranges=max_ranges, now_us=now_us)
        delays = self.ack(ev, rows, now_us)
        fired = self.h.rto(delays, now_us)
        return ev, rows, fired, self.rto(fired, packet_bytes, max_budget)
