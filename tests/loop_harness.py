"""The connection loop of a set on the device (ugo_fec_loop_set_*) beside one
RuleLoop of tests/loop_ref.py per member; test infrastructure only.

The harness owns the four neighbouring sets, with the smallest members they
allow, and moves them through their own calls (record, rto, receive, deliver,
write).  Before a loop call it reads their records back: those are the
operands the rule is given.  After every call every field of every loop record
and every output array are compared in whole; outputs are written into arrays
filled with arbitrary bytes between two guards, and the operand arrays are
compared with what went in.
"""
import numpy as np
import torch

import loop_ref as lf
from listen_harness import GUARD, Guarded, _put
from ugo_amd import fec

NO_CONN = fec.STREAM_NO_CONN
M64 = (1 << 64) - 1
TX_CAP = 4096


def _i64(values):
    return np.asarray([int(v) & M64 for v in values], np.uint64).view(np.int64)


def make_info(status, flags, pn, seed=0):
    """PKT_INFO_DTYPE records with arbitrary bytes in every other field."""
    n = len(status)
    raw = np.random.default_rng(seed).integers(0, 256, (max(n, 1), 64), dtype=np.uint8)
    iv = raw.view(fec.PKT_INFO_DTYPE).reshape(-1)
    iv["status"][:n], iv["flags"][:n], iv["packet_number"][:n] = status, flags, pn
    return raw


class Nbs:
    """The members' neighbouring records: nbs[c] is the dict loop_ref takes."""

    def __init__(self, cols):
        self.cols = {k: np.asarray(v).astype(np.uint64) for k, v in cols.items()}

    def __getitem__(self, c):
        d = {k: int(v[c]) for k, v in self.cols.items()}
        d["cap"] = TX_CAP
        return d

    def __eq__(self, other):
        return all(np.array_equal(v, other.cols[k]) for k, v in self.cols.items())


class LoopHarness:
    def __init__(self, enc, nconn, now_us=0, where="device", **params):
        self.enc, self.nconn, self.where = enc, nconn, where
        self.rxs = [fec.StreamRx(enc, 4096) for _ in range(nconn)]
        self.acks = [fec.AckRx(enc, 2048) for _ in range(nconn)]
        self.txs = [fec.StreamTx(enc, TX_CAP, 4) for _ in range(nconn)]
        self.sents = [fec.SentTx(enc, 1024, 1) for _ in range(nconn)]
        self.rx_set, self.ack_set = fec.StreamRxSet(enc, self.rxs), fec.AckRxSet(enc, self.acks)
        self.tx_set, self.sent_set = fec.StreamTxSet(enc, self.txs), fec.SentTxSet(enc, self.sents)
        self.loop = fec.LoopSet(enc, self.rx_set, self.ack_set, self.tx_set, self.sent_set, now_us=now_us, **params)
        self.rules = [lf.RuleLoop(now_us, **params) for _ in range(nconn)]
        self.calls = 0
        self._nbs = None
        self.check()

    def close(self):
        self.loop.close()
        for s in (self.rx_set, self.ack_set, self.tx_set, self.sent_set):
            s.close()
        for m in self.rxs + self.acks + self.txs + self.sents:
            m.close()

    # ---------------------------------------------------------------- state
    def check(self):
        states = self.loop.states()                        # waits for the last call
        assert states.shape == (self.nconn,)
        for k in lf.RuleLoop.FIELDS:
            exp = np.array([getattr(r, k) for r in self.rules], np.uint64)
            got = states[k].astype(np.uint64)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"loop field {k} differs at members {bad[:8]}: {got[bad[:8]]} vs {exp[bad[:8]]}"
        assert not states["reserved"].any()
        return states

    def nbs(self):
        """The neighbouring records as the device holds them: the rule's operands."""
        if self._nbs is None:
            rx, ak = self.rx_set.states(), self.ack_set.states()
            tx, st = self.tx_set.states(), self.sent_set.states()
            self._nbs = Nbs(dict(stream_err=rx["err"], ack_err=ak["err"], sent_err=st["err"],
                                 rto_count=st["rto_count"], tracked=st["tracked"], last_sent_us=st["last_sent_us"],
                                 tail=tx["tail"], write_pos=tx["write_pos"], rq_len=tx["rq_len"]))
        return self._nbs

    def _neighbours_untouched(self, before):
        self._nbs = None
        assert self.nbs() == before, "a loop call wrote a neighbouring record"

    # ---------------------------------------------------------------- the neighbours' own calls
    def sent_record(self, packets, now_us):
        """packets: [(conn, n)]: one packet of 100 bytes each, one segment."""
        n = len(packets)
        raw = np.zeros((n, 64), np.uint8)
        iv = raw.view(fec.PKT_INFO_DTYPE).reshape(-1)
        iv["packet_number"], iv["n_segments"] = [p[1] for p in packets], 1
        segs = np.zeros((n, 1, 16), np.uint8)
        sv = segs.view(fec.PKT_SEGMENT_DTYPE).reshape(n, 1)
        sv["offset"][:, 0], sv["len"][:, 0] = [10 * p[1] for p in packets], 10
        conn = np.asarray([p[0] for p in packets], np.uint32).view(np.int32)
        self.sent_set.record(_put(raw), _put(segs), _put(conn), _put(np.full(n, 100, np.int16)),
                             _put(np.zeros(n, np.uint8)), now_us)
        self._nbs = None

    def sent_rto(self, now_us):
        fired = self.sent_set.rto(_put(np.zeros(self.nconn, np.int64)), now_us)
        self._nbs = None
        return fired.cpu().numpy()

    def ack_receive(self, packets, now_us):
        """packets: [(conn, n)] of received packet numbers."""
        n = len(packets)
        raw = np.zeros((n, 64), np.uint8)
        raw.view(fec.PKT_INFO_DTYPE).reshape(-1)["packet_number"] = [p[1] for p in packets]
        self.ack_set.receive(_put(raw), _put(np.asarray([p[0] for p in packets], np.uint32).view(np.int32)), now_us)
        self._nbs = None

    def stream_deliver(self, packets):
        """packets: [(conn, offset, len)]: one segment each, its bytes at 16 of a 64-byte slot."""
        n = len(packets)
        raw = np.zeros((n, 64), np.uint8)
        raw.view(fec.PKT_INFO_DTYPE).reshape(-1)["n_segments"] = 1
        segs = np.zeros((n, 1, 16), np.uint8)
        sv = segs.view(fec.PKT_SEGMENT_DTYPE).reshape(n, 1)
        sv["offset"][:, 0], sv["data_off"][:, 0] = [p[1] for p in packets], 16
        sv["len"][:, 0] = sv["avail"][:, 0] = [p[2] for p in packets]
        self.rx_set.deliver(_put(np.zeros((n, 64), np.uint8)), _put(raw), _put(segs),
                            _put(np.asarray([p[0] for p in packets], np.uint32).view(np.int32)))
        self._nbs = None

    def tx_write(self, counts):
        """counts[c] bytes written to member c's send window."""
        src = _put(np.zeros(max(1, max(counts)), np.uint8))
        self.tx_set.write(src, _put(np.zeros(self.nconn, np.int64)), _put(np.asarray(counts, np.int64)))
        self._nbs = None

    # ---------------------------------------------------------------- ugo_fec_loop_set_receive
    def receive(self, status, flags, pn, conn_of, now_us, where=None):
        where = where or self.where
        self.calls += 1
        n = len(conn_of)
        before = self.nbs()
        raw = make_info(status, flags, pn, 100 + self.calls)
        conn0 = np.asarray(conn_of, np.uint32)
        dinfo = _put(raw, where)
        g = Guarded(4 * n, 200 + self.calls, where)
        dconn = g.view(torch.int32, n)
        dconn.copy_(torch.from_numpy(conn0.view(np.int32)))
        self.loop.receive(dinfo, dconn, now_us, npackets=n)
        want = lf.receive_set(self.rules, status, flags, pn, conn0.tolist(), now_us)
        self.check()
        got = g.read().view(np.uint32)
        bad = np.flatnonzero(got != np.asarray(want, np.uint32))
        assert bad.size == 0, f"conn_of differs at {bad[:8]}: {got[bad[:8]]} vs {np.asarray(want)[bad[:8]]}"
        assert np.array_equal(dinfo.cpu().numpy(), raw), "receive wrote info"
        self._neighbours_untouched(before)
        return got

    # ---------------------------------------------------------------- ugo_fec_loop_set_close
    def close_members(self, how, now_us, linger_us=None, where=None):
        where = where or self.where
        self.calls += 1
        before = self.nbs()
        h0 = np.asarray(how, np.uint8)
        dhow = _put(h0, where)
        dl = None if linger_us is None else _put(_i64(linger_us), where)
        self.loop.close_members(dhow, now_us, linger_us=dl)
        lf.close_set(self.rules, h0, linger_us, now_us)
        self.check()
        assert np.array_equal(dhow.cpu().numpy(), h0)
        if dl is not None:
            assert np.array_equal(dl.cpu().numpy(), _i64(linger_us))
        self._neighbours_untouched(before)

    # ---------------------------------------------------------------- ugo_fec_loop_set_check
    def check_call(self, now_us, budget, where=None):
        """Returns (budget, may_ack_only) as lists."""
        where = where or self.where
        self.calls += 1
        before = self.nbs()
        b0 = np.asarray(budget, np.uint32)
        gb, gm = Guarded(4 * self.nconn, 300 + self.calls, where), Guarded(self.nconn, 400 + self.calls, where)
        db = gb.view(torch.int32, self.nconn)
        db.copy_(torch.from_numpy(b0.view(np.int32)))
        self.loop.check(now_us, db, may_ack_only=gm.view(torch.uint8, self.nconn))
        wb, wm = lf.check_set(self.rules, before, now_us, b0.tolist())
        self.check()
        got_b, got_m = gb.read().view(np.uint32).tolist(), gm.read().tolist()
        assert got_b == wb, [(c, g, w) for c, (g, w) in enumerate(zip(got_b, wb)) if g != w][:8]
        assert got_m == wm, [(c, g, w) for c, (g, w) in enumerate(zip(got_m, wm)) if g != w][:8]
        self._neighbours_untouched(before)
        return got_b, got_m

    # ---------------------------------------------------------------- ugo_fec_loop_set_append
    def append(self, total, max_packets, max_segments=2, alias=True, where=None):
        """Returns (info bytes, segs bytes, conn_of, total_out, appended, writes)."""
        where = where or self.where
        self.calls += 1
        before = self.nbs()
        seed = 500 + 10 * self.calls
        gi, gs = Guarded(64 * max_packets, seed, where), Guarded(16 * max_packets * max_segments, seed + 1, where)
        gc, ga = Guarded(4 * max_packets, seed + 2, where), Guarded(self.nconn, seed + 3, where)
        gt = Guarded(16, seed + 4, where)
        tt = gt.view(torch.int64, 2)
        tt[0] = total
        dtotal, dout = tt[0:1], (tt[0:1] if alias else tt[1:2])
        self.loop.append(dtotal, gi.view(torch.uint8, max_packets, 64), gs.view(torch.uint8, max_packets,
                                                                                max_segments, 16),
                         gc.view(torch.int32, max_packets), total_out=dout, appended=ga.view(torch.uint8, self.nconn),
                         max_packets=max_packets)
        writes, wa, wt = lf.append_set(self.rules, before, total, max_packets)
        self.check()
        info = gi.fill[GUARD:GUARD + 64 * max_packets].copy().reshape(max_packets, 64)
        segs = gs.fill[GUARD:GUARD + 16 * max_packets * max_segments].copy().reshape(max_packets, max_segments, 16)
        conn = gc.fill[GUARD:GUARD + 4 * max_packets].copy().view(np.uint32)
        for t, c, what, off, data_off in writes:
            info[t] = 0
            iv = info[t].view(fec.PKT_INFO_DTYPE)
            iv["flags"], iv["n_segments"] = (0x10, 1) if what == lf.FIN else (0x08, 0)
            conn[t] = c
            if what == lf.FIN:
                sv = segs[t, 0].view(fec.PKT_SEGMENT_DTYPE)
                sv["offset"], sv["data_off"], sv["len"], sv["avail"] = off, data_off, 0, 0
        got_i, got_s = gi.read().reshape(max_packets, 64), gs.read().reshape(max_packets, max_segments, 16)
        assert np.array_equal(got_i, info), f"info differs at {np.argwhere(got_i != info)[:8].tolist()}"
        assert np.array_equal(got_s, segs), f"segs differ at {np.argwhere(got_s != segs)[:8].tolist()}"
        assert np.array_equal(gc.read().view(np.uint32), conn), "conn_of differs"
        assert ga.read().tolist() == wa
        tot = gt.read().view(np.uint64)
        exp_tot = gt.fill[GUARD:GUARD + 16].copy().view(np.uint64)
        exp_tot[0] = total
        exp_tot[0 if alias else 1] = wt
        assert tot.tolist() == exp_tot.tolist(), (tot.tolist(), exp_tot.tolist())
        self._neighbours_untouched(before)
        return got_i, got_s, conn, wt, wa, writes

    # ---------------------------------------------------------------- ugo_fec_loop_set_sent
    def sent(self, n_packets, attached, now_us, delay_us=None, max_exits=None, remap=True, where=None):
        """Returns (deadline, exits, reasons, n_exits, new_index, nconn_new)."""
        where = where or self.where
        self.calls += 1
        before = self.nbs()
        cap = self.nconn if max_exits is None else max_exits
        np0, at0 = np.asarray(n_packets, np.uint32), np.asarray(attached, np.uint8)
        dn, da = _put(np0.view(np.int32), where), _put(at0, where)
        dd = None if delay_us is None else _put(_i64(delay_us), where)
        seed = 700 + 10 * self.calls
        gd, ge, gr = Guarded(8, seed, where), Guarded(4 * cap, seed + 1, where), Guarded(cap, seed + 2, where)
        gn, gx, gk = Guarded(8, seed + 3, where), Guarded(4 * self.nconn, seed + 4, where), Guarded(8, seed + 5, where)
        out = (gd.view(torch.int64, 1), ge.view(torch.int32, cap), gr.view(torch.uint8, cap), gn.view(torch.int64, 1),
               gx.view(torch.int32, self.nconn) if remap else None, gk.view(torch.int64, 1) if remap else None)
        self.loop.sent(dn, da, now_us, delay_us=dd, max_exits=cap, out=out)
        want = lf.sent_set(self.rules, before, np0, at0, delay_us, now_us, cap)
        self.check()
        k = len(want[1])
        exits, reasons = ge.read().view(np.uint32), gr.read()
        assert int(gd.read().view(np.uint64)[0]) == want[0], (int(gd.read().view(np.uint64)[0]), want[0])
        assert int(gn.read().view(np.uint64)[0]) == want[3], (int(gn.read().view(np.uint64)[0]), want[3])
        assert exits[:k].tolist() == want[1] and reasons[:k].tolist() == want[2], (exits[:8], want[1][:8])
        assert np.array_equal(exits[k:], ge.fill[GUARD + 4 * k:GUARD + 4 * cap].view(np.uint32)) and \
            np.array_equal(reasons[k:], gr.fill[GUARD + k:GUARD + cap]), "the exit list was written past its end"
        if remap:
            assert gx.read().view(np.uint32).tolist() == want[4]
            assert int(gk.read().view(np.uint64)[0]) == want[5]
        else:
            gx.read(), gk.read()
        assert np.array_equal(dn.cpu().numpy().view(np.uint32), np0) and np.array_equal(da.cpu().numpy(), at0)
        if dd is not None:
            assert np.array_equal(dd.cpu().numpy(), _i64(delay_us))
        self._neighbours_untouched(before)
        return want
