"""A set of sent histories on the device (ugo_fec_sent_set_*) beside one
RuleSent of tests/sent_ref.py per member; test infrastructure only.

After every call SentHarness compares every field of every member's record, the
slot ring and the segment ring of the watched members in whole, and every
output array in whole: the calls write into arrays filled with arbitrary
bytes, so a write outside what they may touch shows, and the operand arrays are
compared with what went in.
"""
import numpy as np
import torch

import sent_ref as sr
from ugo_amd import fec

NO_CONN = fec.STREAM_NO_CONN
M64 = (1 << 64) - 1


def _put(arr, where="device"):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return t.pin_memory() if where == "pinned" else t.cuda()


def _i64(values):
    return np.asarray([v & M64 for v in values], np.uint64).view(np.int64)


class SentHarness:
    def __init__(self, enc, wss, seg_caps=4, watch=None):
        self.wss = list(wss)
        self.nconn = n = len(self.wss)
        self.caps = [seg_caps] * n if isinstance(seg_caps, int) else list(seg_caps)
        self.watch = list(range(n)) if watch is None else list(watch)
        self.txs = [fec.SentTx(enc, ws, cap) for ws, cap in zip(self.wss, self.caps)]
        self.rules = [sr.RuleSent(ws, cap) for ws, cap in zip(self.wss, self.caps)]
        self.set = fec.SentTxSet(enc, self.txs)
        self.enc = enc
        self.calls = 0
        self.check()

    def close(self):
        self.set.close()
        for tx in self.txs:
            tx.close()

    # ---------------------------------------------------------------- state
    def check(self):
        states = self.set.states()                       # waits for the last call
        assert states.shape == (self.nconn,)
        want = [r.record_fields() for r in self.rules]
        for k in sr.RuleSent.FIELDS:
            exp = np.array([w[k] & M64 for w in want], np.uint64)
            got = states[k].astype(np.uint64)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"record field {k} differs at members {bad[:8]}: {got[bad[:8]]} vs {exp[bad[:8]]}"
        assert not states["reserved"].any()
        for c in self.watch:
            got = self.txs[c].slots().cpu().numpy().view(fec.SENT_SLOT_DTYPE).reshape(-1)
            exp = self.rules[c].slot_ring(fec.SENT_SLOT_DTYPE)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"slot ring of member {c} differs at {bad[:8]}: {got[bad[:4]]} vs {exp[bad[:4]]}"
            assert not bool(self.txs[c].scratch().any()), f"member {c}: a difference or claim word is left set"
            seg = self.txs[c].segments().cpu().numpy().view(fec.SENT_SEG_DTYPE).reshape(self.wss[c], self.caps[c])
            ring = self.rules[c].seg_ring
            assert np.array_equal(seg["offset"], ring[:, :, 0]) and np.array_equal(seg["len"], ring[:, :, 1]) and \
                not seg["reserved"].any(), f"segment ring of member {c} differs"
        return states

    def _now(self, now_us):
        self.calls += 1
        return 1000 * self.calls if now_us is None else now_us

    # ---------------------------------------------------------------- record
    def record(self, packets, max_segments=None, now_us=None, where="device"):
        """packets: [(conn, n, wire_len, status, flags, stop_waiting, [(offset,
        len)], n_segments or None)] in batch order; n_segments is what the
        descriptor says when it is not len(segments)."""
        now_us = self._now(now_us)
        npk = len(packets)
        ms = min(self.caps) if max_segments is None else max_segments
        rng = np.random.default_rng(100 + self.calls)
        raw = rng.integers(0, 256, (npk, 64), dtype=np.uint8)
        iv = raw.view(fec.PKT_INFO_DTYPE).reshape(npk)
        segs = rng.integers(0, 256, (npk, ms, 16), dtype=np.uint8)
        sv = segs.view(fec.PKT_SEGMENT_DTYPE).reshape(npk, ms)
        conn = np.zeros(npk, np.uint32)
        lens, status = np.zeros(npk, np.uint16), np.zeros(npk, np.uint8)
        model = []
        for i, p in enumerate(packets):
            c, n, length, st, flags, sw, sg = p[:7]
            nseg = p[7] if len(p) > 7 and p[7] is not None else len(sg)
            conn[i], lens[i], status[i] = c & 0xffffffff, length, st
            iv["packet_number"][i], iv["stop_waiting"][i] = n & M64, sw & M64
            iv["flags"][i], iv["n_segments"][i] = flags, nseg
            for j, (off, ln) in enumerate(sg[:ms]):
                sv["offset"][i, j], sv["len"][i, j] = off & M64, ln
            stored = [(int(sv["offset"][i, j]), int(sv["len"][i, j])) for j in range(min(nseg, ms))]
            model.append((c & 0xffffffff, n & M64, length, st, flags, sw & M64, stored))
        d = [_put(x, where) for x in (raw, segs, conn.view(np.int32), lens.view(np.int16), status)]
        self.set.record(d[0], d[1], d[2], d[3], d[4], now_us)
        sr.record_set(self.rules, model, now_us)
        states = self.check()
        for t, x in zip(d, (raw, segs, conn.view(np.int32), lens.view(np.int16), status)):
            assert np.array_equal(t.cpu().numpy(), x), "record wrote an operand"
        return states

    def send(self, c, numbers, length=100, flags=0, sw=0, segs=None, now_us=None):
        """Member c sends the numbers, one segment of 10 bytes at 10 n each."""
        return self.record([(c, n, length, 0, flags, sw, [(10 * n, 10)] if segs is None else segs) for n in numbers],
                           now_us=now_us)

    # ---------------------------------------------------------------- ack
    def ack(self, packets, max_ranges=4, now_us=None, where="device"):
        """packets: [(status, conn, flags, Ack, n_ranges or None)] in batch
        order.  Returns the event rows (SENT_EVENT_DTYPE [nconn])."""
        now_us = self._now(now_us)
        npk = len(packets)
        rng = np.random.default_rng(200 + self.calls)
        raw = rng.integers(0, 256, (max(npk, 1), 64), dtype=np.uint8)
        iv = raw.view(fec.PKT_INFO_DTYPE).reshape(-1)
        ranges = rng.integers(0, 2 ** 62, (max(npk, 1), max_ranges, 2), dtype=np.int64)
        conn = np.zeros(max(npk, 1), np.uint32)
        model = []
        for i, p in enumerate(packets):
            st, c, flags, a = p[:4]
            nr = p[4] if len(p) > 4 and p[4] is not None else len(a.ranges)
            conn[i] = c & 0xffffffff
            iv["status"][i], iv["flags"][i], iv["n_ranges"][i] = st, flags, nr
            iv["packet_number"][i], iv["largest_acked"][i], iv["largest_in_order"][i] = a.w, a.la, a.lio
            iv["delay_us"][i] = a.delay
            for k, (f, l) in enumerate(a.ranges[:max_ranges]):
                ranges[i, k] = (f, l)
            rows = [(int(ranges[i, k, 0]), int(ranges[i, k, 1])) for k in range(max_ranges)]
            model.append((st, c & 0xffffffff, flags, sr.Ack(a.la, a.lio, rows, a.w, a.delay), nr))
        dinfo, dranges, dconn = _put(raw, where), _put(ranges, where), _put(conn.view(np.int32), where)
        dev = _put(np.random.default_rng(300 + self.calls).integers(0, 256, (self.nconn, 64), dtype=np.uint8), where)
        self.set.ack(dinfo, dranges, dconn, now_us, npackets=npk, events=dev)
        want = sr.ack_set(self.rules, model, now_us, max_ranges)
        self.check()
        got = dev.cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)
        for k in sr.RuleSent.EVENT_FIELDS:
            exp = np.array([w[k] & M64 for w in want], np.uint64)
            bad = np.flatnonzero(got[k].astype(np.uint64) != exp)
            assert bad.size == 0, f"event field {k} differs at members {bad[:8]}: {got[k][bad[:8]]} vs {exp[bad[:8]]}"
        assert not got["reserved"].any()
        assert np.array_equal(dinfo.cpu().numpy(), raw) and np.array_equal(dranges.cpu().numpy(), ranges) and \
            np.array_equal(dconn.cpu().numpy().view(np.uint32), conn)
        return got

    def ack1(self, c, la, lio, ranges=(), w=0, delay=0, **kw):
        return self.ack([(0, c, 0x80, sr.Ack(la, lio, ranges, w, delay))], **kw)

    # ---------------------------------------------------------------- rto
    def rto(self, delays, now_us, where="device"):
        self.calls += 1
        ddel = _put(_i64(delays), where)
        dfired = _put(np.full(self.nconn, 0x77, np.uint8), where)
        self.set.rto(ddel, now_us, fired=dfired)
        want = sr.rto_set(self.rules, delays, now_us)
        self.check()
        got = dfired.cpu().numpy().tolist()
        assert got == want, (got[:16], want[:16])
        assert np.array_equal(ddel.cpu().numpy(), _i64(delays))
        return got

    # ---------------------------------------------------------------- drain
    def drain(self, max_entries, where="device"):
        """Returns (conn_of, offset, len of the entries written, touch, upto)."""
        self.calls += 1
        rng = np.random.default_rng(400 + self.calls)
        conn0 = rng.integers(0, 2 ** 31, max_entries, dtype=np.int64).astype(np.int32)
        off0 = rng.integers(-2 ** 62, 2 ** 62, max_entries, dtype=np.int64)
        len0 = rng.integers(0, 2 ** 31, max_entries, dtype=np.int64).astype(np.int32)
        out = (_put(conn0, where), _put(off0, where), _put(len0, where), _put(np.full(1, -1, np.int64), where),
               _put(np.full(self.nconn, 0x77, np.uint8), where), _put(np.full(self.nconn, 0x55, np.int64), where))
        self.set.drain(max_entries, out=out)
        conn, off, ln, touch, upto = sr.drain_set(self.rules, max_entries)
        self.check()
        n = len(conn)
        assert int(out[3].cpu().numpy()[0]) == n, (int(out[3].cpu().numpy()[0]), n)
        econn, eoff, elen = conn0.view(np.uint32).copy(), off0.view(np.uint64).copy(), len0.view(np.uint32).copy()
        econn[:n], eoff[:n], elen[:n] = conn, np.asarray(off, np.uint64), ln
        econn[n:] = NO_CONN
        for name, got, exp in (("conn_of", out[0].cpu().numpy().view(np.uint32), econn),
                               ("offset", out[1].cpu().numpy().view(np.uint64), eoff),
                               ("len", out[2].cpu().numpy().view(np.uint32), elen)):
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"drain's {name} differs at {bad[:8]}: {got[bad[:8]]} vs {exp[bad[:8]]}"
        assert out[4].cpu().numpy().tolist() == touch
        assert out[5].cpu().numpy().view(np.uint64).tolist() == upto
        return conn, off, ln, touch, upto

    # ---------------------------------------------------------------- attach
    def attach(self, first, counts, max_packets, where="device"):
        self.calls += 1
        info0 = np.random.default_rng(500 + self.calls).integers(0, 256, (max_packets, 64), dtype=np.uint8)
        dinfo = _put(info0, where)
        dfirst, dcount = _put(_i64(first), where), _put(np.asarray(counts, np.uint32).view(np.int32), where)
        datt = _put(np.full(self.nconn, 0x77, np.uint8), where)
        self.set.attach(dfirst, dcount, dinfo, attached=datt)
        writes, attached = sr.attach_set(self.rules, list(first), list(counts), max_packets)
        self.check()
        info = info0.copy()
        iv = info.view(fec.PKT_INFO_DTYPE).reshape(-1)
        for t, sw in writes:
            iv["stop_waiting"][t] = sw
        bad = np.argwhere(dinfo.cpu().numpy() != info)
        assert bad.size == 0, f"attach's info differs at {bad[:8].tolist()}"
        assert datt.cpu().numpy().tolist() == attached
        assert np.array_equal(dfirst.cpu().numpy(), _i64(first))
        return writes, attached
