"""A set of receive histories on the device (ugo_fec_ack_set_*) beside one
RuleAck of tests/ack_ref.py per member; test infrastructure only.

After every call AckHarness compares every field of every member's record, the
whole bitmap of the watched members (default all), and every output array in
whole: attach writes into arrays filled with arbitrary bytes, so a write
outside the fields, rows and records it may touch shows, and the operand
arrays are compared with what went in.
"""
import numpy as np
import torch

import ack_ref as ar
from ugo_amd import fec

NO_CONN = fec.STREAM_NO_CONN
M64 = (1 << 64) - 1


def _put(arr, where="device"):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return t.pin_memory() if where == "pinned" else t.cuda()


def _i64(values):
    return np.asarray([v & M64 for v in values], np.uint64).view(np.int64)


def make_info(packets, seed=0):
    """PKT_INFO_DTYPE [npk] from [(status, conn, n, sw, n_segments)]: the fields
    receive reads as given, every other byte arbitrary."""
    npk = len(packets)
    raw = np.random.default_rng(seed).integers(0, 256, (npk, 64), dtype=np.uint8)
    iv = raw.view(fec.PKT_INFO_DTYPE).reshape(npk)
    iv["status"] = [p[0] for p in packets]
    iv["packet_number"] = np.asarray([p[2] & M64 for p in packets], np.uint64)
    iv["stop_waiting"] = np.asarray([p[3] & M64 for p in packets], np.uint64)
    iv["n_segments"] = [p[4] for p in packets]
    return raw


class AckHarness:
    def __init__(self, enc, wps, watch=None):
        self.wps = list(wps)
        self.nconn = n = len(self.wps)
        self.watch = list(range(n)) if watch is None else list(watch)
        self.rxs = [fec.AckRx(enc, wp) for wp in self.wps]
        self.rules = [ar.RuleAck(wp) for wp in self.wps]
        self.set = fec.AckRxSet(enc, self.rxs)
        self.enc = enc
        self.calls = 0
        self.check()                                     # create: everything zero

    def close(self):
        self.set.close()
        for rx in self.rxs:
            rx.close()

    # ---------------------------------------------------------------- state
    def check(self):
        states = self.set.states()                       # waits for the last call
        assert states.shape == (self.nconn,)
        want = [r.record() for r in self.rules]
        for k in ar.RuleAck.FIELDS:
            exp = np.array([w[k] for w in want], np.uint64)
            got = states[k].astype(np.uint64)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"record field {k} differs at members {bad[:8]}: {got[bad[:8]]} vs {exp[bad[:8]]}"
        assert not states["reserved"].any()
        for c in self.watch:
            got = self.rxs[c].bitmap().cpu().numpy().view(np.uint64)
            exp = self.rules[c].bitmap()
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (f"bitmap of member {c} differs at words {bad[:8]} (of {bad.size}): "
                                   f"{[hex(int(x)) for x in got[bad[:4]]]} vs {[hex(int(x)) for x in exp[bad[:4]]]}")
        if self.watch:                                   # the single-history view agrees with the gather
            c = self.watch[0]
            one = self.rxs[c].state()
            assert one.tobytes() == states[c].tobytes()
        return states

    def adopt(self, c, lio):
        """Start member c at largest_in_order = lio: a stop-waiting of lio + 1."""
        self.receive([(0, c, 0, lio + 1, 0)])

    # ---------------------------------------------------------------- receive
    def receive(self, packets, now_us=None, seg_rows=None, max_segments=0, where="device", seg_shift=0):
        """packets: [(status, conn, packet_number, stop_waiting, n_segments)] in
        batch order.  seg_rows: one list of max_segments statuses per packet,
        handed over seg_shift bytes past an aligned address."""
        self.calls += 1
        now_us = 1000 * self.calls if now_us is None else now_us
        npk = len(packets)
        raw = make_info(packets, seed=self.calls)
        conn = np.asarray([p[1] & 0xffffffff for p in packets], np.uint32)
        dinfo, dconn = _put(raw, where), _put(conn.view(np.int32), where)
        dseg = seg = None
        if seg_rows is not None:
            seg = np.asarray(seg_rows, np.uint8).reshape(npk, max_segments)
            room = _put(np.zeros(npk * max_segments + 64, np.uint8), where)
            at = (-room.data_ptr()) % 16 + seg_shift
            dseg = room[at:at + npk * max_segments].view(npk, max_segments)
            dseg.copy_(torch.from_numpy(seg))
        self.set.receive(dinfo, dconn, now_us, seg_status=dseg)
        ar.receive_set(self.rules, [(p[0], p[1], p[2] & M64, p[3] & M64, p[4], None if seg is None else seg[i])
                                    for i, p in enumerate(packets)], now_us, max_segments)
        states = self.check()
        assert np.array_equal(dinfo.cpu().numpy(), raw) and np.array_equal(dconn.cpu().numpy().view(np.uint32), conn)
        if seg is not None:
            assert np.array_equal(dseg.cpu().numpy(), seg)
        return states

    def touch(self, flags, where="device"):
        self.set.touch(_put(np.asarray(flags, np.uint8), where))
        for r, f in zip(self.rules, flags):
            if f:
                r.touch()
        self.check()

    # ---------------------------------------------------------------- attach
    def attach(self, first, counts, total, max_packets, max_ranges, may=None, now_us=None, where="device",
               alias_total=False):
        """One attach over arrays of arbitrary bytes; first / counts / total as
        set_plan would have left them.  Returns (writes, info, ranges, conn,
        total_out, attached): the rule's writes and the device arrays' host
        images (info as PKT_INFO_DTYPE)."""
        self.calls += 1
        now_us = 1000 * self.calls if now_us is None else now_us
        rng = np.random.default_rng(7000 + self.calls)
        info0 = rng.integers(0, 256, (max_packets, 64), dtype=np.uint8)
        ranges0 = rng.integers(-2 ** 62, 2 ** 62, (max_packets, max_ranges, 2), dtype=np.int64)
        conn0 = rng.integers(0, 2 ** 31, max_packets, dtype=np.int64).astype(np.int32)
        dinfo, dranges, dconn = _put(info0, where), _put(ranges0, where), _put(conn0, where)
        dfirst, dcount = _put(_i64(first), where), _put(np.asarray(counts, np.uint32).view(np.int32), where)
        dtotal = _put(np.asarray([total], np.int64), where)
        dmay = None if may is None else _put(np.asarray(may, np.uint8), where)
        dout = dtotal if alias_total else _put(np.full(1, -1, np.int64), where)
        datt = _put(np.full(self.nconn, 0x77, np.uint8), where)
        self.set.attach(now_us, dfirst, dcount, dtotal, dinfo, dranges, dconn, may_ack_only=dmay, total_out=dout,
                        attached=datt)
        writes, total_out, attached = ar.attach_set(self.rules, now_us, list(first), list(counts), total, may,
                                                    max_packets, max_ranges)
        self.check()
        info, ranges, conn = info0.copy(), ranges0.view(np.uint64).copy(), conn0.view(np.uint32).copy()
        iv = info.view(fec.PKT_INFO_DTYPE).reshape(max_packets)
        for t, c, ack_only, la, lio, delay, nr, rows in writes:
            if ack_only:
                info[t] = 0
                conn[t] = c
            iv["flags"][t] |= 0x80
            iv["largest_acked"][t], iv["largest_in_order"][t], iv["delay_us"][t], iv["n_ranges"][t] = la, lio, delay, nr
            for k, (a, b) in enumerate(rows):
                ranges[t, k] = (a, b)
        for name, got, exp in (("info", dinfo.cpu().numpy(), info),
                               ("ranges", dranges.cpu().numpy().view(np.uint64), ranges),
                               ("conn_of", dconn.cpu().numpy().view(np.uint32), conn)):
            bad = np.argwhere(got != exp)
            assert bad.size == 0, f"attach's {name} differs at {bad[:8].tolist()} (of {len(bad)})"
        got_att = datt.cpu().numpy()
        assert got_att.tolist() == attached, (np.flatnonzero(got_att != np.asarray(attached, np.uint8))[:8],)
        assert int(dout.cpu().numpy()[0]) == total_out, (int(dout.cpu().numpy()[0]), total_out)
        assert np.array_equal(dfirst.cpu().numpy(), _i64(first))
        assert dcount.cpu().numpy().view(np.uint32).tolist() == list(counts)
        if not alias_total:
            assert int(dtotal.cpu().numpy()[0]) == total
        if may is not None:
            assert dmay.cpu().numpy().tolist() == list(may)
        return writes, iv, ranges, conn, total_out, attached
