"""The whole chain of a batch on the device beside the composed rule of
tests/chain_ref.py; test infrastructure only.

ChainHarness owns one side of a link: a member per connection in each of the
four sets, their controllers and the loop, run in THE ORDER of
include/ugo_loop.h, and a RuleEndpoint that ran the same batch first.  After
every call of a batch the call's outputs are copied back and compared whole
with the rule's; after the last call of a batch the records of all six sets
are compared field by field.  What a later stage reads stays on the device
between the calls: the copies are for comparing only.  ServerHarness puts a
connection table in front and rebuilds the sets as members come and go.

A difference is reported as the call, the array and the first differing index
with both values.
"""
import numpy as np
import torch

import chain_ref as ch
from ugo_amd import fec

NO_CONN = ch.NO_CONN
M64 = ch.M64
_FILL64 = int.from_bytes(bytes([ch.SENTINEL]) * 8, "little", signed=True)


def _np(t):
    if not t.is_cuda:                           # pinned: nothing has waited for the call that wrote it yet
        torch.cuda.synchronize()
    return t.cpu().numpy()


def differ(call, name, got, want):
    """Whole-array equality, or the call, the array and the first difference."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{call}: {name} has shape {got.shape}, the rule's {want.shape}"
    if got.dtype != want.dtype:
        got, want = got.astype(np.uint64), want.astype(np.uint64)
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{call}: {name} differs at {at if len(at) > 1 else at[0]} (of {len(bad)} places): "
                             f"device {got[at]!r}, rule {want[at]!r}")


def compare_states(call, name, got, want):
    """got: a structured array of records; want: a list of dicts of the fields compared."""
    assert got.shape == (len(want),), (call, name, got.shape, len(want))
    for k in (want[0] if want else ()):
        exp = np.asarray([int(w[k]) & M64 for w in want], np.uint64)
        differ(call, f"{name} record field {k}", got[k].astype(np.uint64), exp)
    if "reserved" in (got.dtype.names or ()):
        assert not got["reserved"].any(), f"{call}: {name} records have reserved bytes set"


class ChainHarness:
    def __init__(self, enc, n, now, max_ranges, max_packets, max_exits=None, max_budget=8, max_entries=64,
                 where="device", **loop_params):
        self.enc, self.where = enc, where
        self.rule = ch.RuleEndpoint(n, now, max_ranges, max_packets, max_exits=max_exits, max_budget=max_budget,
                                    max_entries=max_entries, **loop_params)
        self.loop_params = loop_params
        self.pad = torch.from_numpy(ch.pad_bytes()).cuda()
        self.rx = [fec.StreamRx(enc, ch.RX_CAP) for _ in range(n)]
        self.ack = [fec.AckRx(enc, ch.ACK_WP) for _ in range(n)]
        self.tx = [fec.StreamTx(enc, ch.TX_CAP, ch.RQ_CAP) for _ in range(n)]
        self.sent = [fec.SentTx(enc, ch.SENT_WS, ch.MS) for _ in range(n)]
        self.sets = None
        self._build_sets(now)
        r = self.rule
        dev = torch.device("cuda")
        self.plan = (torch.zeros((r.NP, 64), dtype=torch.uint8, device=dev),
                     torch.zeros((r.NP, r.MSEG, 16), dtype=torch.uint8, device=dev),
                     self._host_visible(r.NP, torch.int32))
        self.ranges = torch.zeros((r.NP, r.MR, 2), dtype=torch.int64, device=dev)
        self.compare_all("create")

    # ---------------------------------------------------------------- plumbing
    def _host_visible(self, count, dtype):
        """The arrays a host reads (conn_of, sizes, the deadline, n_exits): pinned where the caller asks for it."""
        t = torch.zeros(count, dtype=dtype)
        return t.pin_memory() if self.where == "pinned" else t.cuda()

    def _build_sets(self, now):
        enc, n = self.enc, len(self.rx)
        self.n = n
        self.rset, self.aset = fec.StreamRxSet(enc, self.rx), fec.AckRxSet(enc, self.ack)
        self.tset, self.sset = fec.StreamTxSet(enc, self.tx), fec.SentTxSet(enc, self.sent)
        self.cc = fec.CcSet(enc, self.sset)
        self.loop = fec.LoopSet(enc, self.rset, self.aset, self.tset, self.sset, now_us=now, **self.loop_params)
        self.sets = (self.loop, self.cc, self.rset, self.aset, self.tset, self.sset)
        dev = torch.device("cuda")
        self.budget = self.cc.rto(torch.zeros(n, dtype=torch.uint8, device=dev), ch.PKT_BYTES, self.rule.max_budget)
        differ("create", "budget", _np(self.budget).view(np.uint32), np.asarray(self.rule.budget, np.uint32))
        self.delays = torch.zeros(n, dtype=torch.int64, device=dev)
        self.split = self.cc.cutback()
        self.want = torch.full((n,), ch.WANT, dtype=torch.int64, device=dev)
        self.dst = torch.zeros(n * ch.WANT, dtype=torch.uint8, device=dev)
        self.dst_off = torch.arange(n, dtype=torch.int64, device=dev) * ch.WANT
        self.first = torch.zeros(n, dtype=torch.int64, device=dev)
        self.count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.total = self._host_visible(1, torch.int64)
        self.total_out = self._host_visible(1, torch.int64)

    def _close_sets(self):
        for x in self.sets:
            x.close()
        self.sets = None

    def close(self):
        if self.sets:
            self._close_sets()
        for x in self.rx + self.ack + self.tx + self.sent:
            x.close()
        self.rx = self.ack = self.tx = self.sent = []

    def rebuild(self, keep, n_new, now):
        """The sets over a new member list (RuleEndpoint.rebuild): the survivors'
        per-connection objects carry on, the others are closed."""
        self._close_sets()
        kept = {k for k in keep if k is not None}

        def relist(old, make):
            for k, x in enumerate(old):
                if k not in kept:
                    x.close()
            return [old[k] if k is not None else make() for k in keep]

        enc = self.enc
        self.rx = relist(self.rx, lambda: fec.StreamRx(enc, ch.RX_CAP))
        self.ack = relist(self.ack, lambda: fec.AckRx(enc, ch.ACK_WP))
        self.tx = relist(self.tx, lambda: fec.StreamTx(enc, ch.TX_CAP, ch.RQ_CAP))
        self.sent = relist(self.sent, lambda: fec.SentTx(enc, ch.SENT_WS, ch.MS))
        self.rule.rebuild(keep, n_new, now)
        self._build_sets(now)
        self.compare_all("rebuild")

    eof = property(lambda self: self.rule.eof)
    exits = property(lambda self: self.rule.exits)
    deadline = property(lambda self: self.rule.deadline)
    got = property(lambda self: self.rule.got)

    # ---------------------------------------------------------------- the records of all six sets
    def compare_all(self, call):
        want = self.rule.states()
        compare_states(call, "stream_rx", self.rset.states(), want["stream_rx"])
        compare_states(call, "ack", self.aset.states(), want["ack"])
        compare_states(call, "stream_tx", self.tset.states(), want["stream_tx"])
        compare_states(call, "sent", self.sset.states(), want["sent"])
        cc = self.cc.states()
        compare_states(call, "cc", cc, want["cc"])
        differ(call, "the dense cutback array", _np(self.cc.cutback()).view(np.uint64), cc["cutback"])
        compare_states(call, "loop", self.loop.states(), want["loop"])

    # ---------------------------------------------------------------- between batches
    def write(self, chunks):
        want = self.rule.write(chunks)
        sizes = [len(c) for c in chunks]
        src = torch.from_numpy(np.frombuffer(b"".join(bytes(c) for c in chunks) or b"\0", np.uint8).copy()).cuda()
        off = torch.tensor(np.cumsum([0] + sizes[:-1]), dtype=torch.int64, device="cuda")
        got = self.tset.write(src, off, torch.tensor(sizes, dtype=torch.int64, device="cuda"))
        differ("stream_tx_set_write", "n_written", _np(got).view(np.uint64), ch._u64(want))
        return want

    def close_members(self, how, linger_us, now):
        self.rule.close_members(how, linger_us, now)
        dh = torch.tensor(how, dtype=torch.uint8, device="cuda")
        dl = None if linger_us is None else torch.tensor(linger_us, dtype=torch.int64, device="cuda")
        self.loop.close_members(dh, now, linger_us=dl)

    # ---------------------------------------------------------------- the send half
    def send(self, now):
        R = self.rule.send(now)
        want = dict(R["calls"])
        r, n = self.rule, self.n
        info, segs, conn = self.plan
        may = self.loop.check(now, self.budget)
        w = want["loop_set_check"]
        differ("loop_set_check", "budget", _np(self.budget).view(np.uint32), w["budget"])
        differ("loop_set_check", "may_ack_only", _np(may), w["may_ack_only"])
        self.tset.plan(self.budget, r.NP, max_payload=ch.PAYLOAD, max_segments=r.MSEG,
                       out=(info, segs, conn, self.first, self.count, self.total))
        w = want["stream_tx_set_plan"]
        call = "stream_tx_set_plan"
        differ(call, "first", _np(self.first).view(np.uint64), w["first"])
        differ(call, "count", _np(self.count).view(np.uint32), w["count"])
        differ(call, "total", _np(self.total).view(np.uint64), ch._u64([w["total"]]))
        self._planned(call, w)
        appended = torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.loop.append(self.total, info, segs, conn, appended=appended)       # total_out is total itself
        w = want["loop_set_append"]
        call = "loop_set_append"
        differ(call, "total_out", _np(self.total).view(np.uint64), ch._u64([w["total_out"]]))
        differ(call, "appended", _np(appended), w["appended"])
        self._planned(call, w)
        _, attached = self.aset.attach(now, self.first, self.count, self.total, info, self.ranges, conn,
                                       may_ack_only=may, total_out=self.total_out)
        w = want["ack_set_attach"]
        call = "ack_set_attach"
        differ(call, "total_out", _np(self.total_out).view(np.uint64), ch._u64([w["total_out"]]))
        differ(call, "attached", _np(attached), w["attached"])
        differ(call, "ranges", _np(self.ranges).view(np.uint64), w["ranges"])
        self._planned(call, w)
        sw = self.sset.attach(self.first, self.count, info)
        w = want["sent_set_attach"]
        differ("sent_set_attach", "attached", _np(sw), w["attached"])
        differ("sent_set_attach", "info", _np(info), w["info"])
        npk = int(self.total_out.item())                                        # a size
        assert npk == R["npk"]
        wire = lens = None
        if npk:
            wire, lens, st = self.tset.encode(info, self.ranges, segs, conn, ch.SLOT, npackets=npk, pad=self.pad)
            w = want["stream_tx_set_encode"]
            call = "stream_tx_set_encode"
            differ(call, "status", _np(st), w["status"])
            differ(call, "wire_lens", _np(lens).view(np.uint16), w["wire_lens"])
            differ(call, "wire", _np(wire), w["wire"])          # every slot whole: zeros past round_up(len, 16)
            self.sset.record(info, segs, conn, lens, st, now, npackets=npk)
        cap = r.max_exits
        out = (self._host_visible(1, torch.int64), torch.zeros(cap, dtype=torch.int32, device="cuda"),
               torch.zeros(cap, dtype=torch.uint8, device="cuda"), self._host_visible(1, torch.int64),
               torch.zeros(n, dtype=torch.int32, device="cuda"), self._host_visible(1, torch.int64))
        self.loop.sent(self.count, attached, now, delay_us=self.delays, max_exits=cap, out=out)
        w = want["loop_set_sent"]
        call = "loop_set_sent"
        k = len(w["exits"])
        exits, reasons = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
        exits[:k], reasons[:k] = w["exits"], w["reasons"]
        differ(call, "deadline_us", _np(out[0]).view(np.uint64), ch._u64([w["deadline_us"]]))
        differ(call, "exits", _np(out[1]).view(np.uint32), exits)
        differ(call, "reasons", _np(out[2]), reasons)
        differ(call, "n_exits", _np(out[3]).view(np.uint64), ch._u64([w["n_exits"]]))
        differ(call, "new_index", _np(out[4]).view(np.uint32), w["new_index"])
        differ(call, "nconn_new", _np(out[5]).view(np.uint64), ch._u64([w["nconn_new"]]))
        self.compare_all("after loop_set_sent")
        R["_dev"] = (wire, lens, conn, out[4])
        return R

    def _planned(self, call, w):
        info, segs, conn = self.plan
        differ(call, "info", _np(info), w["info"])
        differ(call, "segs", _np(segs), w["segs"])
        differ(call, "conn_of", _np(conn).view(np.uint32), w["conn_of"])

    # ---------------------------------------------------------------- the receive half
    def stage(self, batch):
        """The device's own wire of the rows the link kept, a forged row where
        the link put one.  Returns (wire, lens, conn_of) for the batch."""
        dwire, dlens, dconn, _ = batch["sender"]["_dev"]
        idx = torch.from_numpy(batch["src"])
        wire, lens = dwire[idx.cuda()].contiguous(), dlens[idx.cuda()].contiguous()
        for k in batch["forged"]:
            wire[k] = torch.from_numpy(batch["wire"][k]).cuda()
            lens[k] = int(batch["lens"][k])
        conn = dconn[idx.to(dconn.device)].contiguous()
        return wire, lens, conn

    def receive(self, batch, now, staged=None):
        """staged: (wire, lens, conn_of) on the device where a listener routed
        the ring; else the link's rows of the sender's wire."""
        r, n = self.rule, self.n
        npk = batch["npk"]
        conn_np = None
        if staged is not None:
            wire, lens, conn = staged
            conn_np = _np(conn).view(np.uint32)
        elif npk:
            wire, lens, conn = self.stage(batch)
            if self.where == "pinned":
                conn = conn.cpu().pin_memory()
        R = r.receive(batch, now, conn_of=conn_np)
        want = dict(R["calls"])
        if npk:
            R_, S_ = max(r.MR, 1), max(r.MSEG, 1)
            out = (torch.full((npk, 64), ch.SENTINEL, dtype=torch.uint8, device="cuda"),
                   torch.full((npk, R_, 2), _FILL64, dtype=torch.int64, device="cuda"),
                   torch.full((npk, S_, 16), ch.SENTINEL, dtype=torch.uint8, device="cuda"))
            info, ranges, segs = self.enc.packet_decode(wire, lens, pad=self.pad, max_ranges=r.MR, max_segments=r.MSEG,
                                                        out=out)
            w = want["packet_decode"]
            call = "packet_decode"
            ok = ~w["failed"]
            gi = _np(info)
            differ(call, "info of the packets that decoded", gi[ok], w["info"][ok])
            for f in ("status", "payload_off", "fec_flag_lo", "reserved"):     # all a failed packet's record defines
                differ(call, f"info field {f} of the packets that failed", ch._iv(gi.copy())[f][~ok],
                       ch._iv(w["info"].copy())[f][~ok])
            differ(call, "ranges", _np(ranges).view(np.uint64)[ok], w["ranges"][ok])
            differ(call, "segs", _np(segs)[ok], w["segs"][ok])
            self.loop.receive(info, conn, now)
            differ("loop_set_receive", "conn_of", _np(conn).view(np.uint32), want["loop_set_receive"]["conn_of"])
            seg_status = torch.full((npk, r.MSEG), 0x77, dtype=torch.uint8, device="cuda")
            self.rset.deliver(wire, info, segs, conn, pad=self.pad, out=seg_status)
            differ("stream_set_deliver", "seg_status", _np(seg_status), want["stream_set_deliver"]["seg_status"])
            self.aset.receive(info, conn, now, seg_status=seg_status)
            n_read, eof = self.rset.read(self.want, self.dst, self.dst_off)
            w = want["stream_set_read"]
            call = "stream_set_read"
            differ(call, "n_read", _np(n_read).view(np.uint64), w["n_read"])
            differ(call, "eof", _np(eof), w["eof"])
            dst = _np(self.dst)
            for c, d in enumerate(w["data"]):
                differ(call, f"the bytes read of member {c}", dst[c * ch.WANT:c * ch.WANT + len(d)],
                       np.frombuffer(d, np.uint8))
            events, rows = self.cc.sent_ack(info, ranges, conn, now, npackets=npk, split=self.split)
            w = want["cc_sent_ack"]
            differ("cc_sent_ack", "events", _np(events), w["events"].view(np.uint8).reshape(n, 64))
            differ("cc_sent_ack", "rows", _np(rows), w["rows"].view(np.uint8).reshape(n, 32))
            self.delays = self.cc.ack(events, rows, now)
            differ("cc_set_ack", "delay_us", _np(self.delays).view(np.uint64), want["cc_set_ack"]["delay_us"])
        fired = self.sset.rto(self.delays, now)
        differ("sent_set_rto", "fired", _np(fired), want["sent_set_rto"]["fired"])
        self.budget = self.cc.rto(fired, ch.PKT_BYTES, r.max_budget)
        differ("cc_set_rto", "budget", _np(self.budget).view(np.uint32), want["cc_set_rto"]["budget"])
        E = r.max_entries
        dev = torch.device("cuda")
        dout = (torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int64, device=dev),
                torch.zeros(E, dtype=torch.int32, device=dev), self._host_visible(1, torch.int64),
                torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))
        rc, ro, rlen, n_entries, touch, upto = self.sset.drain(E, out=dout)
        w = want["sent_set_drain"]
        call = "sent_set_drain"
        differ(call, "conn_of", _np(rc).view(np.uint32), w["conn_of"])
        differ(call, "offset", _np(ro).view(np.uint64), w["offset"])
        differ(call, "len", _np(rlen).view(np.uint32), w["len"])
        differ(call, "n_entries", _np(n_entries).view(np.uint64), ch._u64([w["n_entries"]]))
        differ(call, "touch", _np(touch), w["touch"])
        differ(call, "upto", _np(upto).view(np.uint64), w["upto"])
        status = self.tset.retransmit(rc, ro, rlen)
        differ("stream_tx_set_retransmit", "status", _np(status), want["stream_tx_set_retransmit"]["status"])
        self.aset.touch(touch)
        self.tset.release(upto)
        self.compare_all("after stream_tx_set_release")
        return R


class ServerHarness:
    """A ListenTable and a ChainHarness behind it, beside chain_ref.RuleServer."""

    def __init__(self, enc, max_conn, now, max_ranges, max_packets, **kw):
        self.enc, self.max_conn, self.kw = enc, max_conn, dict(max_ranges=max_ranges, max_packets=max_packets, **kw)
        self.rule = ch.RuleServer(max_conn, now, max_ranges, max_packets, **kw)
        self.table = fec.ListenTable(enc, max_conn)
        self.end = None

    def close(self):
        if self.end is not None:
            self.end.close()
        self.table.close()

    def compare_table(self, call):
        st, w = self.table.state(), self.rule.listener_state()
        for k in ("nconn", "n_dead", "n_slots", "err"):
            assert int(st[k]) == w[k], f"{call}: the table's {k} is {int(st[k])}, the rule's {w[k]}"
        differ(call, "the table's counts", st["counts"], np.asarray(w["counts"], np.uint64))
        got = self.table.entries()
        exp = np.zeros(len(w["entries"]), fec.LISTEN_ENTRY_DTYPE)
        for j, (ip, scope, port, member) in enumerate(w["entries"]):
            exp[j]["ip"] = np.frombuffer(ip, np.uint8)
            exp[j]["scope"], exp[j]["port"], exp[j]["member"] = scope, port, member
        assert len(got) == len(exp), f"{call}: {len(got)} entries, the rule has {len(exp)}"
        for k in ("ip", "scope", "port", "member", "reserved"):
            differ(call, f"entry field {k}", got[k], exp[k])

    def route(self, names, pkts, lens, now):
        """names uint8 [npk, 32], pkts uint8 [npk, SLOT], lens uint16 [npk] (numpy).
        Returns (wire, lens, conn_of) on the device for ChainHarness.receive."""
        npk = len(pkts)
        dn, dp = torch.from_numpy(names).cuda(), torch.from_numpy(pkts).cuda()
        dl = torch.from_numpy(lens.view(np.int16)).cuda()
        cap = min(npk, self.max_conn)
        acc = torch.full((cap, 48), 0x77, dtype=torch.uint8, device="cuda")
        conn_of, cls, acc, n_acc = self.table.route(dn, dp, dl, accepted=acc)
        had = self.rule.end
        (call, w), n_new, _ = self.rule.route(names, pkts, lens, now)
        differ(call, "conn_of", _np(conn_of).view(np.uint32), w["conn_of"])
        differ(call, "cls", _np(cls), w["cls"])
        assert int(n_acc.item()) == w["n_accepted"], f"{call}: n_accepted {int(n_acc.item())}, the rule's {n_new}"
        got = _np(acc)
        differ(call, "accepted", got[:n_new], w["accepted"].view(np.uint8).reshape(n_new, 48))
        assert (got[n_new:] == 0x77).all(), f"{call}: accepted[] was written past the rows the call accepted"
        self.compare_table(call)
        if n_new:                                 # the host's share: the new members and the sets over the longer list
            if self.end is None:
                self.end = ChainHarness(self.enc, n_new, now, **self.kw)
                self.end.rule = self.rule.end
                self.end.compare_all("create")
            else:
                old = self.end.n
                self._rebuild(list(range(old)) + [None] * n_new, old + n_new, now, rule_done=had is not None)
        return dp, dl, conn_of

    def _rebuild(self, keep, n_new, now, rule_done):
        """ChainHarness.rebuild where the RuleServer has rebuilt its endpoint already."""
        end = self.end
        if n_new == 0:                            # a set has a member at least
            end.close()
            self.end = None
            return
        if rule_done:
            redo = end.rule.rebuild
            end.rule.rebuild = lambda *a: None
            try:
                end.rebuild(keep, n_new, now)
            finally:
                end.rule.rebuild = redo
        else:
            end.rebuild(keep, n_new, now)

    def remap(self, dev_new_index, new_index, nconn_new, now):
        call, w = self.rule.remap(new_index, nconn_new, now)
        status = self.table.remap(dev_new_index, nconn_new)
        assert int(status.item()) == w["status"], f"{call}: status {int(status.item())}"
        self.compare_table(call)
        keep = [None] * nconn_new
        for old, new in enumerate(new_index):
            if new != NO_CONN:
                keep[new] = old
        self._rebuild(keep, nconn_new, now, rule_done=True)
