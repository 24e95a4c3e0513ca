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

defer=True holds the chain to stream order on a stream that is behind its
host: no copy follows a call; a comparison becomes a record (call, name, a
clone enqueued on the current stream, view, want) and _flush() synchronises the
stream once, where the host needs a value or a set's records, and runs the
records in order with the same messages.  delay() -- see behind() -- is called
at the head of every run of calls that has no host wait inside it.
"""
import time

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


def calibrate_sleep(target_s=2e-3):
    """torch.cuda._sleep cycles per second of device-side delay, measured with
    events on the current stream: after a first call, which loads the kernel,
    over a delay long enough for the launch not to count."""
    torch.cuda._sleep(1 << 16)
    torch.cuda.current_stream().synchronize()
    cycles = 1 << 18
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        took = a.elapsed_time(b) * 1e-3
        if took >= target_s:
            return cycles / took
        cycles *= 4
    raise AssertionError(f"torch.cuda._sleep({cycles}) took {took} s: it does not delay the stream")


class behind:
    """delay = behind(stream, seconds, cycles_per_s): delay() enqueues a device-side
    delay of `seconds` on `stream`, so that what the host enqueues next lies
    behind it while the host runs on.  A harness appends to delay.runs, for
    every run of calls it enqueued behind a delay, (label, the host's seconds
    from the delay to the last enqueue, whether the run proved nothing).
    stream.query() False right after the last enqueue means the host was ahead
    of the device, so work that went anywhere but the stream would have
    overtaken its operands; a run proved nothing if query() was True, or if the
    enqueue took the host as long as the delay: then a call waited for the
    stream, which no call may, or the thread was preempted."""

    def __init__(self, stream, seconds, cycles_per_s):
        self.stream, self.seconds, self.cycles_per_s = stream, seconds, cycles_per_s
        self.runs, self.longest, self.last = [], seconds, seconds

    def __call__(self, seconds=0.0):
        """seconds: a longer delay for this one run."""
        assert torch.cuda.current_stream() == self.stream, "the delay belongs to the stream the calls go to"
        seconds = max(seconds, self.seconds)
        self.longest, self.last = max(self.longest, seconds), seconds
        torch.cuda._sleep(max(1, int(seconds * self.cycles_per_s)))

    def ran(self, label, enqueue_s):
        self.runs.append((label, enqueue_s, torch.cuda.current_stream().query() or enqueue_s >= self.last))

    def assert_was_behind(self):
        idle = [r for r in self.runs if r[2]]
        assert self.runs and len(idle) <= 0.05 * len(self.runs), \
            f"the stream was not behind: {len(idle)} of {len(self.runs)} runs had finished when their last call " \
            f"was enqueued, or kept the host for the whole delay ({self.seconds * 1e3:.2f} ms; the slowest such " \
            f"run, {max(idle, key=lambda r: r[1], default=('none',))[0]}, took the host " \
            f"{max((r[1] for r in idle), default=0) * 1e3:.2f} ms)"


class _Snap:
    """What a call left in a tensor, to compare several views of: a clone on the stream (defer) or the host copy."""

    def __init__(self, t, defer):
        self.t = t.clone() if defer else None
        self.host = None if defer else _np(t)


class _Comparing:
    """differ() at once, or deferred to _flush()."""

    def _comparing(self, defer, delay):
        self.defer, self.delay = defer, delay
        self._pending, self._t0 = [], None

    def _delay(self, label):
        if self.delay is not None:
            self.delay()
            self._t0 = (label, time.perf_counter())

    def _snap(self, t):
        return _Snap(t, self.defer)

    def _check(self, call, name, t, want, view=None):
        """differ(call, name, view(the tensor's bytes on the host), want), now or at the next _flush()."""
        snap = t if isinstance(t, _Snap) else _Snap(t, self.defer)
        if self.defer:
            self._pending.append((call, name, snap.t, view, want))
        else:
            differ(call, name, snap.host if view is None else view(snap.host), want)

    def _flush(self):
        if not self.defer:
            return
        if self._t0 is not None:
            label, t0 = self._t0
            self._t0 = None
            if hasattr(self.delay, "ran"):
                self.delay.ran(label, time.perf_counter() - t0)
        torch.cuda.current_stream().synchronize()
        pending, self._pending = self._pending, []
        host = {}                                   # one copy of a clone, however many views of it are compared
        for call, name, t, view, want in pending:
            if id(t) not in host:
                host[id(t)] = t.cpu().numpy()
            got = host[id(t)]
            differ(call, name, got if view is None else view(got), want)


def _u64v(a):
    return a.view(np.uint64)


def _u32v(a):
    return a.view(np.uint32)


def _u16v(a):
    return a.view(np.uint16)


class ChainHarness(_Comparing):
    def __init__(self, enc, n, now, max_ranges, max_packets, max_exits=None, max_budget=8, max_entries=64,
                 where="device", defer=False, delay=None, cc_params=None, **loop_params):
        assert not (defer and where == "pinned"), "a pinned clone is a host copy, not stream work"
        self._comparing(defer, delay)
        self.enc, self.where = enc, where
        self.cc_params = dict(cc_params or {})
        self.rule = ch.RuleEndpoint(n, now, max_ranges, max_packets, max_exits=max_exits, max_budget=max_budget,
                                    max_entries=max_entries, cc_params=cc_params, **loop_params)
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
        if self.defer:                              # no upload from pageable memory: it may wait for the stream
            return torch.zeros(count, dtype=dtype, device="cuda")
        t = torch.zeros(count, dtype=dtype)
        return t.pin_memory() if self.where == "pinned" else t.cuda()

    def _build_sets(self, now):
        enc, n = self.enc, len(self.rx)
        self.n = n
        self.rset, self.aset = fec.StreamRxSet(enc, self.rx), fec.AckRxSet(enc, self.ack)
        self.tset, self.sset = fec.StreamTxSet(enc, self.tx), fec.SentTxSet(enc, self.sent)
        self.cc = fec.CcSet(enc, self.sset, **self.cc_params)
        self.loop = fec.LoopSet(enc, self.rset, self.aset, self.tset, self.sset, now_us=now, **self.loop_params)
        self.sets = (self.loop, self.cc, self.rset, self.aset, self.tset, self.sset)
        dev = torch.device("cuda")
        self.budget = self.cc.rto(torch.zeros(n, dtype=torch.uint8, device=dev), ch.PKT_BYTES, self.rule.max_budget)
        self._check("create", "budget", self.budget, np.asarray(self.rule.budget, np.uint32), _u32v)
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
        self._flush()
        for x in self.sets:
            x.close()
        self.sets = None

    def close(self):
        self._flush()
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
        self._flush()
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
        n = torch.tensor(sizes, dtype=torch.int64, device="cuda")
        self._delay("write")                        # behind the uploads: a copy from pageable memory may wait
        got = self.tset.write(src, off, n)
        self._check("stream_tx_set_write", "n_written", got, ch._u64(want), _u64v)
        return want

    def close_members(self, how, linger_us, now):
        self.rule.close_members(how, linger_us, now)
        dh = torch.tensor(how, dtype=torch.uint8, device="cuda")
        dl = None if linger_us is None else torch.tensor(linger_us, dtype=torch.int64, device="cuda")
        self._delay("close_members")
        self.loop.close_members(dh, now, linger_us=dl)

    # ---------------------------------------------------------------- the send half
    def send(self, now):
        R = self.rule.send(now)
        want = dict(R["calls"])
        r, n = self.rule, self.n
        info, segs, conn = self.plan
        self._delay("send: loop_set_check .. sent_set_attach")
        may = self.loop.check(now, self.budget)
        w = want["loop_set_check"]
        self._check("loop_set_check", "budget", self.budget, w["budget"], _u32v)
        self._check("loop_set_check", "may_ack_only", may, w["may_ack_only"])
        self.tset.plan(self.budget, r.NP, max_payload=ch.PAYLOAD, max_segments=r.MSEG,
                       out=(info, segs, conn, self.first, self.count, self.total))
        w = want["stream_tx_set_plan"]
        call = "stream_tx_set_plan"
        self._check(call, "first", self.first, w["first"], _u64v)
        self._check(call, "count", self.count, w["count"], _u32v)
        self._check(call, "total", self.total, ch._u64([w["total"]]), _u64v)
        self._planned(call, w)
        appended = torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.loop.append(self.total, info, segs, conn, appended=appended)       # total_out is total itself
        w = want["loop_set_append"]
        call = "loop_set_append"
        self._check(call, "total_out", self.total, ch._u64([w["total_out"]]), _u64v)
        self._check(call, "appended", appended, w["appended"])
        self._planned(call, w)
        _, attached = self.aset.attach(now, self.first, self.count, self.total, info, self.ranges, conn,
                                       may_ack_only=may, total_out=self.total_out)
        w = want["ack_set_attach"]
        call = "ack_set_attach"
        self._check(call, "total_out", self.total_out, ch._u64([w["total_out"]]), _u64v)
        self._check(call, "attached", attached, w["attached"])
        self._check(call, "ranges", self.ranges, w["ranges"], _u64v)
        self._planned(call, w)
        sw = self.sset.attach(self.first, self.count, info)
        w = want["sent_set_attach"]
        self._check("sent_set_attach", "attached", sw, w["attached"])
        self._check("sent_set_attach", "info", info, w["info"])
        self._flush()
        npk = int(self.total_out.item())                                        # a size
        assert npk == R["npk"]
        self._delay("send: set_encode .. loop_set_sent")
        wire = lens = None
        if npk:
            wire, lens, st = self.tset.encode(info, self.ranges, segs, conn, ch.SLOT, npackets=npk, pad=self.pad)
            w = want["stream_tx_set_encode"]
            call = "stream_tx_set_encode"
            self._check(call, "status", st, w["status"])
            self._check(call, "wire_lens", lens, w["wire_lens"], _u16v)
            self._check(call, "wire", wire, w["wire"])          # every slot whole: zeros past round_up(len, 16)
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
        self._check(call, "deadline_us", out[0], ch._u64([w["deadline_us"]]), _u64v)
        self._check(call, "exits", out[1], exits, _u32v)
        self._check(call, "reasons", out[2], reasons)
        self._check(call, "n_exits", out[3], ch._u64([w["n_exits"]]), _u64v)
        self._check(call, "new_index", out[4], w["new_index"], _u32v)
        self._check(call, "nconn_new", out[5], ch._u64([w["nconn_new"]]), _u64v)
        self.compare_all("after loop_set_sent")
        R["_dev"] = (wire, lens, conn, out[4])
        return R

    def _planned(self, call, w):
        info, segs, conn = self.plan
        self._check(call, "info", info, w["info"])
        self._check(call, "segs", segs, w["segs"])
        self._check(call, "conn_of", conn, w["conn_of"], _u32v)

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
            self._flush()
            conn_np = _np(conn).view(np.uint32)
        elif npk:
            wire, lens, conn = self.stage(batch)
            if self.where == "pinned":
                conn = conn.cpu().pin_memory()
        R = r.receive(batch, now, conn_of=conn_np)
        want = dict(R["calls"])
        self._delay("receive" if npk else "receive: no packets")       # behind stage()'s uploads
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
            gi = self._snap(info)
            self._check(call, "info of the packets that decoded", gi, w["info"][ok], lambda a: a[ok])
            for f in ("status", "payload_off", "fec_flag_lo", "reserved"):     # all a failed packet's record defines
                self._check(call, f"info field {f} of the packets that failed", gi, ch._iv(w["info"].copy())[f][~ok],
                            lambda a, f=f: ch._iv(a.copy())[f][~ok])
            self._check(call, "ranges", ranges, w["ranges"][ok], lambda a: a.view(np.uint64)[ok])
            self._check(call, "segs", segs, w["segs"][ok], lambda a: a[ok])
            self.loop.receive(info, conn, now)
            self._check("loop_set_receive", "conn_of", conn, want["loop_set_receive"]["conn_of"], _u32v)
            seg_status = torch.full((npk, r.MSEG), 0x77, dtype=torch.uint8, device="cuda")
            self.rset.deliver(wire, info, segs, conn, pad=self.pad, out=seg_status)
            self._check("stream_set_deliver", "seg_status", seg_status, want["stream_set_deliver"]["seg_status"])
            self.aset.receive(info, conn, now, seg_status=seg_status)
            n_read, eof = self.rset.read(self.want, self.dst, self.dst_off)
            w = want["stream_set_read"]
            call = "stream_set_read"
            self._check(call, "n_read", n_read, w["n_read"], _u64v)
            self._check(call, "eof", eof, w["eof"])
            dst = self._snap(self.dst)
            for c, d in enumerate(w["data"]):
                self._check(call, f"the bytes read of member {c}", dst, np.frombuffer(d, np.uint8),
                            lambda a, c=c, k=len(d): a[c * ch.WANT:c * ch.WANT + k])
            events, rows = self.cc.sent_ack(info, ranges, conn, now, npackets=npk, split=self.split)
            w = want["cc_sent_ack"]
            self._check("cc_sent_ack", "events", events, w["events"].view(np.uint8).reshape(n, 64))
            self._check("cc_sent_ack", "rows", rows, w["rows"].view(np.uint8).reshape(n, 32))
            self.delays = self.cc.ack(events, rows, now)
            self._check("cc_set_ack", "delay_us", self.delays, want["cc_set_ack"]["delay_us"], _u64v)
        fired = self.sset.rto(self.delays, now)
        self._check("sent_set_rto", "fired", fired, want["sent_set_rto"]["fired"])
        self.budget = self.cc.rto(fired, ch.PKT_BYTES, r.max_budget)
        self._check("cc_set_rto", "budget", self.budget, want["cc_set_rto"]["budget"], _u32v)
        E = r.max_entries
        dev = torch.device("cuda")
        dout = (torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int64, device=dev),
                torch.zeros(E, dtype=torch.int32, device=dev), self._host_visible(1, torch.int64),
                torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))
        rc, ro, rlen, n_entries, touch, upto = self.sset.drain(E, out=dout)
        w = want["sent_set_drain"]
        call = "sent_set_drain"
        self._check(call, "conn_of", rc, w["conn_of"], _u32v)
        self._check(call, "offset", ro, w["offset"], _u64v)
        self._check(call, "len", rlen, w["len"], _u32v)
        self._check(call, "n_entries", n_entries, ch._u64([w["n_entries"]]), _u64v)
        self._check(call, "touch", touch, w["touch"])
        self._check(call, "upto", upto, w["upto"], _u64v)
        status = self.tset.retransmit(rc, ro, rlen)
        self._check("stream_tx_set_retransmit", "status", status, want["stream_tx_set_retransmit"]["status"])
        self.aset.touch(touch)
        self.tset.release(upto)
        self.compare_all("after stream_tx_set_release")
        return R


class ServerHarness(_Comparing):
    """A ListenTable and a ChainHarness behind it, beside chain_ref.RuleServer."""

    def __init__(self, enc, max_conn, now, max_ranges, max_packets, defer=False, delay=None, **kw):
        self._comparing(defer, delay)
        self.enc, self.max_conn = enc, max_conn
        self.kw = dict(max_ranges=max_ranges, max_packets=max_packets, defer=defer, delay=delay, **kw)
        self.rule = ch.RuleServer(max_conn, now, max_ranges, max_packets, **kw)
        self.table = fec.ListenTable(enc, max_conn)
        self.end = None

    def close(self):
        self._flush()
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
        self._delay("listen_route")                 # behind the uploads
        acc = torch.full((cap, 48), 0x77, dtype=torch.uint8, device="cuda")
        conn_of, cls, acc, n_acc = self.table.route(dn, dp, dl, accepted=acc)
        had = self.rule.end
        (call, w), n_new, _ = self.rule.route(names, pkts, lens, now)
        self._check(call, "conn_of", conn_of, w["conn_of"], _u32v)
        self._check(call, "cls", cls, w["cls"])
        self._flush()
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
        self._delay("listen_remap")
        status = self.table.remap(dev_new_index, nconn_new)
        self._flush()
        assert int(status.item()) == w["status"], f"{call}: status {int(status.item())}"
        self.compare_table(call)
        keep = [None] * nconn_new
        for old, new in enumerate(new_index):
            if new != NO_CONN:
                keep[new] = old
        self._rebuild(keep, nconn_new, now, rule_done=True)
