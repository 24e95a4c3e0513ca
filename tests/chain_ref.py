"""The composed rule: the whole chain of a batch on the CPU; test infrastructure
only, runnable without a GPU.

RuleEndpoint  one side of a link: n members, each made of the rules of the
              stages (stream_ref.RuleRx, ack_ref.RuleAck, stream_tx_ref.RuleTx,
              sent_ref.RuleSent, cc_ref.RuleCc, loop_ref.RuleLoop), run in THE
              ORDER of include/ugo_loop.h through the set-level functions of
              those modules.  send() and receive() return every array a call of
              the chain writes, keyed by the name of the device array it stands
              for, one entry per call.  The planned records become wire bytes
              through oracle/packet_ref.py's encoder, and arriving bytes become
              records through its decoder: no code under test produces what the
              device is held against.
RuleServer    a RuleEndpoint behind a listen_ref.RuleListener.
script        a seeded life for a pair of endpoints; link() is the lossy link
              between them and run_pair() the driver, for any two objects with
              RuleEndpoint's methods.
"""
import hashlib
import random
import types

import numpy as np

import ack_ref as ar
import cc_ref as cr
import listen_ref as lr
import loop_ref as lf
import packet_ref as pr
import sent_ref as sr
import stream_ref as rr
import stream_tx_ref as tr
from packet_vectors import keystream
from ugo_amd import fec

NO_CONN = 0xffffffff
M64 = (1 << 64) - 1
SLOT, MS, PAYLOAD, PKT_BYTES = 1488, 2, 1436, 1470
RX_CAP = TX_CAP = 32768
RQ_CAP, ACK_WP, SENT_WS = 64, 1024, 1024
WANT = 1 << 16                                  # bytes a read asks of every member
SENTINEL = 0xA5                                 # what packet_decode's outputs hold before the call
START_US, STEP_US = 1_000_000, 20_000
I_T, S_T = fec.PKT_INFO_DTYPE, fec.PKT_SEGMENT_DTYPE


def pad_bytes():
    return keystream(SLOT).copy()


def _iv(info):
    return info.view(I_T).reshape(-1)


def _sv(segs):
    n, ms = segs.shape[:2]
    return segs.reshape(n, ms * 16).view(S_T).reshape(n, ms)


def decode_expect(raws, max_ranges, max_segments):
    """packet_decode of the plain packets `raws` over outputs filled with
    SENTINEL.  Returns (info uint8 [n, 64], ranges uint64 [n, R, 2], segs uint8
    [n, S, 16], failed bool [n]); of a packet that failed only status,
    payload_off, fec_flag_lo and reserved are defined (include/ugo_pkt.h)."""
    n, R, S = len(raws), max(max_ranges, 1), max(max_segments, 1)
    info = np.full((n, 64), SENTINEL, np.uint8)
    ranges = np.full((n, R, 2), int.from_bytes(bytes([SENTINEL]) * 8, "little"), np.uint64)
    segs = np.full((n, S, 16), SENTINEL, np.uint8)
    failed = np.zeros(n, bool)
    iv, sv = _iv(info), _sv(segs)
    for i, b in enumerate(raws):
        st, out = pr.decode(b)
        rec = np.zeros(1, I_T)
        if st != pr.PKT_OK:
            rec["status"], failed[i] = st, True
            iv[i] = rec[0]
            continue
        rec["flags"], rec["packet_number"] = out["flags"], out["packet_number"]
        rec["stop_waiting"] = out["stop_waiting"]
        rg = []
        if out["sack"] is not None:
            s = out["sack"]
            rec["largest_acked"], rec["largest_in_order"], rec["delay_us"] = \
                s["largest_acked"], s["largest_in_order"], s["delay_us"]
            rg = s["ranges"]
        sg = out["segments"]
        if len(rg) > max_ranges or len(sg) > max_segments:
            rec["status"] = fec.PKT_CAPACITY
        nr, ns = min(len(rg), max_ranges), min(len(sg), max_segments)
        rec["n_ranges"], rec["n_segments"] = nr, ns
        iv[i] = rec[0]
        for k in range(nr):
            ranges[i, k] = rg[k]
        for j in range(ns):
            sv[i, j] = sg[j]
    return info, ranges, segs, failed


def event_array(events):
    out = np.zeros(len(events), fec.SENT_EVENT_DTYPE)
    for k in sr.RuleSent.EVENT_FIELDS:
        out[k] = [e[k] & M64 for e in events]
    return out


def row_array(rows):
    out = np.zeros(len(rows), fec.CC_ROW_DTYPE)
    for k in cr.RuleCc.ROW_FIELDS:
        out[k] = [r[k] for r in rows]
    return out


def _u64(values):
    return np.asarray([int(v) & M64 for v in values], np.uint64)


class RuleEndpoint:
    def __init__(self, n, now, max_ranges, max_packets, max_segments=MS, max_exits=None, max_budget=8,
                 max_entries=64, cc_params=None, **loop_params):
        self.n, self.MR, self.NP, self.MSEG = n, max_ranges, max_packets, max_segments
        self.cc_params = dict(cc_params or {})            # the congestion controllers'; none: the defaults
        self.max_exits = n if max_exits is None else max_exits
        self.max_budget, self.max_entries, self.loop_params = max_budget, max_entries, loop_params
        self.pad = pad_bytes()
        self.rx = [rr.RuleRx(RX_CAP) for _ in range(n)]
        self.ack = [ar.RuleAck(ACK_WP) for _ in range(n)]
        self.tx = [tr.RuleTx(TX_CAP, RQ_CAP) for _ in range(n)]
        self.sent = [sr.RuleSent(SENT_WS, max_segments) for _ in range(n)]
        self.ordered = [0] * n                  # ordered_segments of the receive windows
        self.got = [bytearray() for _ in range(n)]
        self.eof = [False] * n
        self.exits, self.deadline = {}, 0
        self.info = np.zeros((max_packets, 64), np.uint8)
        self.ranges = np.zeros((max_packets, max_ranges, 2), np.uint64)
        self.segs = np.zeros((max_packets, max_segments, 16), np.uint8)
        self.conn = np.zeros(max_packets, np.uint32)
        self._fresh_records(now)

    def _fresh_records(self, now):
        """What LoopSet and CcSet keep in the set starts afresh with the set."""
        n = self.n
        self.loop = [lf.RuleLoop(now, **self.loop_params) for _ in range(n)]
        self.cc = [cr.RuleCc(**self.cc_params) for _ in range(n)]
        self.budget = self._cc_rto([0] * n)
        self.delays = [0] * n

    def rebuild(self, keep, n_new, now):
        """The sets over a new member list: keep[k] is the old index of new
        member k, or None for a new connection.  The per-connection rules carry
        on; the loop and the controller records start afresh."""
        def relist(old, make):
            return [old[k] if k is not None else make() for k in keep]
        assert len(keep) == n_new
        self.rx = relist(self.rx, lambda: rr.RuleRx(RX_CAP))
        self.ack = relist(self.ack, lambda: ar.RuleAck(ACK_WP))
        self.tx = relist(self.tx, lambda: tr.RuleTx(TX_CAP, RQ_CAP))
        self.sent = relist(self.sent, lambda: sr.RuleSent(SENT_WS, self.MSEG))
        self.ordered = relist(self.ordered, lambda: 0)
        self.got = relist(self.got, bytearray)
        self.eof = relist(self.eof, lambda: False)
        self.n, self.exits = n_new, {}
        self._fresh_records(now)

    # ---------------------------------------------------------------- views
    def nbs(self):
        return [dict(stream_err=self.rx[c].err, ack_err=self.ack[c].err, sent_err=self.sent[c].err,
                     rto_count=self.sent[c].rto_count, tracked=self.sent[c].tracked,
                     last_sent_us=self.sent[c].last_sent_us, tail=self.tx[c].tail, write_pos=self.tx[c].write_pos,
                     rq_len=len(self.tx[c].queue), cap=self.tx[c].cap) for c in range(self.n)]

    def states(self):
        """The records of the six sets as lists of dicts, under the views of the stage harnesses."""
        rxs = []
        for c, r in enumerate(self.rx):
            rxs.append(dict(r.record(), ordered_segments=self.ordered[c]))
        return dict(stream_rx=rxs, ack=[r.record() for r in self.ack], stream_tx=[r.record() for r in self.tx],
                    sent=[r.record_fields() for r in self.sent], cc=[r.view() for r in self.cc],
                    loop=[r.view() for r in self.loop])

    def _cc_rto(self, fired):
        return [r.rto(int(f), s.last_sent, s.bytes_in_flight, PKT_BYTES, self.max_budget, s.err)
                for r, s, f in zip(self.cc, self.sent, fired)]

    # ---------------------------------------------------------------- between batches
    def write(self, chunks):
        """chunks[c]: bytes offered to member c.  Returns n_written."""
        return [t.write(bytes(d)) for t, d in zip(self.tx, chunks)]

    def close_members(self, how, linger_us, now):
        lf.close_set(self.loop, how, linger_us, now)

    # ---------------------------------------------------------------- the send half
    def send(self, now):
        n, NP, MSEG = self.n, self.NP, self.MSEG
        iv, sv = _iv(self.info), _sv(self.segs)
        calls = []
        budget, may = lf.check_set(self.loop, self.nbs(), now, self.budget)
        self.budget = budget
        calls.append(("loop_set_check", dict(budget=np.asarray(budget, np.uint32),
                                             may_ack_only=np.asarray(may, np.uint8))))
        wp0 = [t.write_pos for t in self.tx]
        packets, first, counts = tr.plan_set(self.tx, budget, PAYLOAD, MSEG, NP)
        total = len(packets)
        retx = [False] * NP
        for i, (c, pn, sg) in enumerate(packets):
            rec = np.zeros(1, I_T)
            rec["packet_number"], rec["n_segments"] = pn, len(sg)
            iv[i] = rec[0]
            for j, (o, ln) in enumerate(sg):
                sv[i, j] = (o, o & (self.tx[c].cap - 1), ln, ln)
                retx[i] |= o < wp0[c]
            self.conn[i] = c
        self.conn[total:] = NO_CONN             # conn_of is written whole
        calls.append(("stream_tx_set_plan", dict(first=_u64(first), count=np.asarray(counts, np.uint32), total=total,
                                                 info=self.info.copy(), segs=self.segs.copy(),
                                                 conn_of=self.conn.copy())))
        writes, appended, total_a = lf.append_set(self.loop, self.nbs(), total, NP)
        for t, c, what, off, data_off in writes:
            rec = np.zeros(1, I_T)
            rec["flags"], rec["n_segments"] = (0x10, 1) if what == lf.FIN else (0x08, 0)
            iv[t] = rec[0]
            self.conn[t] = c
            if what == lf.FIN:
                sv[t, 0] = (off, data_off, 0, 0)
        pending = sum(1 for r in self.loop if r.pending)
        calls.append(("loop_set_append", dict(total_out=total_a, appended=np.asarray(appended, np.uint8),
                                              info=self.info.copy(), segs=self.segs.copy(), conn_of=self.conn.copy())))
        aw, total_b, attached = ar.attach_set(self.ack, now, first, counts, total_a, may, NP, self.MR)
        trunc = [False] * NP
        ack_only = 0
        for t, c, only, la, lio, delay, nr, rows in aw:
            if only:
                self.info[t] = 0
                self.conn[t] = c
                ack_only += 1
            iv["flags"][t] |= 0x80
            iv["largest_acked"][t], iv["largest_in_order"][t], iv["delay_us"][t], iv["n_ranges"][t] = la, lio, delay, nr
            for k, row in enumerate(rows):
                self.ranges[t, k] = row
            trunc[t] = attached[c] == ar.TRUNCATED
        calls.append(("ack_set_attach", dict(total_out=total_b, attached=np.asarray(attached, np.uint8),
                                             info=self.info.copy(), ranges=self.ranges.copy(), segs=self.segs.copy(),
                                             conn_of=self.conn.copy())))
        sw_writes, sw_attached = sr.attach_set(self.sent, first, counts, NP)
        for t, sw in sw_writes:
            iv["stop_waiting"][t] = sw
        calls.append(("sent_set_attach", dict(attached=np.asarray(sw_attached, np.uint8), info=self.info.copy())))
        npk = total_b
        wire = np.zeros((npk, SLOT), np.uint8)
        lens, status = np.zeros(npk, np.uint16), np.zeros(npk, np.uint8)
        look = np.zeros(npk, [("conn", "<u4"), ("flags", "u1"), ("packet_number", "<u8"), ("n_segments", "<u2"),
                              ("retx", "?"), ("trunc", "?")])
        if npk:
            records = []
            for i in range(npk):
                c, I = int(self.conn[i]), iv[i]
                ns = int(I["n_segments"])
                assert ns <= MSEG and int(I["n_ranges"]) <= self.MR
                sg = [(int(sv[i, j]["offset"]), int(sv[i, j]["len"])) for j in range(ns)]
                assert all(self.tx[c].holds(o, ln) for o, ln in sg), "a planned segment left its window"
                sack = None
                if int(I["flags"]) & 0x80:
                    sack = (int(I["largest_acked"]), int(I["largest_in_order"]),
                            [(int(a), int(b)) for a, b in self.ranges[i, :int(I["n_ranges"])]], int(I["delay_us"]))
                raw = pr.encode(flags=int(I["flags"]), sack=sack, packet_number=int(I["packet_number"]),
                                stop_waiting=int(I["stop_waiting"]),
                                segments=[(o, self.tx[c].stream_bytes(o, ln)) for o, ln in sg])
                assert len(raw) <= SLOT
                wire[i, :len(raw)] = np.frombuffer(raw, np.uint8) ^ self.pad[:len(raw)]
                lens[i] = len(raw)
                look[i] = (c, raw[0], int(I["packet_number"]), ns, retx[i], trunc[i])
                records.append((c, int(I["packet_number"]), len(raw), 0, int(I["flags"]), int(I["stop_waiting"]), sg))
            calls.append(("stream_tx_set_encode", dict(wire=wire, wire_lens=lens, status=status)))
            sr.record_set(self.sent, records, now)
            calls.append(("sent_set_record", {}))
        out = lf.sent_set(self.loop, self.nbs(), counts, attached, self.delays, now, self.max_exits)
        deadline, exits, reasons, n_exits, new_index, nconn_new = out
        calls.append(("loop_set_sent", dict(deadline_us=deadline, exits=np.asarray(exits, np.uint32),
                                            reasons=np.asarray(reasons, np.uint8), n_exits=n_exits,
                                            new_index=np.asarray(new_index, np.uint32), nconn_new=nconn_new)))
        self.deadline = deadline
        for c, why in zip(exits, reasons):
            self.exits[c] = why
        return dict(calls=calls, npk=npk, wire=wire, lens=lens, conn=self.conn[:npk].copy(), look=look,
                    exits=list(exits), n_exits=n_exits, new_index=new_index, nconn_new=nconn_new, ack_only=ack_only,
                    pending=pending)

    # ---------------------------------------------------------------- the receive half
    def receive(self, batch, now, conn_of=None):
        """batch: dict(npk, wire uint8 [npk, SLOT] as on the wire, lens, conn).
        conn_of: the members as a listener routed them, in place of batch's."""
        n, MSEG = self.n, self.MSEG
        calls = []
        npk = batch["npk"]
        stats = dict(trunc_acks=0, retx_delivered=0, late=0)
        if npk:
            wire, lens = batch["wire"], batch["lens"]
            conn = [int(c) for c in (batch["conn"] if conn_of is None else conn_of)]
            raws = [bytes(wire[i, :int(lens[i])] ^ self.pad[:int(lens[i])]) for i in range(npk)]
            info, ranges, segs, failed = decode_expect(raws, self.MR, MSEG)
            calls.append(("packet_decode", dict(info=info, ranges=ranges, segs=segs, failed=failed)))
            civ = _iv(info)                   # a failed packet's row is its status and zeros
            sv = _sv(segs)
            gone = [r.exited for r in self.loop]
            stats["late"] = sum(1 for c in conn if c < n and gone[c])     # packets of members that had exited before
            conn2 = lf.receive_set(self.loop, civ["status"], civ["flags"], civ["packet_number"], conn, now)
            calls.append(("loop_set_receive", dict(conn_of=np.asarray(conn2, np.uint32))))
            packets = rr.packets_from_raw(wire[:npk], civ, sv, self.pad)
            mine = [[] for _ in range(n)]
            for i, c in enumerate(conn2):
                if c < n:
                    mine[c].append(i)
            seg_status = np.zeros((npk, MSEG), np.uint8)
            for c, idx in enumerate(mine):
                if not idx:
                    continue
                rule = self.rx[c]
                before = rule.err
                rows = rule.deliver([packets[i] for i in idx], count_contested=True)
                for i, row in zip(idx, rows):
                    seg_status[i, :len(row)] = row
                self.ordered[c] += rule.contested
                if before == rr.NONE and rule.err == rr.OVERLAP:
                    rule.err_packet = idx[rule.err_packet]
            calls.append(("stream_set_deliver", dict(seg_status=seg_status)))
            ar.receive_set(self.ack, [(int(civ["status"][i]), conn2[i], int(civ["packet_number"][i]),
                                       int(civ["stop_waiting"][i]), int(civ["n_segments"][i]), seg_status[i])
                                      for i in range(npk)], now, MSEG)
            calls.append(("ack_set_receive", {}))
            n_read, eof, data = [], [], []
            for c, r in enumerate(self.rx):
                d, e = r.read(WANT)
                n_read.append(len(d))
                eof.append(int(e))
                data.append(d)
                self.got[c] += d
                self.eof[c] = self.eof[c] or bool(e)
            calls.append(("stream_set_read", dict(n_read=_u64(n_read), eof=np.asarray(eof, np.uint8), data=data)))
            before = [{k: s["state"] for k, s in r.slots.items()} for r in self.sent]
            splits = [r.cutback for r in self.cc]
            model = []
            for i in range(npk):
                nr = int(civ["n_ranges"][i])
                a = sr.Ack(int(civ["largest_acked"][i]), int(civ["largest_in_order"][i]),
                           [(int(f), int(l)) for f, l in ranges[i, :nr]], int(civ["packet_number"][i]),
                           int(civ["delay_us"][i]))
                model.append((int(civ["status"][i]), conn2[i], int(civ["flags"][i]), a, nr))
            events = sr.ack_set(self.sent, model, now, self.MR)
            rows = [cr.cc_row(before[c], self.sent[c], events[c], splits[c]) for c in range(n)]
            calls.append(("cc_sent_ack", dict(events=event_array(events), rows=row_array(rows))))
            self.delays = [r.ack(events[c], rows[c], now, self.sent[c].last_sent, self.sent[c].lio, self.sent[c].err)
                           for c, r in enumerate(self.cc)]
            calls.append(("cc_set_ack", dict(delay_us=_u64(self.delays))))
            look = batch.get("look")
            if look is not None:
                for i in range(npk):
                    handled = conn2[i] < n and not failed[i] and int(civ["status"][i]) == 0
                    stats["trunc_acks"] += bool(handled and look["trunc"][i])
                    stats["retx_delivered"] += bool(look["retx"][i] and rr.ACCEPTED in seg_status[i].tolist())
        fired = sr.rto_set(self.sent, self.delays, now)
        calls.append(("sent_set_rto", dict(fired=np.asarray(fired, np.uint8))))
        self.budget = self._cc_rto(fired)
        calls.append(("cc_set_rto", dict(budget=np.asarray(self.budget, np.uint32))))
        dc, do, dl, touch, upto = sr.drain_set(self.sent, self.max_entries)
        k, E = len(dc), self.max_entries
        e_conn, e_off, e_len = np.full(E, NO_CONN, np.uint32), np.zeros(E, np.uint64), np.zeros(E, np.uint32)
        e_conn[:k], e_off[:k], e_len[:k] = dc, _u64(do), dl
        calls.append(("sent_set_drain", dict(conn_of=e_conn, offset=e_off, len=e_len, n_entries=k,
                                             touch=np.asarray(touch, np.uint8), upto=_u64(upto))))
        st = tr.retransmit_set(self.tx, [(int(c), int(o), int(ln)) for c, o, ln in zip(e_conn, e_off, e_len)])
        calls.append(("stream_tx_set_retransmit", dict(status=np.asarray(st, np.uint8))))
        for r, t in zip(self.ack, touch):
            if t:
                r.touch()
        calls.append(("ack_set_touch", {}))
        for r, u in zip(self.tx, upto):
            r.release(int(u))
        calls.append(("stream_tx_set_release", {}))
        stats["fired"] = int(sum(fired))
        return dict(calls=calls, stats=stats)


# ------------------------------------------------------------------ a server
class RuleServer:
    """A RuleEndpoint behind a RuleListener.  The names and the raw ring go
    through route first; the accepted members are created before deliver; when
    sent lists exits, new_index goes to remap and the per-connection rules are
    re-listed in the new order."""

    def __init__(self, max_conn, now, max_ranges, max_packets, **kw):
        self.listener = lr.RuleListener(max_conn)
        self.kw = dict(max_ranges=max_ranges, max_packets=max_packets, **kw)
        self.end = None

    def route(self, names, pkts, lens, now):
        """Returns (the route call's arrays, how many members were accepted).
        The endpoint is rebuilt over the longer list when there are any."""
        conn_of, cls, accepted = self.listener.route(names, pkts, lens, pkts.shape[1])
        assert not self.listener.unspecified
        acc = np.zeros(len(accepted), fec.LISTEN_ACCEPT_DTYPE)
        for j, (i, m, cid, row) in enumerate(accepted):
            acc[j]["packet"], acc[j]["member"], acc[j]["client_id"] = i, m, cid
            acc[j]["name"] = np.frombuffer(row, np.uint8)
        if accepted:
            if self.end is None:
                self.end = RuleEndpoint(len(accepted), now, **self.kw)
            else:
                self.end.rebuild(list(range(self.end.n)) + [None] * len(accepted), self.end.n + len(accepted), now)
        call = ("listen_route", dict(conn_of=np.asarray(conn_of, np.uint32), cls=np.asarray(cls, np.uint8),
                                     accepted=acc, n_accepted=len(accepted)))
        return call, len(accepted), conn_of

    def remap(self, new_index, nconn_new, now):
        status = self.listener.remap([int(v) for v in new_index], nconn_new)
        assert status == 0, status
        keep = [None] * nconn_new
        for old, new in enumerate(new_index):
            if new != NO_CONN:
                keep[new] = old
        if nconn_new:
            self.end.rebuild(keep, nconn_new, now)
        else:
            self.end = None                     # a set has a member at least: nothing is left to build one over
        return ("listen_remap", dict(status=0))

    def listener_state(self):
        r = self.listener
        return dict(nconn=r.nconn, n_dead=r.n_dead, n_slots=r.n_slots, err=r.err, counts=list(r.counts),
                    entries=r.entries())


# ------------------------------------------------------------------ a seeded life
KINDS = ("close_writer", "close_both", "linger", "abort", "silent", "bad", "idle", "ack_fin")
FORGED = {"bad": bytes([0x20]),                 # PSH and nothing behind it: io.EOF
          "ack_fin": pr.encode(flags=0x10, sack=(1, 1, [], 0), packet_number=0)}


def script(seed, n):
    """The lives of n connections between two sides.  Every member draws its
    writes on both sides (0 to 20,000 bytes in one to four pieces, or none), its
    loss share (0 to 20 %, on FIN and RST too for some), and its ending: one of
    KINDS.  Side 0 is the one that closes first, aborts, or stops hearing its
    peer; `ack_fin` is a peer whose packet the link turns into an ACK|FIN, the
    one way reason PEER_ACK_FIN arises (nothing here sends an ACK|FIN)."""
    rng = random.Random(seed)
    s = types.SimpleNamespace()
    s.seed, s.n = seed, n
    s.idle_us = rng.choice([1_200_000, 400_000_000])
    s.members = []
    for c in range(n):
        m = types.SimpleNamespace()
        # every kind once among the first eight; one silent member a run: each of its RTOs costs the pair rounds
        m.kind = KINDS[(c + seed) % len(KINDS)] if c < len(KINDS) else rng.choice([k for k in KINDS if k != "silent"])
        m.writes = [[], []]
        for side in (0, 1):
            pieces = rng.choice([0, 1, 1, 2, 3, 4])
            total = rng.choice([rng.randint(1, 2500), rng.randint(1, 2500), rng.randint(2501, 20000)]) if pieces else 0
            if side == 0 and m.kind == "linger" and total < 3000:
                pieces, total = max(pieces, 1), rng.randint(3000, 20000)
            if side == 0 and m.kind == "silent":    # thirteen packets or more: an RTO takes one out of flight and the
                pieces, total = 1, rng.randint(18000, 20000)   # window of two sends nothing new, so eleven need twelve
            if total:
                pieces = min(pieces, total)
                cuts = sorted(rng.sample(range(1, total), pieces - 1)) if pieces > 1 else []
                data = np.random.default_rng([seed, c, side]).integers(0, 256, total, dtype=np.uint8).tobytes()
                rounds = sorted(rng.randint(1, 5) for _ in range(pieces))
                if side == 0 and m.kind == "silent":
                    rounds = [1]
                for r, a, b in zip(rounds, [0] + cuts, cuts + [total]):
                    m.writes[side].append((r, data[a:b]))
        m.data = [b"".join(d for _, d in m.writes[side]) for side in (0, 1)]
        last = max([r for w in m.writes for r, _ in w] + [1])
        m.loss = 0.0 if rng.random() < (0.5 if n <= 100 else 0.85) else rng.uniform(0.0, 0.2)   # fewer rounds at 257
        m.loss_ctl = rng.random() < 0.3
        m.at = 1 if m.kind == "silent" else last + rng.randint(0, 3)   # the round of the close, abort, silence, forgery
        m.linger_us = rng.choice([30_000, 5_000_000]) if m.kind == "linger" else 0
        s.members.append(m)
    return s


def _u(*key):
    h = hashlib.blake2b(repr(key).encode(), digest_size=8).digest()
    return int.from_bytes(h, "little") / 2.0 ** 64


def link(scr, state, side, rnd, out):
    """What of the packets side `side` sent in round rnd reaches the peer: the
    decision per packet comes from the seed and the packet's identity (side,
    round, member, number, flags).  Returns a batch for receive(): the kept
    rows, with a forged row where the script says so."""
    keep, forged, lost_fin = [], {}, 0
    look = out["look"]
    for i in range(out["npk"]):
        c, fl, pn = int(look["conn"][i]), int(look["flags"][i]), int(look["packet_number"][i])
        m = scr.members[state["ids"][side][c]]
        if m.kind == "silent" and side == 1 and rnd >= m.at:
            continue
        if m.kind in FORGED and side == 1 and rnd >= m.at and id(m) not in state["forged"]:
            state["forged"].add(id(m))
            forged[len(keep)] = FORGED[m.kind]
            keep.append(i)
            continue
        if (m.loss_ctl or not fl & 0x18) and _u(scr.seed, side, rnd, state["ids"][side][c], pn, fl) < m.loss:
            lost_fin += bool(fl & 0x10)
            continue
        keep.append(i)
    idx = np.asarray(keep, np.int64)
    wire, lens = out["wire"][idx].copy(), out["lens"][idx].copy()
    pad = pad_bytes()
    for k, raw in forged.items():
        wire[k] = 0
        wire[k, :len(raw)] = np.frombuffer(raw, np.uint8) ^ pad[:len(raw)]
        lens[k] = len(raw)
    lk = out["look"][idx].copy()
    for k in forged:
        lk["trunc"][k] = lk["retx"][k] = False
    return dict(npk=len(keep), wire=wire, lens=lens, conn=out["conn"][idx].copy(), look=lk, src=idx, forged=forged,
                lost_fin=lost_fin, sender=out)


def run_pair(scr, A, B, round_cap=200, start_us=START_US):
    """Both sides through the script.  A and B have RuleEndpoint's methods and
    fields.  The clock steps 20 ms a round; when a round sent nothing it jumps
    to the earlier of the two deadlines sent returned, which is how the timers
    fire.  Returns what test_the_script_reaches_what_it_is_for asserts on."""
    n = scr.n
    ends = (A, B)
    state = dict(forged=set(), ids=[list(range(n)), list(range(n))])
    st = dict(rounds=0, trunc_acks=0, retx_delivered=0, late=0, pending_rounds=0, over_exits=0, lost_fin=0, ack_only=0,
              fired=0, fin_round=[{}, {}], data_round=[{}, {}], reasons=[{}, {}], done=False)
    closed = [set(), set()]
    now = start_us
    for rnd in range(1, round_cap + 1):
        st["rounds"] = rnd
        sent_any = False
        for side in (0, 1):
            E, other = ends[side], ends[1 - side]
            t0 = now + 2000 * side
            chunks = [b"".join(d for r, d in m.writes[side] if r == rnd) for m in scr.members]
            if any(chunks):
                assert E.write(chunks) == [len(d) for d in chunks]
            how, linger = [0] * n, [0] * n
            for c, m in enumerate(scr.members):
                if c in closed[side]:
                    continue
                if side == 0 and rnd == m.at and m.kind in ("close_writer", "close_both", "linger"):
                    how[c], linger[c] = lf.HOW_CLOSE, m.linger_us
                elif side == 0 and rnd == m.at and m.kind == "abort":
                    how[c] = lf.HOW_ABORT
                elif side == 1 and E.eof[c] and m.kind in ("close_both", "linger"):
                    how[c] = lf.HOW_CLOSE
                if how[c]:
                    closed[side].add(c)
            if any(how):
                E.close_members(how, linger, t0 - 500)
            out = E.send(t0)
            sent_any |= out["npk"] > 0
            st["ack_only"] += out["ack_only"]
            st["pending_rounds"] += out["pending"] > 0
            st["over_exits"] += out["n_exits"] > len(out["exits"])
            for c, why in E.exits.items():
                st["reasons"][side][c] = why
            for i in range(out["npk"]):
                c = int(out["look"]["conn"][i])
                if int(out["look"]["flags"][i]) & 0x10:
                    st["fin_round"][side].setdefault(c, rnd)
                elif out["look"]["n_segments"][i] and out["look"]["packet_number"][i]:
                    st["data_round"][side][c] = rnd
            batch = link(scr, state, side, rnd, out)
            st["lost_fin"] += batch["lost_fin"]
            got = other.receive(batch, t0 + 1000)
            for k in ("trunc_acks", "retx_delivered", "late", "fired"):
                st[k] += got["stats"][k]
        if len(A.exits) == n and len(B.exits) == n:
            st["done"] = True
            break
        nxt = now + STEP_US
        if not sent_any:
            dl = min(A.deadline, B.deadline)
            if dl < lf.NEVER:
                nxt = max(nxt, dl)
        now = nxt
    return st


# ------------------------------------------------------------------ a server and its clients
def client_name(k, as_mapped=False):
    ip4 = bytes([10, 0, k >> 8, k & 255])
    return lr.name_v6(lr.mapped(ip4), 4000 + k) if as_mapped else lr.name_v4(ip4, 4000 + k)


def _row(raw):
    out = np.zeros(SLOT, np.uint8)
    out[:len(raw)] = np.frombuffer(raw, np.uint8)
    return out, len(raw)


def run_server(scr, S, C, device, round_cap=200):
    """The script with the server as side 0 -- the side that closes first,
    aborts, or is handed a forged packet -- and the clients as side 1, a
    RuleEndpoint C.  S is a RuleServer, or with device a
    chain_harness.ServerHarness.
    Round 1's ring holds the INITs of all clients with their first data behind
    them, interleaved; clients 5 and 6 send their data under the v4-mapped form
    of their address, client 7 repeats its INIT, and a stranger sends data.
    When a round lists exits and three or more wait (or nobody is left), that
    call's new_index goes to remap and the sets are rebuilt over the
    survivors; until then the exited members stay in the sets and what arrives
    for them is masked.  After the first remap that leaves survivors, an
    address that has closed on both sides connects again, and is accepted
    under the next number: st["again"] = (nconn before, its member)."""
    n = scr.n
    rule = S.rule if device else S
    client_of = []                               # server member -> client
    state = dict(forged=set(), ids=[client_of, list(range(n))])
    st = dict(rounds=0, done=False, reasons=[{}, {}], accepted=0, remaps=0, classes=set(), again=None, late=0)
    waiting = 0                                  # exits listed and not yet remapped away
    closed = [set(), set()]
    rng = random.Random(scr.seed)
    now = START_US
    knock = None
    for rnd in range(1, round_cap + 1):
        st["rounds"] = rnd
        chunks = [b"".join(d for r, d in m.writes[1] if r == rnd) for m in scr.members]
        if any(chunks):
            assert C.write(chunks) == [len(d) for d in chunks]
        how = [0] * n
        for c, m in enumerate(scr.members):
            if c not in closed[1] and C.eof[c] and m.kind in ("close_both", "linger"):
                how[c] = lf.HOW_CLOSE
                closed[1].add(c)
        if any(how):
            C.close_members(how, [0] * n, now - 500)
        out = C.send(now)
        batch = link(scr, state, 1, rnd, out)
        lists = [[] for _ in range(n + 1)]
        for i in range(batch["npk"]):
            k = int(batch["conn"][i])
            lists[k].append((client_name(k, as_mapped=k in (5, 6)), batch["wire"][i], int(batch["lens"][i])))
        if rnd == 1:
            for k in range(n):
                lists[k].insert(0, (client_name(k),) + _row(lr.init_packet(0x1000 + k)))
            lists[7 % n].append((client_name(7 % n),) + _row(lr.init_packet(0x1000 + 7 % n)))      # a dup-INIT
            lists[n].append((client_name(9999),) + _row(bytes([0x20, 1, 0, 0, 1, 0x55])))        # a stranger's data
        if knock is not None:                    # a closed address connects again, behind its own late packets
            lists[knock].append((client_name(knock),) + _row(lr.init_packet(0x2000 + knock)))
        order = [k for k, l in enumerate(lists) for _ in l]
        if rnd == 1:
            rng.shuffle(order)                  # interleaved; every client's own rows keep their order
        at = [0] * (n + 1)
        ring = []
        for k in order:
            ring.append(lists[k][at[k]])
            at[k] += 1
        npk = len(ring)
        sent_any = out["npk"] > 0
        if npk:
            names = np.stack([np.frombuffer(r[0], np.uint8) for r in ring])
            pkts = np.stack([r[1] for r in ring])
            lens = np.asarray([r[2] for r in ring], np.uint16)
            before = rule.listener.nconn
            if device:
                staged = S.route(names, pkts, lens, now + 500)
            else:
                (_, w), _, conn_of = S.route(names, pkts, lens, now + 500)
            for m in range(before, rule.listener.nconn):      # the accepted, in member order
                row = rule.listener.rows[m]
                client_of.append(next(k for k in range(n) if lr.clean_row(client_name(k)) == row))
            st["accepted"] += rule.listener.nconn - before
            if knock is not None:
                st["again"] = (before, rule.listener.members[lr.addr_string(client_name(knock))])
                knock = None
            ring_batch = dict(npk=npk, wire=pkts, lens=lens, conn=None)
            if S.end is not None:
                if device:
                    got = S.end.receive(ring_batch, now + 1000, staged=staged)
                else:
                    got = S.end.receive(ring_batch, now + 1000, conn_of=conn_of)
                st["late"] += got["stats"]["late"]
        elif S.end is not None:
            S.end.receive(dict(npk=0), now + 1000)
        st["classes"] |= {c for c, v in enumerate(rule.listener.counts) if v}
        back = dict(npk=0)
        if S.end is not None:
            E = S.end
            chunks = [b"".join(d for r, d in scr.members[k].writes[0] if r == rnd) for k in client_of]
            if any(chunks):
                assert E.write(chunks) == [len(d) for d in chunks]
            how, linger = [0] * len(client_of), [0] * len(client_of)
            for m, k in enumerate(client_of):
                kind = scr.members[k].kind
                if k not in closed[0] and rnd == scr.members[k].at and kind in ("close_writer", "close_both", "linger",
                                                                                 "abort"):
                    how[m], linger[m] = (lf.HOW_ABORT if kind == "abort" else lf.HOW_CLOSE), scr.members[k].linger_us
                    closed[0].add(k)
            if any(how):
                E.close_members(how, linger, now + 1500)
            out2 = E.send(now + 2000)
            sent_any |= out2["npk"] > 0
            back = link(scr, state, 0, rnd, out2)
            back["conn"] = np.asarray([client_of[int(m)] for m in back["conn"]], np.uint32)
            if out2["n_exits"]:
                assert out2["n_exits"] == len(out2["exits"])
                for m, why in zip(out2["exits"], out2["calls"][-1][1]["reasons"]):
                    st["reasons"][0][client_of[m]] = int(why)
                waiting += out2["n_exits"]
            new_index, nconn_new = out2["new_index"], out2["nconn_new"]
            if waiting >= 3 or (waiting and nconn_new == 0):     # a host that rebuilds for three exits or more:
                if device:                                       # until then the exited members stay in the sets
                    S.remap(out2["_dev"][3], new_index, nconn_new, now + 2500)
                else:
                    S.remap(new_index, nconn_new, now + 2500)
                st["remaps"] += 1
                waiting = 0
                gone = [k for m, k in enumerate(client_of) if new_index[m] == NO_CONN and k in C.exits]
                if st["again"] is None and knock is None and nconn_new and gone:
                    knock = gone[0]
                client_of[:] = [k for m, k in enumerate(client_of) if new_index[m] != NO_CONN]
        C.receive(back, now + 3000, conn_of=back["conn"] if back["npk"] else None)
        st["reasons"][1] = dict(C.exits)
        if len(C.exits) == n and rule.listener.nconn == 0:
            st["done"] = True
            break
        nxt = now + STEP_US
        if not sent_any:
            dl = min(C.deadline, S.end.deadline if S.end is not None else lf.NEVER)
            if dl < lf.NEVER:
                nxt = max(nxt, dl)
        now = nxt
    return st
