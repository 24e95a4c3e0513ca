"""A set of send windows on the device (ugo_fec_stream_tx_set_*) beside one
RuleTx of tests/stream_tx_ref.py per member; test infrastructure only.

After every call TxHarness compares every field of every member's record,
every output array in whole -- including what a call must leave alone: the
sentinel-filled entries past n_segments and past total, the slots of refused
packets, the bytes of a slot past round_up(len, 16), the operand arrays -- and,
for the watched members, the whole window against the byte model (windows are
pre-filled with a sentinel, so a write outside [tail, tail+m) shows) and the
live entries of the retransmission ring.  `watch`: the members whose windows
and rings are copied out (default all), for sets too large to copy out member
by member; the other members' windows are not pre-filled.
"""
import numpy as np
import torch

import packet_ref as pr
import stream_tx_ref as tr
from ugo_amd import fec

SENTINEL = 0xC3
NO_CONN = fec.STREAM_NO_CONN


def _put(arr, where="device"):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return t.pin_memory() if where == "pinned" else t.cuda()


def expected_plan_arrays(rules, packets, max_packets, max_segments):
    """plan's info / segs / conn_of over sentinel-filled arrays."""
    info = np.full((max_packets, 64), 0xEE, np.uint8)
    segs = np.full((max_packets, max_segments, 16), 0xDD, np.uint8)
    conn = np.full(max_packets, NO_CONN, np.uint32)
    iv = info.view(fec.PKT_INFO_DTYPE).reshape(max_packets)
    sv = segs.reshape(max_packets, max_segments * 16).view(fec.PKT_SEGMENT_DTYPE).reshape(max_packets, max_segments)
    for i, (c, pn, sg) in enumerate(packets):
        rec = np.zeros(1, fec.PKT_INFO_DTYPE)
        rec["packet_number"], rec["n_segments"] = pn, len(sg)
        iv[i] = rec[0]
        for j, (o, n) in enumerate(sg):
            sv[i, j] = (o, o & (rules[c].cap - 1), n, n)
        conn[i] = c
    return info, segs, conn


def expected_packet(rules, conn, I, S, max_segments, slot, framed, ks):
    """(status, slot image or None, wire_len) of one packet for set_encode: I
    its info record, S its segment row."""
    if not 0 <= conn < len(rules):
        return 0, None, 0
    ns = int(I["n_segments"])
    if ns > max_segments or int(I["n_ranges"]) > 0:
        assert int(I["n_ranges"]) == 0, "the harness states packets without a SACK only"
        return fec.PKT_CAPACITY, None, 0
    r = rules[conn]
    if not all(r.holds(int(S[j]["offset"]), int(S[j]["len"])) for j in range(ns)):
        return fec.PKT_OUT_OF_WINDOW, None, 0
    raw = pr.encode(flags=int(I["flags"]), packet_number=int(I["packet_number"]), stop_waiting=int(I["stop_waiting"]),
                    segments=[(int(S[j]["offset"]), r.stream_bytes(int(S[j]["offset"]), int(S[j]["len"])))
                              for j in range(ns)])
    raw = (bytes(6) if framed else b"") + raw
    if len(raw) > slot:
        return fec.PKT_CAPACITY, None, 0
    img = np.full(slot, SENTINEL, np.uint8)
    body = np.frombuffer(raw, np.uint8)
    img[:len(raw)] = body if ks is None else body ^ ks[:len(raw)]
    img[len(raw):(len(raw) + 15) & ~15] = 0
    return 0, img, len(raw)


class TxHarness:
    def __init__(self, enc, caps, rq_caps=8, starts=None, pns=None, watch=None):
        n = len(caps)
        self.caps = list(caps)
        rq_caps = [rq_caps] * n if isinstance(rq_caps, int) else list(rq_caps)
        starts = [0] * n if starts is None else list(starts)
        pns = [0] * n if pns is None else list(pns)
        self.watch = list(range(n)) if watch is None else list(watch)
        watched = set(self.watch)
        self.txs = [fec.StreamTx(enc, cap, rq, s, p) for cap, rq, s, p in zip(self.caps, rq_caps, starts, pns)]
        self.rules = [tr.RuleTx(cap, rq, s, p, fill=SENTINEL if c in watched else 0)
                      for c, (cap, rq, s, p) in enumerate(zip(self.caps, rq_caps, starts, pns))]
        for c in self.watch:
            self.txs[c].window().fill_(SENTINEL)
        self.set = fec.StreamTxSet(enc, self.txs)
        self.enc, self.nconn = enc, n
        self.check()                                     # create: base = write_pos = tail = start, all else zero

    def close(self):
        self.set.close()
        for tx in self.txs:
            tx.close()

    # ---------------------------------------------------------------- state
    def check(self):
        states = self.set.states()                       # waits for the last call
        assert states.shape == (self.nconn,)
        want = [r.record() for r in self.rules]
        for k in fec.STREAM_TX_STATE_DTYPE.names:
            exp = np.array([w[k] for w in want], np.uint64)
            got = states[k].astype(np.uint64)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"record field {k} differs at members {bad[:8]}: {got[bad[:8]]} vs {exp[bad[:8]]}"
        for c in self.watch:
            r = self.rules[c]
            win = self.txs[c].window().cpu().numpy()
            bad = np.flatnonzero(win != r.W)
            assert bad.size == 0, f"window of member {c} differs at {bad[:8]} (of {bad.size})"
            ring = self.txs[c].queue().cpu().numpy().reshape(-1).view(fec.STREAM_TX_RQ_DTYPE)
            live = [(int(ring[(r.rq_head + k) % r.rq_cap]["offset"]), int(ring[(r.rq_head + k) % r.rq_cap]["len"]))
                    for k in range(len(r.queue))]
            assert live == [tuple(q) for q in r.queue], (c, live, r.queue)
        return states

    # ---------------------------------------------------------------- write
    def write(self, datas, shifts=None, where="device", guard=40):
        """datas[c]: the bytes offered to member c (b"" offers nothing).  Member
        c's bytes start shifts[c] bytes past a 16-B boundary of one source
        buffer.  Returns n_written as a list."""
        assert len(datas) == self.nconn
        shifts = [(2 * c + 1) % 16 for c in range(self.nconn)] if shifts is None else list(shifts)
        offs, cur = [], guard
        for c, d in enumerate(datas):
            cur += (-cur) % 16 + shifts[c]
            offs.append(cur)
            cur += len(d) + guard
        src = np.full(cur + 16, 0x5A, np.uint8)
        for o, d in zip(offs, datas):
            src[o:o + len(d)] = np.frombuffer(d, np.uint8)
        room = _put(np.concatenate([np.zeros(16, np.uint8), src]), where)
        at = (-room.data_ptr()) % 16                      # src itself on a 16-B boundary, the members at their shifts
        dsrc = room[at:at + len(src)]
        dsrc.copy_(torch.from_numpy(src))
        doff = _put(np.asarray(offs, np.int64), where)
        dn = _put(np.asarray([len(d) for d in datas], np.int64), where)
        nw = _put(np.full(self.nconn, -1, np.int64), where)
        self.set.write(dsrc, doff, dn, n_written=nw)
        want = [r.write(d) for r, d in zip(self.rules, datas)]
        self.check()
        assert nw.cpu().numpy().tolist() == want, (nw.cpu().numpy().tolist()[:8], want[:8])
        assert np.array_equal(dsrc.cpu().numpy(), src) and dn.cpu().numpy().tolist() == [len(d) for d in datas]
        return want

    # ---------------------------------------------------------------- release / retransmit
    def release(self, uptos, where="device"):
        self.set.release(_put(np.asarray(uptos, np.uint64).view(np.int64), where))
        for r, u in zip(self.rules, uptos):
            r.release(int(u))
        self.check()

    def retransmit(self, entries, where="device"):
        """entries: [(conn, offset, len)].  Returns the statuses."""
        m = len(entries)
        conn = np.asarray([e[0] for e in entries], np.int64).astype(np.uint32).view(np.int32)
        off = np.asarray([e[1] & tr.M64 for e in entries], np.uint64).view(np.int64)
        ln = np.asarray([e[2] for e in entries], np.int64).astype(np.uint32).view(np.int32)
        st = _put(np.full(m + 32, 0x77, np.uint8), where)
        self.set.retransmit(_put(conn, where), _put(off, where), _put(ln, where), status=st[16:16 + m])
        want = tr.retransmit_set(self.rules, [(e[0], e[1] & tr.M64, e[2]) for e in entries])
        self.check()
        got = st.cpu().numpy()
        assert (got[:16] == 0x77).all() and (got[16 + m:] == 0x77).all()
        assert got[16:16 + m].tolist() == want, (got[16:16 + m].tolist(), want)
        return want

    # ---------------------------------------------------------------- plan
    def plan(self, budgets, max_packets, M=1436, max_segments=8, where="device"):
        """One set_plan over sentinel-filled arrays; every output compared in
        whole.  Returns a dict: the device arrays, their host images (info,
        segs, conn as structured numpy) and `packets`, [(conn, pn, [(offset,
        len)])]."""
        assert len(budgets) == self.nconn
        dev = dict(info=_put(np.full((max_packets, 64), 0xEE, np.uint8), where),
                   segs=_put(np.full((max_packets, max_segments, 16), 0xDD, np.uint8), where),
                   conn=_put(np.full(max_packets, 0x77777777, np.int32), where),
                   first=_put(np.full(self.nconn, -1, np.int64), where),
                   count=_put(np.full(self.nconn, -1, np.int32), where),
                   total=_put(np.full(1, -1, np.int64), where))
        db = _put(np.asarray(budgets, np.int64).astype(np.uint32).view(np.int32), where)
        self.set.plan(db, max_packets, max_payload=M, max_segments=max_segments,
                      out=(dev["info"], dev["segs"], dev["conn"], dev["first"], dev["count"], dev["total"]))
        packets, first, counts = tr.plan_set(self.rules, [int(b) for b in budgets], M, max_segments, max_packets)
        self.check()
        assert int(dev["total"].cpu().numpy()[0]) == len(packets), (int(dev["total"].cpu().numpy()[0]), len(packets))
        got_first, got_count = dev["first"].cpu().numpy(), dev["count"].cpu().numpy()
        assert got_first.tolist() == first, (got_first.tolist()[:8], first[:8])
        assert got_count.tolist() == counts, (got_count.tolist()[:8], counts[:8])
        info, segs, conn = expected_plan_arrays(self.rules, packets, max_packets, max_segments)
        for name, exp in (("info", info), ("segs", segs), ("conn", conn.view(np.int32))):
            got = dev[name].cpu().numpy()
            bad = np.argwhere(got != exp)
            assert bad.size == 0, f"plan's {name} differs at {bad[:8].tolist()} (of {len(bad)})"
        assert db.cpu().numpy().view(np.uint32).tolist() == [int(b) for b in budgets]
        iv = info.view(fec.PKT_INFO_DTYPE).reshape(max_packets)
        sv = segs.reshape(max_packets, max_segments * 16).view(fec.PKT_SEGMENT_DTYPE).reshape(max_packets, max_segments)
        return dict(dev, packets=packets, info_np=iv, segs_np=sv, conn_np=conn, first_np=first, count_np=counts,
                    max_segments=max_segments)

    # ---------------------------------------------------------------- encode
    def encode(self, info, segs, conn, npk, slot=1488, framed=True, pad=None, where="device"):
        """One set_encode of npk packets into sentinel-filled slots with a guard
        slot behind: info / segs / conn are host arrays (PKT_INFO_DTYPE [>= npk],
        PKT_SEGMENT_DTYPE [>= npk, max_segments], uint32 [>= npk]), as plan
        left them or as a test bent them.  Every byte of the wire buffer, the
        lengths and the statuses are compared.  Returns (wire tensor [npk,
        slot], wire_lens tensor, status numpy)."""
        max_segments = segs.shape[1]
        ks = None if pad is None else np.frombuffer(pad, np.uint8)
        dinfo = _put(info.view(np.uint8).reshape(-1, 64), where)
        dsegs = _put(segs.view(np.uint8).reshape(len(segs), max_segments, 16), where)
        dconn = _put(conn.astype(np.uint32).view(np.int32), where)
        ranges = torch.zeros((max(npk, 1), 1, 2), dtype=torch.int64, device="cuda")
        buf = torch.full((npk + 1, slot), SENTINEL, dtype=torch.uint8, device="cuda")
        lens = torch.full((npk,), -1, dtype=torch.int16, device="cuda")
        status = torch.full((npk,), 0xEE, dtype=torch.uint8, device="cuda")
        dpad = None if pad is None else _put(ks[:slot].copy(), where)
        self.set.encode(dinfo, ranges, dsegs, dconn, slot, npackets=npk, pad=dpad, framed=framed,
                        out=(buf[:npk], lens, status))
        self.check()                                     # encode changes no record, window or ring
        exp = np.full((npk + 1, slot), SENTINEL, np.uint8)
        exp_len, exp_st = np.zeros(npk, np.uint16), np.zeros(npk, np.uint8)
        for i in range(npk):
            c = int(conn[i])
            st, img, n = expected_packet(self.rules, c if c != NO_CONN else -1, info[i], segs[i], max_segments, slot,
                                         framed, ks)
            exp_st[i], exp_len[i] = st, n
            if img is not None:
                exp[i] = img
        got, gl, gs = buf.cpu().numpy(), lens.cpu().numpy().view(np.uint16), status.cpu().numpy()
        assert np.array_equal(gs, exp_st), (np.flatnonzero(gs != exp_st)[:8], gs[gs != exp_st][:8], exp_st[gs != exp_st][:8])
        assert np.array_equal(gl, exp_len), (np.flatnonzero(gl != exp_len)[:8], gl[gl != exp_len][:8])
        bad = np.argwhere(got != exp)
        assert bad.size == 0, f"wire differs at (packet, byte) {bad[:8].tolist()} (of {len(bad)})"
        assert np.array_equal(dinfo.cpu().numpy(), info.view(np.uint8).reshape(-1, 64))   # the operands are only read
        return buf[:npk], lens, gs

    def plan_encode(self, budgets, max_packets, M=1436, max_segments=8, slot=1488, framed=True, pad=None,
                    where="device"):
        p = self.plan(budgets, max_packets, M, max_segments, where)
        n = len(p["packets"])
        p["wire"], p["wire_lens"], p["status"] = self.encode(p["info_np"], p["segs_np"], p["conn_np"], n, slot, framed,
                                                             pad, where)
        assert not p["status"].any()
        return p
