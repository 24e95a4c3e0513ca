"""A set of stream connections on the device (ugo_fec_stream_set_*) beside one
rule of tests/stream_ref.py per member; the set analogue of
stream_harness.Harness, test infrastructure only.

demux_deliver is the statement of what a set call means: every member's rule
sees the subsequence of the batch that conn_of gives it, in batch order, a
packet of no connection gets a zero row, and a fatal segment's err_packet is
its index in the batch.  After every deliver and every read SetHarness
compares, for every member, all statuses, every field of the record,
ordered_segments and the whole window (pre-filled with a sentinel).  finish()
tiles every uncovered byte of every member with fresh segments, so that a
claim, contested, C or S bit left anywhere shows.

deliver / read / finish take `members`: the subset whose windows are copied
out and compared (statuses, n_read, eof and the destination buffer are always
compared in whole), for sets too large to copy out window by window.
expected_wblocks / expected_rblocks restate the per-connection grid sizes, so
that a test can assert that its shape is the shape it claims.
"""
import numpy as np
import torch

import stream_ref as sr
from stream_harness import SENTINEL, _place, build_batch
from ugo_amd import fec

NO_CONN = fec.STREAM_NO_CONN


def demux_deliver(rules, packets, conn_of, count_contested=True):
    """The batch through the members' rules.  Returns (rows, contested): the
    expected seg_status row per batch packet, and per member the number of
    segments the ordered pass has to see (None where it was not counted)."""
    nconn = len(rules)
    assert len(conn_of) == len(packets)
    mine = [[] for _ in rules]
    for i, c in enumerate(conn_of):
        if 0 <= c < nconn:
            mine[c].append(i)
    rows = [[sr.NONE] * len(p.segs) for p in packets]
    contested = [0] * nconn
    for c, rule in enumerate(rules):
        if not mine[c]:
            continue                       # no packet of this call: the record stays as it is
        before = rule.err
        got = rule.deliver([packets[i] for i in mine[c]], count_contested=count_contested)
        for i, row in zip(mine[c], got):
            rows[i] = row
        contested[c] = rule.contested
        if before == sr.NONE and rule.err == sr.OVERLAP:
            rule.err_packet = mine[c][rule.err_packet]     # reported by batch index
    return rows, contested


# The per-connection grid sizes of a set, restated from stream_set_wblocks /
# stream_set_rblocks (ugo_amd/csrc/stream_kernels.hip).  Used only to assert
# that a test's shape reaches the branch it names; not an oracle for the device.
def expected_wblocks(max_cap):
    """Blocks per connection of k_apply<Many> / k_scan<Many>: four bitmap words a thread."""
    return max(1, min(-(-max_cap // 65536), 1024))


def expected_rblocks(max_cap, nconn):
    """Blocks per connection of k_read<Many>: four 16-B chunks a thread, the grid near 4,096 blocks."""
    by_window = -(-max_cap // 16384)
    by_grid = 1 if nconn >= 4096 else 4096 // nconn
    return max(1, min(by_window, by_grid, 2048))


def interleave(rng, lists):
    """One batch out of per-connection packet lists: a seeded random merge that
    keeps every connection's own order.  Returns (packets, conn_of)."""
    order = np.concatenate([np.full(len(l), c, np.int64) for c, l in enumerate(lists)]) if lists else np.zeros(0, int)
    rng.shuffle(order)
    at = [0] * len(lists)
    packets = []
    for c in order:
        packets.append(lists[c][at[c]])
        at[c] += 1
    return packets, [int(c) for c in order]


def conn_tensor(conn_of, where="device"):
    arr = np.asarray(conn_of, np.int64).astype(np.uint32).view(np.int32)
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return t.pin_memory() if where == "pinned" else t.cuda()


class SetHarness:
    """caps: the members' window sizes.  rxs: existing windows to build the set
    over (then `rules` are their states, default fresh ones)."""

    def __init__(self, enc, caps, slot=256, max_segments=4, pad=None, rxs=None, rules=None):
        self.caps = list(caps)
        self.own = rxs is None
        self.rxs = [fec.StreamRx(enc, cap) for cap in self.caps] if rxs is None else list(rxs)
        self.slot, self.max_segments, self.pad = slot, max_segments, pad
        self.calls = 0
        if rules is None:
            self.rules = [sr.RuleRx(cap, SENTINEL) for cap in self.caps]
            for rx in self.rxs:
                rx.window().fill_(SENTINEL)
        else:
            self.rules = list(rules)
        self.ordered = [0] * len(self.rxs)
        self.set = fec.StreamRxSet(enc, self.rxs)
        self.nconn = len(self.rxs)

    def close(self):
        self.set.close()
        if self.own:
            for rx in self.rxs:
                rx.close()

    def check(self, members=None):
        states = self.set.states()
        assert states.shape == (self.nconn,)
        for c in (range(self.nconn) if members is None else members):
            want = self.rules[c].record()
            got = {k: int(states[c][k]) for k in want}
            assert got == want, (c, got, want)
            assert int(states[c]["ordered_segments"]) == self.ordered[c], (c, int(states[c]["ordered_segments"]))
            win = self.rxs[c].window().cpu().numpy()
            bad = np.flatnonzero(win != self.rules[c].W)
            assert bad.size == 0, f"window of member {c} differs at {bad[:8]} (of {bad.size})"
        return states

    def deliver(self, packets, conn_of, data_off=None, ordered="count", slot=None, max_segments=None,
                inputs="device", outputs="device", conn_where=None, raw=None, status_shift=0, pkts_guard=(0, 0),
                pad_room=None, members=None):
        """ordered: "count" -- every member's ordered_segments must grow by
        exactly its rule's contested count; a list -- by exactly that per
        member; None -- read back.  inputs / outputs / conn_where: "device" or
        "pinned".  raw, pkts_guard, pad_room: as in stream_harness.Harness.deliver
        -- (pkts, info, segs) numpy arrays used as they are, `packets` being what
        the rules are to see.  status_shift: seg_status starts that many bytes
        past a 256-B boundary.  members: whose windows to compare (default all)."""
        self.calls += 1
        slot = self.slot if slot is None else slot
        ms = self.max_segments if max_segments is None else max_segments
        pad = None if self.pad is None else self.pad[:slot]
        pkts, info, segs = raw if raw is not None else build_batch(packets, slot, ms, pad, data_off, seed=self.calls)
        npk = len(packets)
        dp = _place(pkts, inputs)[pkts_guard[0]:pkts_guard[0] + npk]
        assert tuple(dp.shape) == (npk, slot) and npk + sum(pkts_guard) == len(pkts) and segs.shape == (npk, ms)
        if pad_room is not None:
            dpad = _place(pad_room, inputs)[:slot]
        else:
            dpad = None if pad is None else _place(pad, inputs)
        di = _place(info.view(np.uint8).reshape(npk, 64), inputs)
        ds = _place(segs.view(np.uint8).reshape(npk, ms, 16), inputs)
        dc = conn_tensor(conn_of, inputs if conn_where is None else conn_where)
        n = npk * ms
        room = torch.full((n + 512,), 0x77, dtype=torch.uint8)
        room = room.pin_memory() if outputs == "pinned" else room.cuda()
        assert 0 <= status_shift < 256
        at = (-room.data_ptr()) % 256 + status_shift
        status = room[at:at + n].view(npk, ms)
        assert status.data_ptr() % 256 == status_shift and status.is_contiguous()
        self.set.deliver(dp, di, ds, dc, pad=dpad, out=status)
        want, contested = demux_deliver(self.rules, packets, conn_of, count_contested=ordered == "count")
        states = self.set.states()                              # waits for the call
        whole = room.cpu().numpy()
        got = whole[at:at + n].reshape(npk, ms)
        assert (whole[:at] == 0x77).all() and (whole[at + n:] == 0x77).all()   # nothing around seg_status
        exp = np.zeros_like(got)
        for i, row in enumerate(want):
            exp[i, :len(row)] = row
        assert np.array_equal(got, exp), (np.argwhere(got != exp)[:8], got[got != exp][:8], exp[got != exp][:8])
        for c in range(self.nconn):
            if ordered == "count":
                self.ordered[c] += contested[c]
            elif ordered is None:
                self.ordered[c] = int(states[c]["ordered_segments"])
            else:
                self.ordered[c] += ordered[c]
        self.check(members)
        return got

    def read(self, ns, discard=False, shifts=None, guard=48, where="device", members=None):
        """One set_read: ns[c] bytes of member c.  Member c's bytes go to a place
        of their own in one sentinel-filled buffer, shifts[c] bytes past a 16-B
        boundary and at least `guard` bytes from its neighbours; every byte of
        that buffer outside the bytes read must come back untouched.  Returns
        [(data, eof)] per member."""
        return self.reads([ns], discard, [shifts], guard, where, members)[0]

    def reads(self, ns_list, discard=False, shifts_list=None, guard=48, where="device", members=None):
        """Several set_read calls back to back -- no state call, no host wait in
        between -- each compared like a single one once the last has been
        issued; the records and windows are compared after the last."""
        shifts_list = [None] * len(ns_list) if shifts_list is None else shifts_list
        calls = [self._issue_read(ns, discard, shifts, guard, where) for ns, shifts in zip(ns_list, shifts_list)]
        self.set.states()                                      # waits for the calls
        outs = [self._compare_read(*call) for call in calls]
        self.check(members)
        return outs

    def _issue_read(self, ns, discard, shifts, guard, where):
        ns = [int(v) for v in ns]
        assert len(ns) == self.nconn
        shifts = [0] * self.nconn if shifts is None else list(shifts)

        def put(arr):
            t = torch.from_numpy(arr)
            return t.pin_memory() if where == "pinned" else t.cuda()

        dn = put(np.asarray(ns, np.int64))
        n_read = put(np.full(self.nconn, -1, np.int64))
        eof = put(np.full(self.nconn, 0x33, np.uint8))
        room, ats = None, []
        if discard:
            self.set.read(dn, n_read=n_read, eof=eof)
        else:
            size = sum(guard + 32 + v for v in ns) + guard
            room = put(np.full(size, 0x5A, np.uint8))
            base, cur = room.data_ptr(), guard
            for c, v in enumerate(ns):
                cur += (-(base + cur)) % 16 + shifts[c]
                assert (base + cur) % 16 == shifts[c]
                ats.append(cur)
                cur += v + guard
            assert cur <= size
            self.set.read(dn, dst=room, dst_off=put(np.asarray(ats, np.int64)), n_read=n_read, eof=eof)
        return ns, dn, n_read, eof, room, ats

    def _compare_read(self, ns, dn, n_read, eof, room, ats):
        out = []
        for c, v in enumerate(ns):
            out.append((b"", False) if v == 0 else self.rules[c].read(v))   # n == 0 skips the member
        assert dn.cpu().numpy().tolist() == ns                             # n is only read
        got_n, got_eof = n_read.cpu().numpy(), eof.cpu().numpy()
        assert got_n.tolist() == [len(d) for d, _ in out], (got_n.tolist()[:8], [len(d) for d, _ in out][:8])
        assert got_eof.tolist() == [int(e) for _, e in out], (got_eof.tolist()[:8], [int(e) for _, e in out][:8])
        if room is not None:
            got = room.cpu().numpy()
            exp = np.full(got.size, 0x5A, np.uint8)
            for c, (d, _) in enumerate(out):
                exp[ats[c]:ats[c] + len(d)] = np.frombuffer(d, np.uint8)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"read buffer differs at {bad[:8]} (of {bad.size}); members at {ats[:8]}"
        return out

    def finish(self, seed=0, slot=None, ordered="count", members=None):
        """The call after the history: fresh one-segment packets over every
        uncovered byte of every live member's window (of `members` only, where
        given), interleaved, compared like any other call."""
        rng = np.random.default_rng(seed)
        slot = max(self.slot, 256) if slot is None else slot
        assert self.pad is None or len(self.pad) >= slot
        tiled = range(self.nconn) if members is None else set(members)
        lists = [sr.tile_uncovered(r, rng, slot - 16) if r.err == sr.NONE and c in tiled else []
                 for c, r in enumerate(self.rules)]
        packets, conn_of = interleave(rng, lists)
        assert packets
        errs = [r.err for r in self.rules]
        got = self.deliver(packets, conn_of, data_off=lambda i, j: 1 + (i % 15), ordered=ordered, slot=slot,
                           max_segments=1, members=members)
        assert [r.err for r in self.rules] == errs
        return got
