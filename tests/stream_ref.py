"""Checker for stream delivery (include/ugo_stream.h); test infrastructure only.

Two restatements, both sequential Python:

* ``LiteralConn``: the reference itself -- segmentSorter with its gap list and
  its map of queued segments (ugo/segment_sorter.go:22-115), Conn.handleSegment
  (ugo/conn.go:473-490) and the Conn.Read loop (ugo/conn.go:149-245) over byte
  strings.  Where Read would wait for data it returns what it has.
* ``RuleRx``: the rule of the header over a window, a coverage bitmap C and a
  start bitmap S, with the record the device keeps.

``gen_history`` constructs histories inside the domain where the two agree
(everything but the header's deviations (a), (b), (c)), from any base offset;
both restatements can start at such a base (``RuleRx.at``, ``LiteralConn(base)``).
``clamp_segment`` / ``packets_from_raw`` state what the call makes of raw
descriptors, ``tile_uncovered`` builds the call that closes a history, and
``out_of_window_rows`` the offsets of the out-of-window and aliasing table.
"""
import numpy as np

NONE, ACCEPTED, DUPLICATE, OUT_OF_WINDOW, OVERLAP, TOO_MANY_GAPS = range(6)
MAX_GAPS = 50                # MaxStreamFrameSorterGaps
MAX_BYTE_COUNT = (1 << 62) - 1


class Seg:
    """One stream segment as the decoder reports it: `length` declared bytes at
    `offset`, of which data (len(data) = avail <= length) are present; the rest
    read as zero."""

    def __init__(self, offset, data=b"", length=None):
        self.offset = offset
        self.data = bytes(data)
        self.length = len(self.data) if length is None else length
        assert len(self.data) <= self.length

    def body(self):
        return self.data + bytes(self.length - len(self.data))

    def __repr__(self):
        return f"Seg({self.offset}, len={self.length}, avail={len(self.data)})"


class Packet:
    def __init__(self, segs, status=0):
        self.segs = list(segs)
        self.status = status


def clamp_segment(slot, data_off, length, avail):
    """The avail ugo_fec_stream_deliver uses (include/ugo_stream.h): never more
    than the declared length, never past the end of the packet's slot."""
    return min(avail, length, max(0, slot - data_off))


def packets_from_raw(pkts, info, segs, pad=None):
    """The Packet / Seg list the rule sees for raw descriptors, whatever they
    hold: pkts [npk, slot] uint8 (still encrypted), info [npk] and segs [npk,
    max_segments] structured arrays with the decoder's field names.  n_segments
    is clamped to max_segments, avail by clamp_segment, the pad is XORed by
    position in the slot, and what the clamp cut off reads as zeros."""
    npk, slot = pkts.shape
    max_segments = segs.shape[1]
    out = []
    for i in range(npk):
        row = []
        for j in range(min(int(info[i]["n_segments"]), max_segments)):
            o, off, ln, av = (int(segs[i, j][f]) for f in ("offset", "data_off", "len", "avail"))
            av = clamp_segment(slot, off, ln, av)
            body = pkts[i, off:off + av] if av else np.zeros(0, np.uint8)
            if pad is not None and av:
                body = body ^ pad[off:off + av]
            row.append(Seg(o, body.tobytes(), length=ln))
        out.append(Packet(row, status=int(info[i]["status"])))
    return out


# --------------------------------------------------------------- the reference
class LiteralConn:
    def __init__(self, base=0):
        """base: a connection whose first `base` bytes were delivered and read
        in whole segments (nothing queued, one open gap from there)."""
        self.queued = {}                      # queuedFrames
        self.read_position = base             # segmentSorter.readPosition
        self.gaps = [[base, MAX_BYTE_COUNT]]  # utils.ByteIntervalList
        self.read_offset = base               # Conn.readOffset
        self.read_pos_in_frame = 0
        self.eof = False
        self.err = NONE
        self.hit_start_eq_gap_end = False     # the `start == gap.End` fall-through of push was taken

    # segmentSorter.push, line by line
    def push(self, seg):
        if seg.offset in self.queued:
            return DUPLICATE
        start, end = seg.offset, seg.offset + seg.length
        if start == end:
            self.queued[seg.offset] = seg
            return ACCEPTED
        found = False
        i = 0
        while i < len(self.gaps):
            gap = self.gaps[i]
            if end <= gap[0] or start > gap[1]:
                i += 1
                continue
            if start < gap[0]:
                return OVERLAP
            if start < gap[1] and end > gap[1]:
                return OVERLAP
            found = True
            if start == gap[0]:
                if end == gap[1]:
                    del self.gaps[i]
                    break
                if end < gap[1]:
                    gap[0] = end
                    break
            if end == gap[1]:
                gap[1] = start
                break
            if end < gap[1]:
                self.gaps.insert(i + 1, [end, gap[1]])
                gap[1] = start
                break
            self.hit_start_eq_gap_end = True
            i += 1
        if not found:
            return DUPLICATE
        if len(self.gaps) > MAX_GAPS:
            return TOO_MANY_GAPS
        self.queued[seg.offset] = seg
        return ACCEPTED

    def head(self):
        return self.queued.get(self.read_position)

    def pop(self):
        seg = self.head()
        if seg is not None:
            self.read_position += seg.length
            del self.queued[seg.offset]
        return seg

    # Conn.handleSegment behind Conn.run's reset: a duplicate is swallowed, any
    # other error resets the connection and nothing more is handled
    def handle_segment(self, seg):
        if self.err != NONE:
            return NONE
        r = self.push(seg)
        if r in (OVERLAP, TOO_MANY_GAPS):
            self.err = r
        return r

    def deliver(self, packets):
        out = []
        for p in packets:
            if p.status != 0:        # a packet whose decode failed is dropped
                out.append([NONE] * len(p.segs))
                continue
            out.append([self.handle_segment(s) for s in p.segs])
        return out

    # Conn.Read(p[:n]); returns (bytes, io.EOF returned)
    def conn_read(self, n):
        if self.eof:
            return b"", True
        out = bytearray()
        while len(out) < n:
            frame = self.head()
            if frame is None and len(out) > 0:
                return bytes(out), False
            while True:
                if self.err != NONE:
                    break
                if frame is not None:
                    if frame.length == 0:
                        self.eof = True
                        return bytes(out), True
                    if frame.offset + frame.length <= self.read_offset:
                        self.pop()
                        frame = self.head()
                        continue
                    if frame.offset <= self.read_offset:
                        self.read_pos_in_frame = self.read_offset - frame.offset
                        break
                return bytes(out), False      # the reference waits on chRead here
            if frame is None:
                self.eof = True
                return bytes(out), True
            m = min(n - len(out), frame.length - self.read_pos_in_frame)
            out += frame.body()[self.read_pos_in_frame:self.read_pos_in_frame + m]
            self.read_pos_in_frame += m
            self.read_offset += m
            if self.read_pos_in_frame >= frame.length:
                self.pop()
        return bytes(out), False

    def read(self, n):
        """conn_read, with EOF reported as the device reports it: also when the
        next Read would return (0, io.EOF) at once -- the empty segment is at the
        head and p simply had no room left for the loop to see it."""
        data, eof = self.conn_read(n)
        if not eof and self.err == NONE:
            h = self.head()
            eof = h is not None and h.length == 0
        return data, eof


# -------------------------------------------------------------------- the rule
class RuleRx:
    def __init__(self, cap, sentinel=0):
        assert cap >= 4096 and cap & (cap - 1) == 0
        self.cap = cap
        self.W = np.full(cap, sentinel, np.uint8)
        self.C = np.zeros(cap, bool)
        self.S = np.zeros(cap, bool)
        self.read_pos = self.head_off = self.hi = self.readable = 0
        self.head_valid = self.eof = False
        self.ngaps = 1
        self.err = NONE
        self.err_packet = self.err_segment = 0
        self.accepted = self.duplicate = self.out_of_window = self.skipped_packets = 0
        self.contested = 0   # not device state: what the ordered pass must have seen in the last call

    @classmethod
    def at(cls, cap, read_pos, sentinel=0, window=None, **counters):
        """A connection that has delivered and read [0, read_pos) in whole
        segments: nothing covered, nothing queued, hi = read_pos.  window: the
        ring's content (default: the sentinel); counters: accepted, duplicate,
        out_of_window, skipped_packets so far."""
        r = cls(cap, sentinel)
        r.read_pos = r.hi = read_pos
        if window is not None:
            r.W[:] = window
        for k, v in counters.items():
            assert k in ("accepted", "duplicate", "out_of_window", "skipped_packets"), k
            setattr(r, k, v)
        return r

    def _idx(self, lo, hi):
        return np.arange(lo, hi) & (self.cap - 1)

    def _ring(self, arr, lo, hi):
        """arr over stream positions [lo, hi) (hi - lo <= cap), as a copy."""
        a, n = lo & (self.cap - 1), hi - lo
        if a + n <= self.cap:
            return arr[a:a + n].copy()
        return np.concatenate([arr[a:], arr[:a + n - self.cap]])

    def _ring_fill(self, arr, lo, hi, value):
        a, n = lo & (self.cap - 1), hi - lo
        arr[a:min(a + n, self.cap)] = value
        if a + n > self.cap:
            arr[:a + n - self.cap] = value

    def _covered(self, o, e):
        """(any covered, all covered) over [o, e)."""
        lo = max(o, self.read_pos)
        c = self.C[self._idx(lo, e)] if e > lo else np.zeros(0, bool)
        below = o < self.read_pos
        return bool(below or c.any()), bool(c.all())

    def _segment(self, s):
        rp, cap = self.read_pos, self.cap
        o, e = s.offset, s.offset + s.length
        inwin = rp <= o < rp + cap
        if (inwin and self.S[o & (cap - 1)]) or (self.head_valid and o == self.head_off):
            return DUPLICATE
        if s.length == 0:
            if not inwin:
                return OUT_OF_WINDOW
            self.S[o & (cap - 1)] = True
            return ACCEPTED
        if e > rp + cap:
            return OUT_OF_WINDOW
        anyc, allc = self._covered(o, e)
        if not anyc:
            ix = self._idx(o, e)
            self.C[ix] = True
            self.S[o & (cap - 1)] = True
            self.W[ix] = np.frombuffer(s.body(), np.uint8)
            self.hi = max(self.hi, e)
            self._accepted_data = True
            return ACCEPTED
        if allc:
            return DUPLICATE
        return OVERLAP

    def _claimers(self, packets):
        """(ring indices claimed, partly covered) per claimer of the batch, in
        arrival order; see _contested_count_sets."""
        rp, cap = self.read_pos, self.cap
        for p in packets:
            if p.status != 0:
                continue
            for s in p.segs:
                o, e = s.offset, s.offset + s.length
                inwin = rp <= o < rp + cap
                if (inwin and self.S[o & (cap - 1)]) or (self.head_valid and o == self.head_off):
                    continue
                if s.length == 0:
                    if inwin:
                        yield np.array([o & (cap - 1)]), False
                    continue
                if e > rp + cap or e <= rp:
                    continue
                lo = max(o, rp)
                ix = self._idx(lo, e)
                ux = ix[~self.C[ix]]
                if len(ux):
                    yield ux, bool(o < rp or len(ux) != e - lo)

    def _contested_count(self, packets):
        """_contested_count_sets over two byte maps of the ring (claimed once,
        claimed twice) instead of Python sets: the same count, at any size."""
        once, twice = np.zeros(self.cap, bool), np.zeros(self.cap, bool)
        for ux, _ in self._claimers(packets):
            twice[ux] |= once[ux]
            once[ux] = True
        return sum(1 for ux, partly in self._claimers(packets) if partly or twice[ux].any())

    def _contested_count_sets(self, packets):
        """Segments the parallel passes cannot decide (stream_kernels.hip): the
        claimers -- segments with an uncovered byte that are not duplicates by
        the state before the call, and in-window empty segments -- whose claims
        meet another claimer's, and every partly covered segment."""
        rp, cap = self.read_pos, self.cap
        claims = {}
        partly = []
        n = 0
        for p in packets:
            if p.status != 0:
                continue
            for s in p.segs:
                n += 1
                o, e = s.offset, s.offset + s.length
                inwin = rp <= o < rp + cap
                if (inwin and self.S[o & (cap - 1)]) or (self.head_valid and o == self.head_off):
                    continue
                if s.length == 0:
                    if inwin:
                        claims[n] = {o}
                    continue
                if e > rp + cap or e <= rp:
                    continue
                lo = max(o, rp)
                unc = {x for x in range(lo, e) if not self.C[x & (cap - 1)]}
                if not unc:
                    continue
                claims[n] = unc
                if o < rp or len(unc) != e - lo:
                    partly.append(n)
        seen = {}
        hit = set(partly)
        for k, bits in claims.items():
            for x in bits:
                if x in seen:
                    hit.add(k)
                    hit.add(seen[x])
                else:
                    seen[x] = k
        return len(hit)

    def deliver(self, packets, count_contested=False):
        out = []
        if self.err != NONE:
            self.contested = 0
            return [[NONE] * len(p.segs) for p in packets]
        self.contested = self._contested_count(packets) if count_contested else None
        self._accepted_data = False
        fatal = False
        for i, p in enumerate(packets):
            if fatal:
                out.append([NONE] * len(p.segs))
                continue
            if p.status != 0:
                self.skipped_packets += 1
                out.append([NONE] * len(p.segs))
                continue
            row = []
            for j, s in enumerate(p.segs):
                if fatal:
                    row.append(NONE)
                    continue
                r = self._segment(s)
                row.append(r)
                if r == ACCEPTED:
                    self.accepted += 1
                elif r == DUPLICATE:
                    self.duplicate += 1
                elif r == OUT_OF_WINDOW:
                    self.out_of_window += 1
                elif r == OVERLAP:
                    fatal = True
                    self.err, self.err_packet, self.err_segment = OVERLAP, i, j
            out.append(row)
        self._summary()
        return out

    def _summary(self):
        rp, cap = self.read_pos, self.cap
        cov = self._ring(self.C, rp, self.hi) if self.hi > rp else np.zeros(0, bool)
        unc = ~cov
        runs = int(unc[0]) + int(np.count_nonzero(unc[1:] & cov[:-1])) if len(unc) else 0
        self.ngaps = runs + 1
        u = rp + (int(np.argmax(unc)) if unc.any() else len(unc))
        self.readable = u - rp
        self.eof = bool(u - rp < cap and self.S[u & (cap - 1)])
        if self.err == NONE and self._accepted_data and self.ngaps > MAX_GAPS:
            self.err = TOO_MANY_GAPS

    def read(self, n):
        rp, cap = self.read_pos, self.cap
        m = min(n, self.readable)
        data = self._ring(self.W, rp, rp + m).tobytes()
        eof = m == self.readable and self.eof
        if m > 0:
            new = rp + m
            partly = m < self.readable and not self.S[new & (cap - 1)]
            starts = np.flatnonzero(self._ring(self.S, rp, new))
            if not partly:
                self.head_valid, self.head_off = False, 0
            elif len(starts):
                self.head_valid, self.head_off = True, rp + int(starts[-1])
            self._ring_fill(self.C, rp, new, False)
            self._ring_fill(self.S, rp, new, False)
            self.read_pos = new
            self.readable -= m
        return data, eof

    def record(self):
        return {"read_pos": self.read_pos, "head_off": self.head_off, "head_valid": int(self.head_valid),
                "hi": self.hi, "readable": self.readable, "eof": int(self.eof), "ngaps": self.ngaps,
                "err": self.err, "err_packet": self.err_packet, "err_segment": self.err_segment,
                "accepted": self.accepted, "duplicate": self.duplicate, "out_of_window": self.out_of_window,
                "skipped_packets": self.skipped_packets}


# ------------------------------------------------------------------- histories
def gen_history(rng, total_max=3000, seg_max=64, calls=(3, 6), in_batch_dups=False, max_packets=256,
                base=0, total=None, forced=(), fin=True):
    """A history inside the domain: ('deliver', [Packet]) and ('read', n) steps.

    The stream [0, total) is tiled into segments.  A tile may be sent whole, or
    as a shorter segment at the tile's offset whose remainder follows as a
    segment of its own.  Whatever was sent may be sent again later with the
    same offset and an equal or shorter length.  Tiles go out nearly in order
    (shuffled within runs of 8, so far fewer than 50 gaps ever exist), one
    empty segment closes the stream, reads of random sizes sit between the
    calls.  in_batch_dups: some packets are repeated inside their batch.

    base: the stream is [base, base + total) of a connection that starts there
    (RuleRx.at, LiteralConn(base)); data[k] is stream byte base + k.  total: a
    given length.  forced: (start, length) tiles relative to base that are sent
    whole, so that a segment ends, starts or lies across a chosen offset.
    fin=False: no empty segment, the connection stays open."""
    total = int(rng.integers(200, total_max)) if total is None else total
    data = rng.integers(0, 256, total, dtype=np.uint8).tobytes()
    forced = dict(forced)
    sends = []
    o = 0
    while o < total:
        if o in forced:
            ln = forced[o]
            assert o + ln <= total and not any(o < f < o + ln for f in forced)
            sends.append([Seg(base + o, data[o:o + ln])])
            o += ln
            continue
        stop = min([total] + [f for f in forced if f > o])
        ln = int(min(stop - o, rng.integers(1, seg_max + 1)))
        if ln >= 2 and rng.random() < 0.25:
            short = int(rng.integers(1, ln))
            sends.append([Seg(base + o, data[o:o + short]), Seg(base + o + short, data[o + short:o + ln])])
        else:
            sends.append([Seg(base + o, data[o:o + ln])])
        o += ln
    for k in range(0, len(sends), 8):
        run = sends[k:k + 8]
        rng.shuffle(run)
        sends[k:k + 8] = run
    order = []
    for grp in sends:
        order.extend(grp)
    if fin:
        order.append(Seg(base + total))
    # retransmissions: later than the original, same offset, equal or shorter
    k = 0
    while k < len(order):
        s = order[k]
        if rng.random() < 0.15:
            ln = s.length if rng.random() < 0.5 or s.length < 2 else int(rng.integers(1, s.length))
            at = int(rng.integers(k + 1, min(len(order), k + 40) + 1))
            order.insert(at, Seg(s.offset, s.data[:ln]))
        k += 1
    # packets of 1-3 segments
    packets = []
    k = 0
    while k < len(order):
        n = int(rng.integers(1, 4))
        packets.append(Packet(order[k:k + n]))
        k += n
    ncalls = int(rng.integers(calls[0], calls[1] + 1))
    per = max(1, min(max_packets, -(-len(packets) // ncalls)))
    steps = []
    for k in range(0, len(packets), per):
        batch = packets[k:k + per]
        if in_batch_dups and len(batch) > 1:
            for _ in range(int(rng.integers(1, 4))):
                src = int(rng.integers(0, len(batch)))
                at = int(rng.integers(src + 1, len(batch) + 1))
                batch.insert(at, Packet(batch[src].segs))
            batch = batch[:max_packets]
        steps.append(("deliver", batch))
        for _ in range(int(rng.integers(0, 3))):
            steps.append(("read", int(rng.integers(0, 2 * seg_max + 200))))
    steps.append(("read", total + 10))
    steps.append(("read", 5))
    return steps, data


def shift_history(steps, k):
    """The same history k bytes further along the stream."""
    return [(op, [Packet([Seg(s.offset + k, s.data, s.length) for s in p.segs], p.status) for p in arg])
            if op == "deliver" else (op, arg) for op, arg in steps]


def tile_uncovered(rule, rng, seg_max, lo=None, hi=None):
    """Fresh one-segment packets that tile every uncovered byte of [lo, hi)
    (default: the whole window [read_pos, read_pos + cap)) of `rule`, runs in
    ascending order, segments of 1..seg_max bytes."""
    lo = rule.read_pos if lo is None else lo
    hi = rule.read_pos + rule.cap if hi is None else hi
    unc = np.concatenate([[False], ~rule._ring(rule.C, lo, hi), [False]])
    edges = np.flatnonzero(unc[1:] != unc[:-1])
    packets = []
    for a, b in zip(edges[0::2], edges[1::2]):
        o, e = lo + int(a), lo + int(b)
        while o < e:
            n = int(min(e - o, rng.integers(max(1, seg_max // 2), seg_max + 1)))
            packets.append(Packet([Seg(o, rng.integers(0, 256, n, dtype=np.uint8).tobytes())]))
            o += n
    return packets


def out_of_window_rows(read_pos, cap, live, length):
    """The offsets of the out-of-window and aliasing table for one segment
    length: (name, offset) in a fixed order.  live: positions x that hold a
    start or a coverage bit.  Offsets that 64 bits cannot hold are left out."""
    rows = []
    for x in live:
        rows += [(f"x{x}+cap", x + cap), (f"x{x}+2cap", x + 2 * cap), (f"x{x}+2^32", x + (1 << 32))]
        if 0 <= x - cap < read_pos:
            rows.append((f"x{x}-cap", x - cap))
    rows += [("2^63", 1 << 63), ("2^64-1", (1 << 64) - 1), ("2^64-len", (1 << 64) - length),
             ("2^64-len+1", (1 << 64) - length + 1), ("fits", read_pos + cap - length),
             ("fits+1", read_pos + cap - length + 1)]
    return [(n, o) for n, o in rows if o < (1 << 64)]
