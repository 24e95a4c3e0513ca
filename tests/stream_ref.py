"""Checker for stream delivery (include/ugo_stream.h); test infrastructure only.

Two restatements, both sequential Python:

* ``LiteralConn``: the reference itself -- segmentSorter with its gap list and
  its map of queued segments (ugo/segment_sorter.go:22-115), Conn.handleSegment
  (ugo/conn.go:473-490) and the Conn.Read loop (ugo/conn.go:149-245) over byte
  strings.  Where Read would wait for data it returns what it has.
* ``RuleRx``: the rule of the header over a window, a coverage bitmap C and a
  start bitmap S, with the record the device keeps.

``gen_history`` constructs histories inside the domain where the two agree
(everything but the header's deviations (a), (b), (c)).
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


# --------------------------------------------------------------- the reference
class LiteralConn:
    def __init__(self):
        self.queued = {}                      # queuedFrames
        self.read_position = 0                # segmentSorter.readPosition
        self.gaps = [[0, MAX_BYTE_COUNT]]     # utils.ByteIntervalList
        self.read_offset = 0                  # Conn.readOffset
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

    def _idx(self, lo, hi):
        return np.arange(lo, hi) & (self.cap - 1)

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

    def _contested_count(self, packets):
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
        cov = self.C[self._idx(rp, self.hi)] if self.hi > rp else np.zeros(0, bool)
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
        ix = self._idx(rp, rp + m)
        data = self.W[ix].tobytes()
        eof = m == self.readable and self.eof
        if m > 0:
            new = rp + m
            partly = m < self.readable and not self.S[new & (cap - 1)]
            starts = np.flatnonzero(self.S[ix])
            if not partly:
                self.head_valid, self.head_off = False, 0
            elif len(starts):
                self.head_valid, self.head_off = True, rp + int(starts[-1])
            self.C[ix] = False
            self.S[ix] = False
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
def gen_history(rng, total_max=3000, seg_max=64, calls=(3, 6), in_batch_dups=False, max_packets=256):
    """A history inside the domain: ('deliver', [Packet]) and ('read', n) steps.

    The stream [0, total) is tiled into segments.  A tile may be sent whole, or
    as a shorter segment at the tile's offset whose remainder follows as a
    segment of its own.  Whatever was sent may be sent again later with the
    same offset and an equal or shorter length.  Tiles go out nearly in order
    (shuffled within runs of 8, so far fewer than 50 gaps ever exist), one
    empty segment closes the stream, reads of random sizes sit between the
    calls.  in_batch_dups: some packets are repeated inside their batch."""
    total = int(rng.integers(200, total_max))
    data = rng.integers(0, 256, total, dtype=np.uint8).tobytes()
    sends = []
    o = 0
    while o < total:
        ln = int(min(total - o, rng.integers(1, seg_max + 1)))
        if ln >= 2 and rng.random() < 0.25:
            short = int(rng.integers(1, ln))
            sends.append([Seg(o, data[o:o + short]), Seg(o + short, data[o + short:o + ln])])
        else:
            sends.append([Seg(o, data[o:o + ln])])
        o += ln
    for k in range(0, len(sends), 8):
        run = sends[k:k + 8]
        rng.shuffle(run)
        sends[k:k + 8] = run
    order = []
    for grp in sends:
        order.extend(grp)
    order.append(Seg(total))
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
