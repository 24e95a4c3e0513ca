"""CPU statements of the send side (include/ugo_stream.h, send windows); test
infrastructure only, written from the Go text.

GoSender   a literal restatement of Conn.Write's hand-over, lenOfDataForWriting
           / getDataForWriting (ugo/conn.go:247-275, 753-779), PopSegments,
           popSegmentsForRetransmission, popNormalSegments, maybeSplitOffFrame
           (ugo/segment_sender.go:18-99) and the loop of Conn.sendPacket
           (ugo/conn.go:521-640) with no ACK and no stop-waiting to send.
RuleTx     THE RULE of the header beside it: one send window with its byte
           model W (stream byte x at W[x & (cap-1)]), its retransmission queue
           and its record; write / release / retransmit / plan.
plan_set / retransmit_set   what a set call means for a list of RuleTx.
"""
import numpy as np

H = 4                      # frameHeaderLen / frameHeaderBytes, segment_sender.go:27,53
RQ_QUEUED, RQ_REJECTED, RQ_FULL, RQ_UNSORTED = 1, 2, 3, 4
NO_CONN = 0xFFFFFFFF
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- the reference, literally
class Segment:
    def __init__(self, offset=0, data=None):
        self.offset, self.data = offset, data

    def dataLen(self):
        return 0 if self.data is None else len(self.data)


def maybeSplitOffFrame(s, n):
    """Removes the first n bytes and returns them as a separate frame; None,
    and nothing modified, if n >= len(frame)."""
    if n >= s.dataLen():
        return None
    out = Segment(s.offset, s.data[:n])
    s.data = s.data[n:]
    s.offset += n
    return out


class GoSender:
    """Conn + segmentSender, the send half.  dataForWriting is None for Go's nil."""

    def __init__(self, writeOffset=0, lastPacketNumber=0):
        self.dataForWriting = None
        self.writeOffset = writeOffset
        self.lastPacketNumber = lastPacketNumber
        self.retransmissionQueue = []

    def Write(self, p):                       # conn.go:252-256; the wait for chWriteDone is the caller's
        self.dataForWriting = bytes(p)

    def AddSegmentForRetransmission(self, seg):
        self.retransmissionQueue.append(seg)

    def lenOfDataForWriting(self):
        return 0 if self.dataForWriting is None else len(self.dataForWriting)

    def getDataForWriting(self, maxBytes):
        if self.dataForWriting is None:
            return None
        if len(self.dataForWriting) > maxBytes:
            ret = self.dataForWriting[:maxBytes]
            self.dataForWriting = self.dataForWriting[maxBytes:]
        else:
            ret = self.dataForWriting
            self.dataForWriting = None
        self.writeOffset += len(ret)
        return ret

    def PopSegments(self, maxLen):
        fs, currentLen = self.popSegmentsForRetransmission(maxLen)
        return fs + self.popNormalSegments(maxLen - currentLen)

    def popSegmentsForRetransmission(self, maxLen):
        res, currentLen = [], 0
        while len(self.retransmissionQueue) > 0:
            seg = self.retransmissionQueue[0]
            frameHeaderLen = 4
            if currentLen + frameHeaderLen > maxLen:
                break
            currentLen += frameHeaderLen
            splitSeg = maybeSplitOffFrame(seg, maxLen - currentLen)
            if splitSeg is not None:
                res.append(splitSeg)
                currentLen += splitSeg.dataLen()
                break
            self.retransmissionQueue = self.retransmissionQueue[1:]
            res.append(seg)
            currentLen += seg.dataLen()
        return res, currentLen

    def popNormalSegments(self, maxBytes):
        frame = Segment()
        currentLen = 0
        frame.offset = self.writeOffset
        frameHeaderBytes = 4
        if currentLen + frameHeaderBytes > maxBytes:
            return []
        maxLen = maxBytes - currentLen - frameHeaderBytes
        data = self.getDataForWriting(maxLen)
        if data is None:
            return []
        frame.data = data
        return [frame]

    def sendPackets(self, budget, maxLen):
        """The loop of sendPacket, at most budget times: [(packet_number,
        [(offset, data)])]."""
        out = []
        for _ in range(budget):
            segments = self.PopSegments(maxLen)
            if len(segments) == 0:
                break
            self.lastPacketNumber += 1
            out.append((self.lastPacketNumber, [(s.offset, s.data) for s in segments]))
        return out


# ---------------------------------------------------------------- THE RULE
def rule_packets(queue, write_pos, tail, last_pn, budget, M, max_segments):
    """THE RULE on plain values.  queue: list of [offset, len], changed in
    place.  Returns (packets, write_pos, last_pn, popped) with packets =
    [(packet_number, [(offset, len, from_queue)])]."""
    out, popped = [], 0
    for _ in range(budget):
        cur, segs = 0, []
        while queue and len(segs) < max_segments:
            if cur + H >= M:
                break
            cur += H
            s = queue[0]
            room = M - cur
            if s[1] > room:
                segs.append((s[0], room, True))
                s[0] += room
                s[1] -= room
                cur += room
                break
            queue.pop(0)
            popped += 1
            segs.append((s[0], s[1], True))
            cur += s[1]
        rem, pending = M - cur, tail - write_pos
        if rem > H and pending > 0 and len(segs) < max_segments:
            n = min(pending, rem - H)
            segs.append((write_pos, n, False))
            write_pos += n
        if not segs:
            break
        last_pn += 1
        out.append((last_pn, segs))
    return out, write_pos, last_pn, popped


class RuleTx:
    """One send window under THE RULE, with the byte model of its window."""

    def __init__(self, cap, rq_cap=64, start_offset=0, start_packet_number=0, fill=0):
        assert cap >= 4096 and cap & (cap - 1) == 0
        self.cap, self.rq_cap = cap, rq_cap
        self.W = np.full(cap, fill, np.uint8)
        self.base = self.write_pos = self.tail = start_offset
        self.last_packet_number = start_packet_number
        self.queue = []                 # [offset, len]
        self.rq_head = 0
        self.packets = self.segments = self.bytes_new = self.bytes_retransmitted = self.rq_rejected = 0

    def record(self):
        return dict(base=self.base, write_pos=self.write_pos, tail=self.tail,
                    last_packet_number=self.last_packet_number, packets=self.packets, segments=self.segments,
                    bytes_new=self.bytes_new, bytes_retransmitted=self.bytes_retransmitted,
                    rq_rejected=self.rq_rejected, rq_len=len(self.queue), rq_head=self.rq_head)

    def write(self, data):
        """Conn.Write that never waits; deviation (d): b"" is a no-op."""
        m = min(len(data), self.cap - (self.tail - self.base))
        if m:
            idx = (self.tail + np.arange(m, dtype=np.uint64)) & np.uint64(self.cap - 1)
            self.W[idx.astype(np.int64)] = np.frombuffer(data[:m], np.uint8)
            self.tail += m
        return m

    def release(self, upto):
        lo = min([upto, self.write_pos] + [q[0] for q in self.queue])
        self.base = max(self.base, lo)

    def retransmit(self, entries):
        """entries: [(offset, len)] of one call, in list order.  Returns the statuses."""
        out, full = [], False
        for o, l in entries:
            if full:
                st = RQ_FULL
            elif l == 0 or l > 0xFFFF or o < self.base or o + l > self.write_pos:
                st = RQ_REJECTED
            elif len(self.queue) == self.rq_cap:
                st, full = RQ_FULL, True
            else:
                self.queue.append([o, l])
                st = RQ_QUEUED
            self.rq_rejected += st != RQ_QUEUED
            out.append(st)
        return out

    def plan(self, budget_eff, M, max_segments):
        """[(packet_number, [(offset, len)])]; an idle member changes nothing."""
        pk, wp, pn, popped = rule_packets(self.queue, self.write_pos, self.tail, self.last_packet_number, budget_eff,
                                          M, max_segments)
        self.write_pos, self.last_packet_number = wp, pn
        self.rq_head = (self.rq_head + popped) % self.rq_cap
        self.packets += len(pk)
        for _, segs in pk:
            self.segments += len(segs)
            self.bytes_new += sum(n for _, n, q in segs if not q)
            self.bytes_retransmitted += sum(n for _, n, q in segs if q)
        return [(pn_, [(o, n) for o, n, _ in segs]) for pn_, segs in pk]

    def holds(self, offset, length):
        """What set_encode accepts of a segment."""
        return self.base <= offset <= self.tail and length <= self.tail - offset

    def stream_bytes(self, offset, length):
        idx = (np.uint64(offset) + np.arange(length, dtype=np.uint64)) & np.uint64(self.cap - 1)
        return self.W[idx.astype(np.int64)].tobytes()


def budgets_eff(budgets, max_packets):
    out, before = [], 0
    for b in budgets:
        out.append(min(b, max(0, max_packets - before)))
        before += b
    return out


def plan_set(rules, budgets, M, max_segments, max_packets):
    """The set call: (packets, first_packet, n_packets) with packets =
    [(conn, packet_number, [(offset, len)])] in batch order."""
    packets, first, counts = [], [], []
    for c, (r, b) in enumerate(zip(rules, budgets_eff(budgets, max_packets))):
        pk = r.plan(b, M, max_segments)
        first.append(len(packets))
        counts.append(len(pk))
        packets += [(c, pn, segs) for pn, segs in pk]
    assert len(packets) <= max_packets
    return packets, first, counts


def retransmit_set(rules, entries):
    """entries: [(conn, offset, len)].  Returns the statuses."""
    conns = [e[0] for e in entries]
    if any(b < a for a, b in zip(conns, conns[1:])):
        return [RQ_UNSORTED] * len(entries)
    out = [None] * len(entries)
    for c in sorted(set(conns)):
        idx = [j for j, e in enumerate(entries) if e[0] == c]
        if not 0 <= c < len(rules):
            st = [RQ_REJECTED] * len(idx)
        else:
            st = rules[c].retransmit([(entries[j][1], entries[j][2]) for j in idx])
        for j, s in zip(idx, st):
            out[j] = s
    return out
