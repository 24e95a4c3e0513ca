"""The sender's half of ARQ twice over; test infrastructure only.

GoSender  a literal restatement of ugo/packet_sender.go and ugo/stop_waiting.go
          (packetSender without congestion control and RTT filter): one call
          per packet, in arrival order, the reference's own loops.
RuleSent  THE RULE of include/ugo_sent.h for one member, stated on a dict of
          slots and plain interval lists -- not the device's difference rings.
The *_set functions apply a call to one RuleSent per member as the entry points
of a set do, and return what the device must have written.
"""
import bisect

import numpy as np

M64 = (1 << 64) - 1
NO_CONN = 0xffffffff
PKT_OK = 0
THRESHOLD = 3                       # retransmissionThreshold
TOO_MANY_TRACKED = 1
IN_FLIGHT, QUEUED = 0, 1
RTO_DEFAULT_US, RTO_MIN_US, RTO_MAX_US = 500_000, 200_000, 60_000_000
ACK_FLAG, STOP_FLAG = 0x80, 0x40


class Ack:
    """A SACK as the sender sees it.  ranges: [(first, last)] highest first,
    as packet_decode stores them (the receiver's last row is {lio, lio})."""

    def __init__(self, la, lio, ranges=(), w=0, delay=0):
        self.la, self.lio, self.ranges, self.w, self.delay = la, lio, list(ranges), w, delay

    def __repr__(self):
        return f"Ack(la={self.la}, lio={self.lio}, ranges={self.ranges}, w={self.w})"


# ------------------------------------------------------------------ the reference, literally
class _GoPacket:
    def __init__(self, n, length, flags=0, segments=()):
        self.packetNumber, self.Length, self.flags, self.segments = n, length, flags, list(segments)
        self.missingCount, self.retransmitted, self.sendTime = 0, False, 0


class GoSender:
    def __init__(self):
        self.lastSentPacketNumber = 0
        self.lastSentPacketTime = 0
        self.largestInOrderAcked = 0
        self.largestAcked = 0
        self.largestReceivedPacketWithAck = 0
        self.packetHistory = {}
        self.largestLeastUnackedSent, self.swState = 0, False      # stopWaitingManager
        self.retransmissionQueue = []
        self.bytesInFlight = 0
        self.totalAcked = 0
        self.consecutiveRTOCount = 0

    def ackPacket(self, n):
        if n != 0:
            packet = self.packetHistory.get(n)
            if packet is not None and not packet.retransmitted:
                self.bytesInFlight -= packet.Length
                self.totalAcked += packet.Length
            if self.largestInOrderAcked == n - 1:
                self.largestInOrderAcked += 1
                self.largestLeastUnackedSent = self.largestInOrderAcked + 1
            self.packetHistory.pop(n, None)
            return packet
        return None

    def nackPacket(self, n):
        packet = self.packetHistory.get(n)
        if packet is None:
            return None
        packet.missingCount += 1
        if packet.missingCount > THRESHOLD and not packet.retransmitted:
            self.queuePacketForRetransmission(packet)
            return packet
        return None

    def queuePacketForRetransmission(self, packet):
        self.bytesInFlight -= packet.Length
        self.retransmissionQueue.append(packet)
        packet.retransmitted = True
        if packet.packetNumber == self.largestInOrderAcked + 1:
            self.largestInOrderAcked += 1
            i = self.largestInOrderAcked + 1
            while i <= self.largestAcked:
                if i not in self.packetHistory:
                    self.largestInOrderAcked = i
                else:
                    break
                i += 1
        self.largestLeastUnackedSent, self.swState = self.largestInOrderAcked + 1, True   # SetBoundary

    def sentPacket(self, packet, now=0):
        if packet.flags != ACK_FLAG:
            if packet.packetNumber in self.packetHistory:
                return "errDuplicatePacketNumber"
            self.lastSentPacketTime = now
            packet.sendTime = now
            if packet.Length == 0:
                return "empty"
            self.lastSentPacketNumber = packet.packetNumber
            self.bytesInFlight += packet.Length
            self.packetHistory[packet.packetNumber] = packet
        return None

    def receivedAck(self, ack, withPacketNumber):
        """Returns (error, acked numbers, lost numbers)."""
        if ack.la > self.lastSentPacketNumber:
            return "errAckForUnsentPacket", [], []
        if withPacketNumber != 0 and withPacketNumber <= self.largestReceivedPacketWithAck:
            return "errDuplicateOrOutOfOrderAck", [], []
        if withPacketNumber != 0:
            self.largestReceivedPacketWithAck = withPacketNumber
        if ack.la <= self.largestInOrderAcked:
            return None, [], []
        if ack.la <= self.largestAcked:
            return None, [], []
        self.largestAcked = ack.la
        if self.largestAcked in self.packetHistory:
            self.consecutiveRTOCount = 0
        acked, lost = [], []
        for i in range(self.largestInOrderAcked, ack.lio):
            p = self.ackPacket(i)
            if p is not None:
                acked.append(p.packetNumber)
        idx = 0
        rr = ack.ranges
        for i in range(ack.lio, ack.la + 1):
            if rr:
                r = rr[len(rr) - 1 - idx]
                if i > r[1] and idx < len(rr) - 1:
                    idx += 1
                    r = rr[len(rr) - 1 - idx]
                if i >= r[0]:
                    p = self.ackPacket(i)
                    if p is not None:
                        acked.append(p.packetNumber)
                else:
                    p = self.nackPacket(i)
                    if p is not None:
                        lost.append(p.packetNumber)
            else:
                p = self.ackPacket(i)
                if p is not None:
                    acked.append(p.packetNumber)
        return None, acked, lost

    def dequeuePacketForRetransmission(self):
        while self.retransmissionQueue:
            packet = self.retransmissionQueue.pop()
            if packet.packetNumber not in self.packetHistory:
                continue
            del self.packetHistory[packet.packetNumber]
            return packet
        return None

    def drain_all(self):
        out = []
        while True:
            p = self.dequeuePacketForRetransmission()
            if p is None:
                return sorted(out)
            out.append(p.packetNumber)

    def getRTO(self, delay):
        rto = delay or RTO_DEFAULT_US
        rto = max(rto, RTO_MIN_US)
        rto *= 1 << self.consecutiveRTOCount
        return min(rto, RTO_MAX_US)

    def checkRTO(self, delay, now):
        if self.lastSentPacketTime == 0 or now < self.lastSentPacketTime + self.getRTO(delay):
            return None
        for p in range(self.largestInOrderAcked + 1, self.lastSentPacketNumber + 1):
            packet = self.packetHistory.get(p)
            if packet is not None and not packet.retransmitted:
                self.queuePacketForRetransmission(packet)
                self.lastSentPacketTime = now
                self.consecutiveRTOCount += 1
                return p
        return None

    def GetStopWaitingFrame(self):
        if self.swState:
            self.swState = False
            return self.largestLeastUnackedSent
        return 0

    def view(self):
        """What the families compare: largest_acked, largest_with_ack,
        bytes_in_flight, the tracked numbers with their missing, lio."""
        return (self.largestAcked, self.largestReceivedPacketWithAck, self.bytesInFlight,
                sorted((n, p.missingCount) for n, p in self.packetHistory.items()), self.largestInOrderAcked)


# ------------------------------------------------------------------ THE RULE
class RuleSent:
    FIELDS = ("last_sent", "lio", "largest_acked", "largest_with_ack", "least_unacked", "bytes_in_flight",
              "last_sent_us", "scan_from", "acked_packets", "acked_bytes", "lost_packets", "lost_bytes", "duplicates",
              "unsent_acks", "stale", "tracked", "queued", "queued_segments", "rto_count", "sw_pending", "err")
    EVENT_FIELDS = ("rtt_us", "delay_us", "acked_bytes", "lost_bytes", "bytes_in_flight", "largest_acked",
                    "acked_packets", "lost_packets", "accepted", "has_rtt")

    def __init__(self, ws=1024, seg_cap=8):
        assert ws >= 1024 and ws & (ws - 1) == 0 and 1 <= seg_cap <= 16
        self.ws, self.seg_cap = ws, seg_cap
        self.slots = {}                        # n -> dict(sent_us, len, state, missing, segs, bits)
        self.at = {}                           # ring position -> its occupant
        self.seg_ring = np.zeros((ws, seg_cap, 2), np.uint64)      # {offset, len}: a freed slot's row stays
        self.last_sent = self.lio = self.largest_acked = self.largest_with_ack = 0
        self.least_unacked = self.bytes_in_flight = self.last_sent_us = 0
        self.scan_from = 1
        self.acked_packets = self.acked_bytes = self.lost_packets = self.lost_bytes = 0
        self.duplicates = self.unsent_acks = self.stale = 0
        self.rto_count = self.sw_pending = self.err = 0

    # -------------------------------------------------------------- views
    @property
    def tracked(self):
        return len(self.slots)

    @property
    def queued(self):
        return sum(1 for s in self.slots.values() if s["state"] == QUEUED)

    @property
    def queued_segments(self):
        return sum(len(s["segs"]) for s in self.slots.values() if s["state"] == QUEUED)

    def record_fields(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def slot_ring(self, dtype):
        out = np.zeros(self.ws, dtype)
        for n, s in self.slots.items():
            o = out[n & (self.ws - 1)]
            assert o["packet_number"] == 0, "two numbers in one slot"
            o["packet_number"], o["sent_us"], o["len"], o["state"] = n, s["sent_us"], s["len"], s["state"]
            o["missing"], o["n_segments"], o["bits"] = s["missing"], len(s["segs"]), s["bits"]
            o["min_offset"] = min((off for off, _ in s["segs"]), default=M64)
        return out

    def view(self):
        return (self.largest_acked, self.largest_with_ack, self.bytes_in_flight,
                sorted((n, s["missing"]) for n, s in self.slots.items()), self.lio)

    def _lowest(self):
        return min(self.slots) if self.slots else self.last_sent + 1

    def _advance(self):
        flying = [n for n, s in self.slots.items() if s["state"] == IN_FLIGHT and n > self.lio]
        self.lio = min(flying) - 1 if flying else self.last_sent
        self.least_unacked = self.lio + 1

    # -------------------------------------------------------------- record
    def record(self, pkts, now_us):
        """pkts: [(n, wire_len, flags, stop_waiting, [(offset, len)])] of the
        packets that pass the tests on conn_of, number, status and wire_lens,
        in batch order."""
        if self.err:
            return
        if pkts and self.last_sent == 0 and self.lio == 0:          # adopt the first numbers
            m = min(p[0] for p in pkts)
            self.lio, self.least_unacked, self.scan_from = m - 1, m, m
        lio = self.lio
        stored = False
        for n, length, flags, sw, segs in pkts:
            if n <= lio:
                self.stale += 1
            elif n > lio + self.ws:
                self.err = TOO_MANY_TRACKED
            elif n in self.slots:
                self.duplicates += 1
            elif n & (self.ws - 1) in self.at:             # held by another number
                self.err = TOO_MANY_TRACKED
            else:
                segs = list(segs)[:self.seg_cap]
                self.slots[n] = dict(sent_us=now_us, len=length, state=IN_FLIGHT, missing=0, segs=segs,
                                     bits=(0x80 if flags & 0x80 else 0) | (0x40 if sw else 0))
                self.at[n & (self.ws - 1)] = n
                row = self.seg_ring[n & (self.ws - 1)]
                row[:] = 0
                for j, (off, ln) in enumerate(segs):
                    row[j] = (off, ln)
                self.bytes_in_flight += length
                self.last_sent = max(self.last_sent, n)
                stored = True
        if stored:
            self.last_sent_us = now_us

    def _free(self, n):
        del self.at[n & (self.ws - 1)]
        return self.slots.pop(n)

    # -------------------------------------------------------------- ack
    @staticmethod
    def covers(a, floor):
        """What ACK a acknowledges at or above floor: disjoint (lo, hi) lists."""
        if not a.ranges:
            return [(floor, a.la)] if floor <= a.la else []
        out = []
        minf = a.la + 1
        for f, l in a.ranges:
            if minf == 0:
                break
            hi, lo = min(l, minf - 1), max(f, floor)
            if lo <= hi:
                out.append((lo, hi))
            minf = min(minf, f)
        if minf != 0:
            hi = min(a.lio, minf - 1)
            if floor <= hi:
                out.append((floor, hi))
        return out

    def ack(self, acks, now_us):
        """acks: the member's ACKs of the call in batch order (status OK, the
        flag set, rows clamped).  Returns the event row as a dict."""
        ev = dict.fromkeys(self.EVENT_FIELDS, 0)
        if not self.err:
            self._ack(acks, now_us, ev)
        ev["bytes_in_flight"], ev["largest_acked"] = self.bytes_in_flight, self.largest_acked
        return ev

    def _ack(self, acks, now_us, ev):
        lwa0, thr = self.largest_with_ack, max(self.largest_acked, self.lio)
        accepted = {}
        for a in acks:
            if a.la > self.last_sent:
                self.unsent_acks += 1
                continue
            if a.w != 0 and a.w <= lwa0:
                continue
            self.largest_with_ack = max(self.largest_with_ack, a.w)
            if a.la > thr and a.la not in accepted:
                accepted[a.la] = a
        if not accepted:
            return
        lam = self.largest_acked = max(accepted)
        ev["accepted"] = 1
        if lam in self.slots:
            ev["has_rtt"], ev["rtt_us"] = 1, max(0, now_us - self.slots[lam]["sent_us"])
            ev["delay_us"] = accepted[lam].delay
            self.rto_count = 0
        floor = min(self.slots) if self.slots else lam + 1
        las = sorted(accepted)
        cov = []
        for la in las:
            iv = sorted(self.covers(accepted[la], floor))
            cov.append(([lo for lo, _ in iv], [hi for _, hi in iv]))
        for n in sorted(m for m in self.slots if m <= lam):
            s = self.slots[n]
            first = bisect.bisect_left(las, n)             # the accepted ACKs with n <= la
            acked = nacks = 0
            for k in range(first, len(las)):
                los, his = cov[k]
                j = bisect.bisect_right(los, n) - 1
                if j >= 0 and his[j] >= n:
                    acked += 1
                else:
                    nacks += 1
            if acked:
                self._free(n)
                ev["acked_packets"] += 1
                ev["acked_bytes"] += s["len"]
                if s["state"] == IN_FLIGHT:
                    self.bytes_in_flight -= s["len"]
            else:
                s["missing"] = min(255, s["missing"] + nacks)
                if s["missing"] > THRESHOLD and s["state"] == IN_FLIGHT:
                    s["state"] = QUEUED
                    self.bytes_in_flight -= s["len"]
                    self.sw_pending = 1
                    ev["lost_packets"] += 1
                    ev["lost_bytes"] += s["len"]
        self.acked_packets += ev["acked_packets"]
        self.acked_bytes += ev["acked_bytes"]
        self.lost_packets += ev["lost_packets"]
        self.lost_bytes += ev["lost_bytes"]
        self._advance()
        self.scan_from = self._lowest()

    # -------------------------------------------------------------- rto
    def rto_us(self, delay_us):
        rto = delay_us or RTO_DEFAULT_US
        rto = max(min(rto, RTO_MAX_US), RTO_MIN_US)
        return min(rto << min(self.rto_count, 16), RTO_MAX_US)

    def rto(self, delay_us, now_us):
        if self.err or self.last_sent_us == 0 or now_us < self.last_sent_us + self.rto_us(delay_us):
            return 0
        flying = [n for n, s in self.slots.items() if s["state"] == IN_FLIGHT and self.lio < n <= self.last_sent]
        if not flying:
            return 0
        s = self.slots[min(flying)]
        s["state"] = QUEUED
        self.bytes_in_flight -= s["len"]
        self.lost_packets += 1
        self.lost_bytes += s["len"]
        self.sw_pending = 1
        self._advance()
        self.last_sent_us = now_us
        self.rto_count += 1
        return 1

    # -------------------------------------------------------------- drain, attach
    def drain(self):
        """Every queued slot leaves.  Returns ([n], [(offset, len)], touch)."""
        ns = sorted(n for n, s in self.slots.items() if s["state"] == QUEUED)
        entries, touch = [], 0
        for n in ns:
            s = self._free(n)
            entries += s["segs"]
            touch |= 1 if s["bits"] & 0x80 else 0
            if s["bits"] & 0x40:
                self.sw_pending = 1
        return ns, entries, touch

    def upto(self):
        return min((off for s in self.slots.values() for off, _ in s["segs"]), default=M64)

    def attach(self, have_packet):
        """(attached, the stop-waiting written)."""
        if self.err or not self.sw_pending or not have_packet:
            return 0, 0
        self.sw_pending = 0
        return 1, self.least_unacked


# ------------------------------------------------------------------ sets
def record_set(rules, packets, now_us):
    """packets: [(conn_of, n, wire_len, status, flags, stop_waiting, [(offset,
    len)])] in batch order, the segments already cut to max_segments."""
    per = [[] for _ in rules]
    for c, n, length, status, flags, sw, segs in packets:
        if c < len(rules) and n != 0 and status == 0 and length != 0:
            per[c].append((n, length, flags, sw, segs))
    for r, p in zip(rules, per):
        r.record(p, now_us)


def ack_set(rules, packets, now_us, max_ranges):
    """packets: [(status, conn_of, flags, Ack, n_ranges)] in batch order; the
    Ack's ranges are the rows stored, n_ranges what the descriptor says."""
    per = [[] for _ in rules]
    for status, c, flags, a, nr in packets:
        if status == PKT_OK and flags & 0x80 and c < len(rules):
            per[c].append(Ack(a.la, a.lio, a.ranges[:min(nr, max_ranges)], a.w, a.delay))
    return [r.ack(p, now_us) for r, p in zip(rules, per)]


def rto_set(rules, delays, now_us):
    return [r.rto(d, now_us) for r, d in zip(rules, delays)]


def drain_set(rules, max_entries):
    """Returns (conn_of, offset, len lists of the entries written, touch, upto)."""
    conn, off, ln, touch, upto = [], [], [], [], []
    start = 0
    for c, r in enumerate(rules):
        if r.err:
            touch.append(0)
            upto.append(0)
            continue
        count = r.queued_segments
        t = 0
        if r.queued and start + count <= max_entries:
            _, entries, t = r.drain()
            assert len(entries) == count
            for o, l in entries:
                conn.append(c)
                off.append(o)
                ln.append(l)
        start += count
        r.scan_from = r._lowest()
        touch.append(t)
        upto.append(r.upto())
    return conn, off, ln, touch, upto


def attach_set(rules, first_packet, n_packets, max_packets):
    """Returns ([(t, stop_waiting)], attached)."""
    writes, attached = [], []
    for r, t, k in zip(rules, first_packet, n_packets):
        did, sw = r.attach(k > 0 and t < max_packets)
        attached.append(did)
        if did:
            writes.append((t, sw))
    return writes, attached
