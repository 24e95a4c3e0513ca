"""Congestion control twice over; test infrastructure only.

GoCubicSender  a literal restatement of ugo/congestion/cubic_sender.go,
               cubic.go, rtt_stats.go (UpdateRTT) and hybrid_slow_start.go: one
               call per packet, an injectable clock, numpy.float32 where the
               reference computes in float32, 64-bit wrapping where Go wraps,
               numpy.cbrt on float64 for the root.  Durations and times are
               nanoseconds, as time.Duration is.  What ugo never reads (PRR,
               the recent-min samples, connectionStats, Reno) is left out.
RuleCc         THE RULE of include/ugo_cc.h for one member, driven by an event
               row and a cc row.
GoPair / RulePair put them beside sent_ref.GoSender / RuleSent as packetSender
holds its congestion controller.
"""
import numpy as np

import sent_ref as sr

M64 = (1 << 64) - 1
US = 1000                                  # time.Microsecond
f32 = np.float32

DEFAULTS = dict(initial_cwnd=32, max_cwnd=200, min_cwnd=2, num_connections=2, mss=1460)
CUBE_SCALE = 40
CUBE_CWND_SCALE = 410
CUBE_FACTOR = (1 << CUBE_SCALE) // CUBE_CWND_SCALE
BETA, BETA_LAST_MAX = f32(0.7), f32(0.85)
MAX_CUBIC_INTERVAL_US = 30_000
RTT_ALPHA, ONE_MINUS_ALPHA, RTT_BETA, ONE_MINUS_BETA = f32(0.125), f32(0.875), f32(0.25), f32(0.75)
HS_LOW_WINDOW, HS_MIN_SAMPLES, HS_MIN_THR_US, HS_MAX_THR_US = 16, 8, 4000, 16000


def s64(x):
    """A 64-bit pattern as Go's int64."""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def go_div(a, b):
    """Go's signed division truncates toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def beta_n(n):
    return (f32(n) - f32(1) + BETA) / f32(n)


def alpha_n(n):
    b = beta_n(n)
    return f32(3) * f32(n) * f32(n) * (f32(1) - b) / (f32(1) + b)


def icbrt(x):
    """The largest t with t^3 <= x."""
    t = 0
    for b in range(21, -1, -1):
        cand = t | (1 << b)
        if cand ** 3 <= x:
            t = cand
    return t


def cbrt_go(x):
    """uint32(math.Cbrt(float64(x)))"""
    return int(np.cbrt(np.float64(x)))


# ------------------------------------------------------------------ the reference, literally
class GoCubicSender:
    def __init__(self, clock, initial_cwnd=32, max_cwnd=200, num_connections=2, mss=1460, min_cwnd=2):
        self.clock = clock                                  # () -> ns
        self.mss = mss
        # RTTStats
        self.minRTT = self.latestRTT = self.smoothedRTT = self.meanDeviation = 0
        # HybridSlowStart
        self.endPacketNumber = self.hsLastSent = 0
        self.started = self.hystartFound = False
        self.currentMinRTT = self.rttSampleCount = 0
        # cubicSender
        self.largestSentPacketNumber = self.largestAckedPacketNumber = self.largestSentAtLastCutback = 0
        self.congestionWindow = initial_cwnd
        self.slowstartThreshold = max_cwnd
        self.maxTCPCongestionWindow = max_cwnd
        self.minCongestionWindow = min_cwnd
        self.lastCutbackExitedSlowstart = False
        self.numConnections = num_connections
        self.cutbacks = self.rtos = 0                       # counters of the restatement, not the reference's
        self.cubicReset()

    # ---- Cubic
    def cubicReset(self):
        self.epoch = self.appLimitedStartTime = self.lastUpdateTime = None     # time.Time{}
        self.lastCongestionWindow = self.lastMaxCongestionWindow = 0
        self.ackedPacketsCount = 0
        self.estimatedTCPcongestionWindow = self.originPointCongestionWindow = 0
        self.timeToOriginPoint = 0
        self.lastTargetCongestionWindow = 0

    def OnApplicationLimited(self):
        if self.appLimitedStartTime is None:
            self.appLimitedStartTime = self.clock()

    def CongestionWindowAfterPacketLoss(self, cur):
        if cur < self.lastMaxCongestionWindow:
            self.lastMaxCongestionWindow = int(BETA_LAST_MAX * f32(cur))
        else:
            self.lastMaxCongestionWindow = cur
        self.epoch = None
        return int(f32(cur) * beta_n(self.numConnections))

    def CongestionWindowAfterAck(self, cur, delayMin):
        self.ackedPacketsCount = (self.ackedPacketsCount + 1) & 0xffffffff
        now = self.clock()
        if self.lastCongestionWindow == cur and self.lastUpdateTime is not None and \
                now - self.lastUpdateTime <= MAX_CUBIC_INTERVAL_US * US:
            return max(self.lastTargetCongestionWindow, self.estimatedTCPcongestionWindow)
        self.lastCongestionWindow = cur
        self.lastUpdateTime = now
        if self.epoch is None:
            self.epoch = now
            self.ackedPacketsCount = 1
            self.estimatedTCPcongestionWindow = cur
            if self.lastMaxCongestionWindow <= cur:
                self.timeToOriginPoint = 0
                self.originPointCongestionWindow = cur
            else:
                self.timeToOriginPoint = cbrt_go((CUBE_FACTOR * (self.lastMaxCongestionWindow - cur)) & M64)
                self.originPointCongestionWindow = self.lastMaxCongestionWindow
        elif self.appLimitedStartTime is not None:
            self.epoch += now - self.appLimitedStartTime
            self.appLimitedStartTime = None
        elapsed = go_div(s64(go_div(now + delayMin - self.epoch, US) << 10), 1000000)
        offset = self.timeToOriginPoint - elapsed
        delta = (s64(CUBE_CWND_SCALE * offset * offset * offset) >> CUBE_SCALE) & M64
        target = (self.originPointCongestionWindow - delta) & M64
        while True:
            required = int(f32(self.estimatedTCPcongestionWindow) / alpha_n(self.numConnections))
            if self.ackedPacketsCount < required:
                break
            self.ackedPacketsCount -= required
            self.estimatedTCPcongestionWindow += 1
        self.lastTargetCongestionWindow = target
        return max(target, self.estimatedTCPcongestionWindow)

    # ---- RTTStats
    def UpdateRTT(self, sendDelta, ackDelay):
        if sendDelta <= 0:
            return
        if self.minRTT == 0 or self.minRTT > sendDelta:
            self.minRTT = sendDelta
        sample = sendDelta
        if sample > ackDelay:
            sample -= ackDelay
        self.latestRTT = sample
        if self.smoothedRTT == 0:
            self.smoothedRTT = sample
            self.meanDeviation = sample // 2
        else:
            dev = abs(self.smoothedRTT - sample)
            self.meanDeviation = int(ONE_MINUS_BETA * f32(self.meanDeviation // US) + RTT_BETA * f32(dev // US)) * US
            self.smoothedRTT = int(f32(self.smoothedRTT // US) * ONE_MINUS_ALPHA + f32(sample // US) * RTT_ALPHA) * US

    # ---- HybridSlowStart
    def ShouldExitSlowStart(self, latestRTT, minRTT, congestionWindow):
        if not self.started:
            self.endPacketNumber = self.hsLastSent
            self.currentMinRTT = 0
            self.rttSampleCount = 0
            self.started = True
        if self.hystartFound:
            return True
        self.rttSampleCount += 1
        if self.rttSampleCount <= HS_MIN_SAMPLES:
            if self.currentMinRTT == 0 or self.currentMinRTT > latestRTT:
                self.currentMinRTT = latestRTT
        if self.rttSampleCount == HS_MIN_SAMPLES:
            thr = (minRTT // US) >> 3
            thr = min(thr, HS_MAX_THR_US)
            thr = max(thr, HS_MIN_THR_US) * US
            if self.currentMinRTT > minRTT + thr:
                self.hystartFound = True
        return congestionWindow >= HS_LOW_WINDOW and self.hystartFound

    # ---- cubicSender
    def OnPacketSent(self, n):
        self.largestSentPacketNumber = n
        self.hsLastSent = n

    def InRecovery(self):
        return self.largestAckedPacketNumber <= self.largestSentAtLastCutback and self.largestAckedPacketNumber != 0

    def GetCongestionWindow(self):
        return self.congestionWindow * self.mss

    def InSlowStart(self):
        return self.congestionWindow < self.slowstartThreshold

    def OnCongestionEvent(self, rttUpdated, bytesInFlight, acked, lost):
        if rttUpdated and self.InSlowStart() and \
                self.ShouldExitSlowStart(self.latestRTT, self.minRTT, self.GetCongestionWindow() // self.mss):
            self.slowstartThreshold = self.congestionWindow
        for n in lost:
            self.onPacketLost(n)
        for n in acked:
            self.onPacketAcked(n, bytesInFlight)

    def onPacketAcked(self, n, bytesInFlight):
        self.largestAckedPacketNumber = max(n, self.largestAckedPacketNumber)
        if self.InRecovery():
            return
        self.maybeIncreaseCwnd(bytesInFlight)
        if self.InSlowStart() and self.endPacketNumber < n:
            self.started = False

    def onPacketLost(self, n):
        if n <= self.largestSentAtLastCutback:
            return
        self.lastCutbackExitedSlowstart = self.InSlowStart()
        self.congestionWindow = self.CongestionWindowAfterPacketLoss(self.congestionWindow)
        if self.congestionWindow < self.minCongestionWindow:
            self.congestionWindow = self.minCongestionWindow
        self.slowstartThreshold = self.congestionWindow
        self.largestSentAtLastCutback = self.largestSentPacketNumber
        self.cutbacks += 1

    def maybeIncreaseCwnd(self, bytesInFlight):
        if not self.isCwndLimited(bytesInFlight):
            self.OnApplicationLimited()
            return
        if self.congestionWindow >= self.maxTCPCongestionWindow:
            return
        if self.InSlowStart():
            self.congestionWindow += 1
            return
        self.congestionWindow = min(self.maxTCPCongestionWindow,
                                    self.CongestionWindowAfterAck(self.congestionWindow, self.minRTT))

    def isCwndLimited(self, bytesInFlight):
        cw = self.GetCongestionWindow()
        if bytesInFlight >= cw:
            return True
        available = cw - bytesInFlight
        slowStartLimited = self.InSlowStart() and bytesInFlight > cw // 2
        return slowStartLimited or available <= 3 * self.mss

    def OnRetransmissionTimeout(self, packetsRetransmitted):
        self.largestSentAtLastCutback = 0
        if not packetsRetransmitted:
            return
        self.started = self.hystartFound = False            # Restart
        self.cubicReset()
        self.slowstartThreshold = self.congestionWindow // 2
        self.congestionWindow = self.minCongestionWindow
        self.rtos += 1

    def RetransmissionDelay(self):
        if self.smoothedRTT == 0:
            return 0
        return self.smoothedRTT + self.meanDeviation * 4

    def view(self):
        """The fields RuleCc.view() gives, times in whole us (0 = unset)."""
        t = lambda x: 0 if x is None else x // US          # noqa: E731
        return dict(cwnd=self.congestionWindow, ssthresh=self.slowstartThreshold,
                    largest_acked=self.largestAckedPacketNumber, cutback=self.largestSentAtLastCutback,
                    last_cutback_exited_slowstart=int(self.lastCutbackExitedSlowstart),
                    min_rtt_us=self.minRTT // US, latest_rtt_us=self.latestRTT // US, srtt_us=self.smoothedRTT // US,
                    mean_dev_us=self.meanDeviation // US, end_packet_number=self.endPacketNumber,
                    current_min_rtt_us=self.currentMinRTT // US, sample_count=self.rttSampleCount,
                    started=int(self.started), found=int(self.hystartFound), epoch_us=t(self.epoch),
                    app_limited_us=t(self.appLimitedStartTime), last_update_us=t(self.lastUpdateTime),
                    last_cwnd=self.lastCongestionWindow, last_max_cwnd=self.lastMaxCongestionWindow,
                    acked_count=self.ackedPacketsCount, est_tcp_cwnd=self.estimatedTCPcongestionWindow,
                    origin_cwnd=self.originPointCongestionWindow, time_to_origin=self.timeToOriginPoint,
                    last_target_cwnd=self.lastTargetCongestionWindow, cutbacks=self.cutbacks, rtos=self.rtos)


class GoPair:
    """packetSender with its congestion controller: sent_ref.GoSender and a
    GoCubicSender called where packet_sender.go and conn.go call them."""

    def __init__(self, **params):
        self.now_us = 0
        self.go = sr.GoSender()
        self.cc = GoCubicSender(lambda: self.now_us * US, **params)

    def send(self, numbers, length, now_us):
        self.now_us = now_us
        for n in numbers:
            self.go.sentPacket(sr._GoPacket(n, length), now_us)
            self.cc.OnPacketSent(n)

    def ack(self, a, now_us):
        """receivedAck (packet_sender.go:166-257).  Returns (acked, lost)."""
        self.now_us = now_us
        go = self.go
        passes = a.la <= go.lastSentPacketNumber and not (a.w != 0 and a.w <= go.largestReceivedPacketWithAck) and \
            a.la > go.largestInOrderAcked and a.la > go.largestAcked
        packet = go.packetHistory.get(a.la) if passes else None
        err, acked, lost = go.receivedAck(a, a.w)
        if not passes:
            return [], []
        rtt_updated = packet is not None
        if rtt_updated:
            self.cc.UpdateRTT((now_us - packet.sendTime) * US, a.delay * US)
        self.cc.OnCongestionEvent(rtt_updated, go.bytesInFlight, acked, lost)
        return acked, lost

    def rto(self, now_us):
        """checkRTO (packet_sender.go:314-340) with getRTO's RetransmissionDelay."""
        self.now_us = now_us
        go = self.go
        delay = self.cc.RetransmissionDelay() // US
        if go.lastSentPacketTime == 0 or now_us < go.lastSentPacketTime + go.getRTO(delay):
            return None
        for p in range(go.largestInOrderAcked + 1, go.lastSentPacketNumber + 1):
            packet = go.packetHistory.get(p)
            if packet is not None and not packet.retransmitted:
                self.cc.OnCongestionEvent(False, go.bytesInFlight, [], [p])
                self.cc.OnRetransmissionTimeout(True)
                break
        return go.checkRTO(delay, now_us)

    def budget(self, packet_bytes, max_budget):
        """The loop of conn.go:546-551: CongestionAllowsSending before every
        packet, for packets of packet_bytes each."""
        bif, k = self.go.bytesInFlight, 0
        while k < max_budget and bif <= self.cc.GetCongestionWindow():
            k += 1
            bif += packet_bytes
        return k


# ------------------------------------------------------------------ THE RULE
class RuleCc:
    FIELDS = ("cwnd", "ssthresh", "largest_acked", "cutback", "min_rtt_us", "latest_rtt_us", "srtt_us",
              "mean_dev_us", "end_packet_number", "current_min_rtt_us", "epoch_us", "app_limited_us",
              "last_update_us", "last_cwnd", "last_max_cwnd", "est_tcp_cwnd", "origin_cwnd", "last_target_cwnd",
              "rto_candidate", "cutbacks", "rtos", "sample_count", "acked_count", "time_to_origin",
              "last_cutback_exited_slowstart", "started", "found")
    ROW_FIELDS = ("max_lost", "max_acked", "acked_le")

    def __init__(self, per_packet=False, **params):
        p = dict(DEFAULTS, **params)
        assert 1 <= p["min_cwnd"] <= p["initial_cwnd"] <= p["max_cwnd"] <= 1 << 20
        assert p["num_connections"] >= 1 and p["mss"] >= 1
        self.p = p
        self.per_packet = per_packet        # every step of maybeIncreaseCwnd in turn, no shortcut
        self.steps = 0                      # rounds of grow(): what must not grow with G
        for k in self.FIELDS:
            setattr(self, k, 0)
        self.cwnd, self.ssthresh = p["initial_cwnd"], p["max_cwnd"]

    def view(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def in_slow_start(self):
        return self.cwnd < self.ssthresh

    # -------------------------------------------------------------- Cubic
    def _after_loss(self):
        if self.cwnd < self.last_max_cwnd:
            self.last_max_cwnd = int(BETA_LAST_MAX * f32(self.cwnd))
        else:
            self.last_max_cwnd = self.cwnd
        self.epoch_us = 0
        return int(f32(self.cwnd) * beta_n(self.p["num_connections"]))

    def _loss_reaction(self, last_sent):
        self.last_cutback_exited_slowstart = int(self.in_slow_start())
        self.cwnd = max(self._after_loss(), self.p["min_cwnd"])
        self.ssthresh = self.cwnd
        self.cutback = last_sent
        self.cutbacks += 1

    def _after_ack(self, now):
        """(the window, whether the step took the 30-ms return)"""
        self.acked_count = (self.acked_count + 1) & 0xffffffff
        if self.last_cwnd == self.cwnd and self.last_update_us != 0 and \
                s64(now - self.last_update_us) <= MAX_CUBIC_INTERVAL_US:
            return max(self.last_target_cwnd, self.est_tcp_cwnd), True
        self.last_cwnd, self.last_update_us = self.cwnd, now
        if self.epoch_us == 0:
            self.epoch_us, self.acked_count, self.est_tcp_cwnd = now, 1, self.cwnd
            if self.last_max_cwnd <= self.cwnd:
                self.time_to_origin, self.origin_cwnd = 0, self.cwnd
            else:
                self.time_to_origin = icbrt((CUBE_FACTOR * (self.last_max_cwnd - self.cwnd)) & M64)
                self.origin_cwnd = self.last_max_cwnd
        elif self.app_limited_us != 0:
            self.epoch_us = (self.epoch_us + now - self.app_limited_us) & M64
            self.app_limited_us = 0
        elapsed = go_div(s64((now + self.min_rtt_us - self.epoch_us) << 10), 1000000)
        offset = self.time_to_origin - elapsed
        delta = (s64(CUBE_CWND_SCALE * offset * offset * offset) >> CUBE_SCALE) & M64
        target = (self.origin_cwnd - delta) & M64
        alpha = alpha_n(self.p["num_connections"])
        while True:
            required = int(f32(self.est_tcp_cwnd) / alpha)
            if self.acked_count < required:
                break
            self.acked_count -= required
            self.est_tcp_cwnd += 1
        self.last_target_cwnd = target
        return max(target, self.est_tcp_cwnd), False

    def _limited(self, bif):
        mss = self.p["mss"]
        w = self.cwnd * mss
        if bif >= w:
            return True
        return (self.in_slow_start() and bif > w // 2) or w - bif <= 3 * mss

    def _grow(self, g, bif, now):
        mss, cap = self.p["mss"], self.p["max_cwnd"]
        while g:
            self.steps += 1
            if not self._limited(bif):
                if self.app_limited_us == 0:
                    self.app_limited_us = now
                if self.per_packet:
                    g -= 1
                    continue
                return
            if self.cwnd >= cap:
                if self.per_packet:
                    g -= 1
                    continue
                return
            if self.in_slow_start():
                if self.per_packet:
                    self.cwnd += 1
                    g -= 1
                    continue
                # the first window that is not limited in slow start: c mss >= 2 bif and c mss > bif + 3 mss
                stop = max(-(-2 * bif // mss), bif // mss + 4)
                k = min(g, min(stop, self.ssthresh, cap) - self.cwnd)
                assert k >= 1
                self.cwnd += k
                g -= k
                continue
            before = self.cwnd
            t, early = self._after_ack(now)
            self.cwnd = min(cap, t)
            g -= 1
            if early and self.cwnd == before and not self.per_packet:
                self.acked_count = (self.acked_count + g) & 0xffffffff
                return

    # -------------------------------------------------------------- RTT, hybrid slow start
    def _update_rtt(self, send_delta, ack_delay):
        if self.min_rtt_us == 0 or self.min_rtt_us > send_delta:
            self.min_rtt_us = send_delta
        sample = send_delta
        if sample > ack_delay:
            sample -= ack_delay
        self.latest_rtt_us = sample
        if self.srtt_us == 0:
            self.srtt_us, self.mean_dev_us = sample, sample // 2
        else:
            dev = abs(self.srtt_us - sample)
            self.mean_dev_us = int(ONE_MINUS_BETA * f32(self.mean_dev_us) + RTT_BETA * f32(dev))
            self.srtt_us = int(f32(self.srtt_us) * ONE_MINUS_ALPHA + f32(sample) * RTT_ALPHA)

    def _should_exit(self, last_sent):
        if not self.started:
            self.end_packet_number, self.current_min_rtt_us, self.sample_count, self.started = last_sent, 0, 0, 1
        if self.found:
            return True
        self.sample_count += 1
        if self.sample_count <= HS_MIN_SAMPLES and \
                (self.current_min_rtt_us == 0 or self.current_min_rtt_us > self.latest_rtt_us):
            self.current_min_rtt_us = self.latest_rtt_us
        if self.sample_count == HS_MIN_SAMPLES:
            thr = max(min(self.min_rtt_us >> 3, HS_MAX_THR_US), HS_MIN_THR_US)
            if self.current_min_rtt_us > self.min_rtt_us + thr:
                self.found = 1
        return self.cwnd >= HS_LOW_WINDOW and bool(self.found)

    # -------------------------------------------------------------- the two calls
    def ack(self, ev, row, now_us, last_sent, lio, err=0):
        """ugo_fec_cc_set_ack for this member.  ev, row: dicts (or numpy
        records) of the event row and the cc row; last_sent, lio, err: the
        sent record's.  Returns delay_us[c]."""
        if err:
            return 0
        if ev["accepted"]:
            if ev["has_rtt"] and int(ev["rtt_us"]) > 0:
                self._update_rtt(int(ev["rtt_us"]), int(ev["delay_us"]))
            if ev["has_rtt"] and self.in_slow_start() and self._should_exit(last_sent):
                self.ssthresh = self.cwnd
            cut = False
            if int(ev["lost_packets"]) > 0 and int(row["max_lost"]) > self.cutback:
                self._loss_reaction(last_sent)
                cut = True
            acked, prior = int(ev["acked_packets"]), self.largest_acked
            self.largest_acked = max(prior, int(row["max_acked"]))
            in_recovery = acked if cut else (0 if prior > self.cutback else int(row["acked_le"]))
            g = acked - min(in_recovery, acked)
            self._grow(g, int(ev["bytes_in_flight"]), now_us)
            if g and self.in_slow_start() and int(row["max_acked"]) > self.end_packet_number:
                self.started = 0
        self.rto_candidate = 0 if lio == last_sent else lio + 1
        return 0 if self.srtt_us == 0 else self.srtt_us + 4 * self.mean_dev_us

    def rto(self, fired, last_sent, bif, packet_bytes, max_budget, err=0):
        """ugo_fec_cc_set_rto for this member; last_sent, bif, err: the sent
        record's as they stand after ugo_fec_sent_set_rto.  Returns budget[c]."""
        if err:
            return 0
        if fired:
            if self.rto_candidate != 0 and self.rto_candidate > self.cutback:
                self._loss_reaction(last_sent)
            self.cutback = 0
            self.started = self.found = 0
            self.epoch_us = self.app_limited_us = self.last_update_us = 0
            self.last_cwnd = self.last_max_cwnd = self.est_tcp_cwnd = self.origin_cwnd = self.last_target_cwnd = 0
            self.acked_count = self.time_to_origin = 0
            self.ssthresh = self.cwnd // 2
            self.cwnd = self.p["min_cwnd"]
            self.rtos += 1
        w = self.cwnd * self.p["mss"]
        return 0 if bif > w else min(max_budget, (w - bif) // packet_bytes + 1)


def cc_row(before, rule, ev, split):
    """The ugo_cc_row of one member: before = {n: state} of its RuleSent's
    slots ahead of the ack, rule the RuleSent after it, ev its event row."""
    row = dict.fromkeys(RuleCc.ROW_FIELDS, 0)
    if not ev["accepted"]:
        return row
    freed = [n for n in before if n not in rule.slots]
    lost = [n for n, st in before.items() if st == sr.IN_FLIGHT and n in rule.slots and
            rule.slots[n]["state"] == sr.QUEUED]
    row["max_lost"], row["max_acked"] = max(lost, default=0), max(freed, default=0)
    row["acked_le"] = sum(1 for n in freed if n <= split)
    return row


class RulePair:
    """A RuleSent and its RuleCc, called in THE ORDER of include/ugo_cc.h."""

    def __init__(self, ws=1024, seg_cap=1, per_packet=False, **params):
        self.sent = sr.RuleSent(ws, seg_cap)
        self.cc = RuleCc(per_packet=per_packet, **params)
        self.delay_us = 0

    def send(self, numbers, length, now_us):
        self.sent.record([(n, length, 0, 0, [(10 * n, 10)]) for n in numbers], now_us)

    def ack(self, acks, now_us):
        """ugo_fec_cc_sent_ack, ugo_fec_cc_set_ack.  Returns (event, row, delay_us)."""
        s = self.sent
        before = {n: x["state"] for n, x in s.slots.items()}
        ev = s.ack(acks, now_us)
        row = cc_row(before, s, ev, self.cc.cutback)
        self.delay_us = self.cc.ack(ev, row, now_us, s.last_sent, s.lio, s.err)
        return ev, row, self.delay_us

    def rto(self, now_us, packet_bytes, max_budget):
        """ugo_fec_sent_set_rto with the delay just written, ugo_fec_cc_set_rto.
        Returns (fired, budget)."""
        s = self.sent
        fired = s.rto(self.delay_us, now_us)
        return fired, self.cc.rto(fired, s.last_sent, s.bytes_in_flight, packet_bytes, max_budget, s.err)
