"""The connection loop twice over; test infrastructure only.

GoLoop    a restatement of what ugo's Conn does with finSent, finRcvd, closed,
          originAckTime, lastNetworkActivityTime, linger, CheckForError and
          resetTimer (ugo/conn.go), walked packet by packet and send loop by
          send loop under an injected clock.  Written from the behaviour.
RuleLoop  THE RULE of include/ugo_loop.h for one member, in plain Python.
The *_set functions apply a call to one RuleLoop per member as the entry points
of a set do, and return what the device must have written.

GoConn    GoLoop with the reference's own neighbours beside it: packetSender
          (sent_ref.GoSender), packetReceiver (ack_ref.GoReceiver) and the
          segment sender (stream_tx_ref.GoSender); handlePacket and sendPacket
          as conn.go calls them.
RuleConn  RuleLoop with the rules of the neighbouring stages beside it
          (sent_ref.RuleSent, ack_ref.RuleAck, stream_tx_ref.RuleTx), one batch
          in THE ORDER per call: what the loop reads of them is what they hold.

A member's neighbouring records come in as a dict nb with the keys NB_KEYS:
the receive window's, the receive history's and the sent history's err, the
sent history's rto_count, tracked and last_sent_us, the send window's tail,
write_pos, rq_len and cap.
"""
import ack_ref as ar
import sent_ref as sr
import stream_tx_ref as st

M64 = (1 << 64) - 1
NO_CONN = 0xffffffff
NEVER = M64
PKT_OK, PKT_CAPACITY = 0, 6
ACK_FLAG, STOP_FLAG, FIN_FLAG, RST_FLAG = 0x80, 0x40, 0x10, 0x08
ACK_FIN = ACK_FLAG | FIN_FLAG
DEFAULTS = dict(ack_delay_us=5000, idle_us=300_000_000, max_retries=10)
PEER_ACK_FIN, PEER_RST, BAD_PACKET, CLOSED, FAILURES, SENT_ERR, ACK_ERR, STREAM_ERR, IDLE, LINGER, ABORT = range(1, 12)
OWES_RST = (BAD_PACKET, FAILURES, SENT_ERR, ACK_ERR, STREAM_ERR, IDLE, LINGER, ABORT)
NONE, FIN, RST = 0, 1, 2
HOW_CLOSE, HOW_ABORT, HOW_NODELAY_ON, HOW_NODELAY_OFF = 1, 2, 4, 8
NB_KEYS = ("stream_err", "ack_err", "sent_err", "rto_count", "tracked", "last_sent_us", "tail", "write_pos",
           "rq_len", "cap")
NB_IDLE = dict(stream_err=0, ack_err=0, sent_err=0, rto_count=0, tracked=0, last_sent_us=0, tail=0, write_pos=0,
               rq_len=0, cap=4096)


def rto_us(delay_us, rto_count):
    """getRTO as ugo_fec_sent_set_rto computes it (tests/sent_ref.py states it for a RuleSent)."""
    r = sr.RuleSent.__new__(sr.RuleSent)
    r.rto_count = rto_count
    return sr.RuleSent.rto_us(r, delay_us)


def end_kind(status, flags):
    """0 no, 1 ACK|FIN, 2 RST, 3 decode error."""
    if 1 <= status <= 5:
        return 3
    if status not in (PKT_OK, PKT_CAPACITY):
        return 0
    return 1 if flags == ACK_FIN else 2 if flags == RST_FLAG else 0


def sat(a, b):
    return min(a + b, M64)


# ------------------------------------------------------------------ THE RULE
class RuleLoop:
    FIELDS = ("last_activity_us", "origin_ack_us", "linger_deadline_us", "exit_us", "dropped", "closed", "fin_sent",
              "fin_rcvd", "ack_no_delay", "exited", "reason", "pending", "reported")

    def __init__(self, now_us=0, **params):
        self.p = dict(DEFAULTS, **params)
        self.last_activity_us = now_us
        self.origin_ack_us = self.linger_deadline_us = self.exit_us = self.dropped = 0
        self.closed = self.fin_sent = self.fin_rcvd = self.ack_no_delay = 0
        self.exited = self.reason = self.pending = self.reported = 0

    def view(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def _exit(self, reason, now_us):
        self.exited, self.reason, self.exit_us = 1, reason, now_us
        if reason in OWES_RST:
            self.pending = RST

    def receive(self, packets, now_us):
        """packets: the member's [(status, flags, packet_number)] in batch
        order.  Returns how many of them are handled; the rest are dropped."""
        if self.exited:
            self.dropped += len(packets)
            return 0
        if not packets:
            return 0
        self.last_activity_us = now_us
        handled = len(packets)
        for k, (status, flags, pn) in enumerate(packets):
            kind = end_kind(status, flags)
            if kind:
                handled = k
                if kind == 1:
                    self.fin_rcvd = 1
                self._exit((PEER_ACK_FIN, PEER_RST, BAD_PACKET)[kind - 1], now_us)
                break
            if pn != 0 and self.origin_ack_us == 0:
                self.origin_ack_us = now_us
            if flags & FIN_FLAG:
                self.fin_rcvd = 1
        self.dropped += len(packets) - handled
        return handled

    def close(self, how, linger_us, now_us):
        if self.exited or not how & 15:
            return
        if how & HOW_NODELAY_ON:
            self.ack_no_delay = 1
        if how & HOW_NODELAY_OFF:
            self.ack_no_delay = 0
        if self.closed:
            return
        if how & HOW_ABORT:
            self._exit(ABORT, now_us)
        elif how & HOW_CLOSE:
            self.closed = 1
            if linger_us > 0:
                self.linger_deadline_us = sat(now_us, linger_us)

    def check(self, now_us, nb):
        """Returns (the budget goes to 0, may_ack_only)."""
        if not self.exited:
            reason = 0
            if nb["stream_err"]:
                reason = STREAM_ERR
            elif nb["ack_err"]:
                reason = ACK_ERR
            elif nb["sent_err"]:
                reason = SENT_ERR
            elif nb["rto_count"] > self.p["max_retries"]:
                reason = FAILURES
            elif self.closed and self.linger_deadline_us != 0 and now_us >= self.linger_deadline_us:
                reason = LINGER
            elif now_us >= self.last_activity_us and now_us - self.last_activity_us >= self.p["idle_us"]:
                reason = IDLE
            if reason:
                self._exit(reason, now_us)
            elif self.closed:
                if (not self.fin_sent and self.pending == NONE and nb["tail"] == nb["write_pos"] and
                        nb["rq_len"] == 0 and nb["tracked"] == 0):
                    self.pending = FIN
                if self.fin_rcvd and (self.fin_sent or self.pending == FIN):
                    self._exit(CLOSED, now_us)
        zero = bool(self.exited or self.fin_sent or self.pending)
        may = 0
        if not self.exited:
            may = int(bool(self.ack_no_delay or self.origin_ack_us == 0 or
                           (now_us > self.origin_ack_us and now_us - self.origin_ack_us > self.p["ack_delay_us"])))
        return zero, may

    def appended(self):
        """The member's pending packet found its place.  Returns 1 (FIN) or 2 (RST)."""
        what = self.pending
        if what == FIN:
            self.fin_sent, self.linger_deadline_us = 1, 0
        self.pending = NONE
        return what

    def sent(self, sent_any, delay_us, now_us, nb):
        """The origin reset; returns the member's deadline (NEVER if exited)."""
        if self.exited:
            return NEVER
        if sent_any:
            self.origin_ack_us = 0
        dl = sat(self.last_activity_us, self.p["idle_us"])
        if self.origin_ack_us:
            dl = min(dl, sat(self.origin_ack_us, self.p["ack_delay_us"]))
        if self.linger_deadline_us:
            dl = min(dl, self.linger_deadline_us)
        if nb["last_sent_us"]:
            t = sat(nb["last_sent_us"], rto_us(delay_us, nb["rto_count"]))
            if t > now_us:
                dl = min(dl, t)
        return dl


# ------------------------------------------------------------------ sets
def receive_set(rules, status, flags, pn, conn_of, now_us):
    """The arrays of a batch; returns conn_of as the call leaves it (a list)."""
    per = [[] for _ in rules]
    for i, c in enumerate(conn_of):
        if c < len(rules):
            per[c].append(i)
    out = list(conn_of)
    for c, idx in enumerate(per):
        handled = rules[c].receive([(int(status[i]), int(flags[i]), int(pn[i])) for i in idx], now_us)
        for i in idx[handled:]:
            out[i] = NO_CONN
    return out


def close_set(rules, how, linger_us, now_us):
    for c, r in enumerate(rules):
        r.close(int(how[c]), 0 if linger_us is None else int(linger_us[c]), now_us)


def check_set(rules, nbs, now_us, budget):
    """Returns (budget after the call, may_ack_only)."""
    out, may = list(budget), []
    for c, r in enumerate(rules):
        zero, m = r.check(now_us, nbs[c])
        if zero:
            out[c] = 0
        may.append(m)
    return out, may


def append_set(rules, nbs, total, max_packets):
    """Returns ([(t, c, what, offset, data_off)], appended, total_out)."""
    writes, appended = [], [0] * len(rules)
    t = total
    for c, r in enumerate(rules):
        if r.pending and t < max_packets:
            off = nbs[c]["write_pos"]
            appended[c] = r.appended()
            writes.append((t, c, appended[c], off, off & (nbs[c]["cap"] - 1)))
            t += 1
    return writes, appended, t


def sent_set(rules, nbs, n_packets, attached, delay_us, now_us, max_exits):
    """Returns (deadline, exits, reasons, n_exits, new_index, nconn_new)."""
    deadline = NEVER
    for c, r in enumerate(rules):
        d = 0 if delay_us is None else int(delay_us[c])
        deadline = min(deadline, r.sent(bool(n_packets[c] > 0 or attached[c] != 0), d, now_us, nbs[c]))
    todo = [c for c, r in enumerate(rules) if r.exited and not r.reported]
    for c in todo[:max_exits]:
        rules[c].reported = 1
    new_index, k = [], 0
    for r in rules:
        new_index.append(NO_CONN if r.exited else k)
        k += 0 if r.exited else 1
    return (deadline, todo[:max_exits], [rules[c].reason for c in todo[:max_exits]], len(todo), new_index, k)


# ------------------------------------------------------------------ the reference, restated
class GoLoop:
    """What Conn does with its loop state, one event at a time (ugo/conn.go:
    run, handlePacket, sendPacket, Close, resetConn, resetTimer).  The clock is
    injected, and so is what the loop asks of its neighbours: env holds, for the
    event at hand, what lenOfDataForWriting, len(packetHistory), the segment
    retransmission queue, CheckForError, consecutiveRTOCount and
    timeOfFirstRTO answer, how many data packets the send loop finds to send,
    and which of the arriving packets make packetReceiver or handleSegment
    return an error."""

    def __init__(self, now, ack_delay_us=5000, idle_us=300_000_000, max_retries=10):
        self.ackSendDelay, self.idleLifetime, self.maxRetries = ack_delay_us, idle_us, max_retries
        self.finSent = self.finRcvd = self.ackNoDelay = False
        self.closed = self.eof = 0
        self.appClosed = False                      # closed by Close, not by resetConn
        self.originAckTime = 0                      # the zero time
        self.lastNetworkActivityTime = now
        self.linger = -1                            # SetLinger: < 0 waits, 0 aborts, > 0 arms the timer (us here)
        self.lingerTimer = 0                        # when it fires; 0 = none
        self.ackPending = False                     # packetReceiver.stateChanged
        self.loopExited, self.reason, self.exitTime = False, 0, 0
        self.wire = []                              # "FIN" / "RST" in the order they left
        self.handled = 0                            # packets of the last event that handlePacket took
        self.onlyAck = None                         # the last send loop's answer at conn.go:587
        self.sentAny = False

    # resetConn and exitLoop
    def _exit(self, reason, now, remote_closed=False, by_reset=True):
        if by_reset and not remote_closed:
            self.wire.append("RST")
        if by_reset:
            self.eof = self.closed = 1
        if not self.loopExited:
            self.loopExited, self.reason, self.exitTime = True, reason, now

    def fire_linger_timer(self, now):
        """time.AfterFunc of Close: it fires on its own, between two events."""
        if self.lingerTimer and now >= self.lingerTimer and not self.loopExited:
            at, self.lingerTimer = self.lingerTimer, 0
            self._exit(LINGER, at)

    def SetLinger(self, us):
        self.linger = us

    def SetACKNoDelay(self, on):
        self.ackNoDelay = bool(on)

    def Close(self, now):
        if self.closed == 1:
            return "close closed connection"
        if self.linger == 0:
            self._exit(ABORT, now)
            return None
        self.closed = 1
        self.appClosed = True
        if self.linger > 0:
            self.lingerTimer = now + self.linger
        return None

    def handlePacket(self, p, now, env):
        """p = (status, flags, packet_number, receiver_err, segment_err).  Returns an error or None."""
        status, flags, pn, receiver_err, segment_err = p
        self.lastNetworkActivityTime = now
        if 1 <= status <= 5:
            return BAD_PACKET
        if pn != 0 and self.originAckTime == 0:
            self.originAckTime = now
        if flags & FIN_FLAG == FIN_FLAG:
            self.finRcvd = True
        if flags == ACK_FIN:
            self._exit(PEER_ACK_FIN, now, by_reset=False)
            return None
        if flags == RST_FLAG:
            self._exit(PEER_RST, now, remote_closed=True)
            return None
        self.handled += 1                           # past the top: the rest is the receive stages'
        if pn != 0:
            if receiver_err:
                return ACK_ERR
            self.ackPending = True
        if segment_err:
            return STREAM_ERR
        return None

    def sendPacket(self, now, env):
        self.onlyAck, self.sentAny = None, False
        data = env["n_data"]
        while True:
            if self.closed == 1:
                if env["unsent"] == 0 and env["tracked"] == 0 and not self.finSent:
                    self.wire.append("FIN")
                    self.finSent = True
                    self.lingerTimer = 0
                if self.finSent and self.finRcvd:
                    self._exit(CLOSED, now, by_reset=False)
                    return None
            if env["sent_err"]:
                return SENT_ERR
            if env["rto_count"] > self.maxRetries:
                return FAILURES
            if env["rto_fires"]:                    # checkRTO, behind CheckForError
                env["rto_count"] += 1
                env["rto_fires"] = False
            ack = self.ackPending
            if not ack and data == 0:
                return None
            only = self.originAckTime == 0 or now - self.originAckTime > self.ackSendDelay or self.ackNoDelay
            if self.onlyAck is None:
                self.onlyAck = only                 # as the send loop found it
            if data == 0 and not only:
                return None
            self.ackPending = False
            if data:
                data -= 1
            self.originAckTime = 0
            self.sentAny = True

    def event(self, now, env, packets=()):
        """One turn of run's loop per arriving packet, or one turn for a write
        event or a timer.  Returns the packets handled."""
        self.handled = 0
        self.fire_linger_timer(now)
        turns = list(packets) or [None]
        for p in turns:
            if self.loopExited:
                break
            err = None
            if p is not None:
                err = self.handlePacket(p, now, env)
            if err is None:                         # also behind the packet that closed closeChan
                err = self.sendPacket(now, env)
            if err is not None:
                self._exit(err, now)
                break
            if not self.loopExited and now - self.lastNetworkActivityTime >= self.idleLifetime:
                self._exit(IDLE, now)
        return self.handled

    def resetTimer(self, now, env):
        if self.loopExited:
            return NEVER
        deadline = self.lastNetworkActivityTime + self.idleLifetime
        if self.originAckTime != 0:
            deadline = min(deadline, self.originAckTime + self.ackSendDelay)
        if env["last_sent_us"] != 0:
            rto = env["last_sent_us"] + rto_us(env["delay_us"], env["rto_count"])
            if rto > now:
                deadline = min(deadline, rto)
        return deadline

    def view(self):
        return dict(closed=int(self.appClosed), fin_sent=int(self.finSent), fin_rcvd=int(self.finRcvd),
                    ack_no_delay=int(self.ackNoDelay), exited=int(self.loopExited), reason=self.reason,
                    origin_ack_us=self.originAckTime, last_activity_us=self.lastNetworkActivityTime,
                    exit_us=self.exitTime, linger_deadline_us=self.lingerTimer)


# ------------------------------------------------------------------ both, with their real neighbours
PAYLOAD = 1436                                  # maxPacketSize - 40
SEGMENT = PAYLOAD - st.H                        # what one packet carries of fresh data
BUDGET = 64


class GoConn(GoLoop):
    """A packet is (status, flags, packet_number, sack, stop_waiting, segment_err): sack a sent_ref.Ack or
    None; segment_err makes handleSegment fail (the receive window is not restated here)."""

    def __init__(self, now, **params):
        super().__init__(now, **params)
        self.ps, self.ss, self.pr = sr.GoSender(), st.GoSender(), ar.GoReceiver()
        self.tooManyTracked = False             # errTooManyTrackedSentPackets, injected
        self.packets = []                       # what the last event sent: (packet_number, [(offset, len)], ack, sw)

    def Write(self, data):
        if self.closed != 1 and self.ss.lenOfDataForWriting() == 0:
            self.ss.Write(data)

    def handlePacket(self, p, now, env=None):
        status, flags, pn, sack, sw, segment_err = p
        self.lastNetworkActivityTime = now
        if 1 <= status <= 5:
            return BAD_PACKET
        if pn != 0 and self.originAckTime == 0:
            self.originAckTime = now
        if flags & FIN_FLAG == FIN_FLAG:
            self.finRcvd = True
        if flags == ACK_FIN:
            self._exit(PEER_ACK_FIN, now, by_reset=False)
            return None
        if flags == RST_FLAG:
            self._exit(PEER_RST, now, remote_closed=True)
            return None
        self.handled += 1
        if pn != 0 and self.pr.receivedPacket(pn) is not None:
            return ACK_ERR
        if sack is not None:
            err, _, _ = self.ps.receivedAck(sack, pn)
            assert err is None, err                 # the scripted peer sends no ACK the reference resets on
        if segment_err:
            return STREAM_ERR
        if sw != 0:
            self.pr.receivedStopWaiting(sw)
        return None

    def sendPacket(self, now, env=None):
        self.onlyAck, self.sentAny = None, False
        while True:
            if self.closed == 1:
                if self.ss.lenOfDataForWriting() == 0 and len(self.ps.packetHistory) == 0 and not self.finSent:
                    self.wire.append("FIN")
                    self.finSent = True
                    self.lingerTimer = 0
                if self.finSent and self.finRcvd:
                    self._exit(CLOSED, now, by_reset=False)
                    return None
            if self.tooManyTracked:
                return SENT_ERR
            if self.ps.consecutiveRTOCount > self.maxRetries:
                return FAILURES
            self.ps.checkRTO(0, now)
            rp = self.ps.dequeuePacketForRetransmission()
            if rp is not None:
                if rp.flags & ACK_FLAG:
                    self.pr.stateChanged = True
                if rp.flags & STOP_FLAG:
                    self.ps.swState = True
                for seg in rp.segments:
                    self.ss.AddSegmentForRetransmission(seg)
            ack, err = self.pr.buildSack(False)
            assert err is None, err
            stopWait = self.ps.GetStopWaitingFrame()
            segments = self.ss.PopSegments(PAYLOAD)
            if ack is None and len(segments) == 0 and stopWait == 0:
                return None
            only = self.originAckTime == 0 or now - self.originAckTime > self.ackSendDelay or self.ackNoDelay
            if self.onlyAck is None:
                self.onlyAck = only
            if len(segments) == 0 and stopWait == 0 and not only:
                return None
            if ack is not None:
                self.pr.buildSack(True)
            if len(segments) != 0 or stopWait != 0:
                self.ss.lastPacketNumber += 1
            flags = (ACK_FLAG if ack is not None else 0) | (STOP_FLAG if stopWait else 0) | (0x20 if segments else 0)
            pn = 0 if flags == ACK_FLAG else self.ss.lastPacketNumber
            if pn != 0:
                length = 10 + sum(x.dataLen() for x in segments)
                assert self.ps.sentPacket(sr._GoPacket(pn, length, flags, segments), now) is None
            self.originAckTime = 0
            self.sentAny = True
            self.packets.append((pn, [(x.offset, x.dataLen()) for x in segments], ack is not None, stopWait))

    def event(self, now, env=None, packets=()):
        self.packets = []
        return super().event(now, env, packets)

    def resetTimer(self, now, env=None):
        return super().resetTimer(now, dict(last_sent_us=self.ps.lastSentPacketTime, delay_us=0,
                                            rto_count=self.ps.consecutiveRTOCount))


class RuleConn:
    def __init__(self, now, **params):
        self.loop = RuleLoop(now, **params)
        self.sent, self.ack, self.tx = sr.RuleSent(1024, 8), ar.RuleAck(2048), st.RuleTx(65536, 64)
        self.sent_err = self.stream_err = 0     # injected: the sent history's window and the receive window
        self.packets, self.emitted, self.may, self.deadline = [], [], 0, NEVER

    def write(self, data):
        if not self.loop.closed and not self.loop.exited and self.tx.tail == self.tx.write_pos:
            self.tx.write(data)

    def nb(self):
        return dict(stream_err=self.stream_err, ack_err=self.ack.err, sent_err=self.sent.err or self.sent_err,
                    rto_count=self.sent.rto_count, tracked=self.sent.tracked, last_sent_us=self.sent.last_sent_us,
                    tail=self.tx.tail, write_pos=self.tx.write_pos, rq_len=len(self.tx.queue), cap=self.tx.cap)

    def batch(self, packets, now):
        """One batch in THE ORDER.  Returns the packets handled."""
        handled = self.loop.receive([p[:3] for p in packets], now)
        taken = packets[:handled]                                   # the later stages skip what receive masked
        self.ack.receive([(p[2], p[4]) for p in taken], now)
        self.sent.ack([sr.Ack(p[3].la, p[3].lio, p[3].ranges, p[2], p[3].delay) for p in taken if p[3] is not None],
                      now)
        if any(p[5] for p in taken):
            self.stream_err = 1
        self.sent.rto(0, now)
        _, entries, touch = self.sent.drain()
        self.tx.retransmit(entries)
        if touch:
            self.ack.touch()
        self.tx.release(self.sent.upto())
        zero, self.may = self.loop.check(now, self.nb())
        planned = self.tx.plan(0 if zero else BUDGET, PAYLOAD, 8)
        self.emitted = []
        if self.loop.pending:
            self.emitted.append({FIN: "FIN", RST: "RST"}[self.loop.appended()])
        have_ack = bool(self.ack.changed and not self.ack.err and (planned or self.may))
        if have_ack:
            self.ack.changed = 0
        _, sw = self.sent.attach(bool(planned))
        self.packets, records = [], []
        for k, (pn, segs) in enumerate(planned):
            flags = 0x20 | (ACK_FLAG if have_ack and k == 0 else 0) | (STOP_FLAG if sw and k == 0 else 0)
            records.append((pn, 10 + sum(n for _, n in segs), flags, sw if k == 0 else 0, segs))
            self.packets.append((pn, list(segs), have_ack and k == 0, sw if k == 0 else 0))
        if have_ack and not planned:
            self.packets.append((0, [], True, 0))
        self.sent.record(records, now)
        self.deadline = self.loop.sent(bool(planned) or have_ack, 0, now, self.nb())
        return handled
