"""GoSender with deviation (b) of include/ugo_sent.h and nothing else; test
infrastructure only.

Deviation (b): an ACK frees a queued (retransmitted, not yet drained) packet
under largestInOrderAcked, which the reference's receivedAck never visits: its
first loop starts at largestInOrderAcked itself.  GoSenderB drops exactly those
numbers before it hands an accepted ACK to the reference's own loops.
"""
import sent_ref as sr


class GoSenderB(sr.GoSender):
    def receivedAck(self, ack, withPacketNumber):
        accepted = not (ack.la > self.lastSentPacketNumber
                        or (withPacketNumber != 0 and withPacketNumber <= self.largestReceivedPacketWithAck)
                        or ack.la <= self.largestInOrderAcked
                        or ack.la <= self.largestAcked)
        if accepted:
            for n in sorted(self.packetHistory):
                if n < self.largestInOrderAcked and n < ack.lio:
                    self.packetHistory.pop(n)
        return super().receivedAck(ack, withPacketNumber)
