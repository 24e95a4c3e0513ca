"""include/ugo_sent.h: sent histories, the packetSender's state per
connection, and the set that records, acknowledges and times out many per
call."""
from __future__ import annotations

import ctypes
import weakref
from typing import Optional

import numpy as np

from .abi import (_check_info, _check_ranges, _check_segs, _check_tensor, _Handle, _MemberSet, _raise, _require,
                  _stream_handle, load_library, torch)
from .encoder import Encoder

SENT_MIN_WINDOW = 1024
SENT_MAX_WINDOW = 1 << 20
SENT_MAX_SEG_CAP = 16
SENT_TOO_MANY_TRACKED = 1  # ugo_sent_state.err
SENT_IN_FLIGHT, SENT_QUEUED = 0, 1  # ugo_sent_slot.state
SENT_RTO_DEFAULT_US, SENT_RTO_MIN_US, SENT_RTO_MAX_US = 500_000, 200_000, 60_000_000
SENT_SLOT_DTYPE = np.dtype([("packet_number", "<u8"), ("sent_us", "<u8"), ("min_offset", "<u8"), ("len", "<u4"),
                            ("state", "u1"), ("missing", "u1"), ("n_segments", "u1"), ("bits", "u1")])
SENT_SEG_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("reserved", "<u4")])  # ugo_stream_tx_rq_entry
SENT_STATE_DTYPE = np.dtype([("last_sent", "<u8"), ("lio", "<u8"), ("largest_acked", "<u8"),
                             ("largest_with_ack", "<u8"), ("least_unacked", "<u8"), ("bytes_in_flight", "<u8"),
                             ("last_sent_us", "<u8"), ("scan_from", "<u8"), ("acked_packets", "<u8"),
                             ("acked_bytes", "<u8"), ("lost_packets", "<u8"), ("lost_bytes", "<u8"),
                             ("duplicates", "<u8"), ("unsent_acks", "<u8"), ("stale", "<u8"), ("tracked", "<u4"),
                             ("queued", "<u4"), ("queued_segments", "<u4"), ("rto_count", "<u4"),
                             ("sw_pending", "u1"), ("err", "u1"), ("reserved", "u1", (22,))])
SENT_EVENT_DTYPE = np.dtype([("rtt_us", "<u8"), ("delay_us", "<u8"), ("acked_bytes", "<u8"), ("lost_bytes", "<u8"),
                             ("bytes_in_flight", "<u8"), ("largest_acked", "<u8"), ("acked_packets", "<u4"),
                             ("lost_packets", "<u4"), ("accepted", "u1"), ("has_rtt", "u1"),
                             ("reserved", "u1", (6,))])
assert SENT_SLOT_DTYPE.itemsize == 32 and SENT_SEG_DTYPE.itemsize == 16
assert SENT_STATE_DTYPE.itemsize == 160 and SENT_EVENT_DTYPE.itemsize == 64


class SentTx(_Handle):
    """A connection's sent history on the GPU (include/ugo_sent.h): the
    packetSender's state, a slot ring of window_packets numbers, their segment
    rows and a record.  Every call goes through a SentTxSet; a set of one is
    the single-connection form."""

    _destroy = "ugo_fec_sent_tx_destroy"

    def __init__(self, enc: Encoder, window_packets: int = 4096, seg_cap: int = 8):
        self.check_create(window_packets, seg_cap)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_sent_tx_create(enc._h, window_packets, seg_cap, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the history
        self.window_packets, self.seg_cap = window_packets, seg_cap
        self.device = enc.device
        self._sets = self._dependants = weakref.WeakSet()  # the open sets it is a member of: closed before it

    @staticmethod
    def check_create(window_packets: int, seg_cap: int):
        _require(SENT_MIN_WINDOW <= window_packets <= SENT_MAX_WINDOW and
                 window_packets & (window_packets - 1) == 0,
                 f"window_packets must be a power of two in [{SENT_MIN_WINDOW}, 2^20]")
        _require(1 <= seg_cap <= SENT_MAX_SEG_CAP, f"seg_cap must be 1 to {SENT_MAX_SEG_CAP}")

    def slots(self):
        """The slot ring as a uint8 CUDA tensor [window_packets, 32] over the
        device memory itself (SENT_SLOT_DTYPE rows); valid while this object lives."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_sent_tx_slots(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value * 32).view(n.value, 32)

    def segments(self):
        """The segment ring as a uint8 CUDA tensor [window_packets, seg_cap, 16]
        (SENT_SEG_DTYPE entries) over the device memory itself."""
        p, n, s = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_sent_tx_segments(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(s)))
        return self._view(p.value, n.value * s.value * 16).view(n.value, s.value, 16)

    def scratch(self):
        """The difference ring and the claim ring as an int32 CUDA tensor
        [2 * window_packets] over the device memory itself: zero between calls."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_sent_tx_scratch(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value * 4).view(torch.int32)


class SentTxSet(_MemberSet):
    """An ordered set of sent histories (ugo_fec_sent_set_*): record what
    StreamTxSet.encode sent, ack for a decoded batch, rto, drain into the form
    StreamTxSet.retransmit takes, attach a pending stop-waiting to the plan.
    Operands are tensors in device or pinned host memory.  Nothing is
    synchronised but states().  The set does not own its members; close it
    before them."""

    _member, _nouns, _attr = SentTx, ("history", "histories"), "txs"
    _create, _destroy = "ugo_fec_sent_set_create", "ugo_fec_sent_set_destroy"

    def __init__(self, enc: Encoder, txs):
        super().__init__(enc, txs)
        self.min_seg_cap = min(tx.seg_cap for tx in self.txs)
        for tx in self.txs:
            tx._sets.add(self)
        self._cc_sets = self._dependants = weakref.WeakSet()  # the open controller sets that read it: closed first

    def record(self, info, segs, conn_of, wire_lens, status, now_us: int, npackets: Optional[int] = None,
               stream=None):
        """ugo_fec_sent_set_record: info uint8 [>= npackets, 64], segs uint8
        [>= npackets, max_segments, 16] and conn_of int32 as StreamTxSet.plan left
        them, wire_lens int16 and status uint8 as StreamTxSet.encode returned them."""
        npk = info.shape[0] if npackets is None else npackets
        _check_info(info, npk, at_least=True)
        _require(0 <= npk <= 1 << 31 and 0 <= now_us < 1 << 64)
        _check_segs(segs, npk, at_least=True, max_segments=self.min_seg_cap,
                    msg="segs must be [npackets, max_segments, 16] with max_segments at most the smallest seg_cap")
        # kept: the lists may be longer than npackets, where StreamTxSet.retransmit wants exactly m elements
        _check_tensor(conn_of, npk, 4, "conn_of", at_least=True, integer=True)
        _check_tensor(wire_lens, npk, 2, "wire_lens", at_least=True, integer=True)
        _check_tensor(status, npk, 1, "status", at_least=True, integer=True)
        _raise(load_library().ugo_fec_sent_set_record(
            self._h, info.data_ptr(), segs.data_ptr(), segs.shape[1], conn_of.data_ptr(), wire_lens.data_ptr(),
            status.data_ptr(), npk, now_us, _stream_handle(stream)))

    def ack(self, info, ranges, conn_of, now_us: int, npackets: Optional[int] = None, events=None, stream=None):
        """ugo_fec_sent_set_ack: info uint8 [>= npackets, 64] and ranges int64
        [>= npackets, max_ranges, 2] as packet_decode returned them, conn_of int32.
        Returns events uint8 [nconn, 64] (SENT_EVENT_DTYPE rows); may be given."""
        npk = info.shape[0] if npackets is None else npackets
        _check_info(info, npk, at_least=True)
        _require(0 <= npk <= 1 << 31 and 0 <= now_us < 1 << 64)
        _check_ranges(ranges, npk, at_least=True, max_ranges=0xffff)
        _check_tensor(conn_of, npk, 4, "conn_of", at_least=True, integer=True)
        if events is None:
            events = torch.zeros((self.nconn, 64), dtype=torch.uint8, device=self._dev())
        _check_tensor(events, self.nconn, 1, row=(64,))
        _raise(load_library().ugo_fec_sent_set_ack(
            self._h, info.data_ptr(), ranges.data_ptr() if ranges.numel() else None, ranges.shape[1],
            conn_of.data_ptr(), npk, now_us, events.data_ptr(), _stream_handle(stream)))
        return events

    def rto(self, delay_us, now_us: int, fired=None, stream=None):
        """ugo_fec_sent_set_rto: delay_us int64 [nconn].  Returns fired uint8 [nconn]."""
        self.check_per_conn(delay_us, 8, "delay_us")
        _require(0 <= now_us < 1 << 64)
        if fired is None:
            fired = torch.zeros(self.nconn, dtype=torch.uint8, device=self._dev())
        self.check_per_conn(fired, 1, "fired")
        _raise(load_library().ugo_fec_sent_set_rto(self._h, delay_us.data_ptr(), now_us, fired.data_ptr(),
                                                   _stream_handle(stream)))
        return fired

    def drain(self, max_entries: int, out=None, stream=None):
        """ugo_fec_sent_set_drain.  Returns (conn_of int32 [max_entries], offset
        int64 [max_entries], len int32 [max_entries], n_entries int64 [1], touch
        uint8 [nconn], upto int64 [nconn]); out = such a tuple to write into."""
        _require(0 <= max_entries <= 1 << 31)
        dev = self._dev()
        if out is None:
            out = (torch.zeros(max_entries, dtype=torch.int32, device=dev),
                   torch.zeros(max_entries, dtype=torch.int64, device=dev),
                   torch.zeros(max_entries, dtype=torch.int32, device=dev),
                   torch.zeros(1, dtype=torch.int64, device=dev),
                   torch.zeros(self.nconn, dtype=torch.uint8, device=dev),
                   torch.zeros(self.nconn, dtype=torch.int64, device=dev))
        conn_of, offset, length, n_entries, touch, upto = out
        _check_tensor(conn_of, max_entries, 4, "conn_of", at_least=True, integer=True)
        _check_tensor(offset, max_entries, 8, "offset", at_least=True, integer=True)
        _check_tensor(length, max_entries, 4, "len", at_least=True, integer=True)
        _require(n_entries.numel() == 1 and n_entries.element_size() == 8)  # kept: size alone, as AckRxSet.attach
        self.check_per_conn(touch, 1, "touch")
        self.check_per_conn(upto, 8, "upto")
        _raise(load_library().ugo_fec_sent_set_drain(
            self._h, max_entries, conn_of.data_ptr() if max_entries else None,
            offset.data_ptr() if max_entries else None, length.data_ptr() if max_entries else None,
            n_entries.data_ptr(), touch.data_ptr(), upto.data_ptr(), _stream_handle(stream)))
        return out

    def attach(self, first_packet, n_packets, info, attached=None, stream=None):
        """ugo_fec_sent_set_attach: first_packet int64 [nconn] and n_packets int32
        [nconn] as StreamTxSet.plan returned them, info uint8 [max_packets, 64].
        Returns attached uint8 [nconn]."""
        _check_info(info, info.shape[0])
        _require(info.shape[0] <= 1 << 31)
        self.check_per_conn(first_packet, 8, "first_packet")
        self.check_per_conn(n_packets, 4, "n_packets")
        if attached is None:
            attached = torch.zeros(self.nconn, dtype=torch.uint8, device=self._dev())
        self.check_per_conn(attached, 1, "attached")
        _raise(load_library().ugo_fec_sent_set_attach(
            self._h, first_packet.data_ptr(), n_packets.data_ptr(), info.shape[0],
            info.data_ptr() if info.shape[0] else None, attached.data_ptr(), _stream_handle(stream)))
        return attached

    def states(self) -> np.ndarray:
        """The members' records (SENT_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, SENT_STATE_DTYPE)
        _raise(load_library().ugo_fec_sent_set_state(self._h, out.ctypes.data))
        return out
