"""include/ugo_ack.h: receive histories, the packetReceiver's state per
connection, and the set that tracks and attaches SACKs for many per call."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from .abi import (_check_info, _check_ranges, _check_tensor, _Handle, _MemberSet, _raise, _require, _stream_handle,
                  load_library, torch)
from .encoder import Encoder

ACK_MIN_WINDOW = 1024
ACK_MAX_WINDOW = 1 << 20
ACK_MAX_OUTSTANDING = 1000
ACK_TOO_MANY_OUTSTANDING = 1  # ugo_ack_state.err
ACK_NOT_ATTACHED, ACK_ATTACHED, ACK_TRUNCATED = 0, 1, 2  # attach's attached[c]
ACK_STATE_DTYPE = np.dtype([("largest_in_order", "<u8"), ("largest_observed", "<u8"), ("ignore_below", "<u8"),
                            ("lo_time_us", "<u8"), ("fresh", "<u8"), ("old", "<u8"), ("out_of_window", "<u8"),
                            ("outstanding", "<u4"), ("changed", "u1"), ("err", "u1"), ("reserved", "u1", (2,))])
assert ACK_STATE_DTYPE.itemsize == 64


class AckRx(_Handle):
    """A connection's receive history on the GPU (include/ugo_ack.h): the
    packetReceiver's state, a ring bitmap of window_packets numbers and a
    record.  Every call goes through an AckRxSet; a set of one is the
    single-connection form."""

    _destroy = "ugo_fec_ack_rx_destroy"

    def __init__(self, enc: Encoder, window_packets: int = 4096):
        self.check_window(window_packets)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_ack_rx_create(enc._h, window_packets, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the history
        self.window_packets = window_packets
        self.device = enc.device

    @staticmethod
    def check_window(window_packets: int):
        _require(ACK_MIN_WINDOW <= window_packets <= ACK_MAX_WINDOW and window_packets & (window_packets - 1) == 0,
                 f"window_packets must be a power of two in [{ACK_MIN_WINDOW}, 2^20]")

    def state(self) -> np.ndarray:
        """The record (ACK_STATE_DTYPE scalar); waits for the last call of the sets it is in."""
        out = np.zeros(1, ACK_STATE_DTYPE)
        _raise(load_library().ugo_fec_ack_rx_state(self._h, out.ctypes.data))
        return out[0]

    def bitmap(self):
        """The ring bitmap as an int64 CUDA tensor [window_packets / 64] over the
        device memory itself (packet number n is bit n & 63 of word
        (n & (window_packets - 1)) >> 6); valid while this object lives."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_ack_rx_bitmap(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value // 8).view(torch.int64)


class AckRxSet(_MemberSet):
    """An ordered set of receive histories (ugo_fec_ack_set_*): receive for a
    decoded batch that holds the packets of many connections, attach to write
    every member's SACK into the arrays StreamTxSet.plan left for
    StreamTxSet.encode.  Operands are tensors in device or pinned host memory.
    Nothing is synchronised but states().  The set does not own its members;
    close it before them."""

    _member, _nouns, _attr = AckRx, ("history", "histories"), "rxs"
    _create, _destroy = "ugo_fec_ack_set_create", "ugo_fec_ack_set_destroy"

    def receive(self, info, conn_of, now_us: int, seg_status=None, npackets: Optional[int] = None, stream=None):
        """ugo_fec_ack_set_receive: info uint8 [>= npackets, 64] as packet_decode
        returned it, conn_of int32 [>= npackets] the member of each packet,
        seg_status uint8 [>= npackets, max_segments] as StreamRxSet.deliver
        returned it, or None.  npackets defaults to info.shape[0]."""
        npk = info.shape[0] if npackets is None else npackets
        _require(0 <= npk <= info.shape[0] and 0 <= now_us < 1 << 64)
        _check_info(info, npk, at_least=True)
        _check_tensor(conn_of, npk, 4, "conn_of", "npackets", at_least=True, integer=True)
        max_segments = 0
        if seg_status is not None:
            _require(seg_status.is_contiguous() and seg_status.element_size() == 1 and seg_status.dim() == 2 and
                     seg_status.shape[0] >= npk and 1 <= seg_status.shape[1] <= 0xffff)
            max_segments = seg_status.shape[1]
        _raise(load_library().ugo_fec_ack_set_receive(
            self._h, info.data_ptr(), conn_of.data_ptr(), npk, None if seg_status is None else seg_status.data_ptr(),
            max_segments, now_us, _stream_handle(stream)))

    def touch(self, flags, stream=None):
        """changed = 1 for the members with flags[c] != 0 (uint8 [nconn])."""
        self.check_per_conn(flags, 1, "flags")
        _raise(load_library().ugo_fec_ack_set_touch(self._h, flags.data_ptr(), _stream_handle(stream)))

    def attach(self, now_us: int, first_packet, n_packets, total, info, ranges, conn_of, may_ack_only=None,
               total_out=None, attached=None, stream=None):
        """ugo_fec_ack_set_attach: first_packet int64 [nconn], n_packets int32
        [nconn] and total int64 [1] as StreamTxSet.plan returned them; info uint8
        [max_packets, 64], ranges int64 [max_packets, max_ranges, 2] and conn_of
        int32 [max_packets] the arrays StreamTxSet.encode will be given;
        may_ack_only uint8 [nconn] or None.  Returns (total_out int64 [1],
        attached uint8 [nconn] of ACK_*); both may be given, and total_out may
        be total itself."""
        max_packets = info.shape[0]
        _require(0 <= now_us < 1 << 64 and max_packets <= 1 << 31)
        _check_info(info, max_packets)
        _check_ranges(ranges, max_packets, max_ranges=0xffff)
        _check_tensor(conn_of, max_packets, 4, integer=True)
        self.check_per_conn(first_packet, 8, "first_packet")
        self.check_per_conn(n_packets, 4, "n_packets")
        # kept: the single counts are checked for size alone here, for layout too in the stream and loop families
        _require(total.numel() == 1 and total.element_size() == 8)
        if may_ack_only is not None:
            self.check_per_conn(may_ack_only, 1, "may_ack_only")
        dev = self._dev()
        if total_out is None:
            total_out = torch.zeros(1, dtype=torch.int64, device=dev)
        if attached is None:
            attached = torch.zeros(self.nconn, dtype=torch.uint8, device=dev)
        _require(total_out.numel() == 1 and total_out.element_size() == 8)
        self.check_per_conn(attached, 1, "attached")
        _raise(load_library().ugo_fec_ack_set_attach(
            self._h, now_us, first_packet.data_ptr(), n_packets.data_ptr(), total.data_ptr(),
            None if may_ack_only is None else may_ack_only.data_ptr(), max_packets, info.data_ptr(),
            ranges.data_ptr() if ranges.numel() else None, ranges.shape[1], conn_of.data_ptr(), total_out.data_ptr(),
            attached.data_ptr(), _stream_handle(stream)))
        return total_out, attached

    def states(self) -> np.ndarray:
        """The members' records (ACK_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, ACK_STATE_DTYPE)
        _raise(load_library().ugo_fec_ack_set_state(self._h, out.ctypes.data))
        return out
