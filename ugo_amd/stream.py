"""include/ugo_stream.h: receive windows (batch Conn.handleSegment and
Conn.Read) and send windows (batch Conn.Write, PopSegments and encode), one
connection each, and the sets that serve many connections per call."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

# STREAM_SET_MAX_CONN is this header's, re-exported from the base: the member-set base of every family needs it
from .abi import (STREAM_SET_MAX_CONN, _check_info, _check_ranges, _check_segs, _check_tensor,  # noqa: F401
                  _Handle, _MemberSet, _raise, _require, _stream_handle, load_library, torch)
from .encoder import PKT_FEC_FRAMED, Encoder

# ugo_stream_status (per segment; the last two are the connection's err) and the record
STREAM_NONE = 0
STREAM_ACCEPTED = 1
STREAM_DUPLICATE = 2
STREAM_OUT_OF_WINDOW = 3
STREAM_OVERLAP = 4
STREAM_TOO_MANY_GAPS = 5
STREAM_MAX_GAPS = 50
STREAM_MIN_WINDOW = 4096
STREAM_NO_CONN = 0xffffffff   # conn_of: the packet belongs to no member of the set
STREAM_STATE_DTYPE = np.dtype([("read_pos", "<u8"), ("head_off", "<u8"), ("hi", "<u8"), ("readable", "<u8"),
                               ("accepted", "<u8"), ("duplicate", "<u8"), ("out_of_window", "<u8"),
                               ("skipped_packets", "<u8"), ("ordered_segments", "<u8"), ("err_packet", "<u8"),
                               ("err_segment", "<u4"), ("err", "<u4"), ("ngaps", "<u4"), ("head_valid", "u1"),
                               ("eof", "u1"), ("reserved", "u1", (2,))])
assert STREAM_STATE_DTYPE.itemsize == 96
# send windows
STREAM_TX_MAX_WINDOW = 1 << 31
STREAM_TX_HEADER = 4  # frameHeaderLen of segment_sender.go: H of THE RULE
STREAM_TX_RQ_QUEUED = 1
STREAM_TX_RQ_REJECTED = 2
STREAM_TX_RQ_FULL = 3
STREAM_TX_RQ_UNSORTED = 4
STREAM_TX_RQ_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("reserved", "<u4")])
STREAM_TX_STATE_DTYPE = np.dtype([("base", "<u8"), ("write_pos", "<u8"), ("tail", "<u8"),
                                  ("last_packet_number", "<u8"), ("packets", "<u8"), ("segments", "<u8"),
                                  ("bytes_new", "<u8"), ("bytes_retransmitted", "<u8"), ("rq_rejected", "<u8"),
                                  ("rq_len", "<u4"), ("rq_head", "<u4")])
assert STREAM_TX_STATE_DTYPE.itemsize == 80 and STREAM_TX_RQ_DTYPE.itemsize == 16


class StreamRx(_Handle):
    """A connection's receive window on the GPU (include/ugo_stream.h): batch
    Conn.handleSegment (deliver) and Conn.Read (read) behind packet_decode."""

    _destroy = "ugo_fec_stream_rx_destroy"

    def __init__(self, enc: Encoder, window_bytes: int):
        self.check_window(window_bytes)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_stream_rx_create(enc._h, window_bytes, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the window
        self.window_bytes = window_bytes
        self.device = enc.device

    @staticmethod
    def check_window(window_bytes: int):
        _require(window_bytes >= STREAM_MIN_WINDOW and window_bytes & (window_bytes - 1) == 0,
                 f"window_bytes must be a power of two >= {STREAM_MIN_WINDOW}")

    @staticmethod
    def check_batch(slot: int, pkts_ptr: int, pad_ptr: Optional[int]):
        _require(slot % 16 == 0 and 0 < slot <= 0xffff, "slot must be a multiple of 16, at most 0xffff")
        _require(pkts_ptr % 16 == 0 and (pad_ptr is None or pad_ptr % 16 == 0), "pkts and pad must be 16-B aligned")

    def deliver(self, pkts, info, segs, pad=None, stream=None, out=None):
        """ugo_fec_stream_deliver: pkts = uint8 CUDA [npk, slot] (still encrypted),
        info / segs as packet_decode returned them, pad = the decoder's keystream
        or None.  Returns seg_status, uint8 CUDA [npk, max_segments] of STREAM_*
        (out = such a tensor to reuse).  Nothing is synchronised."""
        npk, slot = pkts.shape
        _require(pkts.is_contiguous() and pkts.element_size() == 1)
        _check_info(info, npk)
        _check_segs(segs, npk)
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        StreamRx.check_batch(slot, pkts.data_ptr(), None if pad is None else pad.data_ptr())
        max_segments = segs.shape[1]
        if out is None:
            out = torch.empty((npk, max_segments), dtype=torch.uint8, device=pkts.device)
        _require(tuple(out.shape) == (npk, max_segments) and out.is_contiguous() and out.element_size() == 1)
        _raise(load_library().ugo_fec_stream_deliver(
            self._h, pkts.data_ptr(), slot, None if pad is None else pad.data_ptr(), info.data_ptr(),
            segs.data_ptr(), max_segments, npk, out.data_ptr(), _stream_handle(stream)))
        return out

    def read(self, n: int, out=None, discard: bool = False, stream=None, n_read=None, eof=None):
        """ugo_fec_stream_read, Conn.Read(p[:n]) that never waits.  Returns CUDA
        tensors (buf uint8 [n] -- None with discard --, n_read int64 [1], eof uint8
        [1]): buf[:n_read] holds the bytes.  out (any alignment), n_read and eof
        may be given, in device or pinned host memory.  Nothing is synchronised."""
        _require(n >= 0)
        dev = self._dev()
        if discard:
            out = None
        elif out is None:
            out = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        if out is not None:
            _require(out.is_contiguous() and out.element_size() == 1 and out.numel() >= n)
        if n_read is None:
            n_read = torch.zeros(1, dtype=torch.int64, device=dev)
        if eof is None:
            eof = torch.zeros(1, dtype=torch.uint8, device=dev)
        _require(n_read.numel() == 1 and n_read.element_size() == 8 and eof.numel() == 1 and eof.element_size() == 1)
        _raise(load_library().ugo_fec_stream_read(self._h, None if out is None else out.data_ptr(), n,
                                                  n_read.data_ptr(), eof.data_ptr(), _stream_handle(stream)))
        return out, n_read, eof

    def state(self) -> np.ndarray:
        """The connection's record (STREAM_STATE_DTYPE scalar); waits for the last deliver / read."""
        out = np.zeros(1, STREAM_STATE_DTYPE)
        _raise(load_library().ugo_fec_stream_rx_state(self._h, out.ctypes.data))
        return out[0]

    def window(self):
        """The window as a uint8 CUDA tensor [window_bytes] over the device memory
        itself (stream byte x at index x & (window_bytes - 1)); valid while this
        object lives."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_stream_rx_window(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value)


class StreamRxSet(_MemberSet):
    """An ordered set of receive windows (ugo_fec_stream_set_*, include/ugo_stream.h):
    one deliver for a batch that holds the packets of many connections, one read
    for all of them.  The set does not own its members; close it before them."""

    _member, _nouns, _attr = StreamRx, ("window", "windows"), "rxs"
    _create, _destroy = "ugo_fec_stream_set_create", "ugo_fec_stream_set_destroy"

    @staticmethod
    def check_conn_of(conn_of, npk: int):
        _check_tensor(conn_of, npk, 4, "conn_of", "npackets", integer=True)

    def deliver(self, pkts, info, segs, conn_of, pad=None, stream=None, out=None):
        """ugo_fec_stream_set_deliver: StreamRx.deliver with conn_of, int32 [npk]
        in device or pinned host memory -- the member index of each packet
        (STREAM_NO_CONN as -1, or any index >= nconn: no connection).  Returns
        seg_status, uint8 [npk, max_segments].  Nothing is synchronised."""
        npk, slot = pkts.shape
        _require(pkts.is_contiguous() and pkts.element_size() == 1)
        _check_info(info, npk)
        _check_segs(segs, npk)
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        StreamRx.check_batch(slot, pkts.data_ptr(), None if pad is None else pad.data_ptr())
        self.check_conn_of(conn_of, npk)
        max_segments = segs.shape[1]
        if out is None:
            out = torch.empty((npk, max_segments), dtype=torch.uint8, device=pkts.device)
        _require(tuple(out.shape) == (npk, max_segments) and out.is_contiguous() and out.element_size() == 1)
        _raise(load_library().ugo_fec_stream_set_deliver(
            self._h, pkts.data_ptr(), slot, None if pad is None else pad.data_ptr(), info.data_ptr(),
            segs.data_ptr(), max_segments, npk, conn_of.data_ptr(), out.data_ptr(), _stream_handle(stream)))
        return out

    def read(self, n, dst=None, dst_off=None, stream=None, n_read=None, eof=None):
        """ugo_fec_stream_set_read: n = int64 [nconn] bytes wanted per member (0
        skips it), dst = uint8 buffer or None to discard, dst_off = int64 [nconn]
        offsets into dst (the caller keeps the ranges disjoint and inside dst).
        Returns (n_read int64 [nconn], eof uint8 [nconn]); both may be given.
        Operands in device or pinned host memory.  Nothing is synchronised."""
        dev = self._dev()
        self.check_per_conn(n, 8, "n")
        if dst is not None:
            _require(dst.is_contiguous() and dst.element_size() == 1)
            _require(dst_off is not None, "dst needs dst_off")
            self.check_per_conn(dst_off, 8, "dst_off")
        if n_read is None:
            n_read = torch.zeros(self.nconn, dtype=torch.int64, device=dev)
        if eof is None:
            eof = torch.zeros(self.nconn, dtype=torch.uint8, device=dev)
        self.check_per_conn(n_read, 8, "n_read")
        self.check_per_conn(eof, 1, "eof")
        _raise(load_library().ugo_fec_stream_set_read(
            self._h, None if dst is None else dst.data_ptr(), None if dst is None else dst_off.data_ptr(),
            n.data_ptr(), n_read.data_ptr(), eof.data_ptr(), _stream_handle(stream)))
        return n_read, eof

    def states(self) -> np.ndarray:
        """The members' records (STREAM_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, STREAM_STATE_DTYPE)
        _raise(load_library().ugo_fec_stream_set_state(self._h, out.ctypes.data))
        return out


class StreamTx(_Handle):
    """A connection's send window on the GPU (include/ugo_stream.h, send
    windows): its unsent and unacknowledged stream bytes and its retransmission
    queue.  Every call goes through a StreamTxSet; a set of one is the
    single-connection form."""

    _destroy = "ugo_fec_stream_tx_destroy"

    def __init__(self, enc: Encoder, window_bytes: int, rq_cap: int = 64, start_offset: int = 0,
                 start_packet_number: int = 0):
        self.check_create(window_bytes, rq_cap)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_stream_tx_create(enc._h, window_bytes, rq_cap, start_offset,
                                                       start_packet_number, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the window
        self.window_bytes, self.rq_cap = window_bytes, rq_cap
        self.device = enc.device

    @staticmethod
    def check_create(window_bytes: int, rq_cap: int):
        _require(STREAM_MIN_WINDOW <= window_bytes <= STREAM_TX_MAX_WINDOW and window_bytes & (window_bytes - 1) == 0,
                 f"window_bytes must be a power of two in [{STREAM_MIN_WINDOW}, 2^31]")
        _require(1 <= rq_cap <= 1 << 24, "rq_cap must be in [1, 2^24]")

    def window(self):
        """The window as a uint8 CUDA tensor [window_bytes] over the device memory
        itself (stream byte x at index x & (window_bytes - 1))."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_stream_tx_window(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value)

    def queue(self):
        """The retransmission ring as a uint8 CUDA tensor [rq_cap, 16] over the
        device memory itself (view on the host with STREAM_TX_RQ_DTYPE)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_stream_tx_queue(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value * 16).view(n.value, 16)


class StreamTxSet(_MemberSet):
    """An ordered set of send windows (ugo_fec_stream_tx_set_*): write, plan and
    encode for all of them per call, release and retransmit for what ARQ on the
    host decides.  Per-connection operands are tensors of nconn elements in
    device or pinned host memory.  Nothing is synchronised but states().  The
    set does not own its members; close it before them."""

    _member, _nouns, _attr = StreamTx, ("window", "windows"), "txs"
    _create, _destroy = "ugo_fec_stream_tx_set_create", "ugo_fec_stream_tx_set_destroy"

    @staticmethod
    def check_plan(max_payload: int, max_segments: int, max_packets: int):
        _require(16 <= max_payload <= 0xffff, "max_payload must be in [16, 0xffff]")
        _require(1 <= max_segments <= 0xffff, "max_segments must be in [1, 0xffff]")
        _require(0 <= max_packets <= 1 << 31, "max_packets must be at most 2^31")

    def write(self, src, src_off, n, n_written=None, stream=None):
        """Conn.Write that never waits: n[c] bytes from src[src_off[c]:] (uint8,
        any alignment; int64 [nconn] both) to member c, as many as its window
        has room for.  Returns n_written int64 [nconn]."""
        _require(src.is_contiguous() and src.element_size() == 1)
        self.check_per_conn(src_off, 8, "src_off")
        self.check_per_conn(n, 8, "n")
        if n_written is None:
            n_written = torch.zeros(self.nconn, dtype=torch.int64, device=self._dev())
        self.check_per_conn(n_written, 8, "n_written")
        _raise(load_library().ugo_fec_stream_tx_set_write(self._h, src.data_ptr(), src_off.data_ptr(), n.data_ptr(),
                                                          n_written.data_ptr(), _stream_handle(stream)))
        return n_written

    def release(self, upto, stream=None):
        """The peer acknowledged everything below upto[c] (int64 [nconn])."""
        self.check_per_conn(upto, 8, "upto")
        _raise(load_library().ugo_fec_stream_tx_set_release(self._h, upto.data_ptr(), _stream_handle(stream)))

    def retransmit(self, conn_of, offset, length, status=None, stream=None):
        """Queue segments for retransmission: conn_of int32 [m] (non-decreasing),
        offset int64 [m], length int32 [m].  Returns status uint8 [m] of
        STREAM_TX_RQ_*."""
        m = conn_of.numel()
        # kept: exactly m elements here, where SentTxSet's lists may be longer than the count they are given
        _check_tensor(conn_of, m, 4, "conn_of", integer=True)
        _check_tensor(offset, m, 8, "offset", integer=True)
        _check_tensor(length, m, 4, "length", integer=True)
        if status is None:
            status = torch.zeros(m, dtype=torch.uint8, device=self._dev())
        _check_tensor(status, m, 1, "status", integer=True)
        _raise(load_library().ugo_fec_stream_tx_set_retransmit(
            self._h, conn_of.data_ptr(), offset.data_ptr(), length.data_ptr(), m, status.data_ptr(),
            _stream_handle(stream)))
        return status

    def plan(self, budget, max_packets: int, max_payload: int = 1436, max_segments: int = 8, out=None, stream=None):
        """The loop of Conn.sendPacket for every member (THE RULE of
        include/ugo_stream.h): budget int32 [nconn] packets at the most per
        member.  Returns (info uint8 [max_packets, 64], segs uint8 [max_packets,
        max_segments, 16], conn_of int32 [max_packets], first_packet int64
        [nconn], n_packets int32 [nconn], total int64 [1]); out = such a tuple
        to reuse."""
        self.check_plan(max_payload, max_segments, max_packets)
        self.check_per_conn(budget, 4, "budget")
        dev = self._dev()
        if out is None:
            out = (torch.zeros((max_packets, 64), dtype=torch.uint8, device=dev),
                   torch.zeros((max_packets, max_segments, 16), dtype=torch.uint8, device=dev),
                   torch.zeros(max_packets, dtype=torch.int32, device=dev),
                   torch.zeros(self.nconn, dtype=torch.int64, device=dev),
                   torch.zeros(self.nconn, dtype=torch.int32, device=dev),
                   torch.zeros(1, dtype=torch.int64, device=dev))
        info, segs, conn_of, first_packet, n_packets, total = out
        _check_info(info, max_packets)
        _check_segs(segs, max_packets)
        _require(segs.shape[1] == max_segments)  # its own output: exactly max_segments a packet
        _check_tensor(conn_of, max_packets, 4, "conn_of", integer=True)
        self.check_per_conn(first_packet, 8, "first_packet")
        self.check_per_conn(n_packets, 4, "n_packets")
        _check_tensor(total, 1, 8, "total", integer=True)
        _raise(load_library().ugo_fec_stream_tx_set_plan(
            self._h, budget.data_ptr(), max_payload, max_segments, max_packets, info.data_ptr(), segs.data_ptr(),
            conn_of.data_ptr(), first_packet.data_ptr(), n_packets.data_ptr(), total.data_ptr(),
            _stream_handle(stream)))
        return out

    def encode(self, info, ranges, segs, conn_of, slot: int, npackets: Optional[int] = None, pad=None,
               framed: bool = False, stream=None, out=None):
        """Encoder.packet_encode with the segment bytes read from the members'
        windows: conn_of int32 [>= npackets] names packet i's member.  npackets
        defaults to info.shape[0]; the arrays may be longer (plan's
        max_packets).  Returns (wire uint8 [npackets, slot], wire_lens int16,
        status uint8)."""
        npk = info.shape[0] if npackets is None else npackets
        _require(0 <= npk <= info.shape[0])
        _check_info(info, npk, at_least=True)
        _check_ranges(ranges, npk, at_least=True)
        _check_segs(segs, npk, at_least=True)
        _check_tensor(conn_of, npk, 4, at_least=True, integer=True)
        _require(not (framed and pad is not None), "framed packets are encrypted by tx_assemble: pad must be None")
        _require(slot % 16 == 0 and 0 < slot <= 0xffff, "slot must be a multiple of 16, at most 0xffff")
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        if out is not None:
            wire, wire_lens, status = out
            _require(wire.dim() == 2 and wire.shape[0] >= npk and wire.shape[1] == slot and wire.is_contiguous() and
                     wire.element_size() == 1)
            _require(wire_lens.numel() >= npk and wire_lens.element_size() == 2 and wire_lens.is_contiguous())
            _require(status.numel() >= npk and status.element_size() == 1 and status.is_contiguous())
        else:
            dev = info.device
            wire = torch.zeros((npk, slot), dtype=torch.uint8, device=dev)
            wire_lens = torch.zeros(npk, dtype=torch.int16, device=dev)
            status = torch.zeros(npk, dtype=torch.uint8, device=dev)
        _raise(load_library().ugo_fec_stream_tx_set_encode(
            self._h, info.data_ptr(), ranges.data_ptr(), ranges.shape[1], segs.data_ptr(), segs.shape[1],
            conn_of.data_ptr(), npk, None if pad is None else pad.data_ptr(), PKT_FEC_FRAMED if framed else 0,
            wire.data_ptr(), slot, wire_lens.data_ptr(), status.data_ptr(), _stream_handle(stream)))
        return wire, wire_lens, status

    def states(self) -> np.ndarray:
        """The members' records (STREAM_TX_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, STREAM_TX_STATE_DTYPE)
        _raise(load_library().ugo_fec_stream_tx_set_state(self._h, out.ctypes.data))
        return out
