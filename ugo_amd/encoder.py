"""include/ugo_fec.h and include/ugo_pkt.h: the (d, p) code bound to one GPU,
group assembly, the packet codec, launch timing and the host-buffer paths."""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np

from .abi import (OK, ErrSingular, ErrTooFewShards, _check_info, _check_ranges, _check_segs, _Handle, _raise,
                  _require, _stream_handle, check_shards, load_library, strerror, torch)

RECONSTRUCT_DATA_ONLY = 1
# include/ugo_fec.h launch timing
KERNEL_NAMES = {1: "encode", 2: "reconstruct", 3: "prepare", 4: "bytes", 5: "rx_assemble", 6: "tx_assemble",
                7: "packet_decode", 8: "packet_encode", 9: "stream_deliver", 10: "stream_read", 11: "stream_tx",
                12: "ack", 13: "sent", 14: "cc", 15: "listen", 16: "loop"}
KERNEL_IDS = {v: k for k, v in KERNEL_NAMES.items()}
LAUNCH_TIME_DTYPE = np.dtype([("kernel", "<u4"), ("ms", "<f4")])
# include/ugo_pkt.h
PKT_FEC_FRAMED = 1
PKT_CAPACITY = 6
PKT_INCONSISTENT_LARGEST_ACKED = 7  # packet_encode's per-packet statuses
PKT_INCONSISTENT_LOWEST_ACKED = 8
PKT_INCONSISTENT_RANGE_COUNT = 9
PKT_OUT_OF_WINDOW = 10  # stream_tx set_encode: a segment outside its send window
PKT_INFO_DTYPE = np.dtype([("packet_number", "<u8"), ("stop_waiting", "<u8"), ("largest_acked", "<u8"),
                           ("largest_in_order", "<u8"), ("delay_us", "<u8"), ("status", "<u4"),
                           ("payload_off", "<u4"), ("n_ranges", "<u2"), ("n_segments", "<u2"), ("flags", "u1"),
                           ("fec_flag_lo", "u1"), ("reserved", "u1", (10,))])
PKT_SEGMENT_DTYPE = np.dtype([("offset", "<u8"), ("data_off", "<u4"), ("len", "<u2"), ("avail", "<u2")])
assert PKT_INFO_DTYPE.itemsize == 64 and PKT_SEGMENT_DTYPE.itemsize == 16


class Encoder(_Handle):
    """A (d, p) code bound to one GPU (reedsolomon.Encoder equivalent)."""

    _destroy = "ugo_fec_destroy"

    def __init__(self, data_shards: int, parity_shards: int, device: int = 0):
        lib = load_library()
        h = ctypes.c_void_p()
        _raise(lib.ugo_fec_create(device, data_shards, parity_shards, ctypes.byref(h)))
        self._h = h
        self.DataShards = data_shards
        self.ParityShards = parity_shards
        self.Shards = data_shards + parity_shards
        self.mask_words = (self.Shards + 63) // 64  # presence words per group (include/ugo_fec.h)
        self.device = device

    def close(self):  # the one owner with more than a handle: its pinned staging buffer goes after the context
        super().close()
        if getattr(self, "_stage_buf", None) is not None:
            host_free(self._stage_buf)
            self._stage_buf = None

    def matrix(self) -> np.ndarray:
        out = np.zeros((self.Shards, self.DataShards), np.uint8)
        _raise(load_library().ugo_fec_matrix(self._h, out.ctypes.data))
        return out

    # -------------------------------------------------- device-resident batch
    def _geom(self, shards, shard_major: bool):
        """(groups, pitch, row_stride, group_stride) of a uint8 tensor whose
        last dimension is contiguous: group-major [G, d+p, pitch] or
        shard-major [d+p, G, pitch] (planar); the row and group strides are the
        tensor's own (a padded row stride is a strided view)."""
        _require(shards.dim() == 3 and shards.element_size() == 1 and shards.stride(2) == 1)
        if shard_major:
            n, G, pitch = shards.shape
            rs, gs = shards.stride(0), shards.stride(1)
        else:
            G, n, pitch = shards.shape
            gs, rs = shards.stride(0), shards.stride(1)
        _require(n == self.Shards, f"expected {self.Shards} rows per group, got {n}")
        return G, pitch, rs, gs

    def encode_batch(self, shards, shard_size: Optional[int] = None, stream=None, shard_major: bool = False):
        """Encode every group of a device tensor: [G, d+p, pitch] (default) or,
        with shard_major=True, the planar [d+p, G, pitch] layout."""
        G, pitch, rs, gs = self._geom(shards, shard_major)
        S = pitch if shard_size is None else shard_size
        _raise(load_library().ugo_fec_encode_strided(self._h, shards.data_ptr(), G, S, rs, gs,
                                                     _stream_handle(stream)))

    def reconstruct_batch(self, shards, present, shard_size: Optional[int] = None, data_only=False,
                          status=None, stream=None, shard_major: bool = False):
        """present: int64/uint64 CUDA tensor [G] of presence bitmasks (bit r = shard r
        non-empty), [G][W] words for d+p > 64 (W = mask_words); status: optional int8
        CUDA tensor [G]."""
        G, pitch, rs, gs = self._geom(shards, shard_major)
        _require(present.is_contiguous() and present.numel() == G * self.mask_words and present.element_size() == 8)
        S = pitch if shard_size is None else shard_size
        st = None if status is None else status.data_ptr()
        _raise(load_library().ugo_fec_reconstruct_strided(self._h, shards.data_ptr(), present.data_ptr(), G, S, rs,
                                                          gs, RECONSTRUCT_DATA_ONLY if data_only else 0, st,
                                                          _stream_handle(stream)))

    def reconstruct_into(self, shards, present, out, shard_size: Optional[int] = None, data_only=False,
                         status=None, stream=None, shard_major: bool = False, out_shard_major: bool = True):
        """Reconstruct with a separate output batch (include/ugo_fec.h
        ugo_fec_reconstruct_into): `shards` is only read; output i of group g (the
        i-th erased row, ascending) goes to `out`, a contiguous uint8 CUDA tensor
        [p][G][opitch] (out_shard_major) or [G][p][opitch]."""
        G, pitch, rs, gs = self._geom(shards, shard_major)
        _require(present.is_contiguous() and present.numel() == G * self.mask_words and present.element_size() == 8)
        _require(out.is_contiguous() and out.element_size() == 1 and out.dim() == 3)
        p = self.ParityShards
        if out_shard_major:
            _require(out.shape[0] == p and out.shape[1] == G)
            opitch = out.shape[2]
            ors, ogs = G * opitch, opitch
        else:
            _require(out.shape[0] == G and out.shape[1] == p)
            opitch = out.shape[2]
            ors, ogs = opitch, p * opitch
        S = pitch if shard_size is None else shard_size
        _require(opitch >= S)
        st = None if status is None else status.data_ptr()
        _raise(load_library().ugo_fec_reconstruct_into(self._h, shards.data_ptr(), present.data_ptr(), G, S, rs, gs,
                                                       out.data_ptr(), ors, ogs,
                                                       RECONSTRUCT_DATA_ONLY if data_only else 0, st,
                                                       _stream_handle(stream)))

    def lossy_groups(self, present, data_only: bool = True, out=None, count=None, stream=None):
        """ugo_fec_lossy_groups: the groups of `present` (int64 CUDA [G]) with an
        erased row to rebuild (data rows only with data_only), ascending.  Returns
        (list, count): an int32 CUDA tensor [G] whose first *count entries are the
        groups, and an int32 CUDA tensor [1]; nothing is synchronised."""
        import torch

        G = present.numel()
        _require(present.is_contiguous() and present.element_size() == 8 and self.mask_words == 1)
        lst = torch.empty(max(G, 1), dtype=torch.int32, device=present.device) if out is None else out
        cnt = torch.empty(1, dtype=torch.int32, device=present.device) if count is None else count
        _require(lst.numel() >= G and lst.element_size() == 4 and cnt.element_size() == 4)
        _raise(load_library().ugo_fec_lossy_groups(self._h, present.data_ptr(), G,
                                                   RECONSTRUCT_DATA_ONLY if data_only else 0, lst.data_ptr(),
                                                   cnt.data_ptr(), _stream_handle(stream)))
        return lst, cnt

    def reconstruct_list(self, shards, present, lst, count, out, shard_size: Optional[int] = None,
                         data_only: bool = True, status=None, stream=None, shard_major: bool = True,
                         max_entries: Optional[int] = None):
        """ugo_fec_reconstruct_list: Reconstruct the groups lst[0 .. *count) of the
        batch; output i of list entry j goes to out[j, i] (out: contiguous uint8
        CUDA tensor [max_entries][slots][opitch], compact in list order) or, out =
        None, in place.  status: int8 CUDA [max_entries] (entry j's status)."""
        G, pitch, rs, gs = self._geom(shards, shard_major)
        _require(present.is_contiguous() and present.numel() == G and present.element_size() == 8)
        m = G if max_entries is None else max_entries
        S = pitch if shard_size is None else shard_size
        ors = oes = 0
        if out is not None:
            _require(out.is_contiguous() and out.element_size() == 1 and out.dim() == 3 and out.shape[0] >= m)
            ors, oes = out.shape[2], out.shape[1] * out.shape[2]
            _require(out.shape[2] >= S)
        _raise(load_library().ugo_fec_reconstruct_list(
            self._h, shards.data_ptr(), present.data_ptr(), G, lst.data_ptr(), count.data_ptr(), m, S, rs, gs,
            None if out is None else out.data_ptr(), ors, oes, RECONSTRUCT_DATA_ONLY if data_only else 0,
            None if status is None else status.data_ptr(), _stream_handle(stream)))

    def recover_data(self, shards, present, out, index, count=None, shard_size: Optional[int] = None,
                     stream=None, shard_major: bool = True):
        """ugo_fec_recover_data: `input`'s recovered data shards of a device batch,
        row-compact in `recovered` order: out[r, :shard_size] (out: contiguous
        uint8 CUDA [max_rows, row]), index[r] = group*(d+p) + row (int32 CUDA
        [max_rows]); returns count (int32 CUDA [1], the number recovered,
        written on the stream)."""
        import torch

        G, pitch, rs, gs = self._geom(shards, shard_major)
        _require(present.is_contiguous() and present.numel() == G and present.element_size() == 8)
        S = pitch if shard_size is None else shard_size
        _require(out.is_contiguous() and out.element_size() == 1 and out.dim() == 2 and out.shape[1] >= S)
        _require(index.is_contiguous() and index.element_size() == 4 and index.numel() >= out.shape[0])
        cnt = torch.empty(1, dtype=torch.int32, device=present.device) if count is None else count
        _raise(load_library().ugo_fec_recover_data(
            self._h, shards.data_ptr(), present.data_ptr(), G, S, rs, gs, out.data_ptr(), out.shape[1], out.shape[0],
            index.data_ptr(), cnt.data_ptr(), _stream_handle(stream)))
        return cnt

    def rx_recover_host(self, wire: np.ndarray, lens: np.ndarray, shard_size: int, groups: int,
                        first_group: int = 0, pad: Optional[bytes] = None, out: Optional[np.ndarray] = None,
                        max_out: Optional[int] = None, present_out: Optional[np.ndarray] = None,
                        out_index: Optional[np.ndarray] = None):
        """ugo_fec_rx_recover_host: the RX path host memory to host memory.  wire =
        uint8 [npk, slot] (pinned for DMA rates), lens = uint16 [npk].  Returns
        (n, index, out, stats): n recovered data shards, the first
        min(n, max_out) of them row-compact in out[r, :shard_size] (out: uint8
        [max_out, row] with row >= shard_size, allocated if None) in ugo's
        `recovered` order, index[r] = window group * (d+p) + row (index: out_index,
        uint32 [>= max_out], or allocated if None).  out's row stride is its second
        dimension; only out[r, :shard_size] and index[r] for r < min(n, max_out)
        are written."""
        npk, slot = wire.shape
        _require(wire.flags.c_contiguous and wire.itemsize == 1)
        _require(lens.flags.c_contiguous and lens.size == npk and lens.itemsize == 2)
        _require(pad is None or len(pad) >= slot, "pad must hold at least slot_stride keystream bytes")
        if present_out is not None:  # C writes groups * 8 bytes there
            _require(isinstance(present_out, np.ndarray) and present_out.flags.c_contiguous
                     and present_out.itemsize == 8 and present_out.size >= groups)
        m = groups * min(self.DataShards, self.ParityShards) if max_out is None else max_out
        if out is None:
            out = np.zeros((max(m, 1), (shard_size + 15) // 16 * 16), np.uint8)
        _require(out.ndim == 2 and out.flags.c_contiguous and out.shape[0] >= m and out.shape[1] >= shard_size)
        index = np.zeros(max(m, 1), np.uint32) if out_index is None else out_index
        _require(isinstance(index, np.ndarray) and index.flags.c_contiguous and index.itemsize == 4
                 and index.size >= m)
        stats = np.zeros(5, np.uint32)
        padb = None if pad is None else np.frombuffer(bytes(pad), np.uint8)
        n_out = ctypes.c_size_t(0)
        _raise(load_library().ugo_fec_rx_recover_host(
            self._h, wire.ctypes.data, slot, lens.ctypes.data, npk, None if padb is None else padb.ctypes.data,
            first_group, groups, shard_size, None if present_out is None else present_out.ctypes.data,
            stats.ctypes.data, out.ctypes.data, out.shape[1], m, index.ctypes.data, ctypes.byref(n_out)))
        return n_out.value, index, out, stats

    def tx_assemble_host(self, pkts: np.ndarray, lens: np.ndarray, wire: np.ndarray, wire_lens: np.ndarray,
                         first_seq: int = 0, pad: Optional[bytes] = None, max_len: int = 1476,
                         status: Optional[np.ndarray] = None):
        """ugo_fec_tx_assemble_host: tx_assemble with host numpy buffers (pinned for
        DMA rates): pkts uint8 [G*d, slot_in], lens uint16 [G*d], wire uint8
        [G*(d+p), slot_out], wire_lens uint16 [G*(d+p)], status int8 [G] or None."""
        d, n = self.DataShards, self.Shards
        _require(pkts.ndim == 2 and wire.ndim == 2 and pkts.shape[0] % d == 0)
        G = pkts.shape[0] // d
        _require(lens.size == G * d and wire.shape[0] == G * n and wire_lens.size == G * n)
        # the C side copies G*d*2, G*n*2 and G bytes and reads round_up(max_len, 16) pad bytes
        for a in (pkts, wire, lens, wire_lens):
            _require(isinstance(a, np.ndarray) and a.flags.c_contiguous)
        _require(pkts.itemsize == 1 and wire.itemsize == 1 and lens.itemsize == 2 and wire_lens.itemsize == 2)
        if status is not None:
            _require(isinstance(status, np.ndarray) and status.flags.c_contiguous and status.size == G
                     and status.itemsize == 1)
        _require(pad is None or len(pad) >= (max_len + 15) // 16 * 16,
                 "pad must hold at least round_up(max_len, 16) keystream bytes")
        padb = None if pad is None else np.frombuffer(bytes(pad), np.uint8)
        _raise(load_library().ugo_fec_tx_assemble_host(
            self._h, pkts.ctypes.data, pkts.shape[1], lens.ctypes.data, G, first_seq,
            None if padb is None else padb.ctypes.data, max_len, wire.ctypes.data, wire.shape[1],
            wire_lens.ctypes.data, None if status is None else status.ctypes.data))

    def set_host_copy_queue(self, on: bool):
        """ugo_fec_set_host_copy_queue: the host paths' H2D copies on a
        low-priority stream (a hardware-queue pool of its own)."""
        _raise(load_library().ugo_fec_set_host_copy_queue(self._h, 1 if on else 0))

    def set_tx_host_route(self, route: str):
        """ugo_fec_set_tx_host_route: tx_assemble_host's wire packets by D2H
        copy ("copy", the default) or written through the pinned buffer's
        mapping ("mapped")."""
        _require(route in ("copy", "mapped"))
        _raise(load_library().ugo_fec_set_tx_host_route(self._h, {"copy": 0, "mapped": 1}[route]))

    def reconstruct_rows(self, rows, present, out, shard_size: int, data_only=False, status=None, stream=None,
                         out_shard_major: bool = True):
        """Reconstruct from a row-pointer table (include/ugo_fec.h
        ugo_fec_reconstruct_rows): rows = int64 tensor [G, d+p] of device
        addresses (device tensor, or pinned host memory as a numpy array /
        CPU tensor viewed through ugo_fec_device_address), present = [G] masks
        (device tensor or pinned numpy array), out = contiguous uint8 CUDA
        tensor [p][G][opitch] (out_shard_major) or [G][p][opitch]."""
        G = present.shape[0]
        _require(rows.shape[0] == G and rows.shape[1] == self.Shards and self.Shards <= 64)
        p = self.ParityShards
        _require(out.dim() == 3 and out.is_contiguous() and out.element_size() == 1)
        if out_shard_major:
            _require(out.shape[0] == p and out.shape[1] == G)
            ors, ogs = G * out.shape[2], out.shape[2]
        else:
            _require(out.shape[0] == G and out.shape[1] == p)
            ors, ogs = out.shape[2], p * out.shape[2]
        _require(out.shape[2] >= shard_size)

        def ptr(x):
            return None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())

        _raise(load_library().ugo_fec_reconstruct_rows(self._h, ptr(rows), ptr(present), G, shard_size, ptr(out),
                                                       ors, ogs, RECONSTRUCT_DATA_ONLY if data_only else 0,
                                                       ptr(status), _stream_handle(stream)))

    def device_address(self, addr: int) -> int:
        """ugo_fec_device_address: the device address of host/device pointer addr."""
        out = ctypes.c_void_p()
        _raise(load_library().ugo_fec_device_address(self._h, ctypes.c_void_p(addr), ctypes.byref(out)))
        return out.value or 0

    def rx_assemble(self, wire, lens, shards, present, first_group: int = 0, shard_size: Optional[int] = None,
                    pad=None, stats=None, stream=None, shard_major: bool = True, frames: bool = False):
        """RX group assembly (include/ugo_fec.h ugo_fec_rx_assemble): wire = uint8 CUDA
        tensor [npk, slot] of received packets, lens = int16/uint16 CUDA tensor [npk];
        pad = uint8 CUDA keystream (>= slot bytes) or None; present = int64 CUDA [G]
        (zeroed by the caller); stats = int32 CUDA [5] (accepted, bad flag, out of
        window, too short, duplicate) or None.  A repeated seqid keeps its first
        copy in ring order (ugo/fec.go:123-129).  frames=True:
        ugo_fec_rx_assemble_frames -- a row holds the decrypted packet (payload at
        column 6, shard_size + 6 bytes); reconstruct it with shard_size + 6."""
        if stats is not None:
            _require(stats.numel() >= 5 and stats.element_size() == 4)
        G, pitch, rs, gs = self._geom(shards, shard_major)
        npk, slot = wire.shape
        _require(wire.is_contiguous() and lens.is_contiguous() and lens.element_size() == 2 and lens.numel() == npk)
        S = (pitch - 6 if frames else pitch) if shard_size is None else shard_size
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        entry = load_library().ugo_fec_rx_assemble_frames if frames else load_library().ugo_fec_rx_assemble
        _raise(entry(
            self._h, wire.data_ptr(), slot, lens.data_ptr(), npk, None if pad is None else pad.data_ptr(),
            first_group, G, shards.data_ptr(), S, rs, gs, present.data_ptr(),
            None if stats is None else stats.data_ptr(), _stream_handle(stream)))

    def tx_assemble(self, pkts, lens, wire, wire_lens, first_seq: int = 0, pad=None, max_len: int = 1476,
                    status=None, stream=None):
        """TX group assembly (include/ugo_fec.h ugo_fec_tx_assemble): pkts = uint8 CUDA
        tensor [G*d, slot_in] of outgoing data packets (6-B header space first),
        lens = int16/uint16 CUDA [G*d]; wire = uint8 CUDA [G*(d+p), slot_out],
        wire_lens = int16/uint16 CUDA [G*(d+p)]; pad = uint8 CUDA keystream or None;
        status = int8 CUDA [G] or None."""
        d, n = self.DataShards, self.Shards
        npk, slot_in = pkts.shape
        _require(npk % d == 0, "pkts must hold whole groups of d data packets")
        G = npk // d
        _require(wire.shape[0] == G * n and wire_lens.numel() == G * n and lens.numel() == npk)
        _require(pkts.is_contiguous() and wire.is_contiguous() and lens.is_contiguous() and wire_lens.is_contiguous())
        _require(lens.element_size() == 2 and wire_lens.element_size() == 2)
        if status is not None:
            _require(status.numel() == G and status.element_size() == 1)
        _raise(load_library().ugo_fec_tx_assemble(
            self._h, pkts.data_ptr(), slot_in, lens.data_ptr(), G, first_seq,
            None if pad is None else pad.data_ptr(), max_len, wire.data_ptr(), wire.shape[1],
            wire_lens.data_ptr(), None if status is None else status.data_ptr(), _stream_handle(stream)))

    def packet_decode(self, pkts, lens, pad=None, framed: bool = False, max_ranges: int = 32,
                      max_segments: int = 8, stream=None, out=None):
        """Batch ugoPacket.decode (include/ugo_pkt.h): pkts = uint8 CUDA [npk, slot],
        lens = int16/uint16 CUDA [npk].  Returns CUDA tensors (info [npk, 64] bytes --
        view on the host with PKT_INFO_DTYPE --, ranges int64 [npk, max_ranges, 2],
        segs [npk, max_segments, 16] bytes -- PKT_SEGMENT_DTYPE)."""
        npk, slot = pkts.shape
        _require(pkts.is_contiguous() and lens.is_contiguous() and lens.element_size() == 2 and lens.numel() == npk)
        dev = pkts.device
        if out is not None:  # reuse (info, ranges, segs) from an earlier call
            info, ranges, segs = out
            _require(info.shape == (npk, 64) and ranges.shape[0] == npk and segs.shape[0] == npk)
            _require(ranges.shape[1] >= max(max_ranges, 1) and segs.shape[1] >= max(max_segments, 1))
        else:
            info = torch.empty((npk, 64), dtype=torch.uint8, device=dev)
            ranges = torch.zeros((npk, max(max_ranges, 1), 2), dtype=torch.int64, device=dev)
            segs = torch.zeros((npk, max(max_segments, 1), 16), dtype=torch.uint8, device=dev)
        _raise(load_library().ugo_fec_packet_decode(
            self._h, pkts.data_ptr(), slot, lens.data_ptr(), npk, None if pad is None else pad.data_ptr(),
            PKT_FEC_FRAMED if framed else 0, info.data_ptr(), ranges.data_ptr(), max_ranges, segs.data_ptr(),
            max_segments, _stream_handle(stream)))
        return info, ranges, segs

    def packet_encode(self, info, ranges, segs, payload, slot: int, payload_stride: int = 0, pad=None,
                      framed: bool = False, stream=None, out=None):
        """Batch ugoPacket.encode (include/ugo_pkt.h ugo_fec_packet_encode), the
        reverse of packet_decode: info = uint8 CUDA [npk, 64] (PKT_INFO_DTYPE),
        ranges = int64 CUDA [npk, max_ranges, 2], segs = uint8 CUDA [npk,
        max_segments, 16] (PKT_SEGMENT_DTYPE); segment data is read from payload
        (uint8 CUDA, any alignment) at i*payload_stride + data_off.  framed: 6 B
        of zeroed header room in front (tx_assemble's input; pad must be None);
        else pad = uint8 CUDA keystream (>= slot bytes) or None.  Returns CUDA
        tensors (wire uint8 [npk, slot], wire_lens int16 [npk], status uint8
        [npk]); out = such a triple to reuse.  Only bytes [0, round_up(len, 16))
        of a slot are written."""
        npk = info.shape[0]
        _check_info(info, npk)
        _check_ranges(ranges, npk)
        _check_segs(segs, npk)
        _require(payload.is_contiguous() and payload.element_size() == 1)
        _require(not (framed and pad is not None), "framed packets are encrypted by tx_assemble: pad must be None")
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        if out is not None:
            wire, wire_lens, status = out
            _require(tuple(wire.shape) == (npk, slot) and wire.is_contiguous() and wire.element_size() == 1)
            _require(wire_lens.numel() == npk and wire_lens.element_size() == 2 and wire_lens.is_contiguous())
            _require(status.numel() == npk and status.element_size() == 1 and status.is_contiguous())
        else:
            dev = info.device
            wire = torch.zeros((npk, slot), dtype=torch.uint8, device=dev)
            wire_lens = torch.zeros(npk, dtype=torch.int16, device=dev)
            status = torch.zeros(npk, dtype=torch.uint8, device=dev)
        _raise(load_library().ugo_fec_packet_encode(
            self._h, info.data_ptr(), ranges.data_ptr(), ranges.shape[1], segs.data_ptr(), segs.shape[1],
            payload.data_ptr(), payload_stride, npk, None if pad is None else pad.data_ptr(),
            PKT_FEC_FRAMED if framed else 0, wire.data_ptr(), slot, wire_lens.data_ptr(), status.data_ptr(),
            _stream_handle(stream)))
        return wire, wire_lens, status

    # ---------------------------------------------------------- launch timing
    def timing_begin(self, max_launches: int):
        """Time the next max_launches kernel launches of this context with
        hipExtLaunchKernel start/stop events (kernel durations, nothing inserted
        between kernels).  Read them with timing_end()."""
        _raise(load_library().ugo_fec_timing_begin(self._h, max_launches))
        self._timing_cap = max_launches

    def timing_end(self):
        """Waits for the timed launches; returns (records, untimed): records is a
        LAUNCH_TIME_DTYPE array (kernel id, ms) in launch order, untimed the
        number of launches past max_launches."""
        cap = getattr(self, "_timing_cap", 0)
        out = np.zeros(cap, LAUNCH_TIME_DTYPE)
        n, untimed = ctypes.c_size_t(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_timing_end(self._h, out.ctypes.data if cap else None, cap, ctypes.byref(n),
                                                 ctypes.byref(untimed)))
        return out[:n.value], untimed.value

    # ------------------------------------------------------ host-buffer batch
    def service_start(self, idle_us: int = 0):
        """Per-call latency service (ugo_fec_service_start): small pinned host
        batches are served by a resident workgroup, no launch per call."""
        _raise(load_library().ugo_fec_service_start(self._h, idle_us))

    def service_stop(self):
        _raise(load_library().ugo_fec_service_stop(self._h))

    def service_config(self, timeout_ms: int = 0, grace_ms: int = 0, test_stall_us: int = 0):
        """The service's watchdog (ugo_fec_service_config): a call's wait for an
        answer and the wait for the workgroup to leave after a timeout (0 = 5000
        ms each); test_stall_us (tests only) delays every request it serves."""
        _raise(load_library().ugo_fec_service_config(self._h, timeout_ms, grace_ms, test_stall_us))

    @property
    def poisoned(self) -> bool:
        """True if a service workgroup never left after a failed call (every call
        on this context now fails; include/ugo_fec.h)."""
        return bool(load_library().ugo_fec_poisoned(self._h))

    def encode_host(self, shards: np.ndarray, shard_size: Optional[int] = None):
        _require(shards.dtype == np.uint8 and shards.flags["C_CONTIGUOUS"] and shards.ndim == 3)
        G, n, pitch = shards.shape
        _require(n == self.Shards)
        S = pitch if shard_size is None else shard_size
        _raise(load_library().ugo_fec_encode_host(self._h, shards.ctypes.data, G, S, pitch))

    def reconstruct_host(self, shards: np.ndarray, present: np.ndarray, shard_size: Optional[int] = None,
                         data_only=False, status: Optional[np.ndarray] = None) -> int:
        """Returns the aggregate status (0 or the first failing group's code);
        per-group codes go to `status` when given.  Does not raise for
        ErrTooFewShards groups (they are reported and left untouched)."""
        _require(shards.dtype == np.uint8 and shards.flags["C_CONTIGUOUS"] and shards.ndim == 3)
        G, n, pitch = shards.shape
        _require(n == self.Shards)
        present = np.ascontiguousarray(present, dtype=np.uint64)
        _require(present.size == G * self.mask_words)
        S = pitch if shard_size is None else shard_size
        st = None if status is None else status.ctypes.data
        if status is not None:
            _require(status.dtype == np.int8 and status.size == G)
        rc = load_library().ugo_fec_reconstruct_host(self._h, shards.ctypes.data, present.ctypes.data, G, S, pitch,
                                                     RECONSTRUCT_DATA_ONLY if data_only else 0, st)
        if rc not in (OK, ErrTooFewShards.code, ErrSingular.code):
            _raise(rc)
        return rc

    # ------------------------------------------- Go-shaped, one group per call
    def _stage(self, S: int) -> np.ndarray:
        """One pinned group [d+p][P] at the 16-B pitch P, reused across calls
        (the cgo shim's staging): the vector kernels, and the
        per-call service when it is on, serve it."""
        P = (S + 15) // 16 * 16
        need = self.Shards * P
        st = getattr(self, "_stage_buf", None)
        if st is None or st.size < need:
            if st is not None:
                host_free(st)
            st = self._stage_buf = host_alloc(max(need, self.Shards * 1488))
        return st[:need].reshape(1, self.Shards, P)

    def Encode(self, shards: List[bytearray]) -> None:
        """reedsolomon Encode: parity shards written in place (ugo/fec.go:238)."""
        if len(shards) != self.Shards:
            raise ErrTooFewShards(strerror(ErrTooFewShards.code))
        S = check_shards([len(s) for s in shards], nil_ok=False)
        buf = self._stage(S)
        for k in range(self.DataShards):
            buf[0, k, :S] = np.frombuffer(bytes(shards[k]), np.uint8)
        self.encode_host(buf, S)
        for k in range(self.DataShards, self.Shards):
            shards[k][:] = buf[0, k, :S].tobytes()

    def _reconstruct(self, shards: list, data_only: bool) -> None:
        if len(shards) != self.Shards:
            raise ErrTooFewShards(strerror(ErrTooFewShards.code))
        lens = [0 if s is None else len(s) for s in shards]
        S = check_shards(lens, nil_ok=True)
        mask = np.zeros(self.mask_words, np.uint64)
        buf = self._stage(S)
        for r, s in enumerate(shards):
            if lens[r]:
                mask[r >> 6] |= np.uint64(1 << (r & 63))
                buf[0, r, :S] = np.frombuffer(bytes(s), np.uint8)
        status = np.zeros(1, np.int8)
        rc = self.reconstruct_host(buf, mask, S, data_only, status)
        _raise(rc)
        limit = self.DataShards if data_only else self.Shards
        for r in range(limit):
            if not lens[r]:
                shards[r] = bytearray(buf[0, r, :S].tobytes())

    def Reconstruct(self, shards: list) -> None:
        """reedsolomon Reconstruct (ugo/fec.go:202): fills every missing shard."""
        self._reconstruct(shards, data_only=False)

    def ReconstructData(self, shards: list) -> None:
        self._reconstruct(shards, data_only=True)


def rc4_keystream(key: bytes, n: int) -> bytes:
    """RC4 keystream prefix (ugo/crypto.go's fixed-key per-packet cipher)."""
    out = (ctypes.c_uint8 * n)()
    k = (ctypes.c_uint8 * len(key)).from_buffer_copy(key)
    _raise(load_library().ugo_fec_rc4_keystream(ctypes.addressof(k), len(key), ctypes.addressof(out), n))
    return bytes(out)


def New(data_shards: int, parity_shards: int, device: int = 0) -> Encoder:
    """reedsolomon.New as called at ugo/fec.go:59."""
    return Encoder(data_shards, parity_shards, device)


def host_alloc(nbytes: int) -> np.ndarray:
    """Pinned host buffer (uint8 numpy view); free with host_free(arr)."""
    lib = load_library()
    p = ctypes.c_void_p()
    _raise(lib.ugo_fec_host_alloc(nbytes, ctypes.byref(p)))
    arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
    return arr


def host_free(arr: np.ndarray) -> None:
    _raise(load_library().ugo_fec_host_free(ctypes.c_void_p(arr.ctypes.data)))
