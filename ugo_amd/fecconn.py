"""include/ugo_fec_conn.h: ugo's per-connection FEC object."""
from __future__ import annotations

import ctypes
from typing import List

from .abi import _CLOCK_T, _Handle, _raise, load_library

UGO_FEC_MAX_PACKET = 1476


def _bind_conn(lib):
    return lib  # load_library gives this header's entry points their argument types with the rest


class FecConn(_Handle):
    """ugo's per-connection FEC object (ugo/fec.go:14-27) as implemented by the
    C++ host mirror (ugo_amd/csrc/host/fec.cpp) behind include/ugo_fec_conn.h."""

    _destroy = "ugo_fecconn_free"

    def __init__(self, rxlimit: int, data_shards: int, parity_shards: int, device: int = 0):
        lib = _bind_conn(load_library())
        h = ctypes.c_void_p()
        _raise(lib.ugo_fecconn_new(rxlimit, data_shards, parity_shards, device, ctypes.byref(h)))
        self._h, self._lib = h, lib
        self.dataShards, self.parityShards = data_shards, parity_shards
        self._clock_cb = None
        self._out = (ctypes.c_uint8 * (data_shards * UGO_FEC_MAX_PACKET))()

    def set_clock(self, fn):
        """fn() -> uint32 milliseconds (replaces currentMs, ugo/fec.go:73)."""
        self._clock_cb = _CLOCK_T(lambda _u: fn() & 0xFFFFFFFF)
        _raise(self._lib.ugo_fecconn_set_clock(self._h, self._clock_cb, None))

    def markData(self, buf: bytearray):
        c = (ctypes.c_uint8 * len(buf)).from_buffer(buf)
        _raise(self._lib.ugo_fecconn_mark_data(self._h, ctypes.addressof(c)))

    def markFEC(self, buf: bytearray):
        c = (ctypes.c_uint8 * len(buf)).from_buffer(buf)
        _raise(self._lib.ugo_fecconn_mark_fec(self._h, ctypes.addressof(c)))

    @property
    def next(self) -> int:
        v = ctypes.c_uint32()
        _raise(self._lib.ugo_fecconn_get_next(self._h, ctypes.byref(v)))
        return v.value

    @next.setter
    def next(self, v: int):
        _raise(self._lib.ugo_fecconn_set_next(self._h, v))

    def _recovered(self, nrec, rlen):
        if not nrec.value:
            return None
        raw = bytes(self._out)
        return [bytearray(raw[i * UGO_FEC_MAX_PACKET: i * UGO_FEC_MAX_PACKET + rlen.value])
                for i in range(nrec.value)]

    def input(self, wire: bytes):
        """decode + input (ugo/conn.go:394-396): returns (seqid, flag, recovered list | None)."""
        seq, flag = ctypes.c_uint32(), ctypes.c_uint16()
        nrec, rlen = ctypes.c_int(), ctypes.c_size_t()
        w = (ctypes.c_uint8 * len(wire)).from_buffer_copy(wire)
        _raise(self._lib.ugo_fecconn_input(self._h, ctypes.addressof(w), len(wire), ctypes.byref(seq),
                                           ctypes.byref(flag), ctypes.addressof(self._out), len(self._out),
                                           ctypes.byref(nrec), ctypes.byref(rlen)))
        return seq.value, flag.value, self._recovered(nrec, rlen)

    def set_batch(self, groups: int, overlap: bool = False):
        """Batched recovery (include/ugo_fec_conn.h): recoverable lossy groups are
        recovered `groups` at a time in one launch; 0 = per call.  overlap: the
        launch runs while input goes on, its shards come back one batch later
        (UGO_FECCONN_BATCH_OVERLAP).  Returns the recovered shards of groups that
        were pending (list | None)."""
        nrec, rlen = ctypes.c_int(), ctypes.c_size_t()
        need = max(groups, 1) * (2 if overlap else 1) * self.dataShards * UGO_FEC_MAX_PACKET
        new_out = (ctypes.c_uint8 * max(need, len(self._out)))()
        old_out, self._out = self._out, new_out
        try:
            _raise(self._lib.ugo_fecconn_set_batch_ex(self._h, groups, 1 if overlap else 0,
                                                      ctypes.addressof(self._out), len(self._out),
                                                      ctypes.byref(nrec), ctypes.byref(rlen)))
        except Exception:
            self._out = old_out
            raise
        rec = self._recovered(nrec, rlen)
        self._out = (ctypes.c_uint8 * need)()
        return rec

    def flush(self):
        """Recover every pending group now (list | None)."""
        nrec, rlen = ctypes.c_int(), ctypes.c_size_t()
        _raise(self._lib.ugo_fecconn_flush(self._h, ctypes.addressof(self._out), len(self._out),
                                           ctypes.byref(nrec), ctypes.byref(rlen)))
        return self._recovered(nrec, rlen)

    def service(self, idle_us: int = 0):
        """Per-call latency service on this object's encoder (ugo_fecconn_service);
        idle_us < 0 stops it."""
        _raise(self._lib.ugo_fecconn_service(self._h, idle_us))

    def pending(self) -> int:
        v = ctypes.c_size_t()
        _raise(self._lib.ugo_fecconn_pending(self._h, ctypes.byref(v)))
        return v.value

    def calcECC(self, data: List[bytearray], offset: int, maxlen: int):
        n = len(data)
        arrs = [(ctypes.c_uint8 * len(b)).from_buffer(b) for b in data]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(a) for a in arrs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in data])
        _raise(self._lib.ugo_fecconn_calc_ecc(self._h, ptrs, lens, n, offset, maxlen))
        return data[self.dataShards:]

    def rx_len(self) -> int:
        v = ctypes.c_size_t()
        _raise(self._lib.ugo_fecconn_rx_len(self._h, ctypes.byref(v)))
        return v.value
