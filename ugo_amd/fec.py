"""Python host mirror of the reedsolomon.Encoder subset used by jflyup/ugo.

ugo/fec.go drives klauspost/reedsolomon through three calls:
  reedsolomon.New(dataShards, parityShards)   ugo/fec.go:59
  enc.Reconstruct(shards)                     ugo/fec.go:202
  enc.Encode(shards)                          ugo/fec.go:238
This module exposes the same names and argument meaning over the C-ABI in
include/ugo_fec.h (libugofec.so, gfx950 kernels):

* ``New(d, p, device=0)`` -> ``Encoder`` (raises ``ErrInvShardNum`` /
  ``ErrMaxShardNum`` like upstream ``New``).
* ``Encoder.Encode(shards)`` / ``Encoder.Reconstruct(shards)`` /
  ``Encoder.ReconstructData(shards)``: Go-shaped, one group per call, shards
  are a list of ``bytearray`` (``None`` or empty = missing), same error
  behaviour (``ErrTooFewShards``, ``ErrShardNoData``, ``ErrShardSize``).
* ``Encoder.encode_batch`` / ``reconstruct_batch``: the device-resident batch
  form (torch uint8 tensors on the GPU, shape [groups, d+p, pitch]).
* ``Encoder.encode_host`` / ``reconstruct_host``: host numpy batches, staged
  through the engine's pipelined H2D -> kernel -> D2H path.

There is no CPU fallback: if libugofec.so is missing the import fails, and
every compute call needs a gfx950 device.

The binding itself lives in one module per public header over ugo_amd/abi.py,
as ugo_amd/csrc does; this module is their import surface, and one namespace:
a name set here (load_library replaced, the cache _lib reset) is set in every
module of the binding that holds it.
"""
from __future__ import annotations

import sys as _sys
import types as _types

from . import abi as _abi
from .abi import *  # noqa: F401,F403
from .abi import _CLOCK_T, _ERRORS, _HERE, _DeviceBytes, _raise, _require, _stream_handle  # noqa: F401
from .encoder import *  # noqa: F401,F403  include/ugo_fec.h, ugo_pkt.h
from .stream import *  # noqa: F401,F403  include/ugo_stream.h
from .ack import *  # noqa: F401,F403  include/ugo_ack.h
from .sent import *  # noqa: F401,F403  include/ugo_sent.h
from .cc import *  # noqa: F401,F403  include/ugo_cc.h
from .listen import *  # noqa: F401,F403  include/ugo_listen.h
from .loop import *  # noqa: F401,F403  include/ugo_loop.h
from .fecconn import *  # noqa: F401,F403  include/ugo_fec_conn.h
from .fecconn import _bind_conn  # noqa: F401

_MODULES = [_sys.modules[f"{__package__}.{m}"] for m in
            ("abi", "encoder", "stream", "ack", "sent", "cc", "listen", "loop", "fecconn")]


class _Surface(_types.ModuleType):
    _lib = property(lambda self: _abi._lib)

    def __setattr__(self, name, value):
        for m in _MODULES:
            if name in vars(m):
                setattr(m, name, value)
        if name != "_lib":
            super().__setattr__(name, value)


_sys.modules[__name__].__class__ = _Surface
