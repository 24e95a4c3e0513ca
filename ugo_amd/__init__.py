"""ugo_amd: MI355X-native Reed-Solomon FEC for jflyup/ugo's ugo/fec.go hot path.

The package holds only what that path needs:
  csrc/        gfx950 HIP kernels + the C-ABI, one ugo_*.cpp per public header
               (built into libugofec.so)
  fec.py       host mirror of the reedsolomon.Encoder subset ugo uses: the import
               surface of the ctypes binding
  abi.py       the binding's base: the library and its prototypes, the errors, the
               handle owner, the member-set base and the operand checks
  encoder.py, stream.py, ack.py, sent.py, cc.py, listen.py, loop.py, fecconn.py
               the binding, one module per public header of include/
  shard.py     multi-GPU partitioning of independent packet groups
"""
from .fec import (  # noqa: F401
    Encoder,
    ErrInvShardNum,
    ErrMaxShardNum,
    ErrShardNoData,
    ErrShardSize,
    ErrTooFewShards,
    FecError,
    New,
    check_shards,
    load_library,
)

__all__ = ["Encoder", "New", "check_shards", "load_library", "FecError", "ErrInvShardNum", "ErrMaxShardNum",
           "ErrTooFewShards", "ErrShardNoData", "ErrShardSize"]
