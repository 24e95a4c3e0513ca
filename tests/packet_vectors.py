"""Directed wire vectors and the whole-output image for ugo_fec_packet_decode;
test infrastructure only.

The random corpus of tests/test_packet_codec.py goes through the restated
encoder, which refuses most of what a decoder has to survive.  The builders
here compose raw bytes instead: uvarint edges in every position a uvarint
occupies, fields moved across the 16-byte chunks the kernel reads by, SACK
arithmetic at the ends of uint64 (each traced by hand from ugo/packet.go),
segment and cap edges, every 16-bit ufloat16, every short string over a small
alphabet, and every prefix of every directed vector.  Each builder returns a
list of (name, bytes) and needs no GPU.

DecodeImage carves the three outputs of the call out of ONE flat buffer,

    | guard | info [n][64] | guard | ranges [n][R][2] u64 | guard | segs [n][S][16] | guard |

filled with 0xA5, and builds the expected image of all of it from
oracle/packet_ref.py under the output rules of include/ugo_pkt.h:

  status OK / CAPACITY  the whole 64-byte record (reserved zero), the first
                        n_ranges / n_segments entries (counts clamped to the
                        caps); every entry past them keeps the caller's bytes
  status 1..5           status, payload_off, fec_flag_lo and reserved; the
                        record's other fields and the packet's own ranges /
                        segs rows are unspecified (masked out)
  always                every other packet's rows and every guard
"""
import functools
import itertools

import numpy as np

import packet_ref as pr
import rc4_ref
from ugo_amd.fec import PKT_INFO_DTYPE, PKT_SEGMENT_DTYPE

SENTINEL = 0xA5
GUARD = 256
KEY = b"1234567890123456"  # ugo/listener.go:92, ugo/dial.go:132
M64 = (1 << 64) - 1
PKT_CAPACITY = 6

POSITIONS = ("packet_number", "stop_waiting", "largest_acked", "first_block", "later_block", "segment_offset")


# ------------------------------------------------------------------ uvarints
def uv(v):
    return pr.put_uvarint(v)


def uv_n(v, n):
    """v as a uvarint of exactly n bytes (non-canonical when n is more than it
    needs): binary.ReadUvarint accepts trailing zero groups, `81 80 00` is 1."""
    assert len(uv(v)) <= n <= 10 and (n < 10 or v >> 63 <= 1)
    out = bytearray()
    for _ in range(n - 1):
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    assert v < 0x80
    return bytes(out)


BIG = bytes([0xFF] * 9 + [0x01])  # 2^64 - 1, the ten-byte form
VALUES = (0, 127, 128, (1 << 14) - 1, 1 << 14, (1 << 56) - 1, (1 << 63) - 1, 1 << 63, M64)

# name -> bytes of one uvarint.  What ReadUvarint makes of it (Go stdlib,
# encoding/binary varint.go, ReadUvarint): bytes below 0x80 end the number; in
# the tenth byte (i == MaxVarintLen64 - 1) anything above 1 overflows; ten
# continuation bytes overflow without an eleventh being read.
ENCODINGS = dict(
    [("v%d" % k, uv(v)) for k, v in enumerate(VALUES)] + [
        ("ten-80x9-01", b"\x80" * 9 + b"\x01"),       # legal: 2^63
        ("ten-ffx9-01", BIG),                          # legal: 2^64 - 1
        ("ten-ffx9-00", b"\xff" * 9 + b"\x00"),        # legal, non-canonical: 2^63 - 1
        ("ten-80x9-02", b"\x80" * 9 + b"\x02"),        # status 3
        ("ten-ffx9-02", b"\xff" * 9 + b"\x02"),        # status 3
        ("ten-80x9-7f", b"\x80" * 9 + b"\x7f"),        # status 3
        ("ten-cont", b"\x80" * 10),                    # status 3 (the loop runs out)
        ("ten-cont-ff", b"\xff" * 10),                 # status 3
        ("eleven-ff", b"\xff" * 11),                   # status 3 after ten bytes
        ("eleven-80x10-00", b"\x80" * 10 + b"\x00"),   # status 3 after ten bytes
        ("nc-81-80-00", b"\x81\x80\x00"),              # 1
        ("nc-80-00", b"\x80\x00"),                     # 0
        ("nc-ff-80-80-00", b"\xff\x80\x80\x00"),       # 127
    ])

SEG = b"\x05\x00\x02\xaa\xbb"  # a segment: offset 5, length 2


def in_position(pos, enc):
    """A packet that holds the uvarint bytes `enc` at position `pos`, and is
    otherwise built to decode; what the value does to the SACK is the
    oracle's business."""
    if pos == "packet_number":
        return b"\x20" + enc + SEG
    if pos == "stop_waiting":
        return b"\x60\x01" + enc + SEG
    if pos == "largest_acked":  # ack | psh, no missing ranges, first block 1
        return b"\xa0\x00" + enc + b"\x05\x00" + b"\x01" + b"\x07" + SEG
    if pos == "first_block":  # largest 2^64 - 1, so every first block length fits
        return b"\xa0\x00" + BIG + b"\x05\x00" + enc + b"\x07" + SEG
    if pos == "later_block":  # ranges (M, M), then gap 1 and a block of `enc`
        return b"\xa0\x20" + BIG + b"\x05\x00" + b"\x01" + b"\x01" + b"\x01" + enc + b"\x07" + SEG
    if pos == "segment_offset":
        return b"\x20\x01" + enc + b"\x00\x02\xaa\xbb"
    raise ValueError(pos)


def uvarint_vectors():
    return [("uv/%s/%s" % (pos, name), in_position(pos, enc)) for pos in POSITIONS for name, enc in ENCODINGS.items()]


# ----------------------------------------------------------------- alignment
def _spread(extra, widths):
    """Split `extra` padding bytes over fields whose canonical widths are
    `widths` (each can grow to 10 bytes)."""
    out = []
    for w in widths:
        take = min(extra, 10 - w)
        out.append(w + take)
        extra -= take
    assert extra == 0, "more padding than the earlier fields hold"
    return out


def alignment_vectors():
    """Each field kind at a run of consecutive payload offsets, by padding the
    uvarints in front of it; the field itself is two or nine bytes long, so
    it straddles a chunk boundary when it starts late in a chunk.  A packet
    starts at byte 0 of its slot, or at byte 6 behind a typeData FEC header,
    which moves every field by 6: the coverage test counts both.  largest_acked
    has no uvarint in front of it (flags, SACK type), so it can only start at
    byte 2 or 8; first_block needs both modes to reach all sixteen."""
    v9 = (1 << 62) + 0x1234567  # nine bytes
    assert len(uv(v9)) == 9
    out = []
    for e in range(19):  # flags type largest delay first | pn: offset 6 + e
        L, F = _spread(e, [1, 1])
        out.append(("al/packet_number/%d" % (6 + e),
                    b"\xa0\x00" + uv_n(100, L) + b"\x05\x00" + uv_n(3, F) + uv(v9) + SEG))
    for e in range(19):  # ... pn | stop: offset 7 + e (27 spare bytes, 18 used)
        L, F, P = _spread(e, [1, 1, 1])
        out.append(("al/stop_waiting/%d" % (7 + e),
                    b"\xe0\x00" + uv_n(100, L) + b"\x05\x00" + uv_n(3, F) + uv_n(9, P) + uv(v9) + SEG))
    # largest at byte 2, nothing to pad: without and with missing ranges
    out.append(("al/largest_acked/2/00", b"\xa0\x00" + uv(v9) + b"\x05\x00" + b"\x02" + b"\x07" + SEG))
    out.append(("al/largest_acked/2/20",
                b"\xa0\x20" + uv(v9) + b"\x05\x00\x01" + b"\x02" + b"\x01\x01" + b"\x07" + SEG))
    for e in range(9):  # flags type largest(2..10) delay [nblocks] | first: offset 6 + e, 7 + e
        (L,) = _spread(e, [2])
        out.append(("al/first_block/%d" % (6 + e),
                    b"\xa0\x00" + uv_n(0x3FFF, L) + b"\x05\x00" + uv(0x1234) + b"\x07" + SEG))
        out.append(("al/first_block/%d-missing" % (7 + e),
                    b"\xa0\x20" + uv_n(0x3FFF, L) + b"\x05\x00\x01" + uv(0x1234) + b"\x01\x01" + b"\x07" + SEG))
    for e in range(17):  # flags type largest delay nblocks first gap | later: offset 10 + e
        L, F = _spread(e, [3, 1])
        head = b"\xa0\x20" + uv_n(0x4321, L) + b"\x05\x00\x01" + uv_n(1, F) + b"\x01"
        out.append(("al/later_block/%d" % (10 + e), head + uv(0x4123) + b"\x07" + SEG))
    for e in range(19):  # flags pn seg0 | offset of segment 1, then its BE16 nine bytes on
        P, O = _spread(e, [1, 1])
        out.append(("al/segment_offset/%d" % (6 + e),
                    b"\x20" + uv_n(7, P) + uv_n(5, O) + b"\x00\x01\xcc" + uv(v9) + b"\x00\x03\xaa\xbb\xcc"))
    for e in range(19):  # flags pn offset | BE16 at 3 + e: its first byte ends a chunk at 15, and at 9 when framed
        P, O = _spread(e, [1, 1])
        out.append(("al/segment_length/%d" % (3 + e), b"\x20" + uv_n(7, P) + uv_n(5, O) + b"\x01\x02" + bytes(258)))
    return out


# --------------------------------------------------------------------- SACKs
def _blocks(n, gap=1, length=1):
    return bytes([gap, length]) * n


def ranges_packet(nranges, largest=10000):
    """A pure ACK with exactly nranges >= 2 ranges of one packet each, a gap
    of one between them: nranges - 1 blocks of (gap 1, length 1)."""
    assert 2 <= nranges <= 256
    return b"\x80\x20" + uv(largest) + b"\x00\x00" + bytes([nranges - 1]) + b"\x01" + _blocks(nranges - 1)


def sack_vectors(range_caps=(2, 32, 256)):
    """Pure ACKs (flags 0x80: no packet number follows) unless said otherwise.
    Line numbers are ugo/packet.go's.  parseSack: the first range is
    [largest - len + 1, largest] (:272-276); a block after a complete range
    opens [last - len + 1, last] with last = previous.first - gap - 1
    (:292-299); a block after a length-0 block moves the open range down,
    first -= gap + len, last -= gap (:285-290); a range is complete once a
    block of length > 0 reached it (:301-306), an incomplete last one is
    dropped (:309-311).  validateAckRanges (:439-474): not exactly one range,
    range 0 ends at largest, first <= last in each, and each range lies
    below its predecessor with a gap: prev.first > first and prev.first >
    last + 1.  All of it in uint64."""
    v = []
    # [1,5]; gap 3 len 2: last = 1-3-1 = 2^64-3, first = 2^64-4.  first <= last
    # holds, but prev.first = 1 <= 2^64-4: invalid.
    v.append(("sack/wrap-below-zero", b"\x80\x20\x05\x00\x00\x01\x05\x03\x02"))
    # largest M = 2^64-1, len 1: [M,M]; gap 1 len 1: last = M-1-1 = M-2, first = M-2.
    # M > M-2 and M > (M-2)+1: valid, largest_in_order = M-2 = 2^64-3.
    v.append(("sack/top-gap1", b"\x80\x20" + BIG + b"\x00\x00\x01\x01\x01\x01"))
    # gap 0: last = M-0-1 = M-1; prev.first = M <= last+1 = M: adjacent, invalid.
    v.append(("sack/top-gap0", b"\x80\x20" + BIG + b"\x00\x00\x01\x01\x00\x01"))
    # largest 10 len 1: [10,10].  (gap 4, len 0) opens last = 10-4-1 = 5, first = 5-0+1 = 6,
    # incomplete.  (gap 5, len 1) moves it: first = 6-(5+1) = 0, last = 5-5 = 0: [0,0],
    # complete.  (gap 0, len 1): last = 0-0-1 = M, first = M.  prev.first = 0 <= M: invalid.
    v.append(("sack/long-chain-to-zero-wraps", b"\x80\x20\x0a\x00\x00\x03\x01\x04\x00\x05\x01\x00\x01"))
    # the same chain without the last block stops at [10,10], [0,0]: valid, in order 0
    v.append(("sack/long-chain-to-zero", b"\x80\x20\x0a\x00\x00\x02\x01\x04\x00\x05\x01"))
    # largest 20 len 2: [19,20]; (1,2): last = 19-1-1 = 17, first = 16; (3,0) opens
    # [13,12], never completed: dropped.  Two ranges remain: valid, in order 16.
    v.append(("sack/incomplete-last-of-three", b"\x80\x20\x14\x00\x00\x02\x02\x01\x02\x03\x00"))
    # largest 20 len 2: [19,20]; (3,0) opens [16,15], dropped: one range, invalid.
    v.append(("sack/nblocks1-len0", b"\x80\x20\x14\x00\x00\x01\x02\x03\x00"))
    v.append(("sack/nblocks0-missing", b"\x80\x20\x05\x00\x00\x00\x01"))      # :262-264
    v.append(("sack/first-len0", b"\x80\x00\x05\x00\x00\x00"))                # :268-270, status 5
    v.append(("sack/first-len0-missing", b"\x80\x20\x05\x00\x00\x01\x00\x01\x01"))
    v.append(("sack/first-above-largest", b"\x80\x00\x05\x00\x00\x06"))       # :271, status 4
    v.append(("sack/first-equals-largest", b"\x80\x00\x05\x00\x00\x05"))      # in order 1
    v.append(("sack/largest0", b"\x80\x00\x00\x00\x00\x01"))                  # 1 > 0: status 4
    # only bit 0x20 of the type byte matters (:241)
    for t in (0x00, 0xDF):
        v.append(("sack/type-%02x" % t, bytes([0xA0, t]) + b"\x09\x34\x12\x02\x07" + SEG))
    for t in (0x20, 0xFF):
        v.append(("sack/type-%02x" % t, bytes([0xA0, t]) + b"\x09\x34\x12\x01\x02\x01\x01\x07" + SEG))
    # with fin / rst, stop-waiting and segments behind the SACK
    v.append(("sack/then-everything",
              b"\xf8\x20\x64\xff\xff\x02\x03\x02\x01\xfe\x00\x01\x02" + b"\x2a" + b"\x29" + SEG + SEG))
    # 255 blocks under largest 10000: 256 ranges, 518 bytes
    v.append(("sack/256-ranges", ranges_packet(256)))
    for cap in range_caps:
        for k in (cap, cap + 1):
            if 2 <= k < 256:  # 256 stands above; one range is invalid, 257 do not fit the block count byte
                v.append(("sack/%d-ranges" % k, ranges_packet(k, largest=70000 + k)))
    # a long-gap chain of 254 length-0 blocks, then one block: two ranges
    v.append(("sack/254-long-blocks",
              b"\x80\x20" + uv(1 << 40) + b"\x00\x00\xff\x01" + _blocks(254, 0xFF, 0) + b"\x07\x03"))
    return v


# ------------------------------------------------------------------ segments
def segments_packet(nseg, pn=b"\x01", seg=b"\x00\x00\x00"):
    return b"\x20" + pn + seg * nseg


MANY_SEGMENTS = 21839  # 2 + 3 * 21839 = 65,519 bytes, the most a slot of 0xfff0 holds


def segment_vectors(segment_caps=(1, 2, 8), top=528):
    v = [("seg/len0", b"\x20\x01\x05\x00\x00"),
         ("seg/len0-twice", b"\x20\x01\x05\x00\x00\x06\x00\x00"),
         ("seg/len0-then-data", b"\x20\x01\x05\x00\x00\x06\x00\x01\xee"),
         ("seg/ffff-1-byte", b"\x20\x01\x00\xff\xff\xaa"),     # avail 1 (packet.go:92-96, a short Read is accepted)
         ("seg/ffff-0-bytes", b"\x20\x01\x00\xff\xff"),        # Read at the end: io.EOF
         ("seg/half-be16", b"\x20\x01\x00\xff"),               # io.ReadFull of 2 with 1 left: ErrUnexpectedEOF
         ("seg/no-be16", b"\x20\x01\x00"),                     # with 0 left: io.EOF
         ("seg/short-last", b"\x20\x01\x05\x00\x02\xaa\xbb\x06\x00\x09\x01\x02\x03"),
         ("seg/none", b"\x20\x01"),
         ("seg/flags-only", b"\x00"),
         ("seg/pure-ack-then-bytes", b"\x80\x00\x09\x00\x00\x01\x05\x00\x01\x77")]
    for k in sorted({c + more for c in segment_caps for more in (0, 1)}):
        v.append(("seg/%d-segments" % k, segments_packet(k, seg=b"\x03\x00\x01\x5a")))
    # as long as the directed corpus's slot: lens[i] == slot
    v.append(("seg/fills-slot",
              b"\x20\x01\x00" + (top - 5).to_bytes(2, "big") + bytes(range(256)) * 2 + bytes(top - 5 - 512)))
    return v


def oversized_vectors():
    """The two packets the other builders leave out: they want a slot of
    0xfff0 and a batch of their own."""
    many = segments_packet(MANY_SEGMENTS)
    assert len(many) == 65519
    big = b"\x20" + uv_n(1, 6) + b"\x00" + (39990).to_bytes(2, "big") + bytes(39990)
    assert len(big) == 40000
    return [("big/21839-segments", many), ("big/40000-bytes", big)]


# ---------------------------------------------------------------- exhaustive
def ufloat16_vectors():
    """One pure ACK per 16-bit delay: 80 00 01 lo hi 01."""
    return [("uf16/%04x" % w, bytes([0x80, 0x00, 0x01, w & 0xFF, w >> 8, 0x01])) for w in range(1 << 16)]


ALPHABET = (0x00, 0x01, 0x02, 0x20, 0x40, 0x7F, 0x80, 0xA0, 0xFF)


def small_alphabet_vectors(maxlen=5):
    return [("alpha/%s" % bytes(t).hex(), bytes(t))
            for n in range(maxlen + 1) for t in itertools.product(ALPHABET, repeat=n)]


# -------------------------------------------------------------------- corpus
@functools.lru_cache(maxsize=None)
def directed():
    """Every directed vector but the oversized ones."""
    v = uvarint_vectors() + alignment_vectors() + sack_vectors() + segment_vectors()
    assert len(set(n for n, _ in v)) == len(v)
    return tuple(v)


@functools.lru_cache(maxsize=None)
def with_prefixes():
    """(name, full, cut) for every directed vector and every truncation of it,
    each distinct byte string once.  The packet is full[:cut]; `full` is what a
    ring slot still holds when an older, longer packet sat in it."""
    seen, out = set(), []
    for name, b in directed():
        for cut in range(len(b), -1, -1):
            if b[:cut] not in seen:
                seen.add(b[:cut])
                out.append((name if cut == len(b) else "%s[:%d]" % (name, cut), b, cut))
    return tuple(out)


FEC_FLAGS = (0xF1, 0xF1, 0xF2, 0x1234)


def frame(packets, start=0):
    """A 6-byte FEC header in front of each packet, the flag rotating through
    typeData, typeData, typeFEC and junk: only the first two are stripped
    (ugo/conn.go:395-405)."""
    return [int(i).to_bytes(4, "little") + FEC_FLAGS[(start + i) % 4].to_bytes(2, "little") + b
            for i, b in enumerate(packets)]


def frame_both(packets):
    """Each packet twice, under the rotation and under the rotation two on: the
    flags two apart are typeData and not, so every packet is decoded once
    behind a stripped header and once from byte 0 with its header in front."""
    assert all((FEC_FLAGS[k] == 0xF1) != (FEC_FLAGS[(k + 2) % 4] == 0xF1) for k in range(4))
    return frame(packets) + frame(packets, start=2)


# --------------------------------------------------------------------- trace
class _TraceReader(pr.Reader):
    def __init__(self, b):
        super().__init__(b)
        self.events = []

    def read_uvarint(self):
        start = self.i
        try:
            v = super().read_uvarint()
        except pr.DecodeError as e:
            self.events.append((start, self.i, None, e.code))
            raise
        self.events.append((start, self.i, v, 0))
        return v


def field_trace(raw):
    """The uvarints oracle/packet_ref.decode reads from `raw`, in order:
    [(position, start, end, value or None, status)], plus ("segment_length",
    start, start + 2, value, 0) for each BE16 it reads whole.  The reads are
    the oracle's own (its Reader, instrumented); the positions follow from
    the order ugoPacket.decode reads in.

    This leans on two things in oracle/packet_ref.py: decode() builds its one
    reader through the module-level name Reader, and it reads the fields in
    the order of order() below.  Both are asserted here (one reader, and the
    block count byte sits two bytes behind largest_acked only because the
    ufloat16 delay lies between), so a refactor of the oracle that breaks
    either fails loudly instead of mislabelling fields."""
    readers = []

    def make(b):
        readers.append(_TraceReader(b))
        return readers[-1]

    saved, pr.Reader = pr.Reader, make
    try:
        status, _ = pr.decode(raw)
    finally:
        pr.Reader = saved
    assert len(readers) == 1, "packet_ref.decode no longer reads through one Reader"
    ev = readers[0].events

    def order():
        flags = raw[0]
        if flags & 0x80:
            yield "largest_acked"
            yield "first_block"
            if raw[1] & 0x20:
                for _ in range(raw[ev[0][1] + 2]):
                    yield "later_block"
        if flags != 0x80:
            yield "packet_number"
        if flags & 0x40:
            yield "stop_waiting"
        while True:
            yield "segment_offset"

    out = []
    for (start, end, v, st), pos in zip(ev, order()):
        out.append((pos, start, end, v, st))
        if pos == "segment_offset" and st == 0 and end + 2 <= len(raw):
            out.append(("segment_length", end, end + 2, int.from_bytes(raw[end:end + 2], "big"), 0))
    return status, out


# --------------------------------------------------------------------- image
@functools.lru_cache(maxsize=None)
def decode(raw):
    """oracle/packet_ref.decode, remembered: the same payload comes back in
    every run of a corpus."""
    return pr.decode(raw)


@functools.lru_cache(maxsize=None)
def keystream(n):
    return np.frombuffer(rc4_ref.keystream(KEY, n), np.uint8)


def payload_start(b, framed):
    """(payload_off, fec_flag_lo) of Conn.handlePacket's framing (ugo/conn.go:
    390-405, FEC.decode ugo/fec.go:78-89): a packet shorter than the header is
    decoded from byte 0 and reports no flag."""
    if not framed or len(b) < 6:
        return 0, 0
    return (6 if b[4] | (b[5] << 8) == 0xF1 else 0), b[4]


def ring(packets, slot, slack=0, fulls=None, rng=None, encrypt=False):
    """Slots [n, slot] and lens for `packets`.  The bytes of a slot past
    lens[i] (the slack) hold: the rest of fulls[i] where given, then `slack`
    (a byte value, or "random" with rng).  encrypt: XOR every whole slot with
    the keystream, so the slack has those values after decryption."""
    n = len(packets)
    if slack == "random":
        slots = rng.integers(0, 256, (n, slot), dtype=np.uint8)
    else:
        slots = np.full((n, slot), slack, np.uint8)
    lens = np.zeros(n, np.uint16)
    for i, b in enumerate(packets):
        if fulls is not None:
            assert fulls[i][:len(b)] == b
            slots[i, :len(fulls[i])] = np.frombuffer(fulls[i], np.uint8)
        slots[i, :len(b)] = np.frombuffer(b, np.uint8)
        lens[i] = len(b)
    if encrypt:
        slots ^= keystream(slot)[None, :]
    return slots, lens


RANGE_DTYPE = np.dtype([("first", "<u8"), ("last", "<u8")])
_INFO_KEPT_ON_ERROR = ("status", "payload_off", "fec_flag_lo", "reserved")


def _field_at(dtype, col):
    for name in dtype.names:
        sub, off = dtype.fields[name][:2]
        if off <= col < off + sub.itemsize:
            return name
    raise ValueError(col)


class DecodeImage:
    """The flat buffer of one call (module docstring).  `out` is the
    (info, ranges, segs) triple for Encoder.packet_decode(out=...).  A cap of
    zero still gets an array of one entry per packet, which the call must not
    touch.  buffer: a uint8 numpy array to build the views on (pinned host
    memory) instead of a device allocation; device=None builds no buffer --
    expected(), decode() and check() need none."""

    def __init__(self, n, max_ranges, max_segments, device="cuda", buffer=None):
        self.n, self.R, self.S = n, max_ranges, max_segments
        self.Ra, self.Sa = max(max_ranges, 1), max(max_segments, 1)
        self.info_off = GUARD
        self.ranges_off = self.info_off + n * 64 + GUARD
        self.segs_off = self.ranges_off + n * self.Ra * 16 + GUARD
        self.size = self.segs_off + n * self.Sa * 16 + GUARD
        self.flat = self.out = None
        if buffer is not None or device is not None:
            import torch

            if buffer is not None:
                assert buffer.dtype == np.uint8 and buffer.size >= self.size
                buffer[:self.size] = SENTINEL
                self.flat = torch.from_numpy(buffer[:self.size])
            else:
                self.flat = torch.full((self.size,), SENTINEL, dtype=torch.uint8, device=device)
            f = self.flat
            self.out = (f[self.info_off:self.info_off + n * 64].view(n, 64),
                        f[self.ranges_off:self.ranges_off + n * self.Ra * 16].view(torch.int64).view(n, self.Ra, 2),
                        f[self.segs_off:self.segs_off + n * self.Sa * 16].view(n, self.Sa, 16))

    @staticmethod
    def bytes_needed(n, max_ranges, max_segments):
        return 4 * GUARD + n * (64 + max(max_ranges, 1) * 16 + max(max_segments, 1) * 16)

    def refill(self):
        self.flat.fill_(SENTINEL)

    # views of a whole-buffer numpy image
    def info(self, img):
        return img[self.info_off:self.info_off + self.n * 64].view(PKT_INFO_DTYPE)

    def ranges(self, img):
        return img[self.ranges_off:self.ranges_off + self.n * self.Ra * 16].view("<u8").reshape(self.n, self.Ra, 2)

    def segs(self, img):
        return img[self.segs_off:self.segs_off + self.n * self.Sa * 16].view(PKT_SEGMENT_DTYPE).reshape(self.n, self.Sa)

    def expected(self, packets, framed=False):
        """(image, mask) of the whole buffer after decoding `packets` (as they
        sit in their slots, FEC header included when framed): mask is False
        where include/ugo_pkt.h leaves the content open."""
        assert len(packets) == self.n
        img = np.full(self.size, SENTINEL, np.uint8)
        mask = np.ones(self.size, bool)
        info, ranges, segs = self.info(img), self.ranges(img), self.segs(img)
        info[:] = np.zeros((), PKT_INFO_DTYPE)
        open_info = np.ones(64, bool)
        for name in _INFO_KEPT_ON_ERROR:
            sub, off = PKT_INFO_DTYPE.fields[name][:2]
            open_info[off:off + sub.itemsize] = False
        for i, b in enumerate(packets):
            off, flag_lo = payload_start(b, framed)
            st, out = decode(b[off:] if off else b)
            rec = info[i]
            rec["payload_off"], rec["fec_flag_lo"] = off, flag_lo
            if st != pr.PKT_OK:
                rec["status"] = st
                o = self.info_off + i * 64
                mask[o:o + 64] = ~open_info
                mask[self.ranges_off + i * self.Ra * 16:self.ranges_off + (i + 1) * self.Ra * 16] = False
                mask[self.segs_off + i * self.Sa * 16:self.segs_off + (i + 1) * self.Sa * 16] = False
                continue
            rec["flags"], rec["packet_number"] = out["flags"], out["packet_number"]
            rec["stop_waiting"] = out["stop_waiting"]
            rg = []
            if out["sack"] is not None:
                s = out["sack"]
                rec["largest_acked"], rec["largest_in_order"], rec["delay_us"] = \
                    s["largest_acked"], s["largest_in_order"], s["delay_us"]
                rg = s["ranges"]
            sg = out["segments"]
            if len(rg) > self.R or len(sg) > self.S:
                rec["status"] = PKT_CAPACITY
            nr, ns = min(len(rg), self.R), min(len(sg), self.S)
            rec["n_ranges"], rec["n_segments"] = nr, ns
            if nr:
                ranges[i, :nr] = np.array(rg[:nr], np.uint64)
            if ns:
                segs[i, :ns] = np.array([(o_, d + off, n_, a) for o_, d, n_, a in sg[:ns]], PKT_SEGMENT_DTYPE)
        return img, mask

    def decode(self, off):
        """Where byte `off` of the buffer lies: "guard", or (array, packet,
        entry, field); entry is None in info, and an entry at or past the cap
        is the unused one a zero cap leaves."""
        for name, base, per, dtype in (("info", self.info_off, 1, PKT_INFO_DTYPE),
                                       ("ranges", self.ranges_off, self.Ra, RANGE_DTYPE),
                                       ("segs", self.segs_off, self.Sa, PKT_SEGMENT_DTYPE)):
            rel = off - base
            if 0 <= rel < self.n * per * dtype.itemsize:
                entry, col = divmod(rel % (per * dtype.itemsize), dtype.itemsize)
                return (name, rel // (per * dtype.itemsize), None if name == "info" else entry, _field_at(dtype, col))
        return "guard"

    def got(self):
        return self.flat.cpu().numpy().copy()

    def mismatch(self, got, want, mask):
        """None, or (count, first offset, where) of the bytes that differ
        under the mask."""
        assert got.shape == want.shape == mask.shape == (self.size,)
        diff = np.flatnonzero((got != want) & mask)
        if diff.size == 0:
            return None
        return diff.size, int(diff[0]), self.decode(int(diff[0]))

    def check(self, got, want, mask, what="", packets=None):
        m = self.mismatch(got, want, mask)
        if m is None:
            return
        count, off, where = m
        kind = "guard" if where == "guard" else "(array, packet, entry, field) = %r" % (where,)
        pkt = ""
        if packets is not None and where != "guard":
            pkt = ", packet bytes %s" % packets[where[1]][:48].hex()
        raise AssertionError("%s: %d bytes differ, first at buffer offset %d, %s: got 0x%02x, want 0x%02x%s"
                             % (what, count, off, kind, got[off], want[off], pkt))
