"""Directed corpus for the batch packet encoder (ugo_fec_packet_encode and
ugo_fec_stream_tx_set_encode, k_packet_encode); test infrastructure only.

Packets are descriptions (_pkt): the encoder's input and the oracle's
arguments at once.  The expected bytes are oracle/packet_ref.py's, except
where a case carries bytes derived by hand from ugo/packet.go (family h, the
gaps the reference's writer would loop over) and
for the one rule the oracle does not know: an encoded length above the slot is
UGO_PKT_CAPACITY (include/ugo_pkt.h).

Families (each a Family with a name, so that a failure can say where it came
from):

  a  copy split, short: one segment, every destination residue x source
     residue {0, 1, 7, 8, 15} x every L in 0..48
  b  copy split of a second and third segment: the third segment's data at
     every residue, L round the 16-B and 32-B edges; 64 segments in one packet
  c  copy loop, long: interior chunk counts at the ends of every leg of the
     four-chunk unroll and of the first three trips, head and tail 0 / 1 / 15;
     9000 B in a 9024-B slot; exactly 0xfff0 B and one more
  d  sizes: segment lengths whose sum passes 16 bits, the width of every length field
  e  uvarint length edges in every field
  f  every ufloat16 code's value and the value below it
  g  SACK blocks: every gap 1..1600, many ranges, the reference's failures
  h  packet-number arithmetic that wraps at 2^64, bytes by hand

EncodeImage is the encoder's three outputs as one allocation between guards,
compared in whole with an image built from the expectation alone.
"""
import functools

import numpy as np
import torch

import packet_ref as pr
from ugo_amd import fec

KEY = b"1234567890123456"  # ugo/listener.go:92, ugo/dial.go:132
SENTINEL = 0xA5
GUARD = 64
M64 = (1 << 64) - 1
MAX_SLOT = 0xFFF0
OFF4 = 1 << 21  # a segment offset of four uvarint bytes: families a, b and c use no other length


def _pkt(flags=0, sack=None, pn=1, sw=0, segments=()):
    """sack = (largest, in_order, ranges, delay_us) or None; segments = [(offset, data)]."""
    return {"flags": flags, "sack": sack, "pn": pn, "sw": sw, "segments": list(segments)}


def _ref_encode(p):
    """(status, bytes) of ugoPacket.encode: the oracle behind the reference's
    two consistency checks (packet.go:367-372)."""
    s = p["sack"]
    if s is not None and s[2]:
        if s[2][0][1] != s[0]:
            return fec.PKT_INCONSISTENT_LARGEST_ACKED, b""
        if s[1] != s[2][-1][0]:
            return fec.PKT_INCONSISTENT_LOWEST_ACKED, b""
    try:
        return 0, pr.encode(flags=p["flags"], sack=s, packet_number=p["pn"], stop_waiting=p["sw"],
                            segments=p["segments"])
    except pr.EncodeError:
        return fec.PKT_INCONSISTENT_RANGE_COUNT, b""


def _two_ranges(gap, hi=1 << 20):
    """A SACK of two ranges with `gap` missing packets between them."""
    lo_last = hi - 10 - gap - 1
    ranges = [(hi - 10, hi), (lo_last - 4, lo_last)]
    return (hi, ranges[-1][0], ranges, 7)


def _many_ranges(n, hi=1 << 20):
    ranges = []
    for _ in range(n):  # length 3, gap 3
        ranges.append((hi - 2, hi))
        hi -= 6
    return (ranges[0][1], ranges[-1][0], ranges, 0)


def _round_trips(p, st):
    """Where decode(encode(x)) == x in the reference: encodes, no gap that is
    a multiple of 255 (written lossily, test_packet_codec.py), not a single range."""
    if st != 0:
        return False
    rg = p["sack"][2] if p["sack"] else []
    gaps = [rg[i - 1][0] - rg[i][1] - 1 for i in range(1, len(rg))]
    return len(rg) != 1 and not any(g >= 255 and g % 255 == 0 for g in gaps)


def _in_decoders_domain(p):
    """What parseSack accepts and keeps whole: a first block of 1..largest
    packets, ranges in strictly descending order with first <= last
    (validateAckRanges), and no more blocks than the count byte holds (the
    writer drops the ranges past them)."""
    if p["sack"] is None:
        return True
    largest, in_order, rg, _ = p["sack"]
    first = (largest - (rg[0][0] if rg else in_order) + 1) & M64
    if not 1 <= first <= largest:
        return False
    blocks = 1 if rg else 0
    for k, (f, l) in enumerate(rg):
        if f > l or (k and not rg[k - 1][0] > l + 1):
            return False
        if k:
            gap = rg[k - 1][0] - l - 1
            blocks += gap // 255 + (1 if gap % 255 else 0)
    return blocks <= 255


def round_trips(p, st):
    return _round_trips(p, st) and _in_decoders_domain(p)


def _fill(rng, n, kind):
    if kind == "zeros":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _describe(pkts, rng, max_ranges, max_segments, residues=None, surround=None, per_packet=False):
    """The encoder's input for `pkts`: info / ranges / segs arrays and a payload
    buffer holding every segment's bytes at a random (or the given) residue
    mod 16, with unrelated bytes around them.  residues[i] is one residue for
    packet i's segments or one per segment.  surround: what the unrelated
    bytes are ("zeros", "ff", "random"; default zeros where they align and
    random elsewhere).  per_packet: the payload is [n, stride] with every
    packet's segments in its own row and data_off counted from the row (the
    payload_stride form); else one flat buffer."""
    n = len(pkts)
    info = np.zeros(n, fec.PKT_INFO_DTYPE)
    ranges = np.zeros((n, max_ranges, 2), np.uint64)
    segs = np.zeros((n, max_segments), fec.PKT_SEGMENT_DTYPE)
    lead, gapk = surround or "random", surround or "zeros"
    rows = []
    blob = bytearray(_fill(rng, 16, lead))
    cols = {k: [0] * n for k in ("flags", "packet_number", "stop_waiting", "largest_acked", "largest_in_order",
                                 "delay_us", "n_ranges", "n_segments")}
    for i, p in enumerate(pkts):
        cols["flags"][i] = p["flags"] | (0x80 if p["sack"] is not None else 0)
        cols["packet_number"][i], cols["stop_waiting"][i] = p["pn"], p["sw"]
        if p["sack"] is not None:
            cols["largest_acked"][i], cols["largest_in_order"][i], rg, cols["delay_us"][i] = p["sack"]
            cols["n_ranges"][i] = len(rg)
            if rg:
                ranges[i, :min(len(rg), max_ranges)] = np.array([(f & M64, l & M64) for f, l in rg[:max_ranges]],
                                                                np.uint64)
        cols["n_segments"][i] = len(p["segments"])
        for j, (off, data) in enumerate(p["segments"][:max_segments]):
            if residues is None:
                want = int(rng.integers(0, 16))
            else:
                want = residues[i] if isinstance(residues[i], (int, np.integer)) else residues[i][j]
            blob += _fill(rng, (want - len(blob)) % 16, gapk)
            segs[i, j] = (off, len(blob), len(data), 0xFFFF)  # avail is ignored
            blob += data
            blob += _fill(rng, int(rng.integers(0, 5)), lead)
        if per_packet:
            rows.append(bytes(blob))
            blob = bytearray(_fill(rng, 16, lead))
    for k, v in cols.items():
        info[k] = np.array(v, np.uint64).astype(info.dtype[k])
    info["status"], info["payload_off"], info["fec_flag_lo"] = 0xDEAD, 0xBEEF, 0x5A  # ignored by the encoder
    if per_packet:
        stride = (max(len(r) for r in rows) + 16 + 15) & ~15 if rows else 16
        payload = np.frombuffer(_fill(rng, n * stride, gapk), np.uint8).reshape(n, stride).copy()
        for i, r in enumerate(rows):
            payload[i, :len(r)] = np.frombuffer(r, np.uint8)
        return info, ranges, segs, payload
    blob += _fill(rng, 16, gapk)
    return info, ranges, segs, np.frombuffer(bytes(blob), np.uint8)


def _data(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _round16(v):
    return (v + 15) & ~15


def uvarint_of_len(nbytes):
    """The smallest value whose uvarint takes nbytes bytes."""
    return 1 << (7 * (nbytes - 1)) if nbytes > 1 else 1


class Family:
    """pkts with what one call over them needs.  hand: {index: (status, bytes)}
    where the expectation is not the oracle's; tags[i]: what packet i is there
    for (for messages and for the coverage assertions); residues as for
    _describe."""

    def __init__(self, name, pkts, max_ranges=1, max_segments=1, slot=None, residues=None, hand=None, tags=None):
        self.name, self.pkts = name, pkts
        self.max_ranges, self.max_segments = max_ranges, max_segments
        self.residues, self.hand, self.tags = residues, hand or {}, tags or [None] * len(pkts)
        assert len(self.tags) == len(pkts) and (residues is None or len(residues) == len(pkts))
        self.fixed_slot = slot

    @functools.cached_property
    def oracle(self):
        """[(status, bytes)] of the reference's encode, slots apart."""
        return [self.hand[i] if i in self.hand else _ref_encode(p) for i, p in enumerate(self.pkts)]

    @functools.cached_property
    def slot(self):
        return self.fixed_slot or max(16, _round16(6 + max(len(raw) for _, raw in self.oracle)))

    def expected(self, framed=False):
        """The oracle's result under the header's capacity rule."""
        room = 6 if framed else 0
        return [(fec.PKT_CAPACITY, b"") if st == 0 and room + len(raw) > self.slot else (st, raw)
                for st, raw in self.oracle]

    def pick(self, n):
        """n packets spread evenly over the family, as a family of their own."""
        at = [(2 * i + 1) * len(self.pkts) // (2 * n) for i in range(n)]
        return Family("%s, %d of it" % (self.name, n), [self.pkts[i] for i in at], self.max_ranges,
                      self.max_segments, self.slot, None if self.residues is None else [self.residues[i] for i in at],
                      {k: self.hand[i] for k, i in enumerate(at) if i in self.hand}, [self.tags[i] for i in at])

    def label(self, i):
        return "family %s, packet %d (%s)" % (self.name, i, self.tags[i])


# ------------------------------------------------------------------ families
def _align(s):
    """(packet_number, stop_waiting) whose uvarints take s bytes together, s in
    1..20: with a four-byte offset the first segment's data starts at byte
    7 + s of the packet."""
    assert 1 <= s <= 20
    a = min(10, s)
    return uvarint_of_len(a), (uvarint_of_len(s - a) if s > a else 0)


SRC_RESIDUES = (0, 1, 7, 8, 15)


@functools.lru_cache(None)
def family_a():
    rng = np.random.default_rng(0xA)
    pk, res, tags = [], [], []
    for s in range(1, 17):  # data at byte 8 .. 23: every residue
        pn, sw = _align(s)
        for r in SRC_RESIDUES:
            for L in range(49):
                pk.append(_pkt(pn=pn, sw=sw, segments=[(OFF4 + len(pk), _data(rng, L))]))
                res.append((r,))
                tags.append(((7 + s) % 16, r, L))
    return Family("a", pk, residues=res, tags=tags)


THIRD_L = (0, 1, 15, 16, 17, 31, 32, 33)


@functools.lru_cache(None)
def family_b():
    rng = np.random.default_rng(0xB)
    pk, res, tags = [], [], []
    for rep in range(3):
        for r in range(16):  # the residue the third segment's data starts at
            for k, L3 in enumerate(THIRD_L):
                L1 = (3 * r + 5 * k + 11 * rep) % 40
                head = 1 + 1 + 3 * 6  # flags, packet number, three segment headers
                L2 = (r - head - L1) % 16 + 16 * ((r + k + rep) % 3)
                pk.append(_pkt(pn=3, segments=[(OFF4 + 1000 * len(pk), _data(rng, L1)),
                                               (OFF4 + 1000 * len(pk) + 100, _data(rng, L2)),
                                               (OFF4 + 1000 * len(pk) + 200, _data(rng, L3))]))
                x = 5 * r + 3 * k + 7 * rep
                res.append((x % 16, (x + 5 + rep) % 16, (x + 11 + k) % 16))
                tags.append((r, L3))
    many = [(OFF4 + (1 << 20) + 50 * j, _data(rng, (8 * j) % 21)) for j in range(64)]
    pk.append(_pkt(pn=3, segments=many))
    res.append(tuple((11 * j + 2) % 16 for j in range(64)))
    tags.append("64 segments")
    return Family("b", pk, max_segments=64, residues=res, tags=tags)


CHUNK_COUNTS = (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 385)


def _long(rng, head, nchunks, tail, at=0):
    """One segment whose copy is `head` bytes up to a chunk boundary, nchunks
    whole chunks and `tail` bytes."""
    pn, sw = _align(((16 - head) % 16 - 7) % 16 or 16)  # data at byte 16 - head (mod 16)
    return _pkt(pn=pn, sw=sw, segments=[(OFF4 + at, _data(rng, head + 16 * nchunks + tail))])


@functools.lru_cache(None)
def family_c():
    rng = np.random.default_rng(0xC)
    pk, res, tags = [], [], []
    for nchunks in CHUNK_COUNTS:
        for head in (0, 1, 15):
            for tail in (0, 1, 15):
                pk.append(_long(rng, head, nchunks, tail, at=8192 * len(pk)))
                res.append(((nchunks + 3 * head + tail) % 16,))
                tags.append((nchunks, head, tail))
    return Family("c", pk, residues=res, tags=tags)


@functools.lru_cache(None)
def family_c_9000():
    rng = np.random.default_rng(0xC9)
    pk = [_pkt(pn=1, segments=[(OFF4 + 9000 * i, _data(rng, 9000))]) for i in range(3)]  # BASELINE's configs[4]
    return Family("c-9000", pk, slot=9024, residues=[(0,), (5,), (15,)], tags=["9000 B"] * 3)


@functools.lru_cache(None)
def family_c_fff0():
    """Exactly the largest slot, one byte more (UGO_PKT_CAPACITY), and exactly
    the slot behind 6 bytes of header room, between small packets."""
    rng = np.random.default_rng(0xCF)
    hdr = 1 + 1 + 4 + 2
    small = lambda: _pkt(pn=2, segments=[(OFF4 + 70, _data(rng, 70))])  # noqa: E731
    pk = [small(), _pkt(pn=1, segments=[(OFF4 + 100000, _data(rng, MAX_SLOT - hdr))]), small(),
          _pkt(pn=1, segments=[(OFF4 + 200000, _data(rng, MAX_SLOT - hdr + 1))]), small(),
          _pkt(pn=1, segments=[(OFF4 + 300000, _data(rng, MAX_SLOT - hdr - 6))]), small()]
    return Family("c-fff0", pk, slot=MAX_SLOT, residues=[(3,), (9,), (4,), (1,), (5,), (15,), (6,)],
                  tags=["small", "0xfff0 B", "small", "0xfff1 B", "small", "0xffea B", "small"])


SIZE_SUMS = ((0x8000, 0x8000), (0xFFFF, 0xFFFF, 0xFFFF), (0xFFFF,))


@functools.lru_cache(None)
def family_d():
    """Segment lengths that sum past the slot and past 16 bits -- the width of
    ugo_pkt_segment.len and of wire_lens --, in slots of 0xfff0: by the
    header's rule UGO_PKT_CAPACITY each, between packets that encode.  The
    segments' bytes are all there, so that an encoder which took such a packet
    for a short one would show in the neighbours' slots."""
    rng = np.random.default_rng(0xD)
    good = lambda: _pkt(pn=5, sw=2, segments=[(OFF4 + 90, _data(rng, 90)), (OFF4, _data(rng, 33))])  # noqa: E731
    pk, tags = [good()], ["good"]
    for lens in SIZE_SUMS:
        pk.append(_pkt(pn=6, segments=[(OFF4 + 8 * j, _data(rng, L)) for j, L in enumerate(lens)]))
        tags.append("len " + " + ".join("%#x" % v for v in lens))
        pk.append(good())
        tags.append("good")
    return Family("d", pk, max_segments=3, slot=MAX_SLOT, tags=tags)


UVARINT_EDGES = tuple(v for k in range(1, 10) for v in ((1 << (7 * k)) - 1, 1 << (7 * k))) + (M64,)
UVARINT_POSITIONS = ("packet_number", "stop_waiting", "largest_acked", "first_length", "range_length", "offset")


@functools.lru_cache(None)
def family_e():
    """One field at a uvarint length edge, the others at one byte.  A first
    block or a range of v packets under a one-byte largest_acked is stated with
    the 2^64 wrap of the header."""
    rng = np.random.default_rng(0xE)
    pk, tags = [], []
    for v in UVARINT_EDGES:
        seg = [(9, _data(rng, 20))]
        pk += [_pkt(pn=v, segments=seg),
               _pkt(pn=1, sw=v, segments=seg),
               _pkt(pn=1, sack=(v, v, [], 3), segments=seg),
               _pkt(pn=1, sack=(5, (5 + 1 - v) & M64, [], 3), segments=seg),
               _pkt(pn=1, sack=(110, (90 - v + 1) & M64, [(100, 110), ((90 - v + 1) & M64, 90)], 3), segments=seg),
               _pkt(pn=1, segments=[(v, _data(rng, 20))])]
        tags += [(pos, v) for pos in UVARINT_POSITIONS]
    return Family("e", pk, max_ranges=2, tags=tags)


UFLOAT16_EXTRA = (0x3FFC0000000 - 1, 0x3FFC0000000, 1 << 42, 1 << 63, M64)


def ufloat16_value(code):
    return pr.Reader(bytes([code & 0xFF, code >> 8])).read_ufloat16()


@functools.lru_cache(None)
def family_f():
    delays = []
    for c in range(1 << 16):
        v = ufloat16_value(c)
        delays += [v, v - 1] if v else [v]
    delays += UFLOAT16_EXTRA
    pk = [_pkt(sack=(128 + i % 16000, 128 + i % 16000, [], d), pn=9) for i, d in enumerate(delays)]  # pure ACKs
    return Family("f", pk, slot=16, tags=delays)


def _g_cases():
    """(packet, (status, bytes) by hand or None, tag)"""
    out = [(_pkt(sack=_two_ranges(g), pn=1), None, "gap %d" % g) for g in range(1, 1601)]
    out += [(_pkt(sack=_many_ranges(n), pn=1), None, "%d ranges" % n) for n in (2, 254, 255, 256, 300)]
    s7 = _two_ranges(20)
    s7 = (s7[0] + 1, s7[1], s7[2], s7[3])  # largest_acked != ranges[0].last
    s8 = _two_ranges(20)
    s8 = (s8[0], s8[1] - 1, s8[2], s8[3])  # largest_in_order != ranges[-1].first
    out += [(_pkt(sack=_two_ranges(g), pn=1), None, "gap %d" % g) for g in (511, 767, 510, 768)]
    # gap 2^40, by hand (test_packet_encode_status_paths): numWritableNackRanges returns 1, the writer emits
    # 2^40 / 255 + 1 blocks -> "inconsistent number of ACK ranges written"
    out.append((_pkt(sack=_two_ranges(1 << 40, hi=1 << 41), pn=1), (9, b""), "gap 2^40"))
    out += [(_pkt(sack=s7, pn=1), None, "largest_acked off"), (_pkt(sack=s8, pn=1), None, "largest_in_order off")]
    # 200 one-block ranges, then a gap of 54 * 255 + 10: numWritableNackRanges counts ceil(13781 / 256) = 54
    # blocks for it (199 + 54 < 255), 254 in all; the writer needs 55 with 54 left
    largest, _, rg, _ = _many_ranges(200)
    last = rg[-1][0] - (54 * 255 + 10) - 1
    rg = rg + [(last - 2, last)]
    out.append((_pkt(sack=(largest, last - 2, rg, 0), pn=1), None, "55 blocks where 54 remain"))
    return out


@functools.lru_cache(None)
def family_g():
    good = lambda: _pkt(sack=_two_ranges(3), pn=1, segments=[(4, b"between")])  # noqa: E731
    pk, hand, tags = [], {}, []
    for p, by_hand, tag in _g_cases():
        st = by_hand[0] if by_hand else _ref_encode(p)[0]
        if st != 0:  # a failing packet sits between two good ones
            pk.append(good())
            tags.append("good")
        if by_hand:
            hand[len(pk)] = by_hand
        pk.append(p)
        tags.append(tag)
        if st != 0:
            pk.append(good())
            tags.append("good")
    return Family("g", pk, max_ranges=300, hand=hand, tags=tags)


def _h(text):
    return bytes.fromhex(text)


# (tag, packet, status, bytes by hand from ugo/packet.go:338-430 and :479-505).  The SACK is written as: type
# (0x20 with ranges), uvarint largestAcked, ufloat16 delay (5 -> 05 00), the block count less one (ranges
# only), uvarint firstAckBlockLength, then per further range a gap byte and uvarint length; all in uint64.
WRAP_CASES = [
    # firstAckBlockLength = 100 - 101 + 1 = 0
    ("first length 0", _pkt(sack=(100, 101, [], 5), pn=7), 0, _h("80 00 64 0500 00")),
    ("first length 0, with a segment", _pkt(sack=(100, 101, [], 5), pn=7, segments=[(3, b"\xaa\xbb")]), 0,
     _h("a0 00 64 0500 00 07 03 0002 aabb")),
    # firstAckBlockLength = 100 - 102 + 1 = 2^64 - 1: nine ff and 01
    ("first length 2^64-1", _pkt(sack=(100, 102, [], 5), pn=7), 0, _h("80 00 64 0500 ffffffffffffffffff01")),
    ("first length 2^64-1, with a segment", _pkt(sack=(100, 102, [], 5), pn=7, sw=2, segments=[(3, b"\xaa\xbb")]),
     0, _h("e0 00 64 0500 ffffffffffffffffff01 07 02 03 0002 aabb")),
    # ranges {100..110}, {first 50, last 40}: numWritableNackRanges gap 100 - 40 = 60 -> 1 block, 2 in all
    # (count byte 01); first block 110 - 100 + 1 = 11; gap 100 - 40 - 1 = 59 = 0x3b; length 40 - 50 + 1 =
    # 2^64 - 9 = 0xfffffffffffffff7 -> f7 ff ff ff ff ff ff ff ff 01
    ("range length 2^64-9", _pkt(sack=(110, 50, [(100, 110), (50, 40)], 5), pn=7), 0,
     _h("80 20 6e 0500 01 0b 3b f7ffffffffffffffff01")),
    ("range length 2^64-9, with a segment",
     _pkt(sack=(110, 50, [(100, 110), (50, 40)], 5), pn=7, segments=[(3, b"\xaa\xbb")]), 0,
     _h("a0 20 6e 0500 01 0b 3b f7ffffffffffffffff01 07 03 0002 aabb")),
    # ascending ranges {2..10}, {2^64-6..2^64-2}: numWritableNackRanges gap 2 - (2^64 - 2) = 4 -> 1 block, 2 in
    # all; first block 10 - 2 + 1 = 9; gap 2 - (2^64 - 2) - 1 = 3; length 5
    ("gap wraps to 3", _pkt(sack=(10, M64 - 5, [(2, 10), (M64 - 5, M64 - 1)], 5), pn=7), 0,
     _h("80 20 0a 0500 01 09 03 05")),
    # ascending ranges {100..110}, {200..210}: numWritableNackRanges gap 100 - 210 = 2^64 - 110, far above 255
    # blocks -> returns 1; the writer's gap 2^64 - 111 takes (2^64 - 111) / 255 + 1 blocks, about 7 * 10^16 of
    # them, and numRangesWritten ends above 1 -> "inconsistent number of ACK ranges written"
    ("gap wraps to 2^64-111", _pkt(sack=(110, 200, [(100, 110), (200, 210)], 5), pn=7), 9, b""),
]


@functools.lru_cache(None)
def family_h():
    """The hand-derived results stand in `hand`: the device is held to them,
    and so is the oracle (test_packet_encode_vectors.py)."""
    good = lambda: _pkt(sack=(1000, 990, [], 7), pn=4, segments=[(4, b"neighbour")])  # noqa: E731
    pk, hand, tags = [good()], {}, ["good"]
    for tag, p, st, raw in WRAP_CASES:
        hand[len(pk)] = (st, raw)
        pk += [p, good()]
        tags += [tag, "good"]
    return Family("h", pk, max_ranges=2, hand=hand, tags=tags)


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "c-9000": family_c_9000, "c-fff0": family_c_fff0,
            "d": family_d, "e": family_e, "f": family_f, "g": family_g, "h": family_h}


# ------------------------------------------------------------- send windows
PLACEMENTS = ("nowhere", "first 16 bytes", "last 16 bytes", "interior, at a chunk boundary",
              "interior, off a chunk boundary")


def data_starts(p, framed):
    """The packet byte at which each segment's data starts (header room included)."""
    body = sum(len(pr.put_uvarint(o)) + 2 + len(d) for o, d in p["segments"])
    pos, out = (6 if framed else 0) + len(_ref_encode(p)[1]) - body, []
    for o, d in p["segments"]:
        pos += len(pr.put_uvarint(o)) + 2
        out.append(pos)
        pos += len(d)
    return out


def wrap_placement(o, L, cap, pos):
    """Where the wrap point of a window of cap bytes falls in the copy of
    stream bytes [o, o + L) to packet byte pos: None if outside them, else
    one of PLACEMENTS[1:] ("short" under 16 bytes, copied byte by byte)."""
    k = (-o) % cap  # segment byte k is the window's byte 0
    if k == 0 or k >= L:
        return None
    if L < 16:
        return "short"
    if k < 16:
        return PLACEMENTS[1]
    if k > L - 16:
        return PLACEMENTS[2]
    return PLACEMENTS[3] if (pos + k) % 16 == 0 else PLACEMENTS[4]


def window_layout(fam, framed):
    """`fam` (four-byte segment offsets, no SACK) as the packets of five send
    windows: packet i belongs to member i % 5, its segments are given stream
    offsets in that member, in order with three other bytes between them, and
    every member's window is just large enough for its bytes.  Member m's
    base is chosen so that the window's wrap point falls at PLACEMENTS[m] of
    its segment with the most bytes past the first chunk boundary.  Returns (family of the moved
    packets, conn_of, caps, bases, stream bytes per member, {member:
    placements met})."""
    rng = np.random.default_rng(len(fam.pkts))
    nm = len(PLACEMENTS)
    rel = [[] for _ in range(nm)]  # (packet, segment, relative offset, L, pos)
    end = [0] * nm
    for i, p in enumerate(fam.pkts):
        m = i % nm
        assert p["sack"] is None
        for j, ((o, d), pos) in enumerate(zip(p["segments"], data_starts(p, framed))):
            assert len(pr.put_uvarint(o)) == 4
            rel[m].append((i, j, end[m], len(d), pos))
            end[m] += len(d) + 3
    caps, bases, streams, met = [], [], [], {}
    new = [dict(p, segments=list(p["segments"])) for p in fam.pkts]
    for m in range(nm):
        cap = max(fec.STREAM_MIN_WINDOW, 1 << (end[m] - 1).bit_length())
        k = 0
        if m:
            _, _, at, L, pos = max(rel[m], key=lambda s: s[3] - (16 - s[4] % 16) % 16)
            head = (16 - pos % 16) % 16
            k = at + (5, L - 5, head + 16, head + 19)[m - 1]
        base = (OFF4 // cap + 2) * cap - k
        assert OFF4 <= base and base + end[m] < 1 << 28
        stream = bytearray(_fill(rng, end[m], "random"))
        met[m] = set()
        for i, j, at, L, pos in rel[m]:
            stream[at:at + L] = fam.pkts[i]["segments"][j][1]
            new[i]["segments"][j] = (base + at, fam.pkts[i]["segments"][j][1])
            met[m].add(wrap_placement(base + at, L, cap, pos))
        met[m].discard(None)
        caps.append(cap)
        bases.append(base)
        streams.append(bytes(stream))
    moved = Family(fam.name + " in windows", new, 1, fam.max_segments, fam.slot, None, None, fam.tags)
    return moved, [i % nm for i in range(len(new))], caps, bases, streams, met


# --------------------------------------------------------------------- image
def keystream(n):
    return np.frombuffer(fec.rc4_keystream(KEY, n), np.uint8)


class EncodeImage:
    """guard | wire [n][slot] | guard | wire_lens [n] | guard | status [n] | guard
    in one allocation filled with SENTINEL: `out` is the encoder's output
    triple over it.  buffer: a pinned host array to lay the image in; default
    device memory.  layout_only: no allocation, the offsets and the expectation alone."""

    def __init__(self, n, slot, buffer=None, layout_only=False):
        self.n, self.slot = n, slot
        self.wire_off = GUARD
        self.lens_off = self.wire_off + n * slot + GUARD
        self.status_off = _round16(self.lens_off + 2 * n) + GUARD
        self.size = _round16(self.status_off + n) + GUARD
        if layout_only:
            return
        if buffer is None:
            self.flat = torch.full((self.size,), SENTINEL, dtype=torch.uint8, device="cuda")
        else:
            assert buffer.size >= self.size and buffer.ctypes.data % 16 == 0
            buffer[:self.size] = SENTINEL
            self.flat = torch.from_numpy(buffer[:self.size])
        f = self.flat
        self.out = (f[self.wire_off:self.wire_off + n * slot].view(n, slot),
                    f[self.lens_off:self.lens_off + 2 * n].view(torch.int16),
                    f[self.status_off:self.status_off + n])

    @staticmethod
    def bytes_needed(n, slot):
        return n * slot + 3 * n + 4 * GUARD + 32

    def got(self):
        return self.flat.cpu().numpy().copy()

    def wire(self, image):
        return image[self.wire_off:self.wire_off + self.n * self.slot].reshape(self.n, self.slot)

    def lens(self, image):
        return image[self.lens_off:self.lens_off + 2 * self.n].view(np.uint16)

    def status(self, image):
        return image[self.status_off:self.status_off + self.n]

    def expected(self, exp, framed=False, ks=None, sentinel=SENTINEL):
        """The image the header promises for the results `exp` [(status, bytes)]:
        bytes [0, round_up(len, 16)) of a slot written, zeros (no pad) behind
        len, a failed slot untouched with wire_lens 0."""
        im = np.full(self.size, sentinel, np.uint8)
        wire, lens = self.wire(im), self.lens(im)
        lens[:] = 0
        room = bytes(6) if framed else b""
        for i, (st, raw) in enumerate(exp):
            if st != 0:
                continue
            body = np.frombuffer(room + raw, np.uint8)
            m = len(body)
            assert m <= self.slot
            wire[i, :m] = body if ks is None else body ^ ks[:m]
            wire[i, m:_round16(m)] = 0
            lens[i] = m
        self.status(im)[:] = [st for st, _ in exp]
        return im

    def where(self, at):
        if self.wire_off <= at < self.wire_off + self.n * self.slot:
            return "wire", (at - self.wire_off) // self.slot, (at - self.wire_off) % self.slot
        if self.lens_off <= at < self.lens_off + 2 * self.n:
            return "wire_lens", (at - self.lens_off) // 2, (at - self.lens_off) % 2
        if self.status_off <= at < self.status_off + self.n:
            return "status", at - self.status_off, 0
        return "guard", None, at

    def check(self, got, want, what, label=None):
        bad = np.flatnonzero(got != want)
        if bad.size == 0:
            return
        part, i, b = self.where(int(bad[0]))
        name = label(i) if label is not None and i is not None else "packet %r" % (i,)
        st = int(want[self.status_off + i]) if i is not None else None
        raise AssertionError("%s: %d bytes of the image differ, the first in %s of %s at byte %d: %#x for %#x "
                             "(expected status %r)" % (what, bad.size, part, name, b, got[bad[0]], want[bad[0]], st))
