"""The directed packet corpus and the output image of tests/packet_vectors.py,
without a GPU.

The hand-derived vectors pin the oracle (oracle/packet_ref.py) where the GPU
tests lean on it hardest: uint64 wrap in parseSack / validateAckRanges and the
tenth byte of a uvarint.  The values asserted here were traced by hand from
ugo/packet.go (the derivations stand next to the vectors in
packet_vectors.sack_vectors) and Go's encoding/binary, not taken from the
oracle's output.  The coverage conditions keep the corpus from thinning out
unnoticed, and the image helper is shown to decode a planted byte to the
right (array, packet, entry, field).
"""
import numpy as np
import pytest

import packet_ref as pr
import packet_vectors as pv

M = pv.M64


def _by_name(vectors):
    return dict(vectors)


def _dec(raw):
    st, out = pr.decode(raw)
    return st, out


# ------------------------------------------------------------- oracle pins
@pytest.mark.parametrize("name,value", [
    ("v0", 0), ("v1", 127), ("v2", 128), ("v3", (1 << 14) - 1), ("v4", 1 << 14), ("v5", (1 << 56) - 1),
    ("v6", (1 << 63) - 1), ("v7", 1 << 63), ("v8", M), ("ten-80x9-01", 1 << 63), ("ten-ffx9-01", M),
    ("ten-ffx9-00", (1 << 63) - 1), ("nc-81-80-00", 1), ("nc-80-00", 0), ("nc-ff-80-80-00", 127)])
def test_oracle_uvarint_legal_forms(name, value):
    enc = pv.ENCODINGS[name]
    r = pr.Reader(enc + b"\x55")
    assert r.read_uvarint() == value and r.i == len(enc)
    # the same through a whole packet, in the two positions that take any value
    st, out = _dec(pv.in_position("packet_number", enc))
    assert st == 0 and out["packet_number"] == value and out["segments"] == [(5, len(enc) + 4, 2, 2)]
    st, out = _dec(pv.in_position("segment_offset", enc))
    assert st == 0 and out["segments"] == [(value, len(enc) + 4, 2, 2)]


@pytest.mark.parametrize("name,consumed", [
    ("ten-80x9-02", 10), ("ten-ffx9-02", 10), ("ten-80x9-7f", 10), ("ten-cont", 10), ("ten-cont-ff", 10),
    ("eleven-ff", 10), ("eleven-80x10-00", 10)])
def test_oracle_uvarint_overflow_forms(name, consumed):
    r = pr.Reader(pv.ENCODINGS[name] + b"\x00")
    with pytest.raises(pr.DecodeError) as e:
        r.read_uvarint()
    assert e.value.code == pr.PKT_VARINT_OVERFLOW and r.i == consumed
    for pos in pv.POSITIONS:
        assert _dec(pv.in_position(pos, pv.ENCODINGS[name]))[0] == pr.PKT_VARINT_OVERFLOW, pos


def test_oracle_noncanonical_packet_number():
    assert _dec(b"\x00\x81\x80\x00") == (0, {"flags": 0, "sack": None, "packet_number": 1, "stop_waiting": 0,
                                              "segments": []})


def test_oracle_uint64_edges_in_the_sack_positions():
    big = pv.BIG
    # largest 2^64-1, first block 1: in order 2^64-1
    st, out = _dec(pv.in_position("largest_acked", big))
    assert st == 0 and out["sack"]["largest_acked"] == M and out["sack"]["largest_in_order"] == M
    # largest 0 with first block 1: 1 > 0
    assert _dec(pv.in_position("largest_acked", b"\x00"))[0] == pr.PKT_INVALID_ACK_RANGES
    # first block 2^64-1 under largest 2^64-1: in order M + 1 - M = 1; 2^63: 2^63
    st, out = _dec(pv.in_position("first_block", big))
    assert st == 0 and out["sack"]["largest_in_order"] == 1
    st, out = _dec(pv.in_position("first_block", pv.ENCODINGS["ten-80x9-01"]))
    assert st == 0 and out["sack"]["largest_in_order"] == 1 << 63
    assert _dec(pv.in_position("first_block", b"\x00"))[0] == pr.PKT_INVALID_FIRST_ACK_RANGE
    # [M,M], gap 1, block 2^63: last = M-2, first = M-2-2^63+1 = 2^63-2
    st, out = _dec(pv.in_position("later_block", pv.ENCODINGS["ten-80x9-01"]))
    assert st == 0 and out["sack"]["ranges"] == [(M, M), ((1 << 63) - 2, M - 2)]
    assert out["sack"]["largest_in_order"] == (1 << 63) - 2 and out["packet_number"] == 7
    # block M-2 reaches down to 1; M-1 to 0; M wraps first above last
    st, out = _dec(pv.in_position("later_block", pv.uv(M - 2)))
    assert st == 0 and out["sack"]["ranges"][1] == (1, M - 2)
    st, out = _dec(pv.in_position("later_block", pv.uv(M - 1)))
    assert st == 0 and out["sack"]["ranges"][1] == (0, M - 2)
    assert _dec(pv.in_position("later_block", big))[0] == pr.PKT_INVALID_ACK_RANGES
    # a block of 0 leaves the second range incomplete: dropped, one range left
    assert _dec(pv.in_position("later_block", b"\x00"))[0] == pr.PKT_INVALID_ACK_RANGES


SACK_PINS = {
    "sack/wrap-below-zero": (4, None, None),
    "sack/top-gap1": (0, [(M, M), (M - 2, M - 2)], M - 2),
    "sack/top-gap0": (4, None, None),
    "sack/long-chain-to-zero-wraps": (4, None, None),
    "sack/long-chain-to-zero": (0, [(10, 10), (0, 0)], 0),
    "sack/incomplete-last-of-three": (0, [(19, 20), (16, 17)], 16),
    "sack/nblocks1-len0": (4, None, None),
    "sack/nblocks0-missing": (4, None, None),
    "sack/first-len0": (5, None, None),
    "sack/first-len0-missing": (5, None, None),
    "sack/first-above-largest": (4, None, None),
    "sack/first-equals-largest": (0, [], 1),
    "sack/largest0": (4, None, None),
    "sack/type-00": (0, [], 8),
    "sack/type-df": (0, [], 8),
    "sack/type-20": (0, [(8, 9), (6, 6)], 6),
    "sack/type-ff": (0, [(8, 9), (6, 6)], 6),
}


@pytest.mark.parametrize("name", sorted(SACK_PINS))
def test_oracle_sack_arithmetic(name):
    status, ranges, in_order = SACK_PINS[name]
    st, out = _dec(_by_name(pv.sack_vectors())[name])
    assert st == status
    if status == 0:
        assert out["sack"]["ranges"] == ranges and out["sack"]["largest_in_order"] == in_order
        if name.startswith("sack/type-"):
            assert out["sack"]["delay_us"] == 0x1234 - (1 << 11) << 1 and out["packet_number"] == 7  # exponent 1
            assert out["segments"] == [(5, len(_by_name(pv.sack_vectors())[name]) - 2, 2, 2)]


def test_oracle_256_ranges_and_the_long_chain():
    raw = _by_name(pv.sack_vectors())["sack/256-ranges"]
    st, out = _dec(raw)
    assert len(raw) == 518 and st == 0
    # [10000,10000], then 255 x (gap 1, length 1): 9998, 9996, ...
    assert out["sack"]["ranges"] == [(10000 - 2 * k, 10000 - 2 * k) for k in range(256)]
    assert out["sack"]["largest_in_order"] == 10000 - 510
    # [2^40,2^40]; (255,0) opens last = 2^40-256, first = last+1; 253 more move it down by 255
    # each; (7,3): first -= 10, last -= 7
    st, out = _dec(_by_name(pv.sack_vectors())["sack/254-long-blocks"])
    last = (1 << 40) - 256 - 253 * 255 - 7
    assert st == 0 and out["sack"]["ranges"] == [(1 << 40, 1 << 40), (last - 2, last)]
    for k in (2, 3, 32, 33):
        st, out = _dec(_by_name(pv.sack_vectors())["sack/%d-ranges" % k])
        assert st == 0 and len(out["sack"]["ranges"]) == k


def test_oracle_segment_edges():
    v = _by_name(pv.segment_vectors())
    assert _dec(v["seg/len0"])[1]["segments"] == [(5, 5, 0, 0)]
    assert _dec(v["seg/len0-twice"])[1]["segments"] == [(5, 5, 0, 0), (6, 8, 0, 0)]
    st, out = _dec(v["seg/ffff-1-byte"])
    assert st == 0 and out["segments"] == [(0, 5, 0xFFFF, 1)]
    assert _dec(v["seg/ffff-0-bytes"])[0] == pr.PKT_EOF
    assert _dec(v["seg/half-be16"])[0] == pr.PKT_UNEXPECTED_EOF
    assert _dec(v["seg/no-be16"])[0] == pr.PKT_EOF
    st, out = _dec(v["seg/short-last"])
    assert st == 0 and out["segments"] == [(5, 5, 2, 2), (6, 10, 9, 3)]
    assert _dec(v["seg/none"]) == (0, {"flags": 0x20, "sack": None, "packet_number": 1, "stop_waiting": 0,
                                       "segments": []})
    st, out = _dec(v["seg/pure-ack-then-bytes"])  # no packet number behind a pure ACK: 05 is a segment offset
    assert st == 0 and out["packet_number"] == 0 and out["segments"] == [(5, 9, 1, 1)]
    for k in (1, 2, 3, 8, 9):
        st, out = _dec(v["seg/%d-segments" % k])
        assert st == 0 and out["segments"] == [(3, 5 + 4 * j, 1, 1) for j in range(k)]
    st, out = _dec(v["seg/fills-slot"])
    assert len(v["seg/fills-slot"]) == 528 and st == 0 and out["segments"] == [(0, 5, 523, 523)]


def test_oracle_oversized_packets():
    v = _by_name(pv.oversized_vectors())
    st, out = _dec(v["big/21839-segments"])
    assert len(v["big/21839-segments"]) == 65519 and st == 0
    assert out["segments"] == [(0, 5 + 3 * j, 0, 0) for j in range(pv.MANY_SEGMENTS)]
    st, out = _dec(v["big/40000-bytes"])
    assert st == 0 and out["packet_number"] == 1 and out["segments"] == [(0, 10, 39990, 39990)]
    assert np.array([40000], np.uint16).view(np.int16)[0] < 0  # negative as the binding's int16


def test_oracle_ufloat16_is_monotonic_and_hits_its_ends():
    d = [pr.decode(b)[1]["sack"]["delay_us"] for _, b in pv.ufloat16_vectors()]
    assert len(d) == 65536 and d[:4097] == list(range(4097)) and d[0xFFFF] == 0x3FFC0000000
    assert all(a < b for a, b in zip(d, d[1:]))
    # float16.go:12-16: above the denormals a value is (mantissa | 1 << 11) << (exponent - 1)
    for w in (0x1000, 0x1801, 0x7ABC, 0xFFFF):
        assert d[w] == ((w & 0x7FF) | 0x800) << ((w >> 11) - 1)


def test_small_alphabet_census():
    from collections import Counter

    v = pv.small_alphabet_vectors()
    c = Counter(pr.decode(b)[0] for _, b in v)
    assert len(v) == 66430 and c == {0: 3552, 1: 42313, 2: 20565}


# ---------------------------------------------------------------- coverage
@pytest.fixture(scope="module")
def traces():
    out = []
    for name, b in pv.directed():
        st, ev = pv.field_trace(b)
        assert st == pr.decode(b)[0]
        out.append((name, b, st, ev))
    return out


def test_corpus_reaches_every_status(traces):
    assert {st for _, _, st, _ in traces} == {0, 1, 2, 3, 4, 5}
    with_prefixes = {pr.decode(full[:cut])[0] for _, full, cut in pv.with_prefixes()}
    assert with_prefixes == {0, 1, 2, 3, 4, 5}
    assert len({full[:cut] for _, full, cut in pv.with_prefixes()}) == len(pv.with_prefixes())


def test_corpus_overflows_and_tops_out_in_every_position(traces):
    overflow = {pos for _, _, _, ev in traces for pos, _, _, _, st in ev if st == pr.PKT_VARINT_OVERFLOW}
    assert overflow == set(pv.POSITIONS)
    top = {pos for _, _, _, ev in traces for pos, _, _, v, st in ev if st == 0 and v >= 1 << 63 and pos in pv.POSITIONS}
    assert top == set(pv.POSITIONS)
    # ... in packets that decode, where the value has to come out right
    top_ok = {pos for _, _, s, ev in traces if s == 0 for pos, _, _, v, st in ev if st == 0 and v >= 1 << 63}
    assert top_ok == set(pv.POSITIONS)


def test_corpus_has_256_ranges_and_the_slot_filler(traces):
    assert max(len(pr.decode(b)[1]["sack"]["ranges"]) for _, b, st, _ in traces
               if st == 0 and pr.decode(b)[1]["sack"]) == 256
    longest = max(len(b) for _, b, _, _ in traces)
    assert longest == 528 and longest % 16 == 0  # lens[i] == slot in the directed batches


def test_framed_batches_give_every_vector_both_framings():
    """The framed GPU batches are frame_both() of the prefix corpus: every
    packet of it once behind a typeData header, which is stripped, and once
    behind another flag, which leaves the header in front of it."""
    pk = [full[:cut] for _, full, cut in pv.with_prefixes()]
    both = pv.frame_both(pk)
    n = len(pk)
    assert len(both) == 2 * n
    for i, b in enumerate(pk):
        a, c = pv.payload_start(both[i], True)[0], pv.payload_start(both[n + i], True)[0]
        assert {a, c} == {0, 6} and both[i][6:] == both[n + i][6:] == b, i


def test_corpus_reaches_every_chunk_offset(traces):
    """Slot offsets modulo 16 at which each field kind starts, in the batches
    the GPU tests decode: the unframed one (every vector at byte 0 of its
    slot) and the framed one, where only the packets whose typeData header is
    stripped count, at byte 6."""
    by_bytes = {b: ev for _, b, _, ev in traces}
    runs = [(0, b) for b in by_bytes]
    for b in pv.frame_both([full[:cut] for _, full, cut in pv.with_prefixes()]):
        off, _ = pv.payload_start(b, True)
        if off == 6 and b[6:] in by_bytes:
            runs.append((6, b[6:]))
    assert sorted(b for base, b in runs if base == 6) == sorted(by_bytes)  # each vector, stripped, once
    starts = {}
    straddles = set()
    for base, b in runs:
        for pos, start, end, _, st in by_bytes[b]:
            if st != 0:
                continue
            starts.setdefault(pos, set()).add((base + start) % 16)
            if (base + start) // 16 != (base + end - 1) // 16:
                straddles.add(pos)
            if pos == "segment_length" and (base + start) % 16 == 15:
                straddles.add(("be16-first-byte-last", base))
    for pos in pv.POSITIONS + ("segment_length",):
        if pos == "largest_acked":  # flags and the SACK type byte are all that precedes it
            assert starts[pos] == {2, 8}
        else:
            assert starts[pos] == set(range(16)), pos
        assert pos in straddles, pos
    # the BE16 with its first byte last in a chunk, both ways of framing
    assert {("be16-first-byte-last", 0), ("be16-first-byte-last", 6)} <= straddles


def test_frame_rotates_the_flags():
    f = pv.frame([b"\x20\x01"] * 5)
    assert [pv.payload_start(b, True) for b in f] == [(6, 0xF1), (6, 0xF1), (0, 0xF2), (0, 0x34), (6, 0xF1)]
    assert pv.payload_start(b"\x00\x00\x00\x00\xf1", True) == (0, 0) and pv.payload_start(f[0], False) == (0, 0)


# ------------------------------------------------------------------- image
PK = [b"\x20\x01\x05\x00\x02\xaa\xbb",                        # OK, one segment
      b"\x80\x20\x14\x00\x00\x02\x02\x01\x02\x01\x01",        # OK, three ranges
      b"\x20\x01\x00\xff",                                    # status 2
      pv.segments_packet(3),                                  # CAPACITY under S = 2
      b""]                                                    # status 1


@pytest.fixture()
def image():
    im = pv.DecodeImage(len(PK), 4, 2, device=None)
    want, mask = im.expected(PK)
    return im, want, mask


def test_image_expected_content(image):
    im, want, mask = image
    info, ranges, segs = im.info(want), im.ranges(want), im.segs(want)
    assert info["status"].tolist() == [0, 0, 2, 6, 1]
    assert info["n_segments"].tolist() == [1, 0, 0, 2, 0] and info["n_ranges"].tolist() == [0, 3, 0, 0, 0]
    assert ranges[1, :3].tolist() == [[19, 20], [16, 17], [14, 14]] and info[1]["largest_in_order"] == 14
    assert (ranges[1, 3] == 0xA5A5A5A5A5A5A5A5).all() and (ranges[0] == 0xA5A5A5A5A5A5A5A5).all()
    assert segs[0, 0].tolist() == (5, 5, 2, 2) and segs[3].tolist() == [(0, 5, 0, 0), (0, 8, 0, 0)]
    assert (want[:pv.GUARD] == pv.SENTINEL).all() and (want[-pv.GUARD:] == pv.SENTINEL).all()
    assert (info["reserved"] == 0).all()
    # what an error packet leaves open: its record but four fields, and its own rows
    assert mask.sum() == mask.size - 2 * ((64 - 4 - 4 - 1 - 10) + 4 * 16 + 2 * 16)
    im.check(want.copy(), want, mask)


@pytest.mark.parametrize("where", [
    ("info", 1, None, "largest_in_order"), ("info", 0, None, "fec_flag_lo"), ("info", 3, None, "n_segments"),
    ("info", 2, None, "status"), ("info", 4, None, "reserved"), ("info", 2, None, "payload_off"),
    ("ranges", 1, 2, "last"), ("ranges", 1, 3, "first"), ("ranges", 0, 0, "first"), ("ranges", 3, 3, "last"),
    ("segs", 0, 0, "data_off"), ("segs", 0, 1, "offset"), ("segs", 3, 1, "avail"), ("segs", 1, 0, "len")])
def test_image_decodes_a_planted_byte(image, where):
    im, want, mask = image
    array, packet, entry, field = where
    dtype = {"info": pv.PKT_INFO_DTYPE, "ranges": pv.RANGE_DTYPE,
             "segs": pv.PKT_SEGMENT_DTYPE}[array]
    base, per = {"info": (im.info_off, 1), "ranges": (im.ranges_off, im.Ra), "segs": (im.segs_off, im.Sa)}[array]
    sub, col = dtype.fields[field][:2]
    off = base + (packet * per + (entry or 0)) * dtype.itemsize + col + sub.itemsize - 1
    got = want.copy()
    got[off] ^= 0x40
    assert im.mismatch(got, want, mask) == (1, off, where)
    with pytest.raises(AssertionError, match=r"\(array, packet, entry, field\) = \(%r, %d" % (array, packet)):
        im.check(got, want, mask, "planted", PK)


def test_image_reports_a_guard_byte_and_ignores_masked_ones(image):
    im, want, mask = image
    for off in (0, im.info_off - 1, im.ranges_off - 1, im.ranges_off - pv.GUARD, im.segs_off - 1, im.size - 1):
        got = want.copy()
        got[off] = 0
        assert im.mismatch(got, want, mask) == (1, off, "guard")
        with pytest.raises(AssertionError, match="guard"):
            im.check(got, want, mask)
    got = want.copy()
    info = im.info(got)
    info[2]["packet_number"] = 77          # an error packet's other fields
    info[4]["n_segments"] = 9
    im.ranges(got)[2] = 1                  # and its own rows
    im.segs(got)[4]["offset"] = 5
    assert im.mismatch(got, want, mask) is None
    im.ranges(got)[3, 0, 0] = 1            # but not the rows of a packet that decoded
    assert im.mismatch(got, want, mask)[2] == ("ranges", 3, 0, "first")


def test_image_zero_caps_keep_one_untouched_entry():
    im = pv.DecodeImage(len(PK), 0, 0, device=None)
    want, mask = im.expected(PK)
    info = im.info(want)
    assert info["status"].tolist() == [6, 6, 2, 6, 1] and not info["n_ranges"].any() and not info["n_segments"].any()
    assert (im.ranges(want) == 0xA5A5A5A5A5A5A5A5).all() and (want[im.segs_off:] == pv.SENTINEL).all()
    assert im.size == pv.DecodeImage.bytes_needed(len(PK), 0, 0)


def test_ring_slack_and_encryption():
    rng = np.random.default_rng(0)
    fulls = [b"\x01\x02\x03\x04\x05", b"\x09"]
    for slack in (0, 0xFF, 0x80, "random"):
        slots, lens = pv.ring([b"\x01\x02", b"\x09"], 16, slack=slack, fulls=fulls, rng=rng)
        assert lens.tolist() == [2, 1] and slots[0, :5].tolist() == [1, 2, 3, 4, 5] and slots[1, 0] == 9
        if slack != "random":
            assert (slots[0, 5:] == slack).all() and (slots[1, 1:] == slack).all()
    enc, _ = pv.ring([b"\x01\x02"], 16, slack=0xFF, encrypt=True)
    assert (enc[0] ^ pv.keystream(16)).tolist() == [1, 2] + [0xFF] * 14
