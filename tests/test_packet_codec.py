"""ugo packet wire codec: the batch decoder
(ugo_fec_packet_decode, one GPU thread per packet) against the restated
ugoPacket.decode / parseSack / parseSegment / ReadUfloat16 / ReadUvarint
(oracle/packet_ref.py, checker only), field by field, on valid packets built
by the restated encoder, every truncation of them, mutated and random bytes,
the FEC-framed receive path of Conn.handlePacket and the RC4 pad.

The reference holds no codec test; the oracle is pinned by the
hand-derived vectors below (Go's documented uvarint example, the ufloat16
definition in ugo/utils/float16.go:12-16) and by encode -> decode round trips.
"""
import os

import numpy as np
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st
import pytest
import torch

import packet_ref as pr
import packet_vectors as pv
import rc4_ref
from ugo_amd import fec

KEY = b"1234567890123456"  # ugo/listener.go:92, ugo/dial.go:132


# ------------------------------------------------------------- oracle pins
def test_oracle_uvarint_and_ufloat16_vectors():
    assert pr.put_uvarint(300) == bytes([0xAC, 0x02])  # encoding/binary docs
    assert pr.put_uvarint(0) == b"\x00" and pr.put_uvarint(127) == b"\x7f" and pr.put_uvarint(128) == b"\x80\x01"
    assert pr.Reader(bytes([0xAC, 0x02])).read_uvarint() == 300
    assert pr.Reader(b"\xff" * 9 + b"\x01").read_uvarint() == (1 << 64) - 1
    for bad, code in [(b"\xff" * 9 + b"\x02", pr.PKT_VARINT_OVERFLOW), (b"\x80" * 10, pr.PKT_VARINT_OVERFLOW),
                      (b"\x80\x80", pr.PKT_UNEXPECTED_EOF), (b"", pr.PKT_EOF)]:
        with pytest.raises(pr.DecodeError) as e:
            pr.Reader(bad).read_uvarint()
        assert e.value.code == code
    # ufloat16 (float16.go:12-16): exponent 0 -> mantissa; else (m | 1<<11) << (e-1)
    rd = lambda w: pr.Reader(bytes([w & 0xFF, w >> 8])).read_ufloat16()  # noqa: E731
    assert rd(0x0000) == 0 and rd(0x07FF) == 2047 and rd(0x0800) == 2048 and rd(0x0FFF) == 4095
    assert rd(0x1000) == 4096 and rd(0x1001) == 4098 and rd(0x1800) == 8192
    assert rd(0xFFFF) == 0x3FFC0000000  # uFloat16MaxValue
    for v in [0, 1, 4095, 4096, 4097, 8191, 12345, 1 << 20, 0x3FFC0000000 - 1, 1 << 50]:
        w = pr.write_ufloat16(v)
        back = pr.Reader(w).read_ufloat16()
        assert back <= v and (v >= 0x3FFC0000000 or back >= v - (v >> 11))  # truncating, 12-bit precision
    assert pr.write_ufloat16(1 << 50) == b"\xff\xff"


def _random_packet(rng):
    kind = rng.integers(0, 6)
    sack = None
    if kind in (0, 2, 3, 5):
        largest = int(rng.integers(1, 1 << int(rng.integers(1, 40))))
        if kind == 3 or kind == 5:  # missing ranges, sometimes with long gaps (> 255)
            ranges, hi = [], largest
            for _ in range(int(rng.integers(2, 7))):
                lo = hi - int(rng.integers(0, 20))
                if lo < 1:
                    break
                ranges.append((lo, hi))
                hi = lo - 2 - int(rng.integers(0, 600 if kind == 5 else 200))
                if hi < 1:
                    break
            if len(ranges) < 2:
                ranges = []
            in_order = ranges[-1][0] if ranges else max(1, largest - int(rng.integers(0, 50)))
            sack = (largest, in_order, ranges, int(rng.integers(0, 1 << 30)))
        else:
            sack = (largest, max(1, largest - int(rng.integers(0, 50))), [], int(rng.integers(0, 5000)))
    segs = []
    if kind != 2:
        for _ in range(int(rng.integers(1, 4)) if kind == 4 else 1):
            segs.append((int(rng.integers(0, 1 << int(rng.integers(1, 60)))),
                         rng.integers(0, 256, int(rng.integers(0, 400)), dtype=np.uint8).tobytes()))
    stop = int(rng.integers(1, 1 << 20)) if rng.random() < 0.3 else 0
    pn = int(rng.integers(1, 1 << int(rng.integers(1, 62))))
    flags = int(rng.choice([0, pr.finFlag, pr.rstFlag])) if rng.random() < 0.2 else 0
    try:
        raw = pr.encode(flags=flags, sack=sack, packet_number=pn, stop_waiting=stop, segments=segs)
    except pr.EncodeError:  # the reference's encode() fails on these: never sent
        return _random_packet(rng)
    return raw, sack, segs, pn


def test_oracle_long_gap_block_count_mismatch_is_an_encode_error():
    # gap 767 between ranges: numWritableNackRanges says 3 blocks, the writer emits 4
    rngs = [(2000, 2010), (2000 - 768 - 5, 2000 - 768)]
    with pytest.raises(pr.EncodeError):
        pr.write_sack(2010, rngs[-1][0], rngs, 0)
    rngs = [(2000, 2010), (2000 - 301 - 5, 2000 - 301)]  # gap 300: consistent, round trips
    st, out = pr.decode(pr.encode(sack=(2010, rngs[-1][0], rngs, 0), packet_number=1))
    assert st == 0 and out["sack"]["ranges"] == rngs


def test_oracle_encode_decode_round_trip():
    rng = np.random.default_rng(3)
    for _ in range(400):
        raw, sack, segs, pn = _random_packet(rng)
        st, out = pr.decode(raw)
        assert st == pr.PKT_OK, raw.hex()
        if out["flags"] != pr.ackFlag:
            assert out["packet_number"] == pn
        assert [(o, raw[d:d + n]) for o, d, n, a in out["segments"]] == segs
        if sack is not None:
            assert out["sack"]["largest_acked"] == sack[0]
            r = sack[2]
            gaps = [r[i - 1][0] - r[i][1] - 1 for i in range(1, len(r))]
            if any(g >= 255 and g % 255 == 0 for g in gaps):
                continue  # the reference's lossy long-gap case (see the test below)
            if r:
                # long gaps are written as extra 0-length blocks and merged back on read
                assert [tuple(x) for x in out["sack"]["ranges"]] == [tuple(x) for x in r]
            assert out["sack"]["largest_in_order"] == sack[1]


def test_oracle_gap_multiple_of_255_decodes_to_a_different_range():
    """ugo/packet.go:393-397 writes a gap of k*255 as (255, 0) x (k-1) then
    (gap % 255 = 0, length); the reader (:285-299) merges the zero-length
    blocks, so the range comes back 255 packets higher -- reference behaviour,
    reproduced, not corrected."""
    pf = 10_000
    rngs = [(pf, pf + 10), (pf - 510 - 1 - 4, pf - 510 - 1)]  # gap 510
    st, out = pr.decode(pr.encode(sack=(pf + 10, rngs[-1][0], rngs, 0), packet_number=1))
    assert st == 0
    assert out["sack"]["ranges"] == [(pf, pf + 10), (pf - 256 - 4, pf - 256)]


# --------------------------------------------------------------- GPU batch
def _corpus(seed, n_valid=600):
    rng = np.random.default_rng(seed)
    pk = []
    for _ in range(n_valid):
        raw, *_ = _random_packet(rng)
        pk.append(raw)
        cut = int(rng.integers(0, len(raw) + 1))  # a truncation of it
        pk.append(raw[:cut])
        if len(raw) > 3:  # a mutation of it
            m = bytearray(raw)
            m[int(rng.integers(0, min(len(m), 24)))] ^= 1 << int(rng.integers(0, 8))
            pk.append(bytes(m))
    for _ in range(300):  # junk
        pk.append(rng.integers(0, 256, int(rng.integers(0, 64)), dtype=np.uint8).tobytes())
    # hand-picked edge cases
    pk += [b"", b"\x80", b"\x80\x00\x05\x00\x00\x01", b"\x20\x01\x00\x05", b"\x20\x01\x00\x05\x01",
           b"\x20\x01\x00\x00", b"\xa0\x20\x0a\x00\x00\x00\x03", b"\x00" + b"\xff" * 11,
           pr.encode(sack=(10, 5, [], 7)), pr.encode(flags=pr.finFlag, sack=(10, 5, [], 7))]
    return pk


def _run(enc, pk, slot, pad_key=None, framed=False, max_ranges=32, max_segments=8):
    host = np.zeros((len(pk), slot), np.uint8)
    for i, b in enumerate(pk):
        host[i, :len(b)] = np.frombuffer(b, np.uint8)
    lens = torch.tensor([len(b) for b in pk], dtype=torch.int16).cuda()
    pad = None
    if pad_key is not None:
        pad = torch.frombuffer(bytearray(fec.rc4_keystream(pad_key, slot)), dtype=torch.uint8).cuda()
        ks = np.frombuffer(fec.rc4_keystream(pad_key, slot), np.uint8)
        host ^= ks[None, :]  # encrypt: the kernel decrypts with the pad
    info, ranges, segs = enc.packet_decode(torch.from_numpy(host).cuda(), lens, pad=pad, framed=framed,
                                           max_ranges=max_ranges, max_segments=max_segments)
    torch.cuda.synchronize()
    info = info.cpu().numpy().view(fec.PKT_INFO_DTYPE).reshape(-1)
    segs = segs.cpu().numpy().reshape(len(pk), -1).view(fec.PKT_SEGMENT_DTYPE).reshape(len(pk), -1)
    return info, ranges.cpu().numpy().view(np.uint64), segs


def _check(pk, info, ranges, segs, framed=False, max_ranges=32, max_segments=8):
    for i, b in enumerate(pk):
        off = 0
        if framed and len(b) >= 6 and b[4] | (b[5] << 8) == 0xF1:
            off = 6
        st, out = pr.decode(b[off:])
        I = info[i]
        assert I["payload_off"] == off, i
        # the low byte of the FEC flag of a packet that holds a whole header, else 0
        assert I["fec_flag_lo"] == (b[4] if framed and len(b) >= 6 else 0), i
        assert not I["reserved"].any(), i
        nr = len(out["sack"]["ranges"]) if st == pr.PKT_OK and out["sack"] else 0
        ns = len(out["segments"]) if st == pr.PKT_OK else 0
        if nr > max_ranges or ns > max_segments:
            st = 6  # UGO_PKT_CAPACITY: decoded, the first max_* are stored and the counts clamped
            nr, ns = min(nr, max_ranges), min(ns, max_segments)
        assert I["status"] == st, f"packet {i} {b.hex()}: status {I['status']} vs {st}"
        if st not in (pr.PKT_OK, 6):
            continue
        assert I["flags"] == out["flags"] and I["packet_number"] == out["packet_number"], i
        assert I["stop_waiting"] == out["stop_waiting"], i
        s = out["sack"] or {"largest_acked": 0, "largest_in_order": 0, "delay_us": 0, "ranges": []}
        assert (I["largest_acked"], I["largest_in_order"], I["delay_us"]) == \
            (s["largest_acked"], s["largest_in_order"], s["delay_us"]), i
        assert I["n_ranges"] == nr, i
        assert [tuple(x) for x in ranges[i, :nr]] == s["ranges"][:nr], i
        assert I["n_segments"] == ns, i
        for j, (o, d, n, a) in enumerate(out["segments"][:ns]):
            assert (segs[i, j]["offset"], segs[i, j]["data_off"], segs[i, j]["len"], segs[i, j]["avail"]) == \
                (o, d + off, n, a), (i, j)


@pytest.mark.gpu
def test_packet_decode_vs_oracle(gpu):
    enc = fec.New(10, 3)
    # the tenth byte of a uvarint and ten continuation bytes, as packet number, stop-waiting,
    # largest acked, first block, later block and segment offset: the random corpus never gets there
    pk = _corpus(1) + [pv.in_position(pos, pv.ENCODINGS[name]) for pos in pv.POSITIONS
                       for name in ("ten-80x9-01", "ten-ffx9-01", "ten-80x9-02", "ten-80x9-7f", "ten-cont")]
    slot = max(len(b) for b in pk) + 15 & ~15
    info, ranges, segs = _run(enc, pk, slot)
    _check(pk, info, ranges, segs)
    codes = set(int(x) for x in info["status"])
    assert {0, 1, 2, 3, 4, 5} <= codes, codes  # the corpus reaches the error paths
    assert (info["status"][-30:] == 3).sum() == 18


@pytest.mark.gpu
def test_packet_decode_small_caps_report_capacity(gpu):
    enc = fec.New(10, 3)
    pk = _corpus(2, n_valid=300)
    slot = max(len(b) for b in pk) + 15 & ~15
    info, ranges, segs = _run(enc, pk, slot, max_ranges=2, max_segments=1)
    _check(pk, info, ranges, segs, max_ranges=2, max_segments=1)
    assert (info["status"] == 6).any()


@pytest.mark.gpu
def test_packet_decode_fec_framed_with_rc4(gpu):
    """Conn.handlePacket with FEC: decrypt, strip the 6-B header of typeData
    packets only (ugo/conn.go:390-405), decode the rest from byte 0."""
    enc = fec.New(10, 3)
    rng = np.random.default_rng(5)
    pk = []
    for i, b in enumerate(_corpus(4, n_valid=200)):
        flag = [0xF1, 0xF1, 0xF2, 0x1234][i % 4]
        pk.append(int(i).to_bytes(4, "little") + flag.to_bytes(2, "little") + b)
    pk += [b"\x00\x00\x00\x00\xf1", b"", rng.integers(0, 256, 5, dtype=np.uint8).tobytes()]
    slot = max(len(b) for b in pk) + 15 & ~15
    info, ranges, segs = _run(enc, pk, slot, pad_key=KEY, framed=True)
    _check(pk, info, ranges, segs, framed=True)
    assert rc4_ref.keystream(KEY, 8) == fec.rc4_keystream(KEY, 8)


@pytest.mark.gpu
@settings(max_examples=int(os.environ.get("UGO_HYP_EXAMPLES_PKT", "40")), deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2**31 - 1), max_ranges=st.integers(1, 40), max_segments=st.integers(1, 10),
       framed=st.booleans(), encrypt=st.booleans())
def test_packet_decode_random_corpora(gpu, seed, max_ranges, max_segments, framed, encrypt):
    """Seeded corpora (valid packets, truncations, bit flips, junk), random
    range / segment caps, FEC framing and RC4 on or off: every packet's status,
    header fields, ranges and segment views equal the restated decoder's."""
    enc = fec.New(10, 3)
    rng = np.random.default_rng(seed)
    pk = []
    for i, b in enumerate(_corpus(seed, n_valid=60)):
        if framed:
            flag = [0xF1, 0xF1, 0xF2, 0x1234][i % 4]
            b = int(rng.integers(0, 2**32)).to_bytes(4, "little") + flag.to_bytes(2, "little") + b
        pk.append(b)
    slot = max(len(b) for b in pk) + 15 & ~15
    info, ranges, segs = _run(enc, pk, slot, pad_key=b"1234567890123456" if encrypt else None, framed=framed,
                              max_ranges=max_ranges, max_segments=max_segments)
    _check(pk, info, ranges, segs, framed=framed, max_ranges=max_ranges, max_segments=max_segments)
