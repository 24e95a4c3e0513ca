"""The directed corpus of tests/packet_encode_vectors.py held on the CPU: the
oracle's WriteUfloat16 against its own ReadUfloat16 as properties, the
hand-derived bytes of the 2^64 wraps against the oracle, what each family has
to reach (so that an edit cannot thin it unnoticed), and the oracle's encode
against its decode over every family.
"""
import numpy as np
import pytest

import packet_encode_vectors as ev
import packet_ref as pr
from ugo_amd import fec

M64 = ev.M64
MAX_VALUE = 0x3FFC0000000  # uFloat16MaxValue, ugo/utils/float16.go


def _code(value):
    b = pr.write_ufloat16(value)
    return b[0] | (b[1] << 8)


# ----------------------------------------------------------------- ufloat16
def test_write_ufloat16_inverts_read_for_every_code():
    values = [ev.ufloat16_value(c) for c in range(1 << 16)]
    assert all(a < b for a, b in zip(values, values[1:])), "read is not strictly increasing"
    assert [_code(v) for v in values] == list(range(1 << 16))


def test_write_ufloat16_truncates():
    """The code written is the largest one whose value is not above the input:
    one below the next code's value still writes this code."""
    for c in range((1 << 16) - 1):
        assert _code(ev.ufloat16_value(c + 1) - 1) == c, c


def test_write_ufloat16_clamps():
    assert ev.ufloat16_value(0xFFFF) == MAX_VALUE
    for x in (MAX_VALUE, MAX_VALUE + 1, (1 << 42) - 1, 1 << 42, (1 << 42) + 1, 1 << 63, M64):
        assert _code(x) == 0xFFFF, hex(x)
    assert _code(MAX_VALUE - 1) == 0xFFFE


# ------------------------------------------------------------ 2^64, by hand
@pytest.mark.parametrize("case", ev.WRAP_CASES, ids=[c[0] for c in ev.WRAP_CASES])
def test_oracle_reproduces_the_hand_derived_wraps(case):
    _, p, st, raw = case
    assert ev._ref_encode(p) == (st, raw)


def _writer_fails_literally(ranges):
    """packet.go:380-427 with its loop over the blocks, counting alone."""
    num_ranges, written = pr._num_writable_nack_ranges(ranges), 1
    for i in range(1, len(ranges)):
        gap = (ranges[i - 1][0] - ranges[i][1] - 1) & M64
        num = gap // 0xFF + 1 - (1 if gap % 0xFF == 0 else 0)
        for _ in range(num):
            written += 1
        if written >= num_ranges:
            break
    return num_ranges != written


def test_oracle_refuses_unbounded_gaps_without_looping():
    """The writer of packet.go emits gap / 255 blocks before it fails: the
    oracle fails at once, and agrees with the loop wherever the loop is short."""
    for gap in (1 << 40, 1 << 62, M64 - (1 << 21)):
        assert ev._ref_encode(ev._pkt(sack=ev._two_ranges(gap, hi=(gap + (1 << 20)) & M64)))[0] == 9, gap
    gaps = sorted({*range(0, 70000, 97), *(k * m + d for k in range(1, 260) for m in (255, 256) for d in (-1, 0, 1))})
    fails = 0
    for gap in gaps:
        s = ev._two_ranges(gap)
        st = ev._ref_encode(ev._pkt(sack=s))[0]
        assert (st == 9) == _writer_fails_literally(s[2]), gap
        fails += st == 9
    assert 100 < fails < len(gaps) - 100
    three = ev._many_ranges(200)[2]
    for gap in (5, 54 * 255, 54 * 255 + 10, 60 * 255 + 5):
        last = three[-1][0] - gap - 1
        rg = three + [(last - 2, last)]
        st = ev._ref_encode(ev._pkt(sack=(rg[0][1], last - 2, rg, 0)))[0]
        assert (st == 9) == _writer_fails_literally(rg), gap


# ----------------------------------------------------------------- coverage
def _first_data_start(raw, L):
    """Where a single segment's data starts: it ends the packet."""
    return len(raw) - L


def test_family_a_reaches_every_residue_and_length():
    f = ev.family_a()
    for framed in (False, True):
        seen = set()
        for p, (st, raw), tag in zip(f.pkts, f.expected(framed), f.tags):
            L = len(p["segments"][0][1])
            assert st == 0 and raw.endswith(p["segments"][0][1])
            pos = (6 if framed else 0) + _first_data_start(raw, L)
            assert framed or pos % 16 == tag[0]
            seen.add((pos % 16, L))
        assert seen == {(r, L) for r in range(16) for L in range(49)}, framed
    assert {(t[0], r[0], t[2]) for t, r in zip(f.tags, f.residues)} == \
        {(d, s, L) for d in range(16) for s in ev.SRC_RESIDUES for L in range(49)}


def test_family_b_reaches_every_residue_for_the_third_segment():
    f = ev.family_b()
    seen = set()
    for p, (st, raw) in zip(f.pkts[:-1], f.oracle[:-1]):
        assert st == 0 and len(p["segments"]) == 3
        L3 = len(p["segments"][2][1])
        seen.add(((len(raw) - L3) % 16, L3))
    assert seen == {(r, L) for r in range(16) for L in ev.THIRD_L}
    assert all(len(set(r)) > 1 for r in f.residues[:48]), "each segment has its own source residue"
    lens = [len(d) for _, d in f.pkts[-1]["segments"]]
    assert len(lens) == f.max_segments == 64 and min(lens) == 0 and max(lens) == 20 and f.oracle[-1][0] == 0


def _chunks(raw, L):
    pos = _first_data_start(raw, L)
    c0, c1 = (pos + 15) >> 4, (pos + L) >> 4
    return c1 - c0, 16 * c0 - pos, pos + L - 16 * c1


def test_family_c_reaches_every_chunk_count():
    f = ev.family_c()
    seen = set()
    for p, (st, raw) in zip(f.pkts, f.oracle):
        assert st == 0
        seen.add(_chunks(raw, len(p["segments"][0][1])))
    assert seen == {(n, h, t) for n in ev.CHUNK_COUNTS for h in (0, 1, 15) for t in (0, 1, 15)}
    assert len(f.pkts) <= 300
    big = ev.family_c_fff0()
    assert [len(raw) for _, raw in big.oracle][1::2] == [0xFFF0, 0xFFF1, 0xFFEA]
    assert [st for st, _ in big.expected(False)] == [0, 0, 0, 6, 0, 0, 0]
    assert [st for st, _ in big.expected(True)] == [0, 6, 0, 6, 0, 0, 0]
    j = ev.family_c_9000()
    assert j.slot == 9024 and all(len(p["segments"][0][1]) == 9000 for p in j.pkts)


def test_family_d_sums_pass_16_bits():
    f = ev.family_d()
    lens = [tuple(len(d) for _, d in p["segments"]) for p in f.pkts[1::2]]
    assert lens == list(ev.SIZE_SUMS) and f.slot == 0xFFF0
    totals = [len(raw) for _, raw in f.oracle[1::2]]
    assert all(t > 0xFFFF and t % (1 << 16) <= f.slot for t in totals)  # a sum held in 16 bits would fit
    assert [st for st, _ in f.expected()] == [0, 6, 0, 6, 0, 6, 0]
    # what such an encoder would write stays inside the slots that follow the packet
    assert all(t <= f.slot * (len(f.pkts) - i) for t, i in zip(totals, (1, 3, 5)))


def test_family_e_has_every_uvarint_length_in_every_position():
    f = ev.family_e()
    seen = set()
    for (pos, v), (st, raw) in zip(f.tags, f.oracle):
        assert st == 0 and pr.put_uvarint(v) in raw, (pos, v)
        seen.add((pos, len(pr.put_uvarint(v))))
    assert seen == {(pos, n) for pos in ev.UVARINT_POSITIONS for n in range(1, 11)}
    # one position at a time: the packets of one value differ from its one-byte form in that field alone
    assert len(f.pkts) == 6 * 19


def test_family_f_holds_every_code():
    f = ev.family_f()
    assert len(f.pkts) == 2 * 65536 - 1 + 5 and f.slot == 16
    codes = {raw[-3] | (raw[-2] << 8) for _, raw in f.oracle}
    assert codes == set(range(1 << 16))
    assert {len(raw) for _, raw in f.oracle} == {7}


def test_family_g_failures_sit_between_good_packets():
    f = ev.family_g()
    exp = f.expected()
    bad = [i for i, (st, _) in enumerate(exp) if st != 0]
    assert len(bad) == 15 + 2 + 1 + 2 + 1  # the gaps of test_oracle_long_gap_pins, 511 and 767 again, 2^40, 7 and 8, 55 / 54
    for i in bad:
        assert exp[i - 1][0] == 0 and exp[i + 1][0] == 0, f.label(i)
    assert sum(t.startswith("gap ") for t in f.tags) == 1600 + 5
    assert len(exp[f.tags.index("300 ranges")][1]) == 517


def test_every_status_occurs():
    seen = set()
    for name, make in ev.FAMILIES.items():
        f = make()
        seen |= {st for st, _ in f.expected(False)} | {st for st, _ in f.expected(True)}
        assert len(f.pkts) == len(f.tags) == len(f.oracle), name
    assert seen == {0, fec.PKT_CAPACITY, fec.PKT_INCONSISTENT_LARGEST_ACKED, fec.PKT_INCONSISTENT_LOWEST_ACKED,
                    fec.PKT_INCONSISTENT_RANGE_COUNT}
    assert (fec.PKT_CAPACITY, fec.PKT_INCONSISTENT_RANGE_COUNT) == (6, 9)


@pytest.mark.parametrize("framed", [False, True], ids=["unframed", "framed"])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_window_layout_meets_every_wrap_placement(name, framed):
    f = ev.FAMILIES[name]()
    moved, conn, caps, bases, streams, met = ev.window_layout(f, framed)
    assert [met[m] for m in range(5)] == [set()] + [{p} for p in ev.PLACEMENTS[1:]]
    for m in range(5):
        assert caps[m] >= len(streams[m]) > caps[m] // 2 or caps[m] == fec.STREAM_MIN_WINDOW  # just large enough
    # the same packets but for the offsets' values: every header byte keeps its place
    for p, q, (st, raw), (st2, raw2) in zip(f.pkts, moved.pkts, f.oracle, moved.oracle):
        assert st == st2 == 0 and len(raw) == len(raw2)
        assert ev.data_starts(p, framed) == ev.data_starts(q, framed)
        assert [d for _, d in p["segments"]] == [d for _, d in q["segments"]]
    for i, q in enumerate(moved.pkts):
        for o, d in q["segments"]:
            at = o - bases[conn[i]]
            assert streams[conn[i]][at:at + len(d)] == d


# --------------------------------------------------------------- round trip
@pytest.mark.parametrize("name", sorted(ev.FAMILIES))
def test_family_round_trips_through_the_oracles_decoder(name):
    f = ev.FAMILIES[name]()
    kept = 0
    for i, (p, (st, raw)) in enumerate(zip(f.pkts, f.oracle)):
        if not ev.round_trips(p, st):
            continue
        kept += 1
        dst, out = pr.decode(raw)
        assert dst == 0, f.label(i)
        assert out["flags"] == raw[0] and out["stop_waiting"] == p["sw"], f.label(i)
        assert out["packet_number"] == (p["pn"] if raw[0] != 0x80 else 0), f.label(i)
        if p["sack"] is None:
            assert out["sack"] is None
        else:
            largest, in_order, rg, delay = p["sack"]
            s = out["sack"]
            assert (s["largest_acked"], s["largest_in_order"], s["ranges"]) == (largest, in_order, rg), f.label(i)
            assert s["delay_us"] == ev.ufloat16_value(_code(delay)), f.label(i)
        assert [(o, n, a) for o, _, n, a in out["segments"]] == [(o, len(d), len(d)) for o, d in p["segments"]], f.label(i)
        assert all(raw[at:at + n] == d for (_, at, n, _), (_, d) in zip(out["segments"], p["segments"])), f.label(i)
    floor = {"a": 3920, "b": 385, "c": 180, "c-9000": 3, "c-fff0": 7, "d": 7, "e": 4 * 19, "f": 131076, "g": 1600,
             "h": 9}
    assert kept >= floor[name], (name, kept)


def test_describe_lays_segments_where_asked():
    """_describe in its three new forms: residues per segment, the bytes
    around the segments, a row of payload per packet."""
    f = ev.family_b()
    for surround in (None, "zeros", "ff", "random"):
        for per_packet in (False, True):
            rng = np.random.default_rng(1)
            info, ranges, segs, payload = ev._describe(f.pkts, rng, 1, 64, f.residues, surround, per_packet)
            assert payload.ndim == (2 if per_packet else 1)
            for i, p in enumerate(f.pkts):
                row = payload[i] if per_packet else payload
                for j, (off, d) in enumerate(p["segments"]):
                    at = int(segs[i, j]["data_off"])
                    assert at % 16 == f.residues[i][j] and segs[i, j]["offset"] == off and segs[i, j]["len"] == len(d)
                    assert row[at:at + len(d)].tobytes() == d and at + len(d) + 16 <= len(row)
            if surround in ("zeros", "ff"):
                own = sum(len(d) for p in f.pkts for _, d in p["segments"])
                fill = 0 if surround == "zeros" else 0xFF
                assert int((payload != fill).sum()) <= own
