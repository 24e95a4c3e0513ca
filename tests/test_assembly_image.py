"""The whole-storage image helper (tests/assembly_image.py) checked on its own,
without a GPU: the expected image it builds is the reference placement inside
the rows and the sentinel everywhere else, in every layout the extent tests use."""
import numpy as np
import pytest

import assembly_image as ai
import rc4_ref


def _case(W, frames, d=10, p=3, G=5, first_group=2, seed=7):
    S = W - 6 if frames else W
    wire = ai.build_rx_ring(d, p, S, G, first_group, seed)
    want, masks, stats = ai.expected_placement(wire, G, d + p, S, ai.round_up(W, 16), first_group, frames)
    return wire, want, masks, stats


def test_crypt_is_the_oracles_rc4():
    w = bytes(range(256)) * 12
    assert ai.crypt(w) == rc4_ref.xor_stream(ai.KEY, w)
    assert ai.crypt(w[:7]) == rc4_ref.xor_stream(ai.KEY, w[:7])


def test_ring_holds_every_kind_of_packet():
    d, p, S, G, fg = 10, 3, 1470, 5, 2
    n = d + p
    wire = ai.build_rx_ring(d, p, S, G, fg, 3)
    _, masks, stats = ai.expected_placement(wire, G, n, S, 1472, fg)
    assert stats[0] > 0.6 * G * n and all(s > 0 for s in stats[1:])
    assert any(len(w) == S + 6 for w in wire) and any(len(w) == 6 for w in wire)
    first = {}
    longer_second = False
    for w in wire:
        if len(w) < 6:
            continue
        seq = int.from_bytes(w[:4], "little")
        if seq in first and len(w) > len(first[seq]) and w[6:len(first[seq])] != first[seq][6:]:
            longer_second = True
        first.setdefault(seq, w)
    assert longer_second
    assert any(bin(int(m)).count("1") < n for m in masks)  # unclaimed rows exist


@pytest.mark.parametrize("frames", [False, True])
def test_dense_planar_image_is_the_reference_placement(frames):
    W = 1476 if frames else 1470
    _, want, masks, _ = _case(W, frames)
    L = ai.rx_layouts(W, 13, 5)[1]
    img = ai.Image(L, device=None)
    e = img.expected(want, masks)
    assert e.size == img.base + L.extent + ai.GUARD and img.base >= ai.GUARD
    assert L.extent == 13 * 5 * L.w16  # dense: the rows are the whole extent
    rows = img.rows(e)
    for g in range(5):
        for r in range(13):
            if (int(masks[g]) >> r) & 1:
                assert np.array_equal(rows[g, r], want[g, r])
                assert not rows[g, r, W:].any()
            else:
                assert (rows[g, r] == ai.SENTINEL).all()
    assert (e[:img.base] == ai.SENTINEL).all() and (e[img.base + L.extent:] == ai.SENTINEL).all()
    # planar: row r of group g at (r*G + g) * w16
    planar = e[img.base:img.base + L.extent].reshape(13, 5, L.w16)
    assert np.array_equal(planar.transpose(1, 0, 2), rows)


@pytest.mark.parametrize("frames", [False, True])
@pytest.mark.parametrize("W", [17, 1476, 2049])
def test_padded_group_major_image_counts_only_placed_rows(W, frames):
    if not frames and W == 1476:
        W = 1470
    _, want, masks, _ = _case(W, frames)
    L = ai.rx_layouts(W, 13, 5)[4]
    assert L.row_stride == L.w16 + 16 and L.group_stride == 13 * L.row_stride + 32 and not L.planar
    img = ai.Image(L, device=None)
    # a payload byte may equal the sentinel by chance, so "sentinel" means: follows the fill value
    # when the image is built with another one
    e, e2 = img.expected(want, masks), img.expected(want, masks, sentinel=0x5A)
    untouched = (e == ai.SENTINEL) & (e2 == 0x5A)
    placed = sum(bin(int(m)).count("1") for m in masks)
    assert 0 < placed < 65
    assert int((~untouched).sum()) == placed * L.w16
    assert np.array_equal(e[~untouched], e2[~untouched])
    # and they are the placed rows' own bytes, each W bytes of the reference then zeros
    rows = img.rows(e)
    for g in range(5):
        for r in range(13):
            o = img.base + L.start(g, r)
            if (int(masks[g]) >> r) & 1:
                assert not untouched[o:o + L.w16].any()
                assert np.array_equal(rows[g, r], want[g, r])
            else:
                assert untouched[o:o + L.w16 + 16].all()  # the slot and the padding behind it


def test_decode_names_rows_slack_and_guards():
    L = ai.rx_layouts(1476, 13, 5)[2]  # 1536-B pitch, rows of 1488
    img = ai.Image(L, device=None)
    assert img.decode(0) == "guard" and img.decode(img.base - 1) == "guard"
    assert img.decode(img.base) == (0, 0, 0)
    assert img.decode(img.base + L.start(3, 7) + 100) == (3, 7, 100)
    assert img.decode(img.base + L.start(3, 7) + 1500) == (3, 7, 1500)  # the slack behind a row
    assert img.decode(img.base + L.start(4, 12) + 1487) == (4, 12, 1487)  # the batch's last byte
    assert img.decode(img.base + L.extent) == "guard"
    got, want = np.zeros(img.size, np.uint8), np.zeros(img.size, np.uint8)
    got[img.base + L.start(2, 1) + 1490] = 1
    with pytest.raises(AssertionError, match=r"\(2, 1, 1490\)"):
        ai.check_equal(got, want, img.decode, "case")
