"""CPU: awr_amd.detect.isolate, the numpy statement of awr_hands_isolate, against a plain per-pixel loop on the small
cases, and the preconditions of the GPU anchor test on every near-hand composite: exactly two components, each one hand's own silhouette,
every foreground pixel labelled, each palm point inside the other hand's crop cube -- so that isolate(composite)[k] IS hand k's own frame."""
import numpy as np
import pytest

import isolate_cases as IC

CUBE = 300.0


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


@pytest.mark.parametrize("name", list(IC.cases()))
def test_isolate_equals_the_pixel_loop(D, name):
    c = IC.cases()[name]
    want = IC.loop_reference(c["frame"], c["labels"], c["roots"])
    got = IC.reference(name)
    assert got.dtype == np.uint16 and got.shape == (4,) + c["frame"].shape and np.array_equal(got, want)
    for K in IC.KS:
        assert np.array_equal(D.isolate(c["frame"], c["labels"], c["roots"][:K]), want[:K])


def test_the_cases_are_what_they_claim(D):
    cs = IC.cases()
    shapes = {c["frame"].shape for c in cs.values()}
    assert shapes == set(IC.SHAPES) and any(h * w % 8 for h, w in shapes) and any(h * w % 8 == 0 for h, w in shapes) and any(w % 2 for h, w in shapes)
    # a root at index 0, and a slot without a component keeps the whole frame
    c = cs["two_blobs_debris"]
    assert c["roots"].tolist()[:3] == [0, 10 * 130 + 70, -1] and c["labels"][0, 0] == 0
    out = IC.reference("two_blobs_debris")
    a, b = c["labels"] == c["roots"][0], c["labels"] == c["roots"][1]
    debris = (c["labels"] >= 0) & ~a & ~b
    assert a.sum() == 14 * 30 and b.sum() == 20 * 50 and debris.sum() > 20
    # each hand alone, the debris in NEITHER frame; the EMPTY slot the unchanged frame
    assert np.array_equal(out[0], np.where(a, c["frame"], 0)) and np.array_equal(out[1], np.where(b, c["frame"], 0))
    assert np.array_equal(out[2], c["frame"]) and np.array_equal(out[3], out[0])
    # a root that is nobody's: every labelled pixel goes
    assert not IC.reference("two_blobs_debris_swapped")[3].any()
    # the hole stays a hole, and the far pixel inside it -- unlabelled -- stays in both frames
    c, out = cs["hole_in_a_hand"], IC.reference("hole_in_a_hand")
    assert c["labels"][16, 30] == -1 and out[0][16, 30] == 1001 and out[1][16, 30] == 1001 and out[0][16, 33] == 0 and c["frame"][16, 33] == 0
    assert (out[0][4:28, 80:110] == 0).all() and (out[1][4:28, 80:110] == 800).all() and out[0][16, 20] == 700 and out[1][16, 20] == 0
    # at dmin + reach: labelled; one millimetre beyond, and beyond zmax: unlabelled, in every output
    c, out = cs["beyond_the_reach_survives"], IC.reference("beyond_the_reach_survives")
    lab = c["labels"]
    assert (lab[10:20, 24:40] == 10 * 64 + 24).all() and (lab[10:20, 40:60] == -1).all() and (lab[30:40, 5:15] == -1).all() and (lab[42:46, 40:50] == -1).all()
    assert c["roots"].tolist() == [10 * 64, 10 * 64 + 24, -1, -1]
    for k in range(4):
        assert (out[k][10:20, 40:60] == 1001).all() and (out[k][30:40, 5:15] == 1001).all() and (out[k][42:46, 40:50] == 2500).all()
    assert (out[0][10:20, 24:40] == 0).all() and (out[1][10:20, 0:20] == 0).all() and (out[1][10:20, 24:40] == 1000).all()
    # the checkerboard: every pixel its own component, so a slot keeps ONE pixel of the mask
    c, out = cs["17x23_checker"], IC.reference("17x23_checker")
    assert (out[0] > 0).sum() == 1 and out[0][0, 0] == c["frame"][0, 0] and (c["frame"] > 0).sum() == (17 * 23 + 1) // 2


def test_argument_errors(D):
    f = np.zeros((4, 4), np.uint16)
    lab = np.full((4, 4), -1, np.int32)
    for args in ((f, lab[:3], [0]), (f, lab.astype(np.float32), [0]), (f, lab, []), (f, lab, [0] * 5), (f, lab, [[0]]), (f, lab, [0.5]),
                 (f.astype(np.int32), lab, [0])):
        with pytest.raises(ValueError):
            D.isolate(*args)


def near_preconditions(D, fa, fb, both, palm_a, palm_b):
    """everything the GPU anchor test relies on, for one composite -> (roots (2,), a_first)"""
    from awr_amd import nyu_data as ND
    from awr_amd.evaluator import uvd2xyz
    ma, mb = fa > 0, fb > 0
    assert ma.sum() >= D.MIN_PIXELS and mb.sum() >= D.MIN_PIXELS
    # no occluded pixel and no 4-adjacent pixel between the hands
    grown = ma.copy()
    grown[1:] |= ma[:-1]
    grown[:-1] |= ma[1:]
    grown[:, 1:] |= ma[:, :-1]
    grown[:, :-1] |= ma[:, 1:]
    assert not (grown & mb).any()
    labels = D.components(both)
    roots, n = np.unique(labels[labels >= 0], return_counts=True)
    assert (n >= D.MIN_PIXELS).sum() == 2 and roots.size == 2, (roots, n)
    # every foreground pixel is labelled, and each component is one hand's own silhouette
    assert np.array_equal(labels >= 0, both > 0)
    ra, rb = int(np.flatnonzero(ma.ravel())[0]), int(np.flatnonzero(mb.ravel())[0])
    assert np.array_equal(labels == ra, ma) and np.array_equal(labels == rb, mb)
    a_first = bool(IC.near_first(fa[None], fb[None])[0])
    centers, status, info, count = D.hand_seeds(both, 2)
    assert status.tolist() == [0, 0] and count == 2
    got = (info[:, 1].astype(np.int64) * both.shape[1] + info[:, 0]).tolist()
    assert got == ([ra, rb] if a_first else [rb, ra])
    # each hand's palm point lies inside the other hand's crop cube (around the single detector's centre of that hand)
    for own, palm_other in ((fa, palm_b), (fb, palm_a)):
        c, st = D.detect(own)
        assert st == 0
        d = uvd2xyz(np.asarray(palm_other, np.float64)[None], ND.PARAS, -1)[0] - uvd2xyz(np.asarray(c, np.float64)[None], ND.PARAS, -1)[0]
        assert (np.abs(d) < CUBE / 2).all(), d
    return np.array(got, np.int32), a_first


@pytest.mark.parametrize("i", range(IC.N_NEAR))
def test_near_hand_composites_isolate_into_the_hands_own_frames(D, i):
    """the statement the anchor test rests on: isolate(composite)[k] == hand k's own frame, hands ordered by smallest depth"""
    fa, fb, both = IC.near_hands_host()
    palm_a, palm_b = IC.near_hands()[4:]
    assert both.shape == (IC.N_NEAR,) + IC.FULL and len(set(IC.NEAR_SEEDS)) == IC.N_NEAR
    roots, a_first = near_preconditions(D, fa[i], fb[i], both[i], palm_a[i], palm_b[i])
    out = D.isolate(both[i], D.components(both[i]), roots)
    want = [fa[i], fb[i]] if a_first else [fb[i], fa[i]]
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])
    assert not np.array_equal(both[i], fa[i]) and not np.array_equal(both[i], fb[i])
