"""CPU: the numpy statements of awr_detect_hands (awr_amd.detect.components / hand_seeds), synth.compose and
synth.place_poses, and the two-hand property the GPU test is anchored to: on 32 two-hand composites the component seeds, refined by the
unchanged detector, are bit for bit the single detector's centres on the single hands' frames."""
import numpy as np
import pytest

import hands_cases as HC


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


@pytest.fixture(scope="module")
def SY():
    import awr_amd  # noqa: F401
    from awr_amd import synth
    return synth


def canonical(frame, depth_range, reach):
    """scipy's labelling of the statement's mask, every label replaced by the smallest raster index of its component"""
    ndi = pytest.importorskip("scipy.ndimage")
    zmin, zmax = depth_range
    fg = (frame >= zmin) & (frame <= zmax) & (frame != 0)
    out = np.full(frame.shape, -1, np.int32)
    if not fg.any():
        return out
    mask = fg & (frame <= min(float(frame[fg].min()) + reach, zmax))
    lab, n = ndi.label(mask)                                              # (the default structure: 4-neighbours)
    first = ndi.minimum(np.arange(frame.size).reshape(frame.shape), lab, np.arange(1, n + 1))
    out[mask] = np.asarray(first, np.int64)[lab[mask] - 1]
    return out


@pytest.mark.parametrize("name", list(HC.cases()) + list(HC.full_cases()))
def test_components_equal_scipy_canonicalised(D, name):
    c = HC.cases()[name] if name in HC.cases() else HC.full_cases()[name]
    labels = HC.reference(name)[0]
    assert labels.dtype == np.int32 and labels.shape == c["frame"].shape
    assert np.array_equal(labels, canonical(c["frame"], c["depth_range"], c["reach"]))


def test_the_patterns_are_what_they_claim(D):
    n_comp = lambda name: np.unique(HC.reference(name)[0][HC.reference(name)[0] >= 0]).size
    assert n_comp("33x130_empty") == 0 and n_comp("33x130_full") == 1 and n_comp("33x130_checker") == (33 * 130 + 1) // 2
    for name in ("33x130_serpentine", "33x130_serpentine_far", "33x130_spiral", "33x130_comb", "48x64_spiral", "full_serpentine"):
        lab = HC.reference(name)[0]
        assert n_comp(name) == 1 and lab[lab >= 0].max() == 0, name                           # one component, and index 0 is its root
    assert n_comp("tile_corner") == 1 and n_comp("tile_corner_block") == 1
    assert (HC.reference("33x130_spiral")[0] >= 0).sum() > 33 * 130 // 3 and n_comp("diagonal_blobs") == 2
    assert max(np.bincount(HC.reference("percolation_60")[0][HC.reference("percolation_60")[0] >= 0])) > 200
    lab = HC.reference("reach_exact")[0]
    assert (lab[10:20, 0:40] == 10 * 64).all() and (lab[10:20, 40:] == -1).all() and (lab[30:40] == -1).all()
    assert (HC.reference("reach_fraction")[0] == lab).all()
    assert (HC.reference("reach_zero")[0] >= 0).sum() == 200
    lab = HC.reference("zmax_cut")[0]
    assert (lab[5:15, 5:45] == 5 * 64 + 5).all() and (lab[5:15, 45:] == -1).all() and (lab[20:] == -1).all()
    lab = HC.reference("zmin_cut")[0]
    assert (lab[5:15, 25:60] == 5 * 64 + 25).all() and (lab[5:15, :25] == -1).all()


def test_hand_seeds_order_ties_thresholds_and_count(D):
    c, s, info, n = HC.reference("equal_zc")[1:]
    # both components' nearest pixel is at 700: the one that starts in row 4 has the smaller root, though it is the larger one
    assert n == 2 and s.tolist() == [0, 0, 1, 1] and info[:2].tolist() == [[30, 4, 16 * 30, 700], [2, 30, 60, 700]]
    assert info[2:].tolist() == [[-1, -1, 0, 0]] * 2 and np.isnan(c[2:]).all()
    # the slab is per component: 700 ... 850 of a component that is 700 at one pixel and 760 elsewhere is all of it
    assert c[0].tolist() == [(16 * sum(range(30, 60))) / 480.0, (30 * sum(range(4, 20))) / 480.0, (700 + 479 * 760) / 480.0]
    c, s, info, n = HC.reference("min_pixels_edge")[1:]
    assert n == 2 and info[:2].tolist() == [[2, 2, 20, 720], [20, 20, 100, 800]]          # the nearer line of 19 pixels is no candidate
    c, s, info, n = HC.reference("six_candidates")[1:]
    # (the reach cuts the far blobs: 860 + 12 r <= 1000 leaves twelve rows of sixteen)
    assert n == 6 and s.tolist() == [0] * 4 and info[:, 3].tolist() == [700, 705, 760, 860] and info[:, 2].tolist() == [256, 256, 256, 192]
    # 12 mm a row: rows 0 ... 12 of a blob lie within 150 mm of its nearest row
    assert c[0].tolist() == [2 + 21 + 7.5, 4 + 6.0, 700 + 72.0]
    assert HC.reference("six_candidates_none_large")[4] == 0 and HC.reference("six_candidates_none_large")[2].tolist() == [1] * 4
    c, s, info, n = HC.reference("zmax_cut")[1:]
    assert n == 1 and info[0].tolist() == [5, 5, 400, 700] and c[0].tolist() == [14.5, 9.5, 700.0]      # the slab ends at 850: the 700s alone
    frame = HC.cases()["zmax_cut"]["frame"]
    assert D.hand_seeds(frame, 1, depth_range=(1.0, 900.0), slab=200.0)[0][0].tolist() == [24.5, 9.5, 800.0]
    assert D.hand_seeds(frame, 1, depth_range=(1.0, 900.0), slab=199.0)[0][0].tolist() == [14.5, 9.5, 700.0]
    for k in HC.KS:
        ck, sk, ik, nk = D.hand_seeds(HC.cases()["six_candidates"]["frame"], k, **HC.knobs(HC.cases()["six_candidates"]))
        assert HC.same(ck, HC.reference("six_candidates")[1][:k]) and HC.same(sk, HC.reference("six_candidates")[2][:k]) and nk == 6 and ck.shape == (k, 3) and ik.dtype == np.int32
    c, s, info, n = D.hand_seeds(np.zeros((4, 4), np.uint16), 2)
    assert n == 0 and s.tolist() == [1, 1] and np.isnan(c).all()


def test_argument_errors(D):
    f = np.zeros((4, 4), np.uint16)
    for kw, exc in ((dict(hands=0), ValueError), (dict(hands=5), ValueError), (dict(hands=True), TypeError), (dict(hands=2.0), TypeError),
                    (dict(hands=1, min_pixels=0), ValueError), (dict(hands=1, min_pixels=1.5), TypeError), (dict(hands=1, reach=-1.0), ValueError),
                    (dict(hands=1, reach=float("nan")), ValueError), (dict(hands=1, slab=-1.0), ValueError), (dict(hands=1, slab="x"), TypeError),
                    (dict(hands=1, depth_range=(5.0, 1.0)), ValueError)):
        with pytest.raises(exc):
            D.hand_seeds(f, **kw)
    with pytest.raises(ValueError):
        D.components(f.astype(np.float32))
    assert (D.MAX_HANDS, D.REACH, D.MIN_PIXELS) == (4, 300.0, 400)


def test_single_component_seed_is_the_nearest_seed(D):
    """one component and nothing else inside the slab: slot 0's seed is detect's "nearest" seed bit for bit, slot 1 is EMPTY"""
    r = np.random.RandomState(3)
    f = np.zeros((60, 80), np.uint16)
    vv, uu = np.indices(f.shape)
    blob = (vv - 30) ** 2 + (uu - 35) ** 2 < 400
    f[blob] = (650 + r.randint(0, 260, f.shape))[blob]
    f[2:5, 70:75] = 2100                                                   # outside the depth range
    want, st = D.detect(f, seed="nearest", iters=0)
    c, s, info, n = D.hand_seeds(f, 2)
    assert st == 0 and n == 1 and s.tolist() == [0, 1] and np.isnan(c[1]).all() and info[1].tolist() == [-1, -1, 0, 0]
    assert c[0].tobytes() == np.array(want, np.float64).tobytes()


def test_compose_and_place_poses(SY):
    r = np.random.RandomState(0)
    a, b, c = (np.where(r.uniform(size=(3, 7, 9)) < 0.5, r.randint(1, 65536, (3, 7, 9)), 0).astype(np.uint16) for _ in range(3))
    got = SY.compose(a, b, c)
    big = np.stack([a, b, c]).astype(np.int64)
    want = np.where(big == 0, 1 << 20, big).min(0)
    assert got.dtype == np.uint16 and np.array_equal(got, np.where(want == 1 << 20, 0, want))
    assert np.array_equal(SY.compose(a), a) and SY.compose(a) is not a
    import torch
    t = SY.compose(*(torch.from_numpy(x) for x in (a, b, c)))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint16 and np.array_equal(t.numpy(), got)
    with pytest.raises(ValueError):
        SY.compose(a, b[:, :5])
    with pytest.raises(ValueError):
        SY.compose(a, b.astype(np.int32))
    model = SY.HandModel(forearm=False)
    poses = SY.sample_poses(5, 9, model)
    u, v, z = np.array([100.0, 200.0, 300.0, 400.0, 500.0]), 240.0, np.array([600.0, 650.0, 700.0, 750.0, 800.0])
    placed = SY.place_poses(poses, u, v, z, model)
    assert set(placed) == set(poses) and all(np.array_equal(placed[k], poses[k]) and placed[k] is not poses[k] for k in poses if k != "position")
    fx, fy, u0, v0 = SY.ND.PARAS
    p = placed["position"] + SY._palm_point(placed, model)
    assert np.allclose(p[:, 0] * fx / p[:, 2] + u0, u, atol=1e-9) and np.allclose(-p[:, 1] * fy / p[:, 2] + v0, v, atol=1e-9) and np.allclose(p[:, 2], z)
    # sample_poses places its own draws by the same arithmetic: placing a pose where it already is changes nothing
    mid = poses["position"] + SY._palm_point(poses, model)
    again = SY.place_poses(poses, mid[:, 0] * fx / mid[:, 2] + u0, -mid[:, 1] * fy / mid[:, 2] + v0, mid[:, 2], model)
    assert np.allclose(again["position"], poses["position"], atol=1e-9)


def test_two_hands_every_frame(D):
    """In EVERY one of the 32 composites hand_seeds(..., 2) followed by detect(seed="given") gives two centres that equal, as float64 bits,
    detect(frame_a) and detect(frame_b), ordered by the single frames' smallest depth."""
    fa, fb, both = HC.two_hands_host()
    assert both.shape == (32, 480, 640)
    single_misses = 0
    for i in range(HC.N_TWO):
        ca, sa = D.detect(fa[i])
        cb, sb = D.detect(fb[i])
        assert sa == 0 and sb == 0
        za, zb = int(fa[i][fa[i] > 0].min()), int(fb[i][fb[i] > 0].min())
        assert za != zb
        want = [ca, cb] if za < zb else [cb, ca]
        seeds, status, info, count = D.hand_seeds(both[i], 2)
        assert status.tolist() == [0, 0] and count == 2, (i, status, count)
        got = [D.detect(both[i], seed="given", center=seeds[k]) for k in range(2)]
        for k in range(2):
            assert got[k][1] == 0 and np.array(got[k][0]).tobytes() == np.array(want[k]).tobytes(), (i, k, got[k], want[k])
        # why the components are needed: the single detector reports at most one of the two, and sometimes neither
        c1, s1 = D.detect(both[i])
        single_misses += int(s1 != 0 or not any(np.array(c1).tobytes() == np.array(w).tobytes() for w in want))
    assert single_misses > 0
