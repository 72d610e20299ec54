"""CPU: the numpy statements of awr_detect_hands_edge (awr_amd.detect.components / hand_seeds with `edge`) against a plain
flood fill, the boundary cases of the depth test built by hand, the composition with `isolate`, and the 16 overlapping two-hand composites
the feature is for: ONE candidate each without the depth test, two or more in most of them with it."""
import numpy as np
import pytest

import edge_cases as EC
import hands_cases as HC

STATEMENT_EDGES = (0, 1, 12.5, 40, float("inf"))


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


@pytest.mark.parametrize("name", list(HC.cases()))
def test_statement_equals_a_plain_flood_fill(D, name):
    c = HC.cases()[name]
    for edge in STATEMENT_EDGES:
        got = D.components(c["frame"], c["depth_range"], c["reach"], edge)
        assert got.dtype == np.int32 and np.array_equal(got, EC.flood(c["frame"], c["depth_range"], c["reach"], edge)), (name, edge)


@pytest.mark.parametrize("name", list(EC.cases()))
def test_new_cases_equal_a_plain_flood_fill(D, name):
    c = EC.cases()[name]
    assert np.array_equal(EC.reference(name)[0], EC.flood(c["frame"], c["depth_range"], c["reach"], c["edge"]))


@pytest.mark.parametrize("name", list(HC.cases()) + list(HC.full_cases()))
def test_no_edge_and_a_wide_edge_are_todays_labels(D, name):
    c = HC.cases()[name] if name in HC.cases() else HC.full_cases()[name]
    today = HC.reference(name)[0]
    for edge in (None, 65535, 65535.5, 70000, float("inf")):
        assert np.array_equal(D.components(c["frame"], c["depth_range"], c["reach"], edge=edge), today), (name, edge)
    if name == "six_candidates":
        for edge in (None, float("inf")):
            got = D.hand_seeds(c["frame"], 4, edge=edge, **HC.knobs(c))
            assert all(HC.same(g, w) for g, w in zip(got, HC.reference(name)[1:]))


def n_components(labels):
    return int(np.unique(labels[labels >= 0]).size)


def test_the_boundary_of_the_depth_test(D):
    """a step of exactly edge joins, edge + 1 does not; 12.5 behaves as 12; 0 joins equal depths only"""
    two = lambda gap: np.array([[700, 700 + gap], [700, 700 + gap]], np.uint16)
    for edge, joins, splits in ((40, 40, 41), (12.5, 12, 13), (12, 12, 13), (0, 0, 1), (0.999, 0, 1), (1, 1, 2)):
        assert n_components(D.components(two(joins), edge=edge)) == 1, (edge, joins)
        lab = D.components(two(splits), edge=edge)
        assert n_components(lab) == 2 and lab.tolist() == [[0, 1], [0, 1]], (edge, splits)
    # the same vertically, and the far side of the step may be the smaller index
    assert D.components(two(13).T.copy(), edge=12.5).tolist() == [[0, 0], [2, 2]]
    assert D.components(np.array([[713, 700]], np.uint16), edge=12.5).tolist() == [[0, 1]]
    # depth 0 and pixels past the reach stay off the mask and join nothing
    assert D.components(np.array([[700, 0, 700, 1001, 700]], np.uint16), edge=1000).tolist() == [[0, -1, 2, -1, 4]]
    for name in EC.cases():
        if "_step_" in name:
            assert EC.reference(name)[4] == (1 if "_exact_" in name else 2), name


def test_a_ramp_is_one_component(D):
    """the transitive closure: 10 mm a pixel with edge = 10 is one component whose ends are 200 mm apart"""
    f = (700 + 10 * np.arange(21, dtype=np.uint16))[None].repeat(3, 0)
    assert int(f[0, -1]) - int(f[0, 0]) == 200
    assert (D.components(f, edge=10) == 0).all() and n_components(D.components(f, edge=9.9)) == 21
    for shape in EC.SMALL:
        tag = "%dx%d_" % shape
        lab = EC.reference(tag + "staircase")[0]
        assert n_components(lab) == 1 and (lab[10:21] == 10 * shape[1]).all() and EC.reference(tag + "staircase_cut")[4] == shape[1]
        assert EC.reference(tag + "serpentine_ramp_e1")[4] == 1 and n_components(EC.reference(tag + "serpentine_ramp_e0")[0]) == shape[0]
        lab = EC.reference(tag + "two_depth_checker")[0]
        assert np.array_equal(lab, np.arange(lab.size, dtype=np.int32).reshape(lab.shape))          # every pixel is its own root
        c = EC.cases()[tag + "smooth_field"]
        d = c["frame"].astype(np.int64)
        passing = np.concatenate([(np.abs(d[1:] - d[:-1]) <= c["edge"]).ravel(), (np.abs(d[:, 1:] - d[:, :-1]) <= c["edge"]).ravel()])
        assert 0.4 < passing.mean() < 0.7 and (d <= HC.NEAR + 300).all()


def test_rear_rectangle_crossed_by_a_nearer_bar(D):
    """three components: the bar, and the rectangle's halves above and below it; hand_seeds orders them by depth, then by root"""
    f = EC.occlusion((40, 60), 20, 30)
    assert n_components(D.components(f)) == 1
    lab = D.components(f, edge=40)
    bar, top, bottom = 18 * 60 + 6, 12 * 60 + 16, 22 * 60 + 16
    assert n_components(lab) == 3 and (lab[18:22, 6:60] == bar).all() and (lab[12:18, 16:46] == top).all() and (lab[22:30, 16:46] == bottom).all()
    c, s, info, n = D.hand_seeds(f, 4, min_pixels=20, edge=40)
    assert n == 3 and s.tolist() == [0, 0, 0, 1]
    assert info.tolist() == [[6, 18, 4 * 54, 700], [16, 12, 6 * 30, 850], [16, 22, 8 * 30, 850], [-1, -1, 0, 0]]
    assert c[0].tolist() == [6 + 53 / 2.0, 19.5, 700.0] and c[1].tolist() == [16 + 29 / 2.0, 14.5, 850.0] and c[2].tolist() == [30.5, 25.5, 850.0]
    # a smaller K keeps the first slots and the count; a larger min_pixels drops the small half but not the order
    c2, s2, info2, n2 = D.hand_seeds(f, 2, min_pixels=20, edge=40)
    assert n2 == 3 and HC.same(c2, c[:2]) and HC.same(info2, info[:2])
    assert D.hand_seeds(f, 4, min_pixels=200, edge=40)[2][:, 2].tolist() == [216, 240, 0, 0]
    for shape in EC.SMALL:
        assert EC.reference("%dx%d_occlusion" % shape)[4] == 3


def test_edge_and_isolate_compose(D):
    """a slot's frame keeps its own component; the other hand AND the fragments that are not the slot's root are zeroed"""
    f = EC.occlusion((40, 60), 20, 30)
    lab = D.components(f, edge=40)
    _, _, info, _ = D.hand_seeds(f, 3, min_pixels=20, edge=40)
    roots = (info[:, 1] * 60 + info[:, 0]).astype(np.int32)
    out = D.isolate(f, lab, roots)
    for k in range(3):
        assert np.array_equal(out[k], np.where(lab == roots[k], f, 0))
    assert (out[1][22:30] == 0).all() and (out[2][12:18] == 0).all() and (out[1] == 700).sum() == 0 and (out[0] == 850).sum() == 0
    # without the depth test the one component is everybody's frame
    lab0 = D.components(f)
    assert np.array_equal(D.isolate(f, lab0, np.array([int(lab0.max())], np.int32))[0], f)


def test_overlapping_composites(D):
    """the 16 composites: ONE candidate each today; with edge = 40 at least two in at least 12 of them, and the listed eight have exactly two,
    the nearer hand (a, placed at 700 mm) first"""
    fa, fb, both = EC.overlap_host()
    assert both.shape == (16, 480, 640)
    overlap = ((fa > 0) & (fb > 0)).reshape(16, -1).sum(1)
    assert overlap.min() > 0
    assert [EC.overlap_reference(i, None)[4] for i in range(16)] == [1] * 16
    counts = [EC.overlap_reference(i, EC.OVER_EDGE)[4] for i in range(16)]
    print("overlap pixels", overlap.tolist(), "candidates at edge 40", counts)
    assert sum(n >= 2 for n in counts) >= 12
    assert all(counts[i] == 2 for i in EC.EXACTLY_TWO)
    for i in EC.EXACTLY_TWO:
        lab, c, s, info, n = EC.overlap_reference(i, EC.OVER_EDGE)
        assert s.tolist() == [0, 0, 1, 1] and info[0, 3] < info[1, 3]
        # a pixel belongs to the hand whose own frame is nearer there: the majority owner of slot 0's component is hand a, of slot 1's
        # hand b, and slot 0's nearest depth is hand a's
        own_a = (fa[i] > 0) & ((fb[i] == 0) | (fa[i] <= fb[i]))
        for k, own in ((0, own_a), (1, (both[i] > 0) & ~own_a)):
            mine = lab == info[k, 1] * 640 + info[k, 0]
            assert mine.sum() == info[k, 2] and 2 * (mine & own).sum() > mine.sum(), (i, k)
        assert info[0, 3] == fa[i][fa[i] > 0].min()


def test_bad_edges_raise(D):
    f = np.full((4, 4), 700, np.uint16)
    for edge, exc in ((-1, ValueError), (-0.5, ValueError), (float("nan"), ValueError), (float("-inf"), ValueError), ("40", TypeError),
                      (True, TypeError), (b"4", TypeError), ([40], TypeError)):
        with pytest.raises(exc, match="edge"):
            D.components(f, edge=edge)
        with pytest.raises(exc, match="edge"):
            D.hand_seeds(f, 2, edge=edge)
    assert D.components(f, edge=np.float32(3)).max() == 0 and D.components(f, edge=np.int64(3)).max() == 0


def test_bad_edges_raise_in_hands_device_and_the_predictor_without_a_gpu(D):
    """the type is checked in Python, the value by the entry point before it looks at a pointer or launches anything"""
    import awr_amd
    from awr_amd import _lib as L
    for edge in ("40", True):
        with pytest.raises(TypeError, match="edge"):
            D.hands_device(None, [0], 2, edge=edge)
    entry = lambda edge: L.lib.awr_detect_hands_edge(None, 0, 1, 8, 8, None, 1, 2, 1.0, 2000.0, 300.0, edge, 150.0, 400, None, None, None, None,
                                                     None, None, None)
    for edge in (-1.0, -1e-300, float("nan"), float("-inf")):
        assert entry(edge) == -1 and "awr_detect_hands_edge: edge" in L.last_error(), (edge, L.last_error())
    for edge in (0.0, 40.0, float("inf")):
        assert entry(edge) == -1 and "NULL pointer" in L.last_error(), (edge, L.last_error())
    assert L.lib.awr_detect_hands(None, 0, 1, 8, 8, None, 1, 2, 1.0, 2000.0, 300.0, 150.0, 400, None, None, None, None, None, None, None) == -1
    assert L.last_error() == "awr_detect_hands: NULL pointer"
    for edge, exc in ((-1, ValueError), (float("nan"), ValueError), ("40", TypeError), (True, TypeError)):
        with pytest.raises(exc, match="edge"):
            awr_amd.Predictor(None, 64, 1.0, hands=2, edge_mm=edge)
    with pytest.raises(ValueError, match="edge_mm"):
        awr_amd.Predictor(None, 64, 1.0, edge_mm=40)
    with pytest.raises(ValueError, match="edge_mm"):
        awr_amd.Predictor(None, 64, 1.0, hands=1, edge_mm=40.0)


def test_predict_py_takes_edge_mm():
    import predict
    a = predict.parse_args(["frames.npy", "--load-model", "x.pth", "--hands", "2", "--edge-mm", "40"])
    assert a.edge_mm == 40.0 and a.hands == 2
    assert predict.parse_args(["frames.npy", "--load-model", "x.pth"]).edge_mm is None
