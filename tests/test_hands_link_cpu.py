"""CPU: the numpy statements of awr_detect_hands_link (awr_amd.detect.components / hand_seeds with `edge`, `link`, `gap`)
against a literal reference -- an explicit edge list from a per-pixel walk and a breadth-first search --, the boundary cases of the walk
built by hand, the 16 overlapping two-hand composites the feature is for, the composition with `isolate`, the refusals and the marshalling
of the new entry point."""
import ctypes as C

import numpy as np
import pytest

import edge_cases as EC
import hands_cases as HC
import link_cases as LC

INF = float("inf")
COUNTS = [2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 2, 2, 2, 2, 2, 2]          # the candidates of the 16 composites at edge 40, link 40, gap 32


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def flood_of(c, **over):
    k = dict(LC.knobs(c), **over)
    return LC.flood_linked(c["frame"], k["depth_range"], k["reach"], k["edge"], k["link"], k["gap"])


@pytest.mark.parametrize("name", list(LC.cases()))
def test_new_cases_equal_the_literal_reference(D, name):
    got = LC.reference(name)[0]
    assert got.dtype == np.int32 and np.array_equal(got, flood_of(LC.cases()[name])), name


@pytest.mark.parametrize("name", list(HC.cases()))
def test_statement_equals_the_literal_reference_on_the_hands_suite(D, name):
    c = HC.cases()[name]
    for edge, link, gap in LC.TRIPLES:
        want = LC.flood_linked(c["frame"], c["depth_range"], c["reach"], edge, link, gap)
        assert np.array_equal(LC.reference(name, (edge, link, gap))[0], want), (name, edge, link, gap)


def test_the_reference_without_a_link_is_the_plain_flood_fill():
    for name in ("33x130_random", "33x130_holes", "percolation_60"):
        c = HC.cases()[name]
        for edge in (None, 12.5):
            assert np.array_equal(LC.flood_linked(c["frame"], c["depth_range"], c["reach"], edge), EC.flood(c["frame"], c["depth_range"], c["reach"], edge))


@pytest.mark.parametrize("name", list(HC.cases()) + list(LC.cases()))
def test_no_link_and_a_wide_edge_are_the_parents_labels(D, name):
    c = HC.cases()[name] if name in HC.cases() else LC.cases()[name]
    args = (c["frame"], c["depth_range"], c["reach"])
    for edge in (0, 40):
        assert np.array_equal(D.components(*args, edge=edge, link=None, gap=7), D.components(*args, edge=edge)), (name, edge)
    today = D.components(*args)
    for edge in (65535, 65535.5, 1e9, INF):
        for link, gap in ((0, 1), (40, 32), (INF, 64)):
            assert np.array_equal(D.components(*args, edge=edge, link=link, gap=gap), today), (name, edge, link, gap)


def labels_of(name):
    return LC.reference(name)[0]


def test_the_gap_boundary_by_hand(D):
    """a bar 4 pixels thick: gap = 4 joins the halves, gap = 3 leaves three components; rows and columns, across a tile border"""
    for shape in LC.SMALL:
        tag = "%dx%d_" % shape
        cv, cu = LC.center(shape)
        for way in "hv":
            joined, split = labels_of(tag + "gap4_joins_" + way), labels_of(tag + "gap3_splits_" + way)
            assert LC.n_components(joined) == 2 and LC.n_components(split) == 3, (shape, way)
            a, b = ((cv - 3, cu), (cv + 2, cu)) if way == "h" else ((cv, cu - 3), (cv, cu + 2))          # the pixels on both sides of the bar
            assert joined[a] == joined[b] >= 0 and split[a] != split[b] and joined[cv, cu] not in (-1, joined[a])
            assert split[a] >= 0 and split[b] >= 0
    # the smallest frames that hold the rule: p, n occluders, q
    row = lambda n: np.array([[850] + [700] * n + [850]], np.uint16)          # noqa: E731
    assert D.components(row(4), edge=40, link=40, gap=4).tolist() == [[0, 1, 1, 1, 1, 0]]
    assert D.components(row(4), edge=40, link=40, gap=3).tolist() == [[0, 1, 1, 1, 1, 5]]
    assert D.components(row(1), edge=40, link=0, gap=1).tolist() == [[0, 1, 0]]
    assert D.components(row(64), edge=40, link=40, gap=64)[0, -1] == 0 and D.components(row(65), edge=40, link=40, gap=64)[0, -1] == 66
    assert D.components(row(3).T.copy(), edge=40, link=40, gap=3).ravel().tolist() == [0, 1, 1, 1, 0]
    assert D.components(row(0), edge=40, link=40, gap=4).tolist() == [[0, 0]]
    for name, n in (("33x130_bar64_gap64", 2), ("33x130_bar64_gap63", 3), ("33x130_bar65_gap64", 3)):
        assert LC.n_components(labels_of(name)) == n, name


def test_the_depth_agreement_boundary_by_hand(D):
    """halves at rear and rear + floor(link) join, + 1 more do not: 12.5 behaves as 12, 0 joins equal depths only"""
    for shape in LC.SMALL:
        for way in "hv":
            for link in (40, 12.5, 0):
                tag = "%dx%d_agree_%%s_%s_l%g" % (shape + (way, link))
                assert LC.n_components(labels_of(tag % "exact")) == 2 and LC.n_components(labels_of(tag % "plus1")) == 3, (shape, way, link)
    pair = lambda k: np.array([[850, 700, 850 + k]], np.uint16)          # noqa: E731
    for link, joins, splits in ((40, 40, 41), (12.5, 12, 13), (12, 12, 13), (0, 0, 1), (0.999, 0, 1), (INF, 150, None)):
        assert D.components(pair(joins), edge=40, link=link, gap=1).tolist() == [[0, 1, 0]], (link, joins)
        assert D.components(pair(joins)[:, ::-1].copy(), edge=40, link=link, gap=1).tolist() == [[0, 1, 0]], (link, joins)
        if splits is not None:
            assert D.components(pair(splits), edge=40, link=link, gap=1).tolist() == [[0, 1, 2]], (link, splits)


def test_the_occluder_boundary_by_hand(D):
    """a bar floor(edge) + 1 nearer is an occluder; one floor(edge) nearer is none, and a neighbour by the depth test of 4.29; a pixel
    FARTHER than p between the two ends the walk"""
    for shape in LC.SMALL:
        tag = "%dx%d_" % shape
        cv, cu = LC.center(shape)
        for edge in (40, 12.5):
            assert LC.n_components(labels_of(tag + "occluder_plus1_e%g" % edge)) == 2
            assert LC.n_components(labels_of(tag + "occluder_exact_e%g" % edge)) == 1
        lab = labels_of(tag + "farther_between")
        assert lab[cv - 3, cu] != lab[cv + 2, cu] and min(lab[cv - 3, cu], lab[cv + 2, cu], lab[cv - 1, cu]) >= 0 and LC.n_components(lab) == 5
    for edge, occ, none in ((40, 41, 40), (12.5, 13, 12), (0, 1, 0)):
        assert D.components(np.array([[850, 850 - occ, 850]], np.uint16), edge=edge, link=0, gap=1).tolist() == [[0, 1, 0]]
        assert D.components(np.array([[850, 0, 850]], np.uint16), edge=edge, link=0, gap=1).tolist() == [[0, -1, 2]]
    assert D.components(np.array([[850, 809, 0, 850]], np.uint16), edge=40, link=40, gap=8).tolist() == [[0, 1, -1, 3]]          # a zero pixel ends the walk
    assert D.components(np.array([[850, 809, 900, 850]], np.uint16), edge=40, link=40, gap=8).tolist() == [[0, 1, 2, 3]]         # so does a farther one
    assert D.components(np.array([[850, 809, 900, 850]], np.uint16), edge=40, link=50, gap=8).tolist() == [[0, 1, 0, 3]]         # ... which may be linked itself
    # the occluder need not be in the mask: nearer than zmin it is unlabelled and still bridged
    assert D.components(np.array([[850, 300, 850]], np.uint16), depth_range=(500.0, 2000.0), edge=40, link=0, gap=1).tolist() == [[0, -1, 0]]
    for shape in LC.SMALL:
        cv, cu = LC.center(shape)
        lab = labels_of("%dx%d_bar_nearer_than_zmin" % shape)
        assert LC.n_components(lab) == 1 and lab[cv, cu] == -1 and lab[cv - 3, cu] == lab[cv + 2, cu] >= 0


def test_the_one_sided_pair_by_hand(D):
    """p = 850, bar = 800, q = 830, edge = 40: the bar occludes p alone, p's walk links p and q; q joins the bar by the rule of 4.29"""
    assert D.components(np.array([[850, 800, 830]], np.uint16), edge=40).tolist() == [[0, 1, 1]]
    assert D.components(np.array([[850, 800, 830]], np.uint16), edge=40, link=40, gap=1).tolist() == [[0, 0, 0]]
    assert D.components(np.array([[830, 800, 850]], np.uint16), edge=40, link=40, gap=1).tolist() == [[0, 0, 0]]
    assert D.components(np.array([[850, 800, 830]], np.uint16), edge=40, link=19, gap=1).tolist() == [[0, 1, 1]]
    for shape in LC.SMALL:
        c = LC.cases()["%dx%d_one_sided" % shape]
        assert LC.n_components(D.components(c["frame"], edge=40)) == 2 and LC.n_components(labels_of(c["name"])) == 1


def test_breaks_by_hand(D):
    for shape in LC.SMALL:
        tag = "%dx%d_" % shape
        cv, cu = LC.center(shape)
        # a zero pixel in the bar breaks its own column's links only: the wide rectangle stays joined, the one-column one does not
        assert LC.n_components(labels_of(tag + "zero_hole")) == 2
        assert LC.n_components(labels_of(tag + "one_column")) == 2 and LC.n_components(labels_of(tag + "one_column_zero_hole")) == 3
        # the walk leaves the frame: no link, whatever the gap
        for name in ("border_ring", "border_ring_gap64"):
            c = LC.cases()[tag + name]
            assert np.array_equal(labels_of(tag + name), D.components(c["frame"], edge=40)) and LC.n_components(labels_of(tag + name)) == 2
        # a half beyond dmin + reach is unlabelled and never linked; one at dmin + reach exactly is
        lab = labels_of(tag + "half_beyond_reach")
        assert (lab[cv + 2:cv + 10] == -1).all() and LC.n_components(lab) == 2
        lab = labels_of(tag + "half_at_reach")
        assert lab[cv + 2, cu] == lab[cv - 3, cu] >= 0 and LC.n_components(lab) == 2
    assert D.components(np.array([[700, 700, 850, 700, 700]], np.uint16), edge=40, link=40, gap=2).tolist() == [[0, 0, 2, 3, 3]]
    assert D.components(np.array([[850, 700, 700]], np.uint16), edge=40, link=40, gap=2).tolist() == [[0, 1, 1]]


def test_a_chain_is_one_component_under_its_smallest_index(D):
    for shape in LC.SMALL:
        tag = "%dx%d_" % shape
        lab, fw = labels_of(tag + "chain"), shape[1]
        root = 8 * fw + 38                                          # piece C's first pixel; A and B reach it only through links
        assert (lab[10:21, 10:20] == root).all() and (lab[10:21, 24:34] == root).all() and (lab[8:21, 38:48] == root).all()
        assert LC.n_components(lab) == 3 and lab[6, 20] == 6 * fw + 20 and lab[6, 34] == 6 * fw + 34
        assert LC.n_components(labels_of(tag + "chain_gap3")) == 5


def test_fragments_below_min_pixels_count_together(D):
    for shape in LC.SMALL:
        c = LC.cases()["%dx%d_fragments_below_min_pixels" % shape]
        k = HC.knobs(c)
        assert D.hand_seeds(c["frame"], 4, edge=40, **k)[3] == 0
        _, centers, status, info, count = LC.reference(c["name"])
        cv, cu = LC.center(shape)
        assert count == 1 and status.tolist() == [0, 1, 1, 1] and info[0].tolist() == [cu - 14, cv - 8, 6 * 30 + 8 * 30, 850]
        assert centers[0].tolist() == [cu - 14 + 29 / 2.0, (6 * 30 * (cv - 5.5) + 8 * 30 * (cv + 5.5)) / 420.0, 850.0]


def test_the_noise_cases_link_something(D):
    for shape in LC.SMALL:
        tag = "%dx%d_smooth_field_gap" % shape
        c = LC.cases()[tag + "1"]
        plain = LC.n_components(D.components(c["frame"], edge=c["edge"]))
        n = [LC.n_components(labels_of(tag + g)) for g in ("1", "5", "64")]
        print(shape, "components at the median step", plain, "with links at gap 1, 5, 64:", n)
        assert plain >= n[0] >= n[1] >= n[2] >= 1 and plain > n[2]          # (a larger gap only adds links)


def owners(i):
    """a pixel's owner is the hand whose own frame is nearer there: -> (own_a, own_b)"""
    fa, fb, both = EC.overlap_host()
    own_a = (fa[i] > 0) & ((fb[i] == 0) | (fa[i] <= fb[i]))
    return own_a, (both[i] > 0) & ~own_a


def test_overlapping_composites(D):
    """the 16 composites at edge 40: the rear hand's fragments are extra candidates in three of them; link 40, gap 32 leaves two (composite 9,
    whose hands touch in depth, stays merged).  A condition: where the edge alone gave exactly two candidates the link leaves exactly two,
    and no component that links joined holds pixels of both hands"""
    before = [EC.overlap_reference(i, EC.OVER_EDGE)[4] for i in range(16)]
    after = [LC.overlap_reference(i)[4] for i in range(16)]
    print("candidates at edge 40", before, "with link 40, gap 32", after)
    assert before == [2, 2, 2, 3, 2, 2, 2, 2, 2, 1, 2, 3, 2, 3, 2, 2]
    assert after == COUNTS
    for i in range(16):
        lab0, lab = EC.overlap_reference(i, EC.OVER_EDGE)[0], LC.overlap_reference(i)[0]
        assert np.array_equal(lab >= 0, lab0 >= 0) and (lab <= lab0).all()          # the same mask; links only merge
        if after[i] != 2:
            continue
        own_a, own_b = owners(i)
        parts = {}
        for r0, r in set(zip(lab0[lab0 >= 0].tolist(), lab[lab0 >= 0].tolist())):
            parts.setdefault(r, set()).add(r0)
        linked = [r for r, p in parts.items() if len(p) > 1]
        for r in linked:
            mine = lab == r
            assert not ((mine & own_a).any() and (mine & own_b).any()), (i, r)
        if i in EC.EXACTLY_TWO:
            assert before[i] == 2
        # the rear slot holds more of the rear hand than before, and nothing of the front one
        info0, info = EC.overlap_reference(i, EC.OVER_EDGE)[3], LC.overlap_reference(i)[3]
        rear0, rear = lab0 == info0[1, 1] * 640 + info0[1, 0], lab == info[1, 1] * 640 + info[1, 0]
        assert (rear & own_b).sum() >= (rear0 & own_b).sum() and not (rear & own_a).any(), i
    assert all(after[i] == 2 for i in EC.EXACTLY_TWO)


def test_link_and_isolate_compose_on_composite_13(D):
    """three candidates without the link -- the front hand and two pieces of the rear one, of which isolate keeps ONE in the rear hand's
    frame -- and two with it: the rear slot's frame keeps both pieces"""
    frame = EC.overlap_host()[2][13]
    lab0, _, _, info0, n0 = EC.overlap_reference(13, EC.OVER_EDGE)
    lab, _, _, info, n = LC.overlap_reference(13)
    assert (n0, n) == (3, 2)
    roots0, roots = (info0[:, 1] * 640 + info0[:, 0]).astype(np.int32), (info[:, 1] * 640 + info[:, 0]).astype(np.int32)
    assert roots[0] == roots0[0] and roots[1] == min(roots0[1], roots0[2]) and info[1, 2] >= info0[1, 2] + info0[2, 2]
    out0, out = D.isolate(frame, lab0, roots0[:3]), D.isolate(frame, lab, roots[:2])
    pieces = (lab0 == roots0[1]) | (lab0 == roots0[2])
    assert np.array_equal(out[1][pieces], frame[pieces]) and (frame[pieces] > 0).all()
    assert (out0[1][lab0 == roots0[2]] == 0).all() and (out0[2][lab0 == roots0[1]] == 0).all()          # what the link repairs
    assert (out[1][lab == roots[0]] == 0).all() and (lab[lab0 == roots0[0]] == roots[0]).all()          # the front hand stays out of it, whole


def test_bad_links_raise_in_the_statement(D):
    f = np.full((4, 4), 700, np.uint16)
    for fn in (lambda **k: D.components(f, **k), lambda **k: D.hand_seeds(f, 2, **k)):
        for link, exc in ((-1, ValueError), (-0.5, ValueError), (float("nan"), ValueError), (-INF, ValueError), ("40", TypeError), (True, TypeError),
                          ([40], TypeError)):
            with pytest.raises(exc, match="link"):
                fn(edge=40, link=link)
        for gap, exc in ((0, ValueError), (65, ValueError), (-3, ValueError), (2.0, TypeError), (True, TypeError), ("4", TypeError), (None, TypeError)):
            with pytest.raises(exc, match="gap"):
                fn(edge=40, link=40, gap=gap)
        with pytest.raises(ValueError, match="link.*needs an edge"):
            fn(link=40)
        with pytest.raises(ValueError, match="edge"):
            fn(edge=-1, link=40)
        assert fn(edge=40, link=None, gap="not looked at") is not None
    assert D.LINK_GAP == 32 and D.MAX_GAP == 64
    assert D.components(f, edge=np.float32(3), link=np.float32(3), gap=np.int64(64)).max() == 0 and D.components(f, edge=1, link=INF, gap=1).max() == 0


def test_bad_links_raise_in_hands_device_the_entry_point_and_the_predictor_without_a_gpu(D):
    """types (and a link without an edge) are refused in Python, values by the entry point before it looks at a pointer or launches anything"""
    import awr_amd
    from awr_amd import _lib as L
    for kw in (dict(link="40"), dict(link=True), dict(link=40, gap=2.0), dict(link=40, gap=True)):
        with pytest.raises(TypeError, match="link|gap"):
            D.hands_device(None, [0], 2, edge=40, **kw)
    with pytest.raises(ValueError, match="link.*needs an edge"):
        D.hands_device(None, [0], 2, link=40)
    assert list(L.lib.awr_detect_hands_link.argtypes)[11:14] == [C.c_double, C.c_double, C.c_int]
    entry = lambda edge, link, gap: L.lib.awr_detect_hands_link(None, 0, 1, 8, 8, None, 1, 2, 1.0, 2000.0, 300.0, edge, link, gap, 150.0, 400, None,      # noqa: E731
                                                                None, None, None, None, None, None)
    for link in (-1.0, -1e-300, float("nan"), -INF):
        assert entry(40.0, link, 32) == -1 and "awr_detect_hands_link: link" in L.last_error(), (link, L.last_error())
    for gap in (0, -1, 65, 1 << 20):
        assert entry(40.0, 40.0, gap) == -1 and "awr_detect_hands_link: gap" in L.last_error(), (gap, L.last_error())
    for edge in (-1.0, float("nan"), -INF):
        assert entry(edge, 40.0, 32) == -1 and "awr_detect_hands_link: edge" in L.last_error(), (edge, L.last_error())
    for edge, link, gap in ((0.0, 0.0, 1), (40.0, 40.0, 32), (INF, INF, 64)):
        assert entry(edge, link, gap) == -1 and L.last_error() == "awr_detect_hands_link: NULL pointer", (edge, link, gap, L.last_error())
    for kw, exc in ((dict(link_mm=-1), ValueError), (dict(link_mm=float("nan")), ValueError), (dict(link_mm="40"), TypeError), (dict(link_mm=True), TypeError),
                    (dict(link_mm=40, link_gap=0), ValueError), (dict(link_mm=40, link_gap=65), ValueError), (dict(link_mm=40, link_gap=2.5), TypeError)):
        with pytest.raises(exc, match="link|gap"):
            awr_amd.Predictor(None, 64, 1.0, hands=2, edge_mm=40, **kw)
    with pytest.raises(ValueError, match="link_mm"):
        awr_amd.Predictor(None, 64, 1.0, hands=2, link_mm=40)               # no edge_mm
    with pytest.raises(ValueError, match="link_mm"):
        awr_amd.Predictor(None, 64, 1.0, link_mm=40)                        # hands = 1
    with pytest.raises(ValueError, match="edge_mm|link_mm"):
        awr_amd.Predictor(None, 64, 1.0, hands=1, edge_mm=40, link_mm=40)


def test_the_predictors_new_parameters_stand_in_front_of_surface():
    import inspect

    import awr_amd
    names = list(inspect.signature(awr_amd.Predictor.__init__).parameters)
    assert names[-3:] == ["link_mm", "link_gap", "surface"]
    p = inspect.signature(awr_amd.Predictor.__init__).parameters
    assert p["link_mm"].default is None and p["link_gap"].default == 32


def test_detect_calls_issues_one_call_of_the_new_name(monkeypatch):
    import awr_amd  # noqa: F401
    from awr_amd import _lib as L, detect_calls as DC
    recorded = []
    monkeypatch.setattr(L, "call", lambda name, *args: recorded.append((name, args)))
    monkeypatch.setattr(L, "stream", lambda: 0x5000)
    p = lambda i: 0x10000 + 256 * i          # noqa: E731
    args = (0x1000, 0, 6, 120, 160, p(0), 2, 2, (200, 1200.0), 300, 40, 100, 400, p(1), p(6), p(2), p(3), p(4), p(5))
    DC.awr_detect_hands(*args, link=40, gap=32)
    assert len(recorded) == 1 and recorded[0][0] == "awr_detect_hands_link"
    sent, proto = recorded.pop()[1], L._SIGS["awr_detect_hands_link"][0]
    assert len(sent) == len(proto) == 23 and sent[-1] == 0x5000
    for i, (x, t) in enumerate(zip(sent, proto)):
        if t is C.c_void_p:
            assert x is None or type(x) is int, (i, x)
        elif t in (C.c_int, C.c_int64):
            assert type(x) is int, (i, x)
        else:
            assert t is C.c_double and type(x) is float, (i, t, x)
    assert sent[8:16] == (200.0, 1200.0, 300.0, 40.0, 40.0, 32, 100.0, 400) and sent[16:22] == (p(1), p(6), p(2), p(3), p(4), p(5))
    # the default gap, and the calls without a link are the parent's
    DC.awr_detect_hands(*args, link=12.5)
    assert recorded.pop()[1][12:14] == (12.5, 32)
    DC.awr_detect_hands(*args)
    DC.awr_detect_hands(*args, link=None, gap=7)
    DC.awr_detect_hands(*(args[:10] + (None,) + args[11:]), link=None, gap=32)
    assert [r[0] for r in recorded] == ["awr_detect_hands_edge", "awr_detect_hands_edge", "awr_detect_hands"]
    assert recorded[0] == recorded[1] and len(recorded[0][1]) == 21 and len(recorded[2][1]) == 20


def test_predict_py_takes_link_mm():
    import predict
    a = predict.parse_args(["frames.npy", "--load-model", "x.pth", "--hands", "2", "--edge-mm", "40", "--link-mm", "40", "--link-gap", "16"])
    assert a.link_mm == 40.0 and a.link_gap == 16 and a.edge_mm == 40.0
    a = predict.parse_args(["frames.npy", "--load-model", "x.pth", "--hands", "2", "--edge-mm", "40"])
    assert a.link_mm is None and a.link_gap is None
