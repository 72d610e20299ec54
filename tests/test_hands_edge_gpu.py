"""GPU: awr_detect_hands_edge (csrc/awr_hands.hip) against its numpy statements awr_amd.detect.components / hand_seeds with
`edge` -- np.array_equal (NaN positions equal) on the labels, the centres, the status, the info rows and the count of every frame -- the
unchanged path of edge=None, and awr_amd.Predictor(hands=2, edge_mm=40) on the overlapping composites against the composition of its
parts."""
import types

import numpy as np
import pytest
import torch

import edge_cases as EC
import hands_cases as HC

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORD = 1024, 0x5A5A5A5A5A5A5A5A
NAMES = ("labels", "centres", "status", "info", "count")
KS = (1, 4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def take(frames, rows):
    """rows of a uint16 device tensor (indexed through its int16 view)"""
    return frames.view(torch.int16)[torch.as_tensor(rows, device=frames.device)].view(torch.uint16)


def make_store(frames, dev):
    data = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.array(frames)).to(dev)      # (a copy: the shared inputs are read-only)
    return types.SimpleNamespace(data=data, ftype=0, fh=int(data.shape[1]), fw=int(data.shape[2]), n=int(data.shape[0]))


def run(D, dev, store, idx, K, labels=True, **knobs):
    """hands_device with a guarded scratch -> numpy (labels or None, centres, status, info, count); the guard words past the reported
    size must survive"""
    from awr_amd import _lib as L
    B = len(idx)
    nbytes = int(L.lib.awr_detect_hands_scratch(B, store.fh, store.fw))
    scratch = torch.full((nbytes // 8 + GUARD,), GUARD_WORD, dtype=torch.int64, device=dev)
    c, s, info, count, lab = D.hands_device(store, idx, K, labels=labels, scratch=scratch, **knobs)
    assert (scratch[nbytes // 8:] == GUARD_WORD).all(), "awr_detect_hands_edge wrote past awr_detect_hands_scratch(...) bytes"
    assert tuple(c.shape) == (K, B, 3) and tuple(s.shape) == (K, B) and tuple(info.shape) == (K, B, 4) and tuple(count.shape) == (B,)
    return (None if lab is None else lab.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy(), info.cpu().numpy(), count.cpu().numpy())


def assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        if g is not None:
            assert HC.same(g, w), (what, name, g, w)


def group_id(k):
    return "%dx%d_%s" % (k[0][0], k[0][1], "_".join(str(x) for x in k[1:]))


GROUPS, NEW_GROUPS = HC.groups(), EC.groups()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("edge", EC.EDGES)
@pytest.mark.parametrize("key", list(GROUPS), ids=group_id)
def test_every_case_of_the_hands_suite_with_an_edge(D, dev, key, edge, K):
    names = GROUPS[key]
    store = make_store(np.stack([HC.cases()[n]["frame"] for n in names]), dev)
    idx = np.arange(len(names))
    want = EC.batch_reference(names, idx, K, len(names), edge)
    knobs = dict(HC.knobs(HC.cases()[names[0]]), edge=edge)
    assert_equal(run(D, dev, store, idx, K, labels=True, **knobs), want, (names, edge))
    assert_equal(run(D, dev, store, idx, K, labels=False, **knobs), want, (names, edge))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("key", list(NEW_GROUPS), ids=group_id)
def test_the_new_cases(D, dev, key, K):
    """33 x 130 and 48 x 64: steps of exactly edge and edge + 1 on row 16, on column 64 and inside a tile, the staircase over three tiles,
    the two-depth checkerboard, the smooth field, the occlusion across a tile corner, the serpentine with a ramp"""
    names = NEW_GROUPS[key]
    store = make_store(np.stack([EC.cases()[n]["frame"] for n in names]), dev)
    idx = np.arange(len(names))
    want = EC.batch_reference(names, idx, K, len(names))
    knobs = EC.knobs(EC.cases()[names[0]])
    assert_equal(run(D, dev, store, idx, K, labels=True, **knobs), want, names)
    assert_equal(run(D, dev, store, idx, K, labels=False, **knobs), want, names)


# ---- 480 x 640, once ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def over(dev):
    """the 16 overlapping composites rendered on the device: -> a store over them"""
    from awr_amd import synth as SY
    prims_a, bbox_a, prims_b, bbox_b = EC.overlap_hands()
    fa = torch.empty((EC.N_OVER,) + HC.FULL, dtype=torch.uint16, device=dev)
    fb = torch.empty_like(fa)
    SY.render_device(prims_a, bbox_a, fa)
    SY.render_device(prims_b, bbox_b, fb)
    return make_store(SY.compose(fa, fb), dev)


def test_full_frames_once(D, dev, over):
    four = [0, 3, 9, 11]                                       # two, three, one and three candidates
    host = EC.overlap_host()[2]
    assert np.array_equal(take(over.data, four).cpu().numpy(), host[four])
    refs = [EC.overlap_reference(i, EC.OVER_EDGE) for i in four]
    assert [r[4] for r in refs] == [2, 3, 1, 3]
    want = EC.batch_reference(None, np.arange(4), 4, 4, ref=refs)
    got = run(D, dev, make_store(take(over.data, four), dev), np.arange(4), 4, min_pixels=EC.OVER_MIN_PIXELS, edge=EC.OVER_EDGE)
    assert_equal(got, want, four)
    # the serpentine, one corridor through all 1200 tiles, its depth one millimetre further every second row
    c = HC.full_cases()["full_serpentine"]
    want = EC.batch_reference(["full_serpentine"], [0], 4, 1, edge=1)
    assert want[4].tolist() == [1] and (want[0][0][c["frame"] > 0] == 0).all()
    assert_equal(run(D, dev, make_store(c["frame"][None], dev), np.arange(1), 4, edge=1, **HC.knobs(c)), want, "full_serpentine")


@pytest.mark.parametrize("K", KS)
def test_mixed_rows(D, dev, K):
    """bad frame indices in the middle of a batch and the same frame twice, with an edge: every row is what it is alone"""
    key = [k for k in NEW_GROUPS if k[0] == (33, 130) and k[-1] == 40 and k[-2] == 6][0]
    names = NEW_GROUPS[key]
    n = len(names)
    store = make_store(np.stack([EC.cases()[x]["frame"] for x in names]), dev)
    knobs = EC.knobs(EC.cases()[names[0]])
    for idx in ([1], [n], [1, -1, 1], [2, n, 2], [n - 1, 1, 0, 1, n + 5, 3, 1, -7, 2]):
        want = EC.batch_reference(names, idx, K, n)
        got = run(D, dev, store, np.array(idx), K, **knobs)
        assert_equal(got, want, idx)
        bad = np.array([not 0 <= i < n for i in idx])
        assert (got[2][:, bad] == D.BAD_FRAME).all() and (got[4][bad] == 0).all() and (got[0][bad] == -1).all()


def test_no_edge_is_todays_entry_and_an_infinite_edge_its_labels(D, dev, monkeypatch):
    from awr_amd import _lib as L
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    key = [k for k in GROUPS if k[0] == (33, 130) and k[1:] == ((1.0, 2000.0), 300.0, 150.0, 6)][0]
    names = GROUPS[key]
    store = make_store(np.stack([HC.cases()[n]["frame"] for n in names]), dev)
    idx = np.arange(len(names))
    knobs = HC.knobs(HC.cases()[names[0]])
    today = HC.batch_reference(names, idx, 4, len(names))
    none = run(D, dev, store, idx, 4, edge=None, **knobs)
    assert calls == ["awr_detect_hands"]
    assert_equal(none, today, names)
    assert_equal(run(D, dev, store, idx, 4, **knobs), today, names)
    assert calls == ["awr_detect_hands"] * 2
    for edge in (float("inf"), 65535, 1e9):
        calls.clear()
        got = run(D, dev, store, idx, 4, edge=edge, **knobs)
        assert calls == ["awr_detect_hands_edge"]
        assert_equal(got, none, (names, edge))


def test_the_new_entry_refuses_a_bad_edge_before_any_launch(D, dev):
    from awr_amd import _lib as L
    store = make_store(np.full((1, 48, 64), 700, np.uint16), dev)
    for edge in (-1.0, -1e-9, float("nan"), float("-inf")):
        with pytest.raises(L.AwrError, match="awr_detect_hands_edge: edge"):
            D.hands_device(store, [0], 2, edge=edge)
    for edge in ("40", True):
        with pytest.raises(TypeError, match="edge"):
            D.hands_device(store, [0], 2, edge=edge)
    # the other arguments' checks are the shared body's
    for kw, word in ((dict(hands=0), "K = 0"), (dict(hands=2, min_pixels=0), "min_pixels"), (dict(hands=2, reach=-1.0), "reach"),
                     (dict(hands=2, slab=float("nan")), "slab")):
        with pytest.raises(L.AwrError, match="awr_detect_hands_edge: .*" + word):
            D.hands_device(store, [0], edge=40, **kw)
    torch.cuda.synchronize()


# ---- the Predictor on the composites with exactly two candidates ---------------------------------------------------------------------------
S, J, NB = 64, 14, len(EC.EXACTLY_TWO)
FIELDS = ("xyz", "uvd", "center_xyz", "M", "status")


@pytest.fixture(scope="module")
def e2e(dev, over):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()
    frames = take(over.data, list(EC.EXACTLY_TWO))

    def make(max_batch=NB, **kw):
        return awr_amd.Predictor(net, S, 1.0, max_batch=max_batch, **kw)
    return types.SimpleNamespace(make=make, frames=frames, store=make_store(frames, dev), idx=torch.arange(NB, dtype=torch.int64, device=dev))


def hand_major(t):
    """a plain prediction's (2 * NB, ...) rows as the (NB, 2, ...) view a hands prediction has"""
    return t.view((2, NB) + tuple(t.shape[1:])).transpose(0, 1)


def test_predictor_finds_one_hand_without_the_edge_and_two_with_it(e2e, monkeypatch):
    from awr_amd import _lib as L
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    plain = e2e.make(hands=2)
    out = plain.predict(e2e.frames)
    assert plain.edge_mm is None and out.n_hands.tolist() == [1] * NB and out.status[:, 1].tolist() == [1] * NB
    assert "awr_detect_hands" in calls and "awr_detect_hands_edge" not in calls
    calls.clear()
    pred = e2e.make(hands=2, edge_mm=40)
    got = pred.predict(e2e.frames)
    assert "awr_detect_hands_edge" in calls and "awr_detect_hands" not in calls
    assert got.n_hands.tolist() == [2] * NB and got.status.tolist() == [[0, 0]] * NB and not torch.isnan(got.xyz).any()
    # the nearer hand first: slots are ordered by their component's nearest depth (without isolate both are then refined on the raw frame,
    # where overlapping hands stand in each other's window: the refined centres are not ordered, and may even meet)
    assert (pred.hand_info[:, 0, 3] < pred.hand_info[:, 1, 3]).all()
    pred.check()
    # the hands stage's rows are the statement's
    for b, i in enumerate(EC.EXACTLY_TWO):
        assert HC.same(pred.hand_info[b].cpu().numpy(), EC.overlap_reference(i, EC.OVER_EDGE)[3][:2])


def test_predictor_edge_and_isolate_equal_the_composition_of_their_parts(D, e2e, dev):
    seeds, st, info, count, labels = D.hands_device(e2e.store, e2e.idx, 2, edge=EC.OVER_EDGE, labels=True)
    assert st.flatten().tolist() == [0] * (2 * NB) and count.tolist() == [2] * NB
    iso, ist = D.isolate_device(e2e.store, e2e.idx, labels, info=info)
    assert ist.tolist() == [0] * NB and tuple(iso.shape) == (2 * NB,) + HC.FULL
    rows = torch.arange(2 * NB, dtype=torch.int64, device=dev)
    c, s = D.detect_device(make_store(iso, dev), rows, seed="given", centers=seeds.view(2 * NB, 3))
    assert s.tolist() == [0] * (2 * NB)
    want = e2e.make(max_batch=2 * NB, refine_iters=0).predict(iso, centers_uvd=c)
    pred = e2e.make(hands=2, isolate=True, edge_mm=EC.OVER_EDGE)
    got = pred.predict(e2e.frames)
    for f in FIELDS:
        g, w = getattr(got, f), hand_major(getattr(want, f))
        assert g.shape == w.shape and torch.equal(g, w) and not torch.isnan(g.float()).any(), f
    assert got.n_hands.tolist() == [2] * NB and pred.isolated.tolist() == [[1, 1]] * NB
    assert torch.equal(pred._all_frames[NB:].view(torch.int16), iso.view(torch.int16))
    pred.check()


def test_edge_mm_option_errors(e2e):
    with pytest.raises(ValueError, match="edge_mm"):
        e2e.make(max_batch=1, edge_mm=40)
    with pytest.raises(ValueError, match="edge_mm"):
        e2e.make(max_batch=1, hands=1, edge_mm=40.0)
    for edge, exc in ((-1, ValueError), (float("nan"), ValueError), ("40", TypeError), (True, TypeError)):
        with pytest.raises(exc, match="edge"):
            e2e.make(max_batch=1, hands=2, edge_mm=edge)
    assert e2e.make(max_batch=1, hands=2, edge_mm=float("inf")).edge_mm == float("inf")
