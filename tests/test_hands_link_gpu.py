"""GPU: awr_detect_hands_link (csrc/awr_hands.hip) against its numpy statements awr_amd.detect.components / hand_seeds with
`edge`, `link` and `gap` -- np.array_equal (NaN positions equal) on the labels, the centres, the status, the info rows and the count of
every frame, guard words round the scratch and the outputs -- the unchanged paths of link=None, and
awr_amd.Predictor(hands=2, isolate=True, edge_mm=40, link_mm=40) on the overlapping composites against the composition of its parts."""
import types

import numpy as np
import pytest
import torch

import edge_cases as EC
import hands_cases as HC
import link_cases as LC

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORD, GUARD_I32 = 1024, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
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
    """hands_device with a guarded scratch and guarded labels -> numpy (labels or None, centres, status, info, count); the guard words
    past the reported scratch size and on both sides of the labels must survive"""
    from awr_amd import _lib as L
    B = len(idx)
    nbytes = int(L.lib.awr_detect_hands_scratch(B, store.fh, store.fw))
    scratch = torch.full((nbytes // 8 + GUARD,), GUARD_WORD, dtype=torch.int64, device=dev)
    n = B * store.fh * store.fw
    guarded = torch.full((n + 2 * GUARD,), GUARD_I32, dtype=torch.int32, device=dev) if labels else None
    lab_in = guarded[GUARD:GUARD + n].view(B, store.fh, store.fw) if labels else False
    c, s, info, count, lab = D.hands_device(store, idx, K, labels=lab_in, scratch=scratch, **knobs)
    assert (scratch[nbytes // 8:] == GUARD_WORD).all(), "awr_detect_hands_link wrote past awr_detect_hands_scratch(...) bytes"
    if labels:
        assert (guarded[:GUARD] == GUARD_I32).all() and (guarded[GUARD + n:] == GUARD_I32).all(), "awr_detect_hands_link wrote outside labels_out"
    assert tuple(c.shape) == (K, B, 3) and tuple(s.shape) == (K, B) and tuple(info.shape) == (K, B, 4) and tuple(count.shape) == (B,)
    return (None if lab is None else lab.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy(), info.cpu().numpy(), count.cpu().numpy())


def assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        if g is not None:
            assert HC.same(g, w), (what, name, g, w)


def batch_reference(refs, idx, K, n_frames):
    return EC.batch_reference(None, idx, K, n_frames, ref=refs)


def group_id(k):
    return "%dx%d_%s" % (k[0][0], k[0][1], "_".join(str(x) for x in k[1:]))


GROUPS, NEW_GROUPS = HC.groups(), LC.groups()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("key", list(NEW_GROUPS), ids=group_id)
def test_the_new_cases(D, dev, key, K):
    """33 x 130 and 48 x 64: the gap, the depth agreement and the occluder at their boundaries along rows and columns, the one-sided pair,
    the breaks, the bar nearer than zmin, the half beyond the reach, the chain, the fragments below min_pixels, the noise"""
    names = NEW_GROUPS[key]
    store = make_store(np.stack([LC.cases()[n]["frame"] for n in names]), dev)
    idx = np.arange(len(names))
    want = batch_reference([LC.reference(n) for n in names], idx, K, len(names))
    knobs = LC.knobs(LC.cases()[names[0]])
    assert_equal(run(D, dev, store, idx, K, labels=True, **knobs), want, names)
    assert_equal(run(D, dev, store, idx, K, labels=False, **knobs), want, names)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("triple", LC.GPU_TRIPLES, ids=lambda t: "e%g_l%g_g%d" % t)
@pytest.mark.parametrize("key", list(GROUPS), ids=group_id)
def test_every_case_of_the_hands_suite_with_a_link(D, dev, key, triple, K):
    names = GROUPS[key]
    store = make_store(np.stack([HC.cases()[n]["frame"] for n in names]), dev)
    idx = np.arange(len(names))
    want = batch_reference([LC.reference(n, triple) for n in names], idx, K, len(names))
    knobs = dict(HC.knobs(HC.cases()[names[0]]), edge=triple[0], link=triple[1], gap=triple[2])
    assert_equal(run(D, dev, store, idx, K, labels=True, **knobs), want, (names, triple))
    assert_equal(run(D, dev, store, idx, K, labels=False, **knobs), want, (names, triple))


@pytest.mark.parametrize("K", KS)
def test_mixed_rows(D, dev, K):
    """bad frame indices in the middle of a batch and the same frame twice, with a link: every row is what it is alone"""
    key = max((k for k in NEW_GROUPS if k[0] == (33, 130)), key=lambda k: len(NEW_GROUPS[k]))
    names = NEW_GROUPS[key]
    n = len(names)
    assert n >= 4
    store = make_store(np.stack([LC.cases()[x]["frame"] for x in names]), dev)
    knobs = LC.knobs(LC.cases()[names[0]])
    refs = [LC.reference(x) for x in names]
    for idx in ([1], [n], [1, -1, 1], [2, n, 2], [n - 1, 1, 0, 1, n + 5, 3, 1, -7, 2]):
        want = batch_reference(refs, idx, K, n)
        got = run(D, dev, store, np.array(idx), K, **knobs)
        assert_equal(got, want, idx)
        bad = np.array([not 0 <= i < n for i in idx])
        assert (got[2][:, bad] == D.BAD_FRAME).all() and (got[4][bad] == 0).all() and (got[0][bad] == -1).all()


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


LINK = dict(min_pixels=EC.OVER_MIN_PIXELS, edge=EC.OVER_EDGE, link=LC.OVER_LINK, gap=LC.OVER_GAP)


def test_full_frames_once(D, dev, over):
    four = [3, 9, 11, 13]                                      # three candidates without the link in 3, 11 and 13; 9 stays merged
    host = EC.overlap_host()[2]
    assert np.array_equal(take(over.data, four).cpu().numpy(), host[four])
    refs = [LC.overlap_reference(i) for i in four]
    assert [r[4] for r in refs] == [2, 1, 2, 2]
    got = run(D, dev, make_store(take(over.data, four), dev), np.arange(4), 4, **LINK)
    assert_equal(got, batch_reference(refs, np.arange(4), 4, 4), four)
    # the constructed worst case: one rear column to `gap` front columns, every rear pixel walks the full gap to both sides
    for gap in (32, 64):
        f = LC.stripes(gap=gap)
        k = dict(HC.knobs(HC.DEFAULT), edge=40, link=40, gap=gap)
        want = LC._statement(f, 4, k)
        rear = len(range(0, 640, gap + 1))                      # the rear columns are ONE component; every front stripe is its own
        assert want[4] == LC.n_components(want[0]) == 1 + rear and (want[0][:, ::gap + 1] == 0).all()
        assert_equal(run(D, dev, make_store(f[None], dev), np.arange(1), 4, **k), batch_reference([want], [0], 4, 1), ("stripes", gap))
    # ... and one column more than the gap crosses: no link, a component per rear column
    f = LC.stripes(gap=33)
    k = dict(HC.knobs(HC.DEFAULT), edge=40, link=40, gap=32)
    want = LC._statement(f, 4, k)
    assert LC.n_components(want[0]) == 2 * len(range(0, 640, 34))
    assert_equal(run(D, dev, make_store(f[None], dev), np.arange(1), 4, **k), batch_reference([want], [0], 4, 1), "stripes of 33 at gap 32")


def test_composite_13_has_three_candidates_without_the_link_and_two_with_it(D, dev, over):
    store = make_store(take(over.data, [13]), dev)
    edge_only = run(D, dev, store, np.arange(1), 4, min_pixels=EC.OVER_MIN_PIXELS, edge=EC.OVER_EDGE)
    linked = run(D, dev, store, np.arange(1), 4, **LINK)
    assert edge_only[4].tolist() == [3] and linked[4].tolist() == [2]
    assert_equal(linked, batch_reference([LC.overlap_reference(13)], [0], 4, 1), 13)
    assert linked[3][1, 0, 2] >= edge_only[3][1, 0, 2] + edge_only[3][2, 0, 2]          # the rear slot holds both former candidates


def test_no_link_never_issues_the_new_entry_and_an_infinite_edge_is_todays_labels(D, dev, monkeypatch):
    from awr_amd import _lib as L
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    key = [k for k in GROUPS if k[0] == (33, 130) and k[1:] == ((1.0, 2000.0), 300.0, 150.0, 6)][0]
    names = GROUPS[key]
    store = make_store(np.stack([HC.cases()[n]["frame"] for n in names]), dev)
    idx = np.arange(len(names))
    knobs = HC.knobs(HC.cases()[names[0]])
    today = run(D, dev, store, idx, 4, **knobs)
    assert_equal(today, HC.batch_reference(names, idx, 4, len(names)), names)
    run(D, dev, store, idx, 4, link=None, gap=5, **knobs)
    edge = run(D, dev, store, idx, 4, edge=12.5, link=None, **knobs)
    assert calls == ["awr_detect_hands", "awr_detect_hands", "awr_detect_hands_edge"]
    assert_equal(edge, EC.batch_reference(names, idx, 4, len(names), 12.5), names)
    # a link with an edge that makes no pixel an occluder equals awr_detect_hands on every field
    for e, link, gap in ((float("inf"), 40, 32), (65535, 0, 1), (1e9, float("inf"), 64)):
        calls.clear()
        got = run(D, dev, store, idx, 4, edge=e, link=link, gap=gap, **knobs)
        assert calls == ["awr_detect_hands_link"]
        assert_equal(got, today, (names, e, link, gap))


def test_the_new_entry_refuses_bad_arguments_before_any_launch(D, dev):
    from awr_amd import _lib as L
    store = make_store(np.full((1, 48, 64), 700, np.uint16), dev)
    for link in (-1.0, -1e-9, float("nan"), float("-inf")):
        with pytest.raises(L.AwrError, match="awr_detect_hands_link: link"):
            D.hands_device(store, [0], 2, edge=40, link=link)
    for gap in (0, 65, -1):
        with pytest.raises(L.AwrError, match="awr_detect_hands_link: gap"):
            D.hands_device(store, [0], 2, edge=40, link=40, gap=gap)
    for edge in (-1.0, float("nan")):
        with pytest.raises(L.AwrError, match="awr_detect_hands_link: edge"):
            D.hands_device(store, [0], 2, edge=edge, link=40)
    with pytest.raises(ValueError, match="needs an edge"):
        D.hands_device(store, [0], 2, link=40)
    # the other arguments' checks are the shared body's
    for kw, word in ((dict(hands=0), "K = 0"), (dict(hands=2, min_pixels=0), "min_pixels"), (dict(hands=2, reach=-1.0), "reach"),
                     (dict(hands=2, slab=float("nan")), "slab")):
        with pytest.raises(L.AwrError, match="awr_detect_hands_link: .*" + word):
            D.hands_device(store, [0], edge=40, link=40, **kw)
    torch.cuda.synchronize()


# ---- the Predictor on the composites whose rear hand the edge alone leaves in pieces, and on those it does not -----------------------------
ROWS = (3, 11, 13, 0, 4)
S, J, NB = 64, 14, len(ROWS)
FIELDS = ("xyz", "uvd", "center_xyz", "M", "status")


@pytest.fixture(scope="module")
def e2e(dev, over):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()
    frames = take(over.data, list(ROWS))

    def make(max_batch=NB, **kw):
        return awr_amd.Predictor(net, S, 1.0, max_batch=max_batch, **kw)
    return types.SimpleNamespace(make=make, frames=frames, store=make_store(frames, dev), idx=torch.arange(NB, dtype=torch.int64, device=dev))


def hand_major(t):
    """a plain prediction's (2 * NB, ...) rows as the (NB, 2, ...) view a hands prediction has"""
    return t.view((2, NB) + tuple(t.shape[1:])).transpose(0, 1)


def test_predictor_link_and_isolate_equal_the_composition_of_their_parts(D, e2e, dev, monkeypatch):
    from awr_amd import _lib as L
    seeds, st, info, count, labels = D.hands_device(e2e.store, e2e.idx, 2, edge=EC.OVER_EDGE, link=LC.OVER_LINK, gap=LC.OVER_GAP, labels=True)
    assert st.flatten().tolist() == [0] * (2 * NB) and count.tolist() == [2] * NB
    iso, ist = D.isolate_device(e2e.store, e2e.idx, labels, info=info)
    assert ist.tolist() == [0] * NB and tuple(iso.shape) == (2 * NB,) + HC.FULL
    rows = torch.arange(2 * NB, dtype=torch.int64, device=dev)
    c, s = D.detect_device(make_store(iso, dev), rows, seed="given", centers=seeds.view(2 * NB, 3))
    assert s.tolist() == [0] * (2 * NB)
    want = e2e.make(max_batch=2 * NB, refine_iters=0).predict(iso, centers_uvd=c)
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    pred = e2e.make(hands=2, isolate=True, edge_mm=EC.OVER_EDGE, link_mm=LC.OVER_LINK)
    assert pred.link_mm == 40.0 and pred.link_gap == 32
    got = pred.predict(e2e.frames)
    assert "awr_detect_hands_link" in calls and "awr_detect_hands_edge" not in calls and "awr_detect_hands" not in calls
    for f in FIELDS:
        g, w = getattr(got, f), hand_major(getattr(want, f))
        assert g.shape == w.shape and torch.equal(g, w) and not torch.isnan(g.float()).any(), f
    assert got.n_hands.tolist() == [2] * NB and pred.isolated.tolist() == [[1, 1]] * NB
    assert torch.equal(pred._all_frames[NB:].view(torch.int16), iso.view(torch.int16))
    pred.check()
    for b, i in enumerate(ROWS):
        assert HC.same(pred.hand_info[b].cpu().numpy(), LC.overlap_reference(i)[3][:2])
    # without the link the same predictor's rear slot is ONE of the rear hand's pieces in the first three rows: fewer pixels
    calls.clear()
    plain = e2e.make(hands=2, isolate=True, edge_mm=EC.OVER_EDGE)
    assert plain.link_mm is None and plain.predict(e2e.frames).n_hands.tolist() == [2] * NB          # (n_hands is clamped at K)
    assert (plain.hand_info[:3, 1, 2] < pred.hand_info[:3, 1, 2]).all() and (plain.hand_info[:, 1, 2] <= pred.hand_info[:, 1, 2]).all()
    assert "awr_detect_hands_edge" in calls and "awr_detect_hands_link" not in calls


def test_link_mm_option_errors(e2e):
    with pytest.raises(ValueError, match="link_mm"):
        e2e.make(max_batch=1, hands=2, link_mm=40)
    with pytest.raises(ValueError, match="link_mm"):
        e2e.make(max_batch=1, link_mm=40)
    for kw, exc in ((dict(link_mm=-1), ValueError), (dict(link_mm=float("nan")), ValueError), (dict(link_mm="40"), TypeError),
                    (dict(link_mm=40, link_gap=0), ValueError), (dict(link_mm=40, link_gap=65), ValueError), (dict(link_mm=40, link_gap=True), TypeError)):
        with pytest.raises(exc, match="link|gap"):
            e2e.make(max_batch=1, hands=2, edge_mm=40, **kw)
    p = e2e.make(max_batch=1, hands=2, edge_mm=40, link_mm=float("inf"), link_gap=64)
    assert p.link_mm == float("inf") and p.link_gap == 64
