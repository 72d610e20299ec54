"""GPU: awr_detect_hands (csrc/awr_hands.hip) against its numpy statements awr_amd.detect.components / hand_seeds --
np.array_equal (NaN positions equal) on the labels, the centres, the status, the info rows and the count of every frame -- and
awr_amd.Predictor(hands=K) against the composition of its parts."""
import types

import numpy as np
import pytest
import torch

import hands_cases as HC

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORD = 1024, 0x5A5A5A5A5A5A5A5A
NAMES = ("labels", "centres", "status", "info", "count")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def make_store(frames, dev):
    data = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.array(frames)).to(dev)      # (a copy: the shared inputs are read-only)
    return types.SimpleNamespace(data=data, ftype=0, fh=int(data.shape[1]), fw=int(data.shape[2]), n=int(data.shape[0]))


def run(D, dev, store, idx, K, labels=True, **knobs):
    """hands_device with a guarded scratch -> numpy (labels or None, centres, status, info, count); the guard words past the reported
    size must survive"""
    from awr_amd import _lib as L
    B = len(idx)
    nbytes = int(L.lib.awr_detect_hands_scratch(B, store.fh, store.fw))
    assert nbytes % 8 == 0 and B * store.fh * store.fw * 12 <= nbytes <= B * (store.fh * store.fw * 12 + 4096)
    scratch = torch.full((nbytes // 8 + GUARD,), GUARD_WORD, dtype=torch.int64, device=dev)
    c, s, info, count, lab = D.hands_device(store, idx, K, labels=labels, scratch=scratch, **knobs)
    assert (scratch[nbytes // 8:] == GUARD_WORD).all(), "awr_detect_hands wrote past awr_detect_hands_scratch(...) bytes"
    assert tuple(c.shape) == (K, B, 3) and tuple(s.shape) == (K, B) and tuple(info.shape) == (K, B, 4) and tuple(count.shape) == (B,)
    return (None if lab is None else lab.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy(), info.cpu().numpy(), count.cpu().numpy())


def assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        if g is not None:
            assert HC.same(g, w), (what, name, g, w)


GROUPS = HC.groups()


@pytest.mark.parametrize("K", HC.KS)
@pytest.mark.parametrize("key", list(GROUPS), ids=lambda k: "%dx%d_%s" % (k[0][0], k[0][1], "_".join(str(x) for x in k[1:])))
def test_every_case(D, dev, key, K):
    names = GROUPS[key]
    store = make_store(np.stack([HC.cases()[n]["frame"] for n in names]), dev)
    idx = np.arange(len(names))
    want = HC.batch_reference(names, idx, K, len(names))
    knobs = HC.knobs(HC.cases()[names[0]])
    assert_equal(run(D, dev, store, idx, K, labels=True, **knobs), want, names)
    assert_equal(run(D, dev, store, idx, K, labels=False, **knobs), want, names)


def test_full_frames_once(D, dev):
    """480 x 640: 40 x 30 tiles; the serpentine is one corridor through all of them"""
    names = list(HC.full_cases())
    store = make_store(np.stack([HC.full_cases()[n]["frame"] for n in names]), dev)
    idx = np.arange(len(names))
    want = HC.batch_reference(names, idx, 4, len(names))
    assert want[4].tolist()[0] == 1 and want[4][2] >= 2
    assert_equal(run(D, dev, store, idx, 4, **HC.knobs(HC.full_cases()[names[0]])), want, names)


@pytest.mark.parametrize("K", HC.KS)
def test_mixed_rows(D, dev, K):
    """batches of 1 and 3 (and more): bad frame indices in the middle of a batch, the same frame twice -- two independent scratch regions --
    and every row what it is alone"""
    key = [k for k in GROUPS if k[0] == (48, 64) and k[1:] == ((1.0, 2000.0), 300.0, 150.0, 6)][0]
    names = GROUPS[key]
    n = len(names)
    store = make_store(np.stack([HC.cases()[x]["frame"] for x in names]), dev)
    knobs = HC.knobs(HC.cases()[names[0]])
    six = names.index("six_candidates")
    for idx in ([six], [n], [six, -1, six], [2, n, 2], [n - 1, six, 0, six, n + 5, 1, six, -7, 3]):
        want = HC.batch_reference(names, idx, K, n)
        got = run(D, dev, store, np.array(idx), K, **knobs)
        assert_equal(got, want, idx)
        bad = np.array([not 0 <= i < n for i in idx])
        assert (got[2][:, bad] == D.BAD_FRAME).all() and (got[4][bad] == 0).all() and (got[0][bad] == -1).all()


def test_argument_errors_come_before_any_launch(D, dev):
    from awr_amd import _lib as L
    store = make_store(np.zeros((1, 48, 64), np.uint16), dev)
    for kw, word in ((dict(hands=0), "K = 0"), (dict(hands=5), "K = 5"), (dict(hands=2, min_pixels=0), "min_pixels"),
                     (dict(hands=2, depth_range=(5.0, 1.0)), "zmin"), (dict(hands=2, reach=-1.0), "reach"), (dict(hands=2, reach=float("nan")), "reach"),
                     (dict(hands=2, slab=-0.5), "slab"), (dict(hands=2, slab=float("nan")), "slab")):
        with pytest.raises(L.AwrError, match=word):
            D.hands_device(store, [0], **kw)
    with pytest.raises(L.AwrError, match="uint16"):
        D.hands_device(types.SimpleNamespace(data=store.data, ftype=1, fh=48, fw=64), [0], 2)
    with pytest.raises(L.AwrError, match="16384"):
        D.hands_device(types.SimpleNamespace(data=store.data, ftype=0, fh=16385, fw=64), [0], 2, scratch=torch.empty(8, dtype=torch.int64, device=dev))
    with pytest.raises(L.AwrError, match="B = 0"):
        D.hands_device(store, np.zeros(0, np.int64), 2, scratch=torch.empty(8, dtype=torch.int64, device=dev))
    assert int(L.lib.awr_detect_hands_scratch(0, 48, 64)) == -1 and int(L.lib.awr_detect_hands_scratch(65536, 48, 64)) == -1
    assert int(L.lib.awr_detect_hands_scratch(1, 16385, 64)) == -1 and int(L.lib.awr_detect_hands_scratch(1, 48, 0)) == -1


# ---- the two-hand composites, rendered on the device --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two(dev):
    """-> frames_a, frames_b, composites (32, 480, 640) uint16 on the device, and stores over them"""
    from awr_amd import synth as SY
    prims_a, bbox_a, prims_b, bbox_b = HC.two_hands()
    fa = torch.empty((HC.N_TWO,) + HC.FULL, dtype=torch.uint16, device=dev)
    fb = torch.empty_like(fa)
    SY.render_device(prims_a, bbox_a, fa)
    SY.render_device(prims_b, bbox_b, fb)
    both = SY.compose(fa, fb)
    assert both.dtype == torch.uint16 and both.is_cuda
    return types.SimpleNamespace(a=make_store(fa, dev), b=make_store(fb, dev), both=make_store(both, dev))


def test_compose_on_the_device(two):
    from awr_amd import synth as SY
    a, b = two.a.data[:2].cpu().numpy(), two.b.data[:2].cpu().numpy()
    assert np.array_equal(two.both.data[:2].cpu().numpy(), SY.compose(a, b)) and (a > 0).any() and (b > 0).any()


def test_two_hands_operator_path_equals_the_single_detectors(D, dev, two):
    """all 32 composites: awr_detect_hands, then awr_detect with the seeds given over the K * B rows = awr_detect on the single hands' frames,
    bit for bit, ordered by the single frames' smallest depth"""
    n = HC.N_TWO
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    ca, sa = D.detect_device(two.a, idx)
    cb, sb = D.detect_device(two.b, idx)
    assert sa.tolist() == [0] * n and sb.tolist() == [0] * n
    seeds, status, info, count, _ = D.hands_device(two.both, idx, 2)
    assert status.flatten().tolist() == [0] * (2 * n) and count.tolist() == [2] * n
    c, s = D.detect_device(two.both, idx.repeat(2), seed="given", centers=seeds.view(2 * n, 3))
    assert s.tolist() == [0] * (2 * n)
    wide = lambda t: t.view(torch.int16).to(torch.int32) & 0xFFFF
    za = torch.where(wide(two.a.data) == 0, 1 << 20, wide(two.a.data)).flatten(1).min(1).values
    zb = torch.where(wide(two.b.data) == 0, 1 << 20, wide(two.b.data)).flatten(1).min(1).values
    assert (za != zb).all() and (info[0, :, 3] == torch.minimum(za, zb)).all() and (info[1, :, 3] == torch.maximum(za, zb)).all()
    a_first = (za < zb)[:, None]
    want = torch.stack([torch.where(a_first, ca, cb), torch.where(a_first, cb, ca)])
    assert torch.equal(c.view(2, n, 3), want)
    # the statement on the same device-rendered frames, for four of them
    for i in (0, 9, 18, 27):
        ref = D.hand_seeds(two.both.data[i].cpu().numpy(), 2)
        assert HC.same(seeds[:, i].cpu().numpy(), ref[0]) and HC.same(info[:, i].cpu().numpy(), ref[2])


# ---- the Predictor ----------------------------------------------------------------------------------------------------------------------
S, J, NB = 64, 14, 8
FIELDS = ("xyz", "uvd", "center_xyz", "M", "status")


@pytest.fixture(scope="module")
def e2e(D, dev, two):
    """eight composites, their refined hand centres (hand-major, (16, 3)) by the operator path, and predictors on one network"""
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()
    frames = two.both.data[:NB]
    tiled = torch.cat([frames.view(torch.int16)] * 2).view(torch.uint16)          # the composites twice: the frame of every hand-major row
    idx = torch.arange(NB, dtype=torch.int64, device=dev)
    store = make_store(frames, dev)
    seeds, _, info, count, _ = D.hands_device(store, idx, 2)
    c, s = D.detect_device(store, idx.repeat(2), seed="given", centers=seeds.view(2 * NB, 3))
    assert s.tolist() == [0] * (2 * NB)

    def make(max_batch=NB, **kw):
        return awr_amd.Predictor(net, S, 1.0, max_batch=max_batch, **kw)
    return types.SimpleNamespace(make=make, frames=frames, tiled=tiled, store=store, idx=idx, centers=c, status=s, info=info, count=count)


def hand_major(t):
    """a plain prediction's (2 * NB, ...) rows as the (NB, 2, ...) view a hands prediction has"""
    return t.view((2, NB) + tuple(t.shape[1:])).transpose(0, 1)


def assert_same_hands(got, want, fields=FIELDS):
    for f in fields:
        g, w = getattr(got, f), hand_major(getattr(want, f))
        assert g.shape == w.shape and torch.equal(g, w) and not torch.isnan(g.float()).any(), f


def test_predictor_hands_equals_a_plain_predictor_on_the_same_rows(e2e):
    """the same plan batch and the same row positions, so the same bits: Predictor(max_batch=16, refine_iters=0) on the composites tiled
    twice, handed the refined hand centres"""
    from awr_amd import predictor as P
    want = e2e.make(max_batch=2 * NB, refine_iters=0).predict(e2e.tiled, centers_uvd=e2e.centers)
    pred = e2e.make(hands=2)
    got = pred.predict(e2e.frames)
    assert type(got) is P.HandsPrediction and got.xyz.shape == (NB, 2, J, 3) and got.M.shape == (NB, 2, 3, 3) and got.status.shape == (NB, 2)
    assert_same_hands(got, want)
    assert got.n_hands.dtype == torch.int32 and got.n_hands.tolist() == [2] * NB == e2e.count.tolist()
    assert torch.equal(pred.hand_info, e2e.info.transpose(0, 1)) and pred.hand_info.shape == (NB, 2, 4)
    pred.check()
    # nothing was copied: the fields are views of the hand-major buffers
    assert got.xyz.transpose(0, 1)[:, :NB].is_contiguous() and got.xyz._base is not None
    # the two hands of a frame are different hands, the nearer one first
    assert (pred.hand_info[:, 0, 3] < pred.hand_info[:, 1, 3]).all() and (got.center_xyz[:, 0, 0] - got.center_xyz[:, 1, 0]).abs().min() > 100.0
    # centres handed in, (nb, K, 3), refined as configured; a NaN row is an absent hand
    given = hand_major(e2e.centers).clone()
    assert_same_hands(pred.predict(e2e.frames, centers_uvd=given), e2e.make(max_batch=2 * NB).predict(e2e.tiled, centers_uvd=e2e.centers))
    given[3, 1] = float("nan")
    out = pred.predict(e2e.frames, centers_uvd=given.cpu().numpy())
    assert out.n_hands.tolist() == [2, 2, 2, 1, 2, 2, 2, 2] and out.status[3].tolist() == [0, 1] and torch.isnan(out.xyz[3, 1]).all()
    assert torch.equal(out.xyz[:3], got.xyz[:3]) and pred.hand_info is None
    pred.check()
    with pytest.raises(Exception, match="centers_uvd"):
        pred.predict(e2e.frames, centers_uvd=e2e.centers)
    # a smaller batch, n_valid: the rows that count are what they are in a full batch (the crop, not the network: that is batch-normalised per row at inference)
    part = pred.predict(e2e.frames[:3], n_valid=2)
    assert part.xyz.shape == (3, 2, J, 3) and torch.equal(part.center_xyz[:2], got.center_xyz[:2]) and torch.equal(part.M[:2], got.M[:2])
    assert part.n_hands[:2].tolist() == [2, 2]


def test_predictor_hands_with_recentring_and_confidence(e2e):
    from awr_amd import predictor as P
    want = e2e.make(max_batch=2 * NB, refine_iters=0, recenter=1, confidence=True).predict(e2e.tiled, centers_uvd=e2e.centers)
    pred = e2e.make(hands=2, recenter=1, confidence=True)
    got = pred.predict(e2e.frames)
    assert type(got) is P.ConfidentHandsPrediction and got.conf.shape == (NB, 2, J)
    assert_same_hands(got, want, FIELDS + ("conf", "peak", "spread_mm"))
    assert pred.recenter_codes.shape == (2, NB, 2) and pred.centers_uvd.shape == (NB, 2, 3) and pred.next_centers_uvd.shape == (NB, 2, 3)
    pred.check()


def test_predictor_hands_with_palm(D, e2e):
    pc, ps, pinfo = D.palm_device(e2e.store, e2e.idx.repeat(2), e2e.centers, e2e.status)
    assert ps.tolist() == [0] * (2 * NB) and not torch.equal(pc, e2e.centers)
    want = e2e.make(max_batch=2 * NB, refine_iters=0).predict(e2e.tiled, centers_uvd=pc)
    pred = e2e.make(hands=2, palm=True)
    got = pred.predict(e2e.frames)
    assert_same_hands(got, want)
    assert torch.equal(pred.palm_info, hand_major(pinfo))
    pred.check()


def test_hands_1_is_todays_path(e2e, monkeypatch):
    """the same launches, in the same order with the same sizes, and the same bits as no argument"""
    from awr_amd import _lib as L
    from awr_amd import predictor as P
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append((name,) + tuple(x for x in a if isinstance(x, (int, float)) and not isinstance(x, bool) and abs(x) < 1 << 20)), real(name, *a))[1])
    a, b = e2e.make(max_batch=2), e2e.make(max_batch=2, hands=1)
    a.predict(e2e.frames[:2])                       # (an engine's first call also uploads its weights: compare the calls after it)
    b.predict(e2e.frames[:2])
    calls.clear()
    out_a = a.predict(e2e.frames[:2])
    calls_a = list(calls)
    calls.clear()
    out_b = b.predict(e2e.frames[:2])
    assert calls == calls_a and len(calls) >= 3 and not any(c[0] == "awr_detect_hands" for c in calls)
    assert type(out_b) is P.Prediction and all(torch.equal(getattr(out_a, f), getattr(out_b, f)) for f in FIELDS)
    assert b.hands == 1 and b.hand_info is None and not hasattr(b, "_hands_scratch")
    assert all(getattr(a, n).shape == getattr(b, n).shape for n in ("_idx", "_scratch", "_centers", "_seed", "_blocks", "_img"))


def test_hands_option_errors(D, e2e):
    for kw in (dict(views=D.make_views(rot=(10.0,))), dict(track=True), dict(smooth=True)):
        with pytest.raises(ValueError, match="not combined yet"):
            e2e.make(max_batch=1, hands=2, **kw)
    for kw, exc in ((dict(hands=0), ValueError), (dict(hands=5), ValueError), (dict(hands=2.0), TypeError), (dict(hands=True), TypeError),
                    (dict(hands=2, reach=-1.0), ValueError), (dict(hands=2, reach="far"), TypeError), (dict(hands=2, min_pixels=0), ValueError),
                    (dict(hands=2, min_pixels=10.5), TypeError), (dict(hands=1, min_pixels=0), ValueError)):
        with pytest.raises(exc):
            e2e.make(max_batch=1, **kw)
    with pytest.raises(Exception, match="dt"):
        e2e.make(max_batch=1, hands=2).predict(e2e.frames[:1], dt=0.03)


def test_one_hand_and_no_hand(D, e2e, two):
    from awr_amd import _lib as L
    pred = e2e.make(max_batch=2, hands=2)
    single = two.a.data[:2]
    got = pred.predict(single)
    assert got.n_hands.tolist() == [1, 1] and got.status.tolist() == [[0, 1], [0, 1]]
    assert torch.isnan(got.xyz[:, 1]).all() and torch.isnan(got.uvd[:, 1]).all() and torch.isnan(got.center_xyz[:, 1]).all()
    assert not torch.isnan(got.xyz[:, 0]).any() and pred.hand_info[:, 1].tolist() == [[-1, -1, 0, 0]] * 2
    pred.check()
    # the one hand is cropped where the single detector crops it
    plain = e2e.make(max_batch=2).predict(single)
    assert torch.equal(got.center_xyz[:, 0], plain.center_xyz) and torch.equal(got.M[:, 0], plain.M)
    empty = torch.zeros((2, 480, 640), dtype=torch.int16, device=single.device).view(torch.uint16)
    out = pred.predict(empty)
    assert out.n_hands.tolist() == [0, 0] and out.status.tolist() == [[1, 1], [1, 1]] and torch.isnan(out.xyz).all()
    with pytest.raises(L.AwrError, match="frame 0 of the batch, hand slot 0"):
        pred.check()
