"""GPU: per-joint confidence and vote spread -- awr_head_confidence_nhwc and awr_head_confidence against the float64
restatement of the definition (tests/confidence_ref.py), measured against the float32 run of the same restatement; one against the other;
reproducibility; InferEngine(confidence=True), Predictor(confidence=True) and FeatureModule.joint_confidence.

The bar of the kernel tests: for each of the four outputs, max over (b, j) of |device - float64| <= 4 x the same figure of the float32
host restatement on the same inputs (the kernel's ~2-ulp exp against libm's, another summation order over up to 4096 pixels).  Measured
gaps: DESIGN.md 4.18."""
import functools

import numpy as np
import pytest
import torch

import awr_oracle as O
import confidence_ref as R

pytestmark = pytest.mark.gpu

#              B   J   F   H
NHWC_SHAPES = [(2, 14, 8, 16),        # one tile per image, JS = 16
               (2, 21, 16, 32),       # JS = 32, several chunks, power-of-two F
               (2, 40, 8, 16),        # JS = 64
               (2, 14, 24, 48),       # general-F path, 9 tiles
               (32, 14, 64, 128)]     # two tiles per workgroup: the prefetch-ahead path
NCHW_SHAPES = [(2, 14, 8, 16), (2, 60, 8, 16)]      # 60 joints: more than the NHWC form takes
KSS = [0.4, 1.0]
FACTOR = 4.0


def ids(shapes):
    return ["B%d-J%d-F%d" % s[:3] for s in shapes]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    import awr_amd  # noqa: F401
    from awr_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def case(B, J, F, H):
    """inputs of one shape, made once and never modified"""
    off, img = R.bump_case(B, J, F, H, seed=100 + J + F)
    d = img[:, 0, ::H // F, ::H // F]
    frac = float((d >= 0.99).float().mean())
    assert 0.2 < frac < 0.4, frac
    return off, img


class Nhwc:
    """one shape's device buffers; head forward + confidence on them"""

    def __init__(self, L, dev, shape, ks):
        self.L, self.shape, self.ks = L, shape, ks
        B, J, F, H = shape
        off, img = case(*shape)
        self.cp = R.padded_channels(J)
        self.pred, self.img = R.to_nhwc(off, self.cp).to(dev), img.to(dev)
        self.scratch = torch.zeros(int(L.lib.awr_head_nhwc_scratch(B, J, F)), device=dev)
        self.jt, self.stat = torch.zeros(B, J, 3, device=dev), torch.zeros(B, J, 2, device=dev)
        L.call("awr_head_forward_nhwc", L.ptr(self.pred), self.cp, L.ptr(self.img), B, J, F, H, ks, L.ptr(self.scratch), L.ptr(self.jt), L.ptr(self.stat),
               L.stream())

    def confidence(self):
        L, (B, J, F, H) = self.L, self.shape
        out = torch.full((B, J, 4), -1.0, device=self.pred.device)
        L.call("awr_head_confidence_nhwc", L.ptr(self.pred), self.cp, L.ptr(self.img), L.ptr(self.jt), L.ptr(self.stat), B, J, F, H, self.ks,
               L.ptr(self.scratch), L.ptr(out), L.stream())
        return out


class Nchw:
    def __init__(self, L, dev, shape, ks):
        self.L, self.shape, self.ks = L, shape, ks
        B, J, F, H = shape
        off, img = case(*shape)
        self.off, self.img = off.to(dev), img.to(dev)
        self.jt, self.stat = torch.zeros(B, J, 3, device=dev), torch.zeros(B, J, 2, device=dev)
        L.call("awr_head_forward", L.ptr(self.off), L.ptr(self.img), B, J, F, H, ks, L.ptr(self.jt), L.ptr(self.stat), L.stream())

    def confidence(self):
        L, (B, J, F, H) = self.L, self.shape
        out = torch.full((B, J, 4), -1.0, device=self.off.device)
        L.call("awr_head_confidence", L.ptr(self.off), L.ptr(self.img), L.ptr(self.jt), L.ptr(self.stat), B, J, F, H, self.ks, L.ptr(out), L.stream())
        return out


def gaps(run, got):
    """(device gap, host float32 gap): per output, max over (b, j) of the distance to the float64 restatement about the joint the head wrote"""
    off, img = case(*run.shape)
    jt = run.jt.cpu()
    ref = R.confidence(off, img, run.ks, jt=jt)
    host = R.confidence(off, img, run.ks, jt=jt, dtype=torch.float32)
    assert host.dtype == torch.float32 and ref.dtype == torch.float64
    return (got.cpu().double() - ref).abs().amax((0, 1)), (host.double() - ref).abs().amax((0, 1)), ref


def check(name, run):
    got = run.confidence()
    g_dev, g_host, ref = gaps(run, got)
    print("\n%s %s ks=%.1f  [conf, var_u, var_v, var_d]  device gap %s  float32 host gap %s  ratio %s  (largest values %s)"
          % (name, run.shape, run.ks, ["%.2e" % v for v in g_dev.tolist()], ["%.2e" % v for v in g_host.tolist()],
             ["%.2f" % (a / b) for a, b in zip(g_dev.tolist(), g_host.tolist())], ["%.2e" % v for v in ref.amax((0, 1)).tolist()]))
    assert bool(torch.isfinite(got).all()) and float(got[..., 1:].min()) >= 0.0
    assert bool((g_dev <= FACTOR * g_host).all()), (g_dev.tolist(), g_host.tolist())
    return g_dev


@pytest.mark.parametrize("ks", KSS)
@pytest.mark.parametrize("shape", NHWC_SHAPES, ids=ids(NHWC_SHAPES))
def test_nhwc_against_the_float64_restatement(L, dev, shape, ks):
    """Measured on an MI355X (device gap / host gap, worst of the four outputs): see DESIGN.md 4.18."""
    run = Nhwc(L, dev, shape, ks)
    # the statistics fed in are the head's: peak = max / 30 is the largest masked heat value
    off, img = case(*shape)
    assert torch.allclose(run.stat[..., 0].cpu() / 30.0, R.peak(off, img), rtol=2.5e-7, atol=1e-12)      # (30 h) / 30: two roundings
    check("nhwc", run)


@pytest.mark.parametrize("ks", KSS)
@pytest.mark.parametrize("shape", NCHW_SHAPES, ids=ids(NCHW_SHAPES))
def test_nchw_against_the_float64_restatement(L, dev, shape, ks):
    B, J, F, H = shape
    if J > 56:          # the NHWC form refuses this joint count
        rc = L.lib.awr_head_confidence_nhwc(16, 256, 16, 16, 16, B, J, F, H, ks, 16, 16, None)
        assert rc == -1
    check("nchw", Nchw(L, dev, shape, ks))


def test_nhwc_against_nchw(L, dev):
    shape = (2, 14, 16, 32)
    a, b = Nhwc(L, dev, shape, 0.4), Nchw(L, dev, shape, 0.4)
    ca, cb = a.confidence(), b.confidence()
    ga, gb = gaps(a, ca)[0], gaps(b, cb)[0]
    d = (ca - cb).abs().amax((0, 1)).cpu().double()
    print("\nnhwc - nchw %s   gaps to float64: %s + %s" % (d.tolist(), ga.tolist(), gb.tolist()))
    assert bool((d <= ga + gb).all())


@pytest.mark.parametrize("det", [False, True])
def test_two_runs_give_the_same_bits(L, dev, det):
    import awr_amd
    was = awr_amd.get_deterministic()
    awr_amd.set_deterministic(det)
    try:
        for run in (Nhwc(L, dev, (2, 21, 16, 32), 0.4), Nhwc(L, dev, (32, 14, 64, 128), 0.4), Nchw(L, dev, (2, 14, 8, 16), 0.4)):
            first, second = run.confidence(), run.confidence()
            assert torch.equal(first, second) and not bool((first == -1.0).any())
    finally:
        awr_amd.set_deterministic(was)


def test_feature_module_joint_confidence(L, dev):
    import awr_amd
    run = Nchw(L, dev, (2, 14, 8, 16), 0.4)
    got = awr_amd.FeatureModule().joint_confidence(run.off, run.img, 0.4)
    assert got.shape == (2, 14, 4) and not got.requires_grad and torch.equal(got, run.confidence())


# ---- engines --------------------------------------------------------------------------------------------------------------------------
J = 14


@pytest.fixture(scope="module")
def net(dev):
    import awr_amd
    n = awr_amd.get_deconv_net(18, J, 2)
    n.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    return n.cuda().eval()


def test_engine_joints_do_not_move_and_conf_is_the_kernels(L, dev, net):
    from awr_amd.trainer import InferEngine
    img, _ = O.synth_batch(2, 128, J, seed=9)
    img = img.to(dev)
    plain = InferEngine(net, 2, 128, 0.4, autotune=False)
    assert plain.stat is None and plain.conf is None
    with pytest.raises(L.AwrError, match="confidence"):
        plain.peak
    jt0 = plain(img).clone()
    eng = InferEngine(net, 2, 128, 0.4, autotune=False, confidence=True)
    jt1 = eng(img).clone()
    assert torch.equal(jt0, jt1)
    assert eng.conf.shape == (2, J, 4) and torch.equal(eng.peak, eng.stat[..., 0] / 30)
    conf = eng.conf.clone()
    assert bool(torch.isfinite(conf).all()) and float(conf[..., 1:].min()) >= 0.0
    # what the engine left is what the entry point gives on the engine's own buffers, and the statement of the definition on its map
    again = torch.zeros_like(conf)
    L.call("awr_head_confidence_nhwc", eng._pred, eng._cp, L.ptr(eng.plan.img), L.ptr(eng.jt), L.ptr(eng.stat), 2, J, 64, 128, 0.4, L.ptr(eng._scratch),
           L.ptr(again), L.stream())
    assert eng.nhwc and torch.equal(conf, again)
    dense = eng.plan.dense_map(eng.stage).cpu()
    ref = R.confidence(dense, img.cpu(), 0.4, jt=jt1.cpu())
    host = R.confidence(dense, img.cpu(), 0.4, jt=jt1.cpu(), dtype=torch.float32)
    g_dev, g_host = (conf.cpu().double() - ref).abs().amax((0, 1)), (host.double() - ref).abs().amax((0, 1))
    print("\nengine: device gap %s host gap %s" % (g_dev.tolist(), g_host.tolist()))
    assert bool((g_dev <= FACTOR * g_host).all())
    assert torch.allclose(eng.peak.cpu(), R.peak(dense, img.cpu()), rtol=2.5e-7, atol=1e-12)
    # a captured graph holds the confidence launch
    graph = InferEngine(net, 2, 128, 0.4, autotune=False, confidence=True, use_graph=True)
    jt2 = graph(img)
    assert graph.graph is not None and torch.equal(jt2, jt0) and torch.equal(graph.conf, conf)
    graph.conf.fill_(-3.0)
    graph(img)
    assert torch.equal(graph.conf, conf)
    # the reference-layout boundary issues the NCHW launch
    nchw = InferEngine(net, 2, 128, 0.4, autotune=False, confidence=True, nhwc_boundary=False)
    nchw(img)
    assert not nchw.nhwc
    direct = torch.zeros_like(conf)
    L.call("awr_head_confidence", L.ptr(nchw.plan.outputs[nchw.stage]), L.ptr(nchw.plan.img), L.ptr(nchw.jt), L.ptr(nchw.stat), 2, J, 64, 128, 0.4,
           L.ptr(direct), L.stream())
    assert torch.equal(nchw.conf, direct)
    g_nchw = (nchw.conf.cpu().double() - R.confidence(dense, img.cpu(), 0.4, jt=nchw.jt.cpu())).abs().amax((0, 1))
    assert bool(((nchw.conf - conf).abs().amax((0, 1)).cpu().double() <= g_dev + g_nchw).all())


def test_engine_with_loss_weights_keeps_its_statistics(L, dev, net):
    """the scoring engine (awr_head_eval_nhwc) hands the same joints, statistics and confidence on"""
    from awr_amd.trainer import InferEngine
    img, jt_gt = O.synth_batch(2, 128, J, seed=9)
    img, jt_gt = img.to(dev), jt_gt.to(dev)
    eng = InferEngine(net, 2, 128, 0.4, autotune=False, confidence=True)
    eng(img)
    scored = InferEngine(net, 2, 128, 0.4, autotune=False, confidence=True, loss_weights=(1.0, 1.0))
    scored(img, jt_gt)
    assert torch.equal(scored.jt, eng.jt) and torch.equal(scored.stat, eng.stat) and torch.equal(scored.conf, eng.conf)


def blob_frames():
    """two 480 x 640 frames: a plane at 1500 mm and a blob at about 700 mm, at different places"""
    f = np.full((2, 480, 640), 1500, np.uint16)
    vv, uu = np.mgrid[0:480, 0:640]
    for b, (cu, cv) in enumerate(((250, 200), (400, 260))):
        m = (np.abs(uu - cu) <= 60) & (np.abs(vv - cv) <= 60)
        f[b][m] = (680 + (uu[m] + vv[m]) % 41).astype(np.uint16)
    return f


def test_predictor_confidence(L, dev, net):
    import awr_amd
    from awr_amd import detect as D
    from awr_amd import predictor as PR
    kw = dict(cube=(300.0, 250.0, 200.0), max_batch=2, seed="nearest", depth_range=(200.0, 1200.0), slab=100.0, refine_iters=2, winograd=False)
    frames = blob_frames()
    plain = awr_amd.Predictor(net, 128, 0.4, **kw)
    out0 = plain.predict(frames)
    plain.check()
    assert type(out0) is PR.Prediction and out0._fields == ("xyz", "uvd", "center_xyz", "M", "status")
    pred = awr_amd.Predictor(net, 128, 0.4, confidence=True, **kw)
    out = pred.predict(frames)
    pred.check()
    assert type(out) is PR.ConfidentPrediction and out.status.tolist() == [0, 0]
    assert torch.equal(out.xyz, out0.xyz) and torch.equal(out.uvd, out0.uvd) and not bool(torch.isnan(out.xyz).any())
    eng = pred.engine
    assert out.conf.shape == out.peak.shape == out.spread_mm.shape == (2, J)
    assert torch.equal(out.conf, eng.conf[..., 0])
    assert torch.equal(out.peak.cpu(), (eng.stat[..., 0].cpu().double() / 30.0).float())          # max / 30, correctly rounded
    assert torch.allclose(out.peak, eng.peak, rtol=2e-7, atol=0.0)                                 # (a device tensor over a scalar may multiply by 1 / 30)
    want = R.spread_mm(eng.conf.cpu(), kw["cube"])
    # sqrt of a sum of three products of float32 numbers: a few units in the last place
    assert torch.allclose(out.spread_mm.cpu(), want, rtol=1e-6, atol=0.0), (out.spread_mm.cpu(), want)
    assert bool((out.spread_mm > 0).all()) and bool(torch.isfinite(out.spread_mm).all())
    # an empty frame: NaN rows, the other frame as before
    empty = frames.copy()
    empty[1] = 0
    both = out.conf.clone(), out.spread_mm.clone(), out.peak.clone()
    out2 = pred.predict(empty)
    assert out2.status.tolist() == [0, D.EMPTY]
    for got, was in zip((out2.conf, out2.spread_mm, out2.peak), both):
        assert bool(torch.isnan(got[1]).all()) and torch.equal(got[0], was[0])
    assert bool(torch.isnan(out2.xyz[1]).all())
    # a padded batch: one frame of a plan of two
    one = pred.predict(frames[:1])
    assert one.conf.shape == (1, J) and torch.equal(one.conf[0], both[0][0]) and torch.equal(one.spread_mm[0], both[1][0])
