"""GPU: awr_detect_palm (csrc/awr_palm.hip) against its numpy statement awr_amd.detect.palm_center -- np.array_equal on
the centre, the status and the info row of every frame -- and awr_amd.Predictor(palm=True) against the composition of its parts."""
import types

import numpy as np
import pytest
import torch

import palm_cases as PC

pytestmark = pytest.mark.gpu

CUBE = (300.0, 300.0, 300.0)
GUARD, GUARD_WORD = 1024, 0x5A5A5A5A


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
    data = torch.from_numpy(np.array(frames)).to(dev)          # (a copy: the shared inputs are read-only)
    return types.SimpleNamespace(data=data, ftype=0, fh=int(frames.shape[1]), fw=int(frames.shape[2]), n=int(frames.shape[0]))


def run(D, dev, store, idx, centers, status, **kw):
    """palm_device with a guarded scratch -> numpy (centres, status, info); the guard words past the reported size must survive"""
    from awr_amd import _lib as L
    B = len(idx)
    nbytes = int(L.lib.awr_detect_palm_scratch(B, store.fh, store.fw))
    assert nbytes >= B * store.fh * store.fw * 4 and nbytes % 4 == 0
    scratch = torch.full((nbytes // 4 + GUARD,), GUARD_WORD, dtype=torch.int32, device=dev)
    c = torch.from_numpy(np.array(centers, dtype=np.float64)).to(dev)          # (copies: the shared inputs are read-only)
    s = torch.from_numpy(np.array(status, dtype=np.int32)).to(dev)
    out = D.palm_device(store, idx, c, s, scratch=scratch, **kw)
    assert (scratch[nbytes // 4:] == GUARD_WORD).all(), "awr_detect_palm wrote past awr_detect_palm_scratch(...) bytes"
    assert PC.same(c.cpu().numpy(), np.ascontiguousarray(centers, dtype=np.float64)), "separate outputs: the inputs stay as they are"
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def assert_rows(got, want, what=""):
    for g, w, name in zip(got, want, ("centre", "status", "info")):
        assert PC.same(g, w), (what, name, g, w)


@pytest.mark.parametrize("shape", [PC.SMALL, PC.TALL])
def test_hand_made_frames(D, dev, shape):
    cases = [c for c in PC.hand_cases().values() if c["frame"].shape == shape]
    assert len(cases) >= 6
    store = make_store(np.stack([c["frame"] for c in cases]), dev)
    ref = [PC.hand_reference(c["name"]) for c in cases]
    want = (np.stack([r[0] for r in ref]), np.array([r[1] for r in ref], np.int32), np.stack([r[2] for r in ref]))
    got = run(D, dev, store, np.arange(len(cases)), [c["center"] for c in cases], [c["status"] for c in cases], paras=cases[0]["paras"])
    for k, c in enumerate(cases):
        assert_rows([g[k] for g in got], [w[k] for w in want], c["name"])
    if shape == PC.SMALL:
        assert set(want[1].tolist()) == {D.OK, D.EMPTY, D.BAD_WINDOW} and (want[2][:, 3] > 0).sum() >= 10


SYNTH = {"small": (6, 77, PC.SMALL, 0.1), "mid": (6, 77, PC.MID, 0.2), "full": (1, 202, PC.FULL, 1.0)}


@pytest.mark.parametrize("which", list(SYNTH))
def test_procedural_hands(D, dev, which):
    """48 x 64 and 96 x 128: windows inside the frame and clipped ones, one row tile; 480 x 640: the real window, about 350 pixels square,
    8 row tiles"""
    frames, _, paras, _ = PC.synth_frames(*SYNTH[which])
    det_c, det_s, palm_c, palm_s, info = PC.synth_reference(*SYNTH[which])
    store = make_store(frames, dev)
    n = len(frames)
    # the detector on the device feeds the palm pass, as the Predictor chains them
    c, s = D.detect_device(store, np.arange(n), paras=paras)
    assert PC.same(c.cpu().numpy(), det_c) and PC.same(s.cpu().numpy(), det_s)
    got = run(D, dev, store, np.arange(n), det_c, det_s, paras=paras)
    assert_rows(got, (palm_c, palm_s, info), which)
    assert (palm_s == 0).all() and not PC.same(palm_c, det_c)
    again = run(D, dev, store, np.arange(n), det_c, det_s, paras=paras)
    assert_rows(again, got, "a second call")


def test_more_columns_than_threads(D, dev):
    """a 20 x 1100 window: the column scan loops over the 1024 threads, a row tile holds 14 rows (two tiles), and ragged random silhouettes
    give ties and short runs everywhere"""
    r = np.random.RandomState(5)
    frames = np.where(r.uniform(size=(2, 20, 1100)) < np.array([0.9, 0.998]).reshape(2, 1, 1), 640 + r.randint(0, 9, (2, 20, 1100)), 0).astype(np.uint16)
    store = make_store(frames, dev)
    centers, cube, paras = [(550.0, 10.0, 644.0)] * 2, (1e6, 1e6, 40.0), PC.paras_for(1.0)
    ref = [D.palm_center(f, c, 0, cube=cube, paras=paras) for f, c in zip(frames, centers)]
    want = (np.array([x[0] for x in ref]), np.array([x[1] for x in ref], np.int32), np.array([x[2] for x in ref], np.int32))
    assert want[1].tolist() == [0, 0]
    assert_rows(run(D, dev, store, [0, 1], centers, [0, 0], cube=cube, paras=paras), want)


@pytest.mark.parametrize("B,stride", [(1, 0), (3, 3), (70, 0), (70, 3)])
def test_batches_indices_and_cubes(D, dev, B, stride):
    frames, _, paras, _ = PC.synth_frames(*SYNTH["small"])
    det_c, det_s = PC.synth_reference(*SYNTH["small"])[:2]
    store = make_store(frames, dev)
    r = np.random.RandomState(B + stride)
    idx = r.randint(0, len(frames), B)                       # permuted and repeated
    cubes = np.array([(300.0, 300.0, 300.0), (240.0, 260.0, 280.0), (420.0, 380.0, 300.0)])[r.randint(0, 3, B)] if stride else np.array(CUBE)
    ref = [D.palm_center(frames[i], det_c[i], det_s[i], cube=cubes[k] if stride else CUBE, paras=paras) for k, i in enumerate(idx)]
    want = (np.array([x[0] for x in ref]), np.array([x[1] for x in ref], np.int32), np.array([x[2] for x in ref], np.int32))
    got = run(D, dev, store, idx, det_c[idx], det_s[idx], cube=cubes, paras=paras)
    assert_rows(got, want, (B, stride))
    assert (want[1] == 0).all()


def test_mixed_rows_bad_indices_in_place_and_null_info(D, dev):
    frames, _, paras, _ = PC.synth_frames(*SYNTH["small"])
    det_c, det_s, palm_c, palm_s, info = PC.synth_reference(*SYNTH["small"])
    store = make_store(frames, dev)
    nan3 = (np.nan,) * 3
    #        frame, centre,              status
    rows = [(0, det_c[0], 0), (6, det_c[1], 0),              # 6 == n_frames: AWR_DET_BAD_FRAME in the middle of the batch
            (1, det_c[1], 0), (2, nan3, 1),                  # a row awr_detect left EMPTY: passes through
            (2, det_c[2], 0), (3, nan3, 0),                  # a NaN centre with status OK: EMPTY, never a fault
            (3, det_c[3], 0), (-1, det_c[4], 0), (4, (1e300, 5.0, 700.0), 0), (5, det_c[5], 0), (5, (20.0, 20.0, 65000.0), 0)]
    idx = np.array([r[0] for r in rows])
    cin, sin = np.array([r[1] for r in rows], np.float64), np.array([r[2] for r in rows], np.int32)
    want_c, want_s, want_i = [], [], []
    for f, c, s in rows:
        if not 0 <= f < len(frames):
            ref = (nan3, D.BAD_FRAME, (-1, -1, 0, 0))
        else:
            ref = D.palm_center(frames[f], c, s, paras=paras)
        want_c.append(ref[0])
        want_s.append(ref[1])
        want_i.append(ref[2])
    want = (np.array(want_c, np.float64), np.array(want_s, np.int32), np.array(want_i, np.int32))
    assert want[1].tolist() == [0, 2, 0, 1, 0, 1, 0, 2, 1, 0, 1]
    got = run(D, dev, store, idx, cin, sin, paras=paras)
    assert_rows(got, want, "separate outputs")
    for k in (0, 2, 4, 6, 9):                               # the neighbours of the odd rows are what they are alone
        assert PC.same(got[0][k], palm_c[idx[k]]) and PC.same(got[2][k], info[idx[k]])
    # in place, and without the info rows
    c = torch.from_numpy(cin).to(dev)
    s = torch.from_numpy(sin).to(dev)
    out = D.palm_device(store, idx, c, s, paras=paras, center_out=c, status_out=s, info=False)
    assert out[0] is c and out[1] is s and out[2] is None
    assert_rows((c.cpu().numpy(), s.cpu().numpy()), want[:2], "in place")


def test_argument_errors_come_before_any_launch(D, dev):
    from awr_amd import _lib as L
    frames, _, paras, _ = PC.synth_frames(*SYNTH["small"])
    store = make_store(frames, dev)
    c = torch.zeros((1, 3), dtype=torch.float64, device=dev)
    s = torch.zeros(1, dtype=torch.int32, device=dev)
    for kw, word in ((dict(search=2.0, tau=(1, 3), rho2=(25, 4), depth_range=(5.0, 1.0)), "zmin"),):
        with pytest.raises(L.AwrError, match=word):
            D.palm_device(store, [0], c, s, paras=paras, **kw)
    fstore = types.SimpleNamespace(data=store.data, ftype=1, fh=store.fh, fw=store.fw)
    with pytest.raises(L.AwrError, match="uint16"):
        D.palm_device(fstore, [0], c, s, paras=paras)
    assert int(L.lib.awr_detect_palm_scratch(0, 48, 64)) == -1 and int(L.lib.awr_detect_palm_scratch(1, 16385, 64)) == -1
    assert 70 * 480 * 640 * 4 <= int(L.lib.awr_detect_palm_scratch(70, 480, 640)) <= 70 * (480 * 640 * 4 + 4096)


# ---- the Predictor ----------------------------------------------------------------------------------------------------------------------
EH, EW, S, J = 120, 160, 64, 14
FIELDS = ("uvd", "xyz", "M", "center_xyz", "status")


@pytest.fixture(scope="module")
def e2e(dev):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()
    frames, _, paras, flip = PC.synth_frames(2, 55, (EH, EW), 0.25)
    frames = np.array(frames)                               # (a copy: the shared frames are read-only)

    def make(**kw):
        return awr_amd.Predictor(net, S, 1.0, cube=CUBE, paras=paras, flip=flip, max_batch=2, frame_shape=(EH, EW), **kw)
    return types.SimpleNamespace(make=make, frames=frames, paras=paras, store=make_store(frames, dev))


def assert_same_prediction(got, want):
    for f in FIELDS:
        g, w = getattr(got, f).cpu().numpy(), getattr(want, f).cpu().numpy()
        assert PC.same(g, w), (f, g, w)


def test_predictor_palm_equals_its_composition(D, e2e):
    c, s = D.detect_device(e2e.store, [0, 1], paras=e2e.paras)
    pc, ps, info = D.palm_device(e2e.store, [0, 1], c, s, paras=e2e.paras)
    assert ps.tolist() == [0, 0] and not PC.same(pc.cpu().numpy(), c.cpu().numpy())
    want = e2e.make(refine_iters=0).predict(e2e.frames, centers_uvd=pc)
    pred = e2e.make(palm=True)
    got = pred.predict(e2e.frames)
    assert_same_prediction(got, want)
    assert PC.same(pred.palm_info.cpu().numpy(), info.cpu().numpy())
    plain = e2e.make().predict(e2e.frames)
    assert not PC.same(plain.xyz.cpu().numpy(), got.xyz.cpu().numpy())
    # one frame of a batch of two, and given centres: palm does not apply to them
    assert_same_prediction(pred.predict(e2e.frames[1:]), e2e.make(refine_iters=0).predict(e2e.frames[1:], centers_uvd=pc[1:]))
    assert_same_prediction(pred.predict(e2e.frames, centers_uvd=c), e2e.make().predict(e2e.frames, centers_uvd=c))
    pred.check()


def test_predictor_defaults_change_nothing(e2e):
    a, b = e2e.make(), e2e.make(palm=False)
    assert_same_prediction(b.predict(e2e.frames), a.predict(e2e.frames))
    assert b.palm_info is None and not hasattr(b, "_palm_scratch") and not hasattr(b, "_palm_info")
    with pytest.raises(TypeError):
        e2e.make(palm=1)
    with pytest.raises(ValueError):
        e2e.make(palm=True, palm_search=0.0)


def test_tracking_with_palm_first_call(D, e2e):
    """no tracked centre yet: every slot falls back to the detector branch, which palm=True has refined"""
    want = e2e.make(palm=True).predict(e2e.frames)
    trk = e2e.make(palm=True, track=True)
    got = trk.predict(e2e.frames)
    assert_same_prediction(got, want)
    c, s = D.detect_device(e2e.store, [0, 1], paras=e2e.paras)
    pc, _, _ = D.palm_device(e2e.store, [0, 1], c, s, paras=e2e.paras)
    assert PC.same(trk.centers_uvd.cpu().numpy(), pc.cpu().numpy())
