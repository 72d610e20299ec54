"""GPU: re-centring on predicted joints and tracking -- awr_joints_center and awr_centers_select against their numpy
statements bit for bit, and awr_amd.Predictor's recenter / track modes against compositions of plain predict() calls."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLIP, CUBE = -1, (300.0, 300.0, 300.0)
EH, EW, S, J = 120, 160, 64, 14
E_PARAS = (147.0, 146.8, 80.0, 60.0)                # NYU's intrinsics scaled to a 160 x 120 frame
OPEN = dict(max_shift=1e9, depth_range=(1, 65535))  # a gate that only non-finite joints fail


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def bits(a):
    """the 64- or 32-bit patterns of a tensor or array: NaN payloads and signed zeros count"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- the operators ----------------------------------------------------------------------------------------------------------------------
def hand_made_batch():
    """tests/test_recenter_cpu.py's batch: B = 6, J = 14 around (-20, 10, 620); a NaN in frame 1 (joint 5), frame 2 too deep, frame 3 200 mm
    off in x, frame 4 with a detector status"""
    from awr_amd.evaluator import xyz2uvd
    r = np.random.RandomState(3)
    B = 6
    cxyz = np.tile(np.array([-20.0, 10.0, 620.0], np.float32), (B, 1))
    xyz = (cxyz[:, None, :] + r.uniform(-100, 100, (B, 14, 3))).astype(np.float32)
    xyz[1, 5, 1] = np.nan
    xyz[2, :, 2] += 2000.0
    xyz[3, :, 0] += 200.0
    status, ustatus = np.zeros(B, np.int32), np.zeros(B, np.int32)
    status[4] = 1
    cuvd = xyz2uvd(cxyz.astype(np.float64), E_PARAS, FLIP).astype(np.float64) + r.uniform(-0.25, 0.25, (B, 3))
    return xyz, cuvd, cxyz, np.full((B, 3), 300.0, np.float32), status, ustatus


GATE_ROWS = {30: 1, 31: 4, 32: 1, 33: 1, 34: 4}


def random_batch(B=300, nj=21, seed=17):
    """more frames than one workgroup holds, with every kind of row mixed in"""
    r = np.random.RandomState(seed)
    cxyz = np.stack([r.uniform(-150, 150, B), r.uniform(-120, 120, B), r.uniform(500, 1000, B)], 1).astype(np.float32)
    cube = np.full((B, 3), 300.0, np.float32)
    if B > 100:
        cube[100:] = np.repeat(r.uniform(200, 400, (B - 100, 1)), 3, 1).astype(np.float32)
    xyz = (cxyz[:, None, :] + r.uniform(-140, 140, (B, nj, 3))).astype(np.float32)
    status, ustatus = np.zeros(B, np.int32), np.zeros(B, np.int32)
    if B > 40:
        status[[3, 50, 290]] = [1, 3, 2]
        ustatus[[7, 50, 260]] = [1, 2, 2]
        xyz[10, 2, 0], xyz[11, 4, 2], xyz[12, 20, 1] = np.inf, -np.inf, np.nan
        xyz[13, 0, 0], xyz[13, 1, 0] = np.inf, -np.inf          # the sum itself becomes NaN
        xyz[20, :, 2] -= 800.0                                  # nearer than zmin = 300
        xyz[21, :, 2] += 2000.0                                 # farther than zmax = 1500
        xyz[22, :, 2] = 1500.0                                  # exactly zmax: inside
        xyz[23, :, 2] = 300.0                                   # exactly zmin: inside (were the shift gate open)
        # shifts exactly at the gate.  nj copies of one float32 value sum and divide exactly in double, so the mean IS that value:
        # |delta| == 1.0 * 300 / 2 must pass, one float32 step more must not
        for row in GATE_ROWS:
            cxyz[row], cube[row] = (-20.0, 10.0, 620.0), 300.0
            xyz[row] = cxyz[row]
        xyz[30, :, 0] = 130.0
        xyz[31, :, 0] = np.nextafter(np.float32(130.0), np.float32(1e9))
        xyz[32, :, 2] = 770.0
        xyz[33, :, 1] = -140.0
        xyz[34, :, 1] = np.nextafter(np.float32(-140.0), np.float32(-1e9))
    cuvd = np.stack([r.uniform(0, 640, B), r.uniform(0, 480, B), r.uniform(400, 1100, B)], 1)
    if B > 40:
        cuvd[[3, 5]] = np.nan          # (row 3 has a status code and is kept, row 5 is moved)
    return xyz, cuvd, cxyz, cube, status, ustatus


def run_center(D, dev, batch, paras=E_PARAS, **kw):
    xyz, cuvd, cxyz, cube, status, ustatus = (torch.from_numpy(a).to(dev) for a in batch)
    return D.joints_center_device(xyz, cuvd, cxyz, cube, status, ustatus, paras, FLIP, **kw)


def assert_center_equal(got, want, rows=slice(None)):
    for g, w, name in zip(got, want, ("center_out", "next", "code")):
        assert same_bits(g[rows], w[rows]), (name, g[rows].cpu().numpy(), w[rows])


def test_joints_center_equals_the_statement_on_the_hand_made_batch(D, dev):
    batch = hand_made_batch()
    for kw in (dict(), dict(joints=[0, 3, 13], **OPEN)):
        want = D.joints_center(*batch, E_PARAS, FLIP, **kw)
        got = run_center(D, dev, batch, **kw)
        assert got[0].dtype == torch.float64 and got[1].dtype == torch.float64 and got[2].dtype == torch.int32
        assert_center_equal(got, want)
        assert want[2].tolist() == ([1, 1, 1, 1, 0, 1] if kw else [1, 2, 3, 4, 0, 1])


def test_joints_center_equals_the_statement_on_a_mixed_batch(D, dev):
    batch = random_batch()
    B = batch[0].shape[0]
    kw = dict(depth_range=(300.0, 1500.0), max_shift=1.0)
    want = D.joints_center(*batch, E_PARAS, FLIP, **kw)
    got = run_center(D, dev, batch, **kw)
    assert_center_equal(got, want)
    code = want[2]
    print("codes of the mixed batch:", np.bincount(code, minlength=5).tolist())
    assert all(code[r] == c for r, c in GATE_ROWS.items()), code[30:35]            # the gate is inclusive, to the float32 step
    assert code[[3, 50, 290, 7, 260]].tolist() == [0] * 5 and code[[10, 11, 12, 13]].tolist() == [2] * 4 and code[[20, 21]].tolist() == [3, 3]
    assert code[22] in (1, 4) and code[23] in (1, 4) and set(np.unique(code).tolist()) == {0, 1, 2, 3, 4} and (code[256:] == 1).any()
    # the centre a pass was cropped at is carried where the frame is kept and plays no part where it moves: the gate is about center_xyz
    assert np.isnan(want[0][3]).all() and code[5] == 1 and np.isfinite(want[0][5]).all() and np.isnan(batch[1][5]).all()
    # a subset of the joints; no gate at all
    for kw2 in (dict(joints=[0, 5, 20], **kw), dict(joints=[20], depth_range=(-1e30, 1e30), max_shift=float("inf"))):
        assert_center_equal(run_center(D, dev, batch, **kw2), D.joints_center(*batch, E_PARAS, FLIP, **kw2))
    # an index outside [0, J): code 2 for every frame that is judged at all, and by construction no read through it
    for bad in ([0, 21, 3], [-1], [5, 1 << 30]):
        want_bad = D.joints_center(*batch, E_PARAS, FLIP, joints=bad, **kw)
        got_bad = run_center(D, dev, batch, joints=bad, **kw)
        assert_center_equal(got_bad, want_bad)
        assert set(want_bad[2].tolist()) == {0, 2} and same_bits(got_bad[0], batch[1]) and torch.isnan(got_bad[1]).all()
    # n_valid < B: the rows past it are neither read nor written (257 = one frame into the second workgroup)
    nv = 257
    outs = (torch.full((B, 3), -7.0, dtype=torch.float64, device=dev), torch.full((B, 3), -7.0, dtype=torch.float64, device=dev),
            torch.full((B,), -7, dtype=torch.int32, device=dev))
    got_nv = run_center(D, dev, batch, n_valid=nv, center_out=outs[0], next_out=outs[1], code=outs[2], **kw)
    assert_center_equal(got_nv, want, slice(0, nv))
    assert (got_nv[0][nv:] == -7.0).all() and (got_nv[1][nv:] == -7.0).all() and (got_nv[2][nv:] == -7).all()
    # center_out aliased onto center_uvd
    t = [torch.from_numpy(a).to(dev) for a in batch]
    alias = D.joints_center_device(t[0], t[1], t[2], t[3], t[4], t[5], E_PARAS, FLIP, center_out=t[1], **kw)
    assert alias[0].data_ptr() == t[1].data_ptr()
    assert_center_equal(alias, want)


@pytest.mark.parametrize("nj", [1, 256])
def test_joints_center_at_the_ends_of_the_joint_range(D, dev, nj):
    batch = random_batch(B=5, nj=nj, seed=nj)
    for kw in (dict(depth_range=(300.0, 1500.0), max_shift=1.0), dict(joints=sorted({nj - 1, 0}, reverse=True), **OPEN)):
        want = D.joints_center(*batch, E_PARAS, FLIP, **kw)
        assert_center_equal(run_center(D, dev, batch, **kw), want)
        assert (want[2] == 1).any()


def test_select_equals_the_statement(D, dev):
    r = np.random.RandomState(23)
    B = 300

    def centres():
        c = np.stack([r.uniform(0, 640, B), r.uniform(0, 480, B), r.uniform(400, 1100, B)], 1)
        raw = c.view(np.uint64)
        for k, payload in enumerate((0x7FF8000000000000, 0x7FF8000000000123, 0xFFF8000000000ABC, 0x7FF0000000000000, 0xFFF0000000000000)):
            rows = r.choice(B, 25, replace=False)
            raw[rows, r.randint(0, 3, 25)] = payload            # quiet NaNs with payloads, and the two infinities
        return c
    a, b = centres(), centres()
    a_st = r.choice([0, 0, 0, 1, 2, 3], B).astype(np.int32)
    b_st = r.choice([0, 0, 1, 2, 3], B).astype(np.int32)
    want = D.select(a, a_st, b, b_st)
    got = D.select_device(*(torch.from_numpy(x).to(dev) for x in (a, a_st, b, b_st)))
    for g, w, name in zip(got, want, ("center", "status", "which")):
        assert same_bits(g, w), name
    which = want[2]
    assert 0 < which.sum() < B and (which[256:] == 0).any() and (which[256:] == 1).any()
    ok_but_not_finite = (a_st == 0) & ~np.isfinite(a).all(1)
    assert ok_but_not_finite.any() and which[ok_but_not_finite].all() and np.isnan(want[0]).any()


# ---- the Predictor ----------------------------------------------------------------------------------------------------------------------
HANDS, DISTRACTORS = ((60, 50), (100, 70)), ((140, 100), (20, 20))


def blob_frames(hands=HANDS, distractors=None):
    """two frames: a far plane and a hand-sized blob of 41 x 41 pixels at 600 ... 640 mm; with `distractors` also a nearer 11 x 11 blob at
    400 mm, which the "nearest" seed finds instead of the hand"""
    f = np.full((2, EH, EW), 1400, np.uint16)
    vv, uu = np.mgrid[0:EH, 0:EW]
    for b, (cu, cv) in enumerate(hands):
        m = (np.abs(uu - cu) <= 20) & (np.abs(vv - cv) <= 20)
        f[b][m] = (600 + (uu[m] + vv[m]) % 41).astype(np.uint16)
        if distractors is not None:
            du, dv = distractors[b]
            f[b][(np.abs(uu - du) <= 5) & (np.abs(vv - dv) <= 5)] = 400
    return f


C0 = np.array([(61.0, 49.0, 622.0), (99.5, 71.25, 618.0)])
FIELDS = ("uvd", "xyz", "M", "center_xyz", "status")
AUTO = dict(seed="nearest", depth_range=(200.0, 1200.0), slab=100.0, refine_iters=2)


@pytest.fixture(scope="module")
def e2e(dev):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()

    def make(**kw):
        return awr_amd.Predictor(net, S, 1.0, cube=CUBE, paras=E_PARAS, flip=FLIP, max_batch=2, frame_shape=(EH, EW), **kw)
    return types.SimpleNamespace(net=net, make=make, frames=blob_frames())


def host_center(D, pred, out, centers, **kw):
    """detect.joints_center of a predict() result: the statement of the step between two passes"""
    nb = out.xyz.shape[0]
    ustatus = pred._last[1][:nb].cpu().numpy()
    return D.joints_center(out.xyz.cpu().numpy(), centers, out.center_xyz.cpu().numpy(), np.tile(np.float32(CUBE), (nb, 1)),
                           out.status.cpu().numpy(), ustatus, E_PARAS, FLIP, **kw)


def assert_same_prediction(got, want, rows=slice(None), fields=FIELDS):
    for f in fields:
        g, w = getattr(got, f)[rows], getattr(want, f)[rows]
        assert same_bits(g, w), (f, g.cpu().numpy(), w.cpu().numpy())


_COMPOSED = {}


def compose(D, e2e, confidence):
    """three plain given-centre calls, each cropped at the joint centre of the one before: what recenter=1 and recenter=2 must reproduce
    (computed once per kind of engine and left unchanged)"""
    if confidence in _COMPOSED:
        return _COMPOSED[confidence]
    plain = e2e.make(refine_iters=0, confidence=confidence, **OPEN)
    assert plain.centers_uvd is None and plain.recenter_codes is None
    outs, centers, codes, nexts = [], [C0], [], []
    for _ in range(3):
        out = plain.predict(e2e.frames, centers_uvd=centers[-1])
        c, nxt, code = host_center(D, plain, out, centers[-1], **OPEN)
        outs.append(out)
        centers.append(c)
        codes.append(code)
        nexts.append(nxt)
        print("pass %d: status %s codes %s centres %s" % (len(outs) - 1, out.status.tolist(), code.tolist(), centers[-1].tolist()))
    # with this gate only non-finite joints keep a frame: the comparison below must be about frames that really moved
    assert (codes[0] == 1).any() and (codes[1] == 1).any(), codes
    assert not same_bits(centers[1], centers[0]) and not same_bits(outs[1].xyz, outs[0].xyz)
    _COMPOSED[confidence] = types.SimpleNamespace(outs=outs, centers=centers, codes=codes, nexts=nexts)
    return _COMPOSED[confidence]


@pytest.mark.parametrize("n", [1, 2])
def test_recentred_passes_equal_their_composition(D, e2e, n):
    composed = compose(D, e2e, False)
    rec = e2e.make(recenter=n, refine_iters=0, **OPEN)
    out = rec.predict(e2e.frames, centers_uvd=C0)
    want = composed.outs[n]
    for f in ("uvd", "xyz", "M", "center_xyz"):
        assert torch.equal(getattr(out, f), getattr(want, f)), f
    assert torch.equal(out.status, want.status) and type(out).__name__ == "Prediction"
    assert rec.recenter_codes.shape == (n + 1, 2) and rec.recenter_codes.dtype == torch.int32
    assert rec.recenter_codes.cpu().numpy().tolist() == [c.tolist() for c in composed.codes[:n + 1]]
    assert same_bits(rec.centers_uvd, composed.centers[n]) and same_bits(rec.next_centers_uvd, composed.nexts[n])
    rec.check()


def test_confidence_rides_on_the_final_pass(D, e2e):
    composed = compose(D, e2e, True)
    rec = e2e.make(recenter=1, refine_iters=0, confidence=True, **OPEN)
    out = rec.predict(e2e.frames, centers_uvd=C0)
    assert type(out).__name__ == "ConfidentPrediction"
    assert_same_prediction(out, composed.outs[1], fields=FIELDS + ("conf", "peak", "spread_mm"))
    assert not same_bits(out.conf, composed.outs[0].conf)


def test_kept_frames_repeat_themselves(D, e2e):
    kw = dict(refine_iters=0, depth_range=(1, 65535))
    plain = e2e.make(**kw)
    kept = e2e.make(recenter=2, max_shift=0.0, **kw)
    want = plain.predict(e2e.frames, centers_uvd=C0)
    out = kept.predict(e2e.frames, centers_uvd=C0)
    assert kept.recenter_codes.tolist() == [[D.KEPT_SHIFT] * 2] * 3
    assert_same_prediction(out, want)
    assert same_bits(kept.centers_uvd, C0) and torch.isnan(kept.next_centers_uvd).all()


def test_defaults_change_nothing(e2e):
    a = e2e.make(confidence=True, **AUTO)
    b = e2e.make(confidence=True, recenter=0, track=False, **AUTO)
    every = FIELDS + ("conf", "peak", "spread_mm")
    for kw in (dict(frames=e2e.frames), dict(frames=e2e.frames[:1]), dict(frames=e2e.frames, centers_uvd=C0),
               dict(frames=e2e.frames[1:], centers_uvd=C0[1:])):
        assert_same_prediction(b.predict(**kw), a.predict(**kw), fields=every)
    # and nothing new is allocated or kept
    assert b.centers_uvd is None and b.next_centers_uvd is None and b.recenter_codes is None
    assert not any(hasattr(b, name) for name in ("_track", "_moved", "_joints", "_tcenters", "_dcenters"))
    with pytest.raises(Exception, match="track=True"):
        b.set_track(C0)


def test_tracking(D, e2e):
    frames = blob_frames(distractors=DISTRACTORS)
    auto, trk = e2e.make(**AUTO), e2e.make(track=True, **AUTO)
    nan3 = [float("nan")] * 3
    hand = np.array([(60.0, 50.0, 620.0), (100.0, 70.0, 620.0)])
    det = auto.predict(frames)
    tracked = auto.predict(frames, centers_uvd=hand)
    assert det.status.tolist() == [0, 0] and tracked.status.tolist() == [0, 0]
    for b in (0, 1):          # the detector sits on the nearer blob, the tracker on the hand: the two sources are told apart below
        assert not same_bits(det.center_xyz[b], tracked.center_xyz[b]) and not same_bits(det.xyz[b], tracked.xyz[b])
    # slot 0 tracked, slot 1 lost
    trk.set_track(np.array([hand[0], nan3]))
    out = trk.predict(frames)
    assert_same_prediction(out, tracked, rows=0)
    assert_same_prediction(out, det, rows=1)
    assert trk.recenter_codes.shape == (1, 2) and trk.centers_uvd.shape == (2, 3)
    # the hand of frame 0 jumps 60 pixels: the tracked window finds nothing, slot 0 falls back to the detector; slot 1 is still tracked
    jumped = blob_frames(hands=((120, 50), HANDS[1]), distractors=DISTRACTORS)
    assert D.detect(jumped[0], seed="given", center=hand[0], cube=CUBE, paras=E_PARAS, iters=2, depth_range=AUTO["depth_range"])[1] == D.EMPTY
    trk.set_track(torch.from_numpy(hand).to(trk.device))          # device input
    out = trk.predict(jumped)
    assert_same_prediction(out, auto.predict(jumped), rows=0)
    assert_same_prediction(out, auto.predict(jumped, centers_uvd=hand), rows=1)
    assert out.status.tolist() == [0, 0]
    # reset_track: the detector alone
    trk.set_track(hand)
    trk.reset_track()
    assert_same_prediction(trk.predict(frames), det)
    # a call with one valid frame leaves slot 1's state untouched: afterwards slot 1 is still tracked at the hand
    trk.set_track(hand)
    one = trk.predict(frames[:1])
    assert one.xyz.shape == (1, J, 3)
    assert_same_prediction(one, tracked, rows=0)
    trk.reset_track(slots=[0])
    out = trk.predict(frames)
    assert_same_prediction(out, det, rows=0)
    assert_same_prediction(out, tracked, rows=1)
    # set_track on chosen slots
    trk.reset_track()
    trk.set_track(hand[1:], slots=[1])
    out = trk.predict(frames)
    assert_same_prediction(out, det, rows=0)
    assert_same_prediction(out, tracked, rows=1)
    # an explicit centers_uvd overrides the tracker
    trk.set_track(hand)
    other = np.array([(138.0, 98.0, 405.0), (22.0, 21.0, 398.0)])
    assert_same_prediction(trk.predict(frames, centers_uvd=other), auto.predict(frames, centers_uvd=other))
    # the tracker takes the joint centre of the call: next_centers_uvd for the valid slots
    trk.set_track(hand)
    trk.predict(frames)
    assert same_bits(trk._track, trk.next_centers_uvd)


def test_a_frame_with_no_hand(D, e2e):
    from awr_amd import _lib as L
    pred = e2e.make(recenter=1, track=True, **AUTO)
    want = pred.predict(e2e.frames)
    pred.check()
    want_codes = pred.recenter_codes.clone()
    empty = e2e.frames.copy()
    empty[1] = 0
    pred.reset_track()
    out = pred.predict(empty)
    with pytest.raises(L.AwrError, match=r"frame 1 .*AWR_DET_EMPTY"):
        pred.check()
    assert out.status.tolist() == [0, D.EMPTY]
    assert torch.isnan(out.xyz[1]).all() and torch.isnan(out.uvd[1]).all() and torch.isnan(out.center_xyz[1]).all()
    assert pred.recenter_codes[:, 1].tolist() == [D.KEPT_FRAME] * 2
    assert torch.isnan(pred.next_centers_uvd[1]).all() and torch.isnan(pred.centers_uvd[1]).all() and torch.isnan(pred._track[1]).all()
    assert_same_prediction(out, want, rows=0)
    assert pred.recenter_codes[:, 0].tolist() == want_codes[:, 0].tolist() and not torch.isnan(out.xyz[0]).any()
