"""GPU: the temporal joint filter -- awr_joints_filter against awr_amd.track.filter_step bit for bit over chained
scenarios whose state never leaves the device, and awr_amd.Predictor(smooth=...) against compositions of plain predictors and the
statement."""
import types

import numpy as np
import pytest
import torch

import track_cases as TC
from test_recenter_gpu import AUTO, CUBE, E_PARAS, EH, EW, FLIP, J, S, blob_frames

pytestmark = pytest.mark.gpu
same_bits = TC.same_bits


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import awr_amd  # noqa: F401
    from awr_amd import track
    return track


# ---- the operator -----------------------------------------------------------------------------------------------------------------------
SHAPES = {"two_workgroups": (20, 21, None), "n_valid": (3, 14, 2), "one_thread": (1, 1, None)}
CONFIGS = {"plain": (dict(), None), "gate": (dict(gate_mm=60.0), None), "conf": (dict(weight="conf"), 0.011),
           "gate_conf_dt": (dict(gate_mm=60.0, weight="conf", beta=0.05, min_cutoff=0.7, d_cutoff=1.5, conf_floor=0.4, max_coast=5), 0.011)}
_SCENARIOS = {}


def scenario(shape):
    if shape not in _SCENARIOS:
        B, nj, _ = SHAPES[shape]
        _SCENARIOS[shape] = TC.scenario(B, nj, T=48, seed=len(shape))
    return _SCENARIOS[shape]


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_filter_equals_the_statement_at_every_step(T, dev, shape, config):
    B, nj, nv = SHAPES[shape]
    cfg, dt = CONFIGS[config]
    steps = scenario(shape)
    state, count = T.filter_state(B, nj)
    if nv is not None:                  # the slots past n_valid hold a track of their own, which no step may touch
        rs = np.random.RandomState(5)
        state[nv:], count[nv:] = rs.uniform(-300, 300, state[nv:].shape), rs.randint(1, 9, count[nv:].shape)
    d_state, d_count = torch.from_numpy(state).to(dev), torch.from_numpy(count).to(dev)          # uploaded once, never again
    rows = slice(0, nv)
    seen = set()
    for t, (xyz, status, ustatus, conf) in enumerate(steps):
        want = T.filter_step(state, count, xyz, status, ustatus, conf, cfg, dt, nv, E_PARAS, FLIP)
        got = T.filter_step_device(d_state, d_count, *(torch.from_numpy(a).to(dev) for a in (xyz, status, ustatus, conf)), cfg, dt, nv,
                                   E_PARAS, FLIP)
        for g, w, name in zip(got, want, ("xyz_f", "uvd_f", "ahead", "code")):
            assert same_bits(g[rows], w[rows]), (t, name, g[rows].cpu().numpy(), w[rows])
        assert same_bits(d_state, state), (t, "state")
        assert same_bits(d_count, count), (t, "count")
        seen |= set(np.unique(want[3][rows]).tolist())
    assert got[0].dtype == torch.float32 and got[3].dtype == torch.int32
    # what the comparison covered (the statement's own codes: tests/test_track_cpu.py checks the generator reaches them)
    assert seen >= {T.NONE, T.INIT, T.UPDATED, T.HELD, T.LOST} and (("gate_mm" in cfg) == (T.GATED in seen)) and (("gate_mm" in cfg) == (T.REINIT in seen))


def test_filter_leaves_rows_past_n_valid_alone(T, dev):
    B, nj, nv = 3, 14, 2
    xyz, status, ustatus, conf = (torch.from_numpy(a).to(dev) for a in scenario("n_valid")[0])
    state, count = T.filter_state_device(B, nj, dev)
    out = tuple(torch.full((B, nj, 3), -7.0, dtype=torch.float32, device=dev) for _ in range(3)) + (torch.full((B, nj), -7, dtype=torch.int32, device=dev),)
    got = T.filter_step_device(state, count, xyz, status, ustatus, conf, True, None, nv, E_PARAS, FLIP, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    assert all(bool((o[nv:] == -7).all()) for o in out) and not state[nv:].any() and not count[nv:].any()
    assert (count[:nv, :-1, 0] == 1).all() and (got[3][:nv, :-1] == T.INIT).all()
    # n_valid = 0: no launch, nothing changes; bad arguments are refused by name
    before = state.clone()
    T.filter_step_device(state, count, xyz, status, ustatus, conf, True, None, 0, E_PARAS, FLIP)
    assert same_bits(state, before)
    from awr_amd import _lib as L
    with pytest.raises(L.AwrError, match="n_valid"):
        T.filter_step_device(state, count, xyz, status, ustatus, conf, True, None, B + 1, E_PARAS, FLIP)


# ---- the Predictor ----------------------------------------------------------------------------------------------------------------------
FIELDS = ("uvd", "xyz", "M", "center_xyz", "status")


@pytest.fixture(scope="module")
def e2e(dev):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()

    def make(**kw):
        return awr_amd.Predictor(net, S, 1.0, cube=CUBE, paras=E_PARAS, flip=FLIP, max_batch=2, frame_shape=(EH, EW), **kw)
    frames = blob_frames()
    moved = blob_frames(hands=((64, 53), (97, 68)))          # the same hands a few pixels on: another measurement for the filter
    empty0 = frames.copy()
    empty0[0] = 0
    # five calls: two plain, one with frame 0 empty, one with one valid frame, one plain
    calls = [dict(frames=frames), dict(frames=moved), dict(frames=empty0), dict(frames=moved[:1]), dict(frames=frames)]
    return types.SimpleNamespace(net=net, make=make, frames=frames, moved=moved, calls=calls)


def host_step(T, cfg, state, count, raw_xyz, status, ustatus, conf, nb, dt=None):
    """filter_step fed one call's raw joints and codes; the rows past nb keep their state"""
    B = state.shape[0]
    xyz = np.full((B, J, 3), np.nan, np.float32)
    xyz[:nb] = raw_xyz.cpu().numpy()
    st, ust = np.ones(B, np.int32), np.ones(B, np.int32)
    st[:nb], ust[:nb] = status[:nb].cpu().numpy(), ustatus[:nb].cpu().numpy()
    cf = None
    if conf is not None:
        cf = np.full((B, J), np.nan, np.float32)
        cf[:nb] = conf[:nb].cpu().numpy()
    return T.filter_step(state, count, xyz, st, ust, cf, cfg, dt, nb, E_PARAS, FLIP)


def assert_filtered(out, pred, want, nb, tag):
    for g, w, name in ((out.xyz, want[0], "xyz"), (out.uvd, want[1], "uvd"), (pred.ahead_xyz, want[2], "ahead_xyz"), (pred.filter_codes, want[3], "codes")):
        assert tuple(g.shape) == w[:nb].shape and same_bits(g, w[:nb]), (tag, name, g.cpu().numpy(), w[:nb])


def test_smooth_none_changes_nothing(e2e):
    from awr_amd import _lib as L
    a, b = e2e.make(confidence=True, **AUTO), e2e.make(confidence=True, smooth=None, **AUTO)
    for kw in e2e.calls:
        x, y = a.predict(**kw), b.predict(**kw)
        for f in FIELDS + ("conf", "peak", "spread_mm"):
            assert same_bits(getattr(x, f), getattr(y, f)), f
    assert b.smooth is None
    assert not any(name.startswith("_filter") or name in ("raw_xyz", "raw_uvd", "ahead_xyz", "filter_codes") for name in vars(b))
    assert not any(hasattr(b, name) for name in ("raw_xyz", "raw_uvd", "ahead_xyz", "filter_codes", "_filter_state", "_filter_count"))
    with pytest.raises(L.AwrError, match="smooth"):
        b.predict(e2e.frames, dt=1 / 30.0)
    with pytest.raises(L.AwrError, match="smooth"):
        b.reset_smooth()


@pytest.mark.parametrize("cfg, dt", [(True, None), (dict(gate_mm=25.0, max_coast=1, beta=0.05), 0.02)])
def test_smoothed_predictor_equals_its_composition(T, e2e, cfg, dt):
    plain, smooth = e2e.make(**AUTO), e2e.make(smooth=cfg, **AUTO)
    assert smooth.smooth == T.check_filter(cfg) and smooth.raw_xyz is None
    state, count = T.filter_state(2, J)
    differs, codes = False, []
    kw_dt = {} if dt is None else dict(dt=dt)
    for i, kw in enumerate(e2e.calls):
        ref = plain.predict(**kw)
        out = smooth.predict(**kw, **kw_dt)
        nb = ref.xyz.shape[0]
        assert type(out).__name__ == "Prediction"
        assert same_bits(smooth.raw_xyz, ref.xyz) and same_bits(smooth.raw_uvd, ref.uvd)
        for f in ("M", "center_xyz", "status"):
            assert same_bits(getattr(out, f), getattr(ref, f)), f
        want = host_step(T, cfg, state, count, ref.xyz, ref.status, plain._last[1], None, nb, dt)
        assert_filtered(out, smooth, want, nb, i)
        assert same_bits(smooth._filter_state, state) and same_bits(smooth._filter_count, count)
        differs |= not same_bits(out.xyz, ref.xyz)
        codes.append(want[3][:nb, 0].tolist())
    assert differs                      # the filter did something: the comparison is not about raw joints passed through
    print("codes of joint 0 per call:", codes)
    # the empty frame of call 2 coasts: held while max_coast allows (the default always does here), else the track is dropped
    assert codes[0] == [T.INIT, T.INIT] and codes[2][0] in ((T.HELD,) if cfg is True else (T.HELD, T.LOST)) and len(codes[3]) == 1
    # the empty frame is still reported, and its joints are the held ones
    out = smooth.predict(**e2e.calls[2], **kw_dt)
    with pytest.raises(Exception, match="frame 0 .*AWR_DET_EMPTY"):
        smooth.check()
    assert out.status.tolist()[0] != 0 and torch.isnan(smooth.raw_xyz[0]).all()
    want = host_step(T, cfg, state, count, smooth.raw_xyz, out.status, smooth._last[1], None, 2, dt)
    assert_filtered(out, smooth, want, 2, "empty again")
    held = smooth.filter_codes[0] == T.HELD
    assert bool(((smooth.filter_codes[0] == T.LOST) | held).all()) and bool((torch.isnan(out.xyz[0]).any(1) == ~held).all())
    if cfg is True:                     # five calls of coasting are allowed and the call before was a good one: every joint is held
        assert bool(held.all()) and not torch.isnan(out.uvd[0]).any()
    # reset_smooth(slots=[0]): slot 0 starts again, slot 1 goes on
    smooth.reset_smooth(slots=[0])
    state[0], count[0] = 0.0, 0
    assert same_bits(smooth._filter_state, state) and same_bits(smooth._filter_count, count)
    ref, out = plain.predict(e2e.frames), smooth.predict(e2e.frames, **kw_dt)
    want = host_step(T, cfg, state, count, ref.xyz, ref.status, plain._last[1], None, 2, dt)
    assert_filtered(out, smooth, want, 2, "after reset")
    assert (smooth.filter_codes[0] == T.INIT).all() and not (smooth.filter_codes[1] == T.INIT).any()
    smooth.reset_smooth()
    assert not smooth._filter_state.any() and not smooth._filter_count.any()


def test_conf_weight_without_confidence_fields(T, e2e):
    cfg = dict(weight="conf", conf_floor=0.05)
    conf_pred, smooth = e2e.make(confidence=True, **AUTO), e2e.make(smooth=cfg, **AUTO)
    unweighted = e2e.make(smooth=dict(), **AUTO)
    assert smooth.engine.confidence and not smooth.confidence
    state, count = T.filter_state(2, J)
    differs = False
    for i, kw in enumerate(e2e.calls):
        ref, out, other = conf_pred.predict(**kw), smooth.predict(**kw), unweighted.predict(**kw)
        nb = ref.xyz.shape[0]
        assert type(out).__name__ == "Prediction" and same_bits(smooth.raw_xyz, ref.xyz)
        want = host_step(T, cfg, state, count, ref.xyz, ref.status, conf_pred._last[1], ref.conf, nb)
        assert_filtered(out, smooth, want, nb, i)
        differs |= not same_bits(out.xyz, other.xyz)
    assert differs                      # the weight took part
    # with confidence=True as well the fields stay the measurement's
    both = e2e.make(confidence=True, smooth=cfg, **AUTO)
    ref, out = conf_pred.predict(e2e.frames), both.predict(e2e.frames)
    assert type(out).__name__ == "ConfidentPrediction"
    for f in ("conf", "peak", "spread_mm", "M", "center_xyz", "status"):
        assert same_bits(getattr(out, f), getattr(ref, f)), f


def test_lead_moves_the_tracker_to_the_look_ahead(T, e2e):
    from awr_amd import detect as D
    with pytest.raises(ValueError, match="track=True"):
        e2e.make(smooth=dict(lead=True), **AUTO)
    open_gate = dict(AUTO, max_shift=1e9)          # the shift gate open: a centre moves wherever its joints' mean is finite and in depth range
    lead, trk = e2e.make(track=True, smooth=dict(lead=True), **open_gate), e2e.make(track=True, smooth=dict(), **open_gate)
    differs = False
    for kw in (dict(frames=e2e.frames), dict(frames=e2e.moved), dict(frames=e2e.frames)):
        out, other = lead.predict(**kw), trk.predict(**kw)
        nb = out.xyz.shape[0]
        cube = np.tile(np.float32(CUBE), (nb, 1))
        for p, o, joints in ((lead, out, lead.ahead_xyz), (trk, other, trk.raw_xyz)):
            want = D.joints_center(joints.cpu().numpy(), p.centers_uvd.cpu().numpy(), o.center_xyz.cpu().numpy(), cube, o.status.cpu().numpy(),
                                   p._last[1][:nb].cpu().numpy(), E_PARAS, FLIP, depth_range=AUTO["depth_range"], max_shift=1e9)
            assert same_bits(p._track, want[1]) and same_bits(p.next_centers_uvd, want[1]) and p.recenter_codes[-1].tolist() == want[2].tolist()
        print("codes:", lead.recenter_codes.tolist(), trk.recenter_codes.tolist())
        differs |= not same_bits(lead._track, trk._track)
    assert differs                      # after a call with motion the look-ahead centre is another centre


def test_views_feed_the_fused_joints(T, e2e):
    from awr_amd import detect as D
    views = D.make_views(rot=(-15, 15))
    ref_pred, smooth = e2e.make(views=views, **AUTO), e2e.make(views=views, smooth=dict(weight="conf"), **AUTO)
    state, count = T.filter_state(2, J)
    for i, kw in enumerate(e2e.calls[:2]):
        ref, out = ref_pred.predict(**kw), smooth.predict(**kw)
        assert type(out).__name__ == "ViewPrediction"
        assert same_bits(smooth.raw_xyz, ref.xyz) and same_bits(smooth.raw_uvd, ref.uvd)
        for f in ("M", "center_xyz", "status", "view_spread_mm", "views_used"):
            assert same_bits(getattr(out, f), getattr(ref, f)), f
        want = host_step(T, dict(weight="conf"), state, count, ref.xyz, ref.status, ref_pred._last[1], smooth.view_outputs.conf[0], 2)
        assert_filtered(out, smooth, want, 2, i)
    assert not same_bits(out.xyz, ref.xyz)
