"""CPU: the statement of the temporal joint filter (awr_amd/track.py filter_step) -- its properties as a filter, its gate
and coasting state machine, the confidence weight, the configuration rules and awr_joints_filter's argument validation (no launch) -- and
synthetic sequences (awr_amd/synth.py sample_sequences).

The bounds on smoothing and lag were fixed before this implementation ran, from a prototype of the same definition at the defaults and
30 fps: std ratio 0.44, jitter ratio 0.17, lags 5.8 / 4.8 / 4.2 mm."""
import ctypes as C

import numpy as np
import pytest

import track_cases as TC


@pytest.fixture(scope="module")
def T():
    import awr_amd  # noqa: F401
    from awr_amd import track
    return track


def chain(T, cfg, points, bad=(), **kw):
    return TC.run_chain(T, cfg, TC.single_joint_steps(points, bad), **kw)


def codes(rows):
    return [int(r[3][0, 0]) for r in rows]


def test_codes_have_names(T):
    assert (T.NONE, T.INIT, T.UPDATED, T.GATED, T.HELD, T.REINIT, T.LOST) == tuple(range(7))
    assert sorted(T.FILTER_NAMES) == list(range(7)) and all(isinstance(v, str) and v for v in T.FILTER_NAMES.values())
    state, count = T.filter_state(3, 14)
    assert state.shape == (3, 14, 6) and state.dtype == np.float64 and count.shape == (3, 14, 2) and count.dtype == np.int32
    assert not state.any() and not count.any()
    assert T.OneEuro() == T.OneEuro(1.0, 0.02, 1.0, 30.0, None, 5, None, 0.25, False)
    with pytest.raises(AttributeError):
        T.OneEuro().beta = 1.0


def test_constant_input_passes_unchanged(T):
    p = np.array([-31.25, 17.5, 640.125], np.float32)
    rows = chain(T, True, np.tile(p, (20, 1)))
    assert codes(rows) == [T.INIT] + [T.UPDATED] * 19
    fx, fy, u0, v0 = (np.float64(v) for v in TC.E_PARAS)
    x = p.astype(np.float64)
    uvd = np.array([x[0] * fx / x[2] + u0, (x[1] * np.float64(TC.FLIP)) * fy / x[2] + v0, x[2]]).astype(np.float32)
    for xyz_f, uvd_f, ahead, _, state, count in rows:
        assert TC.same_bits(xyz_f[0, 0], p) and TC.same_bits(ahead[0, 0], p) and TC.same_bits(uvd_f[0, 0], uvd)
        assert TC.same_bits(state[0, 0], np.concatenate([x, np.zeros(3)]))
    assert rows[-1][5].tolist() == [[[20, 0]]]


def test_a_static_joint_is_smoothed(T):
    rs = np.random.RandomState(11)
    nj, steps = 100, 300
    noisy = (np.array([10.0, -20.0, 600.0]) + rs.normal(0.0, 5.0, (steps, 1, nj, 3))).astype(np.float32)
    state, count = T.filter_state(1, nj)
    ok = np.zeros(1, np.int32)
    out = np.stack([T.filter_step(state, count, noisy[t], ok, ok, None, True, None, None, TC.E_PARAS, TC.FLIP)[0] for t in range(steps)])
    std_ratio = out[100:].astype(np.float64).std(0).mean() / noisy[100:].astype(np.float64).std(0).mean()
    jit = lambda a: np.abs(np.diff(a[100:].astype(np.float64), 2, axis=0)).mean()
    jitter_ratio = jit(out) / jit(noisy)
    print("std ratio %.3f, jitter ratio %.3f" % (std_ratio, jitter_ratio))
    assert std_ratio <= 0.6
    assert jitter_ratio <= 0.3


def test_lag_at_constant_velocity(T):
    v = np.array([600.0, -300.0, 200.0])
    pts = np.array([-500.0, 300.0, 500.0]) + v * (np.arange(300)[:, None] / 30.0)
    lags = {}
    for beta in (0.02, 0.1):
        rows = chain(T, dict(beta=beta), pts)
        assert set(codes(rows)[1:]) == {T.UPDATED}
        lags[beta] = (pts[-1].astype(np.float32).astype(np.float64) - rows[-1][0][0, 0].astype(np.float64)) * np.sign(v)
        print("beta %.2f: lag per axis %s mm" % (beta, np.round(lags[beta], 3).tolist()))
    assert (lags[0.02] > 0).all() and (lags[0.02] <= 8.0).all()
    assert (lags[0.1] > 0).all() and (lags[0.1] < lags[0.02]).all()
    # the look-ahead is ahead: at constant velocity it undoes most of the lag
    ahead = rows[-1][2][0, 0].astype(np.float64)
    assert (np.abs(pts[-1] + v / 30.0 - ahead) < np.abs(pts[-1] + v / 30.0 - rows[-1][0][0, 0])).all()


GATE = dict(gate_mm=60.0, max_coast=3)
HOME, AWAY = np.array([0.0, 0.0, 600.0]), np.array([150.0, 0.0, 600.0])


def test_gate_holds_a_single_outlier(T):
    pts = np.tile(HOME, (8, 1))
    pts[4] += (0.0, 200.0, 0.0)
    rows = chain(T, GATE, pts)
    assert codes(rows) == [T.INIT, T.UPDATED, T.UPDATED, T.UPDATED, T.GATED, T.UPDATED, T.UPDATED, T.UPDATED]
    assert TC.same_bits(rows[4][0], rows[3][0]) and TC.same_bits(rows[4][1], rows[3][1]) and TC.same_bits(rows[4][4], rows[3][4])
    assert rows[4][5].tolist() == [[[4, 1]]] and rows[5][5].tolist() == [[[5, 0]]]
    # exactly at the gate is inside it: |y| = 60 is taken, the next float32 is not (along x, where HOME is 0 and both are representable)
    for d, want in ((60.0, T.UPDATED), (float(np.nextafter(np.float32(60.0), np.float32(100.0))), T.GATED)):
        assert codes(chain(T, GATE, [HOME, HOME + (d, 0.0, 0.0)]))[1] == want
    # without a gate the outlier is filtered in
    assert codes(chain(T, dict(max_coast=3), pts))[4] == T.UPDATED


def test_gate_follows_a_permanent_jump(T):
    rows = chain(T, GATE, [HOME] * 3 + [AWAY] * 6)
    assert codes(rows) == [T.INIT, T.UPDATED, T.UPDATED, T.GATED, T.GATED, T.GATED, T.REINIT, T.UPDATED, T.UPDATED]
    for r in rows[3:6]:
        assert TC.same_bits(r[0][0, 0], HOME.astype(np.float32))
    assert TC.same_bits(rows[6][0][0, 0], AWAY.astype(np.float32)) and rows[6][5].tolist() == [[[1, 0]]]
    assert TC.same_bits(rows[6][4][0, 0], np.concatenate([AWAY, np.zeros(3)]))
    # max_coast = 0 re-initialises at once
    assert codes(chain(T, dict(gate_mm=60.0, max_coast=0), [HOME, HOME, AWAY, AWAY])) == [T.INIT, T.UPDATED, T.REINIT, T.UPDATED]


def test_coasting_over_bad_frames(T):
    # three bad frames: held, and the track goes on
    rows = chain(T, GATE, [HOME] * 8, bad=(3, 4, 5))
    assert codes(rows) == [T.INIT, T.UPDATED, T.UPDATED, T.HELD, T.HELD, T.HELD, T.UPDATED, T.UPDATED]
    for r in rows[3:6]:
        assert TC.same_bits(r[0], rows[2][0]) and TC.same_bits(r[1], rows[2][1]) and TC.same_bits(r[2], rows[2][2])
    assert [r[5][0, 0].tolist() for r in rows[2:7]] == [[3, 0], [3, 1], [3, 2], [3, 3], [4, 0]]
    # four or more: lost, NaN, nothing, and a new track when the frames return
    rows = chain(T, GATE, [HOME] * 10, bad=(2, 3, 4, 5, 6, 7))
    assert codes(rows) == [T.INIT, T.UPDATED, T.HELD, T.HELD, T.HELD, T.LOST, T.NONE, T.NONE, T.INIT, T.UPDATED]
    for r in rows[5:8]:
        assert all(np.isnan(r[k]).all() for k in (0, 1, 2)) and not r[4].any() and not r[5].any()
    assert rows[8][5].tolist() == [[[1, 0]]]
    # a non-finite coordinate is a bad measurement of that joint alone; an un-projection code is a bad frame
    pts = np.tile(HOME, (4, 1))
    pts[2, 1] = np.inf
    assert codes(chain(T, GATE, pts)) == [T.INIT, T.UPDATED, T.HELD, T.UPDATED]
    steps = TC.single_joint_steps([HOME] * 3)
    steps[1][2][0] = 2
    assert [int(r[3][0, 0]) for r in TC.run_chain(T, GATE, steps)] == [T.INIT, T.HELD, T.UPDATED]
    # a joint that never had a measurement
    assert codes(chain(T, GATE, [[np.nan, 0.0, 600.0]] * 3)) == [T.NONE] * 3


def test_confidence_weight(T):
    steps = TC.scenario(2, 5, T=12, seed=4)

    def with_conf(value):
        return [(x, s, u, np.full_like(c, value)) for x, s, u, c in steps]

    def final(cfg, st):
        rows = TC.run_chain(T, cfg, st)
        return [r[0] for r in rows], rows[-1][4]
    plain = final(dict(), steps)
    one = final(dict(weight="conf"), with_conf(1.0))
    above = final(dict(weight="conf"), with_conf(1.5))
    assert all(TC.same_bits(a, b) for a, b in zip(plain[0], one[0])) and TC.same_bits(plain[1], one[1])
    assert all(TC.same_bits(a, b) for a, b in zip(plain[0], above[0])) and TC.same_bits(plain[1], above[1])
    floor = final(dict(weight="conf"), with_conf(0.25))
    for value in (np.nan, 0.1, -3.0, -np.inf):
        got = final(dict(weight="conf"), with_conf(value))
        assert all(TC.same_bits(a, b) for a, b in zip(floor[0], got[0])) and TC.same_bits(floor[1], got[1]), value
    assert not TC.same_bits(floor[1], plain[1])
    half = final(dict(weight="conf", conf_floor=0.5), with_conf(0.3))
    assert TC.same_bits(half[1], final(dict(weight="conf"), with_conf(0.5))[1]) and not TC.same_bits(half[1], floor[1])
    with pytest.raises(ValueError, match="conf"):
        T.filter_step(*T.filter_state(2, 5), steps[0][0], steps[0][1], steps[0][2], None, dict(weight="conf"))


def test_rows_past_n_valid_keep_their_state(T):
    steps = TC.scenario(3, 4, T=6, seed=9)
    state, count = T.filter_state(3, 4)
    rs = np.random.RandomState(2)
    state[2], count[2] = rs.uniform(-5, 5, (4, 6)), rs.randint(1, 4, (4, 2))
    keep = state[2].copy(), count[2].copy()
    full = TC.run_chain(T, True, [tuple(a[:2] for a in s) for s in steps])
    part = TC.run_chain(T, True, steps, n_valid=2, state=state, count=count)
    for f, p in zip(full, part):
        assert all(TC.same_bits(f[k], p[k][:2]) for k in range(6))
        assert TC.same_bits(p[4][2], keep[0]) and TC.same_bits(p[5][2], keep[1])
    # n_valid = 0: nothing moves
    before = state.copy(), count.copy()
    T.filter_step(state, count, *steps[0], True, None, 0)
    assert TC.same_bits(state, before[0]) and TC.same_bits(count, before[1])


def test_the_scenario_reaches_every_code(T):
    """the generator the GPU test compares over: with a gate every code occurs, without one all but GATED / REINIT"""
    steps = TC.scenario(3, 4, seed=1)
    seen = lambda cfg: set(np.unique(np.concatenate([r[3].ravel() for r in TC.run_chain(T, cfg, steps)])).tolist())
    assert seen(dict(gate_mm=60.0)) == set(range(7))
    assert seen(dict()) == {T.NONE, T.INIT, T.UPDATED, T.HELD, T.LOST}
    one = TC.scenario(1, 1, seed=1)
    assert {T.INIT, T.UPDATED, T.GATED, T.HELD, T.REINIT, T.LOST, T.NONE} == set(
        int(r[3][0, 0]) for r in TC.run_chain(T, dict(gate_mm=60.0), one))


@pytest.mark.parametrize("bad, err", [
    (dict(min_cutoff=0.0), ValueError), (dict(min_cutoff=float("nan")), ValueError), (dict(beta=-0.1), ValueError),
    (dict(d_cutoff=0.0), ValueError), (dict(fps=0.0), ValueError), (dict(fps=float("inf")), ValueError), (dict(gate_mm=0.0), ValueError),
    (dict(gate_mm=-1.0), ValueError), (dict(gate_mm=float("nan")), ValueError), (dict(max_coast=-1), ValueError),
    (dict(max_coast=1.5), TypeError), (dict(max_coast=True), TypeError), (dict(weight="peak"), ValueError), (dict(conf_floor=0.0), ValueError),
    (dict(conf_floor=1.5), ValueError), (dict(lead=1), TypeError), (dict(beta="0.1"), TypeError), (dict(cutoff=1.0), ValueError)])
def test_check_filter_rejects(T, bad, err):
    with pytest.raises(err):
        T.check_filter(bad)


def test_check_filter_accepts(T):
    assert T.check_filter(True) == T.OneEuro()
    assert T.check_filter(dict(beta=0, gate_mm=60, max_coast=np.int64(2), conf_floor=1)) == T.OneEuro(beta=0.0, gate_mm=60.0, max_coast=2, conf_floor=1.0)
    cfg = T.OneEuro(weight="conf", lead=True)
    assert T.check_filter(cfg) == cfg
    for bad in (None, False, 1.0, "on", (1.0, 0.02)):
        with pytest.raises(TypeError):
            T.check_filter(bad)
    for bad_dt in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            T.filter_step(*T.filter_state(1, 1), np.zeros((1, 1, 3), np.float32), [0], [0], None, True, bad_dt)


def test_entry_point_validates_before_any_launch(T):
    """awr_joints_filter's argument rules: AWR_ERR_ARG with a message and no HIP call, so a machine without a GPU can check them.  The
    pointers are host buffers that a refused call never reads."""
    from awr_amd import _lib as L
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    good = dict(state=p, count=p, xyz=p, status=p, ustatus=p, conf=None, B=2, J=14, n_valid=2, dt=1 / 30.0, min_cutoff=1.0, beta=0.02,
                d_cutoff=1.0, gate_mm=-1.0, max_coast=5, weight=0, conf_floor=0.25, fx=588.0, fy=587.0, u0=320.0, v0=240.0, flip=-1, xyz_out=p,
                uvd_out=p, ahead_out=p, code=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.lib.awr_joints_filter(*[a[k] for k in good])
    for name in ("state", "count", "xyz", "status", "ustatus", "xyz_out", "uvd_out", "ahead_out", "code"):
        assert call(**{name: None}) == -1 and "NULL" in L.last_error(), name
    assert call(weight=1) == -1 and "conf" in L.last_error()
    for kw, word in ((dict(J=0), "J ="), (dict(J=257), "J ="), (dict(B=0), "B ="), (dict(n_valid=-1), "n_valid"), (dict(n_valid=3), "n_valid"),
                     (dict(dt=0.0), "dt"), (dict(dt=-0.1), "dt"), (dict(dt=float("nan")), "dt"), (dict(dt=float("inf")), "dt"),
                     (dict(min_cutoff=0.0), "min_cutoff"), (dict(min_cutoff=float("nan")), "min_cutoff"), (dict(beta=-1.0), "beta"),
                     (dict(beta=float("nan")), "beta"), (dict(d_cutoff=0.0), "d_cutoff"), (dict(gate_mm=0.0), "gate_mm"),
                     (dict(gate_mm=float("nan")), "gate_mm"), (dict(max_coast=-1), "max_coast"), (dict(conf_floor=0.0), "conf_floor"),
                     (dict(conf_floor=1.25), "conf_floor"), (dict(conf_floor=float("nan")), "conf_floor"), (dict(weight=2), "weight"),
                     (dict(flip=0), "flip"), (dict(flip=2), "flip"), (dict(fx=0.0), "focal"), (dict(fy=0.0), "focal")):
        assert call(**kw) == -1 and word in L.last_error(), (kw, L.last_error())
    # n_valid = 0 is valid and launches nothing
    assert call(n_valid=0) == 0
    assert call(n_valid=0, gate_mm=60.0, weight=1, conf=p, J=256, B=1 << 20) == 0
    assert call(n_valid=0, B=(1 << 20) + 1) == -1 and "B =" in L.last_error()


def test_predict_py_smoothing_options(T):
    import predict
    base = ["frames.npy", "--load-model", "x.pth"]
    cfg = lambda *argv: predict.smooth_config(predict.parse_args(base + list(argv)))
    assert cfg() is None and cfg("--smooth") == {}
    assert cfg("--smooth", "0.5,0.1,2", "--fps", "60", "--gate-mm", "50", "--lead", "--track") == dict(
        min_cutoff=0.5, beta=0.1, d_cutoff=2.0, fps=60.0, gate_mm=50.0, lead=True)
    assert T.check_filter(cfg("--smooth", "0.5,0.1,2", "--fps", "60")) == T.OneEuro(min_cutoff=0.5, beta=0.1, d_cutoff=2.0, fps=60.0)
    for bad in (["--lead"], ["--fps", "60"], ["--gate-mm", "40"], ["--smooth", "1,2"], ["--smooth", "a,b,c"]):
        with pytest.raises(SystemExit):
            cfg(*bad)


# ---- synthetic sequences ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    import awr_amd  # noqa: F401
    from awr_amd import synth
    return synth


def test_sequences_are_deterministic_and_pass_through_their_keys(S):
    n_seq, length, ke = 3, 32, 15
    a = S.sample_sequences(n_seq, length, 7, key_every=ke)
    b = S.sample_sequences(n_seq, length, 7, key_every=ke)
    K = (length - 2) // ke + 2
    keys = S.sample_poses(n_seq * K, 7, rot_range=(50.0, 50.0, 60.0))
    assert K == 4 and sorted(a) == sorted(keys)
    for name in keys:
        assert a[name].shape == (n_seq * length,) + keys[name].shape[1:] and a[name].dtype == np.float64
        assert np.array_equal(a[name], b[name])
        for s in range(n_seq):
            for k in range(0, (length - 1) // ke + 1):
                assert np.array_equal(a[name][s * length + k * ke], keys[name][s * K + k]), (name, s, k)           # sequence-major, key on key
        # between two keys every field lies between them
        lo, hi = np.minimum(keys[name][0], keys[name][1]), np.maximum(keys[name][0], keys[name][1])
        assert (a[name][1:ke] >= lo - 1e-9).all() and (a[name][1:ke] <= hi + 1e-9).all()
    assert not np.array_equal(S.sample_sequences(n_seq, length, 8, key_every=ke)["flex"], a["flex"])
    # consecutive frames are close, frames of different sequences are not
    j = S.forward_kinematics(a)[0]
    step = np.linalg.norm(np.diff(j.reshape(n_seq, length, 21, 3), axis=1), axis=-1)
    assert 0 < step.max() < 60.0
    # a length that ends ON a key, and the shortest sequences
    c = S.sample_sequences(2, 31, 7, key_every=15)
    k3 = S.sample_poses(2 * 3, 7, rot_range=(50.0, 50.0, 60.0))
    assert np.array_equal(c["euler"][30], k3["euler"][2]) and np.array_equal(c["euler"][31 + 15], k3["euler"][3 + 1])
    assert len(S.sample_sequences(2, 1, 7)["scale"]) == 2 and len(S.sample_sequences(1, 2, 7, key_every=1)["scale"]) == 2
    with pytest.raises(ValueError):
        S.sample_sequences(0, 10, 7)


def test_interpolated_angles_stay_in_the_models_ranges(S):
    m = S.HandModel()
    p = S.sample_sequences(8, 40, 3, key_every=8)
    for f in range(5):
        rng = m.THUMB_FLEX if f == S.THUMB else m.FLEX
        for k in range(3):
            assert (p["flex"][:, f, k] >= rng[k][0]).all() and (p["flex"][:, f, k] <= rng[k][1]).all()
    assert (p["abduct"] >= m.ABDUCT[0]).all() and (p["abduct"] <= m.ABDUCT[1]).all()
    for k in range(2):
        assert (p["thumb_base"][:, k] >= m.THUMB_BASE[k][0]).all() and (p["thumb_base"][:, k] <= m.THUMB_BASE[k][1]).all()
    assert (np.abs(p["euler"]) <= (50.0, 50.0, 60.0)).all()


def test_sequence_frames_render(S):
    shape, paras = (48, 64), tuple(0.1 * v for v in S.ND.PARAS)
    p = S.sample_sequences(1, 9, 5, key_every=4, frame_shape=shape, paras=paras)
    joints, prims, bbox = S.forward_kinematics(p, frame_shape=shape, paras=paras)
    lab, centers = S.labels(joints)
    assert lab.shape == (9, 14, 3) and centers.shape == (9, 3)
    rows = [0, 3, 8]
    frames, status = S.render(prims[rows], bbox[rows], shape, paras=paras, return_status=True)
    assert status.tolist() == [S.OK] * 3 and (frames > 0).any(axis=(1, 2)).all()
    assert not np.array_equal(frames[0], frames[2])


def test_synthetic_frames_take_given_poses(S):
    shape, paras = (48, 64), tuple(0.1 * v for v in S.ND.PARAS)
    kw = dict(img_size=32, frame_shape=shape, paras=paras, device=None)
    own = S.SyntheticFrames(3, 21, "test", **kw)
    given = S.SyntheticFrames(3, 21, "test", poses=S.sample_poses(3, 21, frame_shape=shape, paras=paras), **kw)
    assert np.array_equal(own.frames, given.frames) and np.array_equal(own.labels_xyz, given.labels_xyz)
    assert np.array_equal(own.centers, given.centers) and all(np.array_equal(own.poses[k], given.poses[k]) for k in own.poses)
    seq = S.sample_sequences(1, 3, 5, key_every=2, frame_shape=shape, paras=paras)
    sf = S.SyntheticFrames(3, 0, "test", poses=seq, **kw)
    assert sf.frames.shape == (3,) + shape and np.array_equal(sf.joints21, S.forward_kinematics(seq, frame_shape=shape, paras=paras)[0])
    with pytest.raises(ValueError, match="rows"):
        S.SyntheticFrames(4, 0, "test", poses=seq, **kw)
    with pytest.raises(ValueError, match="poses="):
        S.SyntheticFrames(3, 0, "test", poses=seq, edge=True, **kw)
