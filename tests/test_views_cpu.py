"""CPU: test-time views -- the validation of views / fuse, the argument checks of awr_view_centers / awr_view_rotate /
awr_views_fuse, the direction of a view's rotation against a host rendering, the algebra of M_v = R . M, and the statement fuse_views on
hand-made cases (no compute calls -- there is no GPU here)."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PARAS, FLIP = (147.0, 146.8, 80.0, 60.0), -1                # NYU's intrinsics scaled to a 160 x 120 frame
EH, EW, S, CUBE = 120, 160, 64, np.array([300.0, 300.0, 300.0])
MODES = ("mean", "conf", "median")


@pytest.fixture(scope="module")
def lib():
    import awr_amd  # noqa: F401
    from awr_amd import build
    if not os.path.exists(build.LIB):
        build.build_lib(verbose=False)
    from awr_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


@pytest.fixture(scope="module")
def ND():
    import awr_amd  # noqa: F401
    from awr_amd import nyu_data
    return nyu_data


# ---- validation -------------------------------------------------------------------------------------------------------------------------
IDENT = dict(rot=0.0, scale=1.0, shift=(0.0, 0.0, 0.0))
BAD_VIEWS = [
    [dict(rot=5.0), IDENT],                                           # view 0 is not the identity
    [dict(scale=1.1), IDENT],
    [dict(shift=(0, 0, 1)), IDENT],
    [IDENT],                                                          # V = 1
    [IDENT] + [dict(rot=float(k)) for k in range(1, 9)],              # V = 9
    [IDENT, dict(rot=float("nan"))],
    [IDENT, dict(rot=float("inf"))],
    [IDENT, dict(scale=0.0)],
    [IDENT, dict(scale=-1.0)],
    [IDENT, dict(scale=float("inf"))],
    [IDENT, dict(shift=(0.0, float("nan"), 0.0))],
    [IDENT, dict(rotation=3.0)],
]


def test_views_and_fuse_are_validated(D, lib, monkeypatch):
    import torch
    import awr_amd
    for bad in BAD_VIEWS:
        with pytest.raises(ValueError):
            D.check_views(bad)
    for bad in (5, "rot=5", [IDENT, 7], [IDENT, dict(rot="5")], [IDENT, dict(scale=True)], [IDENT, dict(shift=5.0)], [IDENT, (1.0, 2.0)]):
        with pytest.raises(TypeError):
            D.check_views(bad)
    with pytest.raises(ValueError, match="fuse"):
        D.check_views([IDENT, dict(rot=5.0)], "mode")
    # make_views: the identity first, then a view per rotation, per scale, per shift
    views = D.make_views(rot=(-15, 15), scale=(0.9,), shift=((0, 0, 10),))
    assert views == [IDENT, dict(rot=-15.0, scale=1.0, shift=(0.0, 0.0, 0.0)), dict(rot=15.0, scale=1.0, shift=(0.0, 0.0, 0.0)),
                     dict(rot=0.0, scale=0.9, shift=(0.0, 0.0, 0.0)), dict(rot=0.0, scale=1.0, shift=(0.0, 0.0, 10.0))]
    assert D.check_views(views) == D.check_views([(v["rot"], v["scale"], v["shift"]) for v in views])
    assert len(D.make_views(rot=range(1, 8))) == D.MAX_VIEWS == 8
    for bad in (dict(), dict(rot=range(1, 9)), dict(rot=(float("nan"),)), dict(scale=(0.0,)), dict(scale=(-2.0,)), dict(shift=((0, 1),))):
        with pytest.raises((ValueError, TypeError)):
            D.make_views(**bad)
    with pytest.raises(ValueError):
        D.make_views()                                                # V = 1
    with pytest.raises(ValueError):
        D.make_views(rot=range(1, 9))                                 # V = 9
    assert D.parse_views("rot=-15,15; scale=0.9 ;shift=0:0:10") == views
    for bad in ("rot", "rot=", "tilt=3", "rot=1;rot=2", "rot=a"):
        with pytest.raises(ValueError):
            D.parse_views(bad)
    # the constructor: the same checks, before the GPU check and before any plan
    net = awr_amd.get_deconv_net(18, 14, 2)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for bad in BAD_VIEWS:
        with pytest.raises(ValueError):
            awr_amd.Predictor(net, 128, 0.4, views=bad)
    with pytest.raises(TypeError):
        awr_amd.Predictor(net, 128, 0.4, views="rot=5")
    for kw in (dict(fuse="mode"), dict(views=views, fuse="max"), dict(fuse=None)):
        with pytest.raises(ValueError, match="fuse"):
            awr_amd.Predictor(net, 128, 0.4, **kw)
    with pytest.raises(lib.AwrError, match=r"detect\.detect"):       # valid options get as far as the GPU check
        awr_amd.Predictor(net, 128, 0.4, views=views, fuse="median")


def test_entry_points_validate_their_arguments_before_any_hip_call(lib):
    p = 1 << 12

    def centers(ptr=p, V=3, B=4, n=4, stride=0, fx=588.03, flip=-1, out=p):
        return lib.lib.awr_view_centers(ptr, ptr, ptr, stride, ptr, V, B, n, fx, 587.07, 320.0, 240.0, flip, out, out, out, out, None)

    def rotate(ptr=p, V=3, B=4, n=4):
        return lib.lib.awr_view_rotate(ptr, ptr, ptr, ptr, V, B, n, None)

    def fuse(ptr=p, w=p, mode=0, V=3, B=4, J=14, n=4, fx=588.03, flip=-1, out=p):
        return lib.lib.awr_views_fuse(ptr, ptr, ptr, w, mode, V, B, J, n, fx, 587.07, 320.0, 240.0, flip, out, out, out, out, None)
    for f in (centers, rotate, fuse):
        assert f(ptr=None) == -1 and "NULL" in lib.last_error()
        assert f(V=9) == -1 and "V = 9" in lib.last_error()
        assert f(V=0) == -1 and f(B=0) == -1 and f(V=8, B=8192) == -1 and "V * B" in lib.last_error()
        assert f(n=5) == -1 and "n_valid" in lib.last_error()
        assert f(n=-1) == -1
        assert f(n=0) == 0 and f(n=0, V=8, B=8191) == 0                # nothing to do launches nothing
    assert centers(out=None) == -1 and centers(stride=1) == -1 and "cube_stride" in lib.last_error()
    assert centers(fx=0.0) == -1 and centers(flip=0) == -1 and centers(n=0, stride=3) == 0
    assert fuse(J=257) == -1 and "J = 257" in lib.last_error()
    assert fuse(J=0) == -1 and fuse(out=None) == -1
    assert fuse(mode=3) == -1 and "mode" in lib.last_error()
    assert fuse(mode=1, w=None) == -1 and "weights" in lib.last_error()
    assert fuse(mode=0, w=None, n=0) == 0 and fuse(mode=2, w=None, n=0, J=256) == 0 and fuse(mode=1, n=0) == 0
    assert fuse(fx=float("nan")) == -1 and fuse(flip=2) == -1


def test_predict_py_accepts_the_new_flags():
    sys.path.insert(0, REPO)
    try:
        import predict
    finally:
        sys.path.remove(REPO)
    a = predict.parse_args(["frames.npy", "--load-model", "x.pth"])
    assert a.views is None and a.fuse == "mean"
    a = predict.parse_args(["frames.npy", "--load-model", "x.pth", "--views", "rot=-15,15;scale=0.9,1.1", "--fuse", "median"])
    assert a.views == "rot=-15,15;scale=0.9,1.1" and a.fuse == "median"
    with pytest.raises(SystemExit):
        predict.parse_args(["frames.npy", "--load-model", "x.pth", "--fuse", "max"])


# ---- the table and the geometry ---------------------------------------------------------------------------------------------------------
def test_view_table(D, ND):
    views = D.make_views(rot=(30, -30, 360), scale=(1.25,), shift=((10, 0, -15),))
    t = D.view_table(views, S)
    assert t.shape == (6, D.VIEW_TABLE_DOUBLES) and t.dtype == np.float64
    eye = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert t[0].tolist() == eye + [1, 0, 0, 0, 1, 0] + [1, 0, 0, 0] + [0]
    assert t[:, 19].tolist() == [0, 1, 1, 1, 0, 0]                    # 360 degrees rotates, by the reference's test
    assert t[4, 15] == 1.25 and t[5, 16:19].tolist() == [10, 0, -15] and t[4, :9].tolist() == eye
    for row, rot in ((1, 30), (2, -30), (3, 360)):
        R2 = ND.rotation_matrix_2d((S // 2, S // 2), -np.mod(rot, 360), 1)        # Augmenter.rotate's call (loader.py:140-160)
        assert t[row, :6].tolist() == R2.ravel().tolist() and t[row, 6:9].tolist() == [0, 0, 1]
        assert t[row, 9:15].tolist() == ND._invert_affine(R2).ravel().tolist()


BLOB_C = np.array([80.0, 60.0, 620.0])                               # the crop centre; the blob sits 15 pixels to its right
BLOB_UV = (95.0, 60.0)


def blob_frame():
    """far plane 1400 and a 9 x 9 blob at 620 mm, 15 pixels right of the crop centre.  The blob carries +-4 mm of relief: the pixels of a
    perfectly flat one would all equal the crop's maximum, which Loader.normalize (loader.py:88-101) sends to the far plane."""
    f = np.full((EH, EW), 1400, np.uint16)
    vv, uu = np.mgrid[0:EH, 0:EW]
    m = (np.abs(uu - BLOB_UV[0]) <= 4) & (np.abs(vv - BLOB_UV[1]) <= 4)
    f[m] = (616 + (uu[m] + vv[m]) % 9).astype(np.uint16)
    return f


def render_view(ND, frame, center, cube, R2):
    """the host rendering of one view: crop, the rotation's warp where there is one, normalize -- as Augmenter.augment orders them"""
    img, M = ND.crop(frame.astype(np.float32), center, cube, (S, S), E_PARAS)
    depth_max = img.max()
    if R2 is not None:
        img = ND.warp_affine(img, R2, (S, S), 0)
    return ND.normalize(depth_max, img, center, cube), M


@pytest.mark.parametrize("rot", [30, -30, 90])
def test_direction_of_the_rotation(D, ND, rot):
    frame = blob_frame()
    table = D.view_table(D.make_views(rot=(rot,)), S)
    wrong = D.view_table(D.make_views(rot=(-rot,)), S)
    img, M = render_view(ND, frame, BLOB_C, CUBE, table[1, :6].reshape(2, 3))
    vv, uu = np.nonzero(img < 1.0)                                    # foreground: everything nearer than the far plane
    assert 30 <= len(uu) <= 120, len(uu)
    centroid = np.array([uu.mean(), vv.mean()])
    status = np.zeros(2, np.int32)
    Mv = D.view_rotate(None, np.stack([M, M]), status, table)
    Mw = D.view_rotate(None, np.stack([M, M]), status, wrong)
    assert np.array_equal(Mv[0], M) and Mv.dtype == np.float32       # the identity view's matrix is left alone
    p = np.array([BLOB_UV[0], BLOB_UV[1], 1.0])
    want, other, plain = (Mv[1].astype(np.float64) @ p)[:2], (Mw[1].astype(np.float64) @ p)[:2], (M.astype(np.float64) @ p)[:2]
    print("rot %+d: centroid %s, M_v p %s, with the sign flipped %s, unrotated %s" % (rot, centroid, want, other, plain))
    # 1 pixel: the bilinear footprint plus the nearest-neighbour resize
    assert np.linalg.norm(centroid - want) <= 1.0
    assert np.linalg.norm(centroid - other) > 5.0 and np.linalg.norm(centroid - plain) > 5.0


def test_view_rotate_leaves_other_rows_alone(D, lib):
    table = D.view_table(D.make_views(rot=(20,), scale=(1.1,)), S)
    r = np.random.RandomState(2)
    M = r.uniform(-2, 2, (6, 3, 3)).astype(np.float32)              # V = 3, n = 2
    M[3] = np.nan
    status = np.array([0, 0, 0, D.BAD_WINDOW, 0, 0], np.int32)
    blocks = [lib.NyuSample() for _ in range(6)]
    blocks[3] = None
    out = D.view_rotate(blocks, M, status, table)
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(out[keep].view(np.int32), M[keep].view(np.int32)) and not np.array_equal(out[2], M[2])
    assert [b.op for b in blocks if b is not None] == [0, 0, 2, 0, 0]
    assert list(blocks[2].m) == table[1, 9:15].tolist() + [0.0, 0.0, 1.0]
    want = (table[1, :9].reshape(3, 3) @ M[2].astype(np.float64)).astype(np.float32)
    assert np.allclose(out[2], want, rtol=1e-6, atol=1e-6)


def test_matrix_algebra(D, ND):
    """inv(M_v) undoes R . M: what lets awr_joints_unproject treat a rotated view like any other crop"""
    r = np.random.RandomState(11)
    M = ND.center2transmat(BLOB_C, CUBE, (S, S), E_PARAS).astype(np.float64)
    for rot in (20.0, -40.0, 180.0, 333.0):
        R = D.view_table(D.make_views(rot=(rot,)), S)[1, :9].reshape(3, 3)
        Mv = R @ M                                                    # float64, before the float32 store
        p = np.concatenate([r.uniform(0, EW, (200, 1)), r.uniform(0, EH, (200, 1)), np.ones((200, 1))], 1)
        q = (R @ (M @ p.T)).T
        back = (np.linalg.inv(Mv) @ q.T).T
        assert np.all(np.abs(back - p) <= 1e-9 * np.abs(p).max()), np.abs(back - p).max()
        assert np.abs(q[:, :2] - (M @ p.T).T[:, :2]).max() > 5.0      # the view really moves the points


def test_view_centers(D):
    from awr_amd.evaluator import uvd2xyz, xyz2uvd
    table = D.view_table(D.make_views(rot=(20,), scale=(0.8,), shift=((10, 0, 15), (-10, 0, 15))), S)
    c = np.array([(61.0, 49.0, 622.0), (99.5, 71.25, 618.0), (np.nan, 5.0, 600.0)])
    status = np.array([0, 1, 0], np.int32)
    centers, cubes, frame, st = D.view_centers(c, status, CUBE, table, E_PARAS, FLIP)
    assert centers.shape == (15, 3) and cubes.shape == (15, 3) and frame.dtype == np.int64 and st.dtype == np.int32
    assert frame.tolist() == [0, 1, 2] * 5 and st.tolist() == [0, 1, 0] * 5
    for v in (0, 1, 2):                                               # no shift: the centre's bits
        assert np.array_equal(centers[3 * v:3 * v + 3].view(np.int64), c.view(np.int64))
    assert cubes[:6].tolist() == [[300.0] * 3] * 6 and cubes[6:9].tolist() == [[300.0 * 0.8] * 3] * 3
    for v, shift in ((3, (10.0, 0.0, 15.0)), (4, (-10.0, 0.0, 15.0))):
        # float64 in, so the evaluator's own functions keep double until their final float32 cast: the statement agrees to float32
        want = xyz2uvd(uvd2xyz(c[:2], E_PARAS, FLIP).astype(np.float64) + shift, E_PARAS, FLIP)
        assert np.allclose(centers[3 * v:3 * v + 2], want, rtol=1e-5)
        assert np.isnan(centers[3 * v + 2, 0]) and centers[3 * v + 2, 2] == 615.0
        back = uvd2xyz(centers[3 * v:3 * v + 2], E_PARAS, FLIP) - uvd2xyz(c[:2], E_PARAS, FLIP)
        assert np.allclose(back, np.tile(shift, (2, 1)), atol=1e-3)   # the view's centre is `shift` millimetres from the frame's


# ---- fuse_views -------------------------------------------------------------------------------------------------------------------------
def uvd_of(m):
    """evaluator.xyz2uvd in double, stored as float32"""
    fx, fy, u0, v0 = E_PARAS
    return np.array([m[0] * fx / m[2] + u0, (m[1] * FLIP) * fy / m[2] + v0, m[2]]).astype(np.float32)


def hand_made():
    """V = 3, n = 1, J = 2: joint 0 at (0, 0, 600), (3, 0, 600), (0, 6, 630); joint 1 three times the same point"""
    xyz = np.zeros((3, 1, 2, 3), np.float32)
    xyz[:, 0, 0] = [(0, 0, 600), (3, 0, 600), (0, 6, 630)]
    xyz[:, 0, 1] = (10, -20, 700)
    w = np.zeros((3, 1, 2), np.float32)
    w[:, 0, 0], w[:, 0, 1] = (1, 2, 1), (0.25, 0.5, 0.125)
    return xyz, np.zeros((3, 1), np.int32), np.zeros((3, 1), np.int32), w


# joint 0, worked out by hand: the fused point and the weighted mean of the squared distances of the three views from it
#   mean    (1, 2, 610): 1 + 4 + 100, 4 + 4 + 100, 1 + 16 + 400 -> 630 / 3
#   conf    weights 1, 2, 1: (6 / 4, 6 / 4, 2430 / 4); 2.25 + 2.25 + 56.25, twice the same, 2.25 + 20.25 + 506.25 -> 711 / 4
#   median  (0, 0, 600): 0, 9, 36 + 900 -> 945 / 3
HAND = {"mean": ((1.0, 2.0, 610.0), 210.0), "conf": ((1.5, 1.5, 607.5), 177.75), "median": ((0.0, 0.0, 600.0), 315.0)}


@pytest.mark.parametrize("mode", MODES)
def test_fuse_views_on_a_hand_made_case(D, mode):
    xyz, st, ust, w = hand_made()
    fx, fu, sp, used = D.fuse_views(xyz, st, ust, w, mode, E_PARAS, FLIP)
    assert fx.shape == (1, 2, 3) and fx.dtype == np.float32 and fu.dtype == np.float32 and sp.dtype == np.float32 and used.dtype == np.int32
    m, q = HAND[mode]
    assert fx[0, 0].tolist() == list(m) and sp[0, 0] == np.float32(np.sqrt(q)) and used.tolist() == [[3, 3]]
    assert np.array_equal(fu[0, 0], uvd_of(m))
    assert fx[0, 1].tolist() == [10.0, -20.0, 700.0] and sp[0, 1] == 0.0 and np.array_equal(fu[0, 1], uvd_of((10.0, -20.0, 700.0)))
    if mode != "conf":                                                # the weights are read by "conf" alone
        for other in (None, np.full_like(w, np.nan)):
            again = D.fuse_views(xyz, st, ust, other, mode, E_PARAS, FLIP)
            assert all(np.array_equal(a, b) for a, b in zip(again, (fx, fu, sp, used)))


@pytest.mark.parametrize("mode", MODES)
def test_fuse_views_edges(D, mode):
    r = np.random.RandomState(4)
    V, n, J = 4, 3, 5
    xyz = (np.array([-20.0, 10.0, 620.0]) + r.uniform(-100, 100, (V, n, J, 3))).astype(np.float32)
    w = r.uniform(0.1, 1.0, (V, n, J)).astype(np.float32)
    st, ust = np.zeros((V, n), np.int32), np.zeros((V, n), np.int32)
    base = D.fuse_views(xyz, st, ust, w, mode, E_PARAS, FLIP)
    assert (base[3] == V).all() and np.isfinite(base[0]).all() and (base[2] > 0).all()

    def bits(a):
        return np.ascontiguousarray(a).view(np.int32)
    # a single used view gives that view's bits and spread 0: views 0, 1 and 3 of frame 1 carry codes (view 0's would blank the frame, so
    # the single view is view 0 there) -- and a frame whose other views are all NaN in one joint
    st1, ust1 = st.copy(), ust.copy()
    st1[1, 1], ust1[2, 1], st1[3, 1] = 3, 1, 1
    got = D.fuse_views(xyz, st1, ust1, w, mode, E_PARAS, FLIP)
    assert np.array_equal(bits(got[0][1]), bits(xyz[0, 1])) and (got[2][1] == 0.0).all() and (got[3][1] == 1).all()
    assert all(np.array_equal(bits(g[[0, 2]]), bits(b[[0, 2]])) for g, b in zip(got, base))
    x2 = xyz.copy()
    x2[[0, 1, 3], 2, 4, 0] = np.nan
    got = D.fuse_views(x2, st, ust, w, mode, E_PARAS, FLIP)
    assert np.array_equal(bits(got[0][2, 4]), bits(xyz[2, 2, 4])) and got[2][2, 4] == 0.0 and got[3][2, 4] == 1
    assert np.array_equal(bits(got[1][2, 4]), bits(uvd_of(xyz[2, 2, 4].astype(np.float64))))
    # NaN (or an infinity) in one view's joint drops only that joint of that view
    x3 = xyz.copy()
    x3[2, 0, 3, 1], x3[1, 2, 0, 2] = np.nan, np.inf
    got = D.fuse_views(x3, st, ust, w, mode, E_PARAS, FLIP)
    want_used = np.full((n, J), V, np.int32)
    want_used[0, 3] = want_used[2, 0] = V - 1
    assert np.array_equal(got[3], want_used) and np.isfinite(got[0]).all()
    changed = np.zeros((n, J), bool)
    changed[0, 3] = changed[2, 0] = True
    assert all(np.array_equal(bits(g[~changed]), bits(b[~changed])) for g, b in zip(got, base))
    drop = D.fuse_views(np.delete(x3, 2, 0), st[:3], ust[:3], np.delete(w, 2, 0), mode, E_PARAS, FLIP)       # the same without view 2 at all
    assert all(np.array_equal(bits(g[0, 3]), bits(d[0, 3])) for g, d in zip(got[:3], drop[:3]))
    # a non-zero code in view 0 gives a NaN frame
    for codes in ((st, ust), (ust, st)):
        a, b = codes[0].copy(), codes[1]
        a[0, 1] = 2
        got = D.fuse_views(xyz, a, b, w, mode, E_PARAS, FLIP)
        assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all() and np.isnan(got[2][1]).all() and (got[3][1] == 0).all()
        assert all(np.array_equal(bits(g[[0, 2]]), bits(bb[[0, 2]])) for g, bb in zip(got, base))
    # every view of a joint unusable: a NaN joint with views_used = 0 in an otherwise ordinary frame
    x4 = xyz.copy()
    x4[:, 0, 2, 0] = np.nan
    got = D.fuse_views(x4, st, ust, w, mode, E_PARAS, FLIP)
    assert np.isnan(got[0][0, 2]).all() and np.isnan(got[1][0, 2]).all() and np.isnan(got[2][0, 2]) and got[3][0, 2] == 0
    assert np.isfinite(got[0][0, [0, 1, 3, 4]]).all()


def test_fuse_views_conf_weights(D):
    xyz, st, ust, w = hand_made()
    # total weight zero (zeros, negatives and NaN are all max(conf, 0) = no weight): a NaN joint with views_used = 0
    w0 = w.copy()
    w0[:, 0, 0] = (0.0, -0.5, np.nan)
    fx, fu, sp, used = D.fuse_views(xyz, st, ust, w0, "conf", E_PARAS, FLIP)
    assert np.isnan(fx[0, 0]).all() and np.isnan(fu[0, 0]).all() and np.isnan(sp[0, 0]) and used.tolist() == [[0, 3]]
    assert fx[0, 1].tolist() == [10.0, -20.0, 700.0]
    # one weight dropped: the weighted mean of the other two, 1 : 3 -> (0.75 * 3, 0, 600)... of views 1 and 0
    w1 = w.copy()
    w1[:, 0, 0] = (1.0, 3.0, -1.0)
    fx, fu, sp, used = D.fuse_views(xyz, st, ust, w1, "conf", E_PARAS, FLIP)
    assert fx[0, 0].tolist() == [2.25, 0.0, 600.0] and used[0, 0] == 2
    assert sp[0, 0] == np.float32(np.sqrt((1.0 * 2.25 ** 2 + 3.0 * 0.75 ** 2) / 4.0))
    # an infinite weight is no weight either
    w1[:, 0, 0] = (1.0, np.inf, 1.0)
    fx, fu, sp, used = D.fuse_views(xyz, st, ust, w1, "conf", E_PARAS, FLIP)
    assert fx[0, 0].tolist() == [0.0, 3.0, 615.0] and used[0, 0] == 2


def test_fuse_views_median_of_an_even_count(D):
    xyz = np.zeros((4, 1, 1, 3), np.float32)
    xyz[:, 0, 0] = [(4, -1, 600), (1, -7, 640), (3, -3, 610), (2, -5, 700)]
    z = np.zeros((4, 1), np.int32)
    fx, fu, sp, used = D.fuse_views(xyz, z, z, None, "median", E_PARAS, FLIP)
    assert fx[0, 0].tolist() == [2.5, -4.0, 625.0] and used[0, 0] == 4           # the mean of the middle two, per axis
    # five views: the middle one; then one of them dropped by a code: the mean of the middle two of the rest
    xyz5 = np.concatenate([xyz, np.float32([[[[100, 100, 1000]]]])], 0)
    z5 = np.zeros((5, 1), np.int32)
    assert D.fuse_views(xyz5, z5, z5, None, "median", E_PARAS, FLIP)[0][0, 0].tolist() == [3.0, -3.0, 640.0]
    z5[4, 0] = 1
    assert D.fuse_views(xyz5, z5, np.zeros((5, 1), np.int32), None, "median", E_PARAS, FLIP)[0][0, 0].tolist() == [2.5, -4.0, 625.0]
    # two views: their midpoint, and the spread is half their distance
    fx, fu, sp, used = D.fuse_views(xyz[:2], z[:2], z[:2], None, "median", E_PARAS, FLIP)
    assert fx[0, 0].tolist() == [2.5, -4.0, 620.0] and sp[0, 0] == np.float32(np.sqrt(1.5 ** 2 + 3.0 ** 2 + 20.0 ** 2))
