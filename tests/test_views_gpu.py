"""GPU: test-time views -- awr_view_centers, awr_view_rotate and awr_views_fuse against their numpy statements bit for bit,
the rendered views against the host loader's rendering, and awr_amd.Predictor(views=..., fuse=...) against compositions of the statements
and of plain predictors."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLIP, CUBE = -1, (300.0, 300.0, 300.0)
EH, EW, S, J = 120, 160, 64, 14
E_PARAS = (147.0, 146.8, 80.0, 60.0)                # NYU's intrinsics scaled to a 160 x 120 frame
OPEN = dict(max_shift=1e9, depth_range=(1, 65535))  # a gate that only non-finite joints fail
AUTO = dict(seed="nearest", depth_range=(200.0, 1200.0), slab=100.0, refine_iters=2)
MODES = ("mean", "conf", "median")
IDENT = (0.0, 1.0, (0.0, 0.0, 0.0))
# rot 0 / +-20 / 180, scale 0.8 / 1.25, shift (+-10, 0, 15), mixed
POOL = [(20.0, 1.0, (0.0, 0.0, 0.0)), (0.0, 0.8, (0.0, 0.0, 0.0)), (0.0, 1.0, (10.0, 0.0, 15.0)), (-20.0, 1.0, (-10.0, 0.0, 15.0)),
        (180.0, 1.0, (0.0, 0.0, 0.0)), (0.0, 1.25, (10.0, 0.0, 15.0)), (-20.0, 0.8, (0.0, 0.0, 0.0))]


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


def within_one_ulp(a, b):
    """float32 arrays: NaN exactly where the other has NaN, elsewhere (non-negative values) at most one step apart"""
    a, b = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    ia, ib = a[~na].view(np.int32).astype(np.int64), b[~nb].view(np.int32).astype(np.int64)
    return bool((ia >= 0).all() and (ib >= 0).all() and (np.abs(ia - ib) <= 1).all())


# ---- awr_view_centers, awr_view_rotate ----------------------------------------------------------------------------------------------------
def centre_batch(B, seed):
    """centres inside the frame at 500 ... 900 mm; from B = 3 on also row 1 NaN (status EMPTY) and row 2 at the left edge, where the plain
    window still meets the frame (uend = 1) and the window of the view shifted by (-10, 0, 15) mm does not (uend = 0)"""
    r = np.random.RandomState(seed)
    c = np.stack([r.uniform(20, EW - 20, B), r.uniform(20, EH - 20, B), r.uniform(500, 900, B)], 1)
    status = np.zeros(B, np.int32)
    if B >= 3:
        c[1], status[1] = np.nan, 1
        c[2] = (-35.0, 60.0, 620.0)
    if B > 40:
        status[[7, 290]] = [2, 1]
        c[290] = np.nan
    cube = np.tile(np.float64(CUBE), (B, 1))
    if B > 100:
        cube[100:] = np.repeat(r.uniform(200, 400, (B - 100, 1)), 3, 1)
    return c, status, cube


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("V", [2, 5, 8])
def test_view_centers_and_view_rotate_equal_their_statements(D, dev, V, B):
    from awr_amd import _lib as L
    table = D.view_table([IDENT] + POOL[:V - 1], S)
    c, status, cube = centre_batch(B, 10 * V + B)
    cube_arg = cube if B > 100 else np.float64(CUBE)               # a cube per frame (cube_stride 3) and one cube (cube_stride 0)
    want = D.view_centers(c, status, cube_arg, table, E_PARAS, FLIP)
    c_d, st_d, tab_d = torch.from_numpy(c).to(dev), torch.from_numpy(status).to(dev), torch.from_numpy(table).to(dev)
    got = D.view_centers_device(c_d, st_d, cube_arg, tab_d, paras=E_PARAS, flip=FLIP)
    assert [g.dtype for g in got] == [torch.float64, torch.float64, torch.int64, torch.int32]
    for g, w, name in zip(got, want, ("centers", "cubes", "frame", "status")):
        assert same_bits(g, w), (name, V, B)
    # n_valid < B: the rows past it of every view are left as they are (257 = one frame into the second workgroup of view 0)
    if B >= 3:
        nv = 257 if B == 300 else B - 1
        pre = (torch.full((V * B, 3), -7.0, dtype=torch.float64, device=dev), torch.full((V * B, 3), -7.0, dtype=torch.float64, device=dev),
               torch.full((V * B,), -7, dtype=torch.int64, device=dev), torch.full((V * B,), -7, dtype=torch.int32, device=dev))
        D.view_centers_device(c_d, st_d, cube_arg, tab_d, n_valid=nv, paras=E_PARAS, flip=FLIP, out=pre)
        valid = (np.arange(V * B) % B) < nv
        for g, w in zip(pre, want):
            g = g.cpu().numpy()
            assert same_bits(g[valid], w[valid]) and (g[~valid] == -7).all()
    # the unchanged awr_detect_samples over the V * B rows, then awr_view_rotate in place
    centers, cubes, frame, st = want
    blocks, M, cxyz, cube32, st2 = D.samples_device(got[0], cubes, S, got[2], B, (EH, EW), E_PARAS, FLIP, status=got[3].clone())
    h_blocks, h_M, h_cxyz, h_cube, h_st = D.sample_blocks(centers, cubes, S, E_PARAS, FLIP, (EH, EW), frames=frame)
    h_st = np.where(st != 0, st, h_st).astype(np.int32)            # an earlier code is kept
    assert same_bits(st2, h_st) and same_bits(M, h_M) and same_bits(cxyz, h_cxyz) and same_bits(cube32, h_cube)
    if V >= 5 and B >= 3:                                           # the shifted window of row 2 leaves the frame, its plain one does not
        assert h_st[2] == D.OK and h_st[4 * B + 2] == D.BAD_WINDOW and h_st[3 * B + 2] == D.OK
    raw0, M0 = blocks.cpu().numpy().copy(), M.cpu().numpy().copy()
    parsed = [L.NyuSample.from_buffer_copy(bytes(row)) for row in raw0]
    want_M = D.view_rotate(parsed, M0, h_st, table)
    want_raw = np.stack([np.frombuffer(bytes(p), np.uint8) for p in parsed])
    if B >= 3:                                                      # n_valid < B first, on copies: the rows past it keep their bytes
        b2, M2 = blocks.clone(), M.clone()
        D.view_rotate_device(b2, M2, st2, tab_d, n_valid=nv)
        assert np.array_equal(b2.cpu().numpy()[valid], want_raw[valid]) and same_bits(M2.cpu().numpy()[valid], want_M[valid])
        assert np.array_equal(b2.cpu().numpy()[~valid], raw0[~valid]) and same_bits(M2.cpu().numpy()[~valid], M0[~valid])
    D.view_rotate_device(blocks, M, st2, tab_d)
    assert np.array_equal(blocks.cpu().numpy(), want_raw) and same_bits(M, want_M)
    # what was rotated: exactly the AWR_DET_OK rows of the rotating views; a BAD_WINDOW row keeps its pixel-free block and NaN matrix
    rotating = np.repeat(table[:, 19] != 0, B) & (h_st == D.OK)
    ops = np.array([p.op for p in parsed])
    assert rotating.any() and np.array_equal(ops == 2, rotating) and (ops[~rotating] == 0).all()
    changed = (bits(want_M) != bits(M0)).any((1, 2))
    assert not changed[~rotating].any() and changed[rotating].all()
    bad = h_st == D.BAD_WINDOW
    if bad.any():
        assert np.isnan(want_M[bad]).all() and all(parsed[i].rw == 0 for i in np.nonzero(bad)[0])


# ---- awr_views_fuse -----------------------------------------------------------------------------------------------------------------------
def fuse_batch(V, B, nj, seed):
    """joints around (-20, 10, 620) +- 100 mm; about 10 % of the (view, joint) entries NaN; codes on some views (never on view 0 of frame 0;
    on view 0 of frame 1 when there is one); weights with zeros, negatives and NaNs"""
    r = np.random.RandomState(seed)
    xyz = (np.array([-20.0, 10.0, 620.0]) + r.uniform(-100, 100, (V, B, nj, 3))).astype(np.float32)
    hole = r.uniform(size=(V, B, nj)) < 0.10
    xyz[hole, r.randint(0, 3, int(hole.sum()))] = np.nan
    xyz[V - 1, B - 1, nj - 1, 0] = np.inf
    status = (r.uniform(size=(V, B)) < 0.08).astype(np.int32) * r.randint(1, 4, (V, B)).astype(np.int32)
    ustatus = (r.uniform(size=(V, B)) < 0.08).astype(np.int32) * r.randint(1, 3, (V, B)).astype(np.int32)
    status[0, 0] = ustatus[0, 0] = 0
    if B >= 3:
        status[0, 1], ustatus[0, 2], ustatus[V - 1, 0] = 3, 0, 2
    w = r.uniform(-0.2, 1.0, (V, B, nj)).astype(np.float32)
    w[r.uniform(size=w.shape) < 0.05] = 0.0
    w[r.uniform(size=w.shape) < 0.05] = np.nan
    w[0, 0, 0] = -0.0
    return xyz, status, ustatus, w


def assert_fused(got, want, rows=slice(None), what=""):
    for g, w, name in zip(got, want, ("xyz", "uvd", "view_spread_mm", "views_used")):
        g = (g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else g)[rows]
        if name == "view_spread_mm":
            # both sides round a double square root good to 1 ulp of double to float32: at most one float32 step apart
            assert within_one_ulp(g, w[rows]), (name, what)
        else:
            assert same_bits(g, w[rows]), (name, what)


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("nj", [1, 14, 256])
@pytest.mark.parametrize("V", [2, 3, 8])
def test_views_fuse_equals_the_statement(D, dev, V, nj, B):
    xyz, status, ustatus, w = fuse_batch(V, B, nj, 100 * V + nj + B)
    dx, dst, dust, dw = (torch.from_numpy(a).to(dev) for a in (xyz, status, ustatus, w))
    for mode in MODES:
        want = D.fuse_views(xyz, status, ustatus, w, mode, E_PARAS, FLIP)
        got = D.fuse_views_device(dx, dst, dust, dw if mode == "conf" else None, mode, E_PARAS, FLIP)
        assert [g.dtype for g in got] == [torch.float32, torch.float32, torch.float32, torch.int32]
        assert_fused(got, want, what=(mode, V, nj, B))
        used = want[3]
        if B >= 3 and nj >= 14:
            assert (used < V).any() and (used > 0).any()
        if B >= 3:                                                  # a code on view 0 blanks the frame; the frames around it are ordinary
            assert (used[1] == 0).all() and np.isnan(want[0][1]).all() and np.isnan(want[2][1]).all() and (nj < 14 or (used[[0, 2]] > 0).any())
            nv = 257 if B == 300 else B - 1
            pre = (torch.full((B, nj, 3), -7.0, device=dev), torch.full((B, nj, 3), -7.0, device=dev), torch.full((B, nj), -7.0, device=dev),
                   torch.full((B, nj), -7, dtype=torch.int32, device=dev))
            D.fuse_views_device(dx, dst, dust, dw, mode, E_PARAS, FLIP, n_valid=nv, out=pre)
            assert_fused(pre, want, rows=slice(0, nv), what=(mode, "n_valid"))
            assert all((p[nv:] == -7).all() for p in pre)
    if B == 1:                                                      # the only frame with a code on view 0
        for codes in ((1, 0), (0, 2)):
            st1, ust1 = status.copy(), ustatus.copy()
            st1[0, 0], ust1[0, 0] = codes
            want = D.fuse_views(xyz, st1, ust1, w, "mean", E_PARAS, FLIP)
            got = D.fuse_views_device(dx, torch.from_numpy(st1).to(dev), torch.from_numpy(ust1).to(dev), None, "mean", E_PARAS, FLIP)
            assert_fused(got, want)
            assert (want[3] == 0).all() and np.isnan(want[1]).all()


def test_views_fuse_refuses_what_it_cannot_hold(D, dev):
    from awr_amd import _lib as L
    x = torch.zeros((9, 2, 257, 3), device=dev)
    st = torch.zeros((9, 2), dtype=torch.int32, device=dev)
    out = (torch.full((2, 257, 3), -7.0, device=dev), torch.full((2, 257, 3), -7.0, device=dev), torch.full((2, 257), -7.0, device=dev),
           torch.full((2, 257), -7, dtype=torch.int32, device=dev))

    def call(V, nj):
        return L.lib.awr_views_fuse(x.data_ptr(), st.data_ptr(), st.data_ptr(), None, 0, V, 2, nj, 2, *E_PARAS, FLIP, out[0].data_ptr(),
                                    out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), L.stream())
    assert call(9, 14) == -1 and "V = 9" in L.last_error()
    assert call(8, 257) == -1 and "J = 257" in L.last_error()
    with pytest.raises(L.AwrError, match="V = 9"):
        D.fuse_views_device(x[:, :, :14].contiguous(), st, st, None, "mean", E_PARAS, FLIP)
    torch.cuda.synchronize()
    assert all((o == -7).all() for o in out)                         # codes, and no launch
    assert call(8, 256) == 0
    torch.cuda.synchronize()
    used = out[3].flatten()                                           # (the (2, 256) result lies packed at the front of the buffer)
    assert (used[:512] == 8).all() and (used[512:] == -7).all()


# ---- the Predictor ------------------------------------------------------------------------------------------------------------------------
HANDS = ((60, 50), (100, 70))
C0 = np.array([(61.0, 49.0, 622.0), (99.5, 71.25, 618.0)])
FIELDS = ("uvd", "xyz", "M", "center_xyz", "status")
VFIELDS = FIELDS + ("view_spread_mm", "views_used")


def blob_frames(hands=HANDS):
    """tests/test_recenter_gpu.py's frames: a far plane and a hand-sized blob of 41 x 41 pixels at 600 ... 640 mm"""
    f = np.full((2, EH, EW), 1400, np.uint16)
    vv, uu = np.mgrid[0:EH, 0:EW]
    for b, (cu, cv) in enumerate(hands):
        m = (np.abs(uu - cu) <= 20) & (np.abs(vv - cv) <= 20)
        f[b][m] = (600 + (uu[m] + vv[m]) % 41).astype(np.uint16)
    return f


@pytest.fixture(scope="module")
def e2e(dev, D):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()

    def make(max_batch=2, **kw):
        return awr_amd.Predictor(net, S, 1.0, cube=CUBE, paras=E_PARAS, flip=FLIP, max_batch=max_batch, frame_shape=(EH, EW), **kw)
    views = D.make_views(rot=(20, -20), scale=(1.1,), shift=((0, 0, 10),))
    return types.SimpleNamespace(net=net, make=make, frames=blob_frames(), views=views, table=D.view_table(views, S))


def assert_same_prediction(got, want, rows=slice(None), fields=FIELDS):
    assert type(got) is type(want)
    for f in fields:
        g, w = getattr(got, f)[rows], getattr(want, f)[rows]
        assert same_bits(g, w), (f, g.cpu().numpy(), w.cpu().numpy())


def host_view(ND, frame, center, cube, R2):
    """the host loader's rendering of one view: crop, the rotation's warp where there is one, normalize (Augmenter.augment's order)"""
    img, _ = ND.crop(np.asarray(frame, dtype=np.float32), center, cube, (S, S), E_PARAS)
    depth_max = img.max()
    if R2 is not None:
        img = ND.warp_affine(img, R2, (S, S), 0)
    return ND.normalize(depth_max, img, center, cube).astype(np.float32)


def test_rendered_views_equal_the_host_loader(D, e2e):
    from awr_amd import nyu_data as ND
    views = D.make_views(rot=(25, -40), scale=(1.2,))
    table = D.view_table(views, S)
    pred = e2e.make(views=views, refine_iters=0)
    out = pred.predict(e2e.frames, centers_uvd=C0)
    assert out.status.tolist() == [0, 0] and pred.view_outputs.status.tolist() == [[0, 0]] * 4
    img = pred._img.cpu()
    assert img.shape == (8, 1, S, S)
    rendered = []
    for v in range(4):
        for b in range(2):
            R2 = table[v, :6].reshape(2, 3) if table[v, 19] else None
            want = torch.from_numpy(host_view(ND, e2e.frames[b], C0[b], np.float64(CUBE) * table[v, 15], R2))
            assert torch.equal(img[v * 2 + b, 0], want), (v, b, (img[v * 2 + b, 0] != want).sum())
            rendered.append(want)
    assert (rendered[0] < 1).sum() > 500                              # a hand's worth of foreground
    for v in (1, 2, 3):                                               # and every view is a different picture of it
        assert not torch.equal(rendered[2 * v], rendered[0])


_PLAIN = {}


def plain_predictor(e2e, confidence):
    """the predictor without views at the plan batch of five views of two frames (built once per kind of engine)"""
    if confidence not in _PLAIN:
        _PLAIN[confidence] = e2e.make(max_batch=2 * len(e2e.views), refine_iters=0, confidence=confidence)
    return _PLAIN[confidence]


@pytest.mark.parametrize("fuse", MODES)
def test_predictor_equals_its_composition(D, dev, e2e, fuse):
    V = len(e2e.views)
    pred = e2e.make(views=e2e.views, fuse=fuse, refine_iters=0)
    assert pred.view_outputs is None
    out = pred.predict(e2e.frames, centers_uvd=C0)
    pred.check()
    vo = pred.view_outputs
    assert type(out).__name__ == "ViewPrediction"
    assert out._fields == ("xyz", "uvd", "center_xyz", "M", "status", "view_spread_mm", "views_used")
    assert vo.xyz.shape == (V, 2, J, 3) and vo.uvd.shape == (V, 2, J, 3) and vo.M.shape == (V, 2, 3, 3) and vo.status.shape == (V, 2)
    assert vo.center_xyz.shape == (V, 2, 3) and vo.cube.shape == (V, 2, 3) and vo.ustatus.shape == (V, 2)
    assert (fuse == "conf") == hasattr(vo, "conf") and (fuse != "conf" or vo.conf.shape == (V, 2, J))
    # (a) the per-view geometry is the statements'
    centers, cubes, frame, st = D.view_centers(C0, np.zeros(2, np.int32), CUBE, e2e.table, E_PARAS, FLIP)
    h_blocks, h_M, h_cxyz, h_cube, h_st = D.sample_blocks(centers, cubes, S, E_PARAS, FLIP, (EH, EW), frames=frame)
    h_M = D.view_rotate(h_blocks, h_M, h_st, e2e.table)
    assert same_bits(vo.M.reshape(V * 2, 3, 3), h_M) and same_bits(vo.center_xyz.reshape(V * 2, 3), h_cxyz)
    assert same_bits(vo.cube.reshape(V * 2, 3), h_cube) and same_bits(vo.status.reshape(V * 2), h_st) and h_st.tolist() == [0] * (2 * V)
    assert vo.ustatus.tolist() == [[0, 0]] * V
    # the fields that are view 0's
    assert same_bits(out.M, vo.M[0]) and same_bits(out.center_xyz, vo.center_xyz[0]) and same_bits(out.status, vo.status[0])
    # (b) the result is fuse_views of the views' joints
    w = vo.conf.cpu().numpy() if fuse == "conf" else None
    want = D.fuse_views(vo.xyz.cpu().numpy(), vo.status.cpu().numpy(), vo.ustatus.cpu().numpy(), w, fuse, E_PARAS, FLIP)
    assert_fused((out.xyz, out.uvd, out.view_spread_mm, out.views_used), want, what=fuse)
    print("fuse %s: views used %s, spread (mm) %s" % (fuse, np.bincount(want[3].ravel(), minlength=V + 1).tolist(), want[2].round(2).tolist()))
    assert out.views_used.dtype == torch.int32 and out.view_spread_mm.dtype == torch.float32
    if fuse != "conf":                                                # (how many views "conf" uses is up to the weights of the procedural net)
        assert (want[3] == V).all()
    # (c) view 0 is what a predictor without views gives at the same plan batch, in the same rows
    plain = plain_predictor(e2e, fuse == "conf")
    p_out = plain.predict(e2e.frames, centers_uvd=C0)
    assert same_bits(vo.xyz[0], p_out.xyz) and same_bits(vo.uvd[0], p_out.uvd) and same_bits(out.M, p_out.M)
    # (d) the views are different pictures with different answers, all of them finite
    assert torch.isfinite(vo.xyz).all() and torch.isfinite(vo.uvd).all()
    assert all(not same_bits(vo.xyz[v], vo.xyz[0]) for v in range(1, V))
    assert not same_bits(out.xyz, vo.xyz[0]) and (want[2][want[3] >= 2] > 0).all()
    # (e) the geometry end to end, whatever the network says: one image point, sent through every view's M_v on the host in float64, comes
    # back from awr_joints_unproject as the same uvd.  1e-3 pixel / mm: float32 storage of M_v and of coordinates below 640 (ulp 6e-5)
    M_all, cxyz_all, cube_all = vo.M.reshape(V * 2, 3, 3), vo.center_xyz.reshape(V * 2, 3), vo.cube.reshape(V * 2, 3)
    point = np.array([70.0, 55.0, 1.0])
    q = np.einsum("rij,j->ri", M_all.cpu().numpy().astype(np.float64), point)
    jt = np.empty((V * 2, 1, 3), np.float64)
    jt[:, 0, 0], jt[:, 0, 1] = q[:, 0] / (S / 2.0) - 1.0, q[:, 1] / (S / 2.0) - 1.0
    jt[:, 0, 2] = (630.0 - cxyz_all[:, 2].cpu().numpy().astype(np.float64)) / (cube_all[:, 2].cpu().numpy().astype(np.float64) / 2.0)
    uvd, xyz, ust = D.unproject_device(torch.from_numpy(jt.astype(np.float32)).to(dev), cxyz_all.contiguous(), M_all.contiguous(),
                                       cube_all.contiguous(), S, E_PARAS, FLIP)
    err = (uvd[:, 0].cpu().numpy().astype(np.float64) - (70.0, 55.0, 630.0))
    print("un-projection of one point through every view: largest error %s" % np.abs(err).max(0))
    assert ust.tolist() == [0] * (2 * V) and (np.abs(err) <= 1e-3).all()
    assert all(np.abs(q[2 * v:2 * v + 2, :2] - q[:2, :2]).min() > 1.0 for v in (1, 2))      # (the rotated views put the point elsewhere)
    # fewer frames than the plan holds: the same bits for the frame that is there
    one = pred.predict(e2e.frames[:1], centers_uvd=C0[:1])
    assert one.xyz.shape == (1, J, 3) and pred.view_outputs.xyz.shape == (V, 1, J, 3)
    assert_same_prediction(one, out, rows=slice(0, 1), fields=VFIELDS)


def test_confidence_fields_are_view_zeros(D, e2e):
    pred = e2e.make(views=e2e.views, fuse="conf", refine_iters=0, confidence=True)
    out = pred.predict(e2e.frames, centers_uvd=C0)
    assert type(out).__name__ == "ConfidentViewPrediction"
    p_out = plain_predictor(e2e, True).predict(e2e.frames, centers_uvd=C0)
    for f in ("conf", "peak", "spread_mm", "M", "center_xyz", "status"):
        assert same_bits(getattr(out, f), getattr(p_out, f)), f
    assert same_bits(pred.view_outputs.conf[0], out.conf)
    bare = e2e.make(views=e2e.views, fuse="conf", refine_iters=0).predict(e2e.frames, centers_uvd=C0)
    for f in VFIELDS:
        assert same_bits(getattr(bare, f), getattr(out, f)), f


def test_recentring_with_views_equals_its_composition(D, e2e):
    plain = e2e.make(views=e2e.views, refine_iters=0, **OPEN)
    rec = e2e.make(views=e2e.views, recenter=1, refine_iters=0, **OPEN)
    out0 = plain.predict(e2e.frames, centers_uvd=C0)
    ust0 = plain.view_outputs.ustatus[0].cpu().numpy()
    c1, nxt, code = D.joints_center(out0.xyz.cpu().numpy(), C0, out0.center_xyz.cpu().numpy(), np.tile(np.float32(CUBE), (2, 1)),
                                    out0.status.cpu().numpy(), ust0, E_PARAS, FLIP, **OPEN)
    print("codes %s, centres %s -> %s" % (code.tolist(), C0.tolist(), c1.tolist()))
    assert (code == D.MOVED).any() and not same_bits(c1, C0)       # the comparison is about frames that really moved
    out1 = plain.predict(e2e.frames, centers_uvd=c1)
    vo1 = {k: v.clone() for k, v in vars(plain.view_outputs).items()}
    out = rec.predict(e2e.frames, centers_uvd=C0)
    assert_same_prediction(out, out1, fields=VFIELDS)
    assert not same_bits(out.xyz, out0.xyz)
    for k, v in vars(rec.view_outputs).items():
        assert same_bits(v, vo1[k]), k
    assert rec.recenter_codes.shape == (2, 2) and rec.recenter_codes[0].tolist() == code.tolist()
    assert same_bits(rec.centers_uvd, c1)
    rec.check()


def test_a_frame_with_no_hand(D, e2e):
    from awr_amd import _lib as L
    V = len(e2e.views)
    pred = e2e.make(views=e2e.views, recenter=1, track=True, **AUTO)
    want = pred.predict(e2e.frames)
    pred.check()
    assert want.status.tolist() == [0, 0] and torch.isfinite(want.xyz).all()
    empty = e2e.frames.copy()
    empty[1] = 1400                                                   # all far plane, beyond depth_range
    pred.reset_track()
    out = pred.predict(empty)
    with pytest.raises(L.AwrError, match=r"frame 1 .*AWR_DET_EMPTY"):
        pred.check()
    vo = pred.view_outputs
    assert out.status.tolist() == [0, D.EMPTY] and vo.status.tolist() == [[0, D.EMPTY]] * V
    assert torch.isnan(out.xyz[1]).all() and torch.isnan(out.uvd[1]).all() and torch.isnan(out.view_spread_mm[1]).all()
    assert (out.views_used[1] == 0).all() and torch.isnan(out.center_xyz[1]).all() and torch.isnan(vo.xyz[:, 1]).all()
    assert pred.recenter_codes[:, 1].tolist() == [D.KEPT_FRAME] * 2 and torch.isnan(pred._track[1]).all()
    assert_same_prediction(out, want, rows=0, fields=VFIELDS)
    assert (out.views_used[0] == V).all() and not torch.isnan(out.xyz[0]).any()
    torch.cuda.synchronize()


def test_defaults_change_nothing(e2e):
    a = e2e.make(confidence=True, **AUTO)
    b = e2e.make(confidence=True, views=None, fuse="mean", **AUTO)
    every = FIELDS + ("conf", "peak", "spread_mm")
    for kw in (dict(frames=e2e.frames), dict(frames=e2e.frames[:1]), dict(frames=e2e.frames, centers_uvd=C0),
               dict(frames=e2e.frames[1:], centers_uvd=C0[1:])):
        got, want = b.predict(**kw), a.predict(**kw)
        assert type(got).__name__ == "ConfidentPrediction"
        assert_same_prediction(got, want, fields=every)
    # and nothing new is allocated or kept
    assert b.view_outputs is None and b.views is None
    assert not any(name in vars(b) for name in ("_vtable", "_vcenters", "_vcubes", "_vframe", "views", "fuse", "V"))
    assert b._blocks.shape[0] == 2 and b._img.shape[0] == 2 and b.engine.B == 2
