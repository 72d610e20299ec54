"""GPU: prediction from raw depth frames -- the device hand detector against its numpy restatement (bit for bit), the device-built crop
blocks against nyu_device.set_crop / set_normalize, the rendered image against the host loader, the label-free un-projection against the
device evaluator, and awr_amd.Predictor end to end against the hand-assembled pipeline."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FH, FW = 40, 52                                   # the width is no multiple of 8
PARAS = (66.0, 65.5, 26.0, 20.0)                  # a 300 mm cube spans about 20 pixels at 1 m
FLIP, CUBE = -1, (300.0, 300.0, 300.0)
NYU_PARAS = (588.03, 587.07, 320.0, 240.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mods():
    import awr_amd  # noqa: F401
    from awr_amd import _lib, detect, evaluator, nyu_data, nyu_device
    return types.SimpleNamespace(L=_lib, D=detect, E=evaluator, ND=nyu_data, DV=nyu_device)


def make_store(frames, dev):
    data = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    return types.SimpleNamespace(data=data, ftype=0, fh=int(frames.shape[1]), fw=int(frames.shape[2]), n=int(frames.shape[0]))


@pytest.fixture(scope="module")
def small(dev):
    """four 40 x 52 frames of random uint16 in {0} u [400, 1600]; frame 1 is a blob that touches the left and the top border"""
    r = np.random.RandomState(7)
    f = r.randint(400, 1601, (4, FH, FW)).astype(np.uint16)
    f[r.uniform(size=f.shape) < 0.3] = 0
    f[1] = 0
    f[1, 0:9, 0:11] = r.randint(780, 821, (9, 11))
    f[2, :, 30:] = 0
    return f, make_store(f, dev)


def same_bits(a, b):
    """torch.equal with NaN equal to NaN"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def host_detect(D, frames, idx, seed, centers, iters, paras=PARAS, **kw):
    out = [D.detect(frames[i], seed=seed, center=None if centers is None else centers[k], cube=CUBE, paras=paras, iters=iters, **kw)
           for k, i in enumerate(idx)]
    return torch.tensor([c for c, _ in out], dtype=torch.float64), torch.tensor([s for _, s in out], dtype=torch.int32)


GIVEN = [(20.0, 15.0, 1000.0),          # inside
         (3.0, 2.5, 805.0),             # the blob of frame 1: the window is clipped at the left and at the top
         (-500.0, 10.0, 900.0)]         # window wholly outside the frame


@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("seed", ["given", "range", "nearest"])
def test_detector_equals_the_restatement_bit_for_bit(mods, dev, small, seed, iters):
    D = mods.D
    frames, store = small
    idx = [0, 1, 2]
    centers = GIVEN if seed == "given" else None
    kw = dict(depth_range=(450.0, 1500.0), slab=120.0)
    ref_c, ref_s = host_detect(D, frames, idx, seed, centers, iters, **kw)
    for parts in (0, 1, 7, 64):          # 64 workgroups per frame: more than the frame has rows
        c, s = D.detect_device(store, idx, seed=seed, centers=centers, cube=CUBE, paras=PARAS, iters=iters, parts=parts, **kw)
        assert c.dtype == torch.float64 and same_bits(c.cpu(), ref_c), (parts, c.cpu(), ref_c)
        assert torch.equal(s.cpu(), ref_s), (parts, s.cpu(), ref_s)
    if seed == "given" and iters:
        assert ref_s.tolist() == [D.OK, D.OK, D.EMPTY] and torch.isnan(ref_c[2]).all()
    if seed != "given":
        assert ref_s.tolist() == [D.OK] * 3


def test_detector_per_frame_cubes_and_reproducibility(mods, dev, small):
    D = mods.D
    frames, store = small
    idx = [3, 0, 2]
    cubes = np.array([[300.0, 300, 300], [250, 250, 250], [420, 380, 300]])
    ref = [D.detect(frames[i], seed="nearest", cube=cubes[k], paras=PARAS, depth_range=(400, 1600), slab=100, iters=2) for k, i in enumerate(idx)]
    a = D.detect_device(store, idx, seed="nearest", cube=cubes, paras=PARAS, depth_range=(400, 1600), slab=100, iters=2)
    b = D.detect_device(store, idx, seed="nearest", cube=cubes, paras=PARAS, depth_range=(400, 1600), slab=100, iters=2)
    assert same_bits(a[0].cpu(), torch.tensor([c for c, _ in ref], dtype=torch.float64)) and a[1].tolist() == [s for _, s in ref]
    assert same_bits(a[0].cpu(), b[0].cpu()) and torch.equal(a[1], b[1])


def test_frame_index_outside_the_store(mods, dev, small):
    D = mods.D
    frames, store = small
    c, s = D.detect_device(store, [0, 4, -1, 3], seed="range", cube=CUBE, paras=PARAS, depth_range=(400, 1600), iters=1)      # 4 == n_frames
    ref_c, ref_s = host_detect(D, frames, [0, 3], "range", None, 1, depth_range=(400, 1600))
    assert s.tolist() == [D.OK, D.BAD_FRAME, D.BAD_FRAME, D.OK]
    c = c.cpu()
    assert torch.isnan(c[1:3]).all() and same_bits(c[[0, 3]], ref_c)
    # the block builder never hands such an index on
    blocks, M, _, _, st = D.samples_device(torch.tensor([GIVEN[0]] * 2, dtype=torch.float64, device=dev), CUBE, 32, [4, 1], 4, (FH, FW), PARAS, FLIP)
    blk = [mods.L.NyuSample.from_buffer_copy(bytes(r)) for r in blocks.cpu().numpy()]
    assert st.tolist() == [D.BAD_FRAME, D.OK] and (blk[0].frame, blk[0].rw, blk[0].rh) == (0, 0, 0) and blk[1].frame == 1
    assert torch.isnan(M[0]).all()


def test_sums_are_64_bit(mods, dev):
    D = mods.D
    full = np.full((1, 480, 640), 65535, np.uint16)
    store = make_store(full, dev)
    for seed in ("range", "nearest"):
        c, s = D.detect_device(store, [0], seed=seed, cube=CUBE, paras=NYU_PARAS, depth_range=(1.0, 65535.0), slab=0.0, iters=0)
        assert s.tolist() == [D.OK] and c.cpu().tolist() == [[319.5, 239.5, 65535.0]]      # sum of d ~ 2e10 wraps a 32-bit accumulator
    c, s = D.detect_device(store, [0], seed="given", centers=[(320.0, 240.0, 65500.0)], cube=(1e6, 1e6, 300.0), paras=NYU_PARAS, iters=1)
    assert s.tolist() == [D.OK] and c.cpu().tolist() == [[319.5, 239.5, 65535.0]]


HAND_PICKED = [(2.0, 3.0, 900.0),            # window partly outside the frame
               (26.0, 20.0, 1000.0),         # the frame's centre
               (30.0, 18.0, 2000.0)]         # far: a window of about 10 pixels


def block_fields(L, blk):
    return {name: (list(getattr(blk, name)) if name == "m" else getattr(blk, name)) for name, _ in L.NyuSample._fields_}


@pytest.fixture(scope="module")
def centres(mods, dev, small):
    """the detector's centres for frames 0 ... 2 + the hand-picked ones, with their frames"""
    c, s = mods.D.detect_device(small[1], [0, 1, 2], seed="nearest", cube=CUBE, paras=PARAS, depth_range=(450.0, 1500.0), slab=120.0, iters=2)
    assert s.tolist() == [0, 0, 0]
    cs = np.concatenate([c.cpu().numpy(), np.array(HAND_PICKED)], 0)
    return cs, [0, 1, 2, 3, 0, 3]


def test_device_blocks_equal_the_hosts(mods, dev, small, centres):
    L, D, ND, E = mods.L, mods.D, mods.ND, mods.E
    cs, fidx = centres
    blocks, M, cxyz, cube, st = D.samples_device(torch.from_numpy(cs).to(dev), CUBE, 32, fidx, 4, (FH, FW), PARAS, FLIP)
    h_blocks, h_M, h_cxyz, h_cube, h_st = D.sample_blocks(cs, CUBE, 32, PARAS, FLIP, (FH, FW), frames=fidx)
    assert st.tolist() == h_st.tolist() == [0] * 6
    raw = blocks.cpu().numpy()
    for b in range(6):
        got, want = block_fields(L, L.NyuSample.from_buffer_copy(bytes(raw[b]))), block_fields(L, h_blocks[b])
        assert got == want, (b, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        assert torch.equal(M[b].cpu(), torch.from_numpy(ND.center2transmat(cs[b], np.array(CUBE), (32, 32), PARAS)))
        assert torch.equal(cxyz[b].cpu(), torch.from_numpy(E.uvd2xyz(cs[b], PARAS, FLIP)))
    assert torch.equal(M.cpu(), torch.from_numpy(h_M)) and torch.equal(cxyz.cpu(), torch.from_numpy(h_cxyz))
    assert torch.equal(cube.cpu(), torch.tensor([CUBE] * 6, dtype=torch.float32))
    widths = [L.NyuSample.from_buffer_copy(bytes(raw[b])).cw for b in range(6)]
    assert widths[3] > 0 and L.NyuSample.from_buffer_copy(bytes(raw[3])).ustart < 0 and 8 <= widths[5] <= 11


def test_windows_set_crop_refuses(mods, dev):
    L, D = mods.L, mods.D
    cs = np.array([(-500.0, 10.0, 900.0), (26.0, 20.0, 1e7), (np.nan, np.nan, np.nan), (26.0, 20.0, 0.0), (26.0, 20.0, 1000.0)])
    status = torch.tensor([0, 0, D.EMPTY, 0, 0], dtype=torch.int32, device=dev)
    blocks, M, cxyz, cube, st = D.samples_device(torch.from_numpy(cs).to(dev), CUBE, 32, [0] * 5, 4, (FH, FW), PARAS, FLIP, status=status)
    h = D.sample_blocks(cs, CUBE, 32, PARAS, FLIP, (FH, FW))
    assert h[4].tolist() == [D.BAD_WINDOW] * 4 + [D.OK]
    assert st.tolist() == [D.BAD_WINDOW, D.BAD_WINDOW, D.EMPTY, D.BAD_WINDOW, D.OK]          # an earlier code is kept
    raw = blocks.cpu().numpy()
    for b in range(4):
        blk = L.NyuSample.from_buffer_copy(bytes(raw[b]))
        assert (blk.frame, blk.cw, blk.ch, blk.rw, blk.rh) == (0, 0, 0, 0, 0) and torch.isnan(M[b]).all()
    assert not torch.isnan(M[4]).any()


def test_renderer_fed_with_device_blocks_makes_the_hosts_image(mods, dev, small, centres):
    D, ND, DV = mods.D, mods.ND, mods.DV
    frames, store = small
    cs, fidx = centres
    blocks = D.samples_device(torch.from_numpy(cs).to(dev), CUBE, 32, fidx, 4, (FH, FW), PARAS, FLIP)[0]
    img = DV.Renderer(store, 32, 8)(blocks).cpu()
    cube = np.array(CUBE)
    for b in range(6):
        crop, _ = ND.crop(frames[fidx[b]].astype(np.float32), cs[b], cube, (32, 32), PARAS)
        want = ND.normalize(crop.max(), crop, cs[b], cube).astype(np.float32)
        assert torch.equal(img[b, 0], torch.from_numpy(want)), b
    # a refused window renders the constant background, reading nothing
    bad = D.samples_device(torch.tensor([[-500.0, 10.0, 900.0]], dtype=torch.float64, device=dev), CUBE, 32, [0], 4, (FH, FW), PARAS, FLIP)[0]
    assert torch.equal(DV.Renderer(store, 32, 1)(bad).cpu(), torch.ones(1, 1, 32, 32))


def test_unprojection_equals_the_device_evaluator(mods, dev):
    D, E = mods.D, mods.E
    r = np.random.RandomState(11)
    B, J, nv = 5, 14, 3
    pred = r.uniform(-1, 1, (B, J, 3)).astype(np.float32)
    s = r.uniform(0.2, 0.6, B)
    M = np.zeros((B, 3, 3), np.float32)
    M[:, 0, 0] = M[:, 1, 1] = s
    M[:, 0, 2], M[:, 1, 2], M[:, 2, 2] = r.uniform(-300, 300, B), r.uniform(-300, 300, B), 1.0
    center = np.stack([r.uniform(-150, 150, B), r.uniform(-120, 120, B), r.uniform(500, 1000, B)], 1).astype(np.float32)
    cube = np.repeat(r.uniform(250, 350, (B, 1)), 3, 1).astype(np.float32)
    gt = r.uniform(-1, 1, (B, J, 3)).astype(np.float32)
    t = [torch.from_numpy(a).to(dev) for a in (pred, center, M, cube)]
    ev = E.DeviceEvalUtil(128, NYU_PARAS, FLIP, J, device=dev)
    ev.feed_batch(t[0], torch.from_numpy(gt).to(dev), t[1], t[2], t[3], n_valid=nv)
    want_uvd = np.array(ev.jt_uvd_pred)
    uvd0 = torch.full((B, J, 3), -7.0, device=dev)
    xyz0 = torch.full((B, J, 3), -7.0, device=dev)
    uvd, xyz, st = D.unproject_device(*t, 128, NYU_PARAS, FLIP, n_valid=nv, uvd_out=uvd0, xyz_out=xyz0)
    assert torch.equal(uvd[:nv].cpu(), torch.from_numpy(want_uvd))
    assert torch.equal(xyz[:nv].cpu(), torch.from_numpy(E.uvd2xyz(uvd[:nv].cpu().numpy(), NYU_PARAS, FLIP)))
    assert (uvd[nv:] == -7.0).all() and (xyz[nv:] == -7.0).all() and st.tolist() == [0] * B
    # a singular and a non-finite matrix: NaN rows and a code, the other frames as before
    M2 = M.copy()
    M2[1] = 0.0
    M2[2, 0, 0] = np.nan
    u2, x2, st2 = D.unproject_device(t[0], t[1], torch.from_numpy(M2).to(dev), t[3], 128, NYU_PARAS, FLIP)
    assert st2.tolist() == [0, 1, 2, 0, 0]
    assert torch.isnan(u2[1:3]).all() and torch.isnan(x2[1:3]).all() and torch.equal(u2[0], uvd[0]) and torch.equal(x2[0], xyz[0])
    assert not torch.isnan(u2[3:]).any()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
EH, EW, S, J = 120, 160, 64, 14
E_PARAS = (147.0, 146.8, 80.0, 60.0)                # NYU's intrinsics scaled to a 160 x 120 frame


def blob_frames():
    """two frames: a far plane and a blob of about 40 x 40 pixels at 600 ... 640 mm, at different places"""
    f = np.full((2, EH, EW), 1400, np.uint16)
    vv, uu = np.mgrid[0:EH, 0:EW]
    known = []
    for b, (cu, cv) in enumerate(((60, 50), (100, 70))):
        m = (np.abs(uu - cu) <= 20) & (np.abs(vv - cv) <= 20)
        f[b][m] = (600 + (uu[m] + vv[m]) % 41).astype(np.uint16)
        d = f[b][m].astype(np.float64).mean()
        known.append(((cu - E_PARAS[2]) * d / E_PARAS[0], (cv - E_PARAS[3]) * d / E_PARAS[1] * FLIP, d))
    return f, np.array(known)


@pytest.fixture(scope="module")
def e2e(mods, dev):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()
    frames, known = blob_frames()
    given = awr_amd.Predictor(net, S, 1.0, cube=CUBE, paras=E_PARAS, flip=FLIP, max_batch=2, frame_shape=(EH, EW), refine_iters=0)
    auto = awr_amd.Predictor(net, S, 1.0, cube=CUBE, paras=E_PARAS, flip=FLIP, max_batch=2, frame_shape=(EH, EW), seed="nearest",
                             depth_range=(200.0, 1200.0), slab=100.0, refine_iters=2)
    return types.SimpleNamespace(net=net, frames=frames, known=known, given=given, auto=auto)


def test_predictor_equals_the_hand_assembled_pipeline(mods, dev, e2e):
    from awr_amd.trainer import InferEngine
    D, DV = mods.D, mods.DV
    centers = np.array([(61.0, 49.0, 622.0), (99.5, 71.25, 618.0)])
    out = e2e.given.predict(e2e.frames, centers_uvd=centers)
    e2e.given.check()
    assert out.status.tolist() == [0, 0] and out.xyz.shape == (2, J, 3) and out.uvd.is_cuda
    # by hand: host blocks -> Renderer -> InferEngine -> awr_joints_unproject
    blocks, M, cxyz, cube, st = D.sample_blocks(centers, CUBE, S, E_PARAS, FLIP, (EH, EW))
    store = make_store(e2e.frames, dev)
    img = DV.Renderer(store, S, 2)(DV.blocks_to_tensor(blocks))
    jt = InferEngine(e2e.net, 2, S, 1.0)(img)
    uvd, xyz, ust = D.unproject_device(jt, torch.from_numpy(cxyz).to(dev), torch.from_numpy(M).to(dev), torch.from_numpy(cube).to(dev), S, E_PARAS, FLIP)
    assert ust.tolist() == [0, 0] and not torch.isnan(uvd).any()
    assert torch.equal(out.uvd, uvd) and torch.equal(out.xyz, xyz)
    assert torch.equal(out.M.cpu(), torch.from_numpy(M)) and torch.equal(out.center_xyz.cpu(), torch.from_numpy(cxyz))
    # host tensors and device tensors are the same frames
    again = e2e.given.predict(torch.from_numpy(e2e.frames).to(dev), centers_uvd=torch.from_numpy(centers).to(dev))
    assert torch.equal(again.uvd, uvd) and torch.equal(again.xyz, xyz)


def test_predictor_detects_the_blob(mods, dev, e2e):
    out = e2e.auto.predict(e2e.frames)
    e2e.auto.check()
    gap = (out.center_xyz.cpu().double() - torch.from_numpy(e2e.known)).abs().max().item()
    print("detected centre vs the blob's: %.3e mm" % gap)
    assert gap < 1.0 and not torch.isnan(out.xyz).any()
    # the detector's centre is the restatement's
    ref = [mods.D.detect(f, seed="nearest", cube=CUBE, paras=E_PARAS, depth_range=(200.0, 1200.0), slab=100.0, iters=2)[0] for f in e2e.frames]
    assert torch.equal(out.center_xyz.cpu(), torch.from_numpy(mods.E.uvd2xyz(np.array(ref), E_PARAS, FLIP)))


def test_a_padded_batch_gives_the_same_bits(mods, dev, e2e):
    both = e2e.auto.predict(e2e.frames)
    uvd2, xyz2 = both.uvd.clone(), both.xyz.clone()
    for b in (0, 1):
        one = e2e.auto.predict(e2e.frames[b:b + 1])
        assert one.xyz.shape == (1, J, 3) and torch.equal(one.uvd[0], uvd2[b]) and torch.equal(one.xyz[0], xyz2[b])
        assert torch.equal(one.center_xyz[0], both.center_xyz[b]) and one.status.tolist() == [0]


def test_check_names_the_empty_frame(mods, dev, e2e):
    frames = e2e.frames.copy()
    frames[1] = 0
    out = e2e.auto.predict(frames)
    with pytest.raises(mods.L.AwrError, match=r"frame 1 .*AWR_DET_EMPTY"):
        e2e.auto.check()
    assert out.status.tolist() == [0, mods.D.EMPTY] and torch.isnan(out.xyz[1]).all() and torch.isnan(out.uvd[1]).all()
    assert not torch.isnan(out.xyz[0]).any()
    with pytest.raises(mods.L.AwrError, match="max_batch"):
        e2e.auto.predict(np.zeros((3, EH, EW), np.uint16))
    with pytest.raises(mods.L.AwrError, match="uint16"):
        e2e.auto.predict(frames.astype(np.float32))
