"""CPU: the synthetic hand (awr_amd/synth.py) -- kinematics, labels, the numpy statement of the renderer, the golden table, the
half-integer guard that lets tests/test_synth_gpu.py demand np.array_equal, awr_synth_render's argument checks and the host dataset."""
import ctypes as C

import numpy as np
import pytest

import synth_cases as SC


@pytest.fixture(scope="module")
def synth():
    import awr_amd  # noqa: F401
    from awr_amd import synth
    return synth


# ---- kinematics and labels -------------------------------------------------------------------------------------------------------------
def test_every_bone_keeps_its_length_under_every_pose(synth):
    for forearm, edge in ((True, False), (False, True)):
        m = synth.HandModel(forearm=forearm)
        p = synth.sample_poses(200, 3, m, edge=edge)
        J, prims, bbox = synth.forward_kinematics(p, m)
        assert J.shape == (200, 21, 3) and prims.shape == (200, m.K, 8) and bbox.shape == (200, 4) and bbox.dtype == np.int32
        assert m.K == (22 if forearm else 21) and m.K <= synth.MAX_PRIMS
        length = np.linalg.norm(J[:, 1:] - J[:, synth.PARENT[1:]], axis=-1)
        assert np.abs(length - m.bone_lengths()[1:] * p["scale"][:, None]).max() < 1e-9
        assert (m.bone_lengths()[1:] > 15).all() and (m.bone_lengths()[1:] < 110).all()          # millimetres of an adult hand
        assert (prims[:, :, 6] > 0).all() and (prims[:, :, 7] == 0).all() and np.isfinite(prims).all()
        assert (J[:, :, 2] > 200).all()                                                          # in front of the camera
        if forearm:
            arm = prims[:, -1]
            assert np.allclose(arm[:, 0:3], J[:, 0]) and np.allclose(np.linalg.norm(arm[:, 3:6] - arm[:, 0:3], axis=-1), 250.0 * p["scale"])


def test_poses_are_reproducible_per_seed_and_differ_between_seeds(synth):
    a, b, c = (synth.sample_poses(20, s, edge=e) for s, e in ((7, False), (7, False), (8, False)))
    assert sorted(a) == sorted(b) == ["abduct", "euler", "flex", "position", "scale", "thumb_base"]
    for k in a:
        assert np.array_equal(a[k], b[k]) and not np.array_equal(a[k], c[k]), k
    m = synth.HandModel
    assert (a["flex"][:, 1:] >= [f[0] for f in m.FLEX]).all() and (a["flex"][:, 1:] <= [f[1] for f in m.FLEX]).all()
    assert (a["flex"][:, 0] >= [f[0] for f in m.THUMB_FLEX]).all() and (a["flex"][:, 0] <= [f[1] for f in m.THUMB_FLEX]).all()
    assert (a["position"][:, 2] > 350).all() and (a["position"][:, 2] < 1050).all()
    ja, jb = synth.forward_kinematics(a)[0], synth.forward_kinematics(b)[0]
    assert np.array_equal(ja, jb)
    # default poses keep the drawn hand centre inside the frame; edge=True also draws hands whose centre leaves it
    from awr_amd.evaluator import xyz2uvd
    from awr_amd import nyu_data as ND
    inside = lambda uv: ((uv[:, 0] >= 0) & (uv[:, 0] <= 639) & (uv[:, 1] >= 0) & (uv[:, 1] <= 479))
    for edge, want_all in ((False, True), (True, False)):
        p = synth.sample_poses(300, 5, edge=edge)
        _, cen = synth.labels(synth.forward_kinematics(p)[0])
        ok = inside(xyz2uvd(cen, ND.PARAS, -1))
        assert ok.all() if want_all else (not ok.all() and ok.mean() > 0.5)


def test_label_order_and_centres(synth):
    J = synth.forward_kinematics(synth.sample_poses(9, 2))[0]
    lab, cen = synth.labels(J, 14)
    tip, mid, base = (lambda f: 4 + 4 * f), (lambda f: 2 + 4 * f), (lambda f: 1 + 4 * f)
    T, I, M, R, P = range(5)
    want = [tip(P), mid(P), tip(R), mid(R), tip(M), mid(M), tip(I), mid(I), tip(T), mid(T), base(T)]
    assert lab.shape == (9, 14, 3) and np.array_equal(lab[:, :11], J[:, want])
    across = J[:, base(I)] - J[:, base(P)]
    assert np.allclose(lab[:, 11], J[:, 0] + 0.3 * across) and np.allclose(lab[:, 12], J[:, 0] - 0.3 * across)
    assert np.allclose(lab[:, 13], (J[:, 0] + J[:, [base(f) for f in (I, M, R, P)]].sum(1)) / 5)
    assert np.allclose(cen, lab.mean(1), rtol=0, atol=1e-12)
    lab21, cen21 = synth.labels(J, 21)
    assert np.array_equal(lab21, J) and np.allclose(cen21, J.mean(1), rtol=0, atol=1e-12)
    a, b = synth.labels(J, 14, center_jitter_mm=5.0, seed=1)[1], synth.labels(J, 14, center_jitter_mm=5.0, seed=1)[1]
    assert np.array_equal(a, b) and 0 < np.abs(a - cen).max() <= 5.0
    with pytest.raises(ValueError):
        synth.labels(J, 16)
    # the skeleton the visualiser draws joins exactly these: (tip, mid) per finger, thumb chain, everything to the palm (13)
    from awr_amd.vis_tool import _SKELETON
    assert _SKELETON["nyu"][4][0] == (8, 9, 10, 11, 12, 13)


# ---- the statement's geometry ----------------------------------------------------------------------------------------------------------
def _joint_pixels_are_hits(synth, n, seed, frame_shape, paras, **pose_kw):
    """Every skeletal joint lies on a capsule axis, so a sphere about it with the radius r of its thinnest capsule lies inside the hand.
    The nearest pixel centre is at most 0.71 pixels from the joint's projection, so its ray passes the joint at rho <= 0.71 z / fx; the pose
    options keep rho < 0.9 r.  Then the ray enters that sphere -- the pixel is a hit -- at a depth within [z - r - 1, z + 1]: the entry
    lies sqrt(r^2 - rho^2) / |d| before the point of closest approach, whose depth exceeds z by at most rho / 2 (x / (1 + x^2) <= 1 / 2),
    and 0.45 r - 0.44 r / 1.21 < 1 for every radius of the model.  The hand's own depth there is a hit no deeper than the sphere's,
    whatever else of the hand is in front.  (A lower bound on the HAND's depth does not exist: another finger, or the joint's own phalanx
    pointing at the camera, may be far in front of it; the sphere carries the lower bound.)"""
    from awr_amd.evaluator import xyz2uvd
    fh, fw = frame_shape
    m = synth.HandModel()
    p = synth.sample_poses(n, seed, m, frame_shape=frame_shape, paras=paras, **pose_kw)
    J, prims, bbox = synth.forward_kinematics(p, m, frame_shape, paras)
    assert 0.71 * J[:, :, 2].max() / paras[0] < 0.9 * m.RADII.min() * p["scale"].min()
    frames, raw = synth.render(prims, bbox, frame_shape, paras, return_unrounded=True)
    uvd = xyz2uvd(J, paras, -1).astype(np.float64)
    checked = 0
    for i in range(n):
        for j in range(21):
            u, v = int(np.floor(uvd[i, j, 0] + 0.5)), int(np.floor(uvd[i, j, 1] + 0.5))
            if not (0 <= u < fw and 0 <= v < fh):
                continue
            z = J[i, j, 2]
            own = [k for k in range(20) if j in (k + 1, synth.PARENT[k + 1])]                    # capsule k joins PARENT[k + 1] and k + 1
            r = prims[i, own, 6].min()
            ball = np.array([[[*J[i, j], *J[i, j], r, 0.0]]])
            solo = synth.render(ball, np.array([[u, v, u + 1, v + 1]]), frame_shape, paras, return_unrounded=True)[1][0, v, u]
            assert z - r - 1 <= solo <= z + 1, (i, j, solo, z, r)
            assert frames[i, v, u] > 0 and raw[i, v, u] <= solo + 1e-6 and raw[i, v, u] <= z + 1, (i, j, raw[i, v, u], solo, z)
            checked += 1
    return checked


def test_joint_pixels_are_hits_small_frames(synth):
    assert _joint_pixels_are_hits(synth, 12, 21, SC.SMALL, SC.small_paras(), z_range=(200.0, 260.0), scale_range=(1.05, 1.15)) > 150


def test_joint_pixels_are_hits_full_frame(synth):
    from awr_amd import nyu_data as ND
    assert _joint_pixels_are_hits(synth, 1, 22, SC.FULL, ND.PARAS) == 21


def test_sphere_depth_is_analytic_and_nothing_behind_the_camera_hits(synth):
    sp = SC.small_paras()
    # a sphere on the optical axis of pixel (40, 10): the centre pixel sees |c| - r along a ray of length-per-depth sqrt(dd)
    u, v, zc, r = 40, 10, 700.0, 45.0
    dx, dy = (u - sp[2]) / sp[0], -1 * ((v - sp[3]) / sp[1])
    c = np.array([dx * zc, dy * zc, zc])
    prims = np.zeros((1, 3, 8))
    prims[0, 1] = (*c, *c, r, 0.0)
    frames, raw = synth.render(prims, synth.prim_boxes(prims, SC.SMALL, sp), SC.SMALL, sp, return_unrounded=True)
    want = zc - r / np.sqrt(dx * dx + dy * dy + 1.0)
    assert abs(raw[0, v, u] - want) < 1e-9 and frames[0, v, u] == int(np.floor(want + 0.5))
    assert 20 < np.isfinite(raw[0]).sum() < 80 and (raw[0][np.isfinite(raw[0])] < zc).all()      # a disc of about pi (r fx / z)^2 pixels
    # the same sphere and a capsule, wholly at z <= 0
    behind = np.zeros((1, 2, 8))
    behind[0, 0] = (c[0], c[1], -zc, c[0], c[1], -zc, r, 0.0)
    behind[0, 1] = (-50.0, 10.0, -300.0, 60.0, -20.0, -20.0, 20.0, 0.0)
    full = np.array([[0, 0, SC.SMALL[1], SC.SMALL[0]]])
    f, z, st = synth.render(behind, full, SC.SMALL, sp, return_unrounded=True, return_status=True)
    assert not f.any() and not np.isfinite(z).any() and st.tolist() == [synth.EMPTY]
    assert synth.prim_boxes(behind, SC.SMALL, sp).tolist() == [[0, 0, 0, 0]]


def test_status_codes_of_the_special_frames(synth):
    frames, raw, st = SC.reference("special")
    want = {"outside": synth.EMPTY, "nan_row": synth.BAD_PRIM}
    assert st.tolist() == [want.get(k, synth.OK) for k in SC.SPECIAL]
    i = SC.SPECIAL.index
    assert not frames[i("outside")].any() and not frames[i("nan_row")].any()
    assert np.array_equal(frames[i("neighbour")], synth.render(SC.cases()["special"]["prims"][i("neighbour")][None], SC.cases()["special"]["bbox"][i("neighbour")][None],
                                                               **SC.render_kw(SC.cases()["special"]))[0])
    for k, (col, row) in {"cut_left": (0, None), "cut_right": (-1, None), "cut_top": (None, 0), "cut_bottom": (None, -1)}.items():
        f = frames[i(k)]
        assert (f[:, col] if col is not None else f[row]).any(), k                               # the hand reaches that border
    assert frames[i("crosses_z0")].any() and SC.cases()["special"]["bbox"][i("crosses_z0")].tolist() == [0, 0, 64, 48]
    thin = frames[i("thin_far")]
    assert 0 < np.count_nonzero(thin) < 64 and thin.max() > 4900                                # a broken line of single pixels
    # with a wall every frame is full, the wall carries noise, and nothing lies behind it
    wf, _, wst = SC.reference("special_flip_wall_noise")
    assert wf.min() >= 1 and wf.max() <= 900 + 3 and wst[i("outside")] == synth.EMPTY and wst[i("nan_row")] == synth.BAD_PRIM
    assert len(np.unique(wf[i("outside")])) == 7


def test_computed_box_equals_full_frame(synth):
    for name, c in SC.cases().items():
        if c["frame_shape"] == SC.FULL and "K32" in name:
            continue                                                                             # (one full-size case is enough here)
        fh, fw = c["frame_shape"]
        full = np.tile(np.array([0, 0, fw, fh], np.int32), (len(c["prims"]), 1))
        got = synth.render(c["prims"], full, **SC.render_kw(c))
        assert np.array_equal(got, SC.reference(name)[0]), name
        assert (c["bbox"][:, 2] <= fw).all() and (c["bbox"][:, 3] <= fh).all() and (c["bbox"] >= 0).all()
    small = SC.cases()["small_n3_K22"]["bbox"]
    assert ((small[:, 2] - small[:, 0]) * (small[:, 3] - small[:, 1]) < 48 * 64).any()           # the box does cut something away


def test_chunks_equal_one_call_with_noise(synth):
    c = SC.cases()["small_n17_K32_flip_wall_noise"]
    kw = SC.render_kw(c)
    whole = SC.reference(c["name"])[0]
    parts = []
    for lo, hi in ((0, 5), (5, 6), (6, 17)):
        parts.append(synth.render(c["prims"][lo:hi], c["bbox"][lo:hi], **dict(kw, frame0=kw["frame0"] + lo)))
    assert np.array_equal(np.concatenate(parts), whole)
    assert not np.array_equal(synth.render(c["prims"][:2], c["bbox"][:2], **dict(kw, frame0=kw["frame0"] + 1)), whole[:2])      # the index matters
    assert not np.array_equal(synth.render(c["prims"][:2], c["bbox"][:2], **dict(kw, seed=kw["seed"] + 1)), whole[:2])
    # the noise is an integer of [-a, a] on hit pixels, and every value of the range occurs
    clean = synth.render(c["prims"], c["bbox"], **dict(kw, noise_mm=0))
    d = whole.astype(np.int64) - clean.astype(np.int64)
    assert sorted(np.unique(d).tolist()) == [-3, -2, -1, 0, 1, 2, 3]
    h = synth.hash_u32(5, 7, np.arange(6))
    assert h.dtype == np.uint32 and len(set(h.tolist())) == 6 and np.array_equal(h, synth.hash_u32(5, 7 + 2 ** 32, np.arange(6)))


def test_no_unrounded_depth_is_near_a_half_integer(synth):
    """The guard behind the GPU file's np.array_equal: the device's float64 square root may differ from numpy's by 1 ulp (about 1e-13 mm
    in z); that can change a rounded depth only if the unrounded one sits within that of k + 0.5.  On every input the two files and the
    golden use, none lies within 1e-6 mm."""
    def check(name, raw):
        z = raw[np.isfinite(raw)]
        if z.size:
            assert np.abs((z - np.floor(z)) - 0.5).min() > 1e-6, name
        return z.size
    n = 0
    for name in SC.cases():
        n += check(name, SC.reference(name)[1])
    for c, _ in SC.golden_cases():
        n += check(c["name"], synth.render(c["prims"], c["bbox"], return_unrounded=True, **SC.render_kw(c))[1])
    assert n > 30000


def test_golden_table_reproduces_the_golden_frames(synth):
    tags = []
    for c, want in SC.golden_cases():
        got, st = synth.render(c["prims"], c["bbox"], return_status=True, **SC.render_kw(c))
        assert got.dtype == np.uint16 and np.array_equal(got, want) and not st.any(), c["name"]
        tags.append((c["background_mm"] > 0, c["noise_mm"] > 0))
    assert (False, True) in tags and (True, True) in tags and (False, False) in tags           # a noisy frame and a wall frame are in it
    import os
    assert os.path.getsize(SC.GOLDEN) < 64 * 1024


def test_statement_refuses_bad_arguments(synth):
    p, b = np.zeros((1, 33, 8)), np.zeros((1, 4), np.int32)
    with pytest.raises(ValueError):
        synth.render(p, b, SC.SMALL)
    with pytest.raises(ValueError):
        synth.render(p[:, :2], b, SC.SMALL, flip=0)
    with pytest.raises(ValueError):
        synth.render(p[:, :2], b, SC.SMALL, paras=(0.0, 1.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        synth.render(p[:, :2], np.zeros((2, 4), np.int32), SC.SMALL)


# ---- the C entry point without a GPU ---------------------------------------------------------------------------------------------------
def test_awr_synth_render_validates_its_arguments_without_gpu():
    """argument checks run before any launch (as tests/test_abi.py does for other entry points); the pointers are never dereferenced"""
    import awr_amd  # noqa: F401
    from awr_amd import _lib as L
    assert "awr_synth_render" in L.EXPORTS and not L.MISSING
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)

    def call(prims=p, bbox=p, n=1, K=22, fh=48, fw=64, fx=58.8, fy=58.7, u0=32.0, v0=24.0, flip=-1, bg=0, noise=0, seed=0, frame0=0, out=p, row=0,
             cap=1, status=p):
        return L.lib.awr_synth_render(prims, bbox, n, K, fh, fw, fx, fy, u0, v0, flip, bg, noise, seed, frame0, out, row, cap, status, None)
    for kw, word in ((dict(prims=None), "NULL"), (dict(bbox=None), "NULL"), (dict(out=None), "NULL"), (dict(status=None), "NULL"),
                     (dict(K=33), "K = 33"), (dict(K=0), "K = 0"), (dict(n=0), "n = 0"), (dict(n=-3), "n = -3"), (dict(n=65536, cap=1 << 20), "n = 65536"),
                     (dict(flip=0), "flip"), (dict(flip=2), "flip"), (dict(fx=0.0), "focal"), (dict(fy=0.0), "focal"), (dict(fx=float("nan")), "focal"),
                     (dict(fh=0), "frame of"), (dict(fw=16385), "frame of"), (dict(bg=65536), "background_mm"), (dict(noise=-1), "noise_mm"),
                     (dict(frame0=-1), "frame0"), (dict(row=-1), "rows"), (dict(row=1), "rows"), (dict(n=2), "rows")):
        assert call(**kw) == -1 and word in L.last_error(), (kw, L.last_error())
    import torch
    with pytest.raises(L.AwrError):
        from awr_amd import synth
        synth.render_device(np.zeros((1, 2, 8)), np.zeros((1, 4), np.int32), torch.zeros((1, 48, 64), dtype=torch.uint16))      # a host tensor


# ---- the host dataset --------------------------------------------------------------------------------------------------------------------
def test_host_dataset_yields_the_nyu_tuple_and_round_trips(synth):
    import torch
    from awr_amd import nyu_data as ND
    from awr_amd.evaluator import EvalUtil
    sf = synth.SyntheticFrames(6, 3, "test", device=None)
    assert sf.frames.shape == (6, 480, 640) and sf.frames.dtype == np.uint16 and sf.status.tolist() == [0] * 6 and sf.check() == 0
    assert sf.labels_xyz.shape == (6, 14, 3) and sf.centers.shape == (6, 3) and sf.joints21.shape == (6, 21, 3) and sf.frame_store is None
    ds = sf.dataset
    assert isinstance(ds, ND.NYU) and len(ds) == 6 and (ds.test_cube == 300.0).all() and ds.test_cube.shape == (6, 3)
    ev = EvalUtil(128, ds.paras, ds.flip, 14)
    for i in range(6):
        img, jt_xyz, jt_uvd, center, M, cube = ds[i]
        assert [tuple(t.shape) for t in (img, jt_xyz, jt_uvd, center, M, cube)] == [(1, 128, 128), (14, 3), (14, 3), (3,), (3, 3), (3,)]
        assert all(t.dtype == torch.float32 for t in (img, jt_xyz, jt_uvd, center, M, cube))
        assert float(img.min()) >= -1.0 and 0.999 < float(img.max()) <= 1.0 and float((img < 1).float().mean()) > 0.03      # a hand in front of the far plane
        ev.feed_batch(jt_uvd[None].numpy(), jt_xyz[None].numpy(), center[None].numpy(), M[None].numpy(), cube[None].numpy())
    err = np.concatenate(ev._err, 0)
    assert err.shape == (6, 14) and err.max() < 1e-2
    # the train phase augments from the loader's own stream; a 21-joint set and a set without forearm build too
    tr = synth.SyntheticFrames(2, 4, "train", jt_num=21, aug_para=[10, 0.1, 180], device=None, forearm=False, noise_mm=2)
    assert tr.prims.shape == (2, 21, 8) and tuple(tr.dataset[1][1].shape) == (21, 3) and tr.dataset.aug_para == [10, 0.1, 180]
    same = synth.SyntheticFrames(2, 4, "train", jt_num=21, device=None, forearm=False, noise_mm=2)
    assert np.array_equal(same.frames, tr.frames) and not np.array_equal(sf.frames[:2], tr.frames)
