"""GPU: awr_synth_render against the numpy statement awr_amd.synth.render -- np.array_equal on every pixel (tests/test_synth_cpu.py
establishes on these very inputs that no unrounded depth is within 1e-6 mm of a half-integer, so the 1 ulp latitude of the device's
float64 square root cannot show) -- and SyntheticFrames end to end: device loader, detector, Predictor, Trainer.  Inputs and the
statement's frames come from tests/synth_cases.py; each reference is computed once."""
import os

import numpy as np
import pytest
import torch

import synth_cases as SC

pytestmark = pytest.mark.gpu

POISON = 0xBEEF


@pytest.fixture(scope="module")
def synth():
    import awr_amd  # noqa: F401
    from awr_amd import synth
    assert torch.cuda.is_available()
    return synth


def render_into(synth, c, lo=0, hi=None, rows_before=1, rows_after=2, out=None, frame0=None):
    """frames [lo, hi) of a case -> rows [rows_before, ...) of a poisoned (rows_before + n + rows_after, fh, fw) tensor"""
    hi = len(c["prims"]) if hi is None else hi
    fh, fw = c["frame_shape"]
    if out is None:
        out = torch.from_numpy(np.full((rows_before + hi - lo + rows_after, fh, fw), POISON, np.uint16)).cuda()
    kw = SC.device_kw(c)
    kw["frame0"] = c["frame0"] + lo if frame0 is None else frame0
    status = synth.render_device(c["prims"][lo:hi], c["bbox"][lo:hi], out, row=rows_before, **kw)
    return out, status


@pytest.mark.parametrize("name", ["small_n3_K22", "small_n17_K32_flip_wall_noise", "small_n1_K1_sphere", "small_n1_K1_capsule_noise", "special",
                                  "special_flip_wall_noise", "width62_n3_noise", "full_n2_K22_noise", "full_n2_K32_flip_wall"])
def test_render_device_equals_the_statement_on_every_pixel(synth, name):
    c = SC.cases()[name]
    want, _, want_status = SC.reference(name)
    n = len(want)
    out, status = render_into(synth, c)
    got = out.cpu().numpy()
    assert status.dtype == torch.int32 and status.cpu().numpy().tolist() == want_status.tolist()
    bad = [(i, int((got[1 + i] != want[i]).sum())) for i in range(n) if not np.array_equal(got[1 + i], want[i])]
    assert not bad, "frames (index, differing pixels): %s" % bad
    assert np.array_equal(got[1:1 + n], want)
    # rows outside [row, row + n) keep the poison bit for bit
    assert (got[0] == POISON).all() and (got[1 + n:] == POISON).all()


def test_special_frames_status_and_neighbours(synth):
    """EMPTY for the hand outside the frame, BAD_PRIM for the NaN row -- both frames all background -- and the frames next to them exact"""
    c = SC.cases()["special"]
    want, _, _ = SC.reference("special")
    out, status = render_into(synth, c, rows_before=0, rows_after=0)
    got, st = out.cpu().numpy(), status.cpu().numpy()
    i = SC.SPECIAL.index
    assert st[i("outside")] == synth.EMPTY and st[i("nan_row")] == synth.BAD_PRIM and (np.delete(st, [i("outside"), i("nan_row")]) == synth.OK).all()
    assert not got[i("outside")].any() and not got[i("nan_row")].any()
    assert np.array_equal(got[i("neighbour")], want[i("neighbour")]) and got[i("neighbour")].any()
    assert np.array_equal(got[i("cut_bottom")], want[i("cut_bottom")])
    # an Inf, and a NaN radius, are refused the same way; a NaN in an UNUSED row is not looked at
    p = c["prims"][[i("neighbour")] * 3].copy()
    p[0, 7, 0] = np.inf
    p[1, 2, 6] = np.nan
    unused = np.zeros((3, 1, 8))
    unused[:, 0, :6] = np.nan
    p = np.concatenate([p, unused], 1)
    o = torch.from_numpy(np.zeros((3, 48, 64), np.uint16)).cuda()
    st = synth.render_device(p, c["bbox"][[i("neighbour")] * 3], o, **SC.device_kw(c)).cpu().numpy()
    assert st.tolist() == [synth.BAD_PRIM, synth.BAD_PRIM, synth.OK]
    o = o.cpu().numpy()
    assert not o[0].any() and not o[1].any() and np.array_equal(o[2], want[i("neighbour")])


def test_two_chunked_calls_equal_one_call(synth):
    c = SC.cases()["small_n17_K32_flip_wall_noise"]
    want = SC.reference(c["name"])[0]
    out, s1 = render_into(synth, c, 0, 6, rows_before=0, rows_after=11)
    st = torch.empty(11, dtype=torch.int32, device="cuda")
    synth.render_device(c["prims"][6:], c["bbox"][6:], out, row=6, status=st, **dict(SC.device_kw(c), frame0=c["frame0"] + 6))
    assert np.array_equal(out.cpu().numpy(), want) and not s1.cpu().numpy().any() and not st.cpu().numpy().any()
    # a tensor that is too small, a wrong dtype and a negative row are refused before anything is written
    from awr_amd import _lib as L
    with pytest.raises(L.AwrError, match="do not fit"):
        synth.render_device(c["prims"], c["bbox"], out, row=1, **SC.device_kw(c))
    with pytest.raises(L.AwrError):
        synth.render_device(c["prims"], c["bbox"], out.view(torch.int16), **SC.device_kw(c))
    assert np.array_equal(out.cpu().numpy(), want)


def test_golden_table_reproduces_the_golden_frames(synth):
    for c, want in SC.golden_cases():
        out, status = render_into(synth, c, rows_before=0, rows_after=0)
        assert np.array_equal(out.cpu().numpy(), want) and not status.cpu().numpy().any(), c["name"]


# ---- end to end at 480 x 640 -----------------------------------------------------------------------------------------------------------
N = 16


@pytest.fixture(scope="module")
def sets(synth):
    test = synth.SyntheticFrames(N, 5, "test")
    train = synth.SyntheticFrames(N, 6, "train", aug_para=[10, 0.1, 180], noise_mm=2)
    return test, train


def test_synthetic_frames_on_the_device(synth, sets):
    from awr_amd import nyu_device as DV
    for sf in sets:
        assert isinstance(sf.frame_store, DV.FrameStore) and sf.frame_store.data.shape == (N, 480, 640) and sf.frame_store.data.dtype == torch.uint16
        assert (sf.frame_store.n, sf.frame_store.fh, sf.frame_store.fw, sf.frame_store.ftype) == (N, 480, 640, 0)
        assert sf.status.is_cuda and sf.status.cpu().tolist() == [0] * N and sf.check() == 0
        assert isinstance(sf.dataset, DV.DeviceNYU) and sf.dataset.frame_store is sf.frame_store and (sf.dataset.test_cube == 300.0).all()
        # the chunked device render equals the statement (two frames are enough here; the kernel's cases are above)
        want = synth.render(sf.prims[:2], sf.bbox[:2], noise_mm=2 if sf.phase == "train" else 0, seed=sf.seed)
        assert np.array_equal(sf.frame_store.data[:2].cpu().numpy(), want)
    a, b = synth.SyntheticFrames(5, 6, "train", chunk=2, noise_mm=2), synth.SyntheticFrames(5, 6, "train", noise_mm=2)      # chunks of 2, 2, 1 against one call
    assert torch.equal(a.frame_store.data.view(torch.int16), b.frame_store.data.view(torch.int16)) and bool(a.frame_store.data.view(torch.int16).any())
    from awr_amd import _lib as L
    with pytest.raises(L.AwrError, match="device memory"):
        synth.SyntheticFrames(10 ** 7, 1, "test")


def test_device_loader_images_equal_the_host_loader_over_the_downloaded_frames(synth, sets):
    from awr_amd import nyu_data as ND
    from awr_amd import nyu_device as DV
    for sf in sets:
        kw = dict(img_size=128, aug_para=sf.dataset.aug_para)
        host = ND.NYU.from_arrays(sf.frames_host(), sf.labels_xyz, sf.centers, sf.phase, **kw)
        host.test_cube = np.ones([N, 3]) * host.cube
        dev = sf.dataset
        dev.aug.seed = np.random.RandomState(23455)              # the loader's stream from its start, like the host dataset's
        render = DV.Renderer(sf.frame_store, 128, N)
        items = [dev[i] for i in range(N)]
        img = render(torch.stack([it[0] for it in items])).cpu()
        render.check(N)
        for i in range(N):
            h = host[i]
            assert torch.equal(img[i], h[0]), (sf.phase, i)
            for a, b in zip(items[i][1:], h[1:]):
                assert torch.equal(a, b), (sf.phase, i)
        assert float((img < 1).float().mean()) > 0.03


def test_detector_on_the_store_equals_the_host_detector(synth, sets):
    from awr_amd import detect as D
    sf = sets[0]
    frames = sf.frames_host()
    centers, status = D.detect_device(sf.frame_store, np.arange(N))
    assert status.cpu().tolist() == [D.OK] * N
    want = np.array([D.detect(frames[i])[0] for i in range(N)], np.float64)
    assert np.array_equal(centers.cpu().numpy(), want)


def test_predictor_and_trainer_run_on_synthetic_frames(synth, sets, tmp_path):
    import awr_amd
    from awr_amd.config import Config
    from awr_amd.trainer import Trainer
    test, train = sets
    torch.manual_seed(0)
    net = awr_amd.get_deconv_net(18, 14, 2).cuda().eval()
    pred = awr_amd.Predictor(net, 128, 1.0, max_batch=N)
    out = pred.predict(test.frame_store.data)
    pred.check()
    assert out.status.cpu().tolist() == [0] * N and tuple(out.xyz.shape) == (N, 14, 3) and bool(torch.isfinite(out.xyz).all())

    class Cfg(Config):
        net, kernel_size, batch_size, num_workers, max_epoch, output_dir, load_model, exp_id, use_hipgraph, vis_freq, device_eval = \
            "resnet_18", 1.0, 8, 0, 1, os.path.join(str(tmp_path), "out"), "", "synth", False, 0, True
    tr = Trainer(Cfg(), train.dataset, test.dataset)
    assert sorted(tr._render) == ["test", "train"] and tr._render["train"].store is train.frame_store
    tr.train()                                                        # 16 frames in batches of 8: two steps
    mpe = tr.test(-1)
    assert np.isfinite(mpe) and mpe > 0
