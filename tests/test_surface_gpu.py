"""GPU: awr_joints_surface (csrc/awr_surface.hip) against its numpy statement awr_amd.surface.joints_surface -- np.array_equal
of all four outputs on every case of tests/surface_cases.py (gaps as bit patterns), guard words around each output, rows at or past n_valid
untouched, a frame store whose base is shifted by one odd-width row, the refusals, two 480 x 640 procedural frames, and
awr_amd.Predictor(surface=True) in four configurations: its after-call tensors equal the statement applied to what predict() returned,
and what predict() returned equals a predictor without the option bit for bit."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

import surface_cases as SC

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import predictor_trace as PT  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORD = 256, 0x5A5A5A5A       # words on either side of every output, and what every output word holds before the launch
ODD_ROW = 67                              # a base shifted by one odd-width row: 134 bytes, 2-byte aligned and no more


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def SF():
    import awr_amd  # noqa: F401
    from awr_amd import surface
    return surface


def make_store(frames, dev, shift=0):
    """a FrameStore-like object over a copy of `frames`; it starts `shift` pixels (2 bytes each) into a 16-byte aligned allocation"""
    frames = np.ascontiguousarray(frames, dtype=np.uint16)
    flat = torch.zeros(frames.size + shift + 8, dtype=torch.int16, device=dev).view(torch.uint16)
    data = flat[shift:shift + frames.size].view(frames.shape)
    data.copy_(torch.from_numpy(np.array(frames)).to(dev))
    assert data.data_ptr() % 16 == (2 * shift) % 16
    return types.SimpleNamespace(data=data, ftype=0, fh=frames.shape[1], fw=frames.shape[2], n=frames.shape[0])


def guarded(words, dev):
    """-> (the whole allocation, its `words` int32 words in the middle), every word of both the guard pattern"""
    flat = torch.full((2 * GUARD + words,), GUARD_WORD, dtype=torch.int32, device=dev)
    return flat, flat[GUARD:GUARD + words]


@functools.lru_cache(maxsize=None)
def statement(name):
    """the numpy statement on a case, once; read-only"""
    from awr_amd import surface as SF
    c = SC.cases()[name]
    o = c["options"]
    if c["raw_bones"] is not None:
        out = SF._statement(c["frames"], c["frame_idx"], c["uvd"], c["status"], c["ustatus"], c["raw_bones"], o["samples"], o["radius"], o["in_mm"], o["out_mm"],
                            o["min_on"])
    else:
        out = SF.joints_surface(c["frames"], c["frame_idx"], c["uvd"], c["status"], c["ustatus"], **o)
    for a in out:
        a.setflags(write=False)
    return out


def launch(SF, dev, c, shift=0):
    """one launch over a case with guarded outputs -> numpy (codes, gap bits, counts, row_status), each (n, ...) with the guard pattern in
    the rows the launch left alone; the guards are checked here"""
    from awr_amd import _lib as L
    store = make_store(c["frames"], dev, shift)
    n, J = c["uvd"].shape[:2]
    o = c["options"]
    uvd, status, ustatus = (torch.from_numpy(np.array(c[k])).to(dev) for k in ("uvd", "status", "ustatus"))
    bufs = [guarded(w, dev) for w in (n * J, n * J, n * 8, n)]
    out = (bufs[0][1].view(n, J), bufs[1][1].view(torch.float32).view(n, J), bufs[2][1].view(n, 8), bufs[3][1])
    if c["raw_bones"] is not None:
        # the raw entry point: the wrappers refuse a bone index outside [0, J) before any launch, the kernel answers OUTSIDE
        bones = torch.from_numpy(np.array(c["raw_bones"])).to(dev)
        idx = torch.from_numpy(np.array(c["frame_idx"])).to(dev)
        SF.awr_joints_surface(store.data.data_ptr(), 0, store.n, store.fh, store.fw, idx.data_ptr(), L.ptr(uvd), L.ptr(status), L.ptr(ustatus), n, J,
                              c["n_valid"], L.ptr(bones), len(c["raw_bones"]), o["samples"], o["radius"], o["in_mm"], o["out_mm"], o["min_on"],
                              *(L.ptr(t) for t in out))
    else:
        got = SF.joints_surface_device(store, np.array(c["frame_idx"]), uvd, status, ustatus, n_valid=c["n_valid"], out=out, **o)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, out))
    host = []
    for (flat, mid), shape in zip(bufs, ((n, J), (n, J), (n, 8), (n,))):
        h = flat.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == GUARD_WORD).all() and (h[GUARD + mid.numel():] == GUARD_WORD).all(), "awr_joints_surface wrote outside an output"
        host.append(h[GUARD:GUARD + mid.numel()].reshape(shape))
    assert np.array_equal(store.data.cpu().numpy(), c["frames"])          # the frames are only read
    return host


def check(SF, dev, name, shift=0):
    c = SC.cases()[name]
    want = statement(name)
    got = launch(SF, dev, c, shift)
    nv = c["n_valid"]
    for g, w, what in zip(got, (want[0].view(np.uint32), SC.bits(want[1]), want[2].view(np.uint32), want[3].view(np.uint32)),
                          ("codes", "gap_mm", "counts", "row_status")):
        assert np.array_equal(g[:nv], w[:nv]), (name, what)
        assert (g[nv:] == GUARD_WORD).all(), (name, what, "a row at or past n_valid was written")


@pytest.mark.parametrize("name", list(SC.cases()))
def test_every_case(SF, dev, name):
    check(SF, dev, name)


def test_a_frame_store_shifted_by_one_odd_width_row(SF, dev):
    """every 37 x 67 case again, the store's base 134 bytes into its allocation: 2-byte aligned and no more"""
    names = [n for n, c in SC.cases().items() if c["frames"].shape[1:] == (37, 67)]
    assert len(names) >= 20
    for name in names:
        check(SF, dev, name, shift=ODD_ROW)


def test_refusals(SF, dev):
    from awr_amd import _lib as L
    c = SC.cases()["48x64_rows"]
    store = make_store(c["frames"], dev)
    n, J = c["uvd"].shape[:2]
    uvd, status, ustatus = (torch.from_numpy(np.array(c[k])).to(dev) for k in ("uvd", "status", "ustatus"))
    flat, mid = guarded(n * J, dev)
    out = (mid.view(n, J), torch.empty((n, J), dtype=torch.float32, device=dev), torch.empty((n, 8), dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev))

    def run(**kw):
        return SF.joints_surface_device(store, kw.pop("idx", np.array(c["frame_idx"])), kw.pop("uvd", uvd), status, ustatus, out=kw.pop("out", out), **kw)
    for kw, word in ((dict(radius=4), "radius = 4"), (dict(radius=-1), "radius = -1"), (dict(in_mm=-1.0), "in_mm = -1"), (dict(in_mm=float("inf")), "in_mm = inf"),
                     (dict(out_mm=float("nan")), "out_mm"), (dict(min_on=0), "min_on = 0"), (dict(min_on=10), r"min_on = 10 is outside \[1, 9\]"),
                     (dict(samples=0), "samples = 0"), (dict(samples=8), "samples = 8"), (dict(n_valid=n + 1), "n_valid = %d" % (n + 1)),
                     (dict(n_valid=-1), "n_valid = -1")):
        with pytest.raises(L.AwrError, match="awr_joints_surface: .*" + word):
            run(**kw)
    with pytest.raises(L.AwrError, match="uint16"):
        SF.joints_surface_device(types.SimpleNamespace(data=store.data, ftype=1, fh=48, fw=64), np.array(c["frame_idx"]), uvd, status, ustatus, out=out)
    with pytest.raises(L.AwrError, match="B = 0"):
        run(idx=np.zeros(0, np.int64), uvd=uvd[:0])
    with pytest.raises(L.AwrError, match=r"J = 257 is outside \[1, 256\]"):
        run(uvd=torch.zeros((n, 257, 3), dtype=torch.float32, device=dev), out=None, bones=[])
    # the wrappers refuse what is no number and a bone that names no joint themselves
    for kw, exc, word in ((dict(bones=[(0, J)]), ValueError, r"outside \[0, J = 3\)"), (dict(bones=[(-1, 0)]), ValueError, "outside"),
                          (dict(bones=[(0, 1)] * 65), ValueError, "65 pairs"), (dict(radius=1.5), TypeError, "radius"), (dict(in_mm="40"), TypeError, "in_mm")):
        with pytest.raises(exc, match=word):
            run(**kw)
    with pytest.raises(ValueError, match="float32"):
        run(uvd=uvd.double())
    torch.cuda.synchronize()
    assert (flat.cpu().numpy().view(np.uint32) == GUARD_WORD).all()          # nothing was launched
    # n_valid = 0 is no launch and no error
    run(n_valid=0)
    torch.cuda.synchronize()
    assert (flat.cpu().numpy().view(np.uint32) == GUARD_WORD).all()


# ---- 480 x 640: two procedural hands -----------------------------------------------------------------------------------------------------
def test_full_frames(SF, dev):
    from awr_amd import evaluator, nyu_data, synth
    poses = synth.sample_poses(2, 11)
    joints21, prims, bbox = synth.forward_kinematics(poses)
    frames = synth.render(prims, bbox)
    assert frames.shape == (2, 480, 640) and frames.any()
    zero = np.zeros(4, np.int32)
    for J, move in ((14, (0, 0, 0)), (14, (40, 0, 0)), (21, (0, 0, 60)), (21, (0, -20, 0))):
        lab = synth.labels(joints21, J)[0] + np.asarray(move, np.float64)
        uvd = evaluator.xyz2uvd(np.concatenate([lab, lab[::-1]]).astype(np.float32), nyu_data.PARAS, -1)          # rows 2, 3: the other hand's joints
        idx = np.array([0, 1, 0, 1])
        for o in (dict(), dict(radius=3, min_on=4, samples=7), dict(radius=0, in_mm=25.5, out_mm=4.25, samples=1)):
            c = SC.case("full", frames, uvd, frame_idx=idx, **o)
            want = SF.joints_surface(frames, idx, uvd, zero, zero, **c["options"])
            got = launch(SF, dev, c)
            assert np.array_equal(got[0], want[0].view(np.uint32)) and np.array_equal(got[1], SC.bits(want[1])), (J, move, o)
            assert np.array_equal(got[2], want[2].view(np.uint32)) and not got[3].any(), (J, move, o)
            assert want[2][:, 4:].sum() == 4 * o.get("samples", 3) * (13 if J == 14 else 20)
        if move == (0, 0, 0):
            assert not want[2][:2, SF.OFF].any() and want[2][:2, SF.ON].min() >= 10          # the true joints of a hand lie on its surface


# ---- the Predictor -----------------------------------------------------------------------------------------------------------------------
CONFIGS = {"plain": dict(), "hands2": dict(hands=2), "views": dict(views=PT.VIEWS), "denoise_smooth": dict(denoise=True, smooth=True)}


@pytest.fixture(scope="module")
def net():
    return PT.network()


def same(a, b):
    """bit-equal tensors, NaN positions equal"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("config", list(CONFIGS))
def test_predictor_surface(SF, net, config, monkeypatch):
    import awr_amd
    from awr_amd import _lib as L, detect
    kw = CONFIGS[config]
    K = kw.get("hands", 1)
    B, J = PT.B, PT.J
    plain = awr_amd.Predictor(net, PT.S, 1.0, max_batch=B, **PT.SMALL, **kw)
    options = True if config != "views" else dict(radius=2, in_mm=30.0, out_mm=10.0, min_on=2, samples=7)
    pred = awr_amd.Predictor(net, PT.S, 1.0, max_batch=B, **PT.SMALL, surface=options, **kw)
    o = dict(SF.SURFACE_DEFAULTS, **({} if options is True else options))
    assert pred.surface == o and plain.surface is None and "surface" not in vars(plain)
    assert not any(hasattr(plain, a) for a in ("surface_codes", "surface_gap_mm", "surface_counts", "surface_status", "_surface_bones"))
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    stored = np.stack([detect.denoise(f, **detect.DENOISE_DEFAULTS) for f in PT.FRAMES]) if "denoise" in kw else PT.FRAMES
    seen = set()
    for frames, extra in ((PT.WARM, dict()), (PT.FRAMES, dict()), (PT.FRAMES, dict(n_valid=1))):
        del calls[:]
        want = plain.predict(frames, **extra)
        assert "awr_joints_surface" not in calls
        del calls[:]
        out = pred.predict(frames, **extra)
        assert calls.count("awr_joints_surface") == 1 and calls[-1] == "awr_joints_surface"
        # the option changes nothing of what predict() returns (rows past n_valid hold unspecified values)
        nb, nv = len(frames), extra.get("n_valid", len(frames))
        assert type(out) is type(want) and all(same(getattr(out, f)[:nv], getattr(want, f)[:nv]) for f in out._fields)
        if frames is PT.WARM:
            continue
        assert np.array_equal(pred._frames[:nb].cpu().numpy(), stored)          # the stored frames: the denoised ones with denoise
        uvd = (pred.raw_uvd if "smooth" in kw else out.uvd).cpu().numpy().reshape(nb, K, J, 3)
        if "smooth" in kw:
            assert same(pred.raw_uvd[:nv], plain.raw_uvd[:nv]) and not same(out.uvd[:nv], pred.raw_uvd[:nv])          # the measurement, not the filtered joints
        status = out.status.cpu().numpy().reshape(nb, K)
        ustatus = pred._last[1].view(-1, B)[:K, :nb].cpu().numpy().T
        rows = [(b, k) for b in range(nv if K == 1 else nb) for k in range(K)]          # (hands: every row of the plan is valid)
        ws = SF.joints_surface(stored, [b for b, _ in rows], np.stack([uvd[b, k] for b, k in rows]), [status[b, k] for b, k in rows],
                               [ustatus[b, k] for b, k in rows], **o)
        shape = (nb,) if K == 1 else (nb, K)
        got = [t.cpu().numpy() for t in (pred.surface_codes, pred.surface_gap_mm, pred.surface_counts, pred.surface_status)]
        assert [g.shape for g in got] == [shape + (J,), shape + (J,), shape + (8,), shape]
        assert [g.dtype for g in got] == [np.int32, np.float32, np.int32, np.int32]
        for i, (b, k) in enumerate(rows):
            at = (b,) if K == 1 else (b, k)
            assert np.array_equal(got[0][at], ws[0][i]) and np.array_equal(SC.bits(got[1][at]), SC.bits(ws[1][i])), (config, at)
            assert np.array_equal(got[2][at], ws[2][i]) and got[3][at] == ws[3][i], (config, at)
            assert ws[3][i] == (0 if status[b, k] == 0 and ustatus[b, k] == 0 else 1)
            seen.update(ws[0][i].tolist())
        assert (got[3][:nv] == 0).all() if K == 1 else (got[3][:nv, 0] == 0).all()          # the nearest hand of every valid frame was predicted and checked
        assert got[2][(0,) if K == 1 else (0, 0)][4:].sum() == 13 * o["samples"]          # the NYU skeleton's bones
    assert seen & {SF.ON, SF.OCCLUDED, SF.OFF, SF.OUTSIDE}
    pred.check()
