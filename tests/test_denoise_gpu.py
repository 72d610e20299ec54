"""GPU: awr_frames_denoise (csrc/awr_denoise.hip) against its numpy statement awr_amd.detect.denoise -- np.array_equal on
every case of tests/denoise_cases.py over the grid at both radii, in the 8-byte and in the scalar form, with guard words around the output
store -- the frame indirection, the refusals, two noisy 480 x 640 frames, FrameStore.denoised, and awr_amd.Predictor(denoise=...) against
a plain Predictor fed the statement's frames, bit for bit."""
import functools
import types

import numpy as np
import pytest
import torch

import denoise_cases as DC

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORD = 1024, 0x5A5A          # pixels on either side of the output store (2048 bytes: the store itself stays 16-byte aligned)
ODD_ROW = 67                              # a base shifted by one odd-width row: 134 bytes, 2-byte aligned and no more


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """the module's shared references (some 200 MB of host memory over the whole grid) and its predictors end with the module: what they
    hold is released here, at a quiet point, not by the collector somewhere inside a later module's test"""
    import gc
    yield
    statement.cache_clear()
    noisy_statement.cache_clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def make_store(frames, dev, shift=0):
    """a FrameStore-like object over a copy of `frames`; it starts `shift` pixels (2 bytes each) into a 16-byte aligned allocation"""
    frames = np.ascontiguousarray(frames, dtype=np.uint16)
    flat = torch.zeros(frames.size + shift + 8, dtype=torch.int16, device=dev).view(torch.uint16)
    data = flat[shift:shift + frames.size].view(frames.shape)
    data.copy_(torch.from_numpy(np.array(frames)).to(dev))
    assert data.data_ptr() % 16 == (2 * shift) % 16
    return types.SimpleNamespace(data=data, ftype=0, fh=frames.shape[1], fw=frames.shape[2], n=frames.shape[0])


def run(D, store, idx, options, shift=0):
    """denoise_device over batch rows `idx` with a guarded output store `shift` pixels into its allocation -> numpy (out (B, fh, fw), status)"""
    dev = store.data.device
    B, npx = len(idx), store.fh * store.fw
    flat = torch.full((2 * GUARD + shift + B * npx + 8,), GUARD_WORD, dtype=torch.int16, device=dev).view(torch.uint16)
    lo = GUARD + shift
    out = flat[lo:lo + B * npx].view(B, store.fh, store.fw)
    got, status = D.denoise_device(store, np.asarray(idx, np.int64), out=out, **options)
    assert got.data_ptr() == out.data_ptr() and tuple(status.shape) == (B,) and status.dtype == torch.int32
    host = flat.cpu().numpy()
    assert (host[:lo] == GUARD_WORD).all() and (host[lo + B * npx:] == GUARD_WORD).all(), "awr_frames_denoise wrote outside its output store"
    return host[lo:lo + B * npx].reshape(B, store.fh, store.fw), status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def statement(name, radius, edge, support, fill):
    """awr_amd.detect.denoise on a case, once; read-only"""
    from awr_amd import detect
    out = detect.denoise(DC.cases()[name], radius, edge, support, fill)
    out.setflags(write=False)
    return out


def want_rows(names, idx, o):
    z = np.zeros(DC.cases()[names[0]].shape, np.uint16)
    rows = [statement(names[i], o["radius"], o["edge"], o["support"], o["fill"]) if 0 <= i < len(names) else z for i in idx]
    return np.stack(rows), np.array([0 if 0 <= i < len(names) else 2 for i in idx], np.int32)


def check(D, dev, names, idx, options, shift_in=0, shift_out=0):
    store = make_store(np.stack([DC.cases()[n] for n in names]), dev, shift_in)
    for o in options:
        want, want_status = want_rows(names, idx, o)
        got, status = run(D, store, idx, o, shift_out)
        assert np.array_equal(status, want_status), o
        for b, i in enumerate(idx):
            assert np.array_equal(got[b], want[b]), (names[i] if 0 <= i < len(names) else i, o)


def own_options(names, radius):
    seen, out = set(), []
    for n in names:
        for o in DC.OWN.get(n, []):
            if o["radius"] == radius and DC.opt_id(o) not in seen:
                seen.add(DC.opt_id(o))
                out.append(o)
    return out


@pytest.mark.parametrize("radius", (1, 2))
@pytest.mark.parametrize("shape", list(DC.groups()), ids=lambda s: "%dx%d" % s)
def test_every_case_over_the_grid(D, dev, shape, radius):
    """the whole grid, and the threshold cases' own options, one launch per option over all cases of a shape.  48 x 64 takes the 8-byte
    form (fw a multiple of 4, aligned bases); every other shape the scalar form (17 x 67: odd rows, 33 x 130: fw % 4 == 2)"""
    names = DC.groups()[shape]
    check(D, dev, names, list(range(len(names))), DC.grid(radius) + own_options(names, radius))


@pytest.mark.parametrize("shifts", ((1, 1), (ODD_ROW, ODD_ROW), (0, 1), (2, 0), (4, 4)), ids=lambda s: "in%d_out%d" % s)
@pytest.mark.parametrize("shape", DC.ODD + DC.TILES, ids=lambda s: "%dx%d" % s)
def test_shifted_bases(D, dev, shape, shifts):
    """an aligned size behind a base shifted by one pixel, by one odd-width row, on the input or the output alone: the scalar form; a
    base shifted by 8 bytes keeps the 8-byte form"""
    names = DC.groups()[shape]
    for radius in (1, 2):
        check(D, dev, names, list(range(len(names))), DC.grid(radius, thin=True) + own_options(names, radius), *shifts)


@pytest.mark.parametrize("shape", [(48, 64), (33, 130)], ids=lambda s: "%dx%d" % s)
def test_frame_indirection_and_bad_indices(D, dev, shape):
    """B = 1, 3 and 5 and more: repeated and permuted indices, -1 and n_frames in the middle -- a zero row, BAD_FRAME, the neighbours what
    they are alone"""
    names = DC.groups()[shape][:9]
    n = len(names)
    options = [dict(radius=1, edge=40, support=1, fill=6), dict(radius=2, edge=None, support=0, fill=1)]
    for idx in ([4], [n], [-1], [2, 2, 2], [5, -1, 5], [8, 0, 4, 0, 8], [3, n, 1, -1, 3], [n - 1, 3, 0, 3, n + 5, 1, 3, -7, 4]):
        check(D, dev, names, idx, options)
        got, status = run(D, make_store(np.stack([DC.cases()[x] for x in names]), dev), idx, options[0])
        bad = np.array([not 0 <= i < n for i in idx])
        assert (status[bad] == D.BAD_FRAME).all() and (status[~bad] == D.OK).all() and not got[bad].any()


def test_an_overlapping_out_is_refused_and_nothing_is_launched(D, dev):
    from awr_amd import _lib as L
    frames = np.stack([DC.cases()["48x64_random_zeros"]] * 3)
    store = make_store(frames, dev)
    before = store.data.cpu().numpy().copy()
    idx = [0, 1]
    tail = torch.full((2, 48, 64), GUARD_WORD, dtype=torch.int16, device=dev).view(torch.uint16)
    for out in (store.data[:2], store.data[1:], store.data[2:].view(-1)[-8:].view(1, 1, 8)):
        with pytest.raises(L.AwrError, match=r"awr_frames_denoise: out \[.*overlaps the frame store"):
            D.denoise_device(store, idx if out.shape[0] == 2 else [0], out=out, fill=1)
    torch.cuda.synchronize()
    assert np.array_equal(store.data.cpu().numpy(), before)
    # rows of the same allocation right behind the store's rows are fine, as awr_hands_isolate's are
    whole = make_store(np.concatenate([frames, np.zeros_like(frames[:2])]), dev)
    part = types.SimpleNamespace(data=whole.data[:3], ftype=0, fh=48, fw=64, n=3)
    got, status = D.denoise_device(part, idx, out=whole.data[3:], fill=1)
    assert status.tolist() == [0, 0] and np.array_equal(got.cpu().numpy(), np.stack([D.denoise(frames[i], fill=1) for i in idx]))
    assert (tail.view(torch.int16) == GUARD_WORD).all()
    # the other refusals name the entry point and the value, and come before any launch
    for kw, word in ((dict(radius=3), "radius = 3"), (dict(edge=-1.0), "edge = -1"), (dict(edge=float("nan")), "edge"), (dict(support=9), "support = 9"),
                     (dict(radius=2, fill=25), "fill = 25")):
        with pytest.raises(L.AwrError, match="awr_frames_denoise: .*" + word):
            D.denoise_device(store, idx, **kw)
    with pytest.raises(L.AwrError, match="uint16"):
        D.denoise_device(types.SimpleNamespace(data=store.data, ftype=1, fh=48, fw=64), idx)
    with pytest.raises(L.AwrError, match="B = 0"):
        D.denoise_device(store, np.zeros(0, np.int64), out=tail)
    torch.cuda.synchronize()


# ---- 480 x 640: two noisy hands, rendered on the device ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy(dev):
    from awr_amd import synth as SY
    pa, ba, pb, bb = DC.noisy_hands()
    fa = torch.empty((DC.N_FULL,) + DC.FULL, dtype=torch.uint16, device=dev)
    fb = torch.empty_like(fa)
    SY.render_device(pa, ba, fa, noise_mm=DC.NOISE_MM, seed=1)
    SY.render_device(pb, bb, fb, noise_mm=DC.NOISE_MM, seed=2)
    both = SY.compose(fa, fb)
    assert np.array_equal(both.cpu().numpy(), DC.noisy_host())
    return both


@functools.lru_cache(maxsize=None)
def noisy_statement(i, radius, edge, support, fill):
    from awr_amd import detect
    return detect.denoise(DC.noisy_host()[i], radius, edge, support, fill)


def test_full_frames(D, dev, noisy):
    store = types.SimpleNamespace(data=noisy, ftype=0, fh=DC.FULL[0], fw=DC.FULL[1], n=DC.N_FULL)
    for o in DC.FULL_OPTIONS:
        got, status = run(D, store, [0, 1], o)
        assert status.tolist() == [0, 0]
        for i in range(DC.N_FULL):
            assert np.array_equal(got[i], noisy_statement(i, **o)), (i, o)
    assert np.array_equal(noisy.cpu().numpy(), DC.noisy_host())          # the input is only read


def test_frame_store_denoised(D, dev, noisy):
    from awr_amd import nyu_device as DV
    frames = torch.cat([noisy.view(torch.int16), noisy.view(torch.int16)[:1]]).view(torch.uint16)
    store = DV.FrameStore.from_device(frames)
    o = DC.FULL_OPTIONS[1]
    out = store.denoised(chunk=2, **o)                                      # two launches: 2 frames and 1
    assert isinstance(out, DV.FrameStore) and (out.n, out.fh, out.fw, out.ftype) == (3,) + DC.FULL + (0,) and out.data.data_ptr() != store.data.data_ptr()
    host = out.data.cpu().numpy()
    for row, i in enumerate((0, 1, 0)):
        assert np.array_equal(host[row], noisy_statement(i, **o))
    assert np.array_equal(store.denoised().data.cpu().numpy()[1], noisy_statement(1, **D.DENOISE_DEFAULTS))
    with pytest.raises(ValueError, match="denoise"):
        store.denoised(window=3)
    with pytest.raises(ValueError, match="float32"):
        DV.FrameStore.from_device(torch.zeros((1, 8, 8), device=dev)).denoised()


# ---- the Predictor ---------------------------------------------------------------------------------------------------------------------
S, J, NB = 64, 14, DC.N_FULL


@pytest.fixture(scope="module")
def e2e(noisy):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()

    def make(max_batch=NB, **kw):
        return awr_amd.Predictor(net, S, 1.0, max_batch=max_batch, **kw)

    def filtered(o):
        return torch.from_numpy(np.stack([noisy_statement(i, o["radius"], o["edge"], o["support"], o["fill"]) for i in range(NB)]))
    return types.SimpleNamespace(make=make, frames=noisy, filtered=filtered)


def same(a, b):
    """bit-equal tensors, NaN positions equal"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_predictor_without_denoise_never_calls_the_entry_point(e2e, monkeypatch):
    from awr_amd import _lib as L
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for kw in (dict(), dict(hands=2, isolate=True, edge_mm=40), dict(denoise=None)):
        pred = e2e.make(**kw)
        pred.predict(e2e.frames)
        assert "awr_detect" in calls and "awr_frames_denoise" not in calls
        assert pred.denoise is None and "denoise" not in vars(pred) and not any(hasattr(pred, a) for a in ("_raw", "raw_frames", "denoise_status"))
        calls.clear()
    pred = e2e.make(denoise=True)
    calls.clear()                              # (the constructor's calls: the engine's plan)
    pred.predict(e2e.frames)
    assert calls.count("awr_frames_denoise") == 1 and calls[0] == "awr_frames_denoise" and pred.denoise == dict(radius=1, edge=40.0, support=0, fill=None)


@pytest.mark.parametrize("options", (dict(), dict(hands=2, isolate=True, edge_mm=40, min_pixels=200)), ids=("one_hand", "two_hands_isolated"))
def test_predictor_denoise_equals_a_plain_predictor_on_the_statement(e2e, options):
    for opts in (True, dict(radius=2, edge=40, support=6, fill=18)):
        o = dict(radius=1, edge=40.0, support=0, fill=None) if opts is True else opts
        plain, pred = e2e.make(**options), e2e.make(denoise=opts, **options)
        want = plain.predict(e2e.filtered(o))
        got = pred.predict(e2e.frames)
        assert type(got) is type(want)
        for f in got._fields:
            assert same(getattr(got, f), getattr(want, f)), (f, opts)
        assert (got.status == 0).any() and not torch.isnan(got.xyz[got.status == 0]).any()
        # the raw frames are kept, the store holds the filtered ones, the launch's codes are OK
        assert pred.raw_frames.shape == (NB,) + DC.FULL and torch.equal(pred.raw_frames.view(torch.int16), e2e.frames.view(torch.int16))
        assert torch.equal(pred._frames[:NB].view(torch.int16).cpu(), e2e.filtered(o).view(torch.int16))
        assert pred.denoise_status.shape == (NB,) and pred.denoise_status.dtype == torch.int32 and pred.denoise_status.tolist() == [0] * NB
        if "hands" in options:
            for a in ("hand_info", "isolated"):
                assert same(getattr(pred, a), getattr(plain, a)), a
        pred.check()
    # the unfiltered frames give other bits: the option does something
    raw = e2e.make(**options).predict(e2e.frames)
    assert not same(raw.xyz, got.xyz)


def test_predictor_denoise_with_a_short_batch_given_centres_and_the_tracker(e2e):
    """one frame in a plan of three, centres handed in, and track + recenter: the filter runs in front of all of them"""
    o = dict(radius=1, edge=40.0, support=0, fill=None)
    one = e2e.filtered(o)[:1]
    plain, pred = e2e.make(max_batch=3), e2e.make(max_batch=3, denoise=True)
    want, got = plain.predict(one), pred.predict(e2e.frames[:1])
    assert all(same(getattr(got, f), getattr(want, f)) for f in got._fields) and pred.raw_frames.shape[0] == 1 and pred.denoise_status.tolist() == [0]
    centers = torch.tensor([[320.0, 240.0, 800.0]], dtype=torch.float64)
    want, got = plain.predict(one, centers_uvd=centers), pred.predict(e2e.frames[:1], centers_uvd=centers)
    assert all(same(getattr(got, f), getattr(want, f)) for f in got._fields)
    plain, pred = e2e.make(track=True, recenter=1, palm=True), e2e.make(track=True, recenter=1, palm=True, denoise=True)
    for _ in range(2):
        want, got = plain.predict(e2e.filtered(o)), pred.predict(e2e.frames)
        assert all(same(getattr(got, f), getattr(want, f)) for f in got._fields)
        assert same(pred.next_centers_uvd, plain.next_centers_uvd) and same(pred.palm_info, plain.palm_info)
