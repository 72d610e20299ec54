"""GPU: awr_frames_foreground and awr_background_learn (csrc/awr_background.hip) against their numpy statements
awr_amd.background.foreground and learn -- np.array_equal of output, status and model on every case of tests/background_cases.py, in the
16-byte and in the scalar form, with guard words around the output and the model rows -- the frame indirection, per_row, n_valid, a chain
of adapting calls, the refusals, one run at 480 x 640, FrameStore.foreground, and awr_amd.Predictor(background=...) against a plain
Predictor fed the statement's frames, bit for bit."""
import types

import numpy as np
import pytest
import torch

import background_cases as BC

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORD = 1024, 0x5A5A          # pixels on either side of a guarded store (2048 bytes: the store itself stays 16-byte aligned)
PATTERN = 0x3C3C                          # what a model that must stay untouched, or an output that must not be written, is filled with


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def BG():
    import awr_amd  # noqa: F401
    from awr_amd import background
    return background


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """the module's predictors and references end with the module, at a quiet point"""
    import gc
    yield
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


class Guarded:
    """rows of uint16 pixels `shift` pixels into an allocation with guard words on either side"""

    def __init__(self, rows, dev, shift=0, fill=GUARD_WORD):
        rows = np.ascontiguousarray(rows, dtype=np.uint16) if isinstance(rows, np.ndarray) else np.full(rows, fill, np.uint16)
        self.n, self.lo = rows.size, GUARD + shift
        self.flat = torch.full((2 * GUARD + shift + self.n + 8,), GUARD_WORD, dtype=torch.int16, device=dev).view(torch.uint16)
        self.t = self.flat[self.lo:self.lo + self.n].view(rows.shape)
        self.t.copy_(torch.from_numpy(rows.copy()).to(dev))

    def host(self, what):
        h = self.flat.cpu().numpy()
        assert (h[:self.lo] == GUARD_WORD).all() and (h[self.lo + self.n:] == GUARD_WORD).all(), "%s: written outside the store" % what
        return h[self.lo:self.lo + self.n].reshape(tuple(self.t.shape)).copy()


def run(BG, store, idx, models, o, per_row, n_valid=None, shift_out=0, shift_model=0):
    """foreground_device over batch rows `idx` with a guarded output and guarded model rows -> numpy (out, status, models after)"""
    dev = store.data.device
    B = len(idx)
    out = Guarded((B, store.fh, store.fw), dev, shift_out)
    mod = Guarded(np.asarray(models), dev, shift_model)
    got, status = BG.foreground_device(store, np.asarray(idx, np.int64), mod.t, per_row=per_row, n_valid=n_valid, out=out.t, **o)
    assert got.data_ptr() == out.t.data_ptr() and tuple(status.shape) == (B,) and status.dtype == torch.int32
    return out.host("awr_frames_foreground's out"), status.cpu().numpy(), mod.host("awr_frames_foreground's model")


def want_rows(names, idx, models, o, per_row, n_valid=None):
    """the statement, row by row: row b reads case names[idx[b]]'s frame and model row (per_row ? b : 0); rows at or past n_valid do not adapt"""
    n_valid = len(idx) if n_valid is None else n_valid
    models = np.array(models)
    outs, status = [], []
    import awr_amd  # noqa: F401
    from awr_amd import background as BGs
    for b, i in enumerate(idx):
        r = b if per_row else 0
        if not 0 <= i < len(names):
            outs.append(np.zeros(models.shape[1:], np.uint16))
            status.append(2)
            continue
        out, new = BGs.foreground(BC.apply_cases()[names[i]][0], models[r], **o)
        outs.append(out)
        status.append(0)
        if b < n_valid:
            models[r] = new
    return np.stack(outs), np.array(status, np.int32), models


def check(BG, dev, names, idx, options, per_row=True, n_valid=None, shifts=(0, 0, 0)):
    store = make_store(np.stack([BC.apply_cases()[n][0] for n in names]), dev, shifts[0])
    case_models = np.stack([BC.apply_cases()[n][1] for n in names])
    for o in options:
        if o["adapt"] is not None and not per_row and len(idx) > 1:
            continue                                # (refused: test_refusals)
        models = np.stack([case_models[i % len(names)] for i in idx]) if per_row else case_models[idx[0] % len(names)][None]
        want, want_status, want_models = want_rows(names, idx, models, o, per_row, n_valid)
        got, status, got_models = run(BG, store, idx, models, o, per_row, n_valid, shifts[1], shifts[2])
        assert np.array_equal(status, want_status), o
        assert np.array_equal(got, want), o
        assert np.array_equal(got_models, want_models), o
        if o["adapt"] is None:
            assert np.array_equal(got_models, models)


@pytest.mark.parametrize("shape", BC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_case_and_option(BG, dev, shape):
    """B = the cases of a shape, a model row per batch row: 48 x 64 and 16 x 8 take the 16-byte form, 37 x 53 the scalar form"""
    names = BC.apply_groups()[shape]
    check(BG, dev, names, list(range(len(names))), BC.options())
    check(BG, dev, names, [1], BC.options(thin=True))                                   # B = 1
    check(BG, dev, names, [0], BC.options(thin=True), per_row=False)                    # ... on a shared model, adapting too


@pytest.mark.parametrize("shape", BC.SHAPES[:2], ids=lambda s: "%dx%d" % s)
def test_permuted_and_bad_frame_indices(BG, dev, shape):
    names = BC.apply_groups()[shape]
    n = len(names)
    for idx in ([2, 0, 1], [3, n, 1], [-1, 4, 4], [n + 5], [1, 0, 3, 2, 5]):
        check(BG, dev, names, idx, BC.options(thin=True))
        check(BG, dev, names, idx, [dict(margin=30.0, unknown="keep", adapt=None), dict(margin=0, unknown="drop", adapt=None)], per_row=False)
    store = make_store(np.stack([BC.apply_cases()[x][0] for x in names]), dev)
    models = np.stack([BC.apply_cases()[names[0]][1]] * 3)
    got, status, after = run(BG, store, [0, n, 0], models, dict(margin=30.0, unknown="keep", adapt=9), True)
    assert status.tolist() == [0, 2, 0] and not got[1].any() and np.array_equal(after[1], models[1]) and np.array_equal(after[0], after[2])
    assert not np.array_equal(after[0], models[0])


@pytest.mark.parametrize("shifts", ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 4, 4), (8, 8, 8)),
                         ids=lambda s: "in%d_out%d_model%d" % s)
def test_shifted_bases(BG, dev, shifts):
    """the store, the output and the model shifted by 2 and by 8 bytes: any base off a 16-byte boundary takes the scalar form, all on one
    keeps the 16-byte form"""
    for shape in BC.SHAPES[:2]:
        names = BC.apply_groups()[shape]
        check(BG, dev, names, [0, 1, 5], BC.options(thin=True), shifts=shifts)


def test_the_form_without_adapt_never_writes_the_model(BG, dev):
    for shape in BC.SHAPES:
        names = BC.apply_groups()[shape]
        store = make_store(np.stack([BC.apply_cases()[n][0] for n in names]), dev)
        models = np.full((3,) + shape, PATTERN, np.uint16)
        for per_row in (True, False):
            got, status, after = run(BG, store, [0, 1, 2], models, dict(margin=30.0, unknown="drop", adapt=None), per_row)
            assert (after == PATTERN).all() and status.tolist() == [0, 0, 0]
            want = np.stack([BG.foreground(BC.apply_cases()[names[i]][0], models[0], unknown="drop")[0] for i in range(3)])
            assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", BC.SHAPES[:2], ids=lambda s: "%dx%d" % s)
def test_rows_past_n_valid_are_filtered_but_do_not_adapt(BG, dev, shape):
    names = BC.apply_groups()[shape]
    for n_valid in (0, 1, 2, 3):
        check(BG, dev, names, [0, 1, 0], [dict(margin=30.0, unknown="keep", adapt=4), dict(margin=0, unknown="drop", adapt=65535)], n_valid=n_valid)
    store = make_store(np.stack([BC.apply_cases()[n][0] for n in names]), dev)
    models = np.stack([BC.apply_cases()[names[0]][1]] * 3)
    got, _, after = run(BG, store, [0, 0, 0], models, dict(margin=30.0, unknown="keep", adapt=4), True, n_valid=1)
    assert np.array_equal(after[1:], models[1:]) and not np.array_equal(after[0], models[0])
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


@pytest.mark.parametrize("shape", BC.SHAPES[:2], ids=lambda s: "%dx%d" % s)
def test_a_chain_of_six_adapting_calls(BG, dev, shape):
    names = BC.apply_groups()[shape]
    frames = [BC.apply_cases()[n][0] for n in names]
    store = make_store(np.stack(frames), dev)
    model = Guarded(np.stack([BC.apply_cases()[names[0]][1], BC.apply_cases()[names[1]][1]]), dev)
    want = model.host("the model")
    o = dict(margin=12.7, unknown="keep", adapt=7)
    for call in range(6):
        idx = [call % len(names), (call + 2) % len(names)]
        got, status = BG.foreground_device(store, np.asarray(idx, np.int64), model.t, per_row=True, **o)
        for b, i in enumerate(idx):
            out, want[b] = BG.foreground(frames[i], want[b], **o)
            assert np.array_equal(got[b].cpu().numpy(), out), (call, b)
        assert np.array_equal(model.host("the model"), want), call


@pytest.mark.parametrize("n", (1, 2, 63, 64))
def test_learning(BG, dev, n):
    for shape in BC.SHAPES:
        store = make_store(BC.learn_frames(shape, n), dev, shift=1 if shape[1] == 53 else 0)
        for o in BC.learn_options(n):
            out = Guarded((shape), dev)
            order = np.arange(n)[::-1].copy() if o["rank"] == "median" else np.arange(n)          # (the order of the list cannot matter)
            got, status = BG.learn_device(store, order, out=out.t, **o)
            assert got.data_ptr() == out.t.data_ptr() and status.tolist() == [0]
            assert np.array_equal(out.host("awr_background_learn's model"), BC.learn_reference(shape, n, o["rank"], o["min_valid"])), (shape, o)
    # a listed index outside the store contributes no value and sets the status word
    shape = BC.SHAPES[1]
    store = make_store(BC.learn_frames(shape, n), dev)
    idx = np.arange(n)
    idx[n // 2] = n if n % 2 else -1
    got, status = BG.learn_device(store, idx, rank="median", min_valid=1)
    assert status.tolist() == [2] and np.array_equal(got.cpu().numpy(), BC.learn_reference(shape, n, "median", 1, zeroed=(n // 2,)))


def test_refusals_launch_nothing(BG, dev):
    from awr_amd import _lib as L
    shape = BC.SHAPES[0]
    names = BC.apply_groups()[shape]
    store = make_store(np.stack([BC.apply_cases()[n][0] for n in names[:4]]), dev)
    before = store.data.cpu().numpy().copy()
    out = torch.full((2,) + shape, PATTERN, dtype=torch.int16, device=dev).view(torch.uint16)
    model = torch.full((2,) + shape, PATTERN, dtype=torch.int16, device=dev).view(torch.uint16)
    idx = np.array([0, 1], np.int64)
    fg = lambda **kw: BG.foreground_device(store, kw.pop("idx", idx), kw.pop("model", model), out=kw.pop("out", out), **kw)
    for kw, word in ((dict(out=store.data[:2]), r"out \[.*overlaps the frame store"), (dict(out=store.data[3:].view(-1)[-8:].view(1, 1, 8), idx=idx[:1]), r"out \[.*overlaps the frame store"),
                     (dict(model=store.data[2:]), r"the model \[.*overlaps the frame store"), (dict(model=out), r"the model \[.*overlaps out"),
                     (dict(adapt=3), "adapt = 3 with per_row = 0 and B = 2"), (dict(per_row=True, model=model[:1]), "model_rows = 1"),
                     (dict(n_valid=3), "n_valid = 3"), (dict(n_valid=-1), "n_valid = -1"), (dict(margin=-1.0), "margin = -1"),
                     (dict(margin=float("nan")), "margin"), (dict(adapt=65536), "adapt = 65536")):
        with pytest.raises(L.AwrError, match="awr_frames_foreground: .*" + word):
            fg(**kw)
    with pytest.raises(L.AwrError, match="uint16"):
        BG.foreground_device(types.SimpleNamespace(data=store.data, ftype=1, fh=shape[0], fw=shape[1]), idx, model, out=out)
    with pytest.raises(L.AwrError, match="B = 0"):
        BG.foreground_device(store, np.zeros(0, np.int64), model, out=out)
    # learning
    for kw, word in ((dict(rank="median", min_valid=5, idx=np.arange(4)), "min_valid = 5"), (dict(idx=np.zeros(65, np.int64)), "n = 65"),
                     (dict(idx=np.zeros(0, np.int64)), "n = 0"), (dict(out=store.data[1]), r"model_out \[.*overlaps the frame store")):
        with pytest.raises(L.AwrError, match="awr_background_learn: .*" + word):
            BG.learn_device(store, kw.pop("idx", np.arange(3)), out=kw.pop("out", model[0]), **kw)
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == PATTERN).all() and (model.view(torch.int16) == PATTERN).all()
    assert np.array_equal(store.data.cpu().numpy(), before)
    # rows of the same allocation right behind the store's rows are fine, as awr_frames_denoise's are
    whole = make_store(np.concatenate([before, np.zeros_like(before[:2])]), dev)
    part = types.SimpleNamespace(data=whole.data[:4], ftype=0, fh=shape[0], fw=shape[1], n=4)
    m = torch.from_numpy(np.array(BC.apply_cases()[names[0]][1])).to(dev)
    got, status = BG.foreground_device(part, idx, m, out=whole.data[4:])
    assert status.tolist() == [0, 0] and np.array_equal(got.cpu().numpy(), np.stack([BG.foreground(before[i], m.cpu().numpy())[0] for i in idx]))


# ---- 480 x 640 -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    sc = BC.scene()
    return types.SimpleNamespace(host=sc, **{k: torch.from_numpy(np.array(v)).to(dev) for k, v in vars(sc).items()})


def test_full_frames(BG, dev, scene):
    sc = scene.host
    store = types.SimpleNamespace(data=scene.empty, ftype=0, fh=BC.FULL[0], fw=BC.FULL[1], n=BC.N_EMPTY)
    out = Guarded(BC.FULL, dev)
    _, status = BG.learn_device(store, np.arange(BC.N_EMPTY), out=out.t)
    assert status.tolist() == [0] and np.array_equal(out.host("the learnt model"), sc.model)
    assert np.array_equal(BG.learn_device(store, np.arange(BC.N_EMPTY), rank="max", min_valid=2)[0].cpu().numpy(), BG.learn(sc.empty, "max", 2))
    store = types.SimpleNamespace(data=scene.frames, ftype=0, fh=BC.FULL[0], fw=BC.FULL[1], n=BC.N_SCENE)
    models = np.stack([sc.model, sc.model])
    got, status, after = run(BG, store, [0, 1], models, dict(margin=30.0, unknown="keep", adapt=None), False)
    assert status.tolist() == [0, 0] and np.array_equal(got, sc.masked[:2]) and np.array_equal(after, models)
    got, status, after = run(BG, store, [1, 2], models, dict(margin=10, unknown="drop", adapt=3), True)
    for b, i in enumerate((1, 2)):
        want, new = BG.foreground(sc.frames[i], sc.model, margin=10, unknown="drop", adapt=3)
        assert np.array_equal(got[b], want) and np.array_equal(after[b], new)
    assert np.array_equal(scene.frames.cpu().numpy(), sc.frames)          # the input is only read


def test_frame_store_foreground(BG, dev, scene):
    from awr_amd import nyu_device as DV
    sc = scene.host
    store = DV.FrameStore.from_device(scene.frames)
    out = store.foreground(sc.model, chunk=2)                                # two launches: 2 frames and 1
    assert isinstance(out, DV.FrameStore) and (out.n, out.fh, out.fw, out.ftype) == (BC.N_SCENE,) + BC.FULL + (0,) and out.data.data_ptr() != store.data.data_ptr()
    assert np.array_equal(out.data.cpu().numpy(), sc.masked)
    got = store.foreground(scene.model, margin=0, unknown="drop").data.cpu().numpy()
    assert np.array_equal(got[2], BG.foreground(sc.frames[2], sc.model, margin=0, unknown="drop")[0])
    with pytest.raises(ValueError, match="adapt"):
        store.foreground(sc.model, adapt=2)
    with pytest.raises(ValueError, match="unknown options"):
        store.foreground(sc.model, shared=False)
    with pytest.raises(ValueError, match="model must be"):
        store.foreground(sc.model[:10])
    with pytest.raises(ValueError, match="float32"):
        DV.FrameStore.from_device(torch.zeros((1, 8, 8), device=dev)).foreground(np.zeros((8, 8), np.uint16))


# ---- the Predictor ---------------------------------------------------------------------------------------------------------------------
S, J, NB = 64, 14, BC.N_SCENE


@pytest.fixture(scope="module")
def e2e(scene):
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()

    def make(max_batch=NB, **kw):
        return awr_amd.Predictor(net, S, 1.0, max_batch=max_batch, **kw)
    return types.SimpleNamespace(make=make, scene=scene, sc=scene.host)


def same(a, b):
    """bit-equal tensors, NaN positions equal"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def same_fields(got, want):
    assert type(got) is type(want)
    for f in got._fields:
        assert same(getattr(got, f), getattr(want, f)), f


def test_predictor_without_background_never_calls_the_entry_points(e2e, monkeypatch):
    from awr_amd import _lib as L
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for kw in (dict(), dict(hands=2, isolate=True, edge_mm=40), dict(denoise=True), dict(background=None)):
        pred = e2e.make(**kw)
        pred.predict(e2e.scene.frames)
        assert "awr_detect" in calls and "awr_frames_foreground" not in calls and "awr_background_learn" not in calls
        assert pred.background is None and "background" not in vars(pred)
        assert not any(a in vars(pred) for a in ("_sensor", "_bg_model", "_bg_status", "sensor_frames", "background_status"))
        for method in (lambda: pred.learn_background(e2e.sc.empty), lambda: pred.reset_background(), lambda: pred.background_model):
            with pytest.raises(L.AwrError, match="background="):
                method()
        calls.clear()
    pred = e2e.make(background=True, denoise=True)
    calls.clear()                              # (the constructor's calls: the engine's plan)
    pred.predict(e2e.scene.frames)
    assert calls.count("awr_frames_foreground") == 1 and calls[:2] == ["awr_frames_foreground", "awr_frames_denoise"]
    assert pred.background == dict(margin=30.0, unknown="keep", adapt=None, shared=True, rank="median", min_valid=1)
    pred.learn_background(e2e.sc.empty)
    assert calls.count("awr_background_learn") == 1
    with pytest.raises(ValueError, match="shared=True and max_batch = 3"):
        e2e.make(background=dict(adapt=2))
    with pytest.raises(L.AwrError, match="ONE shared model"):
        pred.reset_background(slots=[0])


def test_background_without_a_learnt_model_equals_the_plain_predictor(e2e):
    plain, pred = e2e.make(confidence=True), e2e.make(confidence=True, background=True)
    want, got = plain.predict(e2e.scene.frames), pred.predict(e2e.scene.frames)
    same_fields(got, want)
    assert torch.equal(pred._frames[:NB].view(torch.int16), e2e.scene.frames.view(torch.int16))
    assert tuple(pred.background_model.shape) == (1,) + BC.FULL and not pred.background_model.view(torch.int16).any()
    # ... and after a reset too
    pred.learn_background(e2e.sc.empty)
    assert not same(pred.predict(e2e.scene.frames).xyz, want.xyz)
    pred.reset_background()
    same_fields(pred.predict(e2e.scene.frames), want)


@pytest.mark.parametrize("options", (dict(), dict(hands=2, isolate=True, min_pixels=200), dict(denoise=True)), ids=("one_hand", "two_hands_isolated", "denoise"))
def test_background_equals_a_plain_predictor_on_the_statement(e2e, options):
    from awr_amd import detect as D
    sc = e2e.sc
    plain_options = {k: v for k, v in options.items() if k != "denoise"}
    fed = sc.masked
    if "denoise" in options:
        fed = np.stack([D.denoise(f, **D.DENOISE_DEFAULTS) for f in sc.masked])          # sensor -> foreground -> denoise
    plain, pred = e2e.make(**plain_options), e2e.make(background=True, **options)
    pred.learn_background(sc.empty)                                          # numpy, host
    assert pred.background_learn_status.tolist() == [0] and np.array_equal(pred.background_model.cpu().numpy()[0], sc.model)
    want, got = plain.predict(torch.from_numpy(fed)), pred.predict(e2e.scene.frames)
    same_fields(got, want)
    assert (got.status == 0).any() and not torch.isnan(got.xyz[got.status == 0]).any()
    assert pred.sensor_frames.shape == (NB,) + BC.FULL and torch.equal(pred.sensor_frames.view(torch.int16), e2e.scene.frames.view(torch.int16))
    assert pred.background_status.dtype == torch.int32 and pred.background_status.tolist() == [0] * NB
    assert np.array_equal(pred._frames[:NB].cpu().numpy(), fed)
    if "denoise" in options:
        assert np.array_equal(pred.raw_frames.cpu().numpy(), sc.masked)      # raw_frames keeps its meaning: what denoise read
    if "hands" in options:
        for a in ("hand_info", "isolated"):
            assert same(getattr(pred, a), getattr(plain, a)), a
    pred.check()
    # a model handed in from outside, on the device, does the same
    other = e2e.make(background=True, **options)
    other.set_background(e2e.scene.model)
    same_fields(other.predict(e2e.scene.frames), want)


def test_background_with_the_tracker_a_short_batch_and_n_valid(e2e):
    sc = e2e.sc
    kw = dict(track=True, recenter=1, max_batch=4)
    plain, pred = e2e.make(**kw), e2e.make(background=dict(shared=False), **kw)
    pred.learn_background(e2e.scene.empty)                                   # a device tensor; every slot takes the model
    assert tuple(pred.background_model.shape) == (4,) + BC.FULL and np.array_equal(pred.background_model.cpu().numpy()[3], sc.model)
    for _ in range(2):
        want, got = plain.predict(torch.from_numpy(sc.masked), n_valid=2), pred.predict(e2e.scene.frames, n_valid=2)
        for f in got._fields:
            assert same(getattr(got, f)[:2], getattr(want, f)[:2]), f
        assert same(pred.next_centers_uvd[:2], plain.next_centers_uvd[:2])
        assert np.array_equal(pred._frames[:NB].cpu().numpy(), sc.masked)      # rows past n_valid are filtered too
    # slots: only the named ones change
    pred.reset_background(slots=[1])
    after = pred.background_model.cpu().numpy()
    assert not after[1].any() and np.array_equal(after[0], sc.model) and np.array_equal(after[2], sc.model)
    pred.set_background(sc.model + np.uint16(1), slots=[3])
    assert np.array_equal(pred.background_model.cpu().numpy()[3], sc.model + 1) and np.array_equal(pred.background_model.cpu().numpy()[2], sc.model)


def test_adapting_models_follow_the_statements_chain(e2e, BG):
    sc = e2e.sc
    pred = e2e.make(background=dict(shared=False, adapt=2, margin=20.0))
    pred.learn_background(sc.empty[:3])
    models = np.stack([BG.learn(sc.empty[:3])] * NB)
    for call in range(3):
        frames = np.roll(sc.frames, call, 0)
        pred.predict(frames, n_valid=2)
        for b in range(NB):
            out, new = BG.foreground(frames[b], models[b], margin=20.0, adapt=2)
            assert np.array_equal(pred._frames[b].cpu().numpy(), out), (call, b)
            if b < 2:
                models[b] = new
        assert np.array_equal(pred.background_model.cpu().numpy(), models), call
    assert not np.array_equal(models[0], models[2])


def test_clutter_nearer_than_the_hand(e2e, BG):
    """the premise first: on the cluttered composite the plain predictor's "nearest" centre lies on the bar.  With the model the centre is
    the plain predictor's on the CLUTTER-FREE frame masked the same way"""
    sc = e2e.sc
    plain = e2e.make()
    on_bar = plain.predict(e2e.scene.frames)
    assert (on_bar.status == 0).all() and ((on_bar.center_xyz[:, 2] - BC.BAR_MM).abs() < 60).all()
    pred = e2e.make(background=True)
    pred.learn_background(sc.empty)
    got = pred.predict(e2e.scene.frames)
    want = plain.predict(torch.from_numpy(np.stack([BG.foreground(f, sc.model)[0] for f in sc.hands])))
    assert same(got.center_xyz, want.center_xyz) and (got.status == 0).all() and (got.center_xyz[:, 2] > 600).all()
    same_fields(got, want)
