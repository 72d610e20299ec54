"""GPU: awr_hands_isolate (csrc/awr_isolate.hip) against its numpy statement awr_amd.detect.isolate -- np.array_equal on
every case, in the 8-pixel and in the scalar form, with guard words around the output store -- and awr_amd.Predictor(hands=2,
isolate=True) on the near-hand composites against a plain Predictor fed each hand's OWN frame in the same row positions, torch.equal."""
import types

import numpy as np
import pytest
import torch

import isolate_cases as IC

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORD = 1024, 0x5A5A          # pixels on either side of the output store (2048 bytes: the store itself stays 16-byte aligned)
GROUPS = IC.groups()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def u16(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.uint16)).to(dev)          # (a copy: the shared inputs are read-only)


def make_store(frames, dev, shift=0):
    """a FrameStore-like object over a copy of `frames`; shift = 1 starts it one pixel (2 bytes) into its allocation: no 16-byte alignment"""
    frames = np.ascontiguousarray(frames, dtype=np.uint16)
    flat = torch.zeros(frames.size + 8, dtype=torch.int16, device=dev).view(torch.uint16)
    data = flat[shift:shift + frames.size].view(frames.shape)
    data.copy_(u16(frames, dev))
    assert data.data_ptr() % 16 == 2 * shift
    return types.SimpleNamespace(data=data, ftype=0, fh=frames.shape[1], fw=frames.shape[2], n=frames.shape[0])


def run(D, dev, names, idx, K, shift=0):
    """isolate_device over batch rows `idx` of the stacked cases `names` with a guarded output store -> numpy (out (K * B, fh, fw), status)"""
    cs = IC.cases()
    store = make_store(np.stack([cs[n]["frame"] for n in names]), dev, shift)
    B, npx = len(idx), store.fh * store.fw
    labels = np.full((B, store.fh, store.fw), 12345, np.int32)          # (a bad frame's labels are never read: its outputs are zero frames)
    roots = np.full((K, B), -1, np.int32)
    for b, i in enumerate(idx):
        if 0 <= i < len(names):
            labels[b], roots[:, b] = cs[names[i]]["labels"], cs[names[i]]["roots"][:K]
    flat = torch.full((2 * GUARD + K * B * npx + 8,), GUARD_WORD, dtype=torch.int16, device=dev).view(torch.uint16)
    out = flat[GUARD + shift:GUARD + shift + K * B * npx].view(K * B, store.fh, store.fw)
    got, status = D.isolate_device(store, np.asarray(idx, np.int64), torch.from_numpy(labels).to(dev), roots=roots, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(status.shape) == (B,) and status.dtype == torch.int32
    host = flat.cpu().numpy()
    assert (host[:GUARD + shift] == GUARD_WORD).all() and (host[GUARD + shift + K * B * npx:] == GUARD_WORD).all(), "awr_hands_isolate wrote outside its output store"
    return host[GUARD + shift:GUARD + shift + K * B * npx].reshape(K * B, store.fh, store.fw), status.cpu().numpy()


@pytest.mark.parametrize("shift", (0, 1), ids=("aligned", "shifted"))
@pytest.mark.parametrize("K", IC.KS)
@pytest.mark.parametrize("shape", list(GROUPS), ids=lambda s: "%dx%d" % s)
def test_every_case(D, dev, shape, K, shift):
    """aligned and fh * fw a multiple of 8: the 8-pixel form; anything else, and every shape one pixel off its alignment: the scalar form"""
    names = GROUPS[shape]
    idx = list(range(len(names)))
    want, want_status = IC.batch_reference(names, idx, K)
    got, status = run(D, dev, names, idx, K, shift)
    assert np.array_equal(status, want_status)
    for r in range(len(want)):
        assert np.array_equal(got[r], want[r]), (names[r % len(names)], "slot %d" % (r // len(names)))


@pytest.mark.parametrize("shift", (0, 1), ids=("aligned", "shifted"))
@pytest.mark.parametrize("K", IC.KS)
def test_mixed_rows(D, dev, K, shift):
    """batches of 1 and more: the same frame twice, bad frame indices in the middle -- zero frames, BAD_FRAME, nothing read -- and every
    row what it is alone"""
    names = GROUPS[(48, 64)]
    n = len(names)
    for idx in ([1], [n], [2, -1, 2], [n - 1, 3, 0, 3, n + 5, 1, 3, -7, 4]):
        want, want_status = IC.batch_reference(names, idx, K)
        got, status = run(D, dev, names, idx, K, shift)
        assert np.array_equal(status, want_status) and np.array_equal(got, want), idx
        bad = np.array([not 0 <= i < n for i in idx])
        assert (status[bad] == D.BAD_FRAME).all() and not got.reshape(K, len(idx), -1)[:, bad].any()


def test_info_rows_are_the_roots(D, dev):
    """info (K, B, 4) as awr_detect_hands writes it, straight into the entry point: awr_detect_hands with labels, then awr_hands_isolate"""
    import hands_cases as HC
    c = HC.cases()["six_candidates"]
    store = make_store(c["frame"][None], dev)
    _, status, info, _, labels = D.hands_device(store, [0], 4, labels=True, **HC.knobs(c))
    out, st = D.isolate_device(store, [0], labels, info=info)
    roots = (info[:, 0, 1] * store.fw + info[:, 0, 0]).cpu().numpy()
    assert status.flatten().tolist() == [0] * 4 and st.tolist() == [0] and len(set(roots.tolist())) == 4
    assert np.array_equal(out.cpu().numpy(), D.isolate(c["frame"], labels[0].cpu().numpy(), roots.astype(np.int32)))
    # two hands and two EMPTY slots: the EMPTY slots get the unchanged frame
    c = HC.cases()["diagonal_blobs"]
    store = make_store(c["frame"][None], dev)
    _, status, info, _, labels = D.hands_device(store, [0], 4, labels=True, **HC.knobs(c))
    out, _ = D.isolate_device(store, [0], labels, info=info)
    assert status.flatten().tolist() == [0, 0, 1, 1] and info[2:, 0].tolist() == [[-1, -1, 0, 0]] * 2
    out = out.cpu().numpy()
    assert np.array_equal(out[2], c["frame"]) and np.array_equal(out[3], c["frame"]) and (out[0] > 0).sum() == 64 == (out[1] > 0).sum()
    assert not ((out[0] > 0) & (out[1] > 0)).any()


def test_argument_errors_come_before_any_launch(D, dev):
    from awr_amd import _lib as L
    store = make_store(np.zeros((1, 48, 64), np.uint16), dev)
    labels = torch.full((1, 48, 64), -1, dtype=torch.int32, device=dev)
    info = lambda K: torch.zeros((K, 1, 4), dtype=torch.int32, device=dev)
    for K, word in ((0, "K = 0"), (5, "K = 5")):
        with pytest.raises(L.AwrError, match=word):
            D.isolate_device(store, [0], labels, info=info(K))
    with pytest.raises(L.AwrError, match="uint16"):
        D.isolate_device(types.SimpleNamespace(data=store.data, ftype=1, fh=48, fw=64), [0], labels, info=info(2))
    out = torch.zeros(8, dtype=torch.int16, device=dev).view(torch.uint16)
    for fh, fw in ((16385, 64), (48, 16385), (0, 64)):
        with pytest.raises(L.AwrError, match="16384"):
            D.isolate_device(types.SimpleNamespace(data=store.data, ftype=0, fh=fh, fw=fw), [0], labels, info=info(2), out=out)
    with pytest.raises(L.AwrError, match="B = 0"):
        D.isolate_device(store, np.zeros(0, np.int64), labels, info=torch.zeros((2, 0, 4), dtype=torch.int32, device=dev), out=out)
    with pytest.raises(ValueError):
        D.isolate_device(store, [0], labels)


# ---- the Predictor on the near-hand composites ---------------------------------------------------------------------------------------------
S, J, NB = 64, 14, 2
FIELDS = ("xyz", "uvd", "center_xyz", "M", "status")


@pytest.fixture(scope="module")
def near(D, dev):
    """the composites, rendered on the device (the frames the CPU test proves the preconditions on), and for each batch of NB composites
    the hands' OWN frames in the row positions of a hands prediction: row k * NB + b is hand k (the nearer one first) of composite b"""
    import awr_amd
    import awr_oracle as O
    from awr_amd import synth as SY
    prims_a, bbox_a, prims_b, bbox_b = IC.near_hands()[:4]
    fa = torch.empty((IC.N_NEAR,) + IC.FULL, dtype=torch.uint16, device=dev)
    fb = torch.empty_like(fa)
    SY.render_device(prims_a, bbox_a, fa)
    SY.render_device(prims_b, bbox_b, fb)
    both = SY.compose(fa, fb)
    host = IC.near_hands_host()
    assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip((fa, fb, both), host))
    a_first = torch.from_numpy(IC.near_first(host[0], host[1])).to(dev)[:, None, None]
    wide = lambda t: t.view(torch.int16)
    first, second = torch.where(a_first, wide(fa), wide(fb)), torch.where(a_first, wide(fb), wide(fa))
    batches = [(both[o:o + NB], torch.cat([first[o:o + NB], second[o:o + NB]]).view(torch.uint16)) for o in range(0, IC.N_NEAR, NB)]
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()

    def make(max_batch=NB, **kw):
        return awr_amd.Predictor(net, S, 1.0, max_batch=max_batch, **kw)
    return types.SimpleNamespace(make=make, batches=batches, both=both)


def hand_major(t):
    """a plain prediction's (2 * NB, ...) rows as the (NB, 2, ...) view a hands prediction has"""
    return t.view((2, NB) + tuple(t.shape[1:])).transpose(0, 1)


def same_hands(got, want, fields):
    return all(getattr(got, f).shape == hand_major(getattr(want, f)).shape and torch.equal(getattr(got, f), hand_major(getattr(want, f)))
               for f in fields)


def anchor(near, fields=FIELDS, **options):
    """Predictor(hands=2, isolate=True, **options) on the composites == a plain Predictor(max_batch=2 NB, **options) on each hand's own frame,
    bit for bit, on EVERY composite; the predictor without isolate differs from it on at least one"""
    iso, raw, plain = near.make(hands=2, isolate=True, **options), near.make(hands=2, **options), near.make(max_batch=2 * NB, **options)
    assert iso.iters > 0 and plain.iters == iso.iters
    differs = 0
    for both, own in near.batches:
        want = plain.predict(own)
        got = iso.predict(both)
        assert want.status.tolist() == [0] * (2 * NB) and not any(torch.isnan(getattr(got, f).float()).any() for f in fields)
        for f in fields:
            g, w = getattr(got, f), hand_major(getattr(want, f))
            assert g.shape == w.shape and torch.equal(g, w), f
        assert iso.isolated.dtype == torch.int32 and iso.isolated.tolist() == [[1, 1]] * NB and got.n_hands.tolist() == [2] * NB
        iso.check()
        differs += not same_hands(raw.predict(both), want, fields)
        assert raw.isolated is None
    assert differs >= 1, "the composites do not bite: the raw-frame predictor equals the own-frame one on every composite"
    return iso, raw


def test_predictor_isolate_equals_a_plain_predictor_on_each_hands_own_frame(near):
    iso, raw = anchor(near)
    B = NB
    assert iso._all_frames.shape[0] == B + 2 * B and iso._store.n == 3 * B and raw._all_frames.shape[0] == B and not hasattr(raw, "_labels")
    # the isolated rows of the store ARE the hands' own frames, hand-major behind the raw frames
    both, own = near.batches[-1]
    assert torch.equal(iso._all_frames[:B].view(torch.int16), both.view(torch.int16))
    assert torch.equal(iso._all_frames[B:].view(torch.int16), own.view(torch.int16))


def test_predictor_isolate_with_recentring_and_confidence(near):
    anchor(near, FIELDS + ("conf", "peak", "spread_mm"), recenter=1, confidence=True)


def test_predictor_isolate_with_palm(near):
    iso, _ = anchor(near, palm=True)
    assert iso.palm_info.shape == (NB, 2, 4)


def test_predictor_isolate_with_identity_and_given_centres(D, near):
    from awr_amd import predictor as P
    both, own = near.batches[0]
    iso = near.make(hands=2, isolate=True)
    want = iso.predict(both)
    pred = near.make(hands=2, isolate=True, identity=True)
    got = pred.predict(both)
    assert type(got) is P.TrackedHandsPrediction
    # a first call: every candidate starts an identity, so every slot is fed by a candidate and crops from that candidate's isolated frame
    source = pred.hand_source
    assert sorted(source[0].tolist()) == [0, 1] and torch.equal(source, got.ids - 1) and pred.isolated.tolist() == [[1, 1]] * NB
    pick = source.to(torch.int64)
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        w = torch.gather(w, 1, pick.view((NB, 2) + (1,) * (w.dim() - 2)).expand_as(w))
        assert torch.equal(g, w), f
    # centres handed in come without labels: raw frames, whatever isolate says -- the bits of the predictor without isolate
    store = types.SimpleNamespace(data=both, ftype=0, fh=IC.FULL[0], fw=IC.FULL[1], n=NB)
    idx = torch.arange(NB, dtype=torch.int64, device=both.device)
    seeds = D.hands_device(store, idx, 2)[0]
    centers, status = D.detect_device(store, idx.repeat(2), seed="given", centers=seeds.view(2 * NB, 3))
    assert status.tolist() == [0] * (2 * NB)
    given = hand_major(centers).contiguous()
    raw = near.make(hands=2)
    for p in (iso, pred):
        out = p.predict(both, centers_uvd=given)
        assert p.isolated.shape == (NB, 2) and p.isolated.tolist() == [[0, 0]] * NB and out.status.shape == (NB, 2)
    a, b = iso.predict(both, centers_uvd=given), raw.predict(both, centers_uvd=given)
    assert a.status.tolist() == [[0, 0]] * NB and all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS)
    # with the tracker a slot that follows its tracked centre reads the raw frame; one fed by a candidate its isolated frame
    trk = near.make(hands=2, isolate=True, identity=True, track=True)
    for _ in range(2):
        out = trk.predict(both)
        assert torch.equal(trk.isolated, ((trk.hand_source >= 0) & (out.status == 0)).to(torch.int32))
    assert trk.isolated.shape == (NB, 2)


def test_predictor_isolate_option_errors(D, near):
    with pytest.raises(ValueError, match="isolate"):
        near.make(max_batch=1, isolate=True)
    with pytest.raises(ValueError, match="isolate"):
        near.make(max_batch=1, isolate=True, views=D.make_views(rot=(10.0,)))
    with pytest.raises(ValueError):
        near.make(max_batch=1, hands=2, isolate=True, views=D.make_views(rot=(10.0,)))
    with pytest.raises(TypeError, match="isolate"):
        near.make(max_batch=1, hands=2, isolate=1)
