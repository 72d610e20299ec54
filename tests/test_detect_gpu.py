"""GPU: awr_detect and awr_detect_samples (csrc/awr_detect.hip) against their numpy statements awr_amd.detect.detect / sample_blocks on the
cases of detect_cases -- frames that start at every offset from a 16-byte boundary, windows clipped at every side and narrower than a group
of 8, eight refinement passes, depth ranges at the edges of depth_bounds, batches past one workgroup of the per-row kernels, and crop-block
centres where the refusal tests flip.  Integer sums and IEEE double divisions: every comparison is bit for bit, NaN positions equal.
tests/test_detect_cases_cpu.py shows what the cases reach and that a kernel wrong in its alignment arithmetic would change them."""
import collections

import numpy as np
import pytest
import torch

import detect_cases as DC
from test_isolate_gpu import make_store
from test_predict_gpu import CUBE, E_PARAS, FLIP, J, S, blob_frames, block_fields, same_bits

pytestmark = pytest.mark.gpu

GUARD = 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


@pytest.fixture(scope="module")
def odd(dev):
    """the eight 41 x 51 frames in one aligned store: frame f starts 3 f mod 8 pixels past a 16-byte boundary"""
    store = make_store(DC.dense_frames(DC.ODD), dev)
    assert [(store.data[f].data_ptr() % 16) // 2 for f in range(DC.N_FRAMES)] == [DC.origin_offset(DC.ODD, f) for f in range(DC.N_FRAMES)]
    return store


def run(D, store, frame, centers=None, cube=None, **kw):
    """detect_device on copies of the shared, read-only case arrays"""
    return D.detect_device(store, np.array(frame, np.int64), centers=None if centers is None else np.array(centers, np.float64),
                           cube=np.array(cube, np.float64), **kw)


def equal(got, want):
    """(centres, status) of the device == the statement's, as bits"""
    return same_bits(got[0].cpu(), torch.from_numpy(np.array(want[0]))) and torch.equal(got[1].cpu(), torch.from_numpy(np.array(want[1])))


# ---- 1. the window sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [None] + list(range(8)), ids=lambda s: "odd" if s is None else "shift%d" % s)
def test_window_sweep(D, dev, odd, shift):
    shape = DC.ODD if shift is None else DC.EVEN
    store = odd if shift is None else make_store(DC.dense_frames(shape), dev, shift)
    frame, centers, cubes = DC.sweep(shape)
    want = DC.sweep_reference(shape)
    assert len(frame) > 256
    rows = collections.Counter(w[3] - w[2] for _, w in DC.sweep_windows(shape)).most_common(1)[0][0]
    assert 8 <= rows <= 20
    for parts in (0, 1, 5, rows, 64, 1024):
        got = run(D, store, frame, seed="given", centers=centers, cube=cubes, paras=DC.PARAS, iters=1, parts=parts)
        bad = [b for b in range(len(frame)) if not same_bits(got[0][b].cpu(), torch.from_numpy(np.array(want[0][b])))]
        assert equal(got, want), (parts, bad[:8], got[0][bad[:8]].cpu(), want[0][bad[:8]])


# ---- 2. whole-frame passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("seed", ["range", "nearest"])
def test_whole_frame_passes_on_odd_frames(D, dev, odd, seed, iters):
    """on a 51-wide frame every row starts at another alignment, and each of the eight frames at another offset"""
    frame = np.arange(DC.N_FRAMES, dtype=np.int64)
    want = DC.reference_rows(DC.dense_frames(DC.ODD), frame, seed, None, DC.WIDE, iters, **DC.MIXED_KW)
    assert (want[1] == DC.OK).all()
    for parts in (0, 3, 41):
        got = run(D, odd, frame, seed=seed, cube=DC.WIDE, paras=DC.PARAS, iters=iters, parts=parts, **DC.MIXED_KW)
        assert equal(got, want), (parts, got[0].cpu(), want[0])


# ---- 3. refinement to the limit -----------------------------------------------------------------------------------------------------------
def test_every_refinement_depth_equals_the_host(D, dev):
    store = make_store(DC.slope_frame()[None], dev)
    ref = DC.slope_reference()
    assert len(ref) == D.MAX_ITERS + 1
    for iters, (c, s) in enumerate(ref):
        got = run(D, store, [0], seed="given", centers=[DC.SLOPE_START], cube=DC.SLOPE_CUBE, paras=DC.PARAS, iters=iters)
        assert equal(got, ([c], np.array([s], np.int32))), (iters, got[0].cpu(), c)


def test_eight_passes_stay_inside_scratch_and_outputs(D, dev, odd):
    """awr_detect itself, B = 300 and iters = 8: all ten slots of every row are in use, and the words around the scratch, the centres and the
    status survive"""
    from awr_amd import _lib as L
    B, iters = 300, D.MAX_ITERS
    frame, centers, cubes = (a[:B] for a in DC.sweep(DC.ODD))
    want = tuple(a[:B] for a in DC.sweep_reference(DC.ODD, iters))
    nbytes = int(L.lib.awr_detect_scratch(B))
    assert nbytes == B * (D.MAX_ITERS + 2) * 4 * 8
    word, mark = 0x5A5A5A5A5A5A5A5A, -7.0
    scratch = torch.full((GUARD + nbytes // 8 + GUARD,), word, dtype=torch.int64, device=dev)
    out = torch.full((GUARD + 3 * B + GUARD,), mark, dtype=torch.float64, device=dev)
    status = torch.full((GUARD + B + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    t = [torch.from_numpy(np.array(a)).to(dev) for a in (frame, centers, cubes)]
    L.call("awr_detect", odd.data.data_ptr(), odd.ftype, DC.N_FRAMES, odd.fh, odd.fw, t[0].data_ptr(), B, D.SEED_GIVEN, t[1].data_ptr(), 1.0, 2000.0, 150.0,
           t[2].data_ptr(), 3, DC.PARAS[0], DC.PARAS[1], iters, 0, scratch[GUARD:].data_ptr(), out[GUARD:].data_ptr(), status[GUARD:].data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert (scratch[:GUARD] == word).all() and (scratch[GUARD + nbytes // 8:] == word).all(), "awr_detect wrote outside awr_detect_scratch(B) bytes"
    assert (out[:GUARD] == mark).all() and (out[GUARD + 3 * B:] == mark).all() and (status[:GUARD] == 0x5A5A5A5A).all() and (status[GUARD + B:] == 0x5A5A5A5A).all()
    assert equal((out[GUARD:GUARD + 3 * B].view(B, 3), status[GUARD:GUARD + B]), want)
    # every refinement slot of a row that found pixels holds its count: slots 2 ... 9 were written
    slots = scratch[GUARD:GUARD + nbytes // 8].view(B, D.MAX_ITERS + 2, 4).cpu()
    ok = torch.from_numpy(want[1] == DC.OK)
    assert ok.sum() > 250 and (slots[ok][:, 2:, 0] > 0).all() and (slots[:, 1] == 0).all()


# ---- 4. depth bounds ----------------------------------------------------------------------------------------------------------------------
def test_depth_bounds(D, dev):
    store = make_store(DC.depth_frame()[None], dev)
    frame = np.zeros(len(DC.DEPTH_CUBES), np.int64)
    for seed, rng, slab in DC.depth_cases():
        for iters in (0, 2):
            want = DC.depth_reference(seed, rng, slab, iters)
            got = run(D, store, frame, seed=seed, cube=np.array(DC.DEPTH_CUBES), paras=DC.PARAS, depth_range=rng, slab=slab, iters=iters)
            assert equal(got, want), (seed, rng, slab, iters, got[0].cpu(), got[1].cpu(), want)
            if rng == (0.25, 0.75):
                assert got[1].tolist() == [DC.EMPTY] * len(frame) and torch.isnan(got[0]).all()


# ---- 5. a large mixed batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ["nearest", "range"])
def test_large_mixed_batch(D, dev, odd, seed):
    frame, cubes = DC.mixed_batch()
    want = DC.mixed_reference(seed, 2)
    assert len(frame) >= 300
    got = run(D, odd, frame, seed=seed, cube=cubes, paras=DC.PARAS, iters=2, **DC.MIXED_KW)
    assert equal(got, want)
    bad = torch.from_numpy((frame < 0) | (frame >= DC.N_FRAMES))
    assert bad[:256].any() and bad[256:].any() and (got[1].cpu()[bad] == DC.BAD_FRAME).all() and torch.isnan(got[0].cpu()[bad]).all()
    # each row is what it is alone
    for b in (0, 5, 255, 256, 257, 319):
        one = run(D, odd, frame[b:b + 1], seed=seed, cube=cubes[b:b + 1], paras=DC.PARAS, iters=2, **DC.MIXED_KW)
        assert same_bits(one[0].cpu(), got[0][b:b + 1].cpu()) and one[1].tolist() == got[1][b:b + 1].tolist(), b


# ---- 6. crop blocks -----------------------------------------------------------------------------------------------------------------------
def test_crop_blocks_at_the_refusal_boundaries(D, dev):
    from awr_amd import _lib as L
    centers, cubes, frame, status_in, _ = DC.sample_rows()
    h_blocks, h_M, h_cxyz, h_cube, h_status = DC.sample_reference()
    B = len(centers)
    assert B > 256
    status = torch.from_numpy(status_in.copy()).to(dev)
    blocks, M, cxyz, cube32, st = D.samples_device(torch.from_numpy(centers.copy()).to(dev), np.array(cubes), DC.DSIZE, np.array(frame), DC.N_FRAMES, DC.ODD, DC.PARAS, DC.FLIP,
                                                   status=status)
    assert st.data_ptr() == status.data_ptr() and st.cpu().tolist() == h_status.tolist()
    raw = blocks.cpu().numpy()
    for b in range(B):
        blk = L.NyuSample.from_buffer_copy(bytes(raw[b]))
        if h_blocks[b] is None:
            # a refused row reads no pixel
            assert (blk.frame, blk.rw, blk.rh, blk.cw, blk.ch) == (0, 0, 0, 0, 0) and torch.isnan(M[b]).all(), (b, centers[b])
        else:
            got, want = block_fields(L, blk), block_fields(L, h_blocks[b])
            assert got == want, (b, centers[b], {k: (got[k], want[k]) for k in got if got[k] != want[k]})
    assert same_bits(M.cpu(), torch.from_numpy(h_M)) and same_bits(cxyz.cpu(), torch.from_numpy(h_cxyz)) and same_bits(cube32.cpu(), torch.from_numpy(h_cube))
    keep = torch.from_numpy((status_in != 0) & (frame >= 0) & (frame < DC.N_FRAMES))
    assert keep.sum() >= 8 and torch.equal(st.cpu()[keep], torch.from_numpy(status_in.copy())[keep])


# ---- 7. rendered crops --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 3])
def test_rendered_crops_over_the_edges_of_a_shifted_store(D, dev, shift):
    import awr_amd.nyu_data as ND
    import awr_amd.nyu_device as DV
    frames = DC.dense_frames(DC.ODD)
    store = make_store(frames, dev, shift)
    cs, frame = DC.render_rows()
    cube = (300.0, 300.0, 300.0)
    blocks, _, _, _, st = D.samples_device(torch.from_numpy(cs).to(dev), cube, DC.DSIZE, frame, DC.N_FRAMES, DC.ODD, DC.PARAS, DC.FLIP)
    h_status = D.sample_blocks(cs, cube, DC.DSIZE, DC.PARAS, DC.FLIP, DC.ODD, frames=frame)[4]
    assert st.tolist() == h_status.tolist() and (h_status == DC.OK).sum() >= 9 and (h_status == DC.BAD_WINDOW).sum() == 2
    img = DV.Renderer(store, DC.DSIZE, len(cs))(blocks).cpu()
    for b in range(len(cs)):
        if h_status[b] != DC.OK:
            assert torch.equal(img[b, 0], torch.ones(DC.DSIZE, DC.DSIZE)), b          # the constant background, nothing read
            continue
        crop, _ = ND.crop(frames[frame[b]].astype(np.float32), cs[b], np.array(cube), (DC.DSIZE, DC.DSIZE), DC.PARAS)
        want = ND.normalize(crop.max(), crop, cs[b], np.array(cube)).astype(np.float32)
        assert torch.equal(img[b, 0], torch.from_numpy(want)), (b, cs[b])


# ---- 8. the Predictor on odd frames -------------------------------------------------------------------------------------------------------
def test_predictor_on_odd_frames_equals_the_hand_assembled_pipeline(D, dev):
    """121 x 161: frame 1 of the Predictor's store starts one pixel past a 16-byte boundary.  The detector's seed and two refinement passes,
    the blocks, the render, the network and the un-projection, assembled by hand from the host's centres and blocks"""
    import awr_amd
    import awr_amd.nyu_device as DV
    import awr_oracle as O
    from awr_amd.trainer import InferEngine
    shape = (121, 161)
    frames = np.pad(blob_frames()[0], ((0, 0), (0, 1), (0, 1)), constant_values=1400)
    assert frames.shape == (2,) + shape and frames.dtype == np.uint16
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()
    kw = dict(depth_range=(200.0, 1200.0), slab=100.0)
    pred = awr_amd.Predictor(net, S, 1.0, cube=CUBE, paras=E_PARAS, flip=FLIP, max_batch=2, frame_shape=shape, seed="nearest", refine_iters=2, **kw)
    out = pred.predict(frames)
    pred.check()
    assert out.status.tolist() == [0, 0] and (pred._frames.data_ptr() + 2 * shape[0] * shape[1]) % 16 == 2
    host = [D.detect(f, seed="nearest", cube=CUBE, paras=E_PARAS, iters=2, **kw) for f in frames]
    assert [s for _, s in host] == [0, 0]
    centers = np.array([c for c, _ in host])
    blocks, M, cxyz, cube, st = D.sample_blocks(centers, CUBE, S, E_PARAS, FLIP, shape)
    assert st.tolist() == [0, 0]
    store = make_store(frames, dev)
    img = DV.Renderer(store, S, 2)(DV.blocks_to_tensor(blocks))
    jt = InferEngine(net, 2, S, 1.0)(img)
    uvd, xyz, ust = D.unproject_device(jt, torch.from_numpy(cxyz).to(dev), torch.from_numpy(M).to(dev), torch.from_numpy(cube).to(dev), S, E_PARAS, FLIP)
    assert ust.tolist() == [0, 0] and not torch.isnan(uvd).any()
    assert torch.equal(out.uvd, uvd) and torch.equal(out.xyz, xyz)
    assert torch.equal(out.M.cpu(), torch.from_numpy(M)) and torch.equal(out.center_xyz.cpu(), torch.from_numpy(cxyz))
    # the detector alone, on the same frames in a store of its own
    got = run(D, store, [0, 1], seed="nearest", cube=CUBE, paras=E_PARAS, iters=2, **kw)
    assert equal(got, (centers, np.zeros(2, np.int32)))
