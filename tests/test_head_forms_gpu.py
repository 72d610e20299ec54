"""GPU: every form of the head kernels (csrc/awr_head.hip) at every sampling ratio, map size and joint-slot width of tests/head_cases.py --
the NHWC entry points the engines run (forward, loss step with and without the coordinate loss, eval, confidence), the NCHW kernels of
FeatureModule, one layout against the other, the "peaked" inputs, and the tuning-hook instantiations in a child process.

Reference: the fp32 oracle (oracle/awr_oracle.py).  Bars: tests/test_head_gpu.py's -- joints 3e-6, gradient 3e-6 max|g| + 1e-9, losses
2e-6 relative, GT map bit for bit, awr_dense_loss gradient 1e-6 max|g|.  A case that misses a fixed bar may be judged instead by its distance to
float64 against the fp32 oracle's own (factor 3, test_gradients_elementwise_against_the_fp64_yardstick's) -- only if it is listed in
F64_JUDGED with the figures in DESIGN.md 4.18.1.  Every output and scratch buffer is NaN before the call."""
import json
import os
import subprocess
import sys

import pytest
import torch

import awr_oracle as O
import confidence_ref as R
import head_cases as HC
from head_env_worker import NAN, NhwcRun

pytestmark = pytest.mark.gpu

FACTOR = 4.0                # tests/test_head_confidence_gpu.py's
PEAKED_FACTOR = 1.5         # 1.5 x the worst measured ratio (0.99), rounded up
# (what, case id, ks): judged by the float64 ratio; DESIGN.md 4.18.1 holds both distances of each
F64_JUDGED = {("gradient cw=1", "3x33x8x32x160", 0.4)}
NOT_RS2 = [c for c in HC.NHWC_CASES if c[3] // c[2] != 2]
NCHW_NOT_RS2 = [c for c in HC.NCHW_CASES if c[3] // c[2] != 2]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    import awr_amd  # noqa: F401
    from awr_amd import _lib
    return _lib


@pytest.fixture
def deterministic():
    import awr_amd
    was = awr_amd.get_deterministic()
    awr_amd.set_deterministic(True)
    yield
    awr_amd.set_deterministic(was)


def judge(what, case, ks, got, ref, bar_fn, ref64):
    """`got` against the fp32 oracle on the fixed bar; a case listed in F64_JUDGED: device distance to float64 <= 3 x the oracle's"""
    got = got.detach().cpu()
    d, bar = bar_fn(got, ref)
    print("\n%s %s ks %.1f: %.3e (bar %.3e)" % (what, HC.case_id(case), ks, d, bar))
    assert not bool(torch.isnan(got).any()), "%s: %d NaN left" % (what, int(torch.isnan(got).sum()))
    if d <= bar:
        return
    r64 = ref64()
    g_dev, g_host = float((got.double() - r64).abs().max()), float((ref.double() - r64).abs().max())
    print("  to float64: device %.3e, fp32 oracle %.3e, ratio %.2f" % (g_dev, g_host, g_dev / g_host))
    assert (what, HC.case_id(case), ks) in F64_JUDGED, (what, d, bar, g_dev, g_host)
    assert g_dev <= 3.0 * g_host, (what, g_dev, g_host)


def losses_close(got, cw, ref):
    assert HC.loss_ok(got[0], cw * ref["lc"], 1e-3), ("coord", got[0], cw * ref["lc"])
    assert HC.loss_ok(got[1], ref["ld"]), ("dense", got[1], ref["ld"])


# ---- NHWC ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", HC.NHWC_CASES, ids=HC.case_id)
def test_nhwc_forward(L, dev, case, ks):
    run = NhwcRun(L, dev, case, ks).forward()
    judge("joints", case, ks, run.jt, HC.loss_refs(*case[:4], ks, 0.0)["jt"], HC.joint_bar, lambda: HC.loss_refs64(*case[:4], ks, 0.0)["jt"])
    assert bool(torch.isfinite(run.stat).all())
    assert run.partials_written()           # B * chunks * J * 5 partials, all of them; the rest of the documented size is never touched
    assert bool(torch.isnan(run.g_jt).all()) and bool(torch.isnan(run.grad).all())       # not this entry's


@pytest.mark.parametrize("cw", [0.0, 1.0])
@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", HC.NHWC_CASES, ids=HC.case_id)
def test_nhwc_loss_step(L, dev, case, ks, cw):
    """cw == 0: one MODE 1|2 launch; cw == 1: MODE 1, head_finish_kernel, MODE 2|4.  Joints, both losses and the whole gradient against
    the oracle's autograd."""
    B, J, F, H, cp = case
    run, ref = NhwcRun(L, dev, case, ks).loss_step(cw), HC.loss_refs(B, J, F, H, ks, cw)
    judge("joints", case, ks, run.jt, ref["jt"], HC.joint_bar, lambda: HC.loss_refs64(B, J, F, H, ks, cw)["jt"])
    losses_close(run.losses(), cw, ref)
    g = run.grad.cpu()
    judge("gradient cw=%g" % cw, case, ks, g, HC.to_nhwc(ref["grad"], cp), HC.grad_bar, lambda: HC.to_nhwc(HC.loss_refs64(B, J, F, H, ks, cw)["grad"], cp))
    assert bool((g[:, :, 4 * J:] == 0).all()), "padding channels of the gradient must be zero"
    assert bool(torch.isfinite(run.stat).all()) and run.partials_written()
    # g_jt: written in full by head_finish_kernel when there is a coordinate loss, never touched otherwise
    assert bool(torch.isfinite(run.g_jt).all()) if cw else bool(torch.isnan(run.g_jt).all())


@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", HC.NHWC_CASES, ids=HC.case_id)
def test_nhwc_eval(L, dev, case, ks):
    """MODE 1|8: bitwise the forward entry's joints and statistics, the training entry's losses"""
    fwd = NhwcRun(L, dev, case, ks).forward()
    ev = NhwcRun(L, dev, case, ks).eval(1.0)
    assert torch.equal(ev.jt, fwd.jt) and torch.equal(ev.stat, fwd.stat) and not bool(torch.isnan(ev.jt).any()) and ev.partials_written()
    assert bool(torch.isnan(ev.grad).all()) and bool(torch.isnan(ev.g_jt).all())         # value only: no gradient buffer is touched
    tr, le = NhwcRun(L, dev, case, ks).loss_step(1.0).losses(), ev.losses()
    print("\neval %s / train %s" % (le, tr))
    assert HC.loss_ok(le[0], tr[0], 1e-3) and HC.loss_ok(le[1], tr[1])
    losses_close(le, 1.0, HC.loss_refs(*case[:4], ks, 1.0))


def conf_check(name, case, ks, got, jt):
    c = HC.inputs(*case[:4])
    ref = R.confidence(c["off"], c["img"], ks, jt=jt.cpu())
    host = R.confidence(c["off"], c["img"], ks, jt=jt.cpu(), dtype=torch.float32)
    g_dev, g_host = (got.cpu().double() - ref).abs().amax((0, 1)), (host.double() - ref).abs().amax((0, 1))
    print("\n%s %s ks %.1f [conf, var_u, var_v, var_d]: device gap %s  float32 host gap %s  ratio %s" % (
        name, HC.case_id(case), ks, ["%.2e" % v for v in g_dev.tolist()], ["%.2e" % v for v in g_host.tolist()],
        ["%.2f" % (a / b) for a, b in zip(g_dev.tolist(), g_host.tolist())]))
    assert bool(torch.isfinite(got).all()) and float(got[..., 1:].min()) >= 0.0
    assert bool((g_dev <= FACTOR * g_host).all()), (g_dev.tolist(), g_host.tolist())


@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", NOT_RS2, ids=HC.case_id)
def test_nhwc_confidence_at_the_other_sampling_ratios(L, dev, case, ks):
    """conf_nhwc_kernel's depth sampling at rs != 2: the criterion of tests/test_head_confidence_gpu.py"""
    B, J, F, H, cp = case
    run = NhwcRun(L, dev, case, ks).forward()
    out = torch.full((B, J, 4), NAN, device=dev)
    run.scratch.fill_(NAN)
    L.call("awr_head_confidence_nhwc", L.ptr(run.pred), cp, L.ptr(run.img), L.ptr(run.jt), L.ptr(run.stat), B, J, F, H, ks, L.ptr(run.scratch), L.ptr(out),
           L.stream())
    conf_check("nhwc", case, ks, out, run.jt)
    n = B * run.la["chunks"] * J * 4          # four sums per (image, chunk, joint)
    assert not bool(torch.isnan(run.scratch[:n]).any()) and bool(torch.isnan(run.scratch[n:]).all())


@pytest.mark.parametrize("case", [(256, 14, 24, 48, 64), (3, 40, 24, 24, 160)], ids=HC.case_id)
def test_deterministic_mode_gives_the_same_bits(L, dev, deterministic, case):
    """the ragged case and a JS = 64 case: two loss-step launches, identical bits in acc, jt and grad"""
    a, b = NhwcRun(L, dev, case, 0.4).loss_step(1.0), NhwcRun(L, dev, case, 0.4).loss_step(1.0)
    assert torch.equal(a.acc.view(torch.int64), b.acc.view(torch.int64)) and bool((a.acc.view(torch.int64) != 0).all())
    assert torch.equal(a.jt, b.jt) and torch.equal(a.grad, b.grad) and not bool(torch.isnan(a.grad).any())
    losses_close(a.losses(), 1.0, HC.loss_refs(*case[:4], 0.4, 1.0))


# ---- NCHW ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", HC.NCHW_CASES, ids=HC.case_id)
def test_nchw_joint2offset_bit_exact(dev, case, ks):
    import awr_amd
    B, J, F, H = case
    c = HC.inputs(*case)
    out = awr_amd.FeatureModule().joint2offset(c["jt_gt"].to(dev), c["img"].to(dev), ks, F).cpu()
    ieee = torch.from_numpy(O.joint2offset_ieee(c["jt_gt"], c["img"], ks, F))
    assert torch.equal(out, ieee), "max diff %g, %d elements differ from the IEEE restatement" % (float((out - ieee).abs().max()), int((out != ieee).sum()))


@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", HC.NCHW_CASES, ids=HC.case_id)
def test_nchw_head_forward_backward_and_accumulate(L, dev, case, ks):
    import awr_amd
    B, J, F, H = case
    c = HC.inputs(*case)
    jt_ref, g_ref = HC.head_refs(B, J, F, H, ks)
    x, img = c["off"].to(dev).requires_grad_(True), c["img"].to(dev)
    jt = awr_amd.FeatureModule().offset2joint_softmax(x, img, ks)
    judge("joints", case, ks, jt, jt_ref, HC.joint_bar, lambda: HC.head_refs(B, J, F, H, ks, True)[0])
    (jt * c["g_jt"].to(dev)).sum().backward()
    judge("head gradient", case, ks, x.grad, g_ref, HC.grad_bar, lambda: HC.head_refs(B, J, F, H, ks, True)[1])
    # the entry points on NaN-prefilled buffers: the same bits; accumulate = 1 adds them onto a known gradient with ONE fp32 addition
    off, g_jt = x.detach(), c["g_jt"].to(dev)
    jt2, stat = torch.full((B, J, 3), NAN, device=dev), torch.full((B, J, 2), NAN, device=dev)
    L.call("awr_head_forward", L.ptr(off), L.ptr(img), B, J, F, H, ks, L.ptr(jt2), L.ptr(stat), L.stream())
    assert torch.equal(jt2, jt.detach()) and bool(torch.isfinite(stat).all())
    plain = torch.full_like(off, NAN)
    L.call("awr_head_backward", L.ptr(off), L.ptr(img), L.ptr(jt2), L.ptr(stat), L.ptr(g_jt), B, J, F, H, ks, L.ptr(plain), 0, L.stream())
    assert torch.equal(plain, x.grad)
    known = HC._hashed(tuple(off.shape), 17, float(g_ref.abs().max())).to(dev)
    summed = known.clone()
    L.call("awr_head_backward", L.ptr(off), L.ptr(img), L.ptr(jt2), L.ptr(stat), L.ptr(g_jt), B, J, F, H, ks, L.ptr(summed), 1, L.stream())
    assert torch.equal(summed, known + plain)


@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", HC.NCHW_CASES, ids=HC.case_id)
def test_nchw_dense_loss_three_forms(L, dev, case, ks):
    """awr_dense_loss with a gradient, with accumulate = 1 and with a null gradient pointer (value only).  Reference: the oracle's Huber on
    the IEEE restatement of the GT map (HC.dense_refs says why); the loss also against the torch oracle's map."""
    B, J, F, H = case
    c, w = HC.inputs(*case), 0.7
    ref = HC.dense_refs(B, J, F, H, ks, w)
    assert HC.loss_ok(ref["loss"], w * HC.loss_refs(B, J, F, H, ks, 0.0)["ld"], 1e-3)
    off, img, jg = c["off"].to(dev), c["img"].to(dev), c["jt_gt"].to(dev)

    def run(g, accumulate):
        acc, out = torch.zeros(2, device=dev, dtype=torch.float64), torch.zeros(3, device=dev)
        L.call("awr_dense_loss", L.ptr(off), L.ptr(jg), L.ptr(img), B, J, F, H, ks, HC.DELTA, w, L.ptr(acc), L.ptr(g), accumulate, L.stream())
        L.call("awr_loss_finalize", L.ptr(acc), 2, L.ptr(out), L.stream())
        return out.tolist()
    plain = torch.full_like(off, NAN)
    l = run(plain, 0)
    assert HC.loss_ok(l[0], ref["loss"], 1e-3) and l[1] == 0.0 and l[2] == l[0], (l, ref["loss"])
    gmax = float(ref["grad"].abs().max())
    d = float((plain.cpu() - ref["grad"]).abs().max())
    print("\ndense-loss gradient %s ks %.1f: %.3e (bar %.3e)" % (HC.case_id(case), ks, d, 1e-6 * gmax))
    assert d <= 1e-12 + 1e-6 * gmax and not bool(torch.isnan(plain).any())
    known = HC._hashed(tuple(off.shape), 18, gmax).to(dev)
    summed = known.clone()
    l1 = run(summed, 1)
    assert torch.equal(summed, known + plain) and HC.loss_ok(l1[0], ref["loss"], 1e-3)
    l2 = run(None, 0)
    assert HC.loss_ok(l2[0], ref["loss"], 1e-3)


@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", NCHW_NOT_RS2, ids=HC.case_id)
def test_nchw_confidence_at_the_other_sampling_ratios(L, dev, case, ks):
    B, J, F, H = case
    c = HC.inputs(*case)
    off, img = c["off"].to(dev), c["img"].to(dev)
    jt, stat, out = torch.full((B, J, 3), NAN, device=dev), torch.full((B, J, 2), NAN, device=dev), torch.full((B, J, 4), NAN, device=dev)
    L.call("awr_head_forward", L.ptr(off), L.ptr(img), B, J, F, H, ks, L.ptr(jt), L.ptr(stat), L.stream())
    L.call("awr_head_confidence", L.ptr(off), L.ptr(img), L.ptr(jt), L.ptr(stat), B, J, F, H, ks, L.ptr(out), L.stream())
    conf_check("nchw", case, ks, out, jt)


# ---- one layout against the other ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", HC.KSS)
@pytest.mark.parametrize("case", HC.NHWC_CASES, ids=HC.case_id)
def test_nhwc_against_nchw(L, dev, case, ks):
    """Joints and the head gradient of the two layouts, on the bars both hold against the oracle.  dense_weight = 0 leaves the head's
    backward alone in the NHWC gradient; the NCHW backward gets the upstream gradient head_finish_kernel wrote."""
    B, J, F, H, cp = case
    assert J <= 56
    run = NhwcRun(L, dev, case, ks).loss_step(1.0, 0.0)
    off = HC.inputs(B, J, F, H)["off"].to(dev)
    jt, stat, g = torch.full((B, J, 3), NAN, device=dev), torch.full((B, J, 2), NAN, device=dev), torch.full_like(off, NAN)
    L.call("awr_head_forward", L.ptr(off), L.ptr(run.img), B, J, F, H, ks, L.ptr(jt), L.ptr(stat), L.stream())
    L.call("awr_head_backward", L.ptr(off), L.ptr(run.img), L.ptr(jt), L.ptr(stat), L.ptr(run.g_jt), B, J, F, H, ks, L.ptr(g), 0, L.stream())
    dj, jbar = HC.joint_bar(run.jt.cpu(), jt.cpu())
    dg, gbar = HC.grad_bar(run.grad.cpu(), HC.to_nhwc(g.cpu(), cp))
    print("\nnhwc - nchw %s ks %.1f: joints %.3e (bar %.1e), head gradient %.3e (bar %.3e)" % (HC.case_id(case), ks, dj, jbar, dg, gbar))
    assert dj <= jbar and dg <= gbar and not bool(torch.isnan(run.grad).any()) and not bool(torch.isnan(g).any())


# ---- peaked inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HC.PEAKED_CASES, ids=HC.case_id)
def test_peaked_inputs_against_float64(L, dev, case):
    """Heat channels x 5 (logits up to +-90): the fp32 oracle itself is up to 4e-6 from float64, so no fixed bar applies.  Reference: the
    float64 evaluation; yardstick: the same formulas in float32 on the host (the oracle).  Measured ratios: DESIGN.md 4.18.1."""
    B, J, F, H, cp = case
    run = NhwcRun(L, dev, case, 0.4, peaked=True).loss_step(1.0)
    r32, r64 = HC.loss_refs(B, J, F, H, 0.4, 1.0, 1.0, True), HC.loss_refs64(B, J, F, H, 0.4, 1.0, 1.0, True)
    worst = 0.0
    for what, got, a, b in (("joints", run.jt.cpu(), r32["jt"], r64["jt"]),
                            ("gradient", run.grad.cpu()[:, :, :4 * J], HC.to_nhwc(r32["grad"], 4 * J), HC.to_nhwc(r64["grad"], 4 * J))):
        assert not bool(torch.isnan(got).any())
        g_dev, g_host = float((got.double() - b).abs().max()), float((a.double() - b).abs().max())
        print("\npeaked %s %s: device gap %.3e  host float32 gap %.3e  ratio %.2f  (largest value %.3e)" % (
            HC.case_id(case), what, g_dev, g_host, g_dev / g_host, float(b.abs().max())))
        worst = max(worst, g_dev / g_host)
    assert worst <= PEAKED_FACTOR, worst


# ---- the tuning-hook instantiations ----------------------------------------------------------------------------------------------------
def test_tuning_hook_instantiations():
    """AWR_NHWC_DEPTH=2 AWR_NHWC_WGS=1 in a fresh child (both are read once per process): dense_nhwc_kernel<16, 1 / 1|2 / 2|4, DEPTH 2> walking
    8 + 1, 16 + 9 and 4 tiles per image; the child compares with the oracle and prints its figures."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "head_env_worker.py")
    p = subprocess.run([sys.executable, worker], env=dict(os.environ, AWR_NHWC_DEPTH="2", AWR_NHWC_WGS="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:]          # (nothing is started after a child that failed)
    res = json.loads(p.stdout.strip().splitlines()[-1])["results"]
    assert len(res) == len(HC.ENV_CASES) * len(HC.KSS) * 3
    assert {(r["tiles_per_wg"], r["chunks"], r["last_tiles"]) for r in res} == {(8, 2, 1), (16, 2, 9), (4, 1, 4)}
    for r in res:
        print(r)
        assert r["jt"] <= r["jt_bar"] and r["partials_written"] and r["stat_finite"], r
        if r["form"] != "forward":
            assert r["grad"] <= r["grad_bar"] and r["grad_nans"] == 0 and r["padding_zero"] and r["losses_ok"], r
