"""The shapes, launch arithmetic, inputs and references the operator tests of the head kernels share (csrc/awr_head.hip: the joint decoder,
the GT map, both Huber losses and the gradient the backward starts from, in the NHWC forms the engines run and in the NCHW forms of
FeatureModule; tests/test_head_cases_cpu.py, tests/test_head_forms_gpu.py, tests/head_env_worker.py).

nhwc_launch() restates ONLY the arithmetic of nhwc_geometry / launch_dense_nhwc, so the CPU test can say which launch class each shape of
NHWC_CASES is in.  The references are the fp32 oracle (oracle/awr_oracle.py) and the same formulas in float64 (O.HIGH_PRECISION,
tests/confidence_ref.py); nothing here calls the library."""
import functools

import numpy as np
import torch

import awr_oracle as O
import confidence_ref as R

TPX = 64                    # pixels per tile of dense_nhwc_kernel / conf_nhwc_kernel
WANT_WGS = 1024             # workgroups per launch nhwc_geometry aims for (the default of the AWR_NHWC_WGS hook)
DELTA = 0.01
KSS = [0.4, 1.0]

# (B, J, F, H, Cp): what each is in the table for -- the classes tests/test_head_cases_cpu.py asserts from nhwc_launch().  Three images each:
# one all background, one all foreground, one mixed (inputs()).
NHWC_CASES = [
    (3, 1, 8, 8, 32),           # J == 1: 15 of 16 joint lanes idle; one tile per image; rs 1
    (3, 14, 8, 64, 64),         # rs 8
    (3, 16, 16, 64, 64),        # J == JS (no idle lane), Cp == 4J, rs 4, four chunks
    (3, 5, 8, 16, 64),          # Cp wider than the minimum (32)
    (3, 14, 24, 24, 64),        # JS 16, general F, rs 1
    (3, 14, 40, 160, 64),       # general F, rs 4, 25 chunks
    (3, 17, 24, 96, 96),        # one above the JS 16 boundary: JS 32, general F
    (3, 21, 16, 32, 128),       # JS 32, power-of-two F, Cp wider than the minimum (96)
    (3, 32, 8, 8, 128),         # J == JS == 32
    (3, 33, 8, 32, 160),        # one above the JS 32 boundary: JS 64, power-of-two F
    (3, 40, 24, 24, 160),       # JS 64, general F, Cp == 4J
    (3, 56, 24, 48, 224),       # the widest map: 58 624 B of LDS
    (256, 14, 24, 48, 64),      # 9 tiles, 2 per workgroup, 5 chunks, the last one ragged
    (3, 14, 128, 128, 64),      # the production shape of downsample = 1: 256 chunks, the strided loop of head_finish_kernel
    (3, 14, 32, 128, 64),       # the production shape of downsample = 4
]
# (B, J, F, H)
NCHW_CASES = [
    (3, 14, 4, 16),             # P = 16: 4 working threads, three idle waves; rs 4
    (3, 14, 12, 12),            # P = 144, rs 1
    (3, 60, 8, 16),             # more joints than the NHWC form takes
    (3, 21, 24, 96),            # P = 576, rs 4
    (3, 14, 40, 40),            # P = 1600: one full trip of 1024 pixels and a partial one
    (3, 14, 16, 128),           # rs 8
    (3, 14, 128, 128),          # P = 16384, rs 1
    (3, 14, 32, 128),           # rs 4
]
# one per JS: the "peaked" variant (heat channels x 5: logits up to +-90)
PEAKED_CASES = [(3, 16, 16, 64, 64), (3, 21, 16, 32, 128), (3, 40, 24, 24, 160)]
# the tuning-hook instantiations (AWR_NHWC_DEPTH=2 AWR_NHWC_WGS=1: tests/head_env_worker.py)
ENV_CASES = [
    (3, 14, 24, 48, 64),        # 9 tiles = 8 + 1: the ntile < DEPTH guard
    (3, 14, 40, 80, 64),        # 25 tiles = 16 + 9: an odd tile count under depth 2
    (3, 14, 16, 32, 64),        # 4 tiles, one chunk
]


def case_id(case):
    return "x".join(str(v) for v in case)


def _cdiv(a, b):
    return -(-a // b)


def padded_channels(J):
    return (4 * J + 31) // 32 * 32


def scratch_floats(B, J, F):
    """awr_head_nhwc_scratch: the documented size of the partials buffer, in floats"""
    return B * (F * F // TPX + 1) * J * 5


def nhwc_launch(B, J, F, H, Cp, want_wgs=WANT_WGS):
    """What an NHWC entry point starts for (B, J, F, H, Cp): the checks of check_head_dims / nhwc_geometry (asserted), the joint-slot width JS
    and the POW2 form launch_dense_nhwc picks, the depth sampling ratio, the tiles of one image, how many of them a workgroup walks, the
    chunks (= gridDim.x) and whether the last chunk is shorter, the float4 loads per thread and tile, the lanes without a joint, the LDS."""
    assert B > 0 and J > 0 and F > 0 and H > 0 and F % 4 == 0 and H % F == 0 and (H // F != 2 or H % 8 == 0)
    assert J <= 64 and Cp >= 4 * J and Cp % 32 == 0 and Cp <= 224
    JS = 16 if J <= 16 else 32 if J <= 32 else 64
    assert Cp <= 4 * JS
    P = F * F
    assert P % TPX == 0
    tiles = P // TPX
    per = 1
    while per < 16 and per * 2 <= tiles and B * (tiles // (per * 2)) >= want_wgs:
        per *= 2
    chunks = _cdiv(tiles, per)
    return {"JS": JS, "POW2": F & (F - 1) == 0, "rs": H // F, "tiles": tiles, "tiles_per_wg": per, "chunks": chunks, "ragged": tiles % per != 0,
            "last_tiles": tiles - (chunks - 1) * per, "NL": Cp // 16, "NLMAX": JS // 4, "idle_lanes": (JS - J) * (256 // JS),
            "lds_bytes": (TPX * (Cp + 4) + TPX) * 4, "partials": B * chunks * J * 5}


def launch_classes(B, J, F, H, Cp):
    """The names of the launch classes an NHWC case is in (tests/test_head_cases_cpu.py requires NHWC_CASES to cover ALL_CLASSES)"""
    la = nhwc_launch(B, J, F, H, Cp)
    cls = {"JS %d, %s F" % (la["JS"], "power-of-two" if la["POW2"] else "general"), "rs %d" % la["rs"]}
    cls.add("one tile" if la["tiles"] == 1 else "several chunks" if la["chunks"] > 1 else "one chunk of several tiles")
    if la["chunks"] > 32:
        cls.add("more than 32 chunks")
    if la["tiles_per_wg"] > 1 and la["ragged"]:
        cls.add("ragged last chunk")
    if J == la["JS"]:
        cls.add("J == JS")
    if J in (1, 17, 33):
        cls.add("J == %d" % J)
    cls.add("Cp == 4J" if Cp == 4 * J else "Cp minimal, padded" if Cp == padded_channels(J) else "Cp wider than minimal")
    if (J, Cp) == (56, 224):
        cls.add("widest map")
    return cls


ALL_CLASSES = ({"JS %d, %s F" % (js, f) for js in (16, 32, 64) for f in ("power-of-two", "general")} | {"rs %d" % r for r in (1, 2, 4, 8)}
               | {"one tile", "several chunks", "more than 32 chunks", "ragged last chunk", "J == JS", "J == 1", "J == 17", "J == 33", "Cp == 4J",
                  "Cp minimal, padded", "Cp wider than minimal", "widest map"})


def nchw_classes(B, J, F, H):
    """The classes of an NCHW case: head_fwd_kernel / head_conf_kernel walk P pixels with 256 threads x 4 pixels a trip, the streaming kernels
    (head_bwd_kernel, joint2offset_kernel, dense_loss_kernel) start ceil(P / 1024) workgroups of 256 threads"""
    assert F % 4 == 0 and H % F == 0 and (H // F != 2 or H % 8 == 0)
    P, cls = F * F, {"nchw rs %d" % (H // F)}
    if P < 1024:
        cls.add("P < 1024")
        if P // 4 <= 192:
            cls.add("idle waves")
    if P % 1024:
        cls.add("P not a multiple of 1024")
    if P > 1024 and P % 1024:
        cls.add("full and partial trips")
    if P >= 4096:
        cls.add("P >= 4096")
    if J > 56:
        cls.add("J > 56")
    return cls


ALL_NCHW_CLASSES = {"nchw rs 1", "nchw rs 2", "nchw rs 4", "nchw rs 8", "P < 1024", "idle waves", "P not a multiple of 1024", "full and partial trips",
                    "P >= 4096", "J > 56"}


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def _hashed(shape, stream, scale):
    """uniform in [-scale, scale): tests/test_head_gpu.py's"""
    return torch.from_numpy((O._hash_uniform(int(np.prod(shape)), stream, 99) * np.float32(2 * scale)).reshape(shape).copy())


FAR = (2.0, -2.0, 2.0)      # farther than any ks in KSS from every pixel of the cube [-1, 1]^2 x [-0.9, 0.9]: an empty GT mask


@functools.lru_cache(maxsize=None)
def inputs(B, J, F, H, peaked=False):
    """One shape's inputs, made once and never modified: off (B, 4J, F, F), img (B, 1, H, H), jt_gt (B, J, 3), g_jt (B, J, 3).
    off: _hashed(..., 0.6), the distribution the project's bars were set on; `peaked` multiplies the heat channels by 5 (logits up to +-90).
    img: independent per pixel (uniform in +-0.9, about 30 % at 1.0, confidence_ref.bump_case's), so a neighbouring source pixel differs
    in mask and value; image 0 is all background, image 1 all foreground, the others mixed.
    jt_gt: uniform in +-0.6 like synth_batch's; joint 0 of every image sits at FAR (an empty GT mask); joint J - 1 of the last image sits
    0.01 from a hand pixel the kernels sample (a mask that is not empty, whatever the shape -- for J == 1 this is the one joint of that image).
    g_jt: an upstream gradient for the NCHW backward, _hashed(..., 1.0)."""
    assert B >= 3
    key = 1000 * J + 10 * F + H // F
    off = _hashed((B, 4 * J, F, F), 5 + key, 0.6)
    if peaked:
        off[:, 3 * J:] *= 5.0
    g = torch.Generator().manual_seed(7919 * key + B)
    img = torch.rand(B, 1, H, H, generator=g) * 1.8 - 0.9
    img[torch.rand(B, 1, H, H, generator=g) < 0.3] = 1.0
    img[0] = 1.0
    img[1] = torch.where(img[1] >= 0.99, torch.full_like(img[1], -0.25), img[1])
    jt_gt = (torch.rand(B, J, 3, generator=g) * 2 - 1) * 0.6
    jt_gt[:, 0] = torch.tensor(FAR)
    rs = H // F
    d = img[B - 1, 0, ::rs, ::rs]
    y, x = [int(v[0]) for v in torch.nonzero(d < 0.99, as_tuple=True)]
    a = 2.0 * (torch.arange(F).float() + 0.5) / F - 1.0
    jt_gt[B - 1, J - 1] = torch.stack([a[x] + 0.01, a[y], d[y, x]])
    return {"off": off.contiguous(), "img": img.contiguous(), "jt_gt": jt_gt.contiguous(), "g_jt": _hashed((B, J, 3), 6 + key, 1.0)}


def to_nhwc(x, cp):
    """(B, C, F, F) -> the head GEMM's (B, F*F, cp) rows, padding channels zero"""
    return R.to_nhwc(x, cp)


# ------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------
def gt_map64(jt_gt, img, ks, F):
    """The GT map (util/feature_tool.py:29-39) in float64 WITH THE MASK OF THE IEEE float32 RESTATEMENT: the mask is a hard threshold
    (heat map >= 0), so a pixel whose distance to the joint is within rounding of ks is inside in one precision and outside in the other,
    which moves its four map values by O(1).  That is a decision, not an error: float64 takes the decision the kernels must take
    (O.joint2offset_ieee, bit for bit) and measures the rounding of everything else."""
    B, J, _ = jt_gt.shape
    ieee = torch.from_numpy(O.joint2offset_ieee(jt_gt, img, ks, F))
    mask = ((ieee[:, :3 * J].reshape(B, J, 3, F, F) != 0).any(2) | (ieee[:, 3 * J:] != 0)).double()      # a unit vector is never all zero
    rs = img.shape[-1] // F
    d = img[:, 0, ::rs, ::rs].double()
    a = 2.0 * (torch.arange(F, dtype=torch.float64) + 0.5) / F - 1.0
    coord = torch.stack([a.view(1, 1, F).expand(B, F, F), a.view(1, F, 1).expand(B, F, F), d], 1)
    off = jt_gt.double().view(B, J, 3, 1, 1) - coord.view(B, 1, 3, F, F)
    dist = torch.sqrt((off * off).sum(2) + 1e-8)
    return torch.cat([(off / dist.unsqueeze(2) * mask.unsqueeze(2)).reshape(B, 3 * J, F, F), (ks - dist) / ks * mask], 1)


def _loss_refs(c, ks, cw, dw, f64):
    dt = torch.float64 if f64 else torch.float32
    O.HIGH_PRECISION = bool(f64)
    try:
        img, jt_gt = c["img"].to(dt), c["jt_gt"].to(dt)
        x = c["off"].to(dt).clone().requires_grad_(True)
        jt = O.offset2joint_softmax(x, img, ks)
        gt = gt_map64(c["jt_gt"], c["img"], ks, x.shape[-1]) if f64 else O.joint2offset(jt_gt, img, ks, x.shape[-1])
        lc, ld = O.huber(jt, jt_gt), O.huber(x, gt)
        (cw * lc + dw * ld).backward()
    finally:
        O.HIGH_PRECISION = False
    assert jt.dtype == dt and x.grad.dtype == dt
    return {"jt": jt.detach(), "lc": float(lc.detach()), "ld": float(ld.detach()), "grad": x.grad, "gt": gt.detach()}


@functools.lru_cache(maxsize=None)
def loss_refs(B, J, F, H, ks, cw, dw=1.0, peaked=False):
    """The fp32 oracle's answers for one train-step head: joints, the two Huber means (unweighted), the gradient of cw lc + dw ld with
    respect to the dense map (B, 4J, F, F), the GT map.  Computed once, shared, never modified."""
    return _loss_refs(inputs(B, J, F, H, peaked), ks, cw, dw, False)


def loss_refs64(B, J, F, H, ks, cw, dw=1.0, peaked=False):
    """The same formulas in float64 (not cached: only a case that misses a fixed bar and the peaked cases ask)"""
    return _loss_refs(inputs(B, J, F, H, peaked), ks, cw, dw, True)


@functools.lru_cache(maxsize=None)
def dense_refs(B, J, F, H, ks, w):
    """(w x the dense Huber mean, its gradient with respect to the map) for awr_dense_loss alone, with the GT map of O.joint2offset_ieee.
    The bar on this gradient is 1e-6 max|g| with max|g| = w 0.01 / N, i.e. 1e-8 of the Huber argument z = pred - gt -- below the
    one unit in the last place (6e-8) by which torch's CPU sqrt moves 0.6 % of O.joint2offset's map (tests/test_head_gpu.py::
    test_joint2offset_bit_exact).  The IEEE restatement is the map the kernel reproduces bit for bit, so z is the same float32 number on
    both sides and the bar measures the Huber arithmetic."""
    c = inputs(B, J, F, H)
    gt = torch.from_numpy(O.joint2offset_ieee(c["jt_gt"], c["img"], ks, F))
    x = c["off"].clone().requires_grad_(True)
    loss = w * O.huber(x, gt)
    loss.backward()
    return {"loss": float(loss.detach()), "grad": x.grad}


def head_refs(B, J, F, H, ks, f64=False, peaked=False):
    """(joints, closed-form head gradient for the upstream gradient inputs()["g_jt"]) of the oracle in float32 or float64"""
    c = inputs(B, J, F, H, peaked)
    dt = torch.float64 if f64 else torch.float32
    O.HIGH_PRECISION = bool(f64)
    try:
        jt = O.offset2joint_softmax(c["off"].to(dt), c["img"].to(dt), ks)
        g = O.head_backward(c["off"].to(dt), c["img"].to(dt), ks, c["g_jt"].to(dt))
    finally:
        O.HIGH_PRECISION = False
    assert jt.dtype == dt and g.dtype == dt
    return jt, g


def joint_bar(got, ref):
    """(largest |got - ref|, the project's bar: 1e-3 mm of a 150 mm half-cube is 6.7e-6 normalised; the suite holds 3e-6)"""
    return float((got.double() - ref.double()).abs().max()), 3e-6


def grad_bar(got, ref):
    """(largest |got - ref|, 3e-6 max|ref| + 1e-9)"""
    return float((got.double() - ref.double()).abs().max()), 3e-6 * float(ref.abs().max()) + 1e-9


def loss_ok(got, ref, floor=0.0):
    return abs(got - ref) <= 2e-6 * max(floor, abs(ref)) + 1e-9
