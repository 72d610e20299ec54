"""Host restatement of the per-joint confidence and vote spread (include/awr_hip.h: awr_head_confidence), written from the
reference head, util/feature_tool.py:41-65, in torch on the CPU.  Two-pass: the joint first, the scatter about it second.  `dtype` picks
the precision of every intermediate: float64 is the reference the kernels are measured against, float32 -- the SAME code -- the yardstick
their error is compared with."""
import math

import torch


def votes_and_weights(offset, img, ks, dtype=torch.float64):
    """offset (B, 4J, F, F), img (B, 1, H, H) -> h (B, J, P) masked heat, w (B, J, P) aggregation weights, vote (B, J, 3, P)"""
    B, C4, F, _ = offset.shape
    J, H = C4 // 4, img.shape[-1]
    offset, img = offset.to(dtype), img.to(dtype)
    d = img[:, :, ::H // F, ::H // F]                                   # F.interpolate(img, size=[F, F]) (nearest) for H % F == 0
    axis = 2.0 * (torch.arange(F, dtype=dtype) + 0.5) / F - 1.0
    coords = torch.stack((axis.view(1, F).expand(F, F), axis.view(F, 1).expand(F, F)), 0).unsqueeze(0).expand(B, 2, F, F)
    coords = torch.cat((coords, d), 1).reshape(B, 1, 3, F * F)          # (u, v, depth) of every pixel
    mask = (d.float() < 0.99).to(dtype)                                 # :57  (the comparison is the reference's: on the float32 depth)
    vec = (offset[:, :3 * J] * mask).reshape(B, J, 3, F * F)            # :58
    h = (offset[:, 3 * J:] * mask).reshape(B, J, F * F)                 # :59
    w = torch.softmax(h * 30, dim=-1)                                   # :60
    dis = ks - h * ks                                                   # :61
    vote = vec * dis.unsqueeze(2) + coords                              # the summand of :63
    return h, w, vote


def joints(offset, img, ks, dtype=torch.float64):
    """(B, J, 3): what offset2joint_softmax returns, in `dtype`"""
    _, w, vote = votes_and_weights(offset, img, ks, dtype)
    return (vote * w.unsqueeze(2)).sum(-1)


def confidence(offset, img, ks, jt=None, dtype=torch.float64):
    """(B, J, 4) = [conf, var_u, var_v, var_d] in `dtype`.  jt (B, J, 3): the joint the scatter is taken about -- the one the head WROTE
    (its float32 output) when comparing with a kernel; None: this precision's own."""
    h, w, vote = votes_and_weights(offset, img, ks, dtype)
    jt = (vote * w.unsqueeze(2)).sum(-1) if jt is None else jt.to(dtype)
    conf = (w * h).sum(-1, keepdim=True)
    var = (w.unsqueeze(2) * (vote - jt.unsqueeze(-1)) ** 2).sum(-1)
    return torch.cat((conf, var), -1)


def peak(offset, img):
    """(B, J): the largest masked heat value"""
    h, _, _ = votes_and_weights(offset, img, 1.0, torch.float32)
    return h.max(-1).values


def spread_mm(conf4, cube):
    """conf4 (B, J, 4), cube (B, 3) or (3,) millimetres -> (B, J) float32, in the order of operations of awr_confidence_fields"""
    c = torch.as_tensor(cube, dtype=torch.float32).expand(conf4.shape[0], 3) * 0.5
    c2 = (c * c).unsqueeze(1)
    v = conf4.float()
    return torch.sqrt((v[..., 1] * c2[..., 0] + v[..., 2] * c2[..., 1]) + v[..., 3] * c2[..., 2])


def bump_case(B, J, F, H, seed):
    """The GPU tests' inputs: seeded normal offsets, a heat map of uniform noise in [0, 0.3] plus one Gaussian bump of height 0.9 per joint,
    a depth image with about 30 % of its pixels at 1.0 (background) -> offset (B, 4J, F, F), img (B, 1, H, H) float32"""
    g = torch.Generator().manual_seed(seed)
    vec = torch.randn(B, 3 * J, F, F, generator=g)
    ht = torch.rand(B, J, F, F, generator=g) * 0.3
    cy = torch.rand(B, J, 1, 1, generator=g) * (F - 1)
    cx = torch.rand(B, J, 1, 1, generator=g) * (F - 1)
    yy = torch.arange(F, dtype=torch.float32).view(1, 1, F, 1)
    xx = torch.arange(F, dtype=torch.float32).view(1, 1, 1, F)
    sigma = max(1.0, F / 8.0)
    ht = ht + 0.9 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))
    img = torch.rand(B, 1, H, H, generator=g) * 1.8 - 0.9
    img[torch.rand(B, 1, H, H, generator=g) < 0.3] = 1.0
    return torch.cat((vec, ht), 1).contiguous(), img.contiguous()


def to_nhwc(x, cp):
    """(B, C, F, F) -> the head GEMM's (B, F*F, cp) rows, padding channels zero"""
    B, C, F, _ = x.shape
    out = torch.zeros(B, F * F, cp, dtype=x.dtype)
    out[:, :, :C] = x.permute(0, 2, 3, 1).reshape(B, F * F, C)
    return out.contiguous()


def padded_channels(J):
    return (4 * J + 31) // 32 * 32


E30 = math.exp(30.0)
