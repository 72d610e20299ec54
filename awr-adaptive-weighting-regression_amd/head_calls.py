"""The head and loss launches of both engines (train.py:118-127, test.py:67-88), each entry point's argument list stated once.

Plain functions over an engine `e`: they read its plan, stage, B, J, F, H, ks, its NHWC handles (`_pred` / `_preds`, `_cp`, `_scratch`, `_gpred`)
and `jt_gt`, and pick the NHWC or the reference-layout entry point by `e.nhwc`.  Output tensors, weights, accumulators and the stream are
arguments: TrainEngine and InferEngine keep theirs under different names."""
from . import _lib as L

HUBER_DELTA = 0.01


def reassert_boundary(e):
    """Plans are shared: another engine on this network, or the drop-in module, may have left this one on the other boundary."""
    if e.nhwc != e.plan.nhwc:
        e.plan.set_nhwc_boundary(e.nhwc)


def head_forward(e, jt, stat, s, st=None):
    """Stage st's dense map (default: the engine's stage) -> joints `jt` and, stat not None, the softmax statistics."""
    st = e.stage if st is None else st
    if e.nhwc:
        L.call("awr_head_forward_nhwc", e._pred if st == e.stage else e._preds[st], e._cp, L.ptr(e.plan.img), e.B, e.J, e.F, e.H, e.ks, L.ptr(e._scratch), L.ptr(jt), L.ptr(stat), s)
    else:
        L.call("awr_head_forward", L.ptr(e.plan.outputs[st]), L.ptr(e.plan.img), e.B, e.J, e.F, e.H, e.ks, L.ptr(jt), L.ptr(stat), s)


def loss_step(e, s):
    """train.py:118-127 in one call on the NHWC map: joints, both Huber losses, d(loss)/d(map) written where the backward reads it."""
    L.call("awr_head_loss_step_nhwc", e._pred, e._cp, L.ptr(e.plan.img), L.ptr(e.jt_gt), e.B, e.J, e.F, e.H, e.ks, HUBER_DELTA, e.cw, e.dw,
           L.ptr(e._scratch), L.ptr(e.jt_pred), L.ptr(e.stat), L.ptr(e.g_jt), L.ptr(e.acc), e._gpred, s)


def dense_loss(e, st, nb, dw, acc, gout, s):
    """acc[1] += dw * Huber(stage st's map - GT map) over the first nb images; gout (or None: value only) gets its gradient."""
    L.call("awr_dense_loss", L.ptr(e.plan.outputs[st]), L.ptr(e.jt_gt), L.ptr(e.plan.img), nb, e.J, e.F, e.H, e.ks, HUBER_DELTA, dw,
           acc.data_ptr() + 8, L.ptr(gout), 0, s)


def joint_huber(e, jt, nb, cw, acc, g_jt, s):
    """acc[0] += cw * Huber(jt - jt_gt) over the first nb images; g_jt (or None: value only) gets its gradient."""
    L.call("awr_huber", L.ptr(jt), L.ptr(e.jt_gt), nb * e.J * 3, HUBER_DELTA, cw, L.ptr(acc), L.ptr(g_jt), 0, s)


def head_backward(e, s):
    """d(coord loss)/d(joints) `g_jt` -> added onto the dense-loss gradient of the engine's stage (reference layout)."""
    L.call("awr_head_backward", L.ptr(e.plan.outputs[e.stage]), L.ptr(e.plan.img), L.ptr(e.jt_pred), L.ptr(e.stat), L.ptr(e.g_jt), e.B, e.J, e.F, e.H,
           e.ks, L.ptr(e.plan.grad_outs[e.stage]), 1, s)


def eval_loss(e, st, nv, jt, stat, s):
    """Joints of stage st + its loss terms (means over the first nv images) added onto `e._lacc`.  NHWC: one read-only pass
    (awr_head_eval_nhwc); NCHW boundary: head, dense loss without a gradient buffer, Huber on the joints."""
    cw, dw = e._lw
    if e.nhwc:
        L.call("awr_head_eval_nhwc", e._preds[st], e._cp, L.ptr(e.plan.img), L.ptr(e.jt_gt), e.B, e.J, e.F, e.H, nv, e.ks, HUBER_DELTA, cw, dw,
               L.ptr(e._scratch), L.ptr(jt), L.ptr(stat), L.ptr(e._lacc), s)
        return
    head_forward(e, jt, stat, s, st)
    if nv > 0:
        dense_loss(e, st, nv, dw, e._lacc, None, s)
        if cw != 0.0:
            joint_huber(e, jt, nv, cw, e._lacc, None, s)


def confidence(e, s):
    """The second pass over the last stage's map, behind the head launch that wrote `jt` and `stat`."""
    if e.nhwc:
        L.call("awr_head_confidence_nhwc", e._pred, e._cp, L.ptr(e.plan.img), L.ptr(e.jt), L.ptr(e.stat), e.B, e.J, e.F, e.H, e.ks, L.ptr(e._scratch),
               L.ptr(e.conf), s)
    else:
        L.call("awr_head_confidence", L.ptr(e.plan.outputs[e.stage]), L.ptr(e.plan.img), L.ptr(e.jt), L.ptr(e.stat), e.B, e.J, e.F, e.H, e.ks,
               L.ptr(e.conf), s)
