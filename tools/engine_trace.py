"""What TrainEngine and InferEngine hand to the library, configuration by configuration -> tests/golden/engine_trace.json (and, with
--bits, what they compute)

    python tools/engine_trace.py [--out tests/golden/engine_trace.json] [--bits FILE] [--config NAME ...]

The golden file is recorded ONCE, at the commit before the engines moved out of trainer.py onto one base class and one set of head launches
(DESIGN.md 3.1), and never regenerated from a later engine: tests/test_engine_trace_gpu.py asserts that every configuration still makes the
same library calls, in the same order, with the same small arguments.  The tool uses the public API only (and `from awr_amd.trainer import`),
so it runs unchanged in a checkout of either commit.

Recording (the trick of tools/predictor_trace.py): awr_amd._lib.call is replaced by a recorder from BEFORE the engine is constructed until
after its last step.  Of every call it keeps the entry-point name and, in order, every positional argument that is a bool or an int with
abs(x) < 2**20 (sizes, flags, step counts, the null stream; pointers fall out by their size), every float as its hex, and every None (a NULL
pointer: stat of an engine without confidence, the gradient buffer of a value-only loss).  ctypes out-parameters are not kept, and a run
of the plan layer's listing calls (LISTINGS: one op or tensor per call while a plan is built) is kept as its length.

Fixture: procedural weights, B = 2, H = 128, J = 14, kernel_size 1.0, autotune=False (the shape of tools/plan_snapshot.py: the smallest at
which both networks fork); a fresh network per configuration, so that no configuration sees another's plans.  A training configuration
records construction, compile(), then its steps (three unless its script says otherwise); an inference one construction, a first call, then
three calls.  Every configuration runs at nhwc_boundary True ("<name>/nhwc") and False ("<name>/nchw").  winograd="auto" is left out: its
search order depends on timings (tests/test_winograd_auto_*.py cover it).

--bits FILE additionally writes, per configuration, the SHA-256 of the bytes (after one synchronise) of the losses, the joints, conf,
loss_sums(), the parameter and BatchNorm arenas and the EMA arenas after the last step or call.  It switches awr_amd.set_deterministic on
before anything is built (a default plan may sum in a timing-dependent order); a configuration the deterministic mode refuses is recorded
with the refusal instead of hashes.  With --bits the trace is written only where --out names a file: the golden is recorded without it."""
import argparse
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (REPO, os.path.join(REPO, "oracle")) if p not in sys.path]

B, H, J, KS = 2, 128, 14, 1.0
FULL, RAGGED = ("step", B), ("step", 1)
STEPS3 = (FULL, FULL, FULL)
# name: (network, constructor keywords, script)
TRAIN = {
    "train_defaults": ("resnet_18", dict(), STEPS3),
    "train_coord": ("resnet_18", dict(coord_weight=1.0), STEPS3),
    "train_sgd": ("resnet_18", dict(optimizer="sgd"), STEPS3),
    "train_accum_clip": ("resnet_18", dict(accum_steps=2, clip_grad_norm=1.0), STEPS3 + (("flush",),)),
    "train_grad_norm": ("resnet_18", dict(grad_norm=True), STEPS3),
    "train_ema": ("resnet_18", dict(ema_decay=0.9), STEPS3),
    "train_split_k": ("resnet_18", dict(split_k=True), STEPS3),
    "train_ragged": ("resnet_18", dict(), (FULL, RAGGED, FULL)),
    "train_ragged_accum_ema": ("resnet_18", dict(accum_steps=2, ema_decay=0.9), (FULL, RAGGED, FULL)),
    "train_graph": ("resnet_18", dict(use_graph=True), STEPS3),
    "train_wino_forward_wgrad": ("resnet_18", dict(winograd="forward+wgrad"), STEPS3),
    "train_hourglass_1": ("hourglass_1", dict(), STEPS3),
    "train_timed_hbm": ("resnet_18", dict(), (FULL, ("timed_hbm",))),
    "train_timed_hbm_coord": ("resnet_18", dict(coord_weight=1.0), (FULL, ("timed_hbm",))),
}
PLAIN, GT, GT1 = ("call", False, None), ("call", True, None), ("call", True, 1)
INFER = {
    "infer_defaults": ("resnet_18", dict(), (PLAIN,) * 4),
    "infer_confidence": ("resnet_18", dict(confidence=True), (PLAIN,) * 4),
    "infer_loss": ("resnet_18", dict(loss_weights=(1.0, 1.0)), (GT, GT, GT1, PLAIN)),
    "infer_loss_confidence": ("resnet_18", dict(loss_weights=(0.0, 1.0), confidence=True), (GT, GT, GT1, PLAIN)),
    "infer_hourglass_2_all": ("hourglass_2", dict(loss_weights=(1.0, 1.0), loss_stages="all"), (GT, GT, GT1, PLAIN)),
    "infer_parity": ("resnet_18", dict(parity=True), (PLAIN,) * 4),
    "infer_winograd": ("resnet_18", dict(winograd=True), (PLAIN,) * 4),
    "infer_graph": ("resnet_18", dict(use_graph=True), (PLAIN,) * 4),
    "infer_graph_loss": ("resnet_18", dict(use_graph=True, loss_weights=(1.0, 1.0)), (GT, GT, PLAIN, GT1)),
}
# the plan layer lists what it built one op / tensor per call: a run of these is kept as [name, "times", n]
LISTINGS = ("awr_plan_op", "awr_net_tensor_info", "awr_plan_tensor", "awr_plan_bucket", "awr_plan_gemm")
CONFIGS = ["%s/%s" % (n, b) for n in list(TRAIN) + list(INFER) for b in ("nhwc", "nchw")]
_STATE = {}


def network(name):
    """a fresh `name` ("resnet_18" | "hourglass_<n>") with procedural weights on the GPU"""
    import awr_amd
    import awr_oracle as O
    if name not in _STATE:
        _STATE[name] = O.procedural_state(O.manifest_for(name, J), seed=7)
    m = awr_amd.get_deconv_net(int(name.split("_")[1]), J, 2) if name.startswith("resnet") else awr_amd.PoseNet(name, J)
    m.load_state_dict(_STATE[name], strict=True)
    return m.cuda()


def batch():
    import awr_oracle as O
    if "batch" not in _STATE:
        img, jt = O.synth_batch(B, H, J, seed=71)
        _STATE["batch"] = (img.cuda(), jt.cuda())
    return _STATE["batch"]


def kept(args):
    out = []
    for x in args:
        if isinstance(x, float):
            out.append(x.hex())
        elif x is None or isinstance(x, bool) or (isinstance(x, int) and abs(x) < 1 << 20):
            out.append(x)
    return out


def digest(t):
    t = t.detach().contiguous().cpu()
    return "%s %s %s" % (str(t.dtype), list(t.shape), hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())


def run_train(net, kw, script, nhwc):
    from awr_amd.trainer import TrainEngine
    img, jt = batch()
    eng = TrainEngine(net, B, H, KS, autotune=False, nhwc_boundary=nhwc, **kw)
    assert eng.nhwc == nhwc
    eng.compile(img, jt)
    for op in script:
        if op[0] == "step":
            eng.step(img[:op[1]], jt[:op[1]])
        elif op[0] == "flush":
            eng.flush()
        else:
            assert sorted(eng.timed_hbm(reps=1)) == sorted(
                ["head_loss_step_nhwc", "head_forward_nhwc", "adam_step"] if nhwc else ["head_forward", "dense_loss", "head_backward", "adam_step"])
    return eng


def bits_train(eng):
    net = eng.net
    bits = {"losses": digest(eng.losses), "jt_pred": digest(eng.jt_pred), "params": digest(net.flat_params()), "buffers": digest(net._barena)}
    if eng.ema_decay is not None:
        bits.update(ema_params=digest(eng.ema_net.flat_params()), ema_buffers=digest(eng.ema_net._barena), ema_updates=eng.ema_updates)
    if eng.accum_steps > 1 or eng._max_norm is not None:
        bits["micro_step"] = eng.micro_step
    return bits


def run_infer(net, kw, script, nhwc):
    from awr_amd.trainer import InferEngine
    img, jt = batch()
    eng = InferEngine(net, B, H, KS, autotune=False, nhwc_boundary=nhwc, **kw)
    assert eng.nhwc == nhwc
    for _, gt, nv in script:
        eng(img, *((jt,) if gt else ()), **({} if nv is None else dict(n_valid=nv)))
    return eng


def bits_infer(eng):
    bits = {"jt": digest(eng.jt)}
    if eng.confidence:
        bits.update(conf=digest(eng.conf), peak=digest(eng.peak))
    if eng._lw is not None:
        bits["loss_sums"] = [float(x).hex() for x in eng.loss_sums()]
    return bits


def trace(name, bits=False):
    """-> (the library calls of configuration `name`, its bits or None)"""
    from awr_amd import _lib as L
    base, boundary = name.rsplit("/", 1)
    training = base in TRAIN
    netname, kw, script = (TRAIN if training else INFER)[base]
    net = network(netname)
    calls, real = [], L.call

    def recorder(entry, *args):
        if entry in LISTINGS and calls and calls[-1][0] == entry:
            calls[-1][2] += 1
        else:
            calls.append([entry, "times", 1] if entry in LISTINGS else [entry] + kept(args))
        return real(entry, *args)
    L.call = recorder
    try:
        eng = (run_train if training else run_infer)(net, kw, script, boundary == "nhwc")
    finally:
        L.call = real
    torch.cuda.synchronize()
    return calls, ((bits_train if training else bits_infer)(eng) if bits else None)


def dump(path, what):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in what.items()) + "\n}\n")
    print("%s  %d bytes  sha256 %s" % (path, os.path.getsize(path), hashlib.sha256(open(path, "rb").read()).hexdigest()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="the trace (default without --bits: tests/golden/engine_trace.json)")
    ap.add_argument("--bits", default=None, help="deterministic mode; write the SHA-256 of what every configuration computed to this file")
    ap.add_argument("--config", nargs="*", default=CONFIGS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/engine_trace.py needs a GPU: nothing is launched without one")
    import awr_amd
    from awr_amd import _lib as L
    if a.bits is not None:
        awr_amd.set_deterministic(True)
    elif a.out is None:
        a.out = os.path.join(REPO, "tests", "golden", "engine_trace.json")
    calls, hashes = {}, {}
    for name in a.config:
        try:
            calls[name], hashes[name] = trace(name, a.bits is not None)
        except L.AwrError as e:
            if a.bits is None:
                raise
            calls[name], hashes[name] = [], {"refused": str(e)}
        print("%-36s %4d calls" % (name, len(calls[name])), flush=True)
    if a.out:
        dump(a.out, calls)
    if a.bits:
        dump(a.bits, hashes)


if __name__ == "__main__":
    main()
