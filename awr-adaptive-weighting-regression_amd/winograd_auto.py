"""winograd="auto": the Winograd mode of one engine's plan chosen by timing the candidates (TrainEngine / InferEngine).

The reference turns on `cudnn.benchmark` (train.py:30): the framework times its convolution algorithms per shape and keeps the fastest.  Here the
choice is per PLAN, not per launch (a weight gradient timed alone on its side stream misleads: csrc/awr_plan_run.hip, autotune): every candidate mode
is built as a whole plan, warmed up, tile-tuned and timed over a few steps, one plan alive at a time.  This module holds the host-side rules --
candidates, collapsing of duplicate plans, the choice, the data-parallel agreement and the decision cache -- as plain functions; the engines
supply the callbacks that build and time a plan.
"""
import json
import os
import statistics

import torch

MODES = ("direct", "forward", "forward+wgrad", "full")
TRAIN_CANDIDATES = MODES
INFER_CANDIDATES = ("direct", "forward")          # an eval plan has the forward form only
# candidate -> the mode whose plan it repeats when it adds no Winograd launch (same n_winograd): "forward" adds forward launches to "direct",
# "forward+wgrad" weight gradients to "forward", "full" data gradients to "forward+wgrad" (include/awr_hip.h: awr_set_conv_winograd)
PARENT = {"forward": "direct", "forward+wgrad": "forward", "full": "forward+wgrad"}
# two candidates closer than this (relative) are a tie, decided in favour of fewer Winograd launches: closer to the reference arithmetic
MARGIN = 0.01
DETERMINISTIC_REASON = "deterministic mode: a timing-dependent choice would change the summation order between runs; auto -> direct"


def mode_name(code, training=True):
    """Library code (awr_set_conv_winograd) -> mode name.  Bit 4 (ignore the launch-size rules) and bit 8 (no 64-channel tile form) do not change
    which launches the mode replaces; inference plans take the forward form in every non-zero mode."""
    code = int(code)
    if code == 0:
        return "direct"
    if not training:
        return "forward"
    return {2: "full", 3: "forward+wgrad"}.get(code & 3, "forward")


def choose(timings, n_winograd, margin=MARGIN):
    """timings {mode: ms per step} of the candidates that were timed (collapsed candidates are absent), n_winograd {mode: Winograd launches of
    its plan} -> the mode to run: the fastest, unless another one within `margin` of it has fewer Winograd launches (then the one with the fewest;
    equal counts: the faster)."""
    if not timings:
        raise ValueError("no timed candidate")
    best = min(timings.values())
    close = [m for m, t in timings.items() if t <= best * (1.0 + margin)]
    return min(close, key=lambda m: (n_winograd[m], timings[m], MODES.index(m)))


def search(candidates, build, time_ms, allreduce_max=None, margin=MARGIN):
    """Build the candidates in order and time the distinct ones.

    build(mode) -> n_winograd: makes `mode`'s plan the engine's current plan (the engine releases the previous candidate first);
    time_ms(mode) -> ms per step of the current plan; allreduce_max(list of floats) -> the element-wise maximum over the data-parallel ranks (None:
    one process).  A candidate whose n_winograd equals its PARENT's builds the same plan as the parent: it is collapsed onto it and not timed.
    Returns (chosen mode, {mode: ms} of the timed candidates, {mode: n_winograd}, {collapsed mode: the mode it repeats})."""
    n, timings, collapsed = {}, {}, {}
    for mode in candidates:
        n[mode] = int(build(mode))
        parent = PARENT.get(mode)
        if parent in n and n[mode] == n[parent]:
            collapsed[mode] = collapsed.get(parent, parent)
            continue
        timings[mode] = float(time_ms(mode))
    if allreduce_max is not None:
        # every rank times its own plan; the slowest rank sets a candidate's time, so all ranks choose the same mode (the set of timed
        # candidates depends on the plan shapes only: identical on every rank)
        modes = list(timings)
        timings = dict(zip(modes, (float(t) for t in allreduce_max([timings[m] for m in modes]))))
    return choose(timings, n, margin), timings, n, collapsed


def time_steps(fn, reps=5, per=3):
    """ms per call of `fn` (which enqueues work on the current stream): the median over `reps` HIP-event-timed runs of `per` calls each."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / per)
    return statistics.median(out)


def allreduce_max_fn(process_group, device):
    """allreduce_max for search() over `process_group` (None -> None).  NCCL / RCCL groups reduce on `device`, others (gloo) on the host."""
    if process_group is None:
        return None

    def allreduce_max(vals):
        backend = torch.distributed.get_backend(process_group)
        t = torch.tensor([float(v) for v in vals], dtype=torch.float64, device=device if backend == "nccl" else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX, group=process_group)
        return t.tolist()
    return allreduce_max


def agree(mode, candidates, process_group, device):
    """Data parallel: a decision read from the cache is used only if every rank read the same one (otherwise every rank searches).
    -> mode or None."""
    if process_group is None:
        return mode
    i = candidates.index(mode) if mode in candidates else -1
    hi, neg_lo = allreduce_max_fn(process_group, device)([i, -i])
    return candidates[i] if (hi == i and -neg_lo == i and i >= 0) else None


def decision_key(training, net, J, B, H, products, staging, accum):
    """Cache key of an auto decision: the parts of a plan that do not depend on the Winograd mode."""
    return "winograd_auto/%s/%s/J%d/B%d/H%d/x%d/s%d/a%d" % ("train" if training else "infer", net, J, B, H, products, staging, accum)


def load_decision(key, candidates):
    """-> the stored {"mode", "timings", "n_winograd", ...} under `key` in $AWR_TUNE_CACHE, or None (no cache, no entry, or a mode that is not a
    candidate here)."""
    cache_file = os.environ.get("AWR_TUNE_CACHE")
    if not cache_file or not os.path.exists(cache_file):
        return None
    try:
        ent = json.load(open(cache_file)).get(key)
    except (OSError, ValueError, AttributeError):
        return None
    if not isinstance(ent, dict) or ent.get("mode") not in candidates or not isinstance(ent.get("timings"), dict):
        return None
    return ent


def store_decision(key, mode, timings, n_winograd, collapsed):
    """Add the decision to $AWR_TUNE_CACHE (the file the tile tuner uses; no-op without it)."""
    cache_file = os.environ.get("AWR_TUNE_CACHE")
    if not cache_file:
        return
    try:
        allc = json.load(open(cache_file)) if os.path.exists(cache_file) else {}
    except (OSError, ValueError):
        allc = {}
    allc[key] = {"mode": mode, "timings": timings, "n_winograd": n_winograd, "collapsed": collapsed}
    try:
        json.dump(allc, open(cache_file, "w"))
    except OSError:
        pass
