"""TrainEngine, the optimisation step whose contract trainer.py states, and GradSync, the data-parallel plumbing over its flat arenas."""
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import _split_k_flag
from . import head_calls as HC
from .engine_base import _PlanEngine


class GradSync:
    """Data-parallel plumbing over flat arenas: parameter/buffer broadcast from rank 0 and a bucketed SUM
    all-reduce of the gradient arena [0, n).  Device-agnostic (RCCL on the GPUs, gloo in the CPU tests); the
    1/world averaging is folded into the optimiser kernel (`grad_scale`)."""

    def __init__(self, n, process_group=None, n_buckets=4, min_bucket=1 << 20):
        self.pg = process_group
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        nb = max(1, min(n_buckets, n // min_bucket or 1))
        edges = [round(i * n / nb / 4) * 4 for i in range(nb)] + [n]
        self.buckets = [(edges[i], edges[i + 1]) for i in range(nb) if edges[i + 1] > edges[i]]
        self.grad_scale = 1.0 / self.world

    def broadcast(self, *tensors):
        if self.pg is not None:
            for t in tensors:
                torch.distributed.broadcast(t, 0, group=self.pg)

    def allreduce(self, flat_grad):
        if self.world > 1:
            for lo, hi in self.buckets:
                torch.distributed.all_reduce(flat_grad[lo:hi], group=self.pg)

    def global_mean(self, total, count, device=None):
        """sum(total over ranks) / sum(count over ranks): every rank gets the SAME epoch metric (what drives the LR
        scheduler and the log lines), whatever its own shard looked like."""
        if self.world > 1:
            t = torch.tensor([float(total), float(count)], dtype=torch.float64, device=device)
            torch.distributed.all_reduce(t, group=self.pg)
            total, count = float(t[0]), float(t[1])
        return total / count if count else float("nan")


def _grad_options(accum_steps, clip_grad_norm, grad_norm):
    """TrainEngine's accum_steps / clip_grad_norm / grad_norm, checked (host arithmetic only) -> (accum_steps, max_norm or None, grad_norm)."""
    if isinstance(accum_steps, bool) or not isinstance(accum_steps, int):
        raise TypeError("accum_steps is an int >= 1, not %r" % (accum_steps,))
    if accum_steps < 1:
        raise ValueError("accum_steps is an int >= 1, not %r" % (accum_steps,))
    if clip_grad_norm is not None:
        if isinstance(clip_grad_norm, bool) or not isinstance(clip_grad_norm, (int, float)):
            raise TypeError("clip_grad_norm is None or a finite number > 0, not %r" % (clip_grad_norm,))
        if not (math.isfinite(clip_grad_norm) and clip_grad_norm > 0):
            raise ValueError("clip_grad_norm is None or a finite number > 0, not %r" % (clip_grad_norm,))
        clip_grad_norm = float(clip_grad_norm)
    if not isinstance(grad_norm, bool):
        raise TypeError("grad_norm is True or False, not %r" % (grad_norm,))
    return accum_steps, clip_grad_norm, grad_norm


def _ema_options(ema_decay, ema_warmup):
    """TrainEngine's ema_decay / ema_warmup, checked (host arithmetic only) -> (decay as a float or None, warm-up)."""
    if ema_decay is not None:
        if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)):
            raise TypeError("ema_decay is None or a number in the open interval (0, 1), not %r" % (ema_decay,))
        if not (math.isfinite(ema_decay) and 0.0 < ema_decay < 1.0):
            raise ValueError("ema_decay is None or a number in the open interval (0, 1), not %r" % (ema_decay,))
        ema_decay = float(ema_decay)
    if not isinstance(ema_warmup, bool):
        raise TypeError("ema_warmup is True or False, not %r" % (ema_warmup,))
    return ema_decay, ema_warmup


def ema_decay_at(decay, updates, warmup):
    """The decay d the NEXT weight-EMA update uses (ema = d * ema + (1 - d) * weights), `updates` = the number of updates already applied.
    Warm-up off: `decay`.  Warm-up on: min(decay, (1 + updates) / (10 + updates)), the TF / timm rule -- the first update uses 0.1, so the
    average forgets the initialisation at the rate it has seen weights; 0.999 is reached at updates = 8990.  Host arithmetic in double."""
    if not warmup:
        return decay
    return min(decay, (1.0 + updates) / (10.0 + updates))


class _EmaState:
    """What an engine and its ragged-batch children share behind the optimiser: the shadow network (a clone of the trained one, in eval()
    mode, scored and saved like any network) and the number of EMA updates applied to it (a host int: it drives the warm-up schedule)."""

    def __init__(self, net):
        self.net = net.clone().eval()
        self.updates = 0


class _GradWindow:
    """What an engine and its ragged-batch children share between the gradient arena and the optimiser: the accumulation arena, the number
    of micro-steps pending in it, and the device words awr_grad_norm writes."""

    def __init__(self, n, dev, accumulate, norm):
        self.pending = 0
        self.acc = torch.zeros(n, device=dev) if accumulate else None
        self.norm = self.scale = self.scratch = None
        if norm:
            self.norm = torch.full((1,), float("nan"), device=dev, dtype=torch.float64)          # (NaN: no applying step yet)
            self.scale = torch.ones(1, device=dev)
            self.scratch = torch.zeros(int(L.lib.awr_grad_norm_scratch(n)) // 8, device=dev, dtype=torch.float64)


def _optimizer_names(net):
    """The parameters in torch.optim's order (the index of a state-dict entry is the position in this list)."""
    return [k for k, _, kind in net._layout if kind in ("conv_w", "deconv_w", "conv_b", "bn_w", "bn_b")]


class TrainEngine(_PlanEngine):
    _kind = "train"

    def __init__(self, net, batch_size, img_size, kernel_size, coord_weight=0.0, dense_weight=1.0, lr=1e-3, weight_decay=0.0,
                 optimizer="adam", momentum=0.9, process_group=None, use_graph=False, n_buckets=4, autotune=True, wgrad_streams=2,
                 nhwc_boundary=None, trace_buckets=False, native_rccl=None, accum="auto", winograd=None, split_k=False, accum_steps=1,
                 clip_grad_norm=None, grad_norm=False, ema_decay=None, ema_warmup=True, _share=None):
        """split_k: False (default: the process-wide mode, off unless awr_amd.set_train_split_k / $AWR_TRAIN_SPLIT_K set it) | True -- the small
        forward / data-gradient launches of this engine's plan (few workgroups, a long K loop: low batches, the deep levels) split their K loop
        and take the BatchNorm statistics / fused BatchNorm-backward reductions from the reduce kernel (include/awr_hip.h: awr_set_train_split_k;
        DESIGN.md 4.13).  Any other value raises ValueError.
        accum: "auto" (default) | "ordered" | "blocked" | None (the process-wide mode, awr_amd.set_gemm_accum) -- accumulation order of the
        forward / data-gradient GEMMs of this engine's plan.  "blocked" is the parity mode (a conv's rounding error at torch-CPU's level, a few %
        slower); "auto" blocks only the launches with a long K extent (include/awr_hip.h: awr_set_gemm_accum), where an ordered chain's error
        is largest and blocking is cheapest; "ordered" is one chain per output element everywhere.
        winograd: None (the process-wide mode, awr_amd.set_conv_winograd) | False | True ("forward") | "forward+wgrad" | "full" -- Winograd F(2x2, 3x3)
        forward, or forward + weight gradient, or forward + data gradient + weight gradient, of the eligible stride-1 3x3 convolutions (include/awr_hip.h)
        | "auto" -- the fastest of those for this plan, timed by compile() (winograd_auto.py); `winograd_mode` names what the plan runs,
        `winograd_timings` holds the candidates' ms per step.
        accum_steps: 1 (default) | k > 1 -- gradient accumulation: every step() is a micro-step; micro-steps 1 .. k-1 of a
        window add their gradient into an engine-owned arena (awr_grad_accumulate) and leave the parameters and `step_count` alone, the k-th
        applies the sum with grad_scale = 1 / (world * k).  EVERY micro-step weighs 1/k, whatever its batch size (a ragged last batch counts
        like a full one).  `micro_step` = micro-steps pending in the window; flush() applies a partly filled window.
        clip_grad_norm: None (default) | a finite number > 0 -- every applying step measures the global L2 norm of the gradient the optimiser
        is about to read (awr_grad_norm: after the all-reduce, accumulated and averaged) and the optimiser multiplies by torch's
        clip_grad_norm_ coefficient, read from the device.  grad_norm: True measures the norm without clipping.  With either, `grad_norm`
        (float64, one element) and `clip_scale` (float32, one element) are device tensors valid until the next applying step; nothing
        synchronises.  With all three at their defaults the step issues the launches it always did.
        ema_decay: None (default: no shadow network, no memory, no launch) | d in the open interval (0, 1) -- an exponential moving average of
        the weights on the device: the engine keeps a shadow network (`ema_net` = net.clone(), eval mode) and every APPLYING
        step, and flush(), ends in two awr_ema_update launches behind the optimiser -- ema += (x - ema) * float32(1 - d_t) over the whole
        parameter arena and over the BatchNorm running statistics --, copies num_batches_tracked and counts `ema_updates`.  ema_warmup: True
        (default) -- d_t = ema_decay_at(d, ema_updates, True) = min(d, (1 + t) / (10 + t)) | False -- d_t = d.  The training state is only
        read; nothing synchronises.  A NaN or Inf in a parameter lands in its average and stays there."""
        # every keyword as it was passed: what _ragged builds a child from
        self._options = {k: v for k, v in locals().items() if k not in ("self", "net", "batch_size", "img_size", "kernel_size", "_share")}
        self._split_k = _split_k_flag(split_k)
        self.accum_steps, self._max_norm, self._want_norm = _grad_options(accum_steps, clip_grad_norm, grad_norm)
        self.ema_decay, self.ema_warmup = _ema_options(ema_decay, ema_warmup)
        if not next(net.parameters()).is_cuda:
            raise L.AwrError("TrainEngine needs the network on the GPU")
        self.net, self.B, self.H = net, batch_size, img_size
        self.ks, self.cw, self.dw = float(kernel_size), float(coord_weight), float(dense_weight)
        self.lr, self.wd, self.opt, self.momentum = float(lr), float(weight_decay), optimizer, float(momentum)
        self.J, self.stage, dev = net.J, net.nstage - 1, net.device
        self.F = img_size // getattr(net, "downsample", 2)      # train.py:110: ft_sz = img_size / downsample
        net.train()
        world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.dp = world > 1 or (process_group is not None and os.environ.get("AWR_FORCE_DP") == "1")   # test hook: 1-rank group
        # (single GPU: scattering the packed weight gradients bucket by bucket during the backward, like the data-parallel plans do, instead
        # of in one launch at the tail of the step was measured slower: 14.28-14.32 vs 14.00-14.05 ms, profiles/r03_summary.md)
        self._plan_kw = dict(supervised=(self.stage,), bn_repeat=net.nstage, n_buckets=n_buckets if self.dp else 1, accum=accum,
                             split_k=True if self._split_k else None)
        self._wgrad_streams = wgrad_streams
        self._init_plan(winograd, accum, process_group, nhwc_boundary, autotune)
        self.jt_gt, self.jt_pred, self.g_jt = (torch.zeros(batch_size, self.J, 3, device=dev) for _ in range(3))
        self.stat = torch.zeros(batch_size, self.J, 2, device=dev)
        self.acc = torch.zeros(2, device=dev, dtype=torch.float64)
        self.losses = torch.zeros(3, device=dev)          # [coord, dense, total]
        n = net.n_active
        self._children, self._works, self.step_count, self.graph = {}, [], 0, None
        self.use_graph = use_graph and not self.dp          # (data parallel: the bucket markers interleave RCCL calls with the backward: run it eagerly)
        self.sync = GradSync(n, process_group, n_buckets)
        self.world = self.sync.world
        self.trace_buckets, self._trace, self._tev = bool(trace_buckets), [], None
        # native_rccl (opt-in; AWR_NATIVE_RCCL=1): the library's own RCCL communicator (awr_dp_*, csrc/awr_dp.hip) exchanges the buckets
        # from inside the native replay -- no Python callback, no torch work objects; bootstrapped over `process_group`
        native = self.dp and not trace_buckets and ((os.environ.get("AWR_NATIVE_RCCL") == "1") if native_rccl is None else bool(native_rccl))
        if _share is not None:          # ragged-batch child: what lives in the parent engine -- optimiser state, accumulation window, EMA shadow, communicator
            self.m, self.v, self._win, self._ema, self.dpcomm = _share.m, _share.v, _share._win, _share._ema, _share.dpcomm if native else None
        else:
            if self.dp:             # identical initial parameters and BN buffers on every rank
                self.sync.broadcast(net.flat_params(), net._barena)
                net.weights_changed()
            self.m = torch.zeros(n, device=dev)
            self.v = torch.zeros(n, device=dev) if optimizer == "adam" else None
            self._win = _GradWindow(n, dev, self.accum_steps > 1, self._want_norm or self._max_norm is not None)
            # the shadow is cloned behind the data-parallel broadcast above: replicas start from equal bits (a plain copy, not a kernel call)
            self._ema = _EmaState(net) if self.ema_decay is not None else None
            self.dpcomm = None
        if self.dp:
            if native:
                if self.dpcomm is None:
                    from .engine import DpComm
                    self.dpcomm = DpComm.from_process_group(process_group)
                self.plan.set_dp(self.dpcomm)
            g = net.flat_grads()
            # torch's NCCL work stream waits for the compute stream at the point of the call and runs concurrently with
            # whatever is enqueued afterwards: the rest of the backward overlaps the bucket's all-reduce over xGMI

            def hook(lo, hi):
                if self.trace_buckets:       # timestamps on the stream the bucket was handed to (the plan's comm stream)
                    e0 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                w = torch.distributed.all_reduce(g[lo:hi], group=process_group, async_op=True)
                self._works.append(w)
                if self.trace_buckets:       # (tracing serialises this stream behind the collective; untraced steps do not wait here)
                    w.wait()
                    e1 = torch.cuda.Event(enable_timing=True)
                    e1.record()
                    self._trace.append((lo, hi, e0, e1))
            if self.dpcomm is None:
                self.plan.bucket_hook = hook

    def _attach(self, plan):
        """Make `plan` the engine's plan: side streams, NHWC boundary, head pointers (collectives: __init__ / compile())."""
        self.plan = plan
        # weight-gradient GEMMs on extra HIP stream(s): co-resident DIFFERENT kernels fill each other's bubbles (0 = off); data
        # parallel: one more stream that finished gradient buckets (scatter + all-reduce) are handed to
        plan.set_streams(self._wgrad_streams, comm=(self._wgrad_streams > 0 and self.dp))
        self._attach_head(plan)

    def _wino_plan(self, mode):
        return self.net.get_plan(self.B, self.H, True, winograd=mode, **self._plan_kw)

    # ---- the captured part: repack -> forward -> head + losses -> backward -------------------------------
    def _core(self):
        plan, s = self.plan, L.stream()
        plan.refresh_weights()
        plan.run_forward()
        HC.reassert_boundary(self)      # (the drop-in module shares plans and switches them back to the NCHW boundary)
        if self.nhwc:
            # (self.acc starts at zero and awr_loss_finalize_reset leaves it zeroed: no fill launch per step)
            HC.loss_step(self, s)
            L.call("awr_loss_finalize_reset", L.ptr(self.acc), 2, L.ptr(self.losses), s)
            plan.run_backward()
            return
        HC.head_forward(self, self.jt_pred, self.stat, s)
        L.call("awr_zero_f64", L.ptr(self.acc), 2, s)
        HC.dense_loss(self, self.stage, self.B, self.dw, self.acc, plan.grad_outs[self.stage], s)
        HC.joint_huber(self, self.jt_pred, self.B, self.cw, self.acc, self.g_jt if self.cw != 0.0 else None, s)
        if self.cw != 0.0:          # (otherwise nothing reads d(loss)/d(joints))
            HC.head_backward(self, s)
        L.call("awr_loss_finalize", L.ptr(self.acc), 2, L.ptr(self.losses), s)
        plan.run_backward()

    def bucket_timeline(self):
        """trace_buckets=True: where the gradient exchange of the LAST step sat relative to its backward -- milliseconds from the start
        of the step (stream timestamps): {"backward_end_ms", "buckets": [{"lo", "hi", "mbytes", "start_ms", "end_ms"}], "tail_ms"}.
        backward_end_ms is taken after the end-of-backward join (all side streams and the last bucket's exchange are in); tail_ms = the
        time from handing the LAST bucket over to that join -- the only exchange nothing is left to overlap with; every earlier bucket
        whose end_ms lies before the last bucket's start_ms ran entirely under the backward."""
        if not self.trace_buckets or self._tev is None:
            return None
        torch.cuda.synchronize()
        t0 = self._tev[0]
        bk = [{"lo": lo, "hi": hi, "mbytes": round((hi - lo) * 4e-6, 2), "start_ms": round(t0.elapsed_time(e0), 3), "end_ms": round(t0.elapsed_time(e1), 3)}
              for lo, hi, e0, e1 in self._trace]
        end = round(t0.elapsed_time(self._tev[1]), 3)
        return {"backward_end_ms": end, "buckets": bk, "tail_ms": round(end - bk[-1]["start_ms"], 3) if bk else 0.0}

    def dense_map(self, stage=None):
        """(B, 4J, F, F) dense map of the last step in the reference's layout."""
        return self.plan.dense_map(self.stage if stage is None else stage)

    def timed_core(self, every=False):
        """The captured part once more, serially, with a HIP-event pair around every launch (bench.py's roofline):
        -> {launch name: seconds} of the conv / stem launches (`every`: of all launches).  Not an optimisation step (no optimiser update)."""
        self.plan.refresh_weights()
        per = self.plan.timed("fwd", every)
        per.update(self.plan.timed("bwd", every))
        return per

    def timed_hbm(self, reps=5):
        """Serial passes with an event pair around the HBM-bound launches of the step that live outside the plan (bench.py's
        `roofline_hbm`): the head + loss part (train.py:118-127) and the optimiser (on scratch copies: no parameter moves).
        -> {name: seconds per call}.  Call after a step (the buffers hold real data)."""
        s, res = L.stream(), {}

        def t(name, fn):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name] = e0.elapsed_time(e1) * 1e-3 / reps
        if self.nhwc:
            t("head_loss_step_nhwc", lambda: HC.loss_step(self, s))
            t("head_forward_nhwc", lambda: HC.head_forward(self, self.jt_pred, self.stat, s))
        else:
            t("head_forward", lambda: HC.head_forward(self, self.jt_pred, self.stat, s))
            t("dense_loss", lambda: HC.dense_loss(self, self.stage, self.B, self.dw, self.acc, self.plan.grad_outs[self.stage], s))
            t("head_backward", lambda: HC.head_backward(self, s))
        if self.opt == "adam":
            n = self.net.n_active
            p, g, m, v = (x[:n].clone() for x in (self.net.flat_params(), self.net.flat_grads(), self.m, self.v))
            t("adam_step", lambda: L.call("awr_adam_step", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, self.lr, 0.9, 0.999, 1e-8, self.wd, max(self.step_count, 1),
                                          self.sync.grad_scale, s))
        self.acc.zero_()          # the passes above accumulated into the loss accumulators
        return res

    def _optimizer(self, g=None, g2=None, micro=1):
        """The optimiser launch of an applying step over g (default: the gradient arena) [+ g2], averaged over `micro` micro-steps."""
        net, win, s = self.net, self._win, L.stream()
        n, scale = net.n_active, self.sync.grad_scale
        if g is None and g2 is None and micro == 1 and win.norm is None:      # the defaults: the entry points and launches of a plain step
            if self.opt == "adam":
                L.call("awr_adam_step", L.ptr(net.flat_params()), L.ptr(net.flat_grads()), L.ptr(self.m), L.ptr(self.v), n, self.lr, 0.9, 0.999,
                       1e-8, self.wd, self.step_count, scale, s)
            else:
                L.call("awr_sgd_step", L.ptr(net.flat_params()), L.ptr(net.flat_grads()), L.ptr(self.m), n, self.lr, self.momentum, self.wd,
                       self.step_count, scale, s)
            return
        g = net.flat_grads() if g is None else g
        if micro > 1:
            scale = 1.0 / (self.world * micro)
        if win.norm is not None:      # norm of what the optimiser is about to read (data parallel: the all-reduce waits are behind us)
            L.call("awr_grad_norm", L.ptr(g), L.ptr(g2), n, scale, self._max_norm or 0.0, L.ptr(win.scratch), L.ptr(win.norm), L.ptr(win.scale), s)
        if self.opt == "adam":
            L.call("awr_adam_step_dev", L.ptr(net.flat_params()), L.ptr(g), L.ptr(g2), L.ptr(win.scale), L.ptr(self.m), L.ptr(self.v), n, self.lr,
                   0.9, 0.999, 1e-8, self.wd, self.step_count, scale, s)
        else:
            L.call("awr_sgd_step_dev", L.ptr(net.flat_params()), L.ptr(g), L.ptr(g2), L.ptr(win.scale), L.ptr(self.m), n, self.lr, self.momentum,
                   self.wd, self.step_count, scale, s)

    def _ema_update(self):
        """Behind the optimiser of an applying step, on its stream: the shadow's parameter arena (all n_params: the Hourglass tail past
        n_active never moves, and e + (e - e) * w == e) and buffer arena move towards the trained ones; the host counters are copied."""
        st = self._ema
        if st is None:
            return
        net, shadow, s = self.net, st.net, L.stream()
        # (the subtraction in Python double, rounded to float32 once)
        w = float(np.float32(1.0 - ema_decay_at(self.ema_decay, st.updates, self.ema_warmup)))
        L.call("awr_ema_update", L.ptr(shadow.flat_params()), L.ptr(net.flat_params()), net.n_params, w, s)
        L.call("awr_ema_update", L.ptr(shadow._barena), L.ptr(net._barena), net._barena.numel(), w, s)
        shadow._counters.copy_(net._counters)
        shadow.weights_changed()
        st.updates += 1

    def _ema_state(self):
        if self._ema is None:
            raise L.AwrError("TrainEngine was built without ema_decay: there is no EMA network")
        return self._ema

    ema_net = property(lambda self: self._ema_state().net, doc="the shadow network: the EMA of the weights and BatchNorm statistics, in eval() mode")
    ema_updates = property(lambda self: self._ema_state().updates, doc="EMA updates applied so far (a host int)")

    def ema_state_dict(self):
        """The shadow's state_dict() (the reference's keys, shapes and dtypes) as detached clones."""
        return {k: v.detach().clone() for k, v in self._ema_state().net.state_dict().items()}

    def load_ema_state_dict(self, sd, updates=0):
        """Inverse of ema_state_dict(): `updates` = the number of EMA updates `sd` has seen (it positions the warm-up schedule)."""
        if isinstance(updates, bool) or not isinstance(updates, int) or updates < 0:
            raise ValueError("updates is an int >= 0, not %r" % (updates,))
        st = self._ema_state()
        st.net.load_state_dict(sd)
        st.net.weights_changed()
        st.updates = updates

    def ema_reset(self):
        """shadow <- the current parameters, BatchNorm statistics and counters; ema_updates = 0 (plain copies on the current stream)."""
        st = self._ema_state()
        with torch.no_grad():
            st.net.flat_params().copy_(self.net.flat_params())
            st.net._barena.copy_(self.net._barena)
            st.net._counters.copy_(self.net._counters)
        st.net.weights_changed()
        st.updates = 0

    @property
    def micro_step(self):
        """Micro-steps pending in the accumulation window (a host int; always 0 with accum_steps == 1)."""
        return self._win.pending

    def _norm_tensor(self, name):
        t = getattr(self._win, name)
        if t is None:
            raise L.AwrError("TrainEngine was built without clip_grad_norm / grad_norm=True: the gradient norm is not measured")
        return t

    grad_norm = property(lambda self: self._norm_tensor("norm"), doc="(1,) float64 device tensor: grad_scale * |g| of the last applying step")
    clip_scale = property(lambda self: self._norm_tensor("scale"), doc="(1,) float32 device tensor: the coefficient the last applying step multiplied by")

    def flush(self):
        """Apply a partly filled accumulation window: one optimiser step over the accumulator with grad_scale = 1 / (world * pending).
        Does nothing when no micro-step is pending.  Data parallel: every rank calls it at the same point (no collective is issued: every
        micro-step's gradient was all-reduced when it ran)."""
        win = self._win
        if win.pending == 0:
            return
        self.step_count += 1
        self._optimizer(g=win.acc, micro=win.pending)
        self._ema_update()
        win.pending = 0
        self.net.weights_changed()

    def _ragged(self, b):
        """Engine for a smaller (last-of-epoch) batch: its own static plan, the SAME optimiser state and step counter
        (the reference's DataLoader keeps the ragged last batch, train.py:109 drop_last=False)."""
        eng = self._children.get(b)
        if eng is None:
            if self._wino_pending:          # winograd="auto": the child runs the mode the parent chose (its own plan is not timed)
                self.compile()
            # (nhwc_boundary, trace_buckets, native_rccl are NOT inherited: the child's follow the environment; tests/golden/engine_trace.json holds this)
            kw = dict(self._options, use_graph=False, autotune=False, wgrad_streams=0, winograd=self._winograd, _share=self,
                      nhwc_boundary=None, trace_buckets=False, native_rccl=None)
            eng = self._children[b] = type(self)(self.net, b, self.H, self.ks, **kw)
        eng.lr, eng.step_count = self.lr, self.step_count
        return eng

    def step(self, img, jt_uvd_gt):
        """One optimisation step on this rank's shard.  Returns (losses[coord,dense,total], jt_uvd_pred)
        as device tensors that are valid until the next step; nothing is synchronised.
        accum_steps = k > 1: one micro-step -- forward, losses, backward, BatchNorm statistics and (data parallel) the gradient exchange as
        ever; the first k-1 calls of a window end in awr_grad_accumulate, the k-th in the optimiser.
        ema_decay set: an applying step ends in the EMA update of the shadow network, outside the captured graph like the optimiser."""
        if img.shape[0] != self.B:
            if not 0 < img.shape[0] < self.B:
                raise L.AwrError("TrainEngine built for batches of %d got %d images" % (self.B, img.shape[0]))
            eng = self._ragged(int(img.shape[0]))
            out = eng.step(img, jt_uvd_gt)
            self.step_count = eng.step_count
            return out
        self.plan.img.copy_(img, non_blocking=True)
        self.jt_gt.copy_(jt_uvd_gt, non_blocking=True)
        if not self._compiled:
            self.compile()
        if self.trace_buckets:
            del self._trace[:]
            self._tev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            self._tev[0].record()
        try:
            if self.graph is not None:
                self.graph.replay()
            else:
                self._core()
        except Exception:
            # the NHWC loss call ADDS onto self.acc and only awr_loss_finalize_reset re-arms it: a step that dies between the two would
            # leave the next step's losses inflated
            self.acc.zero_()
            raise
        if self.trace_buckets:
            self._tev[1].record()
        self.net._counters += self.plan.bn_repeat          # num_batches_tracked of every BatchNorm (host side)
        if self.dp:
            for w in self._works:           # compute stream waits for the bucket all-reduces before the optimiser
                w.wait()
            self._works.clear()
        win = self._win
        if win.pending + 1 < self.accum_steps:          # micro-steps 1 .. k-1: parameters and step_count stay
            L.call("awr_grad_accumulate", L.ptr(win.acc), L.ptr(self.net.flat_grads()), self.net.n_active, 1 if win.pending == 0 else 0, L.stream())
            win.pending += 1
            return self.losses, self.jt_pred
        self.step_count += 1
        if win.pending:
            self._optimizer(g2=win.acc, micro=win.pending + 1)
            win.pending = 0
        else:
            self._optimizer()
        self._ema_update()
        self.net.weights_changed()
        return self.losses, self.jt_pred

    def compile(self, img=None, jt_uvd_gt=None):
        """One-off set-up of the static plan, NOT an optimisation step: runs the captured part once eagerly on the batch in the
        input buffers (kernel warm-up; its only side effect -- the BatchNorm running statistics -- is rolled back), times the GEMM
        tile candidates of every launch in place (engine.Plan.autotune) and captures repack + forward + head + losses + backward,
        with the weight-gradient side streams forked and joined inside the capture, as ONE hipGraph.  `step()` calls it on its
        first use; call it directly (optionally with a representative batch) to keep that cost out of the first step.
        winograd="auto" (not settled by the decision cache): first builds and times every distinct candidate plan the same way, one at a
        time, and keeps the chosen one (winograd_auto.py) -- parameters, BatchNorm statistics, optimiser state and inputs are left as they were."""
        if self._compiled:
            return
        if img is not None:
            self.plan.img.copy_(img, non_blocking=True)
            self.jt_gt.copy_(jt_uvd_gt, non_blocking=True)
        self._compiled = True
        if not (self.use_graph or self._wants_tune() or self._wino_pending):
            return
        hook, self.plan.bucket_hook = self.plan.bucket_hook, None          # no collectives during set-up
        if self.dpcomm is not None:
            self.plan.set_dp(None)
        keep = self.net._barena.clone()
        self._setup(restore=lambda: self.net._barena.copy_(keep))
        self.net._barena.copy_(keep)
        self.plan.bucket_hook = hook
        if self.dpcomm is not None:
            self.plan.set_dp(self.dpcomm)

    def set_lr(self, lr):
        self.lr = float(lr)

    # ---- optimizer state in torch.optim layout (checkpoint compatibility, train.py:165-170) ----------------
    def optimizer_state_dict(self):
        if self._win.pending:
            raise L.AwrError("optimizer_state_dict() with %d micro-step(s) pending in the accumulation window: call flush() first (a checkpoint "
                             "cannot hold a partly filled window)" % self._win.pending)
        net = self.net
        names = _optimizer_names(net)
        state = {}
        for i, k in enumerate(names):
            if k in net._unused:
                continue
            o, n, s = net._poff[k]
            ent = {"step": torch.tensor(float(self.step_count))}
            if self.opt == "adam":
                ent["exp_avg"] = self.m[o:o + n].view(s).clone()
                ent["exp_avg_sq"] = self.v[o:o + n].view(s).clone()
            else:
                ent["momentum_buffer"] = self.m[o:o + n].view(s).clone()
            state[i] = ent
        group = {"lr": self.lr, "weight_decay": self.wd, "params": list(range(len(names)))}
        if self.opt == "adam":
            group.update(betas=(0.9, 0.999), eps=1e-8, amsgrad=False)
        else:
            group.update(momentum=self.momentum, dampening=0, nesterov=False)
        return {"state": state if self.step_count else {}, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        """Inverse of optimizer_state_dict(): accepts a stock torch.optim.Adam/SGD state dict (train.py:84)."""
        net, steps = self.net, []
        for i, k in enumerate(_optimizer_names(net)):
            ent = sd.get("state", {}).get(i)
            if ent is None or k in net._unused:
                continue
            o, n, s = net._poff[k]
            if self.opt == "adam":
                self.m[o:o + n].copy_(ent["exp_avg"].reshape(-1))
                self.v[o:o + n].copy_(ent["exp_avg_sq"].reshape(-1))
                steps.append(int(float(ent["step"])))
            else:
                self.m[o:o + n].copy_(ent["momentum_buffer"].reshape(-1))
        if steps:
            self.step_count = max(steps)
        elif self.opt != "adam" and sd.get("state"):
            self.step_count = max(self.step_count, 1)


_load_opt_into = TrainEngine.load_optimizer_state_dict          # the same, spelled _load_opt_into(engine, sd)
