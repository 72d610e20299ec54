"""InferEngine: the evaluation pass of the reference (test.py:67-88) on an eval-mode plan."""
import warnings

import torch

from . import _lib as L
from . import head_calls as HC
from .engine_base import _PlanEngine


class InferEngine(_PlanEngine):
    """test.py:67-86 without the per-sample host loop: img -> dense map -> joints, eval-mode BN; with `loss_weights` also the
    validation loss of test.py:73-88, from the same pass over the dense map (awr_head_eval_nhwc)."""

    _kind = "infer"
    confidence, stat, conf = False, None, None          # an engine without confidence=True: no statistics buffer, stat = NULL in every head launch

    def __init__(self, net, batch_size, img_size, kernel_size, use_graph=False, autotune=True, parity=False, winograd=None,
                 loss_weights=None, loss_stages="last", nhwc_boundary=None, confidence=False):
        """loss_weights: None (default: joints only, nothing about the engine changes) | (coord_weight, dense_weight) -- a call that is handed
        the ground-truth joints adds coord_weight * Huber(joints) + dense_weight * Huber(dense map - GT map) of its batch (test.py:73-86) to a
        device accumulator; `loss_means()` reads it.  loss_stages: "last" -- the stage TrainEngine supervises, what the [train loss] lines
        report | "all" -- the sum over the Hourglass stacks (test.py:74-80).  nhwc_boundary: None ($AWR_NCHW_BOUNDARY decides) | False: the
        reference-layout kernels (what a net with more than 56 joints gets anyway).
        parity=True: blocked accumulation in the GEMMs of this engine's plan (awr_amd.set_gemm_accum) -- scoring passes (test.py:67-86) care
        about the last digits of the joints, not about the last few per cent of throughput.
        winograd: None (the process-wide mode, awr_amd.set_conv_winograd) | False | True -- the eligible stride-1 3x3 convolutions of the eval plan as
        Winograd F(2x2, 3x3) with the folded BatchNorm / residual add in its epilogue (Hourglass: instead of the fused conv2 + conv3 launch) | "auto" --
        "direct" or "forward", whichever the first call times faster (winograd_auto.py; `winograd_mode`, `winograd_timings`).
        confidence: False (default: the launches and stat = NULL of an engine without it) | True -- the head launch also writes its softmax
        statistics and a second, read-only pass over the last stage's map (awr_head_confidence_nhwc / awr_head_confidence)
        follows it: after a call `conf` (B, J, 4) = [conf, var_u, var_v, var_d] and `peak` (B, J) are valid until the next call."""
        if not isinstance(confidence, bool):
            raise TypeError("confidence is True or False, not %r" % (confidence,))
        self.confidence = confidence
        self.net, self.B, self.H, self.ks = net, batch_size, img_size, float(kernel_size)
        self.parity = bool(parity)
        if self.parity and (int(L.lib.awr_get_gemm_products()) != 1 or int(L.lib.awr_get_gemm_staging()) == 0):
            # the blocked kernel exists for FP32-MFMA + LDS-DMA staging only: a scoring pass in the split-operand mode (config.gemm_products = 6)
            # or with register staging runs ordered and says so, instead of failing at its first launch
            warnings.warn("InferEngine(parity=True): blocked accumulation is not available with gemm_products = %d / staging = %d; "
                          "scoring with ordered accumulation" % (L.lib.awr_get_gemm_products(), L.lib.awr_get_gemm_staging()))
            self.parity = False
        net.eval()
        self.J, self.F, self.stage = net.J, img_size // getattr(net, "downsample", 2), net.nstage - 1
        if loss_stages not in ("last", "all"):
            raise ValueError("loss_stages is \"last\" or \"all\", not %r" % (loss_stages,))
        self._lw = None
        if loss_weights is not None:
            cw, dw = loss_weights
            self._lw = (float(cw), float(dw))
            self._loss_stages = list(range(net.nstage)) if loss_stages == "all" else [self.stage]
            self.jt_gt = torch.zeros(batch_size, self.J, 3, device=net.device)
            self._jt_aux = torch.zeros(batch_size, self.J, 3, device=net.device) if len(self._loss_stages) > 1 else None
            self._lacc = torch.zeros(2, device=net.device, dtype=torch.float64)      # sums over stages and batches of the per-batch means
            self._lout, self._lbatches = torch.zeros(3, device=net.device), 0
        self._accum = "blocked" if self.parity else None
        self._init_plan(winograd, self._accum, None, nhwc_boundary, autotune)
        self.jt = torch.zeros(batch_size, self.J, 3, device=net.device)
        if confidence:
            self.stat = torch.zeros(batch_size, self.J, 2, device=net.device)
            self.conf = torch.zeros(batch_size, self.J, 4, device=net.device)
        self.use_graph, self.graph = use_graph, None

    @property
    def peak(self):
        """(B, J): the largest masked heat value of each joint's map -- the head's softmax max over 30 (needs confidence=True)."""
        if self.stat is None:
            raise L.AwrError("InferEngine was built without confidence=True: there are no softmax statistics to read the peak from")
        return self.stat[..., 0] / 30.0

    def _attach(self, plan):
        self.plan = plan
        if plan.n_side == 0:          # forward branches (ResNet downsample projections, Hourglass skip residuals) run beside the main chain
            plan.set_streams(4)
        self._attach_head(plan)
        if self.nhwc and self._lw is not None:
            self._preds = {st: plan.head_nhwc(st)[0] for st in self._loss_stages}

    def _wino_plan(self, mode):
        return self.net.get_plan(self.B, self.H, False, accum=self._accum, winograd=mode)

    def _core(self, loss=None, n_valid=None):
        """loss: None = whenever the engine has loss weights (what the set-up runs and the captured graph do)."""
        HC.reassert_boundary(self)
        self.plan.run_forward()
        if (self._lw is not None) if loss is None else loss:
            self._head_and_loss(self.B if n_valid is None else n_valid)
        else:
            HC.head_forward(self, self.jt, self.stat, L.stream())
        if self.confidence:
            self._confidence()

    def _confidence(self):
        """The second pass over the last stage's map, behind the head launch that wrote `jt` and `stat`."""
        HC.confidence(self, L.stream())

    def _head_and_loss(self, nv):
        """Joints of the last stage + this batch's loss terms (means over its first nv images) of every stage in `_loss_stages`, added
        onto the device accumulator.  NHWC: one read-only pass per stage (awr_head_eval_nhwc); NCHW boundary: head, dense loss without a
        gradient buffer, Huber on the joints."""
        s = L.stream()
        for st in self._loss_stages:
            last = st == self.stage          # (stat: None without confidence=True)
            HC.eval_loss(self, st, nv, self.jt if last else self._jt_aux, self.stat if last else None, s)

    def reset_loss(self):
        """Clear the loss accumulator and the batch count (no synchronisation)."""
        if self._lw is not None:
            L.call("awr_zero_f64", L.ptr(self._lacc), 2, L.stream())
            self._lbatches = 0

    def loss_sums(self):
        """(sum of the per-batch coord terms, sum of the per-batch dense terms, batches) fed since the last reset -- what data-parallel
        ranks add up before dividing.  Synchronises."""
        if self._lw is None:
            raise L.AwrError("InferEngine was built without loss_weights: there is no loss to report")
        L.call("awr_loss_finalize", L.ptr(self._lacc), 2, L.ptr(self._lout), L.stream())      # the only reader of the accumulator (its encoding depends on the mode)
        c, d, _ = self._lout.tolist()
        return c, d, self._lbatches

    def loss_means(self):
        """{"coord", "dense", "total", "batches"}: the mean over the batches fed so far of the per-batch mean loss terms -- what
        AverageValueMeter.add(loss.item()) per batch reports (test.py:88).  The only call of the loss path that synchronises."""
        return _loss_dict(*self.loss_sums())

    def __call__(self, img, jt_uvd_gt=None, n_valid=None):
        """-> joints (B, J, 3) of the last stage.  jt_uvd_gt (needs loss_weights): the batch's ground-truth joints, (B, J, 3) or the first
        n_valid rows; the same pass adds this batch's mean loss terms over its first n_valid images (default: all B) to the accumulator and
        counts the batch.  Images past n_valid -- the padding of a ragged last batch -- still get their joints."""
        want = jt_uvd_gt is not None
        if want and self._lw is None:
            raise L.AwrError("InferEngine was built without loss_weights: it cannot score a batch against jt_uvd_gt")
        nv = self.B if n_valid is None else int(n_valid)
        if not 0 <= nv <= self.B:
            raise L.AwrError("n_valid = %d outside [0, %d]" % (nv, self.B))
        if want:
            rows = int(jt_uvd_gt.shape[0])
            if rows < nv or rows > self.B:
                raise L.AwrError("jt_uvd_gt has %d rows for n_valid = %d of a batch of %d" % (rows, nv, self.B))
            self.jt_gt[:rows].copy_(jt_uvd_gt, non_blocking=True)
        self.net.sync_weights(self.plan)
        self.plan.img.copy_(img, non_blocking=True)
        if not self._compiled:
            self._compiled = True
            self._setup()
            self.reset_loss()         # the candidate timing, the warm-up and the tuner's runs are not batches of the caller's
        if self.graph is not None and want == (self._lw is not None) and (nv == self.B or not want):
            self.graph.replay()       # (the captured launches score all B images; a ragged call or one without its ground truth runs eagerly)
        else:
            self._core(loss=want, n_valid=nv)
        if want and nv > 0:
            self._lbatches += 1
        return self.jt


def _loss_dict(coord, dense, batches):
    n = float(batches)
    c, d = (coord / n, dense / n) if batches else (float("nan"), float("nan"))
    return {"coord": c, "dense": d, "total": c + d, "batches": int(batches)}
