"""What TrainEngine and InferEngine both do with a plan: resolve the Winograd mode and fetch the first plan, decide the head's boundary
layout, and the one-off set-up (Winograd candidate search, eager warm-up, tile autotune, hipGraph capture)."""
import os

import torch

from . import _lib as L
from . import _engine_winograd, _winograd_code
from . import winograd_auto as WA


class _PlanEngine:
    """Base of both engines.  The engine provides `net`, `B`, `H`, `J`, `F`, `stage`, `use_graph`, `graph`, the class tag `_kind`
    ("train" | "infer"), `_attach(plan)`, `_wino_plan(mode)` and `_core()`.
    winograd="auto" in both engines (winograd_auto.py): resolved at construction when deterministic mode or the decision cache settle it,
    otherwise by timing the candidate plans one at a time in the engine's one-off set-up (`_wino_search`)."""

    def _init_plan(self, winograd, accum, process_group, nhwc_boundary, autotune):
        """The constructors' plan stanza: the boundary wish (the argument wins; otherwise $AWR_NCHW_BOUNDARY), `winograd` resolved, the first
        plan built or fetched and attached, `winograd_mode` named."""
        training = self._kind == "train"
        # head + losses on the backbone's own NHWC layout (no transposes at the boundary, the dense map read once per step when
        # coord_weight == 0); AWR_NCHW_BOUNDARY=1 / nhwc_boundary=False keeps the reference-layout kernels (same-box A/B)
        self._want_nhwc = (os.environ.get("AWR_NCHW_BOUNDARY") != "1") if nhwc_boundary is None else bool(nhwc_boundary)
        self._scratch = self.winograd_timings = self.winograd_source = None
        self._wino_pending = False
        winograd = _engine_winograd(winograd)
        if winograd == "auto":          # (ragged-batch children are handed the parent's resolved mode: _ragged)
            winograd = self._wino_start(training, self.net.plan_accum(accum, training), process_group)
        self._winograd = winograd
        n0 = len(self.net._plans)
        self._attach(self._wino_plan(winograd))
        self._wino_own = {id(self.plan)} if len(self.net._plans) > n0 else set()       # plans this engine built (a candidate search may free them)
        self.winograd_mode = WA.mode_name(self.plan.winograd, training=training) if self.plan.n_winograd else "direct"
        self._autotune, self._compiled = bool(autotune), False

    def _attach_head(self, plan):
        """The NHWC boundary where it is wanted and the plan can serve it: the head's pointers into the plan and its scratch."""
        self.nhwc = self._want_nhwc and plan.set_nhwc_boundary(True)
        if self.nhwc:
            self._pred, self._gpred, self._cp = plan.head_nhwc(self.stage)
            if self._scratch is None:
                self._scratch = torch.zeros(int(L.lib.awr_head_nhwc_scratch(self.B, self.J, self.F)), device=self.net.device)

    def _tune_key(self):
        return "%s/%s/J%d/B%d/H%d" % (self._kind, type(self.net).__name__ + str(self.net.nstage), self.J, self.B, self.H)

    def _wants_tune(self):
        return self._autotune and not self.plan.tuned and not self.plan.det

    def _setup(self, restore=None):
        """One-off: [winograd="auto": the candidate plans timed, restore() after each,] eager warm-up run, GEMM tile autotune, hipGraph
        capture.  The caller has detached the collectives and rolls back what the runs changed."""
        if self._wino_pending:
            self._wino_search(restore)
        tune = self._wants_tune()
        if self.use_graph or tune:
            self._core()
            if tune:
                self.plan.autotune(cache_key=self._tune_key())
            if self.use_graph:
                torch.cuda.synchronize()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self._core()

    def _wino_start(self, training, acc, process_group):
        """-> the mode to build the engine's first plan with: the resolved one, or (search pending) the first candidate."""
        self._wino_pg, self._wino_key = process_group, None
        self._wino_candidates = WA.TRAIN_CANDIDATES if training else WA.INFER_CANDIDATES
        if L.lib.awr_get_deterministic():
            self.winograd_timings, self.winograd_source = {"skipped": WA.DETERMINISTIC_REASON}, "deterministic"
            return "direct"
        self._wino_key = WA.decision_key(training, type(self.net).__name__ + str(self.net.nstage), self.J, self.B, self.H,
                                         int(L.lib.awr_get_gemm_products()), int(L.lib.awr_get_gemm_staging()), acc)
        if training and (getattr(self, "_split_k", False) or L.lib.awr_get_train_split_k()):
            self._wino_key += "/k1"           # training split-K changes the direct launches every candidate is timed against
        ent = WA.load_decision(self._wino_key, self._wino_candidates)
        mode = WA.agree(ent["mode"] if ent else None, self._wino_candidates, process_group, self.net.device)
        if mode is not None:
            self.winograd_timings, self.winograd_source = dict(ent["timings"]), "cache"
            return mode
        self._wino_pending = True
        return self._wino_candidates[0]

    def _wino_search(self, restore=None):
        """Build, warm up, tile-tune and time every distinct candidate -- one plan alive at a time: a candidate this engine built is freed
        before the next one is built -- and leave the chosen plan attached, with the tile choices it was timed with.  The input batch is
        carried over to every candidate; restore() (training: the BatchNorm running statistics) runs after each one.  The caller has detached
        the collectives."""
        img, tiles = self.plan.img.clone(), {}

        def build(mode):
            code = _winograd_code(mode)
            if self.plan.winograd != code:
                old, self.plan = self.plan, None
                if id(old) in self._wino_own:
                    self._wino_own.discard(id(old))
                    self.net.release_plan(old)
                del old
                n0 = len(self.net._plans)
                plan = self._wino_plan(mode)
                if len(self.net._plans) > n0:
                    self._wino_own.add(id(plan))
                plan.img.copy_(img)
                self._attach(plan)
            if not self.plan.training:
                self.net.sync_weights(self.plan)          # (training passes repack the weights themselves)
            return self.plan.n_winograd

        def time_ms(mode):
            self._core()                                  # warm-up: kernels loaded, buffers hold real data
            if self._wants_tune():
                self.plan.autotune(cache_key=self._tune_key())
            tiles[mode] = dict(self.plan.tuned)
            ms = WA.time_steps(self._core)
            if restore is not None:
                restore()
            return ms

        mode, timings, n, collapsed = WA.search(self._wino_candidates, build, time_ms, WA.allreduce_max_fn(self._wino_pg, self.net.device))
        rebuild = self.plan.winograd != _winograd_code(mode)
        build(mode)
        if rebuild and tiles.get(mode):
            self.plan.apply_tuned(tiles[mode])
        self._winograd, self.winograd_mode = mode, mode
        self.winograd_timings, self.winograd_source, self._wino_pending = timings, "search", False
        if self._wino_pg is None or torch.distributed.get_rank(self._wino_pg) == 0:
            WA.store_decision(self._wino_key, mode, timings, n, collapsed)


_WinogradAuto = _PlanEngine
