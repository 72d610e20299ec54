"""The NHWC head entry points on NaN-prefilled buffers (NhwcRun, shared with tests/test_head_forms_gpu.py), and the worker of
test_tuning_hook_instantiations: launch_dense_nhwc / nhwc_geometry read AWR_NHWC_DEPTH and AWR_NHWC_WGS once per process, so the DEPTH = 2
instantiations of dense_nhwc_kernel and the 8 / 16-tile runs of one workgroup need a process of their own.  Started with AWR_NHWC_DEPTH=2
AWR_NHWC_WGS=1, it runs the forward and both loss-step forms on HC.ENV_CASES, compares with the oracle and prints one JSON line."""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import head_cases as HC  # noqa: E402

NAN = float("nan")


class NhwcRun:
    """One NHWC case's device buffers and the entry points on them.  Every output and scratch buffer starts as NaN (fresh()), the padding
    channels of `pred` are zero; `want_wgs` is the AWR_NHWC_WGS of the process (the launch restatement needs it to know the partials)."""

    def __init__(self, L, dev, case, ks, peaked=False, want_wgs=HC.WANT_WGS):
        self.L, self.dev, self.case, self.ks = L, dev, case, ks
        B, J, F, H, cp = case
        c = HC.inputs(B, J, F, H, peaked)
        self.la = HC.nhwc_launch(*case, want_wgs=want_wgs)
        self.pred, self.img, self.jt_gt = HC.to_nhwc(c["off"], cp).to(dev), c["img"].to(dev), c["jt_gt"].to(dev)
        assert int(L.lib.awr_head_nhwc_scratch(B, J, F)) == HC.scratch_floats(B, J, F)
        self.fresh()

    def fresh(self):
        B, J, F, H, cp = self.case
        full = lambda *s: torch.full(s, NAN, device=self.dev)      # noqa: E731
        self.scratch, self.jt, self.stat, self.g_jt = full(HC.scratch_floats(B, J, F)), full(B, J, 3), full(B, J, 2), full(B, J, 3)
        self.grad, self.acc = full(B, F * F, cp), torch.zeros(2, device=self.dev, dtype=torch.float64)
        return self

    def forward(self):
        L, (B, J, F, H, cp) = self.L, self.case
        L.call("awr_head_forward_nhwc", L.ptr(self.pred), cp, L.ptr(self.img), B, J, F, H, self.ks, L.ptr(self.scratch), L.ptr(self.jt), L.ptr(self.stat),
               L.stream())
        torch.cuda.synchronize()
        return self

    def loss_step(self, cw, dw=1.0):
        L, (B, J, F, H, cp) = self.L, self.case
        L.call("awr_head_loss_step_nhwc", L.ptr(self.pred), cp, L.ptr(self.img), L.ptr(self.jt_gt), B, J, F, H, self.ks, HC.DELTA, cw, dw,
               L.ptr(self.scratch), L.ptr(self.jt), L.ptr(self.stat), L.ptr(self.g_jt), L.ptr(self.acc), L.ptr(self.grad), L.stream())
        torch.cuda.synchronize()
        return self

    def eval(self, cw, dw=1.0):
        L, (B, J, F, H, cp) = self.L, self.case
        L.call("awr_head_eval_nhwc", L.ptr(self.pred), cp, L.ptr(self.img), L.ptr(self.jt_gt), B, J, F, H, B, self.ks, HC.DELTA, cw, dw,
               L.ptr(self.scratch), L.ptr(self.jt), L.ptr(self.stat), L.ptr(self.acc), L.stream())
        torch.cuda.synchronize()
        return self

    def losses(self):
        """[coord, dense, total] as awr_loss_finalize reports them (weighted)"""
        out = torch.zeros(3, device=self.dev)
        self.L.call("awr_loss_finalize", self.L.ptr(self.acc), 2, self.L.ptr(out), self.L.stream())
        return out.tolist()

    def partials_written(self):
        """the B * chunks * J * 5 partials are all overwritten; what the documented scratch size holds beyond them is never touched"""
        n = self.la["partials"]
        return not bool(torch.isnan(self.scratch[:n]).any()) and bool(torch.isnan(self.scratch[n:]).all())

    def figures(self, cw):
        """after forward() (cw None) or loss_step(cw): the distances to the fp32 oracle with their bars, as plain numbers"""
        B, J, F, H, cp = self.case
        ref = HC.loss_refs(B, J, F, H, self.ks, 0.0 if cw is None else cw)
        dj, jbar = HC.joint_bar(self.jt.cpu(), ref["jt"])
        out = {"jt": dj, "jt_bar": jbar, "partials_written": self.partials_written(), "stat_finite": bool(torch.isfinite(self.stat).all())}
        if cw is not None:
            g, l = self.grad.cpu(), self.losses()
            dg, gbar = HC.grad_bar(g, HC.to_nhwc(ref["grad"], cp))
            out.update(grad=dg, grad_bar=gbar, grad_nans=int(torch.isnan(g).sum()), padding_zero=bool((g[:, :, 4 * J:] == 0).all()),
                       coord=l[0], coord_ref=cw * ref["lc"], dense=l[1], dense_ref=ref["ld"],
                       losses_ok=HC.loss_ok(l[0], cw * ref["lc"], 1e-3) and HC.loss_ok(l[1], ref["ld"]))
        return out


def main():
    assert os.environ.get("AWR_NHWC_DEPTH") == "2" and os.environ.get("AWR_NHWC_WGS") == "1"
    import awr_amd  # noqa: F401
    from awr_amd import _lib as L
    dev = torch.device("cuda:0")
    res = []
    for case in HC.ENV_CASES:
        for ks in HC.KSS:
            for cw in (None, 0.0, 1.0):
                run = NhwcRun(L, dev, case, ks, want_wgs=1)
                fig = run.forward().figures(None) if cw is None else run.loss_step(cw).figures(cw)
                fig.update(case=list(case), ks=ks, form="forward" if cw is None else "loss_step cw=%g" % cw, chunks=run.la["chunks"],
                           tiles_per_wg=run.la["tiles_per_wg"], last_tiles=run.la["last_tiles"])
                res.append(fig)
    print(json.dumps({"results": res}))


if __name__ == "__main__":
    main()
