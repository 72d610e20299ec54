"""Batched evaluator: the headline "mean 3D joint error (mm)" of the reference (util/eval_tool.py:20-122,
util/util.py:13-20) without the per-sample Python loop / per-sample np.linalg.inv / per-sample device sync
of train.py:141-148.  Same class name and methods as the reference's EvalUtil, plus `feed_batch`."""
import numpy as np


def uvd2xyz(pts, paras, flip=1):
    """Pinhole back-projection (util/util.py:13-20); paras = (fx, fy, u0, v0).  Like the reference, the arithmetic runs in
    float64 against the intrinsics and is stored in the dtype of `pts` (float32 from the evaluator, float64 from the loader)
    before the final float32 cast."""
    p = np.array(pts).reshape(-1, 3).copy()
    par = np.asarray(paras, np.float64)
    p[:, :2] = (p[:, :2] - par[2:]) * p[:, 2:] / par[:2]
    p[:, 1] *= flip
    return p.reshape(np.shape(pts)).astype(np.float32)


def xyz2uvd(pts, paras, flip=1):
    """util/util.py:3-10 (same dtype behaviour as uvd2xyz)."""
    p = np.array(pts).reshape(-1, 3).copy()
    par = np.asarray(paras, np.float64)
    p[:, 1] *= flip
    p[:, :2] = p[:, :2] * par[:2] / p[:, 2:] + par[2:]
    return p.reshape(np.shape(pts)).astype(np.float32)


class EvalUtil:
    def __init__(self, img_size, paras, flip, num_kp):
        self.img_size, self.paras, self.flip, self.num_kp = img_size, paras, flip, num_kp
        self.jt_uvd_pred = []          # original-image uvd per frame: what test.py:105-108 writes to results/*.txt
        self._err = []                 # (n, J) blocks of Euclidean errors in mm

    def feed_batch(self, jt_uvd_pred, jt_xyz_gt, center_xyz, M, cube):
        """All arguments batched on axis 0 (numpy or CPU tensors): eval_tool.py:20-46 for B frames at once."""
        jt = np.array(jt_uvd_pred, dtype=np.float32).copy()
        gt = np.asarray(jt_xyz_gt, np.float32)
        c = np.asarray(center_xyz, np.float32)
        Mi = np.linalg.inv(np.asarray(M, np.float32))                      # batched (B,3,3)
        cube = np.asarray(cube, np.float32)
        jt[:, :, :2] = (jt[:, :, :2] + 1) * self.img_size / 2.0            # :38
        jt[:, :, 2] = jt[:, :, 2] * cube[:, None, 2] / 2.0 + c[:, None, 2]  # :39
        hom = np.concatenate([jt[:, :, :2], np.ones(jt.shape[:2] + (1,), np.float64)], -1)
        jt[:, :, :2] = np.einsum("bij,bkj->bki", Mi.astype(np.float64), hom)[:, :, :2]   # :40-41
        self.jt_uvd_pred.extend(list(jt))
        xyz = uvd2xyz(jt, self.paras, self.flip)
        gt_mm = gt * (cube[:, None, :] / 2.0) + c[:, None, :]              # :46
        self._err.append(np.sqrt(np.sum(np.square(gt_mm - xyz), axis=2)))

    def feed(self, jt_uvd_pred, jt_xyz_gt, center_xyz, M, cube, jt_vis=0, skip_check=False):
        self.feed_batch(np.asarray(jt_uvd_pred)[None], np.asarray(jt_xyz_gt)[None], np.asarray(center_xyz)[None],
                        np.asarray(M)[None], np.asarray(cube)[None])

    def get_measures(self):
        """-> (mean error, median error, AUC, PCK curve, thresholds); eval_tool.py:80-122."""
        e = np.concatenate(self._err, 0).astype(np.float64)
        th = np.linspace(0, 50, 100)
        trapz = getattr(np, "trapezoid", None) or np.trapz
        norm = trapz(np.ones_like(th), th)
        mean = np.mean(e.mean(0))
        med = np.mean(np.median(e, 0))
        pck = (e[None, :, :] <= th[:, None, None]).mean(1).T            # (J, 100)
        auc = np.mean([trapz(pck[j], th) / norm for j in range(e.shape[1])])
        return mean, med, auc, pck.mean(0), th

    def plot_pck(self, path, pck_curve_all, thresholds):
        """eval_tool.py:124-135 (PIL instead of matplotlib)."""
        from .vis_tool import plot_pck
        plot_pck(path, pck_curve_all, thresholds)


class DeviceEvalUtil:
    """EvalUtil with the scoring on the GPU (awr_eval_batch, csrc/awr_eval.hip): `feed_batch` takes the engines' device tensors as they are,
    launches one kernel on the current stream and returns without synchronising; per-frame rows and float64 running sums stay on the device
    until `get_measures` / `jt_uvd_pred` / `mean_error` read them -- the only calls that synchronise.

    capacity: rows of the per-frame result buffers (None: they grow geometrically).  store=False keeps the running sums only -- no per-frame
    buffer is ever allocated, so a training run's memory stays constant; `get_measures` and `jt_uvd_pred` are then unavailable.
    A frame whose crop matrix is singular or non-finite (numpy raises on the host) gets NaN rows and a status code: the next read raises AwrError."""

    _MIN_ROWS = 1024

    def __init__(self, img_size, paras, flip, num_kp, capacity=None, device=None, store=True):
        import torch
        from . import _lib as L
        if not torch.cuda.is_available():
            raise L.AwrError("DeviceEvalUtil scores joints with a HIP kernel and needs a GPU: none is visible -- use EvalUtil (config.device_eval = "
                             "False) for host-side scoring")
        if not 0 < int(num_kp) <= 256:
            raise ValueError("num_kp must be in [1, 256] (AWR_EVAL_MAX_JOINTS), got %r" % (num_kp,))
        self.img_size, self.paras, self.flip, self.num_kp = img_size, paras, flip, int(num_kp)
        self.store, self.device = bool(store), torch.device(device if device is not None else "cuda")
        self._L, self._torch = L, torch
        self._acc = torch.zeros(self.num_kp + 2, dtype=torch.float64, device=self.device)     # awr_eval_batch's `acc`
        self._status = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._n = 0                      # frames fed
        self._err = self._uvd = None     # (capacity, J) / (capacity, J, 3) float32 on the device
        self._uvd_host = None
        if self.store and capacity:
            self._reserve(int(capacity), exact=True)

    def _reserve(self, rows, exact=False):
        torch = self._torch
        have = 0 if self._err is None else self._err.shape[0]
        if rows <= have:
            return
        if not exact:                    # geometric growth: a run of N frames copies its rows O(log N) times
            rows = max(rows, 2 * have, self._MIN_ROWS)
        err = torch.empty((rows, self.num_kp), dtype=torch.float32, device=self.device)
        uvd = torch.empty((rows, self.num_kp, 3), dtype=torch.float32, device=self.device)
        if self._n:
            err[:self._n].copy_(self._err[:self._n])
            uvd[:self._n].copy_(self._uvd[:self._n])
        self._err, self._uvd = err, uvd

    def _dev(self, x, tail, what):
        """-> contiguous float32 tensor on the device: device tensors in place, host tensors / arrays uploaded without blocking"""
        torch = self._torch
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        if tuple(x.shape[1:]) != tail:
            raise ValueError("%s must be (B, %s), got %s" % (what, ", ".join(str(t) for t in tail), tuple(x.shape)))
        if not x.is_cuda:
            x = x.to(self.device, non_blocking=True)
        if x.dtype != torch.float32:
            x = x.float()
        return x if x.is_contiguous() else x.contiguous()

    def feed_batch(self, jt_uvd_pred, jt_xyz_gt, center_xyz, M, cube, n_valid=None):
        """eval_tool.py:20-46 for a batch, on the current stream; nothing is synchronised and nothing returned.  Rows >= n_valid (default: all
        of jt_uvd_pred's) of any argument influence nothing; the label arguments need no more than n_valid rows."""
        L, J = self._L, self.num_kp
        jt = self._dev(jt_uvd_pred, (J, 3), "jt_uvd_pred")
        B = int(jt.shape[0])
        n = B if n_valid is None else int(n_valid)
        if not 0 <= n <= B:
            raise ValueError("n_valid = %d is outside [0, %d]" % (n, B))
        if n == 0:
            return
        gt, c = self._dev(jt_xyz_gt, (J, 3), "jt_xyz_gt"), self._dev(center_xyz, (3,), "center_xyz")
        Mt, cb = self._dev(M, (3, 3), "M"), self._dev(cube, (3,), "cube")
        for t, what in ((gt, "jt_xyz_gt"), (c, "center_xyz"), (Mt, "M"), (cb, "cube")):
            if t.shape[0] < n:
                raise ValueError("%s has %d rows, fewer than n_valid = %d" % (what, t.shape[0], n))
        cap = 0
        if self.store:
            self._reserve(self._n + n)
            cap = int(self._err.shape[0])
            self._uvd_host = None
        fx, fy, u0, v0 = (float(p) for p in self.paras)
        L.call("awr_eval_batch", L.ptr(jt), L.ptr(gt), L.ptr(c), L.ptr(Mt), L.ptr(cb), B, J, n, float(self.img_size), fx, fy, u0, v0, int(self.flip),
               L.ptr(self._uvd) if self.store else None, L.ptr(self._err) if self.store else None, self._n, cap,
               self._acc.data_ptr(), self._status.data_ptr(), L.stream())
        self._n += n

    def feed(self, jt_uvd_pred, jt_xyz_gt, center_xyz, M, cube, jt_vis=0, skip_check=False):
        self.feed_batch(*((x if isinstance(x, self._torch.Tensor) else np.asarray(x))[None] for x in (jt_uvd_pred, jt_xyz_gt, center_xyz, M, cube)))

    def __len__(self):
        return self._n

    def check(self):
        """Synchronising: raise where the host evaluator would have (np.linalg.inv of a singular crop matrix)."""
        code, frame = self._status.tolist()
        if code:
            raise self._L.AwrError("device evaluator: the crop matrix M of frame %d is %s (status %d); its rows are NaN and it is left out of the "
                                   "running sums" % (frame, {1: "singular", 2: "not finite"}.get(code, "invalid"), code))

    def _need_rows(self, what):
        if not self.store:
            raise self._L.AwrError("DeviceEvalUtil(store=False) keeps only the running sums: %s needs the per-frame rows" % what)

    def errors(self):
        """(N, J) float32 errors in mm of every frame fed so far: one synchronising download."""
        self._need_rows("errors()")
        e = self._err[:self._n].cpu().numpy() if self._n else np.zeros((0, self.num_kp), np.float32)
        self.check()
        return e

    @property
    def jt_uvd_pred(self):
        """Original-image uvd per frame (what test.py:105-108 writes to results/*.txt), as the host evaluator's list; downloaded on first access."""
        self._need_rows("jt_uvd_pred")
        if self._uvd_host is None:
            u = self._uvd[:self._n].cpu().numpy() if self._n else np.zeros((0, self.num_kp, 3), np.float32)
            self.check()
            self._uvd_host = list(u)
        return self._uvd_host

    def host(self):
        """The host evaluator holding this one's error rows (and, once read, its uvd rows): everything downstream of scoring is EvalUtil's code."""
        ev = EvalUtil(self.img_size, self.paras, self.flip, self.num_kp)
        ev._err = [self.errors()]
        return ev

    def get_measures(self):
        """-> (mean error, median error, AUC, PCK curve, thresholds): EvalUtil.get_measures on the downloaded (N, J) error matrix."""
        return self.host().get_measures()

    def mean_error(self):
        """-> (sum over frames of the frame's mean joint error in mm, frames) from the device's float64 running sums: what the training loop's
        epoch metric needs, without the error matrix.  One synchronising read of J + 2 doubles."""
        acc = self._acc.tolist()
        self.check()
        return acc[self.num_kp + 1], int(acc[self.num_kp])

    def joint_error_sums(self):
        """-> per-joint error sums in mm (J,) float64 over the frames scored so far"""
        acc = self._acc.cpu().numpy()
        self.check()
        return acc[:self.num_kp].copy()

    def plot_pck(self, path, pck_curve_all, thresholds):
        from .vis_tool import plot_pck
        plot_pck(path, pck_curve_all, thresholds)
