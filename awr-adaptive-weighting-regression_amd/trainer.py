"""The optimisation / evaluation step of the reference (train.py:107-131, :182-192; test.py:67-86)
as one fused, graph-capturable sequence of HIP kernels, plus single-node data parallelism.

`TrainEngine.step(img, jt_uvd_gt)` performs exactly the work of one reference iteration:

    offset_gt   = FM.joint2offset(jt_uvd_gt, img, ks, F)            (never materialised: fused into the loss)
    offset_pred = net(img)                                          (training-mode BN, running stats updated)
    jt_uvd_pred = FM.offset2joint_softmax(offset_pred, img, ks)
    loss        = coord_w * crit(jt_uvd_pred, jt_uvd_gt) + dense_w * crit(offset_pred, offset_gt)
    optimizer.zero_grad(); loss.backward(); optimizer.step()        (Adam/SGD with torch semantics)

with no host synchronisation: losses and predictions stay on the device until the caller reads
them.  Hourglass quirk (train.py:116-121): the reference runs the network `stacks` times per
iteration and keeps only the last stack's loss; one forward with the BN momentum compounded
`stacks` times is numerically identical and is what runs here.

Data parallel (new w.r.t. the reference, which is single-GPU): one process per GPU, each rank steps
its own shard of the minibatch, gradients are summed with RCCL all-reduce (torch.distributed backend
"nccl" == RCCL over xGMI) on the flat gradient arena and scaled by 1/world inside the optimiser
kernel.  BatchNorm statistics stay rank-local (what stock DDP does).
"""
import os

import numpy as np
import torch

from . import _lib as L
from .evaluator import DeviceEvalUtil, EvalUtil
# the engines live in modules of their own; everything that was ever imported from here still is
from .engine_base import _WinogradAuto  # noqa: F401
from .head_calls import HUBER_DELTA  # noqa: F401
from .infer_engine import InferEngine, _loss_dict
from .train_engine import GradSync, TrainEngine, _load_opt_into, ema_decay_at  # noqa: F401


class _Plateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'min', patience=2, min_lr=1e-8) (train.py:90),
    defaults factor=0.1, threshold=1e-4 'rel', cooldown=0 -- host-side, drives TrainEngine.set_lr."""

    def __init__(self, lr, patience=2, factor=0.1, min_lr=1e-8, threshold=1e-4):
        self.lr, self.patience, self.factor, self.min_lr, self.threshold = lr, patience, factor, min_lr, threshold
        self.best, self.bad = float("inf"), 0

    def step(self, metric):
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            self.lr = max(self.lr * self.factor, self.min_lr)
            self.bad = 0
        return self.lr


class SyntheticHands(torch.utils.data.Dataset):
    """Stand-in for dataloader/nyu_loader.py (the NYU files are not redistributable): yields the same 6-tuple
    `(img[1,S,S], jt_xyz[J,3], jt_uvd[J,3], center_xyz[3], M[3,3], cube[3])` (nyu_loader.py:66) with joints that lie
    on a synthetic hand surface, so a network can actually fit them."""

    def __init__(self, n, img_size=128, jt_num=14, seed=0):
        g = torch.Generator().manual_seed(seed)
        S = img_size
        yy, xx = torch.meshgrid(torch.arange(S).float(), torch.arange(S).float(), indexing="ij")
        c = S / 2 + (torch.rand(n, 2, generator=g) * 2 - 1) * (S / 16)
        R = 0.31 * S
        r2 = (xx - c[:, 0].view(n, 1, 1)) ** 2 + (yy - c[:, 1].view(n, 1, 1)) ** 2
        depth = (0.5 * r2 / (R * R) - 0.3).clamp(-1.0, 0.98)
        self.img = torch.where(r2 < R * R, depth, torch.ones(())).view(n, 1, S, S).contiguous()
        ang = torch.rand(n, jt_num, generator=g) * 6.2831853
        rad = torch.rand(n, jt_num, generator=g).sqrt() * 0.8 * R
        px = (c[:, 0:1] + rad * torch.cos(ang)).round().clamp(0, S - 1).long()
        py = (c[:, 1:2] + rad * torch.sin(ang)).round().clamp(0, S - 1).long()
        d = self.img[torch.arange(n).view(n, 1), 0, py, px]
        self.jt_uvd = torch.stack([(px.float() + 0.5) * 2 / S - 1, (py.float() + 0.5) * 2 / S - 1, d], -1)
        self.center = torch.tensor([0.0, 0.0, 750.0]).expand(n, 3).contiguous()
        self.cube = torch.tensor([300.0, 300.0, 300.0]).expand(n, 3).contiguous()
        s = 0.45                                   # crop matrix: original-image pixels -> crop pixels
        self.M = torch.tensor([[s, 0.0, 64.0 - 320.0 * s], [0.0, s, 64.0 - 240.0 * s], [0.0, 0.0, 1.0]]).expand(n, 3, 3).contiguous()
        # ground-truth xyz consistent with the evaluator's uvd -> xyz chain, normalised like loader.py:242-260
        from .evaluator import uvd2xyz
        uv = (self.jt_uvd[:, :, :2] + 1) * S / 2.0
        uv = (uv - torch.tensor([64.0 - 320.0 * s, 64.0 - 240.0 * s])) / s
        uvd = torch.cat([uv, self.jt_uvd[:, :, 2:] * 150.0 + 750.0], -1)
        xyz = torch.from_numpy(uvd2xyz(uvd.numpy(), (588.03, 587.07, 320.0, 240.0), -1))
        self.jt_xyz = (xyz - self.center.view(n, 1, 3)) / 150.0
        self.img_size, self.jt_num, self.paras, self.flip = S, jt_num, (588.03, 587.07, 320.0, 240.0), -1

    def __len__(self):
        return self.img.shape[0]

    def __getitem__(self, i):
        return self.img[i], self.jt_xyz[i], self.jt_uvd[i], self.center[i], self.M[i], self.cube[i]


def make_evaluator(config, data, device=None, **kw):
    """The evaluator a loop over `data` scores with: the host EvalUtil, or with config.device_eval the GPU one (kw: capacity, store)."""
    if getattr(config, "device_eval", False):
        return DeviceEvalUtil(data.img_size, data.paras, data.flip, data.jt_num, device=device, **kw)
    return EvalUtil(data.img_size, data.paras, data.flip, data.jt_num)


class Trainer:
    """The reference's Trainer (train.py:27-227, test.py:20-110) on the MI355X engines: same config attributes, same
    log lines, same checkpoint files, with the per-sample host loops removed.  `train_data` / `test_data` are any
    map-style datasets yielding the NYU 6-tuple (the reference's own `NYU(...)` objects work unchanged)."""

    def _datasets(self, config, train_data, test_data):
        """-> (train_data, test_data), from the config where neither was handed in (train.py:58-61), and `_render`: the device loader's
        renderer of each phase that has one."""
        self._render = {}
        if train_data is None and test_data is None:
            if config.dataset != "nyu":
                raise ValueError("only the NYU loader is provided (dataset=%r): pass train_data / test_data objects" % config.dataset)
            from .nyu_data import NYU
            root = os.path.join(config.data_dir, config.dataset)
            if not os.path.isdir(os.path.join(root, "test")):
                raise FileNotFoundError("NYU data not found under %s (expects train/ test/ center_*_refined.txt, dataloader/nyu_loader.py:38-49)" % root)
            kw = dict(img_size=config.img_size, cube=config.cube, jt_num=config.jt_num)
            if getattr(config, "device_loader", False):
                # frames decoded once into a uint16 memmap, resident in HBM for the run; datasets yield 200-byte parameter blocks and the
                # image batch is produced by one kernel launch per step (nyu_device.py)
                from . import nyu_device as DV
                NYU = DV.DeviceNYU
                for phase in ("train", "test"):
                    if os.path.isdir(os.path.join(root, phase)):
                        store = DV.FrameStore(DV.build_frame_cache(root, phase))
                        self._render[phase] = DV.Renderer(store, config.img_size, config.batch_size)
            if os.path.isdir(os.path.join(root, "train")):
                train_data = NYU(root, "train", aug_para=config.augment_para, **kw)
            test_data = NYU(root, "test", **kw)
        for phase, data in (("train", train_data), ("test", test_data)):      # a device dataset handed in as an object brings its frames along
            store = getattr(data, "frame_store", None)
            if store is not None and phase not in self._render:
                from . import nyu_device as DV
                self._render[phase] = DV.Renderer(store, config.img_size, config.batch_size)
        return train_data, test_data

    def __init__(self, config, train_data=None, test_data=None, process_group=None):
        from . import resnet_deconv, hourglass
        self.config, self.EvalUtil = config, EvalUtil
        self.trainData, self.testData = self._datasets(config, train_data, test_data)
        self.pg = process_group
        self.rank = torch.distributed.get_rank(process_group) if process_group is not None else 0
        self.work_dir = os.path.join(config.output_dir, config.dataset, "checkpoint_" + config.exp_id)
        self.result_dir = os.path.join(self.work_dir, "results")
        os.makedirs(self.result_dir, exist_ok=True)
        self.log = open(os.path.join(self.work_dir, "%s_%s.log" % (config.net, config.log_id)), "a") if self.rank == 0 else None
        self._msg("-------------------start programming-------------------", stdout=False)
        for k in sorted(k for k in dir(config) if not k.startswith("_") and not callable(getattr(config, k))):     # train.py:44-46
            self._msg(str(k) + ":" + str(getattr(config, k)))
        if "resnet" in config.net:
            self.net = resnet_deconv.get_deconv_net(int(config.net.split("_")[1]), config.jt_num, config.downsample)
            self.stacks = 1
        else:
            self.stacks = int(config.net.split("_")[1])
            self._msg("hourglass stacks:{}".format(self.stacks))
            self.net = hourglass.PoseNet(config.net, config.jt_num)
        self.net = self.net.cuda()
        self.best_records = {"epoch": 0, "MPE": 1e10, "AUC": 0}
        try:
            from .vis_tool import VisualUtil
            self._vis = VisualUtil(config.dataset)                   # train.py:43
        except ValueError:
            self._vis = None
        if getattr(config, "gemm_products", 1) != 1:      # opt-in split-operand GEMMs (process-wide)
            from . import set_gemm_products
            set_gemm_products(config.gemm_products)
        self.engine = TrainEngine(self.net, config.batch_size, config.img_size, config.kernel_size, config.coord_weight, config.dense_weight,
                                  config.lr, config.weight_decay, config.optimizer, process_group=process_group,
                                  use_graph=getattr(config, "use_hipgraph", False), accum=getattr(config, "accum", "auto"),
                                  winograd=getattr(config, "winograd", None), split_k=getattr(config, "train_split_k", False),
                                  accum_steps=getattr(config, "accum_steps", 1), clip_grad_norm=getattr(config, "clip_grad_norm", None),
                                  grad_norm=bool(getattr(config, "log_grad_norm", False)), ema_decay=getattr(config, "ema_decay", None),
                                  ema_warmup=getattr(config, "ema_warmup", True))
        self._ema_on = self.engine.ema_decay is not None
        if self._ema_on:
            self._msg("weight EMA: decay {}, warm-up {}".format(self.engine.ema_decay, "on" if self.engine.ema_warmup else "off"))
        self._log_norm = bool(getattr(config, "log_grad_norm", False)) or getattr(config, "clip_grad_norm", None) is not None
        # winograd="auto": the training step's choice is logged once; the scoring engine's is reused by every later test pass
        self._wino_logged, self._infer_winograd = False, None
        if config.load_model and os.path.exists(config.load_model):
            self._msg("loading model from {}".format(config.load_model))
            pth = torch.load(config.load_model, map_location="cpu", weights_only=False)     # trusted project artefact (best_records may hold numpy scalars)
            key = "model_ema" if getattr(config, "load_ema", False) else "model"      # load_ema: the averaged weights become the network's
            if key not in pth:
                raise L.AwrError("{} holds no \"{}\" entry{}".format(config.load_model, key, " (load_ema = True needs a checkpoint written with ema_decay)"
                                                                     if key == "model_ema" else ""))
            self.net.load_state_dict(pth[key])
            if "optimizer" in pth:
                self.engine.load_optimizer_state_dict(pth["optimizer"])
            if "best_records" in pth:
                self.best_records = pth["best_records"]
            if self._ema_on:          # (the engine cloned its shadow from the freshly initialised network)
                if "model_ema" in pth:
                    self.engine.load_ema_state_dict(pth["model_ema"], int(pth.get("ema_updates", 0)))
                    self._msg("weight EMA: restored from the checkpoint after {} updates".format(self.engine.ema_updates))
                else:
                    self.engine.ema_reset()
                    self._msg("weight EMA: the checkpoint holds no \"model_ema\", starting from its weights")
        # train.py:94-96: the learning rate is force-reset to config.lr after loading
        self.engine.set_lr(config.lr)
        self._plateau = _Plateau(config.lr) if config.scheduler == "auto" else None
        self._msg("learning rate: {:.1e}".format(config.lr))

    def _msg(self, msg, stdout=True):
        if self.rank != 0:
            return
        if stdout:
            print(msg)
        print(msg, file=self.log)

    def _images(self, first, phase):
        """First element of a batch -> (B, 1, S, S) float32 on the GPU: host-loader images are copied, device-loader parameter blocks
        (uint8, nyu_device.BLOCK_BYTES each) are rendered from the HBM-resident frames by one kernel launch."""
        if first.dtype == torch.uint8:
            r = self._render.get(phase)
            if r is None:
                raise L.AwrError("the dataset yields device-loader parameter blocks but no frame store was built for phase %r" % phase)
            return r(first)
        return first.cuda(non_blocking=True).float()

    def _loader(self, data, shuffle, epoch=0):
        """train.py:109: DataLoader(batch_size, shuffle=True, num_workers) -- drop_last=False like the reference: the ragged last
        batch of an epoch is trained on (TrainEngine keeps a second static plan for it).  Data parallel: every rank iterates its
        own 1/world shard of the epoch's permutation (DistributedSampler pads the shards to equal length, so all ranks see the
        same batch sizes and the 1/world gradient average stays the global mean), batch_size images per rank and step."""
        sampler = None
        if self.pg is not None:
            sampler = torch.utils.data.distributed.DistributedSampler(data, num_replicas=torch.distributed.get_world_size(self.pg), rank=self.rank,
                                                                      shuffle=shuffle, drop_last=False)
            sampler.set_epoch(epoch)
        return torch.utils.data.DataLoader(data, batch_size=self.config.batch_size, shuffle=shuffle and sampler is None, sampler=sampler,
                                           num_workers=int(getattr(self.config, "num_workers", 0)), drop_last=False)

    def train(self):
        cfg, eng = self.config, self.engine
        dev = self.net.device
        # train.py:102: ONE evaluator for the whole run -- the reference's `train mpe` (which drives ReduceLROnPlateau) is the
        # running mean over every frame fed since the start of training, not a per-epoch value.  Reproduced on purpose.
        ev = make_evaluator(cfg, self.trainData, device=dev, store=False)
        dev_eval = isinstance(ev, DeviceEvalUtil)      # config.device_eval: scored on the GPU, running sums only (constant memory over the run)
        for epoch in range(self.best_records["epoch"] + 1, cfg.max_epoch + 1):
            self.net.train()
            lsum, lcnt, pend, last_mean = torch.zeros(3, device=dev), 0, [], float("nan")

            def drain():
                for jt, a, b, c, d in pend:
                    ev.feed_batch(jt.cpu().numpy(), a.numpy(), b.numpy(), c.numpy(), d.numpy())
                del pend[:]

            def meter():                # mean of the per-step losses since the last print, identical on every rank
                if self.pg is None or not lcnt:
                    return (lsum / max(lcnt, 1)).tolist()
                t = torch.cat([lsum.double(), torch.tensor([float(lcnt)], dtype=torch.float64, device=dev)])
                torch.distributed.all_reduce(t, group=self.pg)
                return (t[:3] / t[3]).tolist()
            for ii, (img, jt_xyz_gt, jt_uvd_gt, center_xyz, M, cube) in enumerate(self._loader(self.trainData, True, epoch)):
                losses, jt_pred = eng.step(self._images(img, "train"), jt_uvd_gt.cuda(non_blocking=True))
                if not self._wino_logged and eng.winograd_source is not None:      # winograd="auto": what the first step chose
                    self._wino_logged = True
                    self._msg("winograd: auto -> {} ({}; {})".format(eng.winograd_mode, eng.winograd_source, ", ".join(
                        "{} {:.3f} ms".format(k, v) if isinstance(v, float) else "{}: {}".format(k, v) for k, v in eng.winograd_timings.items())))
                lsum += losses                                      # device-side meter: no loss.item() per iteration
                lcnt += 1
                if dev_eval:            # jt_pred is valid until the next step: scored in place, on the stream the next step is issued on
                    ev.feed_batch(jt_pred, jt_xyz_gt, center_xyz, M, cube)
                else:
                    pend.append((jt_pred.clone(), jt_xyz_gt, center_xyz, M, cube))
                if (ii + 1) % cfg.print_freq == 0:
                    l = meter()
                    last_mean = l[2]
                    # (log_grad_norm / clip_grad_norm: the norm of the last applying step, read where the losses were just read)
                    norm = "[grad norm: {:.5f}]".format(float(eng.grad_norm)) if self._log_norm else ""
                    self._msg("[epoch: {:02d}][train loss: {:.5f}][offset_loss: {:.5f}][coord_loss: {:.5f}]".format(epoch, l[2], l[1], l[0]) + norm)
                    lsum.zero_()
                    lcnt = 0
                    drain()
            drain()
            eng.flush()          # accum_steps: a window the epoch left partly filled is applied before the scheduler, the test pass and the checkpoint
            # rank-uniform metric: every rank must feed the SAME number to its LR scheduler, or the replicas would step the
            # (identical, all-reduced) gradients with different learning rates and silently diverge
            if dev_eval:
                train_mpe = eng.sync.global_mean(*ev.mean_error(), device=dev)     # (0.0, 0) for an epoch without a single batch
            elif ev._err:
                e = np.concatenate(ev._err, 0).astype(np.float64)
                train_mpe = eng.sync.global_mean(e.mean(1).sum(), e.shape[0], device=dev)
            else:
                train_mpe = eng.sync.global_mean(0.0, 0, device=dev)    # an epoch without a single batch (empty shard)
            last = meter()[2] if lcnt else last_mean                     # meter is reset at every print (train.py:139)
            self._msg("[epoch {:02d}], [train loss {:.5f}], [train mpe {:.5f}], [lr {:.1e}]".format(epoch, last, train_mpe, eng.lr))
            if cfg.scheduler == "auto":
                if train_mpe == train_mpe:                               # NaN (nothing evaluated yet) never steps the plateau counter
                    eng.set_lr(self._plateau.step(train_mpe))
            elif cfg.scheduler == "step":                          # StepLR(step_size=cfg.step, gamma=0.1).step(epoch)
                eng.set_lr(cfg.lr * 0.1 ** (epoch // cfg.step))
            if self.testData is not None:
                self.test(epoch)
            if self.rank == 0:
                pth = {"model": self.net.state_dict(), "optimizer": eng.optimizer_state_dict(), "best_records": self.best_records}
                if self._ema_on:
                    pth.update(model_ema=eng.ema_state_dict(), ema_updates=eng.ema_updates)
                torch.save(pth, os.path.join(self.work_dir, "epoch_{}.pth".format(epoch)))
        if self.log:
            self.log.flush()

    @torch.no_grad()
    def test(self, epoch=0):
        """train.py:178-227 / test.py:51-110 -- DataLoader(batch_size, shuffle=False, num_workers) like the reference (worker processes
        decode the 8 252 NYU PNGs while the GPU runs), no per-sample host loop.  Data parallel: rank r evaluates batches r, r + world, ...
        of that loader's order; the per-frame error rows and original-image uvd predictions are gathered and re-assembled in dataset order
        on every rank, so mpe / AUC / the results txt are identical to the single-process run and rank-uniform.
        With config.ema_decay a second pass scores the engine's EMA network the same way (its own log lines tagged `ema`, its own PCK file,
        no results txt, no skeleton overlays); the returned mpe, best_records and the LR scheduler read the raw network's numbers."""
        mpe = self._score(self.net, False, epoch)
        if self._ema_on:
            self.last_test_mpe_ema = self._score(self.engine.ema_net, True, epoch)
        return mpe

    def _gather_rows(self, ev, idx, n, world):
        """Data parallel: the host evaluator `ev` of this rank's frames `idx` ends up with the error and uvd rows of all n frames, in dataset
        order, on every rank."""
        J = self.testData.jt_num
        err = np.concatenate(ev._err, 0) if ev._err else np.zeros((0, J), np.float32)
        uvd = np.asarray(ev.jt_uvd_pred, np.float32).reshape(-1, J, 3)
        parts = [None] * world
        torch.distributed.all_gather_object(parts, (idx, err, uvd), group=self.pg)
        full_e, full_u = np.zeros((n, J), err.dtype), np.zeros((n, J, 3), np.float32)
        for ids, e, u in parts:
            full_e[ids], full_u[ids] = e, u
        ev._err, ev.jt_uvd_pred = [full_e], list(full_u)

    def _score(self, net, ema, epoch):
        """one scoring pass over `net`: the trained network, or (ema) the engine's EMA network"""
        cfg = self.config
        world =torch.distributed.get_world_size(self.pg) if self.pg is not None else 1
        # config.parity_infer = True scores with blocked accumulation (eval-mode plans measure no gain from it: off by default since round 6)
        wino = getattr(cfg, "winograd", None)
        if isinstance(wino, str) and wino == "auto" and self._infer_winograd is not None:
            wino = self._infer_winograd
        test_loss = bool(getattr(cfg, "test_loss", False))      # test.py:73-88: the validation loss, from the pass that decodes the joints
        loss_kw = dict(loss_weights=(cfg.coord_weight, cfg.dense_weight), loss_stages=getattr(cfg, "test_loss_stages", "last")) if test_loss else {}
        inf = InferEngine(net, cfg.batch_size, cfg.img_size, cfg.kernel_size, use_graph=False,
                          parity=bool(getattr(cfg, "parity_infer", False)), winograd=wino, **loss_kw)
        if not ema:
            self._last_infer = inf
        n, bs = len(self.testData), cfg.batch_size
        mine = [b for b in range((n + bs - 1) // bs) if b % world == self.rank]
        idx = [i for b in mine for i in range(b * bs, min(n, (b + 1) * bs))]
        ev = make_evaluator(cfg, self.testData, device=net.device, capacity=len(idx))
        dev_eval = isinstance(ev, DeviceEvalUtil)      # config.device_eval: no download and no sync inside the batch loop
        loader = torch.utils.data.DataLoader(torch.utils.data.Subset(self.testData, idx), batch_size=bs, shuffle=False,
                                             num_workers=int(getattr(cfg, "num_workers", 0)), drop_last=False)
        pad = None
        vis = bool(getattr(cfg, "vis_freq", 0)) and self._vis is not None and not ema
        for k, (img, jt_xyz_gt, jt_uvd_gt, center_xyz, M, cube) in enumerate(loader):
            nb = img.shape[0]
            x = self._images(img, "test")
            if img.dtype == torch.uint8:                             # device loader: the host only ever saw parameter blocks
                img = x[:1].cpu() if (vis and (mine[k] + 1) % cfg.vis_freq == 0) else None
            if nb < bs:                                              # ragged last batch: fill the static plan's batch with zeros, drop them after
                if pad is None:
                    pad = torch.zeros((bs,) + tuple(x.shape[1:]), device=x.device)
                pad.zero_()
                pad[:nb] = x
                x = pad
            gt = (jt_uvd_gt.cuda(non_blocking=True).float(),) if test_loss else ()      # (rows past nb of a ragged batch are not read)
            if dev_eval:
                jt = inf(x, *gt, n_valid=nb)
                ev.feed_batch(jt, jt_xyz_gt, center_xyz, M, cube, n_valid=nb)
            else:
                jt = inf(x, *gt, n_valid=nb)[:nb].cpu().numpy()
                ev.feed_batch(jt, jt_xyz_gt.numpy(), center_xyz.numpy(), M.numpy(), cube.numpy())
            ib = mine[k] + 1
            if vis and ib % cfg.vis_freq == 0:    # train.py:203-213
                half = cfg.img_size / 2.0
                if dev_eval:             # the one joint set this iteration draws
                    jt = jt[:1].cpu().numpy()
                self._vis.plot(img[0].numpy(), os.path.join(self.result_dir, "test_epoch_{}_iter_{}.png".format(epoch, ib)),
                               (jt[0] + 1) * half, (jt_uvd_gt[0].numpy() + 1) * half)
        if not ema:          # (the EMA network is never trained: it stays in eval mode)
            self.net.train()
        if not ema and inf.winograd_source is not None and not inf._wino_pending:
            self._infer_winograd = inf.winograd_mode
        if dev_eval:           # one download of the error and uvd rows; from here on it is the host evaluator's code
            rows = ev.jt_uvd_pred
            ev = ev.host()
            ev.jt_uvd_pred = rows
        if world > 1:          # every rank ends up with the whole test set, in dataset order
            self._gather_rows(ev, idx, n, world)
        mpe, mid, auc, pck, thresh = ev.get_measures()
        if self.rank == 0:
            ev.plot_pck(os.path.join(self.work_dir, "test_pck_{}epoch_{}.png".format("ema_" if ema else "", epoch)), pck, thresh)      # train.py:216
        if epoch in (0, -1) and self.rank == 0 and not ema:                    # train.py:217-221 / test.py:103-108
            jt_uvd = np.array(ev.jt_uvd_pred, dtype=np.float32)
            np.savetxt(os.path.join(self.work_dir, "test_%.3f.txt" % mpe), jt_uvd.reshape([jt_uvd.shape[0], cfg.jt_num * 3]), fmt="%.3f")
        if ema:
            self._msg("[epoch {:2d}], [test mpe ema {:.3f}]".format(epoch, mpe))
        else:
            self._msg("[epoch {:2d}], [test mpe {:.3f}], [lr {:.1e}]".format(epoch, mpe, self.engine.lr))
        if test_loss:          # per-rank sums and batch counts are added up: every rank holds and logs the same means (like train()'s meter)
            t = torch.tensor(inf.loss_sums(), dtype=torch.float64, device=net.device)
            if world > 1:
                torch.distributed.all_reduce(t, group=self.pg)
            c, d, nbat = t.tolist()
            l = _loss_dict(c, d, int(nbat))
            setattr(self, "last_test_loss_ema" if ema else "last_test_loss", l)
            head = "[epoch {:2d}], [test loss ema {:.5f}]" if ema else "[epoch {:2d}], [test loss {:.5f}]"
            self._msg((head + "[offset_loss {:.5f}][coord_loss {:.5f}]").format(epoch, l["total"], l["dense"], l["coord"]))
        return mpe
