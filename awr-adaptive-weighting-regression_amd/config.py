"""`opt`: the configuration object the reference's entry points read (reference config.py:19-52).  Attribute names
and default values are the reference's -- train.py / test.py address them as `self.config.<name>` -- but the object is
built from tables, validates what it is given, and carries the knobs of the MI355X path."""

# per-dataset constants: joints, LR-decay step (epochs), epochs               (reference config.py:1-18)
_DATASETS = {
    #            joints  step  epochs
    "nyu":      (14,     30,   40),
    "icvl":     (16,     10,   40),
    "msra":     (21,     10,   25),
    "hands17":  (21,      5,   10),
}
JOINT = {k: v[0] for k, v in _DATASETS.items()}
STEP = {k: v[1] for k, v in _DATASETS.items()}
EPOCH = {k: v[2] for k, v in _DATASETS.items()}

_RUN = dict(gpu_id=0, exp_id="nyu_hourglass", log_id="dense", print_freq=100, vis_freq=1)
_PATHS = dict(data_dir="./data", output_dir="./output/", load_model="./results/hourglass_1.pth")
_DATA = dict(dataset="nyu", cube=[300, 300, 300], augment_para=[10, 0.1, 180], img_size=128, batch_size=32, num_workers=8)
_MODEL = dict(net="hourglass_1",      # or 'resnet_18'
              downsample=2,           # 1, 2 or 4: feature size = img_size / downsample
              kernel_size=0.4)        # 0.4 for hourglass, 1 for resnet
_OPTIM = dict(loss_type="MyL1Loss", dense_weight=1.0, coord_weight=0, lr=1e-3, optimizer="adam", scheduler="step", weight_decay=0)
_MI355X = dict(use_hipgraph=False,    # True: replay each step as one hipGraph (measured slower than eager two-stream issue at every batch size)
               world_size=1,          # data-parallel ranks (one process per GPU, RCCL)
               gemm_products=1,       # 1 = FP32 MFMA, 6 = split-operand mode
               parity_infer=False,    # True: scoring passes (Trainer.test = test.py:67-86) run their GEMMs with blocked accumulation.  Eval-mode plans gain
                                      # nothing measurable from it (1.851e-4 mm from the oracle either way, profiles/r05_parity_report.json) and pay ~3 %
               accum="auto",          # accumulation order of the training GEMMs: "auto" | "ordered" | "blocked" (TrainEngine)
               winograd=None,         # Winograd F(2x2, 3x3) forward of the stride-1 3x3 convolutions: None = the process-wide mode (awr_amd.set_conv_winograd,
                                      # $AWR_WINOGRAD), False / True (forward) / "full" (forward + data and weight gradients) = this run's own (the scoring pass takes the forward form),
                                      # "auto" = each engine times the modes on its own plan and keeps the fastest (logged at the first step)
               train_split_k=False,   # True: the training plan's small forward / data-gradient launches split their K loop, BatchNorm statistics from the reduce
                                      # kernel (TrainEngine(split_k=...)).  False = the process-wide mode (off unless $AWR_TRAIN_SPLIT_K).  Nothing else is accepted
               device_loader=True,    # NYU datasets built from this config keep their decoded frames in HBM and crop / augment / normalise on the
                                      # GPU (awr_amd.nyu_device: bit-identical to the host loader nyu_data.NYU, which False selects)
               device_eval=False,     # True: the train and test loops score joints on the GPU (evaluator.DeviceEvalUtil: no download of the predictions and
                                      # no sync per batch).  False = the host evaluator (EvalUtil), as the reference does it
               test_loss=False,       # True: Trainer.test also computes the validation loss of test.py:73-88 (coord_weight / dense_weight, the mean over the
                                      # batches of the per-batch mean) in the same pass over the dense map that decodes the joints, and logs it in a
                                      # second line (InferEngine(loss_weights=...)).  False = joints only
               accum_steps=1,         # k > 1: gradient accumulation -- k micro-batches of batch_size per optimiser step, each weighing 1/k; a window the epoch leaves
                                      # partly filled is applied at its end (TrainEngine(accum_steps=...), flush())
               clip_grad_norm=None,   # a finite number > 0: the optimiser applies torch's clip_grad_norm_ coefficient to the global gradient norm, measured and
                                      # applied on the device (TrainEngine(clip_grad_norm=...)); the print_freq lines gain [grad norm: ...].  None = no clipping
               log_grad_norm=False,   # True: measure the gradient norm without clipping and add [grad norm: ...] to the print_freq lines
               ema_decay=None,        # d in the open interval (0, 1), e.g. 0.999: an exponential moving average of the weights and BatchNorm statistics, kept on the
                                      # device behind every optimiser step (TrainEngine(ema_decay=...)), scored by Trainer.test in a second pass
                                      # ([test mpe ema ...]) and saved as "model_ema" / "ema_updates" next to "model".  None = no EMA, nothing changes
               ema_warmup=True,       # True: the decay of update t is min(ema_decay, (1 + t) / (10 + t)) (the TF / timm rule) | False: ema_decay from the first update.
                                      # Only read with ema_decay set
               load_ema=False,        # True: config.load_model's "model_ema" is loaded as THE network instead of "model" (test.py on the averaged weights, or a
                                      # run resumed from them); a checkpoint without that entry raises
               test_loss_stages="last")   # "last": the stage the training loss supervises (what the [train loss] lines report) | "all": the sum over the
                                      # Hourglass stacks, as test.py:74-80 adds them up.  Only read with test_loss = True


class Config(object):
    """Attribute bag.  Defaults live on the class (so the reference's idiom -- subclass or edit and override attributes --
    keeps working); keyword overrides are validated; dataset-derived entries (jt_num, step, max_epoch) follow `dataset`
    unless a subclass or an override sets them."""

    def __init__(self, **overrides):
        unknown = [k for k in overrides if not hasattr(type(self), k) and k not in _DERIVED]
        if unknown:
            raise AttributeError("unknown config entries: %s" % sorted(unknown))
        for k, v in overrides.items():
            setattr(self, k, v)
        if not isinstance(self.train_split_k, bool):
            raise ValueError("train_split_k is False or True, not %r" % (self.train_split_k,))
        if not isinstance(self.device_eval, bool):
            raise ValueError("device_eval is False or True, not %r" % (self.device_eval,))
        if not isinstance(self.test_loss, bool):
            raise ValueError("test_loss is False or True, not %r" % (self.test_loss,))
        if not (isinstance(self.test_loss_stages, str) and self.test_loss_stages in ("last", "all")):
            raise ValueError("test_loss_stages is \"last\" or \"all\", not %r" % (self.test_loss_stages,))
        if isinstance(self.accum_steps, bool) or not isinstance(self.accum_steps, int) or self.accum_steps < 1:
            raise ValueError("accum_steps is an int >= 1, not %r" % (self.accum_steps,))
        c = self.clip_grad_norm
        if c is not None and (isinstance(c, bool) or not isinstance(c, (int, float)) or not (0 < c < float("inf"))):
            raise ValueError("clip_grad_norm is None or a finite number > 0, not %r" % (c,))
        if not isinstance(self.log_grad_norm, bool):
            raise ValueError("log_grad_norm is False or True, not %r" % (self.log_grad_norm,))
        d = self.ema_decay
        if d is not None and (isinstance(d, bool) or not isinstance(d, (int, float)) or not (0 < d < 1)):
            raise ValueError("ema_decay is None or a number in the open interval (0, 1), not %r" % (d,))
        if not isinstance(self.ema_warmup, bool):
            raise ValueError("ema_warmup is False or True, not %r" % (self.ema_warmup,))
        if not isinstance(self.load_ema, bool):
            raise ValueError("load_ema is False or True, not %r" % (self.load_ema,))
        if self.dataset not in _DATASETS:
            raise ValueError("dataset must be one of %s" % sorted(_DATASETS))
        for k, v in zip(_DERIVED, _DATASETS[self.dataset]):
            if k not in overrides and not hasattr(type(self), k):
                setattr(self, k, v)


_DERIVED = ("jt_num", "step", "max_epoch")
for _table in (_RUN, _PATHS, _DATA, _MODEL, _OPTIM, _MI355X):
    for _k, _v in _table.items():
        setattr(Config, _k, _v)

opt = Config()
