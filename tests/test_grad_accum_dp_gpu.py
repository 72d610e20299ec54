"""GPU: gradient accumulation and clipping in the data-parallel TrainEngine, TWO real ranks on GPU 0 over gloo (tests/grad_accum_dp_worker.py;
with this process three hold the GPU).  Every micro-step is all-reduced, the norm is measured behind the all-reduce waits: replicas stay bitwise
equal and agree on the norm to the bit."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, clip):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = os.path.join(str(tmp_path), "dp")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), AWR_DETERMINISTIC="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "grad_accum_dp_worker.py"), out, repr(clip)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:          # a worker that outlived its time limit (or its peer's failure) is not left behind
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, lg in zip(procs, logs):
        assert p.returncode == 0, lg[-3000:]
    return [torch.load("%s.rank%d" % (out, r)) for r in range(2)]


def _single(awr_amd, O, **kw):
    """one window of two micro-steps in this process, from rank 0's initial weights"""
    from awr_amd.trainer import TrainEngine
    torch.manual_seed(1234)
    net = awr_amd.get_deconv_net(18, 14, 2).cuda()
    eng = TrainEngine(net, 2, 128, 1.0, coord_weight=1.0, lr=1e-3, use_graph=False, autotune=False, accum_steps=2, **kw)
    for s in range(2):
        img, jt = O.synth_batch(2, 128, 14, seed=70 + s)
        eng.step(img.cuda(), jt.cuda())
    torch.cuda.synchronize()
    n = net.n_active
    return {"params": net.flat_params()[:n].cpu(), "m": eng.m[:n].cpu(), "v": eng.v[:n].cpu(), "buffers": net._barena.cpu(),
            "grad_norm": eng.grad_norm.cpu(), "clip_scale": eng.clip_scale.cpu()}


@pytest.mark.timeout(1200)
def test_two_rank_accumulation_window_with_clipping(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import awr_amd
    import awr_oracle as O
    awr_amd.set_deterministic(True)                  # the workers run with AWR_DETERMINISTIC=1: the single-process window must match them bitwise
    try:
        norm = float(_single(awr_amd, O, grad_norm=True)["grad_norm"])
        assert norm > 0 and norm == norm
        clip = 0.5 * norm                            # below the observed norm: the window is clipped
        ref = _single(awr_amd, O, clip_grad_norm=clip)
    finally:
        awr_amd.set_deterministic(False)
    assert 0.0 < float(ref["clip_scale"]) < 1.0
    r0, r1 = _run(tmp_path, clip)
    for mode in ("same", "split"):                   # replicas: equal parameters and optimiser state, the same norm and coefficient to the bit
        a, b = r0[mode], r1[mode]
        for k in ("params", "m", "v"):
            assert torch.equal(a[k], b[k]), (mode, k)
        assert torch.equal(a["grad_norm"].view(torch.int64), b["grad_norm"].view(torch.int64)), mode
        assert torch.equal(a["clip_scale"].view(torch.int32), b["clip_scale"].view(torch.int32)), mode
    # both ranks fed the same shard: (g + g) / 2 == g exactly in every micro-step, so the window IS the single-process window, bit for bit
    for k in ("params", "m", "v", "buffers"):
        assert torch.equal(r0["same"][k], ref[k]), k
    assert torch.equal(r0["same"]["grad_norm"].view(torch.int64), ref["grad_norm"].view(torch.int64))
    assert torch.equal(r0["same"]["clip_scale"].view(torch.int32), ref["clip_scale"].view(torch.int32))
    assert not torch.equal(r0["split"]["params"], r0["same"]["params"])
    assert not torch.equal(r0["split"]["buffers"], r1["split"]["buffers"])      # BatchNorm statistics stay rank-local
