"""GPU: the weight EMA in the data-parallel TrainEngine, TWO real ranks on GPU 0 over gloo (tests/ema_dp_worker.py; with this process three
hold the GPU).  Equal parameters go through an equal schedule: the EMA parameters are bitwise equal on every rank; the EMA buffers average
rank-local BatchNorm statistics and stay rank-local."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = os.path.join(str(tmp_path), "dp")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), AWR_DETERMINISTIC="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "ema_dp_worker.py"), out], env=env,
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


def _single(awr_amd, O):
    """the same two steps in this process, from rank 0's initial weights"""
    from awr_amd.trainer import TrainEngine
    torch.manual_seed(1234)
    net = awr_amd.get_deconv_net(18, 14, 2).cuda()
    eng = TrainEngine(net, 2, 128, 1.0, coord_weight=1.0, lr=1e-3, use_graph=False, autotune=False, ema_decay=0.5)
    for s in range(2):
        img, jt = O.synth_batch(2, 128, 14, seed=70 + s)
        eng.step(img.cuda(), jt.cuda())
    torch.cuda.synchronize()
    return {"params": net.flat_params().cpu(), "buffers": net._barena.cpu(), "ema_params": eng.ema_net.flat_params().cpu(),
            "ema_buffers": eng.ema_net._barena.cpu()}


@pytest.mark.timeout(1200)
def test_two_rank_ema(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import awr_amd
    import awr_oracle as O
    awr_amd.set_deterministic(True)                  # the workers run with AWR_DETERMINISTIC=1: the single-process run must match them bitwise
    try:
        ref = _single(awr_amd, O)
    finally:
        awr_amd.set_deterministic(False)
    r0, r1 = _run(tmp_path)
    for mode in ("same", "split"):                   # replicas: equal parameters, so equal EMA parameters, to the bit
        assert torch.equal(r0[mode]["params"], r1[mode]["params"]), mode
        assert torch.equal(r0[mode]["ema_params"], r1[mode]["ema_params"]), mode
        assert not torch.equal(r0[mode]["ema_params"], r0[mode]["params"]), mode
    # different shards: BatchNorm statistics are rank-local, and so is their average
    assert not torch.equal(r0["split"]["buffers"], r1["split"]["buffers"])
    assert not torch.equal(r0["split"]["ema_buffers"], r1["split"]["ema_buffers"])
    # both ranks fed the same shard: (g + g) / 2 == g exactly, so the run IS the single-process run, bit for bit -- and so is its EMA
    for k in ("params", "buffers", "ema_params", "ema_buffers"):
        assert torch.equal(r0["same"][k], ref[k]), k
        assert torch.equal(r1["same"][k], ref[k]), k
    assert not torch.equal(r0["split"]["ema_params"], r0["same"]["ema_params"])
