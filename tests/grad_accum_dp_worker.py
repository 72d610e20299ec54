"""Worker of tests/test_grad_accum_dp_gpu.py: one rank of a 2-rank data-parallel TrainEngine run with gradient accumulation and clipping.
Both ranks share GPU 0 over gloo (see tests/dp_worker.py).  One accumulation window of two micro-steps per mode: "same" -- both ranks feed
the same shard; "split" -- every rank its own."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))


def main():
    rank, world, out = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), sys.argv[1]
    clip = float(sys.argv[2])
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    import awr_amd
    import awr_oracle as O
    from awr_amd.trainer import TrainEngine
    res = {}
    for mode in ("same", "split"):
        torch.manual_seed(1234 + rank)                   # different initial weights per rank: the broadcast must fix that
        net = awr_amd.get_deconv_net(18, 14, 2).cuda()
        eng = TrainEngine(net, 2, 128, 1.0, coord_weight=1.0, lr=1e-3, process_group=torch.distributed.group.WORLD, use_graph=False, autotune=False,
                          accum_steps=2, clip_grad_norm=clip)
        assert eng.dp and eng.world == world
        n = net.n_active
        start = net.flat_params()[:n].cpu()
        for s in range(2):
            img, jt = O.synth_batch(2, 128, 14, seed=70 + s + (0 if mode == "same" else 10 * (rank + 1)))
            eng.step(img.cuda(), jt.cuda())
            if s == 0:
                assert eng.micro_step == 1 and eng.step_count == 0 and torch.equal(net.flat_params()[:n].cpu(), start)
        assert eng.micro_step == 0 and eng.step_count == 1
        torch.cuda.synchronize()
        res[mode] = {"params": net.flat_params()[:n].cpu(), "m": eng.m[:n].cpu(), "v": eng.v[:n].cpu(), "buffers": net._barena.cpu(),
                     "grad_norm": eng.grad_norm.cpu(), "clip_scale": eng.clip_scale.cpu()}
    torch.save(res, "%s.rank%d" % (out, rank))
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
