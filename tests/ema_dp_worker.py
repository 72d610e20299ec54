"""Worker of tests/test_ema_dp_gpu.py: one rank of a 2-rank data-parallel TrainEngine run with a weight EMA.  Both ranks share GPU 0 over gloo
(see tests/dp_worker.py).  Two steps per mode: "same" -- both ranks feed the same shard; "split" -- every rank its own."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))


def main():
    rank, world, out = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), sys.argv[1]
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    import awr_amd
    import awr_oracle as O
    from awr_amd.trainer import TrainEngine
    res = {}
    for mode in ("same", "split"):
        torch.manual_seed(1234 + rank)                   # different initial weights per rank: the shadow must be cloned behind the broadcast
        net = awr_amd.get_deconv_net(18, 14, 2).cuda()
        eng = TrainEngine(net, 2, 128, 1.0, coord_weight=1.0, lr=1e-3, process_group=torch.distributed.group.WORLD, use_graph=False, autotune=False,
                          ema_decay=0.5)
        assert eng.dp and eng.world == world
        assert torch.equal(eng.ema_net.flat_params(), net.flat_params()) and torch.equal(eng.ema_net._barena, net._barena)
        for s in range(2):
            img, jt = O.synth_batch(2, 128, 14, seed=70 + s + (0 if mode == "same" else 10 * (rank + 1)))
            eng.step(img.cuda(), jt.cuda())
        assert eng.ema_updates == 2 and eng.step_count == 2
        torch.cuda.synchronize()
        res[mode] = {"params": net.flat_params().cpu(), "buffers": net._barena.cpu(), "ema_params": eng.ema_net.flat_params().cpu(),
                     "ema_buffers": eng.ema_net._barena.cpu()}
    torch.save(res, "%s.rank%d" % (out, rank))
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
