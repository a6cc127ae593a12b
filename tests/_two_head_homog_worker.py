"""Child process of tests/test_gpu_semisupervised_homog.py: one data-parallel rank of the homogeneous two-headed fused step (ranks
SHARE cuda:0 and reduce through gloo, as tests/_ddp_worker.py does), or with world = 1 the single-rank full-batch step it is
compared with.  argv: rank world port out_path"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hydra-gnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

N_GRAPHS, STEPS = 9, 3


def graphs_with_masks():
    from hydra_gnn_amd import workloads

    rng = np.random.Generator(np.random.PCG64(78))
    graphs = [workloads.stanford_like_graph(rng) for _ in range(N_GRAPHS)]
    for g in graphs:  # per-node train split, fixed per graph (so every sharding sees the same rows)
        g.train_mask = torch.from_numpy(rng.random(int(g.y.numel())) < 0.6)
    graphs[0].train_mask[:] = False  # unequal counts across ranks
    return graphs


def main():
    rank, world, port, out_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from hydra_gnn_amd import parallel
    from hydra_gnn_amd.data import collate_homogeneous
    from hydra_gnn_amd.models import HomogeneousNetwork

    torch.cuda.set_device(0)
    torch.manual_seed(100 + rank)  # ranks start different: the step broadcasts rank 0's weights
    net = HomogeneousNetwork(6, output_dim_dict={"room": 15, "object": 35}, conv_block="GraphSAGE", hidden_dim=64, num_layers=3,
                             dropout=0.0).to("cuda:0")
    graphs = graphs_with_masks()
    mine = parallel.shard_graphs(N_GRAPHS, rank, world)
    batch = collate_homogeneous([graphs[i] for i in mine]).to("cuda:0")
    step = net.semisupervised_step(lr=0.002, weight_decay=0.001, use_graph=False, process_group=True if world > 1 else None)
    losses = []
    for _ in range(STEPS):
        step(batch)
        losses.append(step.loss())
    torch.cuda.synchronize()
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu()
    torch.save({"params": flat, "losses": losses, "steps": step.steps_taken()}, out_path)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
