#!/usr/bin/env python3
"""In-kernel phase times of grad_reduce_kernel in the config-2 training step (profiling build: make -C hydra-gnn_amd/csrc KTIME=1).

    HMP_LIB=hydra-gnn_amd/hydra_gnn_amd/libhydra_mp_kt.so python tools/ktime_grad.py

Stamps of thread 0 (csrc/optim.hip, GKT): [0] entry, [1] segment known, [2] descriptor complete (first slab address computed),
[3] all loads back, [4] stores issued.  Workgroup 0 stamps slots 0..4, the selected workgroup slots 8..12; the kernel notes the
first workgroup of a 16-slab and of an 8-slab segment in slots 20 / 21, and this script selects them in turn.  Prints the
median and the range over N steps of every interval, in microseconds (100 MHz wall clock: 0.01 us per tick).
"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hydra-gnn_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402

NAMES = ["entry->segment", "segment->descriptor", "descriptor->loads back", "loads back->stores", "entry->stores"]
BIG = 1 << 62


def main():
    n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = HeterogeneousNetwork(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64,
                               num_layers=3, dropout=0.25).to(dev)
    net.train()
    batch = workloads.config2_batch(32).to(dev)
    y = batch["rooms"].y
    step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, use_graph=False)
    lib = _lib.load()
    buf_t = C.c_ulonglong * 64
    for name in ("hmp_debug_ktime_optim", "hmp_debug_ktime_optim_set"):
        getattr(lib, name).argtypes = [C.POINTER(C.c_ulonglong)]
        getattr(lib, name).restype = C.c_int
    lib.hmp_debug_ktime_optim_select.argtypes = [C.c_int]
    lib.hmp_debug_ktime_optim_select.restype = C.c_int

    def read():
        buf = buf_t()
        assert lib.hmp_debug_ktime_optim(buf) == 0
        return list(buf)

    preset = buf_t()
    preset[20] = preset[21] = BIG
    assert lib.hmp_debug_ktime_optim_set(preset) == 0
    for _ in range(20):
        step(batch, y)
    torch.cuda.synchronize()
    v = read()
    blk16, blk8 = v[20], v[21]
    print(f"first workgroup of a 16-slab segment: {blk16 if blk16 < BIG else None}, of an 8-slab segment past 0: {blk8 if blk8 < BIG else None}")

    def sample(base):
        rows = []
        for _ in range(n_steps):
            step(batch, y)
            torch.cuda.synchronize()
            t = read()[base:base + 5]
            rows.append([(t[1] - t[0]) / 100.0, (t[2] - t[1]) / 100.0, (t[3] - t[2]) / 100.0, (t[4] - t[3]) / 100.0, (t[4] - t[0]) / 100.0])
        return rows

    def show(title, rows):
        print(title)
        for k, name in enumerate(NAMES):
            col = [r[k] for r in rows]
            print(f"  {name:26s} median {statistics.median(col):6.2f} us   range {min(col):6.2f} .. {max(col):6.2f}")

    show("workgroup 0", sample(0))
    for tag, blk in (("16-slab", blk16), ("8-slab", blk8)):
        if blk >= BIG:
            continue
        assert lib.hmp_debug_ktime_optim_select(int(blk)) == 0
        step(batch, y)
        torch.cuda.synchronize()
        show(f"workgroup {blk} (first of a {tag} segment)", sample(8))


if __name__ == "__main__":
    main()
