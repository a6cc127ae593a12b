#!/usr/bin/env python3
"""Many scene graphs per request: ``dsg.FramePipeline.convert_batch`` against the single-frame path, and
``store.GraphStore.from_frames`` against ``GraphStore(list)``, on one MI355X.

For K in ``--ks`` (default 1,8,32,64) frames of the size of the reference's test graph (the fixture, 62 kept objects and 5 rooms,
K times) and for the typed baseline and the typed H-tree pipeline, these legs alternate call by call inside one process:

  single_path        K x (``convert`` + a copy of the result, which is valid only until the next ``convert``) + ``data.collate`` +
                     ``.to(device)``: the only way from K frames to a collated batch without ``convert_batch``.  ``data.collate``
                     is host code, so the copy is ``.to("cpu")``
  convert_only       K x ``convert`` and nothing else: the single-frame path per frame, for scale
  convert_batch      ``convert_batch`` of the K frames
  store_list         K x (``convert`` + copy) + ``GraphStore(list)``
  store_from_frames  ``GraphStore.from_frames``

Every call is timed to completion (host call + ``torch.cuda.synchronize()``); a figure is the median in microseconds of ``--reps``
calls after ``--warmup`` calls, with the p90 next to it, and ``per_frame_us`` = median / K.  The first two legs and ``store_list``
use no interface this tool's commit adds: ``--package-root DIR`` imports ``hydra_gnn_amd`` from another checkout (one that was
built), where the other legs are skipped if the package lacks them.  Prints one JSON line per (mode, K); ``--out FILE`` appends
them.  A measurement needs the GPU: without one the tool fails.

``--convert-loop N``: only N ``convert_batch`` calls of K = 32 per pipeline, for a kernel trace.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,32,64")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--package-root", default=ROOT, help="checkout whose hydra_gnn_amd is measured")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--out")
    ap.add_argument("--convert-loop", type=int, default=0)
    a = ap.parse_args()
    sys.path[:0] = [a.package_root, os.path.join(a.package_root, "hydra-gnn_amd")]
    import numpy as np
    import torch

    from hydra_gnn_amd import _lib, data, dsg
    from hydra_gnn_amd.store import GraphStore

    _lib.require_device()
    dev = "cuda:0"
    arrays = dsg.scene_arrays(dsg.load_dsg_json(os.path.join(ROOT, "tests", "golden", "dsg_x8F5xyUWy9e.json")))
    y = (np.arange(arrays[0].size, dtype=np.int64) * 7) % 26
    modes = {"typed_baseline": dict(), "typed_htree": dict(htree=True, clique_dim=6)}
    has_batch = hasattr(dsg.FramePipeline, "convert_batch")

    if a.convert_loop:
        for kw in modes.values():
            pipe = dsg.FramePipeline(dev, **kw)
            for _ in range(a.convert_loop):
                pipe.convert_batch([arrays] * 32)
        torch.cuda.synchronize()
        return

    def copies(pipe, k):
        return [pipe.convert(*arrays)[0].to("cpu") for _ in range(k)]

    for mode, kw in modes.items():
        pipe = dsg.FramePipeline(dev, **kw)
        for k in [int(v) for v in a.ks.split(",")]:
            frames, ys = [arrays] * k, [y] * k
            legs = {"single_path": lambda: data.collate(copies(pipe, k)).to(dev),
                    "convert_only": lambda: [pipe.convert(*arrays) for _ in range(k)],
                    "store_list": lambda: GraphStore(copies(pipe, k), dev)}
            if has_batch:
                legs["convert_batch"] = lambda: pipe.convert_batch(frames)
                legs["store_from_frames"] = lambda: GraphStore.from_frames(pipe, frames)
            times = {name: [] for name in legs}
            for it in range(a.warmup + a.reps):
                for name, fn in legs.items():  # the legs alternate call by call
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        times[name].append((time.perf_counter() - t0) * 1e6)
            rec = {"tool": "frame_batch_latency", "tag": a.tag, "mode": mode, "k": k, "reps": a.reps, "legs": {}}
            for name, v in times.items():
                med, p90 = float(np.median(v)), float(np.percentile(v, 90))
                rec["legs"][name] = {"median_us": round(med, 1), "p90_us": round(p90, 1), "per_frame_us": round(med / k, 1)}
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
