"""Batch-1 latency of the inference hot loop (bin/room_classification_server:283-287).

  a) the reference's expression on this engine:  model(data).argmax(dim=1).cpu()   under torch.no_grad()
  b) model.predict(data): native eval forward + hmp_argmax_rows + one pinned D2H of the labels
  c) the step in front of the model call, GnnModel.convert_graph: the existing stages of hydra_gnn_amd/dsg.py and htree.py next to
     dsg.FramePipeline.convert, median and p90 of ``--reps`` calls (default 200); ``--convert-loop N`` runs only N converts per
     pipeline, for a kernel trace (``--convert-loop N --homogeneous``: of the two homogeneous pipelines)
  d) ``--homogeneous-legs``: only the input of the HOMOGENEOUS models (HomogeneousNetwork / HomogeneousNeuralTreeNetwork), three
     ways in alternation (plus the typed convert alone, for scale): the host conversion + ``data.heterogeneous_*_to_homogeneous`` + one ``.to(device)``; the typed pipeline
     brought back to the host for the same conversion; ``FramePipeline(homogeneous=True).convert``.  The first two use only
     interfaces older than the third, which is skipped where the package does not have it

One MP3D-like scene graph per call (a fresh graph object every call, as the server receives a new frame), 306-d objects,
3-layer SAGE hidden 64 and the shipped GAT shape (3 layers, 3 heads, hidden 64, concat False).  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, "hydra-gnn_amd")
from hydra_gnn_amd import dsg, htree, workloads  # noqa: E402
from hydra_gnn_amd.data import heterogeneous_data_to_homogeneous, heterogeneous_htree_to_homogeneous  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402

DEV = "cuda:0"


def timed(fn, frames, reps):
    for f in frames[:8]:
        fn(f)
    torch.cuda.synchronize()
    ts = []
    for r in range(reps):
        f = frames[r % len(frames)]
        t0 = time.perf_counter_ns()
        fn(f)
        ts.append((time.perf_counter_ns() - t0) * 1e-3)
    ts = np.array(ts)
    return {"median_us": round(float(np.median(ts)), 1), "p90_us": round(float(np.percentile(ts, 90)), 1)}


def main():
    torch.manual_seed(0)
    frames = [workloads.mp3d_like_batch(1, 100 + i).to(DEV) for i in range(32)]
    out = {"frames": len(frames), "objects_median": int(np.median([f["objects"].x.size(0) for f in frames]))}
    nets = {
        "sage_h64_l3": dict(conv_block="GraphSAGE", hidden_dim=64, num_layers=3),
        "gat_h64x3_l3": dict(conv_block="GAT", GAT_hidden_dims=[64, 64], GAT_heads=[3, 3, 3], GAT_concats=[False, False, False]),
    }
    for name, kw in nets.items():
        net = HeterogeneousNetwork(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, dropout=0.25, **kw).to(DEV).eval()

        def ref_expr(f):
            with torch.no_grad():
                return net(f).argmax(dim=1).cpu()

        a = timed(ref_expr, frames, 400)
        b = timed(net.predict, frames, 400)
        for f in frames[:4]:
            assert torch.equal(ref_expr(f), net.predict(f))
        out[name] = {"forward_argmax_cpu": a, "predict": b}
    # ---- the step before the model: scene graph -> HeteroData (hydra_gnn_amd/dsg.py), on the reference's test graph and on a
    # 300-object synthetic frame: the existing stages (Python loops + torch glue, three launches and a read-back for the object
    # edges, the H-tree through generate_htree) next to dsg.FramePipeline.convert (one host stage, one copy, one launch)
    out["dsg_frame_62_objects"] = frame_stages(dsg.load_dsg_json(json.load(open(FIXTURE))), nets["sage_h64_l3"], raw=json.load(open(FIXTURE)))
    if hasattr(workloads, "synthetic_scene"):
        out["dsg_frame_300_objects"] = frame_stages(scene_graph(workloads.synthetic_scene(300, 3, seed=1)), nets["sage_h64_l3"])
    print(json.dumps(out))


FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "dsg_x8F5xyUWy9e.json")
REPS = 200


def scene_graph(arrays):
    """dsg.SceneGraph of flat arrays (ids, layer, pos, bb_min, bb_max, label, edges as node ids)"""
    ids, layer, pos, bb_min, bb_max, label, edges = arrays
    index = {int(v): i for i, v in enumerate(ids)}
    adj = [set() for _ in ids]
    for a, b in zip(edges[0].tolist(), edges[1].tolist()):
        a, b = index[a], index[b]
        adj[a].add(b)
        adj[b].add(a)
    return dsg.SceneGraph(ids, layer.astype(np.int64), pos, bb_min, bb_max, label, adj)


def flat_arrays(sg):
    if hasattr(dsg, "scene_arrays"):
        return dsg.scene_arrays(sg)
    pairs = np.array([(i, j) for i, nb in enumerate(sg.adj) for j in nb if i < j], dtype=np.int64).reshape(-1, 2).T
    return sg.ids, sg.layer, sg.pos, sg.bb_min, sg.bb_max, sg.label, sg.ids[pairs]


def frame_stages(sg, sage_kw, raw=None):
    """median and p90 over REPS calls of every stage, each call timed to completion (host call + torch.cuda.synchronize())"""
    net6 = HeterogeneousNetwork(input_dim_dict={"objects": 6, "rooms": 6}, output_dim=26, dropout=0.25, **sage_kw).to(DEV).eval()
    stages = {}

    def stage(name, fn, reps=REPS):
        for _ in range(5):
            r = fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter_ns()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter_ns() - t0) * 1e-3)
        stages[name + "_us"] = round(float(np.median(ts)), 1)
        stages[name + "_p90_us"] = round(float(np.percentile(ts, 90)), 1)
        return r

    if raw is not None:  # the JSON step in front of everything (host only)
        stage("parse_static_layers", lambda: dsg.load_dsg_json(raw))
    rog = stage("room_object_graph", lambda: dsg.RoomObjectGraph(sg))
    oo = stage("object_connectivity_hip", lambda: dsg.object_connectivity(rog, 1.5, 2.0, 0.2, DEV))
    data = stage("to_hetero_data", lambda: dsg.to_hetero_data(rog, oo, None, DEV))
    stage("predict", lambda: net6.predict(data))
    stage("generate_htree", lambda: htree.generate_htree(data, clique_dim=6))
    stages["objects"], stages["object_edges"] = int(rog.objects.size), int(oo.size(1))
    if hasattr(dsg, "FramePipeline"):
        flat = flat_arrays(sg)
        pipe, pipe_h = dsg.FramePipeline(DEV), dsg.FramePipeline(DEV, htree=True, clique_dim=6)
        stage("scene_arrays", lambda: flat_arrays(sg))
        frame, _ = stage("pipeline_convert", lambda: pipe.convert(*flat))
        stage("pipeline_convert_htree", lambda: pipe_h.convert(*flat))
        assert torch.equal(net6.predict(frame).clone(), net6.predict(data))
    return stages


def to_homogeneous(frame, htree_mode):
    """the host conversion of a typed frame on the CPU (Hydra_mp3d_data.to_homogeneous / heterogeneous_htree_to_homogeneous)"""
    if htree_mode:
        return heterogeneous_htree_to_homogeneous(frame)
    d, types = heterogeneous_data_to_homogeneous(frame)
    d.room_mask = d.node_type == types.index("rooms")
    return d


def has_homogeneous_pipeline():
    import inspect

    return hasattr(dsg, "FramePipeline") and "homogeneous" in inspect.signature(dsg.FramePipeline.__init__).parameters


def homogeneous_legs(sg, reps, htree_reps):
    """The homogeneous models' input, each call timed to completion, the legs alternating call by call (one session, so drift hits
    all of them alike): median and p90 in us per leg, for the baseline frame and for its H-tree"""
    flat = flat_arrays(sg)
    out = {}
    for htree_mode in (False, True):
        kw = dict(htree=True, clique_dim=6) if htree_mode else {}
        typed = dsg.FramePipeline(DEV, **kw)

        def host_route():  # everything on the host, then one .to(device) of the Data
            rog = dsg.RoomObjectGraph(sg)
            oo = torch.from_numpy(dsg.frame_host_stage(*flat)["oo_edges"].astype(np.int64))  # the native predicates, host memory only
            frame = dsg.to_hetero_data(rog, oo, None, "cpu")
            if htree_mode:
                frame = htree.generate_htree(frame, clique_dim=6)
            return to_homogeneous(frame, htree_mode).to(DEV)

        def roundtrip_route():  # the typed pipeline, back to the host for the conversion, up again
            return to_homogeneous(typed.convert(*flat)[0].to("cpu"), htree_mode).to(DEV)

        # the typed convert on its own: not a way to the homogeneous Data, only the scale of the two pipeline legs
        legs = {"host_to_homogeneous": host_route, "typed_pipeline_roundtrip": roundtrip_route,
                "typed_pipeline_convert": lambda: typed.convert(*flat)[0]}
        if has_homogeneous_pipeline():
            pipe = dsg.FramePipeline(DEV, homogeneous=True, **kw)
            legs["pipeline_convert_homogeneous"] = lambda: pipe.convert(*flat)[0]
        results = {}
        for name, fn in legs.items():
            for _ in range(3):
                results[name] = fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in legs}
        n = htree_reps if htree_mode else reps
        for _ in range(n):
            for name, fn in legs.items():
                t0 = time.perf_counter_ns()
                fn()
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter_ns() - t0) * 1e-3)
        if "pipeline_convert_homogeneous" in legs and not htree_mode:  # the three legs made the same Data
            want = vars(results["typed_pipeline_roundtrip"])
            got = vars(legs["pipeline_convert_homogeneous"]())
            assert all(torch.equal(got[k], want[k]) for k in want if k != "_plan_cache")
        tag = "htree" if htree_mode else "baseline"
        for name, t in ts.items():
            out[f"{tag}_{name}_us"] = round(float(np.median(t)), 1)
            out[f"{tag}_{name}_p90_us"] = round(float(np.percentile(t, 90)), 1)
        out[f"{tag}_reps"] = n
    return out


def homogeneous_main(reps):
    out = {"homogeneous_legs": True, "has_homogeneous_pipeline": has_homogeneous_pipeline()}
    out["dsg_frame_62_objects"] = homogeneous_legs(dsg.load_dsg_json(json.load(open(FIXTURE))), reps, max(5, reps // 4))
    big = scene_graph(workloads.synthetic_scene(300, 3, seed=1))
    out["dsg_frame_300_objects"] = homogeneous_legs(big, reps, max(5, reps // 20))  # its H-tree: 0.45 s per call and leg
    print(json.dumps(out))


def convert_loop(n, homogeneous=False):
    """only the pipeline's convert calls (baseline, then H-tree), for a kernel trace of the conversion on its own"""
    flat = flat_arrays(dsg.load_dsg_json(json.load(open(FIXTURE))))
    kw = dict(homogeneous=True) if homogeneous else {}
    for pipe in (dsg.FramePipeline(DEV, **kw), dsg.FramePipeline(DEV, htree=True, clique_dim=6, **kw)):
        for _ in range(n):
            pipe.convert(*flat)
    torch.cuda.synchronize()
    print(json.dumps({"convert_loop": n, "pipelines": 2, "homogeneous": homogeneous}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--convert-loop":
        convert_loop(int(sys.argv[2]), homogeneous="--homogeneous" in sys.argv[3:])
    elif len(sys.argv) > 1 and sys.argv[1] == "--homogeneous-legs":  # [--reps N]
        homogeneous_main(int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[2] == "--reps" else REPS)
    else:
        if len(sys.argv) > 2 and sys.argv[1] == "--reps":  # the H-tree of the 300-object frame takes 0.45 s per call
            REPS = int(sys.argv[2])
        main()
