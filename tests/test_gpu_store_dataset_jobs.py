"""The training jobs over resident stores: ``jobs.SemiSupervisedTrainingJob(StoreDataset(store, ...))`` after
``generate_node_split`` and ``jobs.BaseTrainingJob`` over three ``StoreDataset``s against the same jobs over host list datasets (the
stand-ins of ``tests/test_gpu_training_job.py``), whose masks the restated reference split set.  Same seeds, same kernels, same bytes:
the per-epoch losses, the results and the final state are bit-equal."""
import struct

import numpy as np
import pytest
import torch

import _node_split_reference as nsr
import _store_derive_cases as sc
from hydra_gnn_amd import _lib, jobs
from hydra_gnn_amd.store import GraphStore, StoreDataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 8
OPT = {"lr": 0.004, "weight_decay": 0.001, "batch_size": B, "shuffle": True, "num_epochs": 3}
TRAIN_KW = dict(decay_epochs=2, decay_rate=0.5, min_log_epoch=1)
FEATURES = {"objects": sc.OBJ_W, "rooms": sc.ROOM_W}
PARAMS = dict(conv_block="GraphSAGE", hidden_dim=16, num_layers=2)


class _Info:
    def __init__(self, features, rooms, objects):
        self._f, self._r, self._o = features, rooms, objects

    def num_node_features(self):
        return self._f

    def num_room_labels(self):
        return self._r

    def num_object_labels(self):
        return self._o


class GraphDataset:
    """a host list dataset as the jobs read one (tests/test_gpu_training_job.py)"""

    def __init__(self, data_type, graphs, features, rooms, objects=None):
        self._type, self.graphs, self._info = data_type, list(graphs), _Info(features, rooms, objects)

    def data_type(self):
        return self._type

    def __len__(self):
        return len(self.graphs)

    def __getitem__(self, i):
        return self.graphs[i]

    def get_data(self, i):
        return self._info


def graphs(n, seed):
    """typed baseline graphs whose labels are a function of a feature (two of the 15 classes): random labels would often leave a
    short run without any validation improvement, and such a run has no best state"""
    rng = np.random.default_rng(seed)
    gs = sc.baseline_graphs(True, counts=[(int(rng.integers(3, 9)), int(rng.integers(1, 4))) for _ in range(n)], seed=seed, ro_edges=True)
    for g in gs:
        for t in ("objects", "rooms"):
            g[t].y = (g[t].x[:, 3] > 0).to(torch.int64)
    return gs


def bits(values):
    return [struct.pack("<d", float(v)).hex() for v in values]


def check_equal(got, want):
    (net_a, res_a, info_a), (net_b, res_b, info_b) = got, want
    assert info_a["num_epochs"] == info_b["num_epochs"] == OPT["num_epochs"]
    assert bits(info_a["loss"]) == bits(info_b["loss"]) and all(np.isfinite(info_a["loss"]))
    assert info_a["validation_result"] == info_b["validation_result"] and info_a["best_epoch"] == info_b["best_epoch"]
    assert isinstance(res_a, tuple) and len(res_a) == 2 and bits(res_a) == bits(res_b)
    sa, sb = net_a.state_dict(), net_b.state_dict()
    assert list(sa) == list(sb)
    for k in sb:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


def test_semisupervised_job_over_a_store_dataset(tmp_path):
    gs = graphs(24, 3)
    store = GraphStore(gs, DEV)
    ds = StoreDataset(store, "heterogeneous", dict(FEATURES), 15, 15)
    assert len(ds) == 24
    ds.generate_node_split(0.7, 0.1, 0.2, seed=1)
    host = [sc.clone(g) for g in gs]
    nsr.generate_node_split(host, "heterogeneous", 0.7, 0.1, 0.2, seed=1)
    outs = []
    for dataset in (ds, GraphDataset("heterogeneous", host, dict(FEATURES), 15, 15)):
        torch.manual_seed(4)
        job = jobs.SemiSupervisedTrainingJob(dataset, dict(PARAMS))
        torch.manual_seed(18)
        outs.append(job.train(str(tmp_path), dict(OPT), **TRAIN_KW))
        if dataset is ds:
            assert job._store("all", ds, torch.device(DEV)) is store  # the resident store itself, no copy
    check_equal(*outs)


def test_room_job_over_three_store_datasets(tmp_path):
    split = {"train": graphs(24, 5), "val": graphs(8, 6), "test": graphs(8, 7)}
    resident = {s: StoreDataset(GraphStore(g, DEV), "heterogeneous", dict(FEATURES), 15) for s, g in split.items()}
    host = {s: GraphDataset("heterogeneous", g, dict(FEATURES), 15) for s, g in split.items()}
    outs = []
    for dd in (resident, host):
        torch.manual_seed(3)
        job = jobs.BaseTrainingJob(dd, dict(PARAMS))
        torch.manual_seed(17)
        outs.append(job.train(str(tmp_path), dict(OPT), **TRAIN_KW))
        assert bits([job.test("test")]) == bits([outs[-1][1][1]])
    check_equal(*outs)


def test_a_store_on_another_device_is_refused():
    ds = StoreDataset(GraphStore(graphs(2, 1), DEV), "heterogeneous", dict(FEATURES), 15)
    torch.manual_seed(0)
    job = jobs.BaseTrainingJob({"train": ds, "val": ds, "test": ds}, dict(PARAMS))
    with pytest.raises(_lib.HydraMPError, match="the job runs on"):
        job._store("train", ds, torch.device("cuda:1"))
