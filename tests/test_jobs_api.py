"""CPU checks of hydra_gnn_amd.jobs: the model class a job builds from ``data_type()``, the reference's parameter cleaning, the
training order (a torch DataLoader over the indices, the only consumer of the global generator) and the refusal to train without
a device."""
import pytest
import torch
from torch.utils.data import DataLoader

from hydra_gnn_amd import _lib, jobs, workloads
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,
                                  HomogeneousNeuralTreeNetwork)

HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}


class _Info:
    def __init__(self, features, rooms=26, objects=28):
        self._f, self._r, self._o = features, rooms, objects

    def num_node_features(self):
        return self._f

    def num_room_labels(self):
        return self._r

    def num_object_labels(self):
        return self._o


class _Dataset:
    """what the jobs read of a reference dataset: data_type(), len, [i] -> torch data, get_data(i) -> the dimension queries"""

    def __init__(self, data_type, features, graphs=()):
        self._type, self._info, self._graphs = data_type, _Info(features), list(graphs)

    def data_type(self):
        return self._type

    def __len__(self):
        return len(self._graphs)

    def __getitem__(self, i):
        return self._graphs[i]

    def get_data(self, i):
        return self._info


CASES = [("homogeneous", 6, HomogeneousNetwork), ("heterogeneous", {"objects": 306, "rooms": 6}, HeterogeneousNetwork),
         ("homogeneous_htree", 6, HomogeneousNeuralTreeNetwork), ("heterogeneous_htree", HT_DIMS, HeterogeneousNeuralTreeNetwork)]


@pytest.mark.parametrize("data_type,features,cls", CASES)
def test_job_builds_the_model_class_of_the_data_type(data_type, features, cls):
    ds = _Dataset(data_type, features)
    job = jobs.BaseTrainingJob({"train": ds, "val": ds, "test": ds}, {"conv_block": "GraphSAGE", "hidden_dim": 16, "num_layers": 2})
    assert type(job._net) is cls
    assert job._net.classification_task == "room"
    assert job.train_job_type() == " ".join([data_type.split("_")[0], "neural_tree" if "htree" in data_type else "baseline"])
    assert job.ignored_label() == 25 and job.get_dataset("val") is ds
    assert job.get_network_params()["output_dim"] == 26
    semi = jobs.SemiSupervisedTrainingJob(ds, {"conv_block": "GraphSAGE", "hidden_dim": 16, "num_layers": 2})
    assert type(semi._net) is cls and semi._net.classification_task == "all"
    want = {"rooms": 26, "objects": 28} if "htree" not in data_type else {"room": 26, "object": 28, "object-room": 1, "room-room": 1}
    assert semi.get_network_params()["output_dim_dict"] == want


def test_parameter_cleaning_follows_the_conv_block():
    ds = _Dataset("heterogeneous", {"objects": 306, "rooms": 6})
    dd = {"train": ds, "val": ds, "test": ds}
    sage = jobs.BaseTrainingJob(dd, {"conv_block": "GraphSAGE", "hidden_dim": 16, "num_layers": 2}).get_network_params()
    assert not {"GAT_hidden_dims", "GAT_heads", "GAT_concats"} & set(sage) and sage["num_layers"] == 2 and sage["hidden_dim"] == 16
    gat = jobs.BaseTrainingJob(dd, {"conv_block": "GAT_edge", "GAT_hidden_dims": [8], "GAT_heads": [2, 2],
                                    "GAT_concats": [True, False]}).get_network_params()
    assert "num_layers" not in gat and "hidden_dim" not in gat and gat["GAT_heads"] == [2, 2]
    defaults = jobs.BaseTrainingJob.create_default_params()
    assert defaults["optimization_params"] == {"lr": 0.01, "num_epochs": 200, "weight_decay": 0.001, "batch_size": 64, "shuffle": True}
    assert defaults["network_params"]["ignored_label"] == 25 and defaults["network_params"]["conv_block"] == "GraphSAGE"


@pytest.mark.parametrize("n,B", [(50, 16), (7, 8)])
@pytest.mark.parametrize("seed", [0, 12345])
def test_training_order_is_a_torch_dataloader_over_the_indices(n, B, seed):
    torch.manual_seed(seed)
    want = [[[int(i) for i in batch] for batch in DataLoader(range(n), batch_size=B, shuffle=True)] for _ in range(3)]
    after_want = torch.rand(1)
    torch.manual_seed(seed)
    loader = jobs.order_loader(n, B, True)
    got = [[list(ids) for ids in loader] for _ in range(3)]
    assert got == want
    assert all(isinstance(i, int) for epoch in got for ids in epoch for i in ids)
    assert torch.equal(torch.rand(1), after_want), "the order loader consumed the global generator differently"
    assert [sorted(i for ids in e for i in ids) for e in got] == [list(range(n))] * 3
    assert [list(ids) for ids in jobs.order_loader(n, B, False)] == jobs.id_chunks(n, B)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_train_without_a_device_raises(tmp_path):
    import numpy as np

    rng = np.random.default_rng(0)
    ds = _Dataset("heterogeneous", {"objects": 306, "rooms": 6}, [workloads.mp3d_like_graph(rng) for _ in range(4)])
    job = jobs.BaseTrainingJob({"train": ds, "val": ds, "test": ds}, {"conv_block": "GraphSAGE", "hidden_dim": 8, "num_layers": 2})
    with pytest.raises(_lib.HydraMPError):
        job.train(str(tmp_path), {"num_epochs": 1, "batch_size": 2})
    semi = jobs.SemiSupervisedTrainingJob(ds, {"conv_block": "GraphSAGE", "hidden_dim": 8, "num_layers": 2})
    with pytest.raises(_lib.HydraMPError):
        semi.train(str(tmp_path), {"num_epochs": 1, "batch_size": 2})
