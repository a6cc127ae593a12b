"""GraphStore.class_counts / class_weights (hmp_label_counts + hmp_balanced_class_weights, csrc/evaluate.hip) against their numpy
statement -- np.bincount over the counted labels and w_c = N / (K * n_c) in float64 cast to float32 -- bit for bit: typed and
homogeneous stores, with and without train_mask, n_classes 1 / 26 / 41 / 256 (and 300: the kernel without the LDS histogram),
absent classes, out-of-range labels, and a node split drawn again with another seed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.store import GraphStore, balanced_weights_host  # noqa: E402

DEV = "cuda:0"
N_CLASSES = [1, 26, 41, 256, 300]


def graphs_of(shape):
    if shape == "hetero":
        return workloads.semisupervised_graphs(9, seed=3)
    if shape == "homog":
        return workloads.stanford_semisupervised_graphs(9, seed=4)
    return workloads.stanford_htree_semisupervised_graphs(5, seed=5)


def host_rows(shape, graphs, head, mask):
    """numpy (labels, counted rows) of a head, from the host graphs"""
    if shape == "hetero":
        t = "rooms" if head == "rooms" else "objects"
        y = np.concatenate([g[t].y.numpy() for g in graphs])
        rows = np.ones(y.shape, dtype=bool)
        if mask:
            rows &= np.concatenate([getattr(g[t], mask).numpy() for g in graphs])
        return y, rows
    y = np.concatenate([g.y.numpy() for g in graphs])
    rm = np.concatenate([g.room_mask.numpy() for g in graphs])
    if head == "rooms":
        rows = rm.copy()
    else:
        rows = np.concatenate([g.object_mask.numpy() for g in graphs]) if shape == "homog_htree" else ~rm
    if mask:
        rows &= np.concatenate([getattr(g, mask).numpy() for g in graphs])
    return y, rows


def numpy_statement(y, rows, n_classes, ignored):
    y = y[rows]
    if ignored is not None:
        y = y[y != ignored]
    inside = (y >= 0) & (y < n_classes)
    counts = np.bincount(y[inside], minlength=n_classes).astype(np.int64)
    K, N = int((counts > 0).sum()), int(counts.sum())
    w = np.zeros(n_classes, dtype=np.float64)
    w[counts > 0] = N / (K * counts[counts > 0].astype(np.float64))
    return counts, int((~inside).sum()), w.astype(np.float32)


def check(store, shape, graphs, head, mask, n_classes, ignored):
    y, rows = host_rows(shape, graphs, head, mask)
    counts, outside, w = numpy_statement(y, rows, n_classes, ignored)
    kw = dict(label_type=head, mask=mask, n_classes=n_classes, ignored_label=ignored)
    got = store.class_counts(**kw)
    assert got.dtype == torch.int64 and got.shape == (n_classes,) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), counts), (shape, head, mask, n_classes)
    assert int(got.out_of_range) == outside
    gw = store.class_weights(**kw)
    assert gw.dtype == torch.float32 and gw.shape == (n_classes,) and gw.is_cuda
    assert np.array_equal(gw.cpu().numpy().view(np.int32), w.view(np.int32)), (shape, head, mask, n_classes)
    assert np.array_equal(balanced_weights_host(counts).view(np.int32), w.view(np.int32))
    return counts, outside


@pytest.mark.parametrize("n_classes", N_CLASSES)
@pytest.mark.parametrize("shape", ["hetero", "homog", "homog_htree"])
def test_counts_and_weights_equal_the_numpy_statement(shape, n_classes):
    graphs = graphs_of(shape)
    store = GraphStore(graphs, DEV)
    seen = 0
    for head in ("rooms", "objects"):
        for mask in (None, "train_mask"):
            counts, outside = check(store, shape, graphs, head, mask, n_classes, None)
            seen += int(counts.sum())
            if n_classes >= 41:
                assert (counts == 0).any()  # an absent class: weight 0
            if n_classes == 1:
                assert outside > 0  # labels past the class count go to the out-of-range slot, not into a bin
    assert seen > 0
    check(store, shape, graphs, "rooms", "train_mask", n_classes, 0)  # class 0 ignored


def test_out_of_range_labels_and_the_default_head_of_a_homogeneous_store():
    graphs = graphs_of("homog")
    rows = torch.nonzero(graphs[2].room_mask)[:, 0]
    graphs[2].y[rows[0]] = -3
    graphs[4].y[torch.nonzero(graphs[4].room_mask)[0, 0]] = 1 << 40
    store = GraphStore(graphs, DEV)
    counts, outside = check(store, "homog", graphs, "rooms", None, 26, None)
    assert outside == 2
    assert torch.equal(store.class_counts(n_classes=26), store.class_counts("rooms", n_classes=26))  # homogeneous: rooms by default
    with pytest.raises(_lib.HydraMPError, match="unknown scheme 'sqrt'"):
        store.class_weights("rooms", n_classes=26, scheme="sqrt")
    with pytest.raises(_lib.HydraMPError, match="n_classes"):
        store.class_counts("rooms")
    with pytest.raises(_lib.HydraMPError, match="'rooms' or 'objects'"):
        store.class_counts("node", n_classes=26)
    with pytest.raises(_lib.HydraMPError, match="no mask 'holdout_mask'"):
        store.class_counts("rooms", mask="holdout_mask", n_classes=26)
    typed = GraphStore(graphs_of("hetero"), DEV)
    with pytest.raises(_lib.HydraMPError, match="label_type"):
        typed.class_counts(n_classes=26)
    with pytest.raises(_lib.HydraMPError, match="no node type 'walls'"):
        typed.class_counts("walls", n_classes=26)


@pytest.mark.parametrize("shape", ["hetero", "homog"])
def test_counts_follow_a_new_node_split(shape):
    graphs = graphs_of(shape)
    store = GraphStore(graphs, DEV)
    seen = []
    for seed in (1, 2):
        store.generate_node_split(0.5, 0.25, 0.25, seed=seed)
        for head, C in (("rooms", 26), ("objects", 41)):
            if shape == "hetero":
                y = store.node_attrs[head]["y"].data.cpu().numpy()
                rows = store.node_attrs[head]["train_mask"].data.cpu().numpy()
            else:
                from hydra_gnn_amd.store import HOMO_NODE

                attrs = store.node_attrs[HOMO_NODE]
                y = attrs["y"].data.cpu().numpy()
                rm = attrs["room_mask"].data.cpu().numpy()
                rows = (rm if head == "rooms" else ~rm) & attrs["train_mask"].data.cpu().numpy()
            counts, outside, w = numpy_statement(y, rows, C, None)
            got = store.class_counts(head, mask="train_mask", n_classes=C)
            assert np.array_equal(got.cpu().numpy(), counts) and int(got.out_of_range) == outside
            gw = store.class_weights(head, mask="train_mask", n_classes=C)
            assert np.array_equal(gw.cpu().numpy().view(np.int32), w.view(np.int32))
            seen.append(counts)
    assert not (np.array_equal(seen[0], seen[2]) and np.array_equal(seen[1], seen[3]))  # the second split is another one
