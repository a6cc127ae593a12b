"""Host side of the class-weighted cross entropy: the new exports and the ABI number, the numpy statement of the balanced weights,
balanced accuracy from a hand-made confusion matrix, and the refusals by name.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from hydra_gnn_amd import _lib, evaluate
from hydra_gnn_amd.models.utils import class_weight_tensor, cross_entropy_loss
from hydra_gnn_amd.store import CLASS_WEIGHT_SCHEMES, balanced_weights_host, check_weight_scheme

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hydra_mp.h")
NEW = ["hmp_net_set_class_weights", "hmp_masked_ce_weighted", "hmp_label_counts", "hmp_balanced_class_weights"]
NEW_DIAGNOSTIC = ["hmp_head_tails_weighted", "hmp_linear_heads_run_weighted"]


def test_new_exports_and_the_abi_number_agree():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW + NEW_DIAGNOSTIC:
        assert re.search(rf"^int {name}\(", text, re.M), f"{name} is not declared in include/hydra_mp.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert getattr(lib, name).restype is not None
    header_abi = int(re.search(r"^#define\s+HMP_ABI_VERSION\s+(\d+)", text, re.M).group(1))
    assert lib.hmp_abi_version() == header_abi == _lib.ABI_VERSION
    # the additions change no struct: every layout the binding mirrors still has the library's size
    import ctypes as C

    for i, st in enumerate(_lib._STRUCTS):
        assert lib.hmp_sizeof(i) == C.sizeof(st), st.__name__


def test_argument_checks_of_the_new_entries_without_a_device():
    lib = _lib.load()
    assert lib.hmp_net_set_class_weights(None, 0, None, 0) != 0 and b"null net" in lib.hmp_last_error()
    assert lib.hmp_label_counts(None, -1, None, 0, 26, None, None) != 0 and b"label_counts" in lib.hmp_last_error()
    assert lib.hmp_label_counts(None, 0, None, 0, 0, None, None) != 0  # n_classes >= 1
    assert lib.hmp_label_counts(None, 0, None, 0, 26, None, None) == 0  # no rows: nothing launched
    assert lib.hmp_balanced_class_weights(None, 26, None, None) != 0 and b"balanced_class_weights" in lib.hmp_last_error()
    assert lib.hmp_masked_ce_weighted(None, 4, 1, 4, None, -1, None, None, 4, None, None) != 0
    assert b"hmp_masked_ce_weighted" in lib.hmp_last_error()


def numpy_balanced(labels, n_classes):
    counts = np.bincount(labels, minlength=n_classes).astype(np.int64)
    K, N = int((counts > 0).sum()), int(counts.sum())
    w = np.zeros(n_classes, dtype=np.float64)
    w[counts > 0] = N / (K * counts[counts > 0].astype(np.float64))
    return counts, w.astype(np.float32)


@pytest.mark.parametrize("n_classes", [1, 26, 41, 256])
def test_balanced_weights_host_is_the_numpy_statement(n_classes):
    rng = np.random.default_rng(n_classes)
    p = rng.dirichlet(np.full(n_classes, 0.3))  # skewed, as room labels are
    labels = rng.choice(n_classes, size=997, p=p)
    counts, want = numpy_balanced(labels, n_classes)
    got = balanced_weights_host(counts)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got == 0, counts == 0)  # absent classes weigh 0
    # scikit-learn's property: the weighted class sizes are equal, N / K each
    present = counts > 0
    np.testing.assert_allclose(got[present].astype(np.float64) * counts[present], counts.sum() / present.sum(), rtol=1e-6)
    assert np.array_equal(balanced_weights_host(np.zeros(n_classes, dtype=np.int64)), np.zeros(n_classes, dtype=np.float32))


def test_balanced_accuracy_from_a_hand_made_confusion_matrix():
    #            pred 0  1  2  3
    conf = np.array([[8, 2, 0, 0],    # recall 0.8
                     [1, 1, 0, 2],    # recall 0.25
                     [0, 0, 0, 0],    # no support: not part of the mean
                     [0, 3, 0, 3]])   # recall 0.5
    want = (0.8 + 0.25 + 0.5) / 3
    assert evaluate.balanced_accuracy(conf) == pytest.approx(want, abs=1e-15)
    assert evaluate.balanced_accuracy(torch.from_numpy(conf).reshape(-1)) == pytest.approx(want, abs=1e-15)
    plain = np.trace(conf) / conf.sum()
    assert plain == 12 / 20 and evaluate.balanced_accuracy(conf) < plain  # the majority class no longer dominates
    with pytest.raises(ZeroDivisionError):
        evaluate.balanced_accuracy(np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="not square"):
        evaluate.balanced_accuracy(np.zeros(7))


def test_refusals_by_name():
    with pytest.raises(_lib.HydraMPError, match=r"class_weight: \(25,\) weights for 26 classes \(wrong length\)"):
        class_weight_tensor([1.0] * 25, 26, "cpu")
    with pytest.raises(_lib.HydraMPError, match="wrong length"):
        class_weight_tensor(torch.ones(2, 13), 26, "cpu")
    with pytest.raises(_lib.HydraMPError, match="negative weight"):
        class_weight_tensor([1.0, -0.5, 2.0], 3, "cpu")
    with pytest.raises(_lib.HydraMPError, match="negative weight"):
        class_weight_tensor(torch.tensor([1.0, float("nan")]), 2, "cpu", "w")
    with pytest.raises(_lib.HydraMPError, match="floating point"):
        class_weight_tensor(torch.ones(3, dtype=torch.int64), 3, "cpu")
    w = class_weight_tensor([0.0, 0.5, 2.0], 3, "cpu")  # zeros are weights too
    assert w.dtype == torch.float32 and w.tolist() == [0.0, 0.5, 2.0]
    assert CLASS_WEIGHT_SCHEMES == ("balanced",) and check_weight_scheme("balanced") == "balanced"
    with pytest.raises(_lib.HydraMPError, match="unknown scheme 'inverse_sqrt'"):
        check_weight_scheme("inverse_sqrt")
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):  # the weighted loss is native too
        cross_entropy_loss(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), None, weight=torch.ones(3))
