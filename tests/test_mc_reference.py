"""CPU checks of tests/_mc_reference.py, the float64 restatement the Monte-Carlo dropout kernels are compared with: the identities
the statistics must satisfy, and the share of rows the label rule leaves out over the seeded score sets of the kernel test."""
import numpy as np
import pytest

from _mc_reference import (CLASSES, LABEL_GAP, MAX_EXEMPT, ROWS, SAMPLES, SEEDS, check_mc, entropy_tol, label_rows, mc_reference,
                           seeded_scores)


def test_one_sample_has_no_mutual_information_and_no_spread():
    for C in (1, 2, 5, 41):
        r = mc_reference(seeded_scores(11, 1, 65, C))
        assert (r["mutual_info"] == 0).all() and (r["std"] == 0).all()


def test_identical_samples_have_no_mutual_information_and_no_spread():
    s = seeded_scores(12, 1, 64, 17)
    one, four = mc_reference(s), mc_reference(np.repeat(s, 4, axis=0))
    assert np.array_equal(one["labels"], four["labels"])
    assert np.abs(one["mean"] - four["mean"]).max() <= 1e-15 and four["mutual_info"].max() <= 1e-14 and four["std"].max() <= 1e-7


@pytest.mark.parametrize("C", [1, 2, 5, 26, 130])
def test_uniform_scores_have_entropy_ln_c(C):
    for value in (0.0, -3.5, 1e4):
        r = mc_reference(np.full((3, 7, C), value, dtype=np.float32))
        assert np.abs(r["entropy"] - np.log(C)).max() <= 1e-12 and (r["labels"] == 0).all()
        assert np.abs(r["mean"] - 1.0 / C).max() <= 1e-15 and r["mutual_info"].max() <= 1e-12


@pytest.mark.parametrize("T", SAMPLES)
def test_zero_le_mi_le_entropy_le_ln_c(T):
    for C in CLASSES:
        r = mc_reference(seeded_scores(13, T, 130, C))
        assert (r["mutual_info"] >= 0).all() and (r["mutual_info"] <= r["entropy"] + 1e-12).all()
        assert (r["entropy"] <= np.log(C) + 1e-12).all() and (r["entropy"] >= -1e-15).all()
        assert (r["std"] >= 0).all() and (r["std"] <= 0.5 + 1e-12).all()  # a value in [0, 1] has variance at most 1 / 4
        assert np.abs(r["mean"].sum(axis=1) - 1).max() <= 1e-12


def test_one_class_is_all_zeros_with_label_0():
    r = mc_reference(seeded_scores(11, 8, 63, 1))
    assert (r["labels"] == 0).all() and (r["mean"] == 1).all()
    assert (r["std"] == 0).all() and (r["entropy"] == 0).all() and (r["mutual_info"] == 0).all()


def test_first_maximum_wins_a_tie():
    s = np.zeros((2, 3, 4), dtype=np.float32)
    s[:, 1, 2] = s[:, 1, 3] = 5.0
    s[:, 2, 3] = 2.0
    assert mc_reference(s)["labels"].tolist() == [0, 2, 3]


def test_mutual_information_of_two_opposed_samples():
    """two samples that are certain of different classes: the mean is a coin, every sample has entropy ~0"""
    s = np.zeros((2, 1, 2), dtype=np.float32)
    s[0, 0, 0] = s[1, 0, 1] = 40.0
    r = mc_reference(s)
    assert abs(r["entropy"][0] - np.log(2)) <= 1e-12 and abs(r["mutual_info"][0] - np.log(2)) <= 1e-12 and abs(r["std"][0] - 0.5) <= 1e-12


def test_the_label_rule_leaves_out_at_most_half_a_percent_of_the_seeded_rows():
    """over the whole list of the kernel test; classes == 1 has no second class and no gap"""
    exempt = total = 0
    for seed in SEEDS:
        for T in SAMPLES:
            for n in ROWS:
                for C in CLASSES:
                    use = label_rows(mc_reference(seeded_scores(seed, T, n, C)))
                    exempt += int((~use).sum())
                    total += n
    print(f"{exempt} of {total} rows have a top-two gap of the mean within {LABEL_GAP}")
    assert total == len(SEEDS) * len(SAMPLES) * sum(ROWS) * len(CLASSES)
    assert exempt <= MAX_EXEMPT * total


def test_check_mc_accepts_the_reference_and_refuses_an_error_past_the_bars():
    T, C = 8, 26
    r = mc_reference(seeded_scores(12, T, 65, C))
    good = (r["labels"], r["mean"].astype(np.float32), r["std"].astype(np.float32), r["entropy"].astype(np.float32),
            r["mutual_info"].astype(np.float32))
    check_mc(good, r, T, C, "reference in float32")
    for i, bump in ((1, 3e-5), (3, 4 * entropy_tol(T, C)), (4, 4 * entropy_tol(T, C))):
        bad = [a.copy() for a in good]
        bad[i].reshape(-1)[0] += bump
        with pytest.raises(AssertionError):
            check_mc(bad, r, T, C, "bumped")
    wrong = [a.copy() for a in good]
    row = int(np.argmax(r["gap"]))
    wrong[0][row] = (wrong[0][row] + 1) % C
    with pytest.raises(AssertionError):
        check_mc(wrong, r, T, C, "label")
