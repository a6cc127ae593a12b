"""Float64 numpy restatement of the Monte-Carlo dropout contract (include/hydra_mp.h: hmp_mc_accumulate_rows, hmp_mc_finish): no
project code.  From the per-sample scores s [T, n, C]:

    p_t[c]  = exp(s_t[c] - max_c s_t) / sum_c' exp(s_t[c'] - max_c s_t)        h_t = -sum_c p_t[c] log p_t[c]   (0 log 0 = 0)
    mean[c] = sum_t p_t[c] / T                                                  label = first-maximum argmax of mean
    std     = sqrt(max(0, sum_t p_t[label]^2 / T - mean[label]^2))
    entropy = -sum_c mean[c] log mean[c]                                        mutual_info = max(0, entropy - sum_t h_t / T)

and the tolerances a float32 kernel is held to.  tests/test_mc_reference.py checks the identities of this file on the CPU.

Tolerances.  A float32 softmax probability carries a relative error of about (C + 8) ulp (the sum of C terms, expf, the division);
averaging T of them adds T roundings: |mean - ref| <= (T + C + 8) * 2^-23 <= 1.8e-5 * max p for the largest case here -- inside the
project's float32 bar of 1e-5 absolute for these sizes because p <= 1 spreads over the classes.  The variance B / T - mean^2
cancels, so 1e-5 is a bar on the variance itself: std^2 is compared, not std.  Through x log x, whose derivative is 1 + log x, a
relative error e of the probabilities moves the entropy by at most e * (1 + ln C): entropy and mutual information are held to
(T + C + 8) * 2^-23 * (1 + ln C).

Labels are compared on the rows whose float64 top-two gap of `mean` exceeds LABEL_GAP = 4e-5 (4 x the bar on mean: two entries
each off by 1e-5 cannot swap across it); MAX_EXEMPT caps the share of rows the rule may leave out."""
import numpy as np

PROB_TOL = 1e-5
LABEL_GAP = 4e-5
MAX_EXEMPT = 0.005

# the seeded score sets of the kernel test (tests/test_gpu_mc_kernels.py)
SEEDS = (11, 12, 13)
SAMPLES = (1, 2, 3, 8, 17)
ROWS = (1, 63, 64, 65, 130)
CLASSES = (1, 2, 3, 4, 5, 15, 16, 17, 26, 41, 64, 65, 130)


def seeded_scores(seed, T, n, C):
    """float32 [T, n, C]"""
    rng = np.random.Generator(np.random.PCG64(seed * 1000003 + T * 10007 + n * 101 + C))
    return 3 * rng.standard_normal((T, n, C), dtype=np.float32)


def _xlogx(p):
    return np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)


def softmax64(s):
    s = np.asarray(s, dtype=np.float64)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def first_argmax(x):
    """index of the first maximum of every row, spelled out"""
    m = x.max(axis=1, keepdims=True)
    idx = np.broadcast_to(np.arange(x.shape[1])[None, :], x.shape)
    return np.where(x == m, idx, x.shape[1]).min(axis=1).astype(np.int64)


def mc_reference(scores):
    """scores [T, n, C] -> dict(labels int64 [n], mean [n, C], std, var, entropy, mutual_info [n], gap [n]) in float64; gap is the
    top-two gap of mean (inf for C == 1)"""
    s = np.asarray(scores, dtype=np.float64)
    assert s.ndim == 3 and s.shape[0] >= 1 and s.shape[2] >= 1
    T, n, C = s.shape
    p = softmax64(s)
    h = -_xlogx(p).sum(axis=2)  # [T, n]
    mean = p.sum(axis=0) / T
    labels = first_argmax(mean) if n else np.zeros(0, dtype=np.int64)
    rows = np.arange(n)
    var = np.maximum(0.0, (p * p).sum(axis=0)[rows, labels] / T - mean[rows, labels] ** 2)
    entropy = -_xlogx(mean).sum(axis=1)
    mi = np.maximum(0.0, entropy - h.sum(axis=0) / T)
    if C >= 2:
        top = np.sort(mean, axis=1)[:, ::-1]
        gap = top[:, 0] - top[:, 1]
    else:
        gap = np.full(n, np.inf)
    return dict(labels=labels, mean=mean, std=np.sqrt(var), var=var, entropy=entropy, mutual_info=mi, gap=gap)


def entropy_tol(T, C):
    return (T + C + 8) * 2.0 ** -23 * (1.0 + np.log(C))


def label_rows(ref):
    """bool [n]: the rows whose label is compared"""
    return ref["gap"] > LABEL_GAP


def score_bars(T, C, score_err=0.0):
    """(mean, variance, entropy, mutual information, label gap) bars.  score_err = d: the largest error of the SCORES the kernel
    computes for itself in float32 before its softmax (a pooled mean, a linear head's logits), measured as |float32 host scores -
    float64 scores| -- 0 where the scores are the kernel's input.  A score error d_c moves p_c by p_c (d_c - sum_j p_j d_j), at most
    2 p_c (1 - p_c) d <= d / 2; p_c^2 and mean^2 by at most 4 p^2 (1 - p) d <= 0.6 d each; the entropy -sum p ln p by
    |sum ln p_c dp_c| <= 2 d sum p_c |ln p_c| <= 2 d ln C, and the mutual information, a difference of two entropies, by twice
    that.  Two labels can swap when their means come within twice the bar on the mean."""
    d = float(score_err)
    lnc = float(np.log(C))
    return (PROB_TOL + d / 2, PROB_TOL + 1.2 * d, entropy_tol(T, C) + 2 * d * lnc, entropy_tol(T, C) + 4 * d * lnc, LABEL_GAP + 2 * d)


def check_mc(got, ref, T, C, tag, members=None, score_err=0.0):
    """got: (labels, mean, std, entropy, mutual_info) numpy arrays of a finishing launch over the reference's rows; members: bool [n],
    the rows outside hold -1 / 0; score_err: score_bars' d.  Prints each figure before it asserts.  Returns (rows exempt from the
    label rule, rows compared)."""
    labels, mean, std, entropy, mi = [np.asarray(a) for a in got]
    n = ref["mean"].shape[0]
    mem = np.ones(n, dtype=bool) if members is None else np.asarray(members, dtype=bool)
    assert labels.dtype == np.int64 and labels.shape == (n,) and mean.shape == (n, C), tag
    assert all(a.dtype == np.float32 and a.shape == (n,) for a in (std, entropy, mi)), tag
    assert (labels[~mem] == -1).all() and (mean[~mem] == 0).all(), f"{tag}: a row outside the head holds a label or a probability"
    assert (std[~mem] == 0).all() and (entropy[~mem] == 0).all() and (mi[~mem] == 0).all(), f"{tag}: a row outside the head holds a statistic"
    if not mem.any():
        return 0, 0
    b_mean, b_var, b_ent, b_mi, b_gap = score_bars(T, C, score_err)
    d_mean = np.abs(mean[mem].astype(np.float64) - ref["mean"][mem]).max()
    d_var = np.abs(std[mem].astype(np.float64) ** 2 - ref["var"][mem]).max()
    d_ent = np.abs(entropy[mem].astype(np.float64) - ref["entropy"][mem]).max()
    d_mi = np.abs(mi[mem].astype(np.float64) - ref["mutual_info"][mem]).max()
    print(f"  {tag}: mean {d_mean:.2e} (bar {b_mean:.2e}) var {d_var:.2e} (bar {b_var:.2e}) entropy {d_ent:.2e} (bar {b_ent:.2e}) "
          f"mi {d_mi:.2e} (bar {b_mi:.2e}) score error {score_err:.2e}")
    assert d_mean <= b_mean, f"{tag}: mean_probs off by {d_mean:.3e} (bar {b_mean:.3e})"
    assert d_var <= b_var, f"{tag}: std^2 off by {d_var:.3e} (bar {b_var:.3e})"
    assert d_ent <= b_ent, f"{tag}: entropy off by {d_ent:.3e} (bar {b_ent:.3e})"
    assert d_mi <= b_mi, f"{tag}: mutual_info off by {d_mi:.3e} (bar {b_mi:.3e})"
    assert (mi[mem] >= 0).all() and (std[mem] >= 0).all()
    use = (ref["gap"] > b_gap) & mem
    assert (labels[use] == ref["labels"][use]).all(), f"{tag}: {int((labels[use] != ref['labels'][use]).sum())} labels differ on compared rows"
    assert ((labels[mem] >= 0) & (labels[mem] < C)).all()
    return int((mem & ~use).sum()), int(mem.sum())
