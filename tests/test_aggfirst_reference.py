"""The float64 reference of tests/_aggfirst_reference.py against dense-matrix algebra and torch autograd on the CPU, so that the
reference the GPU tests trust is not wrong in the same way as a kernel: every operation is written a second time with a dense
incidence matrix or with the library's own operators (index_add_, relu, elu, autograd)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _aggfirst_reference import (ACT_ELU, ACT_NONE, ACT_RELU, bf16_bits, bf16_value, dx_gather_reference, edges_with_extents,
                                 lists_from_edges, mask_factor, pow2_parts, seg_mean_reference, seg_mean_t_reference, transposed_terms)


def _graph(seed, n_src=11, n_dst=7, n_edges=40):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n_src, n_edges)
    dst = rng.integers(0, n_dst - 2, n_edges)  # the last two destination rows stay empty
    src[:3] = n_src - 1  # a repeated neighbour, the last source row
    dst[:2] = 0
    return rng, src, dst, n_src, n_dst


def _dense(src, dst, n_src, n_dst):
    a = np.zeros((n_dst, n_src))
    np.add.at(a, (dst, src), 1.0)  # repeated edges count twice
    return a


def test_lists_are_stable_csr_and_csc():
    _, src, dst, n_src, n_dst = _graph(0)
    rowptr, col, t_rowptr, t_col, degf = lists_from_edges(src, dst, n_src, n_dst)
    for i in range(n_dst):
        assert col[rowptr[i]:rowptr[i + 1]].tolist() == [int(s) for s, d in zip(src, dst) if d == i]
    for j in range(n_src):
        assert t_col[t_rowptr[j]:t_rowptr[j + 1]].tolist() == [int(d) for s, d in zip(src, dst) if s == j]
    deg = np.diff(rowptr)
    assert deg[-1] == 0 and deg[-2] == 0 and rowptr[-1] == t_rowptr[-1] == src.size
    np.testing.assert_array_equal(degf, (1.0 / np.maximum(deg, 1)).astype(np.float32))


@pytest.mark.parametrize("seed", [1, 2])
def test_mean_is_the_dense_product_and_scatter_mean(seed):
    rng, src, dst, n_src, n_dst = _graph(seed)
    rowptr, col, _, _, _ = lists_from_edges(src, dst, n_src, n_dst)
    x = rng.normal(size=(n_src, 5))
    a = _dense(src, dst, n_src, n_dst)
    deg = a.sum(axis=1)
    m = seg_mean_reference(x, rowptr, col)
    np.testing.assert_allclose(m, (a @ x) / np.maximum(deg, 1)[:, None], rtol=1e-13, atol=1e-13)
    assert np.all(m[deg == 0] == 0)
    # [PyG] scatter(reduce="mean"): index_add of the gathered rows, divided by the clamped count
    xt = torch.from_numpy(x)
    s = torch.zeros(n_dst, 5, dtype=torch.float64).index_add_(0, torch.from_numpy(dst), xt[torch.from_numpy(src)])
    cnt = torch.zeros(n_dst, dtype=torch.float64).index_add_(0, torch.from_numpy(dst), torch.ones(src.size, dtype=torch.float64))
    np.testing.assert_allclose(m, (s / cnt.clamp(min=1)[:, None]).numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("seed", [3, 4])
def test_transposed_sum_is_the_exact_adjoint_of_the_mean(seed):
    """<M(x), d> == <x, M^T(d)> in float64, against the dense transpose, and against autograd of scatter-mean"""
    rng, src, dst, n_src, n_dst = _graph(seed)
    rowptr, col, t_rowptr, t_col, degf = lists_from_edges(src, dst, n_src, n_dst)
    x = rng.normal(size=(n_src, 6))
    d = rng.normal(size=(n_dst, 6))
    poisoned = 1.0 / np.maximum(np.diff(rowptr), 1)  # float64 reciprocals (degf holds them rounded to float32)
    np.testing.assert_array_equal(poisoned.astype(np.float32), degf)
    poisoned[np.diff(rowptr) == 0] = 1e30  # never read
    g, absum = transposed_terms(d, t_rowptr, t_col, poisoned)
    lhs = float((seg_mean_reference(x, rowptr, col) * d).sum())
    rhs = float((x * g).sum())
    assert abs(lhs - rhs) <= 1e-13 * float((np.abs(x) * absum).sum())
    a = _dense(src, dst, n_src, n_dst)
    np.testing.assert_allclose(g, a.T @ (d / np.maximum(a.sum(axis=1), 1)[:, None]), rtol=1e-13, atol=1e-13)
    assert np.all(absum >= np.abs(g) - 1e-15)
    xt = torch.from_numpy(x).requires_grad_(True)
    s = torch.zeros(n_dst, 6, dtype=torch.float64).index_add(0, torch.from_numpy(dst), xt[torch.from_numpy(src)])
    cnt = torch.from_numpy(np.maximum(a.sum(axis=1), 1))
    ((s / cnt[:, None]) * torch.from_numpy(d)).sum().backward()
    np.testing.assert_allclose(g, xt.grad.numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_ELU])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_mask_factor_is_autograd_of_the_stored_activation(act, p):
    """stored h = keep * act(z) / (1 - p), a dropped element stored as -0.0: d (h . w) / d z = w . factor(h)"""
    g = torch.Generator().manual_seed(10 * act + int(p * 10))
    z = torch.randn(9, 8, generator=g, dtype=torch.float64)
    keep = (torch.rand(9, 8, generator=g) >= p).double() if p > 0 else torch.ones(9, 8, dtype=torch.float64)
    scale = 1.0 / (1.0 - p)
    zl = z.clone().requires_grad_(True)
    y = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_ELU: F.elu}[act](zl) * keep * scale
    w = torch.randn(9, 8, generator=g, dtype=torch.float64)
    (y * w).sum().backward()
    h = y.detach().numpy().copy()
    if p > 0:
        h[keep.numpy() == 0] = -0.0
        assert np.signbit(h[keep.numpy() == 0]).all()
    f = mask_factor(h, act, p > 0, scale)
    np.testing.assert_allclose(f * w.numpy(), zl.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_mask_factor_treats_signed_zeros_as_the_contract_says():
    h = np.array([0.0, -0.0, -0.5, 0.25], dtype=np.float32)
    assert mask_factor(h, ACT_RELU, False, 1.0).tolist() == [0.0, 0.0, 0.0, 1.0]
    assert mask_factor(h, ACT_ELU, False, 1.0).tolist() == [1.0, 1.0, 0.5, 1.0]  # -0.0 without dropout: an ordinary zero
    assert mask_factor(h, ACT_NONE, False, 1.0).tolist() == [1.0, 1.0, 1.0, 1.0]
    assert mask_factor(h, ACT_RELU, True, 2.0).tolist() == [0.0, 0.0, 0.0, 2.0]
    assert mask_factor(h, ACT_ELU, True, 2.0).tolist() == [2.0, 0.0, 1.5, 2.0]  # -0.0 under dropout: dropped
    assert mask_factor(h, ACT_NONE, True, 2.0).tolist() == [2.0, 0.0, 2.0, 2.0]


def test_masked_transpose_and_gather_add_compose_in_the_stated_order():
    rng, src, dst, n_src, n_dst = _graph(5)
    _, _, t_rowptr, t_col, degf = lists_from_edges(src, dst, n_src, n_dst)
    d = rng.normal(size=(n_dst, 4))
    h = rng.normal(size=(n_src, 6)).astype(np.float32)
    h[0, 0] = -0.0
    s, a = transposed_terms(d, t_rowptr, t_col, degf)
    g, ga = seg_mean_t_reference(d, t_rowptr, t_col, degf, h, ACT_ELU, True, 2.0)
    f = mask_factor(h[:, :4], ACT_ELU, True, 2.0)
    np.testing.assert_array_equal(g, f * s)
    np.testing.assert_array_equal(ga, np.abs(f) * a)
    assert g[0, 0] == 0.0
    prod = rng.normal(size=(n_src, 4))
    out = dx_gather_reference(prod, s, h, ACT_RELU, True, 2.0)
    fr = mask_factor(h[:, :4], ACT_RELU, True, 2.0)
    np.testing.assert_array_equal(out, fr * (prod + s))
    assert np.abs(out - (fr * prod + s)).max() > 0.1  # the mask applied before the add is a different function
    np.testing.assert_array_equal(dx_gather_reference(prod, s), prod + s)


def test_bf16_helpers_round_to_nearest_even_like_torch():
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.normal(size=1000).astype(np.float32) * 100, np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -3.5], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16)
    np.testing.assert_array_equal(bf16_bits(x).view(np.int16), want.view(torch.int16).numpy())
    np.testing.assert_array_equal(bf16_value(bf16_bits(x)), want.float().numpy())


@pytest.mark.parametrize("total,n", [(1, 1), (7, 3), (134, 9), (65610, 300)])
def test_pow2_parts_and_edge_maker(total, n):
    parts = pow2_parts(total, n)
    assert len(parts) == n and sum(parts) == total and all(p & (p - 1) == 0 for p in parts)
    ext = np.zeros(max(total // 2, 1), dtype=np.int64)
    ext[:] = total // ext.size
    ext[0] += total - int(ext.sum())
    src, dst = edges_with_extents(ext, n, np.random.default_rng(0))
    assert np.bincount(src, minlength=ext.size).tolist() == ext.tolist()
    deg = np.bincount(dst)
    assert deg.sum() == total and all(int(q) & (int(q) - 1) == 0 and q > 0 for q in deg)
