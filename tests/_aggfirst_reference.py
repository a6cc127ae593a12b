"""Float64 numpy restatements of the aggregate-first SAGE conv operations (csrc/aggfirst.hip, the gather-add term of the
input-gradient GEMM): no project code.  Written from the contract, not from the kernels:

    mean        M[i, :] = (1 / max(deg_i, 1)) * sum_{k in CSR row i} X[col[k], :]                     (an empty row is 0)
    transpose   S[j, :] = sum_{k in CSC row j} dM[t_col[k], :] * degf[t_col[k]]                        degf[i] = 1 / max(deg_i, 1)
                G[j, :] = factor(H[j, :]) . S[j, :]
    factor      from the STORED activations h and the dropout scale s (1 without dropout):
                  under dropout an element stored as -0.0 was dropped: 0
                  none: s        relu: h > 0 ? s : 0        elu: h > 0 ? s : h + s      (stored h = s * elu(z): s * elu'(z) = h + s)
                without dropout -0.0 is an ordinary zero (relu 0, elu 0 + s)
    dx + gather G = factor(H) . (dZ W + S)       the term enters BEFORE the mask

tests/test_aggfirst_reference.py checks this file on the CPU against dense-matrix algebra and torch autograd."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2


def lists_from_edges(src, dst, n_src, n_dst):
    """int32 (rowptr [n_dst + 1], col [E], t_rowptr [n_src + 1], t_col [E]) and float32 degf [n_dst] of the edges src[e] -> dst[e]:
    CSR by destination and CSC by source, both stable in edge order; degf = 1 / max(in-degree, 1)"""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    assert src.shape == dst.shape
    assert src.size == 0 or (src.min() >= 0 and src.max() < n_src and dst.min() >= 0 and dst.max() < n_dst)
    deg = np.bincount(dst, minlength=n_dst)
    tdeg = np.bincount(src, minlength=n_src)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    t_rowptr = np.concatenate([[0], np.cumsum(tdeg)])
    col = src[np.argsort(dst, kind="stable")]
    t_col = dst[np.argsort(src, kind="stable")]
    degf = (1.0 / np.maximum(deg, 1)).astype(np.float32)
    return rowptr.astype(np.int32), col.astype(np.int32), t_rowptr.astype(np.int32), t_col.astype(np.int32), degf


def seg_mean_reference(x, rowptr, col):
    """float64 [n_rows, F]: the mean of the listed rows of x per CSR row (divisor max(deg, 1))"""
    x = np.asarray(x, dtype=np.float64)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    out = np.zeros((rowptr.size - 1, x.shape[1]), dtype=np.float64)
    for i in range(rowptr.size - 1):
        b, e = rowptr[i], rowptr[i + 1]
        if e > b:
            out[i] = x[col[b:e]].sum(axis=0) / float(e - b)
    return out


def transposed_terms(dm, t_rowptr, t_col, degf):
    """float64 (S [n_rows, F], sum of |terms| [n_rows, F]): S[j] = sum over CSC row j of dm[t_col[k]] * degf[t_col[k]]; degf of a
    destination row no entry names is never read"""
    dm = np.asarray(dm, dtype=np.float64)
    t_rowptr = np.asarray(t_rowptr, dtype=np.int64)
    t_col = np.asarray(t_col, dtype=np.int64)
    degf = np.asarray(degf, dtype=np.float64)
    n = t_rowptr.size - 1
    s = np.zeros((n, dm.shape[1]), dtype=np.float64)
    a = np.zeros_like(s)
    for j in range(n):
        for k in range(t_rowptr[j], t_rowptr[j + 1]):
            t = dm[t_col[k]] * degf[t_col[k]]
            s[j] += t
            a[j] += np.abs(t)
    return s, a


def mask_factor(h, act, drop_on, scale):
    """float64 factor per element of the stored activations h (a float array that keeps the sign of its zeros)"""
    h = np.asarray(h)
    h64 = h.astype(np.float64)
    if act == ACT_RELU:
        f = np.where(h64 > 0, scale, 0.0)
    elif act == ACT_ELU:
        f = np.where(h64 > 0, scale, h64 + scale)
    else:
        assert act == ACT_NONE
        f = np.full(h64.shape, float(scale))
    if drop_on:
        f = np.where((h64 == 0) & np.signbit(h64), 0.0, f)
    return f


def seg_mean_t_reference(dm, t_rowptr, t_col, degf, h=None, act=ACT_NONE, drop_on=False, scale=1.0):
    """float64 G [n_rows, F] and the sum of |terms| (times |factor|) for error bounds"""
    s, a = transposed_terms(dm, t_rowptr, t_col, degf)
    if h is None:
        return s, a
    f = mask_factor(np.asarray(h)[:, : s.shape[1]], act, drop_on, scale)
    return f * s, np.abs(f) * a


def dx_gather_reference(prod, term, h=None, act=ACT_NONE, drop_on=False, scale=1.0):
    """float64 factor(h) . (prod + term): prod = dZ W and term = transposed_terms(...)[0], both [M, N]"""
    out = np.asarray(prod, dtype=np.float64) + np.asarray(term, dtype=np.float64)
    if h is not None:
        out = mask_factor(np.asarray(h)[:, : out.shape[1]], act, drop_on, scale) * out
    return out


# ---- bf16 (numpy has no such type): bit patterns as uint16 --------------------------------------------------------------------
def bf16_bits(x):
    """uint16 bit patterns of float32 x rounded to bf16 (nearest, ties to even); x finite"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    """float32 values of bf16 bit patterns"""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---- graph makers shared by the GPU tests -------------------------------------------------------------------------------------
def pow2_parts(total, n):
    """n powers of two that add up to total (total >= n >= popcount(total)): the in-degrees of n destination rows whose reciprocal
    is exact"""
    parts = [1 << b for b in range(total.bit_length()) if (total >> b) & 1]
    assert len(parts) <= n <= total
    while len(parts) < n:
        parts.sort()
        big = parts.pop()
        parts += [big // 2, big // 2]
    assert sum(parts) == total and all(p & (p - 1) == 0 for p in parts)
    return sorted(parts)


def edges_with_extents(extents, n_dst_used, rng):
    """(src, dst) with extents[j] edges leaving source row j, their destinations a shuffle of rows 0 .. n_dst_used - 1 with
    power-of-two in-degrees"""
    extents = np.asarray(extents, dtype=np.int64)
    total = int(extents.sum())
    src = np.repeat(np.arange(extents.size), extents)
    if total == 0:
        return src, np.zeros(0, dtype=np.int64)
    n = max(min(n_dst_used, total), bin(total).count("1"))
    dst = np.repeat(np.arange(n), pow2_parts(total, n))
    return src, rng.permutation(dst)
