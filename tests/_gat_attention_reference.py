"""Plain-torch / numpy CPU reference of the attention export (csrc/gat.hip gat_attention_kernel): no project code.  It sits next
to tests/_topk_reference.py.

    kept     the input edges whose endpoints exist, minus -- for a conv with self loops -- the input edges i -> i
    entries  the kept edges, then one loop i -> i (edge attributes 0) for i < n_loop = min(n_src, n_dst) with self loops
    raw      a_src[j, h] + a_dst[i, h] + <edge_attr, v_edge[:, h]>
    alpha    segment softmax per destination over its entries of leaky_relu(raw, 0.2), max-subtracted, denominator + 1e-16
    rows     row e < E = input edge e (0 when it is not kept), row E + i = loop i

float64 is the reference for alpha.  The top-k outputs are a function of the EXPORTED float32 alpha alone (head mean in float32,
heads added in ascending order, then a stable descending sort by CSR position): `top_from_alpha` restates it in numpy and the
kernel's two outputs must agree with it bit for bit."""
import numpy as np
import torch


def kept_edges(ei, n_src, n_dst, self_loops):
    """bool [E]: the input edges that are entries of the softmax"""
    j, i = ei[0], ei[1]
    ok = (j >= 0) & (j < n_src) & (i >= 0) & (i < n_dst)
    return ok & (j != i) if self_loops else ok


def attention_reference(a_src, a_dst, edge_attr, v_edge, ei, n_src, n_dst, self_loops):
    """alpha [E + n_loop, H] float64.  a_src [n_src, H], a_dst [n_dst, H], edge_attr [E, D] or None, v_edge [D, H] or None,
    ei int64 [2, E]"""
    E, H = ei.size(1), a_src.size(1)
    n_loop = min(n_src, n_dst) if self_loops else 0
    keep = kept_edges(ei, n_src, n_dst, self_loops)
    loop = torch.arange(n_loop, dtype=torch.int64)
    j = torch.cat([ei[0][keep], loop])
    i = torch.cat([ei[1][keep], loop])
    raw = a_src.double()[j] + a_dst.double()[i]
    if edge_attr is not None:
        ea = torch.cat([edge_attr.double()[keep], torch.zeros(n_loop, edge_attr.size(1), dtype=torch.float64)])
        raw = raw + ea @ v_edge.double()
    e = torch.nn.functional.leaky_relu(raw, 0.2)
    idx = i[:, None].expand(-1, H)
    m = torch.full((n_dst, H), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, e, "amax", include_self=True)
    p = torch.exp(e - m[i])
    den = torch.zeros(n_dst, H, dtype=torch.float64).index_add(0, i, p) + 1e-16
    a = p / den[i]
    out = torch.zeros(E + n_loop, H, dtype=torch.float64)
    nk = int(keep.sum())
    out[:E][keep] = a[:nk]
    out[E:] = a[nk:]
    return out


def top_from_alpha(alpha, ei, n_src, n_dst, self_loops, k):
    """(src int64 [n_dst, k], w float32 [n_dst, k]) from the exported alpha (numpy float32 [E + n_loop, H]): per destination row
    its kept edges in ascending edge id, then its loop (the CSR order of a stable plan); head mean (a_0 + a_1 + ...) / H in
    float32; stable descending sort; -1 / 0 past the row's entries"""
    alpha = np.asarray(alpha, dtype=np.float32)
    E, H = ei.size(1), alpha.shape[1]
    n_loop = min(n_src, n_dst) if self_loops else 0
    keep = kept_edges(ei, n_src, n_dst, self_loops).numpy()
    src_of, dst_of = ei[0].numpy(), ei[1].numpy()
    mean = alpha[:, 0].copy()
    for h in range(1, H):
        mean = (mean + alpha[:, h]).astype(np.float32)
    mean = (mean / np.float32(H)).astype(np.float32)
    src = np.full((n_dst, k), -1, dtype=np.int64)
    w = np.zeros((n_dst, k), dtype=np.float32)
    for r in range(n_dst):
        rows = [e for e in np.nonzero(keep & (dst_of == r))[0]]
        srcs = [int(src_of[e]) for e in rows]
        if r < n_loop:
            rows.append(E + r)
            srcs.append(r)
        if not rows:
            continue
        v = mean[np.asarray(rows)]
        order = np.argsort(-v, kind="stable")[:k]
        src[r, :len(order)] = np.asarray(srcs)[order]
        w[r, :len(order)] = v[order]
    return src, w
