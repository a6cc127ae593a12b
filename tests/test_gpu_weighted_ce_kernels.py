"""Class-weighted cross entropy at the kernel entries: hmp_masked_ce_weighted (ce_row, csrc/optim.hip), hmp_head_tails_weighted
(ce_group in tail_ce_kernel / pool_ce_kernel, csrc/semisup.hip) and hmp_linear_heads_run_weighted (csrc/heads.hip).

The rule (csrc/tail_fns.h): a counted row contributes {w[y] * nll, w[y]} and w[y] * (softmax - onehot); a row of weight 0 does not
count, exactly as an ignored one; w is indexed by labels inside [0, classes) only; without weights the bits are the unweighted
ones.  The normaliser (the sum of weights) is used as it is when > 0.

Assertions, per entry:
  1. weights all 1.0                 bit-identical to the unweighted call
  2. weights all 0.25                the loss pair is 0.25 x the unweighted pair bit for bit (a power of two scales exactly); the
                                     standalone entry: 3 valid rows (weight sum 0.75), one Adam step divided by that sum leaves
                                     parameters and moments bit-identical to the unweighted step -- only if no clamp at 1 survives
  3. one class of weight 0           bit-identical to that class's labels replaced by `ignored`
  4. random positive weights         against float64 torch on the CPU, F.cross_entropy(weight=, reduction="sum") and the weight
                                     sum, with the tolerance of tests/test_gpu_ops.py::test_masked_ce (atol = rtol = 1e-5; the
                                     loss sum atol 1e-5 x max(1, valid rows)), on the loss and every gradient the entry writes
                                     (d loss / d logits or d z; the linear heads: d z, dW, db).  The linear heads run on the
                                     inputs of tests/test_gpu_tail_kernels.py with W scaled by 1/16 (exact): as they are, 64 + 64
                                     classes at F = 65 give logits near +-40, where one float32 ulp of a logit (3.8e-6) already
                                     puts 1e-5 into weight x softmax x W (measured on those inputs: dz off by 1.2e-5 on 2 of 2145
                                     elements, dW by 3.1e-5 on 5 of 8320; that file says the same of its F = 1024 case and holds
                                     these tensors to a float32 yardstick instead).  With logits inside +-5 float32 resolves the
                                     absolute 1e-5 this file asks of every tensor
  5. all weights 0                   loss 0, gradients 0, an Adam step moves the parameters by weight decay alone, all finite
  6. a label outside [0, classes)    status bit 1 (tails, heads), no contribution, and no read past the weight vector, which is
                                     allocated with exactly `classes` entries at the END of a buffer whose neighbours hold NaN
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import test_gpu_tail_kernels as tk  # noqa: E402  (the inputs, descriptors and launch helpers of the unweighted tests)
from _tail_reference import _act, head_members  # noqa: E402
from hydra_gnn_amd import _lib  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5  # tests/test_gpu_ops.py
IGNORED = tk.IGNORED
CLASSES = [1, 5, 64, 65, 130, 255, 256]
ROWS = [1, 17, 67]
N, R, E = tk.N, tk.R, tk.E


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def weight_vector(values):
    """exactly len(values) floats at the end of an allocation, NaN in front: a read at index -1 or of a stale pointer is poison"""
    buf = torch.full((len(values) + 8,), float("nan"), dtype=torch.float32, device=dev())
    w = buf[8:]
    w.copy_(torch.as_tensor(values, dtype=torch.float32))
    assert w.numel() == len(values)
    return w


def random_weights(classes, seed):
    g = torch.Generator().manual_seed(900 + seed)
    return (torch.rand(classes, generator=g) * 3.0 + 0.05).float()


def vp_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


# ---- the standalone entry ----------------------------------------------------------------------------------------------------------
def ce_inputs(n, c, seed=0, bad=False):
    rng = np.random.default_rng(1000 * n + c + seed)
    logits = torch.from_numpy(rng.normal(0, 3, size=(n, c)).astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, c, size=n).astype(np.int64))
    if n >= 17:
        labels[1] = IGNORED
        if bad:
            labels[2], labels[3] = -1, c
    return logits, labels


def masked_ce(logits, labels, w=None, grad=True):
    """(out2, grad [n, ld]) of hmp_masked_ce (w None) or hmp_masked_ce_weighted; grad starts as NaN"""
    lib = _lib.require_device()
    n, c = logits.shape
    ld = ((c + 3) // 4) * 4 + 4
    lg = torch.full((n, ld), float("nan"), device=dev())
    lg[:, :c] = logits.to(dev())
    g = torch.full((n, ld), float("nan"), device=dev()) if grad else None
    out2 = torch.full((2,), float("nan"), device=dev())
    lab = labels.to(dev())
    gp = g.data_ptr() if grad else None
    if w is None:
        _lib.check(lib.hmp_masked_ce(lg.data_ptr(), ld, n, c, lab.data_ptr(), IGNORED, gp, ld, out2.data_ptr(), _lib.stream_ptr()))
    else:
        _lib.check(lib.hmp_masked_ce_weighted(lg.data_ptr(), ld, n, c, lab.data_ptr(), IGNORED, w.data_ptr(), gp, ld, out2.data_ptr(),
                                              _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out2, g


def adam_step(p0, g, count, wd=0.01):
    """one hmp_adam_flat step from p0 with moments 0: (p, m, v)"""
    lib = _lib.require_device()
    p = p0.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    gg = g.contiguous()
    _lib.check(lib.hmp_adam_flat(p.data_ptr(), gg.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 0.01, 0.9, 0.999, 1e-8, wd, 1,
                                 count.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return p, m, v


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("n", ROWS)
def test_standalone_unit_zero_class_and_random_weights(n, c):
    logits, labels = ce_inputs(n, c)
    out0, g0 = masked_ce(logits, labels)
    # 1. all ones
    out1, g1 = masked_ce(logits, labels, weight_vector([1.0] * c))
    assert torch.equal(bits(out0), bits(out1)) and torch.equal(bits(g0), bits(g1))
    # 3. class z of weight 0 == its labels ignored
    z = int(labels[0]) if int(labels[0]) >= 0 else 0
    wz = [1.0] * c
    wz[z] = 0.0
    outz, gz = masked_ce(logits, labels, weight_vector(wz))
    lab_ign = labels.clone()
    lab_ign[labels == z] = IGNORED
    outi, gi = masked_ce(logits, lab_ign)
    assert torch.equal(bits(outz), bits(outi)) and torch.equal(bits(gz), bits(gi))
    # 4. random positive weights against float64 torch
    w = random_weights(c, n)
    outw, gw = masked_ce(logits, labels, weight_vector(w.tolist()))
    valid = labels != IGNORED
    l64 = logits.double().requires_grad_(True)
    got = outw.cpu().double()
    if int(valid.sum()) == 0:
        assert got.tolist() == [0.0, 0.0]
        return
    ref = F.cross_entropy(l64[valid], labels[valid], weight=w.double(), reduction="sum")
    ref.backward()
    wsum = w.double()[labels[valid]].sum()
    print(f"  n {n} c {c}: loss {float(got[0]):.6f} (ref {float(ref.detach()):.6f}), weight sum {float(got[1]):.6f} (ref {float(wsum):.6f})")
    torch.testing.assert_close(got[0], ref.detach(), atol=ATOL * max(1, int(valid.sum())), rtol=RTOL)
    torch.testing.assert_close(got[1], wsum, atol=ATOL * max(1, int(valid.sum())), rtol=RTOL)
    torch.testing.assert_close(gw[:, :c].cpu().double(), l64.grad, atol=ATOL, rtol=RTOL)
    assert torch.all(gw[:, c:] == 0)
    # the weighted mean is torch's
    mean_ref = F.cross_entropy(logits.double()[valid], labels[valid], weight=w.double())
    torch.testing.assert_close(got[0] / got[1], mean_ref, atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("c", CLASSES)
def test_standalone_quarter_weights_three_valid_rows_full_step(c):
    """weight sum 0.75 < 1: the pair is 0.25 x the unweighted pair and the Adam step divided by 0.75 equals the step divided by 3"""
    logits, labels = ce_inputs(17, c)
    labels[:] = IGNORED
    labels[0], labels[7], labels[16] = 0, c - 1, c // 2  # waves 0, 7 and the second round of wave 0
    out0, g0 = masked_ce(logits, labels)
    outq, gq = masked_ce(logits, labels, weight_vector([0.25] * c))
    assert out0.cpu().tolist()[1] == 3.0 and outq.cpu().tolist()[1] == 0.75
    assert torch.equal(bits(outq), bits(out0 * 0.25))
    assert torch.equal(bits(gq), bits(g0 * 0.25))
    p0 = torch.randn(g0.numel(), generator=torch.Generator().manual_seed(c)).to(dev())
    ref = adam_step(p0, g0.reshape(-1), out0[1:])
    got = adam_step(p0, gq.reshape(-1), outq[1:])
    for a, b, name in zip(got, ref, ("parameters", "m", "v")):
        assert torch.equal(bits(a), bits(b)), f"{name} differ: a clamp at 1 survives in the optimiser"


@pytest.mark.parametrize("c", [1, 5, 65, 256])
@pytest.mark.parametrize("n", ROWS)
def test_standalone_all_zero_weights(n, c):
    logits, labels = ce_inputs(n, c)
    out, g = masked_ce(logits, labels, weight_vector([0.0] * c))
    assert out.cpu().tolist() == [0.0, 0.0]
    assert bool((g == 0).all())
    p0 = torch.randn(g.numel(), generator=torch.Generator().manual_seed(n + c)).to(dev())
    p, m, v = adam_step(p0, g.reshape(-1), out[1:], wd=0.01)
    pz, mz, vz = adam_step(p0, torch.zeros_like(g).reshape(-1), torch.ones(1, device=dev()), wd=0.01)  # weight decay alone
    for a, b in ((p, pz), (m, mz), (v, vz)):
        assert bool(torch.isfinite(a).all()) and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("c", [1, 5, 64, 256])
def test_standalone_out_of_range_label_never_indexes_the_weights(c):
    logits, labels = ce_inputs(17, c, bad=True)
    labels[4] = 1 << 40
    w = random_weights(c, 3)
    out, g = masked_ce(logits, labels, weight_vector(w.tolist()))
    ok = (labels >= 0) & (labels < c)
    ref = F.cross_entropy(logits.double()[ok], labels[ok], weight=w.double(), reduction="sum")
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(g).all())
    torch.testing.assert_close(got[0], ref, atol=ATOL * 17, rtol=RTOL)
    torch.testing.assert_close(got[1], w.double()[labels[ok]].sum(), atol=ATOL * 17, rtol=RTOL)
    assert bool((g[~ok.to(dev())] == 0).all())


# ---- tails -----------------------------------------------------------------------------------------------------------------------
def run_tail(heads, mode, act, weights=None):
    """one CE launch (mode 0 unpooled, 2 pooled) with per-head weight vectors (None: the unweighted entry)"""
    outs = [h.outputs() for h in heads]
    state = torch.zeros(5, dtype=torch.int32, device=dev())
    arr = (_lib.TailDesc * len(heads))(*[h.desc(o, mode == 2) for h, o in zip(heads, outs)])
    lib = _lib.load()
    if weights is None:
        rc = lib.hmp_head_tails(arr, len(heads), mode, act, IGNORED, state.data_ptr(), None, _lib.stream_ptr())
    else:
        rc = lib.hmp_head_tails_weighted(arr, len(heads), vp_array(weights), mode, act, IGNORED, state.data_ptr(), None, _lib.stream_ptr())
    assert rc == 0, lib.hmp_last_error()
    return outs, tk.sync_status(state)


def same_outputs(a, b, heads, mode):
    for h, x, y in zip(heads, a, b):
        keys = ("grad", "row_lv") + (("dpool",) if mode == 2 else ())
        for k in keys:
            xa, ya = x[k], y[k]
            if k == "dpool":  # the scratch is defined on the columns of the classes' quads
                xa, ya = xa[:h.n_pool, :tk.align4(h.classes)], ya[:h.n_pool, :tk.align4(h.classes)]
            assert torch.equal(bits(xa), bits(ya)), k


def tail_reference_weighted(h, w):
    """float64 torch: F.cross_entropy(weight=w, reduction="sum") over the valid rows of y = dropout(act(z)) (pooled: their means)"""
    zl = h.z[:h.n_rows, :h.classes].double().clone().requires_grad_(True)
    y = _act(zl, h.act)
    if h.p > 0:
        y = y * h.keep[:, :h.classes].double() / (1.0 - h.p)
    if h.pool is not None:
        rowptr = torch.as_tensor(np.asarray(h.pool[0]), dtype=torch.int64)
        col = torch.as_tensor(np.asarray(h.pool[1]), dtype=torch.int64)
        deg = rowptr[1:] - rowptr[:-1]
        seg = torch.repeat_interleave(torch.arange(h.n_pool), deg)
        y = torch.zeros(h.n_pool, h.classes, dtype=torch.float64).index_add(0, seg, y[col]) / deg.clamp(min=1).double()[:, None]
    lab = h.labels[:h.n_pool]
    m = torch.ones(h.n_pool, dtype=torch.bool) if h.mask is None else h.mask[:h.n_pool] != 0
    valid = m & (lab != IGNORED) & (lab >= 0) & (lab < h.classes)
    row_w = torch.where(valid, w.double()[lab.clamp(0, h.classes - 1)], torch.zeros(h.n_pool, dtype=torch.float64))
    if int(valid.sum()) == 0:
        return torch.zeros((), dtype=torch.float64), row_w, torch.zeros_like(zl)
    loss = F.cross_entropy(y[valid], lab[valid], weight=w.double(), reduction="sum")
    loss.backward()
    return loss.detach(), row_w, zl.grad


def check_tail_forms(heads, mode, act):
    out0, st0 = run_tail(heads, mode, act)
    ones = [weight_vector([1.0] * h.classes) for h in heads]
    # 1. all ones; and a null vector per head is the unweighted entry
    same_outputs(run_tail(heads, mode, act, ones)[0], out0, heads, mode)
    same_outputs(run_tail(heads, mode, act, [None] * len(heads))[0], out0, heads, mode)
    # 2. all 0.25: the pair scales exactly
    outq, _ = run_tail(heads, mode, act, [weight_vector([0.25] * h.classes) for h in heads])
    for h, q, o in zip(heads, outq, out0):
        assert torch.equal(bits(q["row_lv"][:h.n_pool]), bits(o["row_lv"][:h.n_pool] * 0.25))
        if mode == 0:
            assert torch.equal(bits(q["grad"][:h.n_rows]), bits(o["grad"][:h.n_rows] * 0.25))
    # 3. one class of weight 0 == its labels ignored
    wz, saved = [], []
    for h in heads:
        z = int(h.labels[h.n_pool // 2]) if h.n_pool and 0 <= int(h.labels[h.n_pool // 2]) < h.classes else 0
        v = [1.0] * h.classes
        v[z] = 0.0
        wz.append(weight_vector(v))
        saved.append((z, h.d_labels))
    outz, stz = run_tail(heads, mode, act, wz)
    for h, (z, d_lab) in zip(heads, saved):
        lab = h.labels.clone()
        lab[lab == z] = IGNORED
        h.d_labels = lab.to(dev())
    try:
        outi, sti = run_tail(heads, mode, act)
    finally:
        for h, (_, d_lab) in zip(heads, saved):
            h.d_labels = d_lab
    same_outputs(outz, outi, heads, mode)
    assert stz == sti == st0  # 6. the out-of-range labels of the inputs raise the status with weights set as without
    # 5. all zero
    outn, _ = run_tail(heads, mode, act, [weight_vector([0.0] * h.classes) for h in heads])
    for h, o in zip(heads, outn):
        assert bool((o["row_lv"][:h.n_pool] == 0).all()) and bool((o["grad"][:h.n_rows] == 0).all())
    # 4. random positive weights against float64 torch (6.: the inputs hold labels -1 and `classes`; the vectors end at `classes`)
    ws = [random_weights(h.classes, i) for i, h in enumerate(heads)]
    outw, stw = run_tail(heads, mode, act, [weight_vector(w.tolist()) for w in ws])
    assert stw == st0
    for h, o, w in zip(heads, outw, ws):
        loss, row_w, dz = tail_reference_weighted(h, w)
        lv = o["row_lv"][:h.n_pool].cpu().double()
        grad = o["grad"][:h.n_rows].cpu().double()
        assert bool(torch.isfinite(lv).all()) and bool(torch.isfinite(grad).all())
        n_valid = max(1, int((row_w > 0).sum()))
        print(f"  rows {h.n_pool} classes {h.classes}: loss {float(lv[:, 0].sum()):.6f} (ref {float(loss):.6f})")
        torch.testing.assert_close(lv[:, 1], row_w.float().double(), atol=0, rtol=0)  # the row's weight itself: exact
        torch.testing.assert_close(lv[:, 0].sum(), loss, atol=ATOL * n_valid, rtol=RTOL)
        torch.testing.assert_close(grad[:, :h.classes], dz, atol=ATOL, rtol=RTOL)
        assert float(grad[:, h.classes:].abs().sum()) == 0.0


TAIL_ACTS = [(N, 0.0), (R, 0.25), (E, 0.25)]


@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("rows", ROWS)
def test_unpooled_tail_one_head(rows, classes):
    act, p = TAIL_ACTS[(rows + classes) % 3]
    h = tk.Tail(rows, classes, act, p, ldz_pad=8, ldg_pad=4, use_mask=classes % 2 == 1, seed=600 + rows)
    check_tail_forms([h], 0, act)


@pytest.mark.parametrize("c0,c1", [(5, 65), (256, 1), (64, 130), (255, 5)])
def test_unpooled_tail_two_heads(c0, c1):
    act, p = TAIL_ACTS[(c0 + c1) % 3]
    heads = [tk.Tail(17, c0, act, p, ldz_pad=8, use_mask=True, seed=700, slot=0),
             tk.Tail(67, c1, act, p, ldg_pad=4, use_mask=False, seed=701, slot=1)]
    check_tail_forms(heads, 0, act)


@pytest.mark.parametrize("profile,classes", [("ones", 1), ("mixed", 5), ("leaf012", 64), ("mixed", 65), ("mixed", 130), ("leaf012", 255),
                                             ("mixed", 256)])
def test_pooled_tail(profile, classes):
    act, p = TAIL_ACTS[classes % 3]
    h = tk.pooled_head(profile, classes, act, p, classes % 7, 0, True)
    check_tail_forms([h], 2, act)


# ---- linear heads ----------------------------------------------------------------------------------------------------------------
def run_heads(H, weights=None):
    out = H.outputs()
    state = torch.zeros(5, dtype=torch.int32, device=dev())
    nb = C.c_int32(-1)
    lib = _lib.load()
    if weights is None:
        rc = lib.hmp_linear_heads_run(C.byref(H.desc(out)), 1, state.data_ptr(), None, C.byref(nb), _lib.stream_ptr())
    else:
        rc = lib.hmp_linear_heads_run_weighted(C.byref(H.desc(out)), vp_array(weights), 1, state.data_ptr(), None, C.byref(nb),
                                               _lib.stream_ptr())
    assert rc == 0, lib.hmp_last_error()
    st = tk.sync_status(state)
    out["slabs"] = out["slabs"][:nb.value]
    return out, st


def heads_reference_weighted(H, ws, dtype=torch.float64):
    zl = H.z[:H.n_rows, :H.F].to(dtype).clone().requires_grad_(True)
    y = _act(zl, H.act)
    if H.p > 0:
        y = y * H.keep[:, :H.F].to(dtype) / (1.0 - H.p)
    m = torch.ones(H.n_rows, dtype=torch.bool) if H.mask is None else H.mask != 0
    members = head_members(H.n_rows, H.member[0], H.member[1])
    Ws = [w.to(dtype).clone().requires_grad_(True) for w in H.W]
    bs = [b.to(dtype).clone().requires_grad_(True) for b in H.b]
    loss = torch.zeros((), dtype=dtype)
    row_w = torch.zeros(H.n_rows, dtype=dtype)
    for h in range(2):
        Cn = H.classes[h]
        valid = members[h] & m & (H.labels != IGNORED) & (H.labels >= 0) & (H.labels < Cn)
        if int(valid.sum()):
            logits = y @ Ws[h].t() + bs[h]
            loss = loss + F.cross_entropy(logits[valid], H.labels[valid], weight=ws[h].to(dtype), reduction="sum")
            row_w = row_w + torch.where(valid, ws[h].to(dtype)[H.labels.clamp(0, Cn - 1)], torch.zeros_like(row_w))
    if loss.requires_grad:
        loss.backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)  # noqa: E731
    return loss.detach(), row_w, zero(zl), torch.cat([zero(w) for w in Ws]), torch.cat([zero(b) for b in bs])


@pytest.mark.parametrize("classes,F_,rows,members,act,p", [
    ((1, 1), 3, 1, "both_null", N, 0.0), ((3, 2), 30, 33, "second_null", R, 0.25), ((15, 35), 30, 67, "both_given", E, 0.25),
    ((64, 64), 65, 33, "both_given", R, 0.25), ((1, 64), 30, 17, "both_given", N, 0.0), ((64, 1), 3, 67, "both_given", R, 0.0),
])
def test_linear_heads(classes, F_, rows, members, act, p):
    H = tk.Heads(classes, F_, rows, act, p, ldz_pad=8, members=members, use_mask=rows % 2 == 1, seed=40 + rows)
    H.W = [w / 16 for w in H.W]  # logits inside +-5 (see the file's docstring); a power of two: ties stay ties
    H.d["W0"], H.d["W1"] = H.W[0].to(dev()), H.W[1].to(dev())
    out0, st0 = run_heads(H)

    def same(a, b):
        for k in ("grad", "row_lv", "slabs"):
            assert torch.equal(bits(a[k]), bits(b[k])), k

    same(run_heads(H, [weight_vector([1.0] * c) for c in classes])[0], out0)  # 1.
    same(run_heads(H, [None, None])[0], out0)
    outq, _ = run_heads(H, [weight_vector([0.25] * c) for c in classes])  # 2.
    assert torch.equal(bits(outq["row_lv"]), bits(out0["row_lv"] * 0.25))
    # 3. class 0 of both heads has weight 0 == label 0 ignored
    outz, stz = run_heads(H, [weight_vector([0.0] + [1.0] * (c - 1)) for c in classes])
    keep = H.d["labels"]
    lab = H.labels.clone()
    lab[lab == 0] = IGNORED
    H.d["labels"] = lab.to(dev())
    try:
        outi, sti = run_heads(H)
    finally:
        H.d["labels"] = keep
    same(outz, outi)
    assert stz == sti == st0  # 6.
    outn, _ = run_heads(H, [weight_vector([0.0] * c) for c in classes])  # 5.
    assert bool((outn["row_lv"] == 0).all()) and bool((outn["grad"] == 0).all())
    # 4. (and 6.: rows 2 and 3 of the larger cases carry the labels -1 and min(classes))
    ws = [random_weights(c, 5 + i) for i, c in enumerate(classes)]
    outw, stw = run_heads(H, [weight_vector(w.tolist()) for w in ws])
    assert stw == st0
    loss, row_w, dz, dW, db = heads_reference_weighted(H, ws)
    lv, grad, slabs = outw["row_lv"].cpu().double(), outw["grad"].cpu().double(), outw["slabs"].cpu().double()
    assert bool(torch.isfinite(lv).all()) and bool(torch.isfinite(grad).all())
    nb = slabs.shape[0]
    gW = slabs[:, :H.K * H.ld_slab].reshape(nb, H.K, H.ld_slab)[:, :, :H.F].sum(dim=0)
    gb = slabs[:, H.K * H.ld_slab:H.K * H.ld_slab + H.K].sum(dim=0)
    n_valid = max(1, int((row_w > 0).sum()))
    print(f"  heads {classes} F {F_} rows {rows}: loss {float(lv[:, 0].sum()):.6f} (ref {float(loss):.6f})")
    torch.testing.assert_close(lv[:, 1], row_w, atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(lv[:, 0].sum(), loss, atol=ATOL * n_valid, rtol=RTOL)
    torch.testing.assert_close(grad[:, :H.F], dz, atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(gW, dW, atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(gb, db, atol=ATOL, rtol=RTOL)
