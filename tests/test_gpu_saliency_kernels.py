"""GPU checks of the gradient-saliency unit entries: hmp_saliency_seed, hmp_saliency_scores, hmp_saliency_topk against the float64 /
exact restatements of tests/_saliency_reference.py.

Seed: the one-hot form only copies constants, so it is compared bit for bit; the log-probability form against float64 at the
project's standing ATOL = RTOL = 1e-5; padding columns and unselected rows are exactly 0 over a NaN-prefilled buffer.
Scores: against float64 at 1e-5 of the row's sum |g x| (the scale of what was added up); gnorm also at 1e-5 of its own value; a
rerun and every combination of requested outputs give the same bits.
Top-k: a function of the float32 scores that only compares and copies: equal to ``top_from_scores`` bit for bit, padding and
the prefill of unselected rows included."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib  # noqa: E402
from test_gpu_ops import build_plan, rand_edges  # noqa: E402
from test_gpu_gat_attention_kernels import edges_of  # noqa: E402
from _saliency_reference import (SEL_ALL, SEL_MASK, SEL_ORDINAL, WRT_LOGIT, WRT_LOGPROB, scores_reference, seed_reference,  # noqa: E402
                                 selected_rows, top_from_scores)

ATOL, RTOL = 1e-5, 1e-5
DEV = "cuda:0"


def ptr_of(t):
    return t.data_ptr() if t is not None else None


def selections(rng, n_rows):
    """(name, mode, mask, p, ptr) cases over n_rows rows: all, a random mask, and ordinals over a ptr with an empty graph, p = 0,
    a p beyond some graphs and a p beyond all"""
    yield "all", SEL_ALL, None, 0, None
    yield "mask", SEL_MASK, rng.integers(0, 2, n_rows).astype(bool), 0, None
    if n_rows == 0:
        yield "ordinal0", SEL_ORDINAL, None, 0, np.array([0, 0], dtype=np.int64)
        return
    cuts = np.sort(rng.integers(0, n_rows + 1, 3))
    ptr = np.concatenate([[0], cuts[:1], cuts[:1], cuts[1:], [n_rows]]).astype(np.int64)  # graph 1 is empty
    sizes = np.diff(ptr)
    for p in sorted({0, 1, int(sizes.max()) - 1, int(sizes.max())}):
        if p >= 0:
            yield f"ordinal{p}", SEL_ORDINAL, None, p, ptr


def run_seed(lib, z, n_rows, n_classes, ld_g, target, mode, mask, p, ptr, wrt):
    gout = torch.full((max(n_rows, 1), ld_g), float("nan"), device=DEV)
    tg = torch.from_numpy(target).to(DEV) if target is not None else None
    mk = torch.from_numpy(mask).to(DEV) if mask is not None else None
    pt = torch.from_numpy(ptr).to(DEV) if ptr is not None else None
    _lib.check(lib.hmp_saliency_seed(z.data_ptr(), z.stride(0), n_rows, n_classes, ptr_of(tg), mode, ptr_of(mk), p, ptr_of(pt),
                                     len(ptr) - 1 if ptr is not None else 0, wrt, gout.data_ptr(), ld_g, _lib.stream_ptr()))
    return gout[:n_rows].cpu().numpy()


@pytest.mark.parametrize("n_rows", [0, 1, 65])
@pytest.mark.parametrize("n_classes,ld,ld_g", [(1, 4, 4), (26, 28, 28), (26, 27, 40), (35, 36, 36), (35, 35, 37)])
def test_seed(n_classes, ld, ld_g, n_rows):
    lib = _lib.require_device()
    rng = np.random.default_rng(100 * n_classes + ld + n_rows)
    z = rng.normal(0, 2, size=(max(n_rows, 1), ld)).astype(np.float32)
    if n_rows > 3 and n_classes > 4:
        z[1, 3] = z[1, 9 % n_classes] = z[1].max() + 1.0          # two equal maxima: the first wins
        z[2, :] = 0.5                                               # a row of equal values: class 0
        z[3, :n_classes] = -np.abs(z[3, :n_classes])
        z[3, n_classes:] = 100.0                                    # padding larger than every class: never read
    zd = torch.from_numpy(z).to(DEV)
    target = rng.integers(0, n_classes, max(n_rows, 1)).astype(np.int64)
    if n_rows > 8:
        target[4], target[5], target[6] = -1, n_classes, 1 << 40   # out of range: the prediction instead
    pred = torch.empty(max(n_rows, 1), dtype=torch.int64, device=DEV)
    _lib.check(lib.hmp_predict_rows(zd.data_ptr(), ld, n_rows, n_classes, None, pred.data_ptr(), _lib.stream_ptr()))
    pred = pred[:n_rows].cpu().numpy()
    for (name, mode, mask, p, ptr), tg, wrt in itertools.product(selections(rng, n_rows), (None, target[:n_rows]), (WRT_LOGIT, WRT_LOGPROB)):
        got = run_seed(lib, zd, n_rows, n_classes, ld_g, None if tg is None else target, mode, mask, p, ptr, wrt)
        sel = selected_rows(n_rows, mode, mask, p, ptr)
        want, cls = seed_reference(z[:n_rows], n_classes, ld_g, tg, sel, wrt)
        tag = f"C={n_classes} ld={ld} ld_g={ld_g} rows={n_rows} {name} target={'y' if tg is not None else 'n'} wrt={wrt}"
        assert got.shape == (n_rows, ld_g) and not np.isnan(got).any(), tag
        assert (got[~sel] == 0).all() and (got[:, n_classes:] == 0).all(), f"{tag}: unselected rows / padding columns are not exactly 0"
        if tg is None:
            assert np.array_equal(cls, pred), f"{tag}: the reference argmax is not hmp_predict_rows'"
        if wrt == WRT_LOGIT:
            assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), f"{tag}: one-hot rows differ"
        else:
            err = np.abs(got.astype(np.float64) - want)
            print(f"{tag}: max |seed - ref| = {err.max() if err.size else 0.0:.3e}")
            torch.testing.assert_close(torch.from_numpy(got).double(), torch.from_numpy(want), atol=ATOL, rtol=RTOL, msg=lambda m: f"{tag}: {m}")
        if n_rows > 3 and n_classes > 4 and tg is None and sel[1] and sel[2] and wrt == WRT_LOGIT:
            assert got[1].argmax() == min(3, 9 % n_classes) and got[2, 0] == 1.0


def run_scores(lib, g, x, n, F, groups, want=(True, True, True)):
    ng = len(groups)
    lo = (C.c_int32 * max(ng, 1))(*[a for a, _ in groups])
    hi = (C.c_int32 * max(ng, 1))(*[b for _, b in groups])
    gxi = torch.full((max(n, 1),), float("nan"), device=DEV) if want[0] else None
    gn = torch.full((max(n, 1),), float("nan"), device=DEV) if want[1] else None
    gr = torch.full((max(n, 1), max(ng, 1)), float("nan"), device=DEV) if want[2] and ng else None
    _lib.check(lib.hmp_saliency_scores(g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), n, F, ng, lo, hi, ptr_of(gxi), ptr_of(gn),
                                       ptr_of(gr), _lib.stream_ptr()))
    cut = lambda t: t[:n].cpu().numpy() if t is not None else None  # noqa: E731
    return cut(gxi), cut(gn), cut(gr)


@pytest.mark.parametrize("n", [0, 1, 65])
@pytest.mark.parametrize("F,ldg,ldx", [(3, 3, 4), (6, 8, 6), (64, 64, 67), (306, 306, 308), (306, 309, 306)])
def test_scores(F, ldg, ldx, n):
    lib = _lib.require_device()
    rng = np.random.default_rng(10 * F + ldg + n)
    g = torch.from_numpy(rng.normal(0, 1, size=(max(n, 1), ldg)).astype(np.float32)).to(DEV)
    x = torch.from_numpy(rng.normal(0, 1, size=(max(n, 1), ldx)).astype(np.float32)).to(DEV)
    # the three feature blocks; an empty range, a ragged one and one clipped at F; the full row and a range past F; none
    for groups in (((0, 3), (3, 6), (6, F)), ((2, 2), (1, min(F, 70)), (F - 1, F + 50), (5, 3)), ((0, F), (F, F + 4)), ()):
        gxi, gn, gr = run_scores(lib, g, x, n, F, groups)
        ref_gxi, ref_gn, ref_gr, scale = scores_reference(g.cpu().numpy()[:n], x.cpu().numpy()[:n], F, groups)
        tag = f"F={F} ldg={ldg} ldx={ldx} n={n} groups={groups}"
        bound = ATOL * scale
        for name, got, ref in (("gxi", gxi, ref_gxi), ("gnorm", gn, ref_gn)) + ((("groups", gr, ref_gr),) if groups else ()):
            assert got is not None and not np.isnan(got).any(), f"{tag}: {name}"
            if name == "groups":
                got = got[:, :len(groups)]
            err = np.abs(got.astype(np.float64) - ref)
            b = bound if name != "groups" else bound[:, None]
            print(f"{tag}: {name} max err / sum|g x| = {(err / np.maximum(b / ATOL, 1e-300)).max() if err.size else 0.0:.3e}")
            assert (err <= b).all(), f"{tag}: {name} off by {err.max():.3e}"
        assert (np.abs(gn.astype(np.float64) - ref_gn) <= RTOL * ref_gn).all(), f"{tag}: gnorm against its own scale"
        for i, (lo, hi) in enumerate(groups):
            if min(hi, F) <= max(lo, 0):
                assert (gr[:, i] == 0).all(), f"{tag}: an empty range is not exactly 0"
        # a rerun, and every combination of requested outputs, hold the same bits
        bits = lambda a: a.view(np.uint32)  # noqa: E731
        again = run_scores(lib, g, x, n, F, groups)
        for a, b in zip((gxi, gn, gr), again):
            assert (a is None and b is None) or np.array_equal(bits(a), bits(b)), f"{tag}: a rerun differs"
        for want in itertools.product((False, True), repeat=3):
            part = run_scores(lib, g, x, n, F, groups, want)
            for w, a, b in zip(want, (gxi, gn, gr), part):
                if not w or a is None:
                    assert b is None
                else:
                    assert np.array_equal(bits(a), bits(b)), f"{tag}: outputs {want} differ from requesting all"


def run_topk(lib, plan, score, n_dst, k, mode=SEL_ALL, mask=None, p=0, ptr=None, want=(True, True), prefill=(-7, -7.0)):
    src = torch.full((max(n_dst, 1), k), prefill[0], dtype=torch.int64, device=DEV) if want[0] else None
    sc = torch.full((max(n_dst, 1), k), prefill[1], device=DEV) if want[1] else None
    mk = torch.from_numpy(mask).to(DEV) if mask is not None else None
    pt = torch.from_numpy(ptr).to(DEV) if ptr is not None else None
    _lib.check(lib.hmp_saliency_topk(plan["plan"], score.data_ptr(), k, mode, ptr_of(mk), p, ptr_of(pt), len(ptr) - 1 if ptr is not None else 0,
                                     ptr_of(src), ptr_of(sc), _lib.stream_ptr()))
    cut = lambda t: t[:n_dst].cpu().numpy() if t is not None else None  # noqa: E731
    return cut(src), cut(sc)


@pytest.mark.parametrize("shape", ["loops7", "deg80", "empty", "dropped"])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_topk(k, shape):
    lib = _lib.require_device()
    rng = np.random.default_rng(17 * k + len(shape))
    ei, n_src, n_dst, status = edges_of(shape, rng)
    plan = build_plan(ei.to(DEV), n_src, n_dst)
    assert plan["status"] == status
    score = rng.normal(0, 1, n_src).astype(np.float32)
    score[: n_src // 2] = np.round(score[: n_src // 2])          # many equal magnitudes, zeros among them ...
    score[1], score[2] = 1.0, -1.0                               # ... and opposite signs: the lower source first
    if n_src > 12:
        score[11], score[12] = -0.75, 0.75
    sd = torch.from_numpy(score).to(DEV)
    ein = ei.numpy()
    for name, mode, mask, p, ptr in selections(rng, n_dst):
        sel = selected_rows(n_dst, mode, mask, p, ptr)
        src, sc = run_topk(lib, plan, sd, n_dst, k, mode, mask, p, ptr)
        want_src, want_sc = top_from_scores(score, ein, n_src, n_dst, k, sel)
        tag = f"{shape} k={k} {name}"
        assert np.array_equal(src, want_src), f"{tag}: sources differ"
        assert np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32)), f"{tag}: scores differ"
        assert (src[~sel] == -7).all() and (sc[~sel] == -7.0).all(), f"{tag}: an unselected row lost its prefill"
        # one output alone holds what it holds next to the other
        only_src, none = run_topk(lib, plan, sd, n_dst, k, mode, mask, p, ptr, want=(True, False))
        none2, only_sc = run_topk(lib, plan, sd, n_dst, k, mode, mask, p, ptr, want=(False, True))
        assert none is None and none2 is None and np.array_equal(only_src, src) and np.array_equal(only_sc.view(np.uint32), sc.view(np.uint32))
    if shape == "deg80":
        deg = np.bincount(ein[1], minlength=n_dst)
        src, sc = run_topk(lib, plan, sd, n_dst, k)
        assert deg.max() > 16 and (src[3] == -1).all() and (sc[3] == 0).all() and (src[4, 1:] == -1).all()
        for d in range(3):  # more edges than sources: every source is listed once
            named = src[d][src[d] >= 0]
            assert len(set(named.tolist())) == len(named)
    if shape == "loops7":  # the duplicated edge lists its source once
        dup_dst = int(ein[1, 10])
        src, _ = run_topk(lib, plan, sd, n_dst, 8)
        named = src[dup_dst][src[dup_dst] >= 0]
        assert len(set(named.tolist())) == len(named) == len(set(ein[0][ein[1] == dup_dst].tolist()))
    # ordinal passes fill one output: the union of the passes is the ALL result
    if n_dst > 0:
        ptr = np.array([0, n_dst // 2, n_dst // 2, n_dst], dtype=np.int64)
        src = torch.full((n_dst, k), -7, dtype=torch.int64, device=DEV)
        sc = torch.full((n_dst, k), -7.0, device=DEV)
        pt = torch.from_numpy(ptr).to(DEV)
        for p in range(int(np.diff(ptr).max())):
            _lib.check(lib.hmp_saliency_topk(plan["plan"], sd.data_ptr(), k, SEL_ORDINAL, None, p, pt.data_ptr(), 3, src.data_ptr(),
                                             sc.data_ptr(), _lib.stream_ptr()))
        all_src, all_sc = run_topk(lib, plan, sd, n_dst, k)
        assert np.array_equal(src.cpu().numpy(), all_src) and np.array_equal(sc.cpu().numpy().view(np.uint32), all_sc.view(np.uint32))


def test_refusals():
    lib = _lib.require_device()
    rng = np.random.default_rng(5)
    plan = build_plan(rand_edges(rng, 10, 4, 4).to(DEV), 4, 4)
    z = torch.zeros(4, 8, device=DEV)
    a = z.data_ptr()
    for k in (0, 9, -1):
        assert lib.hmp_saliency_topk(plan["plan"], a, k, 0, None, 0, None, 0, a, a, _lib.stream_ptr()) == 1 and b"k = " in lib.hmp_last_error()
    assert lib.hmp_saliency_topk(plan["plan"], a, 3, 1, None, 0, None, 0, a, a, _lib.stream_ptr()) == 1 and b"mask" in lib.hmp_last_error()
    assert lib.hmp_saliency_topk(plan["plan"], a, 3, 2, None, 0, None, 0, a, a, _lib.stream_ptr()) == 1 and b"ordinal" in lib.hmp_last_error()
    assert lib.hmp_saliency_topk(plan["plan"], a, 3, 5, None, 0, None, 0, a, a, _lib.stream_ptr()) == 1 and b"selection mode" in lib.hmp_last_error()
    assert lib.hmp_saliency_seed(a, 8, 4, 8, None, 0, None, 0, None, 0, 2, a, 8, _lib.stream_ptr()) == 1 and b"wrt" in lib.hmp_last_error()
    assert lib.hmp_saliency_seed(a, 8, 4, 9, None, 0, None, 0, None, 0, 0, a, 12, _lib.stream_ptr()) == 1 and b"n_classes" in lib.hmp_last_error()
    assert lib.hmp_saliency_seed(a, 8, 4, 8, None, 0, None, 0, None, 0, 0, a, 4, _lib.stream_ptr()) == 1
    lo, hi = (C.c_int32 * 5)(), (C.c_int32 * 5)()
    assert lib.hmp_saliency_scores(a, 8, a, 8, 4, 8, 5, lo, hi, a, None, None, _lib.stream_ptr()) == 1 and b"column ranges" in lib.hmp_last_error()
    assert lib.hmp_saliency_scores(a, 4, a, 8, 4, 8, 0, None, None, a, None, None, _lib.stream_ptr()) == 1
