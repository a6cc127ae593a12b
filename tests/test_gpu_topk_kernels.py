"""The top-k launchers driven directly (hmp_topk_rows, hmp_head_tails_topk, hmp_linear_heads_topk): topk_rows_kernel
(csrc/evaluate.hip), tail_topk_kernel and pool_topk_kernel (csrc/semisup.hip) and linear_heads_kernel<HL_TOPK> (csrc/heads.hip)
against the float64 reference of tests/_topk_reference.py, which states the tolerances and the rows left out of the order check.

The cases (final states, pools, weights, member masks) are those of tests/test_gpu_predict_kernels.py plus rows whose maximum is
shared by more than k columns.  Every output starts as a sentinel with 8 sentinel rows behind it: each element of rows [0, n) must
be overwritten and nothing past n touched.  The padding columns hold NaN and 1e30 in turn.  Column 0 is compared with the predict
launcher's output exactly, on every row.  ELU cases keep k <= 3."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from _tail_reference import head_members  # noqa: E402
from _topk_reference import check_topk, head_scores, order_rows, stable_order, tail_scores, yard_of  # noqa: E402
from hydra_gnn_amd import _lib  # noqa: E402
from test_gpu_predict_kernels import E, N, R, Heads, Tail, align4, dev, pool_edges, ptr, run_tails  # noqa: E402

SENT = -7
TAILROWS = 8
HMP_E_ARG = 1
CLASSES = [1, 2, 3, 4, 5, 63, 64, 65, 66, 130]
ROWS = [0, 1, 15, 16, 17]


def ks_of(act):
    return [1, 3] if act == E else [1, 2, 3, 8]


def sentinels(n, k):
    k = max(k, 1)  # (a refused k still gets buffers to find untouched)
    return (torch.full((n + TAILROWS, k), SENT, dtype=torch.int64, device=dev()),
            torch.full((n + TAILROWS, k), float(SENT), dtype=torch.float32, device=dev()))


def written(out, n, tag):
    """host rows [0, n) of a sentinel-filled output: every element overwritten, nothing behind them touched"""
    h = out.cpu()
    assert bool((h[n:] == SENT).all()), f"{tag}: an element past row n = {n} was written"
    assert bool((h[:n] != SENT).all()), f"{tag}: an element below row n = {n} was not written"
    return h[:n]


def shared_maximum_rows(z, n_rows, classes, act):
    """row 11: every second column shares the maximum (more than k columns from 2 k classes on); row 12: every column ties; row 13:
    the maximum three times, 64 columns apart (three passes of a 16-lane group), with a tied pair below it"""
    if act == E or n_rows < 15:
        return
    z[11, :classes] = -1.0
    z[11, 0:classes:2] = 2.0
    z[12, :classes] = 1.0
    z[13, :classes] = -2.0
    for c in (1, 65, 129):
        if c < classes:
            z[13, c] = 3.5
    if classes >= 5:
        z[13, 2] = z[13, 4] = 0.5


# ---- hmp_topk_rows ----------------------------------------------------------------------------------------------------------------
def rows_case(n_rows, classes, seed):
    """scores on the CPU [n_rows, classes]: multiples of 1/4 (ties are frequent), some +0.0 / -0.0, the shared-maximum rows"""
    g = torch.Generator().manual_seed(5000 + 17 * seed + classes)
    x = torch.randint(-16, 17, (max(n_rows, 1), classes), generator=g).float() / 4
    u = torch.rand(max(n_rows, 1), classes, generator=g)
    x[u < 0.05] = 0.0
    x[(u >= 0.05) & (u < 0.1)] = -0.0
    shared_maximum_rows(x, n_rows, classes, N)
    return x[:n_rows]


def padded(x, ld):
    """x in a [rows + 1, ld] device buffer, NaN / 1e30 in the padding columns and the spare row; the view of its rows"""
    buf = torch.full((x.shape[0] + 1, ld), float("nan"))
    buf[:, 1::2] = 1e30
    buf[:x.shape[0], :x.shape[1]] = x
    return buf.to(dev())


def run_rows(buf, ld, n_rows, classes, members, k, labels=True, probs=True):
    lab, prb = sentinels(n_rows, k)
    rc = _lib.load().hmp_topk_rows(buf.data_ptr(), ld, n_rows, classes, ptr(members), k, lab.data_ptr() if labels else None,
                                   prb.data_ptr() if probs else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, lab, prb


def predict_rows(buf, ld, n_rows, classes, members):
    out = torch.full((n_rows + 1,), SENT, dtype=torch.int64, device=dev())
    _lib.check(_lib.load().hmp_predict_rows(buf.data_ptr(), ld, n_rows, classes, ptr(members), out.data_ptr(), _lib.stream_ptr()))
    return out[:n_rows].cpu()


@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("classes", CLASSES)
def test_topk_rows(classes, k):
    """pitch aligned to 4 (quad walk, with and without padding) and not (scalar walk); members NULL and with the first and last
    row out; the scalar walk owns the same columns per lane: its probabilities are the quad walk's bit for bit"""
    for i, n_rows in enumerate(ROWS):
        x = rows_case(n_rows, classes, seed=i)
        s64 = x.double()
        use = order_rows(s64, k, 0.0, "rows")
        mem = torch.ones(n_rows, dtype=torch.bool)
        if n_rows:
            mem[0] = mem[-1] = False
        first = None
        for pad in (0, 8, 1, 3):
            ld = align4(classes) + pad
            buf = padded(x, ld)
            for members in (None, mem):
                tag = f"topk_rows {n_rows}x{classes} k {k} ld {ld} members {members is not None}"
                d_mem = members.to(dev()) if members is not None else None
                rc, lab, prb = run_rows(buf, ld, n_rows, classes, d_mem, k)
                assert rc == 0, _lib.load().hmp_last_error()
                lab, prb = written(lab, n_rows, tag), written(prb, n_rows, tag)
                if n_rows == 0:
                    continue
                assert torch.equal(lab[:, 0], predict_rows(buf, ld, n_rows, classes, d_mem)), f"{tag}: column 0 is not the predicted label"
                check_topk(lab, prb, s64, k, 0.0, use, tag, members)
                if members is None:
                    if first is None:
                        first = (lab, prb)
                    assert torch.equal(lab, first[0]) and torch.equal(prb, first[1]), f"{tag}: the result depends on the pitch"
        if n_rows >= 15 and classes >= 2:
            lab = first[0]
            assert lab[11, :min(k, (classes + 1) // 2)].tolist() == list(range(0, classes, 2))[:k]  # a maximum shared by > k columns
            assert lab[12, :min(k, classes)].tolist() == list(range(min(k, classes)))
            assert float((first[1][12, :min(k, classes)].double() - 1.0 / classes).abs().max()) <= 1e-7  # every column ties: 1 / C


@pytest.mark.parametrize("pad", [0, 3])
def test_topk_rows_past_one_pass_of_the_grid(pad):
    """16401 rows: more than the grid's 1024 x 16, so workgroups stride over rows"""
    n_rows, classes, k = 16401, 26, 3
    x = rows_case(n_rows, classes, seed=9)
    ld = align4(classes) + pad
    buf = padded(x, ld)
    mem = torch.rand(n_rows, generator=torch.Generator().manual_seed(1)) < 0.6
    mem[0] = mem[-1] = False
    rc, lab, prb = run_rows(buf, ld, n_rows, classes, mem.to(dev()), k)
    assert rc == 0, _lib.load().hmp_last_error()
    lab, prb = written(lab, n_rows, "strided"), written(prb, n_rows, "strided")
    assert torch.equal(lab[:, 0], predict_rows(buf, ld, n_rows, classes, mem.to(dev())))
    check_topk(lab, prb, x.double(), k, 0.0, torch.ones(n_rows, dtype=torch.bool), f"topk_rows strided ld {ld}", mem)


def test_topk_rows_skips_a_null_output():
    x = rows_case(17, 26, seed=3)
    buf = padded(x, 28)
    rc, lab, prb = run_rows(buf, 28, 17, 26, None, 3)
    assert rc == 0
    rc, lab1, prb1 = run_rows(buf, 28, 17, 26, None, 3, probs=False)
    assert rc == 0 and torch.equal(lab1, lab) and bool((prb1 == SENT).all())
    rc, lab2, prb2 = run_rows(buf, 28, 17, 26, None, 3, labels=False)
    assert rc == 0 and torch.equal(prb2, prb) and bool((lab2 == SENT).all())


# ---- unpooled tail ----------------------------------------------------------------------------------------------------------------
def run_tail_topk(heads, pooled, act, k, descs=None, labels=True, probs=True):
    outs = [sentinels(h.n_out if pooled else h.n_rows, k) for h in heads]
    arr = (_lib.TailDesc * len(heads))(*(descs or [h.desc(pooled) for h in heads]))
    lab = (C.c_void_p * len(heads))(*[o[0].data_ptr() if labels else None for o in outs])
    prb = (C.c_void_p * len(heads))(*[o[1].data_ptr() if probs else None for o in outs])
    rc = _lib.load().hmp_head_tails_topk(arr, len(heads), int(pooled), act, k, lab, prb, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, outs


def tail_case(n_rows, classes, act, seed, ldz_pad=0):
    h = Tail(n_rows, classes, act, seed=seed, ldz_pad=ldz_pad)
    shared_maximum_rows(h.z, n_rows, classes, act)
    h.d_z = h.z.to(dev())
    return h


def check_tail(h, pooled, act, k, outs, pred, yard, use, tag):
    n = h.n_out if pooled else h.n_rows
    lab, prb = written(outs[0], n, tag), written(outs[1], n, tag)
    if n == 0:
        return lab, prb
    assert torch.equal(lab[:, 0], pred), f"{tag}: column 0 is not the predicted label"
    s64 = tail_scores(h.z[:h.n_rows], h.classes, act, h.pool if pooled else None)
    check_topk(lab, prb, s64, k, yard, use, tag)
    return lab, prb


@pytest.mark.parametrize("act", [N, R, E])
@pytest.mark.parametrize("classes", CLASSES)
def test_unpooled_tail(classes, act):
    """the kernel reads the z the reference reads and the activation is monotone: the order of every row is compared exactly"""
    for i, n_rows in enumerate(ROWS):
        h = tail_case(n_rows, classes, act, seed=i, ldz_pad=8 * (i % 2))
        s64 = tail_scores(h.z[:n_rows], classes, act)
        s32 = tail_scores(h.z[:n_rows], classes, act, dtype=torch.float32)
        yard = yard_of(s32, s64)
        assert yard == 0.0 or act == E
        assert torch.equal(stable_order(s32)[:, :4], stable_order(s64)[:, :4])  # the float32 activation keeps the reference's order
        use = torch.ones(n_rows, dtype=torch.bool)
        rc, pred = run_tails([h], False, act)
        assert rc == 0, _lib.load().hmp_last_error()
        for k in ks_of(act):
            tag = f"tail {n_rows}x{classes} act {act} k {k}"
            rc, outs = run_tail_topk([h], False, act, k)
            assert rc == 0, _lib.load().hmp_last_error()
            lab, prb = check_tail(h, False, act, k, outs[0], pred[0][:n_rows].cpu(), yard, use, tag)
            if act == R and n_rows >= 15:
                kk = min(k, classes)
                assert lab[10, :kk].tolist() == list(range(kk))  # all negative behind ReLU: a row of zeros, labels 0 .. k-1
                assert float((prb[10, :kk].double() - 1.0 / classes).abs().max()) <= 1e-7  # ... with equal probabilities


@pytest.mark.parametrize("rows,classes,act,k", [((17, 33), (5, 70), R, 8), ((0, 40), (64, 5), N, 3), ((40, 0), (65, 130), E, 2),
                                                ((33, 17), (1, 35), R, 2)])
def test_two_heads_ride_in_one_launch(rows, classes, act, k):
    """(17, 33): entry 1 starts in block 2; (0, 40) / (40, 0): an entry without rows next to a full one (block_start)"""
    heads = [tail_case(rows[0], classes[0], act, seed=20, ldz_pad=8), tail_case(rows[1], classes[1], act, seed=21)]
    rc, pred = run_tails(heads, False, act)
    assert rc == 0, _lib.load().hmp_last_error()
    rc, outs = run_tail_topk(heads, False, act, k)
    assert rc == 0, _lib.load().hmp_last_error()
    for h, o, p in zip(heads, outs, pred):
        yard = yard_of(tail_scores(h.z[:h.n_rows], h.classes, act, dtype=torch.float32), tail_scores(h.z[:h.n_rows], h.classes, act))
        check_tail(h, False, act, k, o, p[:h.n_rows].cpu(), yard, torch.ones(h.n_rows, dtype=torch.bool), f"tails {rows} x {classes} k {k}")


# ---- pooled tail ------------------------------------------------------------------------------------------------------------------
def pooled_case(classes, act, seed, k):
    """(head, yard, rows whose order is compared): the 1 % cap is asserted here, before anything is launched"""
    n_leaves, n_pool, edges = pool_edges(seed)
    h = Tail(n_leaves, classes, act, seed=seed, ldz_pad=8 * (seed % 2), pool=(n_pool, edges))
    s64 = tail_scores(h.z[:h.n_rows], classes, act, h.pool)
    yard = yard_of(tail_scores(h.z[:h.n_rows], classes, act, h.pool, dtype=torch.float32), s64)
    # without ELU the sums are exact (multiples of 1/4) and the one division is monotone: every row's order is compared
    return h, yard, order_rows(s64, k, yard if act == E else 0.0, f"pool {classes} act {act} k {k}")


@pytest.mark.parametrize("act", [N, R, E])
@pytest.mark.parametrize("classes", [1, 3, 5, 64, 65, 130, 256])
def test_pooled_tail(classes, act):
    for k in ks_of(act):
        h, yard, use = pooled_case(classes, act, classes % 7 + act, k)
        tag = f"pool {classes} act {act} k {k}"
        rc, pred = run_tails([h], True, act)
        assert rc == 0, _lib.load().hmp_last_error()
        rc, outs = run_tail_topk([h], True, act, k)
        assert rc == 0, _lib.load().hmp_last_error()
        lab, prb = check_tail(h, True, act, k, outs[0], pred[0][:h.n_pool].cpu(), yard, use, tag)
        kk = min(k, classes)
        assert int(h.csr[0][1]) == 0  # pooled row 0 has no leaf: all zeros, labels 0 .. k-1, each 1 / C
        assert lab[0, :kk].tolist() == list(range(kk))
        assert float((prb[0, :kk].double() - 1.0 / classes).abs().max()) <= 1e-7


@pytest.mark.parametrize("classes,act,k", [((65, 5), R, 8), ((5, 256), E, 3)])
def test_identity_pool_next_to_a_real_one(classes, act, k):
    pooled, yard, use = pooled_case(classes[0], act, 3, k)
    ident = Tail(33, classes[1], act, seed=31, ldz_pad=8)  # rowptr NULL: row v's only leaf is v
    iy = yard_of(tail_scores(ident.z[:33], classes[1], act, dtype=torch.float32), tail_scores(ident.z[:33], classes[1], act))
    for heads in ([pooled, ident], [ident, pooled]):
        rc, pred = run_tails(heads, True, act)
        assert rc == 0, _lib.load().hmp_last_error()
        rc, outs = run_tail_topk(heads, True, act, k)
        assert rc == 0, _lib.load().hmp_last_error()
        for h, o, p in zip(heads, outs, pred):
            if h is pooled:
                check_tail(h, True, act, k, o, p[:h.n_pool].cpu(), yard, use, f"pool+identity {classes} k {k}")
            else:
                lab, prb = written(o[0], 33, "identity"), written(o[1], 33, "identity")
                assert torch.equal(lab[:, 0], p[:33].cpu())
                check_topk(lab, prb, tail_scores(h.z[:33], h.classes, act), k, iy, torch.ones(33, dtype=torch.bool), f"identity {classes} k {k}")


# ---- linear heads -----------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [((15, 35), 16), ((1, 64), 80), ((15, 35), 768), ((2, 3), 20)]
HEAD_ROWS = [1, 31, 33, 7681]
# activation and k per (shape, row count).  ELU keeps k <= 3.  F = 768 meets ELU at 31 rows, not at 7681: its logits reach |50|, where
# the kernel's logits -- when these cases were chosen, one 768-term fmaf chain; since then summed per 64-column chunk -- were further from
# float64 than the blocked sum of the host's float32 matmul, the yardstick.  Measured at 7681 rows with the chain: probabilities off by
# 3.6e-5 against a tolerance of 4.1e-5 that moves with the host's BLAS -- a property of the logits of pass 1 (unchanged by the top-k
# mode; tests/test_gpu_tail_kernels.py measures its cross entropy), not of the top-k behind them.
HEAD_ACTS = [[R, E, N, E], [E, N, E, R], [N, E, R, N], [E, R, E, N]]
HEAD_KS = [[3, 1, 8, 3], [1, 8, 3, 2], [8, 3, 2, 1], [3, 2, 1, 8]]


def run_heads_topk(H, desc, k, labels=(True, True), probs=(True, True)):
    outs = [sentinels(H.n_rows, k), sentinels(H.n_rows, k)]
    lab = (C.c_void_p * 2)(*[o[0].data_ptr() if on else None for o, on in zip(outs, labels)])
    prb = (C.c_void_p * 2)(*[o[1].data_ptr() if on else None for o, on in zip(outs, probs)])
    nb = C.c_int32(-1)
    rc = _lib.load().hmp_linear_heads_topk(C.byref(desc), k, lab, prb, C.byref(nb), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, outs, nb.value


def heads_case(H, k, tag):
    """(float64 logits, yard, rows whose order is compared) per head, from the reference alone"""
    l64 = head_scores(H.z[:H.n_rows], H.F, H.W, H.b, H.act)
    l32 = head_scores(H.z[:H.n_rows], H.F, H.W, H.b, H.act, dtype=torch.float32)
    yard = max(yard_of(a, b) for a, b in zip(l32, l64))
    assert H.act == E or yard == 0.0  # multiples of 1/4 and 1/8: the float32 sums are exact
    return l64, yard, [order_rows(l, k, yard, f"{tag} head {h}") for h, l in enumerate(l64)]


@pytest.mark.parametrize("n_rows", HEAD_ROWS)
@pytest.mark.parametrize("shape", range(len(HEAD_SHAPES)))
def test_linear_heads(shape, n_rows):
    """7681 rows = 240 tiles + 1: one workgroup takes a second tile.  Classes 0 and 1 of a head duplicate their weight rows: an
    exact tie on every row, class 0 always directly in front of class 1"""
    classes, F = HEAD_SHAPES[shape]
    act, k = HEAD_ACTS[shape][HEAD_ROWS.index(n_rows)], HEAD_KS[shape][HEAD_ROWS.index(n_rows)]
    assert k <= 3 or act != E
    H = Heads(classes, F, n_rows, act, seed=10 * shape + n_rows % 7)
    tag = f"heads {classes} F {F} rows {n_rows} act {act} k {k}"
    l64, yard, use = heads_case(H, k, tag)
    for pattern, (m0, m1) in H.patterns.items():
        desc = H.desc(pattern)
        pred = [torch.full((n_rows + 1,), SENT, dtype=torch.int64, device=dev()) for _ in range(2)]
        prd = (C.c_void_p * 2)(*[p.data_ptr() for p in pred])
        assert _lib.load().hmp_linear_heads_predict(C.byref(desc), prd, None, _lib.stream_ptr()) == 0
        rc, outs, nb = run_heads_topk(H, desc, k)
        assert rc == 0, _lib.load().hmp_last_error()
        assert nb == min(-(-n_rows // 32), 240)
        members = head_members(n_rows, m0, m1)
        for h in range(2):
            t = f"{tag} {pattern} head {h}"
            lab, prb = written(outs[h][0], n_rows, t), written(outs[h][1], n_rows, t)
            assert torch.equal(lab[:, 0], pred[h][:n_rows].cpu()), f"{t}: column 0 is not the predicted label"
            check_topk(lab, prb, l64[h], k, yard, use[h], t, members[h])
            if classes[h] >= 2 and k >= 2:  # the duplicated class follows its original at once, on every row that names either
                on = members[h]
                pos0 = (lab[on] == 0).float().argmax(dim=1)
                has0 = (lab[on] == 0).any(dim=1) & (pos0 + 1 < min(k, classes[h]))
                nxt = lab[on].gather(1, (pos0 + 1).clamp(max=k - 1)[:, None])[:, 0]
                assert bool((nxt[has0] == 1).all()), f"{t}: class 1 does not follow class 0"


def test_linear_heads_without_rows_launch_nothing():
    H = Heads((15, 35), 16, 0, R, seed=5)
    rc, outs, nb = run_heads_topk(H, H.desc("both_given"), 3)
    assert rc == 0 and nb == 0 and untouched(outs)


def test_linear_heads_skip_null_outputs():
    H = Heads((15, 35), 16, 33, R, seed=77)
    desc = H.desc("both_given")
    rc, full, _ = run_heads_topk(H, desc, 3)
    assert rc == 0
    rc, outs, _ = run_heads_topk(H, desc, 3, labels=(False, True), probs=(False, False))  # head 0 skipped, head 1 labels alone
    assert rc == 0
    assert bool((outs[0][0] == SENT).all()) and bool((outs[0][1] == SENT).all()) and bool((outs[1][1] == SENT).all())
    assert torch.equal(outs[1][0], full[1][0])
    rc, outs, _ = run_heads_topk(H, desc, 3, labels=(False, False), probs=(True, False))  # head 0 probabilities alone
    assert rc == 0 and torch.equal(outs[0][1], full[0][1]) and bool((outs[1][0] == SENT).all()) and bool((outs[1][1] == SENT).all())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def untouched(outs):
    return all(bool((t == SENT).all()) for o in outs for t in o)


def test_topk_launchers_refuse_and_launch_nothing():
    lib = _lib.load()
    ok = Tail(20, 5, R, seed=41)
    wide = Tail(20, 257, R, seed=40)
    H = Heads((3, 2), 64, 40, R, seed=42)
    x = torch.zeros(8, 8, device=dev())
    for k in (0, 9, -1):
        rc, outs = run_tail_topk([ok], False, R, k)
        assert rc == HMP_E_ARG and b"k = " in lib.hmp_last_error() and untouched(outs)
        rc, outs = run_tail_topk([ok], True, R, k)
        assert rc == HMP_E_ARG and untouched(outs)
        rc, outs, _ = run_heads_topk(H, H.desc("both_given"), k)
        assert rc == HMP_E_ARG and b"k = " in lib.hmp_last_error() and untouched(outs)
        rc, lab, prb = run_rows(x, 8, 8, 5, None, k)
        assert rc == HMP_E_ARG and b"k = " in lib.hmp_last_error() and untouched([(lab, prb)])
    rc, outs = run_tail_topk([wide], True, R, 3)  # pooled rows are held in registers: at most 256 classes
    assert rc == HMP_E_ARG and b"257 classes" in lib.hmp_last_error() and untouched(outs)
    rc, outs = run_tail_topk([ok, wide], True, R, 3)  # refused as the second entry too: the first must not have run
    assert rc == HMP_E_ARG and untouched(outs)
    for over in (dict(z=ok.d_z.data_ptr() + 4), dict(ldz=6), dict(ldz=4), dict(classes=0)):
        rc, outs = run_tail_topk([ok], False, R, 3, descs=[ok.desc(False, **over)])
        assert rc == HMP_E_ARG and untouched(outs), over
    rc, outs = run_tail_topk([ok], True, R, 3, descs=[ok.desc(True, n_pool=19)])  # an identity pool has a row per leaf
    assert rc == HMP_E_ARG and untouched(outs)
    rc, outs = run_tail_topk([ok], False, R, 3, labels=False, probs=False)  # rows without any output
    assert rc == HMP_E_ARG and untouched(outs)
    assert lib.hmp_head_tails_topk(None, 1, 0, R, 3, None, None, None) == HMP_E_ARG
    for msg, over in ((b"linear heads: F = 1025", dict(F=1025, ldz=1028)), (b"final state", dict(ldz=62))):
        rc, outs, _ = run_heads_topk(H, H.desc("both_given", **over), 3)
        assert rc == HMP_E_ARG and msg in lib.hmp_last_error() and untouched(outs), over
    assert lib.hmp_linear_heads_topk(None, 3, None, None, None, None) == HMP_E_ARG
    rc, lab, prb = run_rows(x, 4, 8, 5, None, 3)  # ld < classes
    assert rc == HMP_E_ARG and untouched([(lab, prb)])
    rc, lab, prb = run_rows(x, 8, 8, 5, None, 3, labels=False, probs=False)  # no output at all
    assert rc == HMP_E_ARG
    assert lib.hmp_topk_rows(None, 8, 8, 5, None, 3, lab.data_ptr(), prb.data_ptr(), _lib.stream_ptr()) == HMP_E_ARG
    torch.cuda.synchronize()
    assert untouched([(lab, prb)])
    rc, outs = run_tail_topk([ok], False, R, 3)  # and the launchers still run
    assert rc == 0 and not untouched(outs)
