"""The label launchers driven directly (hmp_head_tails_predict, hmp_linear_heads_predict, hmp_predict_rows): tail_predict_kernel and
pool_predict_kernel (csrc/semisup.hip), linear_heads_kernel<HL_PREDICT> (csrc/heads.hip) and predict_rows_kernel (csrc/evaluate.hip)
against the float64 reference of tests/_tail_reference.py (tail_reference(...)["pred"], the heads' logits, _first_argmax).

Every output buffer starts as a sentinel: each row in [0, n) must be overwritten and nothing past n touched.  The padding columns
of the final state hold NaN and 1e30 in turn (the kernels may load them, never use them).

Which rows are compared.  An unpooled tail reads the z the reference reads and the activation is monotone: every row is compared,
exactly.  A pooled mean and a head's logits are float32 sums, so a row (and head) whose float64 top-two gap is at most 64 x the
largest |float32 yardstick - float64| entry of the case's rows is left out, at most 1 % of the case's rows (asserted on the CPU
before anything is launched).  The yardstick is the same formulas in float32 as tests/_tail_reference.py writes them.  One kind of
row inside that bound is compared all the same: an exact float64 tie of the maximum (gap 0) whose next entry BELOW the maximum is
further away than the bound must predict the first of the tied classes -- the ties of these cases are built from equal operands
(an empty pooled row, a row of zeros behind ReLU, duplicated weight rows), which are equal in float32 too.  Cases without ELU draw
z from multiples of 1/4 and W, b from multiples of 1/8, so their float32 sums are exact and the bound is 0."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _tail_reference import (ACT_ELU, ACT_NONE, ACT_RELU, _first_argmax, _top2_gap, _y, head_members, linear_heads_reference,  # noqa: E402
                             pool_csr_csc, tail_reference)
from hydra_gnn_amd import _lib  # noqa: E402

NAN = float("nan")
SENTINEL = -7
TAIL = 8  # sentinel rows behind every output
HMP_E_ARG = 1
N, R, E = ACT_NONE, ACT_RELU, ACT_ELU


def dev():
    return torch.device("cuda:0")


def align4(x):
    return (x + 3) & ~3


def ptr(t):
    return t.data_ptr() if t is not None else None


def sentinel(n):
    return torch.full((n + TAIL,), SENTINEL, dtype=torch.int64, device=dev())


def check_written(out, n, tag):
    """host labels of rows [0, n): all overwritten, nothing behind them touched"""
    h = out.cpu()
    assert bool((h[n:] == SENTINEL).all()), f"{tag}: a row past n = {n} was written"
    assert bool((h[:n] != SENTINEL).all()), f"{tag}: a row below n = {n} was not written"
    return h[:n]


def make_z(g, n_rows, width, ld, act):
    """final state [n_rows, ld] on the CPU: multiples of 1/4 in [-4, 4] (ELU: normal draws), some exact +0.0 / -0.0, NaN and 1e30
    alternating in the padding columns"""
    n = max(n_rows, 1)
    z = torch.randn(n, ld, generator=g) * 1.5 if act == E else torch.randint(-16, 17, (n, ld), generator=g).float() / 4
    u = torch.rand(n, ld, generator=g)
    z[u < 0.03] = 0.0
    z[(u >= 0.03) & (u < 0.06)] = -0.0
    pad = z[:, width:]
    pad[:] = NAN
    pad[(torch.arange(n)[:, None] + torch.arange(ld - width)[None, :]) % 2 == 1] = 1e30
    return z


def tie_rows(z, n_rows, classes, act):
    """rows 5 .. 9 share their maximum between two columns (inside a quad, across lanes, 64 columns apart, the last two); row 10 is
    all negative: behind ReLU a row of zeros, class 0"""
    if act == E or n_rows < 15:
        return
    if classes >= 2:
        for r, (a, b) in zip(range(5, 10), [(0, 1), (1, 5), (2, 66), (3, 129), (classes - 2, classes - 1)]):
            if b < classes:
                z[r, :classes] = -1.0
                z[r, a] = z[r, b] = 3.0
    z[10, :classes] = -torch.arange(1, classes + 1).float() / 4  # the maximum of z is class 0 too, the ReLU tie covers all


class Tail:
    def __init__(self, n_rows, classes, act, seed, ldz_pad=0, pool=None):
        g = torch.Generator().manual_seed(9000 + 131 * seed + classes)
        self.n_rows, self.classes, self.act = n_rows, classes, act
        self.ldz = align4(classes) + ldz_pad
        self.z = make_z(g, n_rows, classes, self.ldz, act)
        self.pool, self.n_pool, self.d_csr = None, n_rows, None
        if pool is not None:
            self.n_pool = pool[0]
            self.csr = pool_csr_csc(pool[0], n_rows, pool[1])
            self.pool = self.csr[:2]
            self.d_csr = [torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, np.int32))).to(dev()) for a in self.csr[:2]]
        else:
            tie_rows(self.z, n_rows, classes, act)
        self.d_z = self.z.to(dev())
        self.n_out = self.n_pool

    def reference(self):
        """float64 tail_reference: pred and gap per output row"""
        return tail_reference(self.z[:self.n_rows], self.classes, self.act, None, 0.0, torch.zeros(self.n_pool, dtype=torch.int64), None,
                              -100, pool=self.pool)

    def rows(self, dtype):
        """the pooled rows by the formulas of tail_reference (its lines for y and the segment mean), in dtype"""
        _, y = _y(self.z[:self.n_rows], self.classes, self.act, None, 0.0, dtype)
        rowptr = torch.as_tensor(np.asarray(self.pool[0]), dtype=torch.int64)
        col = torch.as_tensor(np.asarray(self.pool[1]), dtype=torch.int64)
        deg = rowptr[1:] - rowptr[:-1]
        seg = torch.repeat_interleave(torch.arange(self.n_pool), deg)
        return (torch.zeros(self.n_pool, self.classes, dtype=dtype).index_add(0, seg, y[col]) / deg.clamp(min=1).to(dtype)[:, None]).detach()

    def desc(self, pooled, **over):
        d = _lib.TailDesc(z=ptr(self.d_z), ldz=self.ldz, n_rows=self.n_rows, classes=self.classes)
        if pooled:
            d.n_pool = self.n_pool
            if self.pool is not None:  # the CSR alone: the label launch never walks the plan by leaf
                d.rowptr, d.col = [ptr(t) for t in self.d_csr]
        for k, v in over.items():
            setattr(d, k, v)
        return d


def run_tails(heads, pooled, act, descs=None):
    outs = [sentinel(h.n_out if pooled else h.n_rows) for h in heads]
    arr = (_lib.TailDesc * len(heads))(*(descs or [h.desc(pooled) for h in heads]))
    prd = (C.c_void_p * len(heads))(*[o.data_ptr() for o in outs])
    rc = _lib.load().hmp_head_tails_predict(arr, len(heads), int(pooled), act, prd, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, outs


# ---- unpooled tail ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [N, R, E])
@pytest.mark.parametrize("classes", [1, 5, 15, 35, 64, 65, 130])
def test_unpooled_tail_labels_are_exact(classes, act):
    """row-group and workgroup tails (1, 15, 16, 17, 33 rows), ldz with padding; no row is excluded"""
    for i, n_rows in enumerate([1, 15, 16, 17, 33]):
        h = Tail(n_rows, classes, act, seed=i, ldz_pad=8 * (i % 2))
        ref = h.reference()
        rc, outs = run_tails([h], False, act)
        assert rc == 0, _lib.load().hmp_last_error()
        got = check_written(outs[0], n_rows, f"tail {n_rows}x{classes} act {act}")
        assert torch.equal(got, ref["pred"]), f"tail {n_rows}x{classes} act {act}: {got.tolist()} != {ref['pred'].tolist()}"
        if act == R and n_rows >= 15:
            assert int(got[10]) == 0  # all negative behind ReLU: a row of zeros, the first index wins
            if classes >= 2:
                assert int(got[5]) == 0  # a duplicated maximum predicts the first


@pytest.mark.parametrize("rows,classes,act", [((17, 33), (5, 70), R), ((0, 40), (64, 5), N), ((40, 0), (65, 130), E), ((33, 17), (1, 35), R)])
def test_two_heads_ride_in_one_launch(rows, classes, act):
    """(17, 33): entry 1 starts in block 2; (0, 40) / (40, 0): an entry without rows next to a full one (block_start)"""
    heads = [Tail(rows[0], classes[0], act, seed=20, ldz_pad=8), Tail(rows[1], classes[1], act, seed=21)]
    rc, outs = run_tails(heads, False, act)
    assert rc == 0, _lib.load().hmp_last_error()
    for h, o in zip(heads, outs):
        got = check_written(o, h.n_rows, f"tails {rows} x {classes}")
        assert torch.equal(got, h.reference()["pred"][:h.n_rows])


# ---- pooled tail ------------------------------------------------------------------------------------------------------------------
def pool_edges(seed, n_leaves=40, n_pool=35):
    """degrees 0, 1, 2, 7, 30 in turn (row 0 has no leaf); leaf 3 has two pool edges, to rows 1 and 2; shuffled edge order"""
    rng = np.random.default_rng(seed)
    degs = [[0, 1, 2, 7, 30][v % 5] for v in range(n_pool)]
    edges = [(int(l), v) for v, d in enumerate(degs) for l in rng.integers(0, n_leaves, d)]
    edges[0] = (3, 1)
    edges[1] = (3, 2)
    return n_leaves, n_pool, [edges[i] for i in rng.permutation(len(edges))]


def compared(rows64, gap, bound, tag):
    """rows the rule compares; the 1 % cap is asserted here, on the reference alone.  `gap` is the reference's top-two gap; where
    it is 0 (an exact tie of the maximum) the distance from the maximum to the largest entry below it takes its place"""
    m = rows64.max(dim=1, keepdim=True).values
    below = torch.where(rows64 < m, rows64, torch.full_like(rows64, float("-inf"))).max(dim=1).values
    dist = torch.where(gap > 0, gap, m[:, 0] - below)
    skip = dist <= bound
    assert int(skip.sum()) * 100 <= skip.numel(), f"{tag}: {int(skip.sum())} of {skip.numel()} rows inside the bound {bound:.3e}"
    return ~skip


def pooled_case(classes, act, seed):
    n_leaves, n_pool, edges = pool_edges(seed)
    h = Tail(n_leaves, classes, act, seed=seed, ldz_pad=8 * (seed % 2), pool=(n_pool, edges))
    ref = h.reference()
    r64, r32 = h.rows(torch.float64), h.rows(torch.float32)
    assert torch.equal(_first_argmax(r64), ref["pred"]) and torch.equal(_top2_gap(r64), ref["gap"])  # the same formulas
    bound = 64.0 * float((r32.double() - r64).abs().max())
    return h, ref, compared(r64, ref["gap"], bound, f"pool {classes} act {act}")


@pytest.mark.parametrize("act", [N, R, E])
@pytest.mark.parametrize("classes", [5, 64, 65, 256])
def test_pooled_labels(classes, act):
    h, ref, use = pooled_case(classes, act, seed=classes % 7 + act)
    rc, outs = run_tails([h], True, act)
    assert rc == 0, _lib.load().hmp_last_error()
    got = check_written(outs[0], h.n_pool, f"pool {classes} act {act}")
    assert int(np.diff(h.csr[0])[0]) == 0 and int(got[0]) == 0  # a pooled row without leaves predicts 0
    assert torch.equal(got[use], ref["pred"][use]), f"pool {classes} act {act}: {got.tolist()} != {ref['pred'].tolist()}"


@pytest.mark.parametrize("classes,act", [((65, 5), R), ((5, 256), E)])
def test_identity_pool_next_to_a_real_one(classes, act):
    pooled, ref, use = pooled_case(classes[0], act, seed=3)
    ident = Tail(33, classes[1], act, seed=31, ldz_pad=8)  # rowptr NULL: row v's only leaf is v
    iref = ident.reference()["pred"]
    for heads in ([pooled, ident], [ident, pooled]):
        rc, outs = run_tails(heads, True, act)
        assert rc == 0, _lib.load().hmp_last_error()
        for h, o in zip(heads, outs):
            got = check_written(o, h.n_out, f"pool+identity {classes}")
            if h is pooled:
                assert torch.equal(got[use], ref["pred"][use])
            else:
                assert torch.equal(got, iref)


# ---- linear heads -----------------------------------------------------------------------------------------------------------------
class Heads:
    def __init__(self, classes, F, n_rows, act, seed):
        g = torch.Generator().manual_seed(7100 + seed)
        self.classes, self.F, self.n_rows, self.act = classes, F, n_rows, act
        self.ldz = align4(F) + 8 * (seed % 2)
        self.z = make_z(g, n_rows, F, self.ldz, act)
        self.W = [torch.randint(-16, 17, (c, F), generator=g).float() / 8 for c in classes]
        self.b = [torch.randint(-16, 17, (c,), generator=g).float() / 8 for c in classes]
        for h in range(2):  # classes 0 and 1 of a head tie on every row, exactly: the first must win
            if classes[h] >= 2:
                self.W[h][1], self.b[h][1] = self.W[h][0], self.b[h][0]
        m0 = (torch.rand(n_rows, generator=g) < 0.5).to(torch.uint8)
        m1 = (torch.rand(n_rows, generator=g) < 0.5).to(torch.uint8)
        if n_rows >= 31:
            m0[2:6] = torch.tensor([1, 1, 0, 0], dtype=torch.uint8)
            m1[2:6] = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)  # a row in both heads, in one each, in neither
        self.patterns = {"both_given": (m0, m1), "second_null": (m0, None), "both_null": (None, None)}
        self.d = {k: v.to(dev()) for k, v in dict(z=self.z, W0=self.W[0], W1=self.W[1], b0=self.b[0], b1=self.b[1], m0=m0, m1=m1).items()}

    def logits(self, dtype):
        """the heads' logits by the formulas of linear_heads_reference, in dtype"""
        _, y = _y(self.z[:self.n_rows], self.F, self.act, None, 0.0, dtype)
        return [(y @ w.to(dtype).t() + b.to(dtype)).detach() for w, b in zip(self.W, self.b)]

    def desc(self, pattern, **over):
        d = _lib.LinearHeadsDesc(z=ptr(self.d["z"]), ldz=self.ldz, n_rows=self.n_rows, F=self.F, act=self.act)
        d.W[0], d.W[1], d.bias[0], d.bias[1] = ptr(self.d["W0"]), ptr(self.d["W1"]), ptr(self.d["b0"]), ptr(self.d["b1"])
        m = self.patterns[pattern]
        d.member[0] = ptr(self.d["m0"]) if m[0] is not None else None
        d.member[1] = ptr(self.d["m1"]) if m[1] is not None else None
        d.classes[0], d.classes[1] = self.classes
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def run(self, desc):
        outs = [sentinel(self.n_rows), sentinel(self.n_rows)]
        prd = (C.c_void_p * 2)(*[o.data_ptr() for o in outs])
        nb = C.c_int32(-1)
        rc = _lib.load().hmp_linear_heads_predict(C.byref(desc), prd, C.byref(nb), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, outs, nb.value


HEAD_SHAPES = [((15, 35), 16), ((1, 64), 80), ((15, 35), 768)]


@pytest.mark.parametrize("n_rows", [1, 31, 33, 7681])
@pytest.mark.parametrize("shape", range(len(HEAD_SHAPES)))
def test_linear_head_labels(shape, n_rows):
    """7681 rows = 240 tiles + 1: one workgroup takes a second tile"""
    classes, F = HEAD_SHAPES[shape]
    act = [R, E, N, E][(shape + [1, 31, 33, 7681].index(n_rows)) % 4]
    H = Heads(classes, F, n_rows, act, seed=10 * shape + n_rows % 7)
    tag = f"heads {classes} F {F} rows {n_rows} act {act}"
    l64, l32 = H.logits(torch.float64), H.logits(torch.float32)
    bound = 64.0 * max(float((a.double() - b).abs().max()) for a, b in zip(l32, l64))
    full = linear_heads_reference(H.z[:n_rows], F, H.W[0], H.b[0], H.W[1], H.b[1], act, None, 0.0, torch.zeros(n_rows, dtype=torch.int64),
                                  None, None, None, -100)
    assert all(torch.equal(_top2_gap(l), g) for l, g in zip(l64, full["gap"]))  # the same formulas
    use = [compared(l, g, bound, f"{tag} head {h}") for h, (l, g) in enumerate(zip(l64, full["gap"]))]
    pred = [_first_argmax(l) for l in l64]
    for h in range(2):
        if classes[h] >= 2:
            assert bool((pred[h] != 1).all())  # class 1 duplicates class 0: never the FIRST maximum
    for pattern, (m0, m1) in H.patterns.items():
        rc, outs, nb = H.run(H.desc(pattern))
        assert rc == 0, _lib.load().hmp_last_error()
        assert nb == min(-(-n_rows // 32), 240)
        members = head_members(n_rows, m0, m1)
        for h in range(2):
            got = check_written(outs[h], n_rows, f"{tag} {pattern} head {h}")
            assert torch.equal(got == -1, ~members[h]), f"{tag} {pattern} head {h}: -1 not exactly on the non-member rows"
            on = members[h] & use[h]
            assert torch.equal(got[on], pred[h][on]), f"{tag} {pattern} head {h}: {int((got[on] != pred[h][on]).sum())} rows differ"


def test_linear_heads_skip_a_null_output():
    H = Heads((15, 35), 16, 33, R, seed=77)
    out = sentinel(33)
    prd = (C.c_void_p * 2)(None, out.data_ptr())
    assert _lib.load().hmp_linear_heads_predict(C.byref(H.desc("both_given")), prd, None, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = check_written(out, 33, "head 1 alone")
    m = head_members(33, *H.patterns["both_given"])[1]
    assert torch.equal(got[m], _first_argmax(H.logits(torch.float64)[1])[m]) and bool((got[~m] == -1).all())


# ---- hmp_predict_rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes", [1, 26])
@pytest.mark.parametrize("ld_pad,n_rows", [(0, 37), (1, 37), (0, 16401), (3, 16401)])
def test_predict_rows(ld_pad, n_rows, n_classes):
    """ld = align4(classes) (16-byte rows: the quad walk) or that + 1 / + 3 (the scalar walk); 16401 rows: more than the grid's
    1024 x 16, so workgroups stride over rows; members NULL and given"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(n_rows + n_classes + ld_pad)
    ld = align4(n_classes) + ld_pad
    x = (torch.randint(-16, 17, (n_rows, ld), generator=g).float() / 4).to(dev())  # ties are frequent: the first maximum counts
    want = torch.empty(n_rows, dtype=torch.int64, device=dev())
    _lib.check(lib.hmp_argmax_rows(x.data_ptr(), ld, n_rows, n_classes, want.data_ptr(), _lib.stream_ptr()))
    assert torch.equal(want.cpu(), _first_argmax(x[:, :n_classes].cpu()))
    members = (torch.rand(n_rows, generator=g) < 0.6).to(dev())
    for m in (None, members):
        out = sentinel(n_rows)
        _lib.check(lib.hmp_predict_rows(x.data_ptr(), ld, n_rows, n_classes, ptr(m), out.data_ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = check_written(out, n_rows, f"predict_rows ld {ld}")
        ref = want.cpu() if m is None else torch.where(m.cpu(), want.cpu(), torch.full_like(want.cpu(), -1))
        assert torch.equal(got, ref)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def untouched(outs):
    return all(bool((o == SENTINEL).all()) for o in outs)


def test_predict_launchers_refuse_and_launch_nothing():
    lib = _lib.load()
    wide = Tail(20, 257, R, seed=40)
    rc, outs = run_tails([wide], True, R)  # pooled rows are held in registers: at most 256 classes
    assert rc == HMP_E_ARG and b"257 classes" in lib.hmp_last_error() and untouched(outs)
    ok = Tail(20, 5, R, seed=41)
    rc, outs = run_tails([ok, wide], True, R)  # refused as the second entry too: the first must not have run
    assert rc == HMP_E_ARG and untouched(outs)
    rc, outs = run_tails([wide], False, R)  # the unpooled launch takes any width
    assert rc == 0 and torch.equal(check_written(outs[0], 20, "257 unpooled"), wide.reference()["pred"])
    for over in (dict(z=ok.d_z.data_ptr() + 4), dict(ldz=6), dict(ldz=4), dict(classes=0)):
        rc, outs = run_tails([ok], False, R, descs=[ok.desc(False, **over)])
        assert rc == HMP_E_ARG and untouched(outs), over
    rc, outs = run_tails([ok], True, R, descs=[ok.desc(True, n_pool=19)])  # an identity pool has a row per leaf
    assert rc == HMP_E_ARG and untouched(outs)
    assert lib.hmp_head_tails_predict(None, 1, 0, R, None, None) == HMP_E_ARG
    arr = (_lib.TailDesc * 1)(ok.desc(False))
    assert lib.hmp_head_tails_predict(arr, 3, 0, R, (C.c_void_p * 1)(outs[0].data_ptr()), None) == HMP_E_ARG
    assert lib.hmp_head_tails_predict(arr, 1, 0, R, (C.c_void_p * 1)(None), _lib.stream_ptr()) == HMP_E_ARG  # rows without an output

    H = Heads((3, 2), 64, 40, R, seed=42)
    for msg, over in ((b"linear heads: F = 1025", dict(F=1025, ldz=1028)), (b"linear heads: F = 0", dict(F=0)),
                      (b"final state", dict(ldz=62)), (b"final state", dict(z=H.d["z"].data_ptr() + 4))):
        rc, outs, _ = H.run(H.desc("both_given", **over))
        assert rc == HMP_E_ARG and msg in lib.hmp_last_error() and untouched(outs), over
    d = H.desc("both_given")
    d.classes[0] = 65
    rc, outs, _ = H.run(d)
    assert rc == HMP_E_ARG and b"linear heads: classes" in lib.hmp_last_error() and untouched(outs)
    assert lib.hmp_linear_heads_predict(None, None, None, None) == HMP_E_ARG
    assert H.run(H.desc("both_given"))[0] == 0

    x = torch.zeros(8, 8, device=dev())
    out = sentinel(8)
    assert lib.hmp_predict_rows(x.data_ptr(), 4, 8, 5, None, out.data_ptr(), _lib.stream_ptr()) == HMP_E_ARG  # ld < classes
    assert lib.hmp_predict_rows(None, 8, 8, 5, None, out.data_ptr(), _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_predict_rows(x.data_ptr(), 8, 8, 5, None, None, _lib.stream_ptr()) == HMP_E_ARG
    torch.cuda.synchronize()
    assert untouched([out])
