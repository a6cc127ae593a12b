"""The readout launchers driven directly (hmp_head_tails, hmp_linear_heads_run): tail_ce_kernel, pool_ce_kernel, pool_grad_kernel,
the two count kernels (csrc/semisup.hip) and linear_heads_kernel<TRAIN> (csrc/heads.hip) at the class widths, degrees, row counts
and leading dimensions the models never reach, against the float64 reference of tests/_tail_reference.py.

Every output buffer (grad, dpool, row_lv, slabs) starts as NaN and must hold no NaN inside [n_rows][ld] afterwards; the padding
columns of the FINAL STATE hold NaN and 1e30 in turn (the kernels may load them, never use them).  z holds exact +0.0 and -0.0 entries (3 %
each), the labels some ignored ones, one negative and one equal to `classes` (status bit 1, no contribution).  Every launch runs
twice into fresh buffers and the two results are bit-equal.

Tolerance of loss and gradients: the error of the same formulas evaluated in float32 by plain torch on the CPU is the yardstick;
the kernel may be off by 4 x that, with a floor of 4 float32 ulps of the tensor's largest |ref| (_tail_reference.within).  Counts
are exact: for act none / ReLU z is drawn from multiples of 1/4 in [-4, 4] (W, b from multiples of 1/8 in [-2, 2]), so every
float32 sum is exact, a pooled division by deg <= 300 keeps strict order (quotients differ by >= 0.25 / 300) and ties stay ties;
for ELU the rows whose float64 top-two gap is below 1e-4 leave the mask (fewer than 1 % of the rows).

Measured float32 yardsticks (max abs error, max relative error over |ref| > 1e-6) of the widest cases, and the kernel's figures
(on the masks SEED draws with both seed words in the generator's key, csrc/common.h drop_pair):

    case                                                 tensor     yardstick abs / rel     kernel abs / rel
    unpooled tail, 4099 rows x 300 classes, ELU, p 0.25  dz         5.2e-07 / 1.3e-06      7.8e-07 / 1.5e-05 (rel: under the floor 6.4e-07)
                                                         row loss   9.9e-07 / 2.4e-07      1.1e-06 / 2.1e-07
    heads 64 + 64, F = 1024, 33 rows, ELU, p 0.25        dz         1.9e-05 / 1.9e+00      1.1e-05 / 1.9e+00
                                                         row loss   3.6e-05 / 3.4e-07      1.7e-05 / 3.1e-07
                                                         dW         2.5e-05 / 2.5e-03      2.3e-05 / 2.1e-03
                                                         db         5.5e-06 / 5.0e-04      5.5e-06 / 5.0e-04
    heads 64 + 64, F = 65, 15365 rows, ELU, p 0.25       dz         1.8e-05 / 3.0e+00      1.8e-05 / 3.0e+00
      (slab sums of 240 workgroups x 2 or 3 tiles)       row loss   2.3e-05 / 2.5e-01      2.3e-05 / 2.5e-01
                                                         dW         8.4e-05 / 2.3e-03      7.8e-05 / 6.6e-03
                                                         db         4.5e-05 / 1.8e-05      2.5e-05 / 2.2e-05

The logits of linear_heads_kernel are summed per 64-column chunk and the chunk sums added up.  As one fmaf chain over all of F the
row loss at F = 1024 was off by 2.0e-04 on this data (1.9e-04 on the masks of the earlier key), 5.6 x the yardstick against the 4 x
allowed: every step of the chain rounds at the magnitude of the growing logit (~100).

The relative figures of the heads' dz, dW and db are decided by a few nearly cancelled elements (|ref| ~ 1e-6 .. 1e-4 carrying the
absolute error every element carries: logits of magnitude ~100 at F = 1024 put 1e-5 into the softmax); such signed matrix products
are held to the absolute yardstick alone (_tail_reference.within, signed_sum).  A relative error of 1.0 in a row loss is a loss
near 1e-6 that float32 rounds to 0, in torch as in the kernel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _tail_reference import (ACT_ELU, ACT_NONE, ACT_RELU, linear_heads_reference, pool_csr_csc, tail_reference,  # noqa: E402
                             within, yardstick)
from hydra_gnn_amd import _lib  # noqa: E402

IGNORED = -100
NAN = float("nan")
SEED = 0x5EED1234ABCD
GAP = 1e-4


def dev():
    return torch.device("cuda:0")


def cdiv(a, b):
    return -(-a // b)


def align4(x):
    return (x + 3) & ~3


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev())


def bits(t):
    return t.view(torch.int32)


def ptr(t):
    return t.data_ptr() if t is not None else None


def sync_status(state):
    torch.cuda.synchronize()
    return int(state.cpu()[1])


def keep_mask(step, stream, p, n_rows, width):
    """the engine's keep bits of the site (SEED, step, stream) for an [n_rows, width] tensor (all ones without dropout)"""
    m = torch.ones(max(n_rows, 1), width, dtype=torch.uint8, device=dev())
    if p > 0 and n_rows > 0:
        _lib.check(_lib.load().hmp_dropout_mask(SEED, step, stream, p, n_rows, width, m.data_ptr(), _lib.stream_ptr()))
    return m[:n_rows].cpu()


def make_z(g, n_rows, width, ld, act):
    """final state [n_rows, ld] on the CPU: multiples of 1/4 in [-4, 4] (ELU: normal draws), 3 % exact +0.0 and 3 % exact -0.0,
    NaN and 1e30 alternating in the padding columns"""
    n = max(n_rows, 1)
    if act == ACT_ELU:
        z = torch.randn(n, ld, generator=g) * 1.5
    else:
        z = torch.randint(-16, 17, (n, ld), generator=g).float() / 4
    u = torch.rand(n, ld, generator=g)
    z[u < 0.03] = 0.0
    z[(u >= 0.03) & (u < 0.06)] = -0.0
    pad = z[:, width:]  # poison: NaN spoils a sum that reads it, 1e30 a maximum or an argmax (fmaxf and > skip a NaN)
    pad[:] = NAN
    pad[(torch.arange(n)[:, None] + torch.arange(ld - width)[None, :]) % 2 == 1] = 1e30
    return z


def tie_rows(z, n_rows, classes, labels, act):
    """rows whose maximum is shared: inside one quad, across two lanes, across two quad walks of one lane (64 columns apart) and
    across the 256-column boundary; the label is the SECOND maximum in two of them (a later-maximum rule would count them)"""
    if act == ACT_ELU or n_rows < 15 or classes < 2:
        return
    pairs = [(0, 1), (1, 5), (2, 66), (3, 259), (classes - 2, classes - 1)]
    for r, (a, b) in zip(range(5, 10), pairs):
        if b >= classes:
            continue
        z[r, :classes] = -1.0
        z[r, a] = z[r, b] = 3.0
        labels[r] = b if r % 2 else a


def make_labels(g, n, classes, use_mask):
    """labels of n CE rows: uniform, then ignored ones, one negative, one == classes; a second out-of-range label sits in a
    masked-out row when there is a mask (it must not raise the status)"""
    n1 = max(n, 1)
    lab = torch.randint(0, classes, (n1,), generator=g)
    lab[torch.rand(n1, generator=g) < 0.15] = IGNORED
    mask = None
    if use_mask:
        mask = (torch.rand(n1, generator=g) < 0.8).to(torch.uint8)
    if n >= 15:
        lab[2], lab[3], lab[4] = -1, classes, IGNORED
        if use_mask:
            mask[2] = mask[3] = 1
            lab[11], mask[11] = classes + 7, 0
    return lab, mask


# ---- tails -------------------------------------------------------------------------------------------------------------------------
class Tail:
    """One head of a tail launch: inputs on the CPU and the device, the descriptor, float64 / float32 references."""

    def __init__(self, n_rows, classes, act, p, *, ldz_pad=0, ldg_pad=0, ldp_pad=0, use_mask=False, seed=0, slot=0, pool=None):
        g = torch.Generator().manual_seed(1000 * seed + classes)
        self.n_rows, self.classes, self.act, self.p, self.slot = n_rows, classes, act, p, slot
        self.ldz, self.ldg = align4(classes) + ldz_pad, align4(classes) + ldg_pad
        self.ldp = self.ldg + ldp_pad
        self.step, self.stream = 3 + seed, 16 + slot
        self.z = make_z(g, n_rows, classes, self.ldz, act)
        self.pool = None
        self.n_pool = n_rows
        if pool is not None:  # (n_pool, edges [(leaf, pooled row)])
            self.n_pool = pool[0]
            self.csr = pool_csr_csc(pool[0], n_rows, pool[1])
            self.pool = self.csr[:2]
            # (a list without edges still needs a non-null pointer: one unused element)
            self.d_csr = [torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, np.int32))).to(dev()) for a in self.csr]
        self.labels, self.mask = make_labels(g, self.n_pool, classes, use_mask)
        if pool is None:
            tie_rows(self.z, n_rows, classes, self.labels, act)
        self.d_z, self.d_labels = self.z.to(dev()), self.labels.to(dev())
        self.d_mask = self.mask.to(dev()) if self.mask is not None else None
        self.keep = keep_mask(self.step, self.stream, p, n_rows, classes)

    def cut(self, t, n):
        return t[:n] if t is not None else None

    def reference(self, dtype=torch.float64, train=True, mask=None):
        m = self.cut(self.mask if mask is None else mask, self.n_pool)
        return tail_reference(self.z[:self.n_rows], self.classes, self.act, self.keep, self.p if train else 0.0,
                              self.labels[:self.n_pool], m, IGNORED, pool=self.pool, dtype=dtype)

    def desc(self, out, pooled, mask=None):
        d = _lib.TailDesc(z=ptr(self.d_z), labels=ptr(self.d_labels), mask=ptr(self.d_mask if mask is None else mask),
                          ldz=self.ldz, n_rows=self.n_rows, classes=self.classes, slot=self.slot,
                          rng_step=self.step, rng_stream=self.stream, p=self.p, seed=SEED)
        if out is not None:
            d.grad, d.ldg, d.row_lv = ptr(out["grad"]), self.ldg, ptr(out["row_lv"])
        if pooled:
            d.n_pool = self.n_pool
            if self.pool is not None:
                d.rowptr, d.col, d.t_rowptr, d.t_col = [ptr(t) for t in self.d_csr]
            if out is not None:
                d.dpool, d.ldp = ptr(out["dpool"]), self.ldp
        return d

    def outputs(self):
        return {"grad": nans(max(self.n_rows, 1), self.ldg), "row_lv": nans(max(self.n_pool, 1), 2),
                "dpool": nans(max(self.n_pool, 1), self.ldp)}


def run_ce(heads, mode, act):
    """one CE launch (mode 0 or 2) of the heads into fresh NaN buffers: (rc, outputs per head, status word)"""
    outs = [h.outputs() for h in heads]
    state = torch.zeros(5, dtype=torch.int32, device=dev())
    arr = (_lib.TailDesc * len(heads))(*[h.desc(o, mode == 2) for h, o in zip(heads, outs)])
    rc = _lib.load().hmp_head_tails(arr, len(heads), mode, act, IGNORED, state.data_ptr(), None, _lib.stream_ptr())
    return rc, outs, sync_status(state)


def run_count(heads, mode, act, masks):
    counts = torch.zeros(4, dtype=torch.int64, device=dev())
    arr = (_lib.TailDesc * len(heads))(*[h.desc(None, mode == 3, mask=m) for h, m in zip(heads, masks)])
    _lib.check(_lib.load().hmp_head_tails(arr, len(heads), mode, act, IGNORED, None, counts.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return counts.cpu().tolist()


def check_close(name, got, ref64, ref32, signed_sum=False):
    yard = yardstick(ref32, ref64)
    ok, msg = within(got, ref64, yard, signed_sum=signed_sum)
    print(f"  {name}: {msg}")
    assert ok, f"{name}: {msg}"


def check_ce(heads, mode, act, tag):
    rc, outs, status = run_ce(heads, mode, act)
    assert rc == 0, _lib.load().hmp_last_error()
    rc2, outs2, status2 = run_ce(heads, mode, act)
    assert rc2 == 0 and status2 == status
    bad = 0
    for i, (h, o, o2) in enumerate(zip(heads, outs, outs2)):
        for k in o:
            assert torch.equal(bits(o[k]), bits(o2[k])), f"{tag} head {i}: {k} differs between two runs"
        r64, r32 = h.reference(), h.reference(torch.float32)
        bad += r64["bad"]
        grad = o["grad"][:h.n_rows].cpu()
        assert not bool(torch.isnan(grad).any()), f"{tag} head {i}: NaN left in grad [n_rows][ldg]"
        assert float(grad[:, h.classes:].abs().sum()) == 0.0, f"{tag} head {i}: gradient columns past classes are not 0"
        lv = o["row_lv"][:h.n_pool].cpu()
        assert not bool(torch.isnan(lv).any()), f"{tag} head {i}: NaN left in row_lv"
        if mode == 2:  # the scratch the leaf-gradient launch reads: the columns of the classes' quads
            assert not bool(torch.isnan(o["dpool"][:h.n_pool, :align4(h.classes)]).any()), f"{tag} head {i}: NaN left in dpool"
        assert torch.equal(lv[:, 1].double(), r64["row_valid"]), f"{tag} head {i}: valid flags"
        check_close(f"{tag} head {i} dz", grad[:, :h.classes], r64["dz"], r32["dz"])
        check_close(f"{tag} head {i} row loss", lv[:, 0], r64["row_loss"], r32["row_loss"])
        check_close(f"{tag} head {i} loss", lv[:, 0].double().sum(), r64["loss"], r32["loss"])
    assert status == (2 if bad else 0), f"{tag}: status {status} with {bad} out-of-range labels"
    return outs


def check_count(heads, mode, act, tag):
    masks, want = [], [0, 0, 0, 0]
    for h in heads:
        r = h.reference(train=False)
        m = torch.ones(max(h.n_pool, 1), dtype=torch.uint8) if h.mask is None else h.mask.clone()
        if act == ACT_ELU and h.n_pool:
            near = r["gap"] < GAP
            if h.pool is not None:  # an empty pooled row is exactly 0 in every precision: it stays
                near &= torch.from_numpy(np.diff(h.csr[0]) > 0)
            assert int(near.sum()) * 100 < max(h.n_pool, 1), f"{tag}: {int(near.sum())} of {h.n_pool} rows are near-ties"
            m[:h.n_pool][near] = 0
            r = h.reference(train=False, mask=m)
        masks.append(m.to(dev()))
        want[2 * h.slot] += r["correct"]
        want[2 * h.slot + 1] += r["total"]
    got = run_count(heads, mode, act, masks)
    assert got == run_count(heads, mode, act, masks)
    print(f"  {tag} counts {got} (reference {want})")
    assert got == want, f"{tag}: counts {got}, reference {want}"


N, R, E = ACT_NONE, ACT_RELU, ACT_ELU
# (rows, classes) per head, act, p, (ldz_pad, ldg_pad), mask
TAIL_ONE = [
    (17, 1, N, 0.0, (0, 0), False), (15, 3, R, 0.25, (8, 4), True), (16, 4, E, 0.25, (0, 4), False), (1, 5, N, 0.25, (8, 0), True),
    (17, 63, R, 0.0, (0, 4), True), (4099, 64, N, 0.25, (8, 4), True), (16, 65, E, 0.0, (0, 0), False), (4099, 70, R, 0.25, (0, 4), False),
    (15, 255, N, 0.0, (8, 0), True), (17, 256, E, 0.25, (0, 4), True), (16, 257, R, 0.25, (8, 4), False),
    (4099, 300, E, 0.25, (8, 4), True),
    (1, 300, N, 0.0, (0, 0), False), (4099, 257, N, 0.25, (0, 0), True), (4099, 5, E, 0.0, (0, 4), False), (1, 1, R, 0.25, (8, 4), True),
    (15, 64, E, 0.25, (0, 0), False), (17, 65, R, 0.25, (8, 4), True), (16, 256, N, 0.25, (8, 0), False), (17, 3, N, 0.0, (0, 0), True),
    (4099, 4, R, 0.0, (8, 4), True), (1, 63, E, 0.25, (8, 0), False), (16, 70, N, 0.25, (0, 4), True), (4099, 255, R, 0.25, (0, 4), False),
]
TAIL_TWO = [
    ((17, 5), (33, 70), R, 0.25, True), ((17, 300), (33, 3), E, 0.0, False), ((17, 64), (33, 257), N, 0.25, True),
    ((17, 255), (33, 256), E, 0.25, False), ((0, 70), (40, 5), R, 0.25, True), ((0, 4), (40, 300), N, 0.0, False),
    ((40, 65), (0, 3), E, 0.25, True), ((40, 256), (0, 257), R, 0.0, False), ((17, 1), (33, 63), N, 0.0, True),
    ((0, 1), (40, 1), E, 0.0, False), ((40, 300), (0, 300), N, 0.25, True), ((17, 65), (33, 65), R, 0.25, False),
]


@pytest.mark.parametrize("case", range(len(TAIL_ONE)))
def test_unpooled_tail_one_head(case):
    rows, classes, act, p, (ldz_pad, ldg_pad), use_mask = TAIL_ONE[case]
    h = Tail(rows, classes, act, p, ldz_pad=ldz_pad, ldg_pad=ldg_pad, use_mask=use_mask, seed=case, slot=case % 2)
    tag = f"tail {rows}x{classes} act {act} p {p}"
    check_ce([h], 0, act, tag)
    check_count([h], 1, act, tag)


@pytest.mark.parametrize("case", range(len(TAIL_TWO)))
def test_unpooled_tail_two_heads(case):
    """(17, 33): entry 1 starts in block 2, not on a multiple of its own rows; (0, 40) / (40, 0): an empty entry next to a full one"""
    (r0, c0), (r1, c1), act, p, use_mask = TAIL_TWO[case]
    heads = [Tail(r0, c0, act, p, ldz_pad=8, ldg_pad=0, use_mask=use_mask, seed=50 + case, slot=0),
             Tail(r1, c1, act, p if case % 3 else 0.0, ldz_pad=0, ldg_pad=4, use_mask=not use_mask, seed=80 + case, slot=1)]
    tag = f"tails {r0}x{c0} + {r1}x{c1} act {act} p {p}"
    check_ce(heads, 0, act, tag)
    check_count(heads, 1, act, tag)


# ---- pooled tails -----------------------------------------------------------------------------------------------------------------
def pool_profile(name, seed):
    """(n_leaves, n_pool, edges) in a shuffled edge order (the plan's lists are stable in it)"""
    rng = np.random.default_rng(seed)
    if name == "ones":  # every pooled row has one leaf, a permutation
        n_leaves = n_pool = 37
        edges = [(int(l), v) for v, l in enumerate(rng.permutation(n_leaves))]
    elif name == "mixed":  # degrees 0, 1, 2, 37, 300 over three workgroups of pooled rows; a leaf may repeat
        n_leaves, n_pool = 100, 35
        degs = [[0, 1, 2, 37, 300][v % 5] for v in range(n_pool)]
        edges = [(int(l), v) for v, d in enumerate(degs) for l in rng.integers(0, n_leaves, d)]
    elif name == "empty":  # no pool edge at all
        n_leaves, n_pool, edges = 24, 20, []
    else:  # "leaf012": leaf i has i % 3 pool edges
        assert name == "leaf012"
        n_leaves, n_pool = 50, 19
        edges = [(l, int(v)) for l in range(n_leaves) for v in rng.integers(0, n_pool, l % 3)]
    order = rng.permutation(len(edges))
    return n_leaves, n_pool, [edges[i] for i in order]


POOL_CASES = [
    ("ones", 1, N, 0.0), ("mixed", 5, R, 0.25), ("empty", 64, E, 0.25), ("leaf012", 65, N, 0.25), ("mixed", 130, E, 0.25),
    ("leaf012", 255, R, 0.0), ("mixed", 256, N, 0.25), ("ones", 256, E, 0.25), ("empty", 5, N, 0.0), ("leaf012", 130, E, 0.0),
    ("mixed", 65, R, 0.25), ("ones", 64, R, 0.25), ("mixed", 255, E, 0.0), ("leaf012", 1, R, 0.25),
]


def pooled_head(profile, classes, act, p, seed, slot, use_mask):
    n_leaves, n_pool, edges = pool_profile(profile, seed)
    return Tail(n_leaves, classes, act, p, ldz_pad=8 * (seed % 2), ldg_pad=4 * (seed % 2), ldp_pad=4 * ((seed // 2) % 2), use_mask=use_mask,
                seed=200 + seed, slot=slot, pool=(n_pool, edges))


@pytest.mark.parametrize("case", range(len(POOL_CASES)))
def test_pooled_tail(case):
    profile, classes, act, p = POOL_CASES[case]
    h = pooled_head(profile, classes, act, p, case, case % 2, case % 2 == 0)
    tag = f"pool {profile} classes {classes} act {act} p {p}"
    check_ce([h], 2, act, tag)
    check_count([h], 3, act, tag)


@pytest.mark.parametrize("classes,act,p", [((130, 5), R, 0.25), ((64, 256), E, 0.25), ((1, 255), N, 0.0)])
def test_pooled_head_next_to_an_identity_pool(classes, act, p):
    pooled = pooled_head("mixed", classes[0], act, p, 7, 0, True)
    ident = Tail(33, classes[1], act, p, ldz_pad=8, ldg_pad=4, ldp_pad=4, use_mask=False, seed=300, slot=1)
    for heads in ([pooled, ident], [ident, pooled]):
        tag = f"pool+identity {classes} act {act} (first {'pooled' if heads[0] is pooled else 'identity'})"
        check_ce(heads, 2, act, tag)
        check_count(heads, 3, act, tag)


@pytest.mark.parametrize("classes", [1, 5, 64, 65, 130, 255, 256])
@pytest.mark.parametrize("act,p", [(N, 0.0), (R, 0.25), (E, 0.25)])
def test_identity_pool_equals_the_unpooled_tail_bit_for_bit(classes, act, p):
    """tail_fns.h: ce_group's association is "the same whatever NQ" -- the pooled kernel holds the row in registers (NQ = 4), the
    unpooled one walks it (NQ = 0); with an identity pool both see the same rows"""
    h = Tail(37, classes, act, p, ldz_pad=8, ldg_pad=4, use_mask=True, seed=400 + classes)
    rc0, o0, s0 = run_ce([h], 0, act)
    rc2, o2, s2 = run_ce([h], 2, act)
    assert rc0 == 0 and rc2 == 0 and s0 == s2
    assert not bool(torch.isnan(o0[0]["grad"]).any())
    assert torch.equal(bits(o0[0]["row_lv"]), bits(o2[0]["row_lv"]))
    assert torch.equal(bits(o0[0]["grad"]), bits(o2[0]["grad"]))


def test_pooled_tail_refuses_257_classes_and_launches_nothing():
    h = Tail(20, 257, R, 0.0, seed=500)
    rc, outs, status = run_ce([h], 2, R)
    assert rc != 0 and b"pool tail: 257 classes" in _lib.load().hmp_last_error()
    assert all(bool(torch.isnan(t).all()) for t in outs[0].values()) and status == 0
    ok = Tail(20, 5, R, 0.0, seed=501)
    rc, outs, _ = run_ce([ok, h], 2, R)  # refused as the second entry too: the first must not have run
    assert rc != 0 and all(bool(torch.isnan(t).all()) for o in outs for t in o.values())
    lib = _lib.load()
    counts = torch.zeros(4, dtype=torch.int64, device=dev())
    arr = (_lib.TailDesc * 1)(h.desc(None, True))
    assert lib.hmp_head_tails(arr, 1, 3, R, IGNORED, None, counts.data_ptr(), _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [0, 0, 0, 0]


def test_tail_launchers_refuse_bad_layouts():
    lib = _lib.load()
    h = Tail(20, 5, N, 0.0, seed=502)

    def rc_of(mode, **over):
        out = h.outputs()
        d = h.desc(out, mode == 2)
        for k, v in over.items():
            setattr(d, k, v)
        state = torch.zeros(5, dtype=torch.int32, device=dev())
        rc = lib.hmp_head_tails((_lib.TailDesc * 1)(d), 1, mode, N, IGNORED, state.data_ptr(), None, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 or all(bool(torch.isnan(t).all()) for t in out.values())
        return rc

    assert rc_of(0) == 0 and rc_of(2) == 0
    assert rc_of(0, ldz=6) != 0 and rc_of(0, ldz=4) != 0 and rc_of(0, ldg=4) != 0 and rc_of(0, ldg=10) != 0
    assert rc_of(0, classes=0) != 0 and rc_of(0, z=h.d_z.data_ptr() + 4) != 0
    assert rc_of(2, ldp=4) != 0 and rc_of(2, n_pool=19) != 0 and rc_of(2, dpool=None) != 0
    assert rc_of(2, rowptr=h.d_labels.data_ptr()) != 0  # a CSR without its CSC
    assert lib.hmp_head_tails(None, 1, 0, N, IGNORED, None, None, None) != 0
    assert lib.hmp_head_tails((_lib.TailDesc * 1)(h.desc(h.outputs(), False)), 3, 0, N, IGNORED, None, None, None) != 0


# ---- linear heads -----------------------------------------------------------------------------------------------------------------
class Heads:
    def __init__(self, classes, F, n_rows, act, p, *, ldz_pad=0, members="both_given", use_mask=False, seed=0):
        g = torch.Generator().manual_seed(7000 + seed)
        self.classes, self.F, self.n_rows, self.act, self.p = classes, F, n_rows, act, p
        self.K = classes[0] + classes[1]
        self.ldz, self.ldg = align4(F) + ldz_pad, align4(F)
        self.ld_slab = F + 3
        self.slab_stride = self.K * (self.ld_slab + 1) + 5
        self.step, self.stream = 11 + seed, 24
        self.z = make_z(g, n_rows, F, self.ldz, act)
        self.W = [torch.randint(-16, 17, (c, F), generator=g).float() / 8 for c in classes]
        self.b = [torch.randint(-16, 17, (c,), generator=g).float() / 8 for c in classes]
        cmin = min(classes)
        self.labels = torch.randint(0, cmin, (n_rows,), generator=g)
        self.labels[torch.rand(n_rows, generator=g) < 0.15] = IGNORED
        self.mask = (torch.rand(n_rows, generator=g) < 0.8).to(torch.uint8) if use_mask else None
        self.member = [None, None]
        if members != "both_null":
            self.member[0] = (torch.rand(n_rows, generator=g) < 0.5).to(torch.uint8)
        if members == "both_given":
            self.member[1] = (torch.rand(n_rows, generator=g) < 0.5).to(torch.uint8)
        if n_rows >= 31:
            self.labels[2], self.labels[3], self.labels[4] = -1, cmin, IGNORED
            if use_mask:
                self.mask[2] = self.mask[3] = 1
            if members == "both_given":
                self.member[0][2:8] = torch.tensor([1, 1, 1, 1, 0, 0], dtype=torch.uint8)
                self.member[1][2:8] = torch.tensor([1, 1, 0, 1, 0, 1], dtype=torch.uint8)  # rows in both, one, neither
        if act != ACT_ELU:  # classes 0 and 1 of a head tie on every row: the first must win
            for h in range(2):
                if classes[h] >= 2:
                    self.W[h][1], self.b[h][1] = self.W[h][0], self.b[h][0]
            if cmin >= 2:  # labels on both sides of the tie
                self.labels[self.labels == 0] = torch.randint(0, 2, (int((self.labels == 0).sum()),), generator=g)
        self.d = {k: (v.to(dev()) if v is not None else None) for k, v in
                  dict(z=self.z, W0=self.W[0], W1=self.W[1], b0=self.b[0], b1=self.b[1], labels=self.labels, mask=self.mask,
                       m0=self.member[0], m1=self.member[1]).items()}
        self.keep = keep_mask(self.step, self.stream, p, n_rows, F)
        self.n_blocks = min(cdiv(n_rows, 32), 240)

    def reference(self, dtype=torch.float64, train=True, mask=None):
        return linear_heads_reference(self.z[:self.n_rows], self.F, self.W[0], self.b[0], self.W[1], self.b[1], self.act, self.keep,
                                      self.p if train else 0.0, self.labels, self.mask if mask is None else mask, self.member[0],
                                      self.member[1], IGNORED, dtype=dtype)

    def desc(self, out, mask=None, **over):
        d = _lib.LinearHeadsDesc(z=ptr(self.d["z"]), labels=ptr(self.d["labels"]), mask=ptr(self.d["mask"] if mask is None else mask),
                                 slab_stride=self.slab_stride, ignored=IGNORED, seed=SEED, ldz=self.ldz, n_rows=self.n_rows,
                                 F=self.F, act=self.act, ldg=self.ldg, ld_slab=self.ld_slab, rng_step=self.step,
                                 rng_stream=self.stream, p=self.p)
        d.W[0], d.W[1], d.bias[0], d.bias[1] = ptr(self.d["W0"]), ptr(self.d["W1"]), ptr(self.d["b0"]), ptr(self.d["b1"])
        d.member[0], d.member[1] = ptr(self.d["m0"]), ptr(self.d["m1"])
        d.classes[0], d.classes[1] = self.classes
        if out is not None:
            d.grad, d.row_lv, d.slabs = ptr(out["grad"]), ptr(out["row_lv"]), ptr(out["slabs"])
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def outputs(self, ldg=None):
        return {"grad": nans(self.n_rows, ldg or self.ldg), "row_lv": nans(self.n_rows, 2),
                "slabs": nans(self.n_blocks + 2, self.slab_stride)}

    def run_train(self, **over):
        out = self.outputs(over.get("ldg"))
        state = torch.zeros(5, dtype=torch.int32, device=dev())
        nb = C.c_int32(-1)
        rc = _lib.load().hmp_linear_heads_run(C.byref(self.desc(out, **over)), 1, state.data_ptr(), None, C.byref(nb), _lib.stream_ptr())
        return rc, out, sync_status(state), nb.value

    def run_count(self, mask):
        counts = torch.zeros(4, dtype=torch.int64, device=dev())
        nb = C.c_int32(-1)
        _lib.check(_lib.load().hmp_linear_heads_run(C.byref(self.desc(None, mask=mask)), 0, None, counts.data_ptr(), C.byref(nb),
                                                    _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert nb.value == self.n_blocks
        return counts.cpu().tolist()


def check_heads(H, tag):
    rc, out, status, nb = H.run_train()
    assert rc == 0, _lib.load().hmp_last_error()
    rc2, out2, status2, _ = H.run_train()
    assert rc2 == 0 and status2 == status
    for k in out:
        assert torch.equal(bits(out[k]), bits(out2[k])), f"{tag}: {k} differs between two runs"
    assert nb == H.n_blocks == min(cdiv(H.n_rows, 32), 240)
    r64, r32 = H.reference(), H.reference(torch.float32)
    grad, lv, slabs = out["grad"].cpu(), out["row_lv"].cpu(), out["slabs"].cpu()
    assert not bool(torch.isnan(grad).any()), f"{tag}: NaN left in grad [n_rows][ldg]"
    assert float(grad[:, H.F:].abs().sum()) == 0.0, f"{tag}: gradient columns past F are not 0"
    assert not bool(torch.isnan(lv).any()), f"{tag}: NaN left in row_lv"
    assert bool(torch.isnan(slabs[nb:]).all()), f"{tag}: a slab past n_blocks_out was written"
    used = slabs[:nb].double()
    dW = used[:, :H.K * H.ld_slab].reshape(nb, H.K, H.ld_slab)[:, :, :H.F]
    db = used[:, H.K * H.ld_slab:H.K * H.ld_slab + H.K]
    assert not bool(torch.isnan(dW).any()) and not bool(torch.isnan(db).any()), f"{tag}: NaN left in a used slab"
    dW, db = dW.sum(dim=0), db.sum(dim=0)
    assert torch.equal(lv[:, 1].double(), r64["row_valid"]), f"{tag}: valid counts"
    assert status == (2 if r64["bad"] else 0), f"{tag}: status {status} with {r64['bad']} out-of-range labels"
    check_close(f"{tag} dz", grad[:, :H.F], r64["dz"], r32["dz"], signed_sum=True)
    check_close(f"{tag} row loss", lv[:, 0], r64["row_loss"], r32["row_loss"])
    check_close(f"{tag} loss", lv[:, 0].double().sum(), r64["loss"], r32["loss"])
    check_close(f"{tag} dW", dW, torch.cat(r64["dW"]), torch.cat(r32["dW"]), signed_sum=True)
    check_close(f"{tag} db", db, torch.cat(r64["db"]), torch.cat(r32["db"]), signed_sum=True)
    # accuracy count (eval mode)
    r = H.reference(train=False)
    m = torch.ones(H.n_rows, dtype=torch.uint8) if H.mask is None else H.mask.clone()
    if H.act == ACT_ELU:
        near = (r["counted"][0] & (r["gap"][0] < GAP)) | (r["counted"][1] & (r["gap"][1] < GAP))
        assert int(near.sum()) * 100 < H.n_rows, f"{tag}: {int(near.sum())} of {H.n_rows} rows are near-ties"
        m[near] = 0
        r = H.reference(train=False, mask=m)
    want = [r["correct"][0], r["total"][0], r["correct"][1], r["total"][1]]
    got = H.run_count(m.to(dev()))
    assert got == H.run_count(m.to(dev()))
    print(f"  {tag} counts {got} (reference {want})")
    assert got == want, f"{tag}: counts {got}, reference {want}"


# classes, F, ldz_pad, n_rows, members, act, p
HEAD_CASES = [
    ((1, 1), 1, 0, 1, "both_null", N, 0.0), ((3, 2), 3, 8, 31, "second_null", R, 0.25), ((15, 35), 30, 0, 33, "both_given", E, 0.25),
    ((1, 64), 64, 0, 32, "both_given", R, 0.0), ((64, 1), 65, 8, 33, "second_null", N, 0.25), ((64, 64), 130, 0, 33, "both_given", R, 0.25),
    ((64, 64), 1024, 8, 33, "both_given", E, 0.25), ((64, 64), 1024, 0, 31, "second_null", N, 0.0),
    ((15, 35), 64, 0, 7680, "both_given", R, 0.25), ((64, 64), 65, 8, 7681, "both_given", N, 0.25),
    ((64, 64), 65, 0, 15365, "both_given", E, 0.25), ((3, 2), 30, 8, 15365, "second_null", R, 0.0),
    ((1, 1), 3, 0, 7681, "both_null", E, 0.0), ((3, 2), 1, 8, 33, "both_given", E, 0.25), ((15, 35), 130, 8, 1, "both_given", N, 0.0),
    ((1, 64), 30, 0, 7680, "second_null", N, 0.25), ((64, 1), 3, 0, 31, "both_null", R, 0.25), ((15, 35), 65, 0, 32, "both_null", E, 0.0),
]


@pytest.mark.parametrize("case", range(len(HEAD_CASES)))
def test_linear_heads(case):
    """n_rows 7680 / 7681 / 15365: exactly 240 tiles, one workgroup with a second tile, every workgroup with two or three"""
    classes, F, ldz_pad, n_rows, members, act, p = HEAD_CASES[case]
    H = Heads(classes, F, n_rows, act, p, ldz_pad=ldz_pad, members=members, use_mask=case % 2 == 1, seed=case)
    check_heads(H, f"heads {classes} F {F} rows {n_rows} {members} act {act} p {p}")


def test_linear_heads_refusals():
    """(65, 1) classes, F = 1025, and a gradient ld other than align4(F): the column walk ends at roundup(F, 64), so the launch
    refuses a wider gradient (kernels.h: LinHeadArgs::ldg) instead of leaving columns unwritten.  Nothing is launched."""
    lib = _lib.load()
    H = Heads((3, 2), 64, 40, R, 0.0, seed=90)

    def refused(msg, **over):
        rc, out, status, _ = H.run_train(**over)
        assert rc != 0 and msg in lib.hmp_last_error(), (over, lib.hmp_last_error())
        assert all(bool(torch.isnan(t).all()) for t in out.values()) and status == 0

    assert H.run_train()[0] == 0
    refused(b"gradient ld 68", ldg=68)  # F = 64: columns 64 .. 67 would never be written
    refused(b"gradient ld 60", ldg=60)
    refused(b"linear heads: F = 1025", F=1025, ldz=1028, ldg=1028)
    refused(b"linear heads: F = 0", F=0)
    refused(b"final state", ldz=62)
    refused(b"slab layout", ld_slab=63)
    refused(b"slab layout", slab_stride=H.K * (H.ld_slab + 1) - 1)
    for cls in ((65, 1), (1, 65), (0, 3)):
        d = H.desc(H.outputs())
        d.classes[0], d.classes[1] = cls
        state = torch.zeros(5, dtype=torch.int32, device=dev())
        assert lib.hmp_linear_heads_run(C.byref(d), 1, state.data_ptr(), None, None, _lib.stream_ptr()) != 0
        assert b"linear heads: classes" in lib.hmp_last_error()
        counts = torch.zeros(4, dtype=torch.int64, device=dev())
        assert lib.hmp_linear_heads_run(C.byref(d), 0, None, counts.data_ptr(), None, _lib.stream_ptr()) != 0
    assert lib.hmp_linear_heads_run(None, 1, None, None, None, None) != 0
    assert lib.hmp_linear_heads_run(C.byref(H.desc(None)), 1, None, None, None, _lib.stream_ptr()) != 0  # no outputs
