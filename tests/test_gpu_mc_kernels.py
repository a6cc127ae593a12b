"""The Monte-Carlo dropout launches driven directly: hmp_mc_accumulate_rows / hmp_mc_finish (csrc/evaluate.hip) on seeded scores, and
the descriptor entries hmp_head_tails_mc (csrc/semisup.hip, plain and pooled) and hmp_linear_heads_mc (csrc/heads.hip) over the case
lists of tests/test_gpu_tail_kernels.py, against the float64 restatement of tests/_mc_reference.py (which states the tolerances and
the label rule; every figure is printed before it is asserted).

Every buffer a launch writes starts as 0xA5 bytes: what the contract leaves alone -- the bytes behind every output, the pitch gap of
the accumulators, the rows outside a head, the columns of mean_probs at or past the classes -- must still hold them afterwards.  The
descriptor entries draw their tail dropout on the device; the expected scores apply the masks of the host restatement
(tests/_dropout_reference.py) at the same (seed, step + t, stream)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _dropout_reference import keep_mask as host_keep_mask  # noqa: E402
from _mc_reference import CLASSES, MAX_EXEMPT, ROWS, SAMPLES, SEEDS, check_mc, mc_reference, seeded_scores  # noqa: E402
from _tail_reference import _y, head_members  # noqa: E402
from hydra_gnn_amd import _lib, ops  # noqa: E402
from test_gpu_tail_kernels import HEAD_CASES, POOL_CASES, SEED, TAIL_ONE, TAIL_TWO, Heads, Tail, pooled_head  # noqa: E402

FILL = 0xA5
TAILB = 24  # bytes behind every output
HMP_E_ARG = 1


def dev():
    return torch.device("cuda:0")


def align4(x):
    return (x + 3) & ~3


def filled(nbytes):
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev())


def is_fill(t):
    return bool((t.contiguous().view(torch.uint8) == FILL).all())


def acc_ld(C_):
    return int(_lib.load().hmp_mc_acc_ld(C_))


class Acc:
    """accumulators [n, ld] inside 0xA5 bytes, TAILB more behind them"""

    def __init__(self, n, C_, pad=0, nan=False):
        self.n, self.C, self.ld = n, C_, acc_ld(C_) + pad
        self.raw = filled(4 * n * self.ld + TAILB)
        self.rows = self.raw[:4 * n * self.ld].view(torch.float32).view(n, self.ld)
        if nan:
            self.rows.fill_(float("nan"))

    def ptr(self):
        return self.raw.data_ptr()

    def used(self):
        """bool [ld]: the columns the layout names"""
        cp = align4(self.C)
        u = torch.zeros(self.ld, dtype=torch.bool)
        u[:self.C] = True
        u[cp:cp + self.C] = True
        u[2 * cp] = True
        return u

    def check_fill(self, members, tag):
        """the pitch gap of every row, the rows outside `members` and the bytes behind the buffer still hold the fill"""
        rows = self.rows.cpu()
        mem = torch.ones(self.n, dtype=torch.bool) if members is None else members
        assert is_fill(self.raw[4 * self.n * self.ld:]), f"{tag}: bytes behind the accumulators were written"
        assert is_fill(rows[:, ~self.used()]), f"{tag}: the pitch gap of the accumulators was written"
        assert is_fill(rows[~mem]), f"{tag}: the accumulators of a row outside the head were written"
        assert not bool(torch.isnan(rows[mem][:, self.used()]).any()), f"{tag}: NaN in the accumulators"


class Outs:
    """the five outputs of a finishing launch inside ONE 0xA5 buffer (one copy brings all down): labels [n], mean [n, C + 3],
    std / entropy / mutual_info [n], TAILB bytes behind each"""

    def __init__(self, n, C_):
        self.n, self.C, self.ldm = n, C_, C_ + 3
        sizes = [8 * n, 4 * n * self.ldm, 4 * n, 4 * n, 4 * n]
        self.off = np.cumsum([0] + [s + TAILB for s in sizes])
        self.sizes = sizes
        self.raw = filled(int(self.off[-1]))

    def ptrs(self, on=(True,) * 5):
        return [self.raw.data_ptr() + int(o) if use else None for o, use in zip(self.off[:5], on)]

    def fetch(self, tag, on=(True,) * 5):
        host = self.raw.cpu()
        part = lambda i: host[int(self.off[i]):int(self.off[i]) + self.sizes[i]]  # noqa: E731
        for i in range(5):
            assert is_fill(host[int(self.off[i]) + self.sizes[i]:int(self.off[i + 1])]), f"{tag}: bytes behind output {i} were written"
            if not on[i]:
                assert is_fill(part(i)), f"{tag}: the skipped output {i} was written"
        mean = part(1).view(torch.float32).view(self.n, self.ldm)
        if on[1]:
            assert is_fill(mean[:, self.C:]), f"{tag}: columns of mean_probs at or past the classes were written"
        return (part(0).view(torch.int64).numpy(), mean[:, :self.C].numpy().copy(), part(2).view(torch.float32).numpy(),
                part(3).view(torch.float32).numpy(), part(4).view(torch.float32).numpy())


def finish(acc, T, members, tag, on=(True,) * 5):
    out = Outs(acc.n, acc.C)
    p = out.ptrs(on)
    rc = _lib.load().hmp_mc_finish(acc.ptr(), acc.ld, acc.n, acc.C, T, members.data_ptr() if members is not None else None, p[0], p[1],
                                   out.ldm, p[2], p[3], p[4], _lib.stream_ptr())
    assert rc == 0, _lib.load().hmp_last_error()
    torch.cuda.synchronize()
    return out.fetch(tag, on)


def place(scores, walk):
    """scores float32 [T, n, C] on the device in the layout of `walk`: "vec" = 16-byte aligned base, pitch a multiple of 4 (the quad
    walk); "pitch" = an odd pitch; "base" = an aligned pitch behind a base 4 bytes past the alignment (the scalar walk).  Returns
    (storage, address of sample 0, ld, bytes per sample); the padding holds NaN (a sum that read it would show)."""
    T, n, C_ = scores.shape
    ld = align4(C_) + (4 if walk == "vec" else 1 if walk == "pitch" else 0)
    lead = 1 if walk == "base" else 0
    per = align4(n * ld) if walk != "pitch" else n * ld  # samples of the vec / base walks keep their alignment class
    buf = torch.full((lead + T * per + 4,), float("nan"), dtype=torch.float32)
    for t in range(T):
        buf[lead + t * per:lead + t * per + n * ld].view(n, ld)[:, :C_] = torch.from_numpy(scores[t])
    d = buf.to(dev())
    addr = d.data_ptr() + 4 * lead
    assert (addr % 16 == 0 and ld % 4 == 0) == (walk == "vec")
    return d, addr, ld, 4 * per


def accumulate(scores, walk, members, acc):
    d, addr, ld, per = place(scores, walk)
    T, n, C_ = scores.shape
    for t in range(T):
        rc = _lib.load().hmp_mc_accumulate_rows(addr + t * per, ld, n, C_, members.data_ptr() if members is not None else None,
                                                1 if t == 0 else 0, acc.ptr(), acc.ld, _lib.stream_ptr())
        assert rc == 0, _lib.load().hmp_last_error()
    return d


def members_of(n, seed):
    g = torch.Generator().manual_seed(900 + seed)
    m = torch.rand(n, generator=g) < 0.6
    if n >= 3:
        m[0], m[1] = False, True
    return m


# ---- 1. the op-level entries on the seeded scores ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", SAMPLES)
@pytest.mark.parametrize("seed", SEEDS)
def test_rows_against_the_reference(seed, T):
    """every (n, C) of the lists, on both walks, with and without members; the label rule's exemptions stay under the cap"""
    exempt = compared = 0
    for n in ROWS:
        for C_ in CLASSES:
            scores = seeded_scores(seed, T, n, C_)
            ref = mc_reference(scores)
            for walk in ("vec", "pitch" if (n + C_) % 2 else "base"):
                for with_members in (False, True):
                    tag = f"seed {seed} T {T} n {n} C {C_} {walk}{' members' if with_members else ''}"
                    mem = members_of(n, seed + n + C_) if with_members else None
                    d_mem = mem.to(dev()) if mem is not None else None
                    acc = Acc(n, C_, pad=3 if walk != "vec" else 0)
                    keep = accumulate(scores, walk, d_mem, acc)
                    got = finish(acc, T, d_mem, tag)
                    del keep
                    acc.check_fill(mem, tag)
                    e, c = check_mc(got, ref, T, C_, tag, None if mem is None else mem.numpy())
                    if not with_members and walk == "vec":
                        exempt, compared = exempt + e, compared + c
    print(f"seed {seed} T {T}: {exempt} of {compared} rows exempt from the label rule")
    assert compared == sum(ROWS) * len(CLASSES) and exempt <= MAX_EXEMPT * compared


@pytest.mark.parametrize("T", [1, 2, 4])
def test_identical_samples_equal_the_top1_kernel_bit_for_bit(T):
    """T = 1, and T = 2 / 4 copies of one sample (sums and divisions by powers of two are exact): mean_probs[r, label] is column 0 of
    hmp_topk_rows' probabilities, labels are hmp_predict_rows', on both walks"""
    for n in ROWS:
        for C_ in CLASSES:
            s = seeded_scores(12, 1, n, C_)
            scores = np.repeat(s, T, axis=0)
            x = torch.from_numpy(s[0]).to(dev())
            top_l, top_p = ops.topk_rows(x, 1)
            pred = ops.predict_rows(x)
            for walk in ("vec", "base", "pitch"):
                tag = f"T {T} n {n} C {C_} {walk}"
                acc = Acc(n, C_)
                keep = accumulate(scores, walk, None, acc)
                labels, mean, sd, ent, mi = finish(acc, T, None, tag)
                del keep
                labels = torch.from_numpy(labels)
                assert torch.equal(labels, pred.cpu()) and torch.equal(labels, top_l[:, 0].cpu()), tag
                conf = torch.from_numpy(mean).gather(1, labels[:, None])[:, 0]
                assert torch.equal(conf, top_p[:, 0].cpu()), f"{tag}: mean_probs[label] is not the top-1 probability"
                assert float(np.abs(sd).max()) <= 2.0 ** -11, tag  # sqrt of one rounding of p^2 against p * p


def test_every_probability_of_one_sample_is_the_topk_kernels():
    """C <= 8: the k = C columns of hmp_topk_rows name every class, so all of mean_probs is compared bit for bit"""
    for C_ in (1, 2, 3, 4, 5, 8):
        for n in (1, 65):
            s = seeded_scores(13, 1, n, C_)
            x = torch.from_numpy(s[0]).to(dev())
            top_l, top_p = ops.topk_rows(x, C_)
            acc = Acc(n, C_)
            keep = accumulate(s, "vec", None, acc)
            _, mean, _, _, _ = finish(acc, 1, None, f"C {C_} n {n}")
            del keep
            want = torch.zeros(n, C_).scatter_(1, top_l.cpu(), top_p.cpu())
            assert torch.equal(torch.from_numpy(mean), want), f"C {C_} n {n}"


@pytest.mark.parametrize("walk", ["vec", "pitch"])
def test_a_nan_filled_accumulator_with_first_equals_a_zeroed_one_and_two_runs_are_bit_equal(walk):
    T, n, C_ = 3, 65, 17
    scores = seeded_scores(11, T, n, C_)
    mem = members_of(n, 4).to(dev())
    runs = []
    for kind in ("fill", "nan", "zero", "fill"):
        acc = Acc(n, C_, nan=kind == "nan")
        if kind == "zero":
            acc.rows.zero_()
        keep = accumulate(scores, walk, mem, acc)
        got = finish(acc, T, mem, f"{walk} {kind}")
        del keep
        used = acc.rows.cpu()[mem.cpu()][:, acc.used()]
        runs.append((used, got))
    for used, got in runs[1:]:
        assert torch.equal(used.view(torch.int32), runs[0][0].view(torch.int32))
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, runs[0][1]))


def test_null_outputs_are_skipped_and_not_all_may_be_null():
    T, n, C_ = 2, 33, 5
    scores = seeded_scores(12, T, n, C_)
    acc = Acc(n, C_)
    keep = accumulate(scores, "vec", None, acc)
    full = finish(acc, T, None, "all outputs")
    for on in ((True, False, False, False, False), (False, True, False, False, False), (False, False, True, False, True),
               (False, False, False, True, False)):
        got = finish(acc, T, None, f"outputs {on}", on)
        for i in range(5):
            if on[i]:
                assert np.array_equal(got[i], full[i])
    del keep
    lib = _lib.load()
    assert lib.hmp_mc_finish(acc.ptr(), acc.ld, n, C_, T, None, None, None, C_, None, None, None, _lib.stream_ptr()) == HMP_E_ARG
    assert b"no output" in lib.hmp_last_error()


def test_no_rows_launch_nothing_and_bad_ranges_are_refused():
    lib = _lib.load()
    acc = Acc(4, 5)
    x = torch.zeros(4, 8, device=dev())
    assert lib.hmp_mc_accumulate_rows(x.data_ptr(), 8, 0, 5, None, 1, acc.ptr(), acc.ld, _lib.stream_ptr()) == 0
    out = Outs(4, 5)
    p = out.ptrs()
    assert lib.hmp_mc_finish(acc.ptr(), acc.ld, 0, 5, 3, None, p[0], p[1], out.ldm, p[2], p[3], p[4], _lib.stream_ptr()) == 0
    for T in (0, 4097):
        assert lib.hmp_mc_finish(acc.ptr(), acc.ld, 4, 5, T, None, p[0], p[1], out.ldm, p[2], p[3], p[4], _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_mc_finish(acc.ptr(), 2 * 8, 4, 5, 3, None, p[0], p[1], out.ldm, p[2], p[3], p[4], _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_mc_finish(acc.ptr(), acc.ld, 4, 5, 3, None, p[0], p[1], 4, p[2], p[3], p[4], _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_mc_accumulate_rows(x.data_ptr(), 8, 4, 5, None, 1, acc.ptr(), 2 * 8, _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_mc_accumulate_rows(x.data_ptr(), 4, 4, 5, None, 1, acc.ptr(), acc.ld, _lib.stream_ptr()) == HMP_E_ARG  # ld < classes
    torch.cuda.synchronize()
    assert is_fill(acc.raw) and is_fill(out.raw)


def test_the_operators_wrap_the_entries():
    T, n, C_ = 3, 64, 26
    scores = seeded_scores(13, T, n, C_)
    ref = mc_reference(scores)
    mem = members_of(n, 9)
    acc = ops.mc_acc(n, C_, dev())
    assert tuple(acc.shape) == (n, acc_ld(C_)) and acc.dtype == torch.float32
    for t in range(T):
        assert ops.mc_accumulate_rows(torch.from_numpy(scores[t]).to(dev()), acc, t == 0, mem.to(dev())) is acc
    got = ops.mc_finish(acc, C_, T, mem.to(dev()))
    assert [tuple(g.shape) for g in got] == [(n,), (n, C_), (n,), (n,), (n,)]
    check_mc([g.cpu().numpy() for g in got], ref, T, C_, "ops", mem.numpy())
    bufs = (torch.full((n + 2,), -7, dtype=torch.int64, device=dev()), torch.full((n + 2, C_), -7.0, device=dev()),
            torch.full((n + 2,), -7.0, device=dev()), torch.full((n + 2,), -7.0, device=dev()), torch.full((n + 2,), -7.0, device=dev()))
    views = ops.mc_finish(acc, C_, T, mem.to(dev()), out=bufs)
    assert all(v.data_ptr() == b.data_ptr() and torch.equal(v, g) and bool((b[n:] == -7).all()) for v, b, g in zip(views, bufs, got))
    with pytest.raises(_lib.HydraMPError, match="acc"):
        ops.mc_accumulate_rows(torch.zeros(n, C_, device=dev()), acc[:, :2 * C_], True)
    with pytest.raises(_lib.HydraMPError, match="rows"):
        ops.mc_accumulate_rows(torch.zeros(n - 1, C_, device=dev()), acc, True)


# ---- 2. the descriptor entries -------------------------------------------------------------------------------------------------------
MC_T = 3


def tail_sample_scores(h, t, pooled, dtype=torch.float64):
    """scores of sample t of a Tail: y = keep * act(z) / (1 - p) with the host restatement's mask at step + t, pooled or not"""
    keep = torch.from_numpy(host_keep_mask(SEED, h.step + t, h.stream, h.p, h.n_rows, h.classes)) if h.p > 0 else None
    _, y = _y(h.z[:h.n_rows], h.classes, h.act, keep, h.p, dtype)
    y = y.detach()
    if not pooled or h.pool is None:
        return y.numpy()
    rowptr = torch.as_tensor(np.asarray(h.pool[0]), dtype=torch.int64)
    col = torch.as_tensor(np.asarray(h.pool[1]), dtype=torch.int64)
    deg = rowptr[1:] - rowptr[:-1]
    seg = torch.repeat_interleave(torch.arange(h.n_pool), deg)
    return (torch.zeros(h.n_pool, h.classes, dtype=dtype).index_add(0, seg, y[col]) / deg.clamp(min=1).to(dtype)[:, None]).numpy()


def run_tails_mc(heads, pooled, act, T=MC_T, skip=()):
    """T samples of the heads into fresh accumulators: per head (Acc or None, finished outputs or None)"""
    rows = [h.n_pool if pooled else h.n_rows for h in heads]
    accs = [Acc(n, h.classes, pad=4 * (i % 2)) if i not in skip else None for i, (n, h) in enumerate(zip(rows, heads))]
    ptrs = (C.c_void_p * len(heads))(*[a.ptr() if a is not None else None for a in accs])
    lds = (C.c_int32 * len(heads))(*[a.ld if a is not None else 0 for a in accs])
    for t in range(T):
        descs = []
        for h in heads:
            d = h.desc(None, pooled)
            d.rng_step = h.step + t
            descs.append(d)
        arr = (_lib.TailDesc * len(heads))(*descs)
        rc = _lib.load().hmp_head_tails_mc(arr, len(heads), int(pooled), act, 1 if t == 0 else 0, ptrs, lds, _lib.stream_ptr())
        assert rc == 0, _lib.load().hmp_last_error()
    torch.cuda.synchronize()
    return accs


def check_tail_mc(h, acc, pooled, T, tag):
    n = h.n_pool if pooled else h.n_rows
    if n == 0:
        assert is_fill(acc.raw), f"{tag}: a head without rows wrote"
        return
    s64 = np.stack([tail_sample_scores(h, t, pooled) for t in range(T)])
    s32 = np.stack([tail_sample_scores(h, t, pooled, torch.float32) for t in range(T)])
    ref = mc_reference(s64)
    got = finish(acc, T, None, tag)
    acc.check_fill(None, tag)
    check_mc(got, ref, T, h.classes, tag, score_err=float(np.abs(s32.astype(np.float64) - s64).max()))  # the yardstick of the scores
    return got, ref


SMALL_TAIL_ONE = [c for c in TAIL_ONE if c[0] <= 17] + [(130, 41, 1, 0.25, (8, 4), False), (65, 15, 2, 0.25, (0, 0), False)]


@pytest.mark.parametrize("case", range(len(SMALL_TAIL_ONE)))
def test_unpooled_tail(case):
    rows, classes, act, p, (ldz_pad, _), _ = SMALL_TAIL_ONE[case]
    p = p or 0.25  # the tail draws in every case
    h = Tail(rows, classes, act, p, ldz_pad=ldz_pad, seed=case, slot=case % 2)
    tag = f"tail mc {rows}x{classes} act {act} p {p}"
    accs = run_tails_mc([h], False, act)
    check_tail_mc(h, accs[0], False, MC_T, tag)
    again = run_tails_mc([h], False, act)
    assert torch.equal(accs[0].raw, again[0].raw), f"{tag}: two runs differ"


@pytest.mark.parametrize("case", range(len(TAIL_TWO)))
def test_two_tails_ride_in_one_launch(case):
    """(17, 33): entry 1 starts in block 2; (0, 40) / (40, 0): an entry without rows next to a full one, with and without its
    accumulator (the head-skipping NULL rule: a NULL accumulator needs a head without rows)"""
    (r0, c0), (r1, c1), act, p, _ = TAIL_TWO[case]
    heads = [Tail(r0, c0, act, p or 0.25, ldz_pad=8, seed=50 + case, slot=0), Tail(r1, c1, act, 0.25, ldz_pad=0, seed=80 + case, slot=1)]
    tag = f"tails mc {r0}x{c0} + {r1}x{c1} act {act}"
    accs = run_tails_mc(heads, False, act)
    for i, (h, a) in enumerate(zip(heads, accs)):
        check_tail_mc(h, a, False, MC_T, f"{tag} head {i}")
    empty = [i for i, h in enumerate(heads) if h.n_rows == 0]
    if empty:
        skipped = run_tails_mc(heads, False, act, skip=empty)
        for i, a in enumerate(skipped):
            assert a is None or torch.equal(a.raw, accs[i].raw)
    else:  # a head with rows and no accumulator is refused and nothing is launched
        lib = _lib.load()
        acc = Acc(heads[1].n_rows, heads[1].classes)
        arr = (_lib.TailDesc * 2)(*[h.desc(None, False) for h in heads])
        rc = lib.hmp_head_tails_mc(arr, 2, 0, act, 1, (C.c_void_p * 2)(None, acc.ptr()), (C.c_int32 * 2)(0, acc.ld), _lib.stream_ptr())
        assert rc == HMP_E_ARG and b"no accumulator" in lib.hmp_last_error()
        torch.cuda.synchronize()
        assert is_fill(acc.raw)


@pytest.mark.parametrize("case", range(len(POOL_CASES)))
def test_pooled_tail(case):
    """pool degrees 0, 1, 2, 37 and 300 ("mixed"), leaves with 0 / 1 / 2 pool edges, no edge at all: an empty pooled row is all zeros,
    p = 1 / C in every sample"""
    profile, classes, act, p = POOL_CASES[case]
    h = pooled_head(profile, classes, act, p or 0.25, case, case % 2, False)
    tag = f"pool mc {profile} classes {classes} act {act}"
    accs = run_tails_mc([h], True, act)
    got, ref = check_tail_mc(h, accs[0], True, MC_T, tag)
    empty = np.diff(np.asarray(h.csr[0])) == 0
    if empty.any():
        assert float(np.abs(got[1][empty].astype(np.float64) - 1.0 / classes).max()) <= 1e-7 and (got[0][empty] == 0).all()
        assert float(np.abs(got[4][empty]).max()) <= 1e-6 and float(np.abs(got[2][empty]).max()) <= 2.0 ** -11


def test_pooled_head_next_to_an_identity_pool():
    act = 1
    pooled = pooled_head("mixed", 41, act, 0.25, 7, 0, False)
    ident = Tail(33, 15, act, 0.25, ldz_pad=8, seed=300, slot=1)  # rowptr NULL: row v's only leaf is v
    for heads in ([pooled, ident], [ident, pooled]):
        accs = run_tails_mc(heads, True, act)
        for h, a in zip(heads, accs):
            check_tail_mc(h, a, True, MC_T, f"pool+identity mc (first {'pooled' if heads[0] is pooled else 'identity'})")


def test_tail_launcher_refusals():
    lib = _lib.load()
    h = Tail(17, 5, 1, 0.25, seed=1)
    acc = Acc(17, 5)
    arr = (_lib.TailDesc * 1)(h.desc(None, False))
    ptrs, good = (C.c_void_p * 1)(acc.ptr()), (C.c_int32 * 1)(acc.ld)
    assert lib.hmp_head_tails_mc(arr, 1, 0, 1, 1, ptrs, (C.c_int32 * 1)(16), _lib.stream_ptr()) == HMP_E_ARG and b"ld_acc" in lib.hmp_last_error()
    assert lib.hmp_head_tails_mc(arr, 1, 0, 1, 1, None, good, _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_head_tails_mc(arr, 1, 0, 1, 1, ptrs, None, _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_head_tails_mc(arr, 3, 0, 1, 1, ptrs, good, _lib.stream_ptr()) == HMP_E_ARG
    d = h.desc(None, False)
    d.p = 1.0
    assert lib.hmp_head_tails_mc((_lib.TailDesc * 1)(d), 1, 0, 1, 1, ptrs, good, _lib.stream_ptr()) == HMP_E_ARG
    wide = Tail(17, 257, 1, 0.25, seed=2)
    wacc = Acc(17, 257)
    rc = lib.hmp_head_tails_mc((_lib.TailDesc * 1)(wide.desc(None, True)), 1, 1, 1, 1, (C.c_void_p * 1)(wacc.ptr()), (C.c_int32 * 1)(wacc.ld),
                               _lib.stream_ptr())
    assert rc == HMP_E_ARG and b"classes" in lib.hmp_last_error()  # pooled rows live in registers: at most 256 classes
    torch.cuda.synchronize()
    assert is_fill(acc.raw) and is_fill(wacc.raw)


# ---- linear heads ---------------------------------------------------------------------------------------------------------------------
SMALL_HEAD_CASES = [c for c in HEAD_CASES if c[3] <= 65] + [((15, 41), 30, 0, 65, "both_given", 1, 0.25)]


def head_sample_scores(H, t, dtype=torch.float64):
    keep = torch.from_numpy(host_keep_mask(SEED, H.step + t, H.stream, H.p, H.n_rows, H.F)) if H.p > 0 else None
    _, y = _y(H.z[:H.n_rows], H.F, H.act, keep, H.p, dtype)
    return [(y @ w.to(dtype).t() + b.to(dtype)).detach().numpy() for w, b in zip(H.W, H.b)]


def run_heads_mc(H, T=MC_T, on=(True, True)):
    accs = [Acc(H.n_rows, c, pad=4 * h) if on[h] else None for h, c in enumerate(H.classes)]
    ptrs = (C.c_void_p * 2)(*[a.ptr() if a is not None else None for a in accs])
    lds = (C.c_int32 * 2)(*[a.ld if a is not None else 0 for a in accs])
    nb = C.c_int32(-1)
    for t in range(T):
        rc = _lib.load().hmp_linear_heads_mc(C.byref(H.desc(None, rng_step=H.step + t)), 1 if t == 0 else 0, ptrs, lds, C.byref(nb),
                                             _lib.stream_ptr())
        assert rc == 0, _lib.load().hmp_last_error()
    torch.cuda.synchronize()
    return accs, nb.value


@pytest.mark.parametrize("case", range(len(SMALL_HEAD_CASES)))
def test_linear_heads(case):
    """rows 1 / 31 / 32 / 33 / 65 against the 32-row tile, classes 1 .. 64, F up to 1024 (16 LDS chunks), the three member patterns"""
    classes, F, ldz_pad, n_rows, members, act, p = SMALL_HEAD_CASES[case]
    H = Heads(classes, F, n_rows, act, p or 0.25, ldz_pad=ldz_pad, members=members, seed=case)
    tag = f"heads mc {classes} F {F} rows {n_rows} {members} act {act}"
    accs, nb = run_heads_mc(H)
    assert nb == min(-(-n_rows // 32), 240)
    mem = head_members(n_rows, H.member[0], H.member[1])
    samples = [head_sample_scores(H, t) for t in range(MC_T)]
    samples32 = [head_sample_scores(H, t, torch.float32) for t in range(MC_T)]
    for h in range(2):
        s64 = np.stack([s[h] for s in samples])
        yard = float(np.abs(np.stack([s[h] for s in samples32]).astype(np.float64) - s64).max()) if n_rows else 0.0
        ref = mc_reference(s64)
        got = finish(accs[h], MC_T, mem[h].to(dev()), f"{tag} head {h}")
        accs[h].check_fill(mem[h], f"{tag} head {h}")
        check_mc(got, ref, MC_T, classes[h], f"{tag} head {h}", mem[h].numpy(), score_err=yard)  # the yardstick of the logits
    again, _ = run_heads_mc(H)
    assert all(torch.equal(a.raw, b.raw) for a, b in zip(accs, again)), f"{tag}: two runs differ"
    # a NULL accumulator skips its head, the other head's bytes do not change
    for on in ((True, False), (False, True)):
        part, _ = run_heads_mc(H, on=on)
        for h in range(2):
            assert part[h] is None or torch.equal(part[h].raw, accs[h].raw), f"{tag}: head {h} with the other skipped"


def test_linear_heads_without_rows_launch_nothing_and_refusals():
    lib = _lib.load()
    H = Heads((15, 35), 16, 0, 1, 0.25, seed=5)
    accs, nb = run_heads_mc(H)
    assert nb == 0
    H = Heads((3, 2), 64, 40, 1, 0.25, seed=90)
    accs = [Acc(40, 3), Acc(40, 2)]
    ptrs = (C.c_void_p * 2)(accs[0].ptr(), accs[1].ptr())
    good = (C.c_int32 * 2)(accs[0].ld, accs[1].ld)
    assert lib.hmp_linear_heads_mc(C.byref(H.desc(None)), 1, ptrs, (C.c_int32 * 2)(accs[0].ld, 8), None, _lib.stream_ptr()) == HMP_E_ARG
    assert b"ld_acc" in lib.hmp_last_error()
    assert lib.hmp_linear_heads_mc(C.byref(H.desc(None)), 1, None, good, None, _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_linear_heads_mc(C.byref(H.desc(None, p=1.0)), 1, ptrs, good, None, _lib.stream_ptr()) == HMP_E_ARG
    assert lib.hmp_linear_heads_mc(C.byref(H.desc(None, F=1025)), 1, ptrs, good, None, _lib.stream_ptr()) == HMP_E_ARG
    torch.cuda.synchronize()
    assert all(is_fill(a.raw) for a in accs)
