"""The grouped GEMM launchers as the executor calls them (hmp_gemm_grouped): gemm_launch (fp32 tiled classes, the tall TN kernel,
the x3 kernel), gemm_bf16_launch (128 / 256 tiles, dw / tiled peeling) and gemm_tn_direct_launch, with split-K slabs, the virtual
ones column, the EPI_ACTMASK epilogue, the Cadd addend and multi-problem batches.

Every result is compared element by element with a float64 product of the operands as stored (rounded to bf16 first on the bf16
route): |error| <= c * (|op(A)| @ |op([B | 1])| + |Cadd|) * |act'(H)|, c = 2e-6 (the bar of the x3 test in test_gpu_ops.py).
Split-K launches: every slab starts as NaN, the result is the float64 sum of slabs 0 .. ksplit_out[i] - 1; those slabs must be
written inside [M, N] and nothing else (later slabs, columns [N, ldc), rows past M) may be touched.  Which kernel ran is shown by
ksplit_out (the split only the intended tile plan produces: a mirror of the launchers' planning below) or by a bitwise difference
from the other setting of the launcher's switch."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib  # noqa: E402

TOL = 2e-6
ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2
EPI_ACTMASK = 1
TALL_SLABS = 192  # GEMM_TALL_SLABS: the tall kernel's own cap (the executor's slab buffer holds that many)


def dev():
    return torch.device("cuda:0")


def cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def randn(rows, cols, seed, dtype=torch.float32):
    """operand storage (cached across parametrizations; never written by a launch)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(max(rows, 1), max(cols, 1), device=dev(), generator=g).to(dtype)


class Prob:
    """One problem of a launch: operand storage, its descriptor and its float64 reference.

    A is op(A) = [M, K] (stored [K][M] when trans_a), B has n_real columns (stored [n_real][K] when trans_b), N = n_real + aug.
    a_off shifts A's first element by that many elements (an unaligned operand); slabs: C holds that many slabs of M + 2 rows."""

    def __init__(self, M, n_real, K, ta=0, tb=0, aug=0, *, seed=0, lda_pad=0, ldb_pad=0, ldc_pad=0, a_off=0, a16=False, b16=False,
                 epi=False, act=ACT_NONE, drop_p=0.0, h16=False, cadd=False, slabs=1, bf16_route=False, A=None, B=None):
        self.M, self.n_real, self.K, self.ta, self.tb, self.aug = M, n_real, K, ta, tb, aug
        self.N = N = n_real + aug
        ar, ac = (K, M) if ta else (M, K)
        br, bc = (n_real, K) if tb else (K, n_real)
        self.A_st = A if A is not None else randn(ar, ac + lda_pad + a_off, seed * 4 + 1, torch.bfloat16 if a16 else torch.float32)
        self.B_st = B if B is not None else randn(br, bc + ldb_pad, seed * 4 + 2, torch.bfloat16 if b16 else torch.float32)
        assert self.A_st.shape[0] >= max(ar, 1) and self.A_st.shape[1] >= ac + a_off and self.B_st.shape[0] >= max(br, 1)
        self.a_off = a_off
        A = self.A_st[:ar, a_off:a_off + ac].double()
        B = self.B_st[:br, :bc].double()
        if bf16_route:  # the bf16 launcher rounds fp32 operands to bf16 (nearest even) on their way into LDS
            if not a16:
                A = self.A_st[:ar, a_off:a_off + ac].to(torch.bfloat16).double()
            if not b16:
                B = self.B_st[:br, :bc].to(torch.bfloat16).double()
        opA = A.t() if ta else A
        opB = B.t() if tb else B
        if aug:
            opB = torch.cat([opB, torch.ones(K, 1, dtype=torch.float64, device=dev())], 1)
        ref = opA @ opB
        scale = opA.abs() @ opB.abs()
        self.ldc = max(N + ldc_pad, 1)
        self.slab_rows = M + 2
        self.C_all = torch.full((slabs, self.slab_rows, self.ldc), float("nan"), device=dev())
        self.Cadd = self.H = None
        if cadd:
            self.Cadd = randn(M, N + 2, seed * 4 + 3)
            c = self.Cadd[:M, :N].double()
            ref = ref + c
            scale = scale + c.abs()
        self.epi, self.act, self.drop_p, self.h16 = epi, act, drop_p, h16
        if epi:
            self.H = make_h(M, N, act, drop_p, seed * 4 + 4, h16)
            f = act_factor(self.H[:M, :N].double(), act, drop_p)
            ref = ref * f
            scale = scale * f.abs()
        self.ref, self.scale = ref, scale
        self.a16, self.b16 = a16, b16

    def desc(self):
        d = _lib.GemmDesc()
        es_a = self.A_st.element_size()
        d.A = self.A_st.data_ptr() + self.a_off * es_a
        d.B = self.B_st.data_ptr()
        d.C = self.C_all.data_ptr()
        d.M, d.N, d.K = self.M, self.N, self.K
        d.lda, d.ldb, d.ldc = self.A_st.stride(0), self.B_st.stride(0), self.ldc
        d.trans_a, d.trans_b = self.ta, self.tb
        d.n_real, d.aug_ones = self.n_real, self.aug
        d.slab_stride = self.slab_rows * self.ldc
        d.a_bf16, d.b_bf16 = int(self.a16), int(self.b16)
        if self.Cadd is not None:
            d.Cadd, d.ldadd = self.Cadd.data_ptr(), self.Cadd.stride(0)
        if self.epi:
            d.epi, d.act, d.drop_p = EPI_ACTMASK, self.act, self.drop_p
            d.H, d.ldh, d.h_bf16 = self.H.data_ptr(), self.H.stride(0), int(self.h16)
        return d

    def reset(self):
        self.C_all.fill_(float("nan"))

    def check(self, ks, max_slabs, tag=""):
        """the slabs are exactly what ksplit_out says, and their sum is the product within the per-element bound"""
        M, N = self.M, self.N
        assert 1 <= ks <= max_slabs, (tag, ks, max_slabs)
        Cs = self.C_all
        assert torch.isnan(Cs[ks:]).all(), (tag, "a slab past ksplit_out was written", ks)
        assert torch.isnan(Cs[:, M:, :]).all(), (tag, "rows past M were written")
        assert torch.isnan(Cs[:, :, N:]).all(), (tag, "columns [N, ldc) were written")
        if M == 0 or N == 0:
            return None
        live = Cs[:ks, :M, :N]
        assert not torch.isnan(live).any(), (tag, "a slab below ksplit_out was left unwritten", ks)
        got = live.double().sum(0)
        err = (got - self.ref).abs()
        bound = TOL * self.scale
        bad = err > bound
        assert not bad.any(), (tag, "max excess", (err - bound).max().item(), "at", bad.nonzero()[:4].tolist(), "ks", ks)
        return got


def make_h(M, N, act, drop_p, seed, h16):
    """stored activations y = dropout(act(z)): negative ELU outputs, +0.0 kept zeros, and -0.0 for dropped elements"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ld = N + 3
    z = torch.randn(max(M, 1), ld, device=dev(), generator=g)
    scale = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(drop_p))) if drop_p > 0 else 1.0
    if act == ACT_RELU:
        y = torch.relu(z)
    elif act == ACT_ELU:
        y = torch.nn.functional.elu(z)
    else:
        y = z.clone()
    y = y * scale
    u = torch.rand(max(M, 1), ld, device=dev(), generator=g)
    y = torch.where(u < 0.1, torch.zeros_like(y), y)  # +0.0 kept zeros (and ReLU's own)
    if drop_p > 0:
        y = torch.where((u >= 0.1) & (u < 0.1 + drop_p), torch.full_like(y, -0.0), y)
    return y.to(torch.bfloat16) if h16 else y


def act_factor(h, act, drop_p):
    """d out / d pre from the stored output (float64 from the stored values; the scale is the fp32 1 / (1 - p) of make_drop)"""
    s = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(drop_p))) if drop_p > 0 else 1.0
    if act == ACT_RELU:
        f = torch.where(h > 0, torch.full_like(h, s), torch.zeros_like(h))
    elif act == ACT_ELU:
        f = torch.where(h > 0, torch.full_like(h, s), h + s)
    else:
        f = torch.full_like(h, s)
    if drop_p > 0:
        f = torch.where((h == 0) & torch.signbit(h), torch.zeros_like(h), f)
    return f


def launch(probs, route, want_split, max_slabs):
    lib = _lib.require_device()
    n = len(probs)
    for p in probs:
        if want_split:  # room for every slab the launcher may write (the tall kernel: up to 192; the bf16 128 tile: up to 64)
            need = max(max_slabs, 64 if route == 1 else 1, TALL_SLABS if route == 0 and p.K >= 32768 else 1)
            if p.C_all.shape[0] < need:
                p.C_all = torch.empty(need, p.slab_rows, p.ldc, device=dev())
        p.reset()
    arr = (_lib.GemmDesc * max(n, 1))(*[p.desc() for p in probs])
    ks = (C.c_int32 * max(n, 1))()
    torch.cuda.synchronize()
    _lib.check(lib.hmp_gemm_grouped(arr, n, route, int(want_split), max_slabs, ks, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return [ks[i] for i in range(n)]


def run_check(probs, route, want_split, max_slabs, tag="", cap=None):
    ks = launch(probs, route, want_split, max_slabs)
    outs = []
    for i, (p, k) in enumerate(zip(probs, ks)):
        outs.append(p.check(k, cap[i] if cap else (max_slabs if want_split else 1), f"{tag}[{i}]"))
    return ks, outs


# ---- mirrors of the launchers' split planning (the evidence of which kernel ran) -------------------------------------------
def plan_tiled(probs, BM, BN, BK, max_slabs, want_split=True):
    """gemm.hip launch_cfg through gemm_plan_tiles: power-of-two split aiming at 1024 workgroups"""
    tiles = [cdiv(p.M, BM) * cdiv(p.N, BN) for p in probs]
    all_tiles = sum(tiles)
    out = []
    for p, t in zip(probs, tiles):
        ks = 1
        if want_split and t > 0:
            ks = max(1, min(1024 // all_tiles, cdiv(p.K, BK), max_slabs))
            while ks & (ks - 1):
                ks &= ks - 1
        kchunk = max(BK, cdiv(cdiv(p.K, ks), BK) * BK)
        out.append(cdiv(p.K, kchunk) if p.K > 0 else 1)
    return out


def plan_tall(probs):
    """gemm.hip tall_launch: ~512 workgroups shared out by K x slices, <= GEMM_TALL_SLABS"""
    ns = [cdiv(p.N, 80) for p in probs]
    work = sum(p.K * n for p, n in zip(probs, ns))
    out = []
    for p, n in zip(probs, ns):
        ks = int(512.0 * (p.K * n / work) / n + 0.5)
        ks = min(max(ks, 1), TALL_SLABS)
        kchunk = cdiv(cdiv(p.K, ks), 32) * 32
        out.append(cdiv(p.K, kchunk))
    return out


def plan_bf16_128(probs, max_slabs):
    """gemm_bf16.hip, 128 x 128 tiles (ones column folded into the first column tile), BK 64, <= 64 slabs"""
    tiles = [cdiv(p.M, 128) * cdiv(p.n_real if p.n_real > 0 else 1, 128) if p.aug else cdiv(p.M, 128) * cdiv(p.N, 128) for p in probs]
    all_tiles = sum(tiles)
    out = []
    for p, t in zip(probs, tiles):
        ks = max(1, min(1024 // all_tiles, cdiv(p.K, 64), 64)) if t > 0 else 1
        kchunk = max(64, cdiv(cdiv(p.K, ks), 64) * 64)
        out.append(cdiv(p.K, kchunk) if p.K > 0 else 1)
    return out


def plan_x3(probs, RM, RN, per_cu, max_slabs):
    """gemm_x3.hip x3_launch_cfg: one workgroup per CU and resident slot, K stages of 32, the ones column folded"""
    tiles = [cdiv(p.M, RM) * cdiv((p.n_real if p.n_real > 0 else 1) if p.aug else p.N, RN) for p in probs]
    all_tiles = sum(tiles)
    out = []
    for p, t in zip(probs, tiles):
        ks = max(1, min(256 * per_cu // all_tiles, cdiv(p.K, 32), max_slabs)) if t > 0 else 1
        kchunk = max(32, cdiv(cdiv(p.K, ks), 32) * 32)
        out.append(cdiv(p.K, kchunk) if p.K > 0 else 1)
    return out


def plan_direct(p, max_slabs):
    """gemm_direct.hip: None when the kernel declines"""
    tiles = cdiv(p.M, 32) * cdiv(p.N, 32)
    trips = 4 if tiles >= 512 else 2
    ks = max(1, cdiv(p.K, 2 * 4 * 24 * trips))
    if ks > max_slabs:
        return None
    while ks * 2 <= max_slabs and cdiv(p.K, ks * 2) >= 32 and tiles * ks < 256:
        ks *= 2
    kchunk = max(2, cdiv(cdiv(p.K, ks), 2) * 2)
    return cdiv(p.K, kchunk) if p.K > 0 else 1


# ---- fp32 tiled kernel: every tile class, form, split ------------------------------------------------------------------------
FORMS = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0), "TT": (1, 1)}
# class -> (shape of the split launch, shape of the plain launch, tile plan); the shapes are ragged in M, N and K
CLASSES = {
    "32x32_bk64": ((100, 70, 50), (100, 70, 50), (32, 32, 64)),        # K below one stage
    "32x32_bk128": ((100, 70, 1000), (100, 70, 1000), (32, 32, 128)),
    "64x64": ((2000, 200, 3000), (2000, 200, 3000), (64, 64, 32)),     # >= 10^9 MACs, N < 256
    "128x128": ((300, 270, 12400), (4096, 1024, 256), (128, 128, 32)),  # split: deep K; plain: >= 256 tiles of 128
}


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("form", list(FORMS))
def test_fp32_tiled_classes_forms_and_split(cls, form, monkeypatch):
    monkeypatch.setenv("HMP_GEMM_X3", "0")
    monkeypatch.delenv("HMP_GEMM_BIG", raising=False)
    ta, tb = FORMS[form]
    split_shape, plain_shape, (BM, BN, BK) = CLASSES[cls]
    for want_split, (M, N, K) in ((True, split_shape), (False, plain_shape)):
        p = Prob(M, N, K, ta, tb, seed=M + N + K, lda_pad=1, ldb_pad=2, ldc_pad=3)
        ks, outs = run_check([p], 0, want_split, 64, f"{cls}/{form}/split={want_split}")
        if want_split:
            assert ks == plan_tiled([p], BM, BN, BK, 64), (cls, ks)
            for other in {(32, 32, 128), (64, 64, 32), (128, 128, 32)} - {(BM, BN, BK)}:
                if K > 64:  # (at K <= 64 every class has one slab)
                    assert plan_tiled([p], *other, 64) != ks, (cls, other)
        if cls == "128x128":  # HMP_GEMM_BIG=0: the same launch on 64x64 tiles (the same k-ordered fp32 chain per element: only the
            # split tells the two apart)
            monkeypatch.setenv("HMP_GEMM_BIG", "0")
            ks0, _ = run_check([p], 0, want_split, 64, f"{cls}/{form}/BIG=0")
            monkeypatch.delenv("HMP_GEMM_BIG")
            if want_split:
                assert ks0 == plan_tiled([p], 64, 64, 32, 64) != ks


def test_fp32_ragged_k_and_empty_problems(monkeypatch):
    """K = 0 (the product is zero, one slab written), K below one stage, K one past a stage; padded pitches; an unaligned A"""
    monkeypatch.setenv("HMP_GEMM_X3", "0")
    for want_split in (True, False):
        probs = [Prob(37, 45, 0, 0, 0, seed=1, ldc_pad=5), Prob(37, 45, 1, 1, 0, seed=2), Prob(65, 33, 129, 0, 1, seed=3, a_off=1),
                 Prob(33, 31, 257, 1, 0, seed=4, lda_pad=3, ldb_pad=1, ldc_pad=1)]
        ks, outs = run_check(probs, 0, want_split, 64, f"ragged/split={want_split}")
        assert (outs[0] == 0).all()
        if want_split:
            assert ks == plan_tiled(probs, 32, 32, 128, 64)


@pytest.mark.parametrize("want_split", [True, False])
def test_fp32_mixed_forms_in_one_launch(want_split, monkeypatch):
    """launch_form 3 (the run-time layout variant): NT, NN, TN, TT problems in one table, ones columns on the NN / TN problems, an
    empty problem in the middle (the tile_start search walks past it).  The same table on the bf16 route (128 x 128 tiles), and a
    mixed NT / NN / TN table of just over 10^9 multiply-adds on the x3 kernel (square and narrow tile; its ones column belongs to
    the TN problem only): the three kernels share the tile walk and the epilogue."""
    monkeypatch.setenv("HMP_GEMM_X3", "0")
    monkeypatch.delenv("HMP_GEMM_X3_TILE", raising=False)
    probs = [Prob(70, 50, 300, 0, 1, seed=11), Prob(40, 32, 200, 0, 0, aug=1, seed=12), Prob(0, 20, 100, 0, 0, seed=13),
             Prob(90, 63, 333, 1, 0, aug=1, seed=14, ldc_pad=2), Prob(33, 65, 129, 1, 1, seed=15)]
    ks, _ = run_check(probs, 0, want_split, 64, "mixed")
    if want_split:
        assert ks == plan_tiled(probs, 32, 32, 128, 64)
    bprobs = [Prob(70, 50, 300, 0, 1, seed=11, bf16_route=True), Prob(40, 32, 200, 0, 0, aug=1, seed=12, bf16_route=True),
              Prob(0, 20, 100, 0, 0, seed=13, bf16_route=True), Prob(90, 63, 333, 1, 0, aug=1, seed=14, ldc_pad=2, bf16_route=True),
              Prob(33, 65, 129, 1, 1, seed=15, bf16_route=True)]
    ks, _ = run_check(bprobs, 1, want_split, 64, "mixed bf16")
    if want_split:
        assert ks == plan_bf16_128(bprobs, 64)
    xprobs = [Prob(2047, 299, 602, 0, 1, seed=16), Prob(2048, 300, 600, 0, 0, seed=17, ldc_pad=1), Prob(2050, 301, 610, 1, 0, aug=1, seed=18)]
    assert sum(p.M * p.N * p.K for p in xprobs) >= 1e9
    monkeypatch.setenv("HMP_GEMM_X3", "0")
    _, outs0 = run_check(xprobs, 0, want_split, 64, "mixed X3=0")
    monkeypatch.delenv("HMP_GEMM_X3")
    for tile in ("128",) if want_split else ("128", "64"):  # (a split-K launch takes the square tile under either setting)
        monkeypatch.setenv("HMP_GEMM_X3_TILE", tile)
        ks, outs = run_check(xprobs, 0, want_split, 64, f"mixed x3 tile {tile}")
        if want_split:
            assert ks == plan_x3(xprobs, 128, 128, 2, 64)
        for o, o0 in zip(outs, outs0):
            assert not torch.equal(o, o0), "the x3 kernel did not run"


# ---- the virtual ones column ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_real", [31, 32, 63, 64, 127, 128, 255, 256])
def test_ones_column_fp32_tiled_and_bf16_128(n_real, monkeypatch):
    """ones column at n_real = N - 1 across tile edges: fp32 tiled (TN split-K, NN plain) and the bf16 128 tile (folded ones product;
    at n_real % 128 == 0 the ones column lies past the last column tile)"""
    monkeypatch.setenv("HMP_GEMM_X3", "0")
    tn = Prob(40, n_real, 700, 1, 0, aug=1, seed=n_real, slabs=64)
    ks, _ = run_check([tn], 0, True, 64, f"fp32 TN ones {n_real}")
    assert ks == plan_tiled([tn], 32, 32, 128, 64)
    nn = Prob(40, n_real, 300, 0, 0, aug=1, seed=n_real + 1000, ldc_pad=1)
    run_check([nn], 0, False, 1, f"fp32 NN ones {n_real}")
    for want_split in (True, False):
        b = Prob(150, n_real, 700, 1, 0, aug=1, seed=n_real + 2000, slabs=64, bf16_route=True)
        ks, _ = run_check([b], 1, want_split, 64, f"bf16 ones {n_real}")
        if want_split:
            assert ks == plan_bf16_128([b], 64)


def test_ones_column_alone():
    """n_real = 0, N = 1: the bias column sums (GAT), every launcher"""
    for route in (0, 1, 2):
        for want_split in (True, False) if route < 2 else (True,):
            p = Prob(70, 0, 517, 1, 0, aug=1, seed=5, slabs=16, bf16_route=route == 1)
            run_check([p], route, want_split, 16, f"ones alone route {route}")


def test_ones_column_bf16_256_tile_and_bf16_b():
    """the 256 x 256 tile (split-K weight gradient over >= 2^17 nodes) with the folded ones product: an fp32 B with n_real = 255 and
    a bf16-stored B with n_real = 256 (the ones column past the last column tile); the 128 tile with a bf16 B at n_real = 256"""
    K = 1 << 17
    A = randn(K, 300, 21)
    big = [Prob(300, 255, K, 1, 0, aug=1, seed=22, A=A, slabs=192, bf16_route=True),
           Prob(300, 256, K, 1, 0, aug=1, seed=23, A=A, b16=True, slabs=192, bf16_route=True)]
    for p in big:
        ks, _ = run_check([p], 1, True, 192, "bf16 256")
        # 256 tile: ~512 workgroups over the launch's tiles x K (the 128 tile would stop at 64 slabs)
        t = cdiv(300, 256) * cdiv(p.n_real, 256)
        assert ks[0] == cdiv(K, cdiv(cdiv(K, min(int(512.0 * K / (t * K)), cdiv(K, 32), 192)), 32) * 32) and ks[0] > 64, ks
    small = Prob(150, 256, 3000, 1, 0, aug=1, seed=24, b16=True, slabs=64, bf16_route=True)
    ks, _ = run_check([small], 1, True, 64, "bf16 128 b16")
    assert ks == plan_bf16_128([small], 64)


# ---- the tall TN kernel -------------------------------------------------------------------------------------------------------
TALL_K = 40001  # the last K chunk is partial


@functools.lru_cache(maxsize=None)
def tall_operands():
    return randn(TALL_K, 192, 31), randn(TALL_K, 162, 32)


@pytest.mark.parametrize("M", [4, 48, 100, 192])
def test_tall_kernel_slices_and_ones_column(M, monkeypatch):
    """K >= 32768: the tall kernel against float64 and against HMP_GEMM_TALL=0 (the tiled split-K kernel).  n_real = 78: the ones
    column inside the first 80-column slice; 80 / 160: the ones column opens a new slice; 160 without ones: N ends on a slice edge"""
    monkeypatch.setenv("HMP_GEMM_X3", "0")
    A, B = tall_operands()
    for n_real, aug in ((78, 1), (80, 1), (160, 1), (160, 0), (2, 1)):
        p = Prob(M, n_real, TALL_K, 1, 0, aug=aug, A=A, B=B, slabs=TALL_SLABS)
        monkeypatch.delenv("HMP_GEMM_TALL", raising=False)
        ks, outs = run_check([p], 0, True, 64, f"tall M={M} n_real={n_real}", cap=[TALL_SLABS])
        assert ks == plan_tall([p]), ks
        monkeypatch.setenv("HMP_GEMM_TALL", "0")
        ks0, outs0 = run_check([p], 0, True, 64, f"tiled M={M} n_real={n_real}")
        assert not torch.equal(outs[0], outs0[0]), "the tall kernel did not run"


def peel_batch(order):
    """tall-eligible problems (T*) between ineligible ones: odd n_real, M = 196, K < 32768, an unaligned A, an empty problem"""
    A, B = tall_operands()
    mk = {
        "T1": lambda: Prob(192, 160, TALL_K, 1, 0, aug=1, A=A, B=B, slabs=TALL_SLABS),
        "T2": lambda: Prob(48, 78, 36000, 1, 0, aug=1, A=A, B=B, slabs=TALL_SLABS),
        "T3": lambda: Prob(100, 40, 33000, 1, 0, aug=0, A=A, B=B, slabs=TALL_SLABS),
        "odd": lambda: Prob(100, 61, 36000, 1, 0, aug=1, A=A, B=B, slabs=TALL_SLABS),
        "M196": lambda: Prob(196, 41, 33000, 1, 0, aug=1, seed=41, slabs=TALL_SLABS),
        "short": lambda: Prob(64, 64, 30000, 1, 0, aug=1, A=A, B=B, slabs=TALL_SLABS),
        "unal": lambda: Prob(48, 40, 34000, 1, 0, aug=1, seed=42, a_off=1, slabs=TALL_SLABS),
        "empty": lambda: Prob(0, 10, 35000, 1, 0, seed=43, slabs=TALL_SLABS),
    }
    return [mk[k]() for k in order], [k.startswith("T") for k in order]


@pytest.mark.parametrize("order", [
    ["T1", "odd", "T2", "M196", "empty", "T3", "short", "unal"],
    ["unal", "short", "T3", "empty", "M196", "T2", "odd", "T1"],
    ["odd", "M196", "empty", "short", "unal", "T1", "T2", "T3"],
])
def test_peeled_batch_tall_and_tiled(order, monkeypatch):
    """one split-K launch that the tall kernel and the tiled kernel share: ksplit_out of every problem must describe the slabs that
    problem got (gemm_launch_rest maps the rest's split back by index), at the executor's max_slabs of 64"""
    monkeypatch.delenv("HMP_GEMM_TALL", raising=False)
    monkeypatch.delenv("HMP_GEMM_X3", raising=False)
    probs, tall = peel_batch(order)
    caps = [TALL_SLABS if t else 64 for t in tall]
    ks, _ = run_check(probs, 0, True, 64, "peel", cap=caps)
    want_tall = plan_tall([p for p, t in zip(probs, tall) if t])
    want_rest = plan_tiled([p for p, t in zip(probs, tall) if not t], 32, 32, 128, 64)
    assert [k for k, t in zip(ks, tall) if t] == want_tall
    assert [k for k, t in zip(ks, tall) if not t] == want_rest


@pytest.mark.parametrize("order", [["DW1", "T1", "empty", "DW2", "T2"], ["T2", "DW2", "T1", "empty", "DW1"]])
def test_peeled_batch_bf16_dw_and_tiled(order, monkeypatch):
    """the bf16 launcher peels dw-eligible weight gradients (bf16 dZ, M % 256 == 0, n_real = 256, >= 65536 nodes) off to the
    output-stationary kernel and launches the rest tiled; HMP_GEMM_DW=0 sends all of them to the tiled kernel"""
    monkeypatch.delenv("HMP_GEMM_DW", raising=False)
    K = 65536
    A16 = randn(K + 4, 512, 51, torch.bfloat16)
    B = randn(K + 4, 256, 52)
    B16 = randn(K + 4, 256, 53, torch.bfloat16)
    mk = {
        "DW1": lambda: Prob(256, 256, K, 1, 0, aug=1, A=A16, B=B, a16=True, slabs=192, bf16_route=True),
        "DW2": lambda: Prob(512, 256, K + 3, 1, 0, aug=1, A=A16, B=B16, a16=True, b16=True, slabs=192, bf16_route=True),
        "T1": lambda: Prob(100, 99, 5000, 1, 0, aug=1, seed=54, slabs=192, bf16_route=True),
        "T2": lambda: Prob(200, 256, K, 1, 0, aug=1, A=A16, B=B, a16=True, slabs=192, bf16_route=True),  # M % 256 != 0
        "empty": lambda: Prob(0, 8, 100, 1, 0, seed=55, slabs=192, bf16_route=True),
    }
    probs = [mk[k]() for k in order]
    dw = [k.startswith("DW") for k in order]
    ks, outs = run_check(probs, 1, True, 192, "bf16 peel")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for k, p, d in zip(ks, probs, dw):
        if d:
            groups = max(8, 8 * (cus // (8 * (p.M // 256))))
            while groups > 8 and groups > 192:
                groups -= 8
            assert k == groups, (k, groups)
    assert [k for k, d in zip(ks, dw) if not d] == plan_bf16_128([p for p, d in zip(probs, dw) if not d], 192)
    monkeypatch.setenv("HMP_GEMM_DW", "0")
    ks0, outs0 = run_check(probs, 1, True, 192, "bf16 peel DW=0")
    for o, o0, d in zip(outs, outs0, dw):
        if d:
            assert not torch.equal(o, o0), "the dw kernel did not run"


# ---- the x3 kernel --------------------------------------------------------------------------------------------------------------
def test_x3_split_k_with_ones_column(monkeypatch):
    """split-K weight gradients over < 32768 nodes go to x3 with the folded ones column; HMP_GEMM_X3=2 also takes them above"""
    monkeypatch.delenv("HMP_GEMM_X3", raising=False)
    p = Prob(512, 255, 8200, 1, 0, aug=1, seed=61, slabs=64)
    ks, outs = run_check([p], 0, True, 64, "x3 split")
    monkeypatch.setenv("HMP_GEMM_X3", "0")
    _, outs0 = run_check([p], 0, True, 64, "x3 split X3=0")
    assert not torch.equal(outs[0], outs0[0]), "the x3 kernel did not run"
    A, B = tall_operands()
    q = Prob(192, 160, TALL_K, 1, 0, aug=1, A=A, B=B, slabs=TALL_SLABS)
    monkeypatch.setenv("HMP_GEMM_X3", "2")
    ks2, outs2 = run_check([q], 0, True, 64, "x3=2 tall shape")
    monkeypatch.setenv("HMP_GEMM_X3", "0")
    ks_tall, outs_tall = run_check([q], 0, True, 64, "tall", cap=[TALL_SLABS])
    assert not torch.equal(outs2[0], outs_tall[0]) and ks_tall == plan_tall([q]) and ks2 != ks_tall


# ---- EPI_ACTMASK and Cadd -------------------------------------------------------------------------------------------------------
# kernel -> (env, route, shape (M, N, K) of the NN input-gradient product)
EPI_KERNELS = {
    "32x32": ({"HMP_GEMM_X3": "0"}, 0, (300, 70, 500)),
    "64x64": ({"HMP_GEMM_X3": "0"}, 0, (2000, 200, 3000)),
    "128x128": ({"HMP_GEMM_X3": "0"}, 0, (4096, 1024, 256)),
    "x3_128": ({"HMP_GEMM_X3_TILE": "128"}, 0, (2048, 300, 2048)),
    "x3_64": ({"HMP_GEMM_X3_TILE": "64"}, 0, (2048, 300, 2048)),
    "bf16": ({}, 1, (300, 70, 500)),
    "bf16_h16": ({}, 1, (300, 70, 500)),
}


@pytest.mark.parametrize("kernel", list(EPI_KERNELS))
def test_actmask_epilogue_and_cadd(kernel, monkeypatch):
    """act' of none / relu / elu read off the stored H, with and without dropout (-0.0 = dropped, kept ones scaled by 1 / (1 - p)),
    on top of the Cadd addend"""
    for k in ("HMP_GEMM_X3", "HMP_GEMM_X3_TILE", "HMP_GEMM_BIG"):
        monkeypatch.delenv(k, raising=False)
    env, route, (M, N, K) = EPI_KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    results = {}
    for act in (ACT_NONE, ACT_RELU, ACT_ELU):
        for drop_p in (0.0, 0.3):
            p = Prob(M, N, K, 0, 0, seed=M + act, epi=True, act=act, drop_p=drop_p, h16=kernel == "bf16_h16", cadd=True, ldc_pad=1,
                     bf16_route=route == 1)
            _, outs = run_check([p], route, False, 1, f"{kernel} act={act} p={drop_p}")
            results[(act, drop_p)] = outs[0]
    if kernel.startswith("x3"):  # the kernel really ran: the fp32-MFMA kernel's result differs bitwise
        p = Prob(M, N, K, 0, 0, seed=M + ACT_ELU, epi=True, act=ACT_ELU, drop_p=0.3, cadd=True, ldc_pad=1)
        monkeypatch.setenv("HMP_GEMM_X3", "0")
        _, outs0 = run_check([p], 0, False, 1, f"{kernel} other")
        assert not torch.equal(outs0[0], results[(ACT_ELU, 0.3)])
    if kernel == "128x128":  # the same epilogue in a split-K launch (the mask is linear, Cadd rides in slab 0): the 128x128 plan's split,
        # and the 64x64 one under HMP_GEMM_BIG=0 (both forms run the same k-ordered fp32 chain: the values cannot tell them apart)
        p = Prob(M, N, K, 0, 0, seed=M + ACT_ELU, epi=True, act=ACT_ELU, drop_p=0.3, cadd=True, ldc_pad=1)
        ks, _ = run_check([p], 0, True, 64, "128x128 epilogue split")
        monkeypatch.setenv("HMP_GEMM_BIG", "0")
        ks0, _ = run_check([p], 0, True, 64, "64x64 epilogue split")
        assert ks == plan_tiled([p], 128, 128, 32, 64) and ks0 == plan_tiled([p], 64, 64, 32, 64) and ks != ks0


@pytest.mark.parametrize("cls", ["32x32_bk128", "64x64", "128x128", "bf16_128", "x3_128"])
def test_cadd_with_split_k(cls, monkeypatch):
    """Cadd is added once: by the first K group of the block (32x32: four waves split the stage) and the first slab only.  Every
    tiled kernel whose launcher splits an NN problem: the three fp32 classes, the bf16 128 x 128 tile and the square x3 tile.  (The
    bf16 256 x 256 tile splits TN problems only and the narrow x3 tile is chosen for plain launches only: neither ever splits an
    NN problem.)"""
    for k in ("HMP_GEMM_X3_TILE", "HMP_GEMM_BIG"):
        monkeypatch.delenv(k, raising=False)
    route = 1 if cls == "bf16_128" else 0
    if cls == "x3_128":
        monkeypatch.delenv("HMP_GEMM_X3", raising=False)
    else:
        monkeypatch.setenv("HMP_GEMM_X3", "0")
    (M, N, K), _, plan = CLASSES["128x128" if cls in ("bf16_128", "x3_128") else cls]
    for want_split in (True, False):
        p = Prob(M, N, K, 0, 0, seed=71, cadd=True, slabs=64, bf16_route=route == 1)
        ks, outs = run_check([p], route, want_split, 64, f"cadd {cls}")
        if want_split:
            want = plan_bf16_128([p], 64) if cls == "bf16_128" else plan_x3([p], 128, 128, 2, 64) if cls == "x3_128" else plan_tiled([p], *plan, 64)
            assert ks == want and ks[0] > 1
        if cls == "x3_128":  # the kernel really ran: the fp32-MFMA kernel's result differs bitwise
            monkeypatch.setenv("HMP_GEMM_X3", "0")
            _, outs0 = run_check([p], 0, want_split, 64, "cadd x3 other")
            monkeypatch.delenv("HMP_GEMM_X3")
            assert not torch.equal(outs[0], outs0[0])


# ---- the register-direct TN kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 191, 192, 193, 383, 384, 385])
def test_direct_tn_chunks(K):
    """node chunks of 192 / 384 and the odd-K tail, with the ones column; compared with float64 and the planned split"""
    p = Prob(40, 33, K, 1, 0, aug=1, seed=K, slabs=16)
    ks, _ = run_check([p], 2, True, 16, f"direct K={K}")
    assert ks == [plan_direct(p, 16)]


def test_direct_tn_slab_limit_and_four_trips():
    """exactly max_slabs slabs; one node more declines (ksplit_out all 0, nothing written); >= 512 output tiles take 4 trips"""
    p = Prob(40, 33, 1536, 1, 0, aug=1, seed=81, slabs=4)
    ks, _ = run_check([p], 2, True, 4, "direct at max_slabs")
    assert ks == [4]
    q = Prob(40, 33, 1537, 1, 0, aug=1, seed=82, slabs=4)
    ks = launch([p, q], 2, True, 4)
    assert ks == [0, 0]
    assert torch.isnan(p.C_all).all() and torch.isnan(q.C_all).all()
    wide = Prob(512, 1023, 1000, 1, 0, aug=1, seed=83, slabs=16)
    ks, _ = run_check([wide], 2, True, 16, "direct 4 trips")
    assert ks == [2] and plan_direct(wide, 16) == 2  # 2 trips would need cdiv(1000, 384) = 3 slabs


def test_direct_tn_batch_with_empty_problem():
    probs = [Prob(64, 50, 500, 1, 0, aug=1, seed=91, slabs=16), Prob(0, 20, 300, 1, 0, aug=1, seed=92, slabs=16),
             Prob(33, 0, 100, 1, 0, aug=1, seed=93, slabs=16), Prob(96, 95, 700, 1, 0, aug=1, seed=94, slabs=16, ldc_pad=3)]
    ks, _ = run_check(probs, 2, True, 16, "direct batch")
    assert ks == [plan_direct(p, 16) for p in probs]


def test_entry_validates_arguments():
    lib = _lib.require_device()
    p = Prob(8, 8, 8, 0, 0, seed=1)
    d = p.desc()
    bad = []
    for field, value in (("A", None), ("ldc", 4), ("n_real", 7), ("lda", 4), ("drop_p", 1.0)):
        e = p.desc()
        setattr(e, field, value)
        bad.append(e)
    ks = (C.c_int32 * 9)()
    for e in bad:
        assert lib.hmp_gemm_grouped((_lib.GemmDesc * 1)(e), 1, 0, 0, 1, ks, _lib.stream_ptr()) != 0
    assert lib.hmp_gemm_grouped((_lib.GemmDesc * 9)(*([d] * 9)), 9, 0, 0, 1, ks, _lib.stream_ptr()) != 0
    assert lib.hmp_gemm_grouped((_lib.GemmDesc * 1)(d), 1, 2, 1, 1, ks, _lib.stream_ptr()) != 0  # direct: TN only
    assert torch.isnan(p.C_all).all()
