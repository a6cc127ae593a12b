"""The front launch's layer-0 projection and pack role (csrc/front.hip) and the stand-alone pack (pack_launch) on their own,
through ``hmp_front_run`` / ``hmp_pack_run``: the descriptors are copied into the structures the executor fills and the block maps
are the executor's (pack_seg_blocks / pack_block_map).

Reference and case tables: tests/_front_reference.py (float64 numpy; tests/test_front_reference.py checks it on the CPU and proves
from front.hip's constants which load width, stages, K-group forms and source-count instantiation every case reaches).  Every
output starts as NaN and every operand lies between NaN guards, A's padding columns included.

Projection: |got - ref64| <= TOL * (|A| @ sum_q |W_q|.T) element by element, TOL the bar of tests/test_gpu_gemm_launch.py for the
project's fp32 MFMA GEMMs; columns without a segment are +0.0; [N, ldc), the rows past M and the guards stay NaN.
Pack: PACK_SUM / PACK_HEADS bit-equal to the float32 left-to-right sum / the copy, the transposed image bit-equal to the packed
element at its rule position, padding +0.0, the attention dots within gamma_C * sum_c |a_c w_c| (gamma_C = C u / (1 - C u), u = 2^-24:
a C-term float32 dot product in any order, fused or not); every owned element written, every other one still NaN.

``pytest -s`` prints the largest error ratio of every projection case."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _front_reference as R  # noqa: E402
from hydra_gnn_amd import _lib  # noqa: E402
from test_gpu_gemm_launch import TOL  # noqa: E402

DEV = "cuda:0"
G = R.GUARD
NAN = float("nan")


def to_dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# projection
# ---------------------------------------------------------------------------------------------------------------------------
class Launch:
    """operands of one launch on the device; run() fills fresh NaN outputs"""

    def __init__(self, cases, seed, slack=0):
        self.params_np, self.lays = R.lay_out_proj(cases, seed)
        if slack:  # room behind the blocks for descriptors that a refusal test bends
            self.params_np = np.concatenate([self.params_np, np.full(slack, np.nan, np.float32)])
        self.params = to_dev(self.params_np)
        self.a = [to_dev(np.concatenate([l.a_buf, np.full(slack, np.nan, np.float32)])) for l in self.lays]
        self.c = None

    def descs(self, which=None):
        which = range(len(self.lays)) if which is None else which
        arr = (_lib.FrontProb * max(len(which), 1))()
        for d, i in zip(arr, which):
            lay, p = self.lays[i], self.lays[i].case
            d.A = self.a[i].data_ptr() + 4 * lay.a0
            d.C = self.c[i].data_ptr() + 4 * G
            d.lda, d.ldc, d.M, d.N, d.K, d.n_seg = p.ld_a, p.ldc, p.M, p.n, p.K, len(p.segs)
            for s, (col0, rows, nsrc), offs in zip(d.seg, p.segs, lay.offs):
                s.col0, s.rows, s.nsrc, s.ld = col0, rows, nsrc, p.K
                for q, off in enumerate(offs):
                    s.off[q] = off
        return arr

    def fresh(self):
        self.c = [torch.full((2 * G + l.c_rows * l.case.ldc,), NAN, device=DEV) for l in self.lays]

    def call(self, arr, n, pack=None):
        lib = _lib.require_device()
        segs, n_segs, packed, n_packed, step, mirror = pack if pack else (None, 0, None, 0, None, None)
        rc = lib.hmp_front_run(arr, n, self.params.data_ptr(), self.params.numel(), segs, n_segs, packed, n_packed, step, mirror,
                               _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, which=None, pack=None):
        self.fresh()
        arr = self.descs(which)
        _lib.check(self.call(arr, len(self.lays) if which is None else len(which), pack))
        return [c.clone() for c in self.c]


@functools.lru_cache(maxsize=None)
def proj_ref(launch_key, i):
    L = LAUNCHES[launch_key]
    return R.proj_reference(L.lays[i], L.params_np)


LAUNCHES = {}


def launch_of(key, cases, seed, **kw):
    if key not in LAUNCHES:
        LAUNCHES[key] = Launch(cases, seed, **kw)
    return LAUNCHES[key]


def check_projection(key, i, cbuf):
    """one problem's C allocation against the reference; returns the largest |error| / bound operand"""
    L = LAUNCHES[key]
    lay, p = L.lays[i], L.lays[i].case
    buf = cbuf.cpu().numpy()
    assert np.isnan(buf[:G]).all() and np.isnan(buf[-G:]).all(), f"{p.name}: a guard around C was written"
    Cm = buf[G:-G].reshape(lay.c_rows, p.ldc)
    assert np.isnan(Cm[p.M:]).all(), f"{p.name}: rows past M were written"
    assert np.isnan(Cm[:, p.n:]).all(), f"{p.name}: columns [N, ldc) were written"
    got = Cm[:p.M, :p.n]
    assert not np.isnan(got).any(), f"{p.name}: {int(np.isnan(got).sum())} of {got.size} elements are NaN (unwritten, or an unmasked read)"
    ref, bound, live = proj_ref(key, i)
    assert (got[:, ~live].view(np.int32) == 0).all(), f"{p.name}: a column without a segment is not +0.0"
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err[:, live] / bound[:, live]).max()) if live.any() else 0.0
    print(f"projection {p.name}: K {p.K} M {p.M} N {p.n} max |err| / (|A| @ sum|W|.T) = {ratio:.3e}")
    bad = err > TOL * bound
    assert not bad.any(), f"{p.name}: {int(bad.sum())} elements over the bar, worst ratio {ratio:.3e} (bar {TOL:g}), first at {np.argwhere(bad)[0]}"
    return ratio


CASES = R.proj_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_projection(case):
    key = "one:" + case.name
    L = launch_of(key, [case], 11 + CASES.index(case))
    (c,) = L.run()
    check_projection(key, 0, c)


def test_four_problems_in_one_launch_equal_each_launched_alone():
    L = launch_of("multi", R.multi_cases(), 7)
    together = L.run()
    for i, c in enumerate(together):
        check_projection("multi", i, c)
    for i in range(len(L.lays)):
        alone = L.run(which=[i])  # (the output buffers of the others stay NaN)
        assert torch.equal(bits(alone[i]), bits(together[i])), f"problem {i} differs from the same problem launched alone"
        for j, c in enumerate(alone):
            assert j == i or torch.isnan(c).all()


@pytest.mark.parametrize("name", ["straddle", "k384", "nsrc1+5"])
def test_two_launches_give_the_same_bits(name):
    case = next(c for c in CASES if c.name == name)
    L = launch_of("one:" + name, [case], 11 + CASES.index(case))
    (a,) = L.run()
    (b,) = L.run()
    assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------------------------------------------------------
TABLES = R.pack_tables()


@functools.lru_cache(maxsize=None)
def pack_layout(table):
    lay = R.lay_out_pack(TABLES[table], 23 + sorted(TABLES).index(table))
    refs, alone = R.pack_reference(lay)
    return lay, refs, alone, to_dev(lay.params)


def pack_descs(lay):
    arr = (_lib.PackSeg * len(lay.segs))()
    for a, s, d in zip(arr, lay.segs, lay.desc):
        a.dst, a.rows, a.rows_pad, a.cols, a.ld_dst, a.ld_src, a.nsrc = d["dst"], s.rows, s.rows_pad, s.cols, s.ld_dst, s.ld_src, s.nsrc
        a.kind, a.H, a.C, a.Cp, a.att = s.kind, s.H, s.C, s.Cp, d["att"]
        for q, off in enumerate(d["src"]):
            a.src[q] = off
        a.dst_t, a.ld_dst_t, a.col_t, a.pad_t = d["dst_t"], s.ld_dst_t, s.col_t, s.pad_t
    return arr


def run_pack(table, route, step0=41):
    lib = _lib.require_device()
    lay, refs, alone, params = pack_layout(table)
    packed = torch.full((lay.n_packed,), NAN, device=DEV)
    step = torch.tensor([step0], dtype=torch.int32, device=DEV)
    mirror = torch.tensor([-1], dtype=torch.int32, device=DEV)
    _lib.check(lib.hmp_pack_run(pack_descs(lay), len(lay.segs), route, params.data_ptr(), params.numel(), packed.data_ptr(), packed.numel(),
                                step.data_ptr(), mirror.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return packed, int(step.item()), int(mirror.item())


def check_pack(table, packed):
    lay, refs, alone, _ = pack_layout(table)
    got_all = packed.cpu().numpy()
    assert np.isnan(got_all[alone]).all(), f"{int((~np.isnan(got_all[alone])).sum())} elements outside the segments were written"
    for i, (s, r) in enumerate(zip(lay.segs, refs)):
        what = f"{table}[{i}] kind {s.kind} rows {s.rows}/{s.rows_pad} cols {s.cols}/{s.ld_dst} nsrc {s.nsrc} H {s.H} C {s.C}"
        got = got_all[r["own"]]
        assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} owned elements are NaN (unwritten, or an unmasked read)"
        if r["exact"] is not None:
            same = got.view(np.int32) == r["exact"].view(np.int32)
            assert same.all(), f"{what}: {int((~same).sum())} elements differ from the float32 left-to-right sum / copy, first at {np.argwhere(~same)[0]}"
        else:
            err = np.abs(got.astype(np.float64) - r["val"])
            assert (err <= r["bound"]).all(), f"{what}: worst |err| / bound {np.nanmax(err / np.where(r['bound'] > 0, r['bound'], np.nan)):.3f}"
            assert (got.view(np.int32)[r["bound"] == 0] == 0).all(), f"{what}: padding is not +0.0"
        if r["img"] is not None:
            assert (got_all[r["img"]].view(np.int32) == got.view(np.int32)).all(), f"{what}: the image differs from the packed element"
            assert (got_all[r["img_zero"]].view(np.int32) == 0).all(), f"{what}: the image's padding is not +0.0"


@pytest.mark.parametrize("route", [0, 1], ids=["pack_launch", "front_role"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_pack(table, route):
    packed, step, mirror = run_pack(table, route)
    check_pack(table, packed)
    assert (step, mirror) == (42, 42), "the launch raises the step counter by one and mirrors it"
    again, step, mirror = run_pack(table, route, step0=step)
    assert (step, mirror) == (43, 43)
    assert torch.equal(bits(again), bits(packed))


@pytest.mark.parametrize("table", sorted(TABLES))
def test_both_pack_routes_give_the_same_bits(table):
    a, _, _ = run_pack(table, 0)
    b, _, _ = run_pack(table, 1)
    assert torch.equal(bits(a), bits(b))


def test_projection_and_pack_in_one_launch_equal_the_two_alone():
    L = launch_of("multi", R.multi_cases(), 7)
    alone_c = L.run()
    lay, refs, alone, params = pack_layout("sum")
    # the pack's blocks behind the projection's in one parameter buffer
    base = (L.params_np.size + 3) // 4 * 4
    both = to_dev(np.concatenate([L.params_np, np.full(base - L.params_np.size, np.nan, np.float32), lay.params]))
    arr = pack_descs(lay)
    for a in arr:
        a.att += base
        for q in range(6):
            a.src[q] += base
    packed = torch.full((lay.n_packed,), NAN, device=DEV)
    step = torch.tensor([7], dtype=torch.int32, device=DEV)
    mirror = torch.tensor([-1], dtype=torch.int32, device=DEV)
    keep = L.params
    L.params = both
    try:
        together = L.run(pack=(arr, len(lay.segs), packed.data_ptr(), packed.numel(), step.data_ptr(), mirror.data_ptr()))
    finally:
        L.params = keep
    for i, (a, b) in enumerate(zip(alone_c, together)):
        assert torch.equal(bits(a), bits(b)), f"projection {i} changes when the pack role rides along"
    check_pack("sum", packed)
    alone_p, _, _ = run_pack("sum", 1)
    assert torch.equal(bits(alone_p), bits(packed))
    assert (int(step.item()), int(mirror.item())) == (8, 8)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: host-side argument checks, nothing is launched
# ---------------------------------------------------------------------------------------------------------------------------
BASE = R.Proj("base", 6, 5, ((0, 4, 1), (4, 4, 2)))


def _set_k(d, k, lda=None):
    d.K, d.lda = k, k if lda is None else lda
    for s in d.seg:
        s.ld = k


def _swap(d):
    a = _lib.FrontSeg.from_buffer_copy(d.seg[0])
    d.seg[0] = d.seg[1]
    d.seg[1] = a


REFUSALS = {
    "k2": lambda d: _set_k(d, 2),
    "k386": lambda d: _set_k(d, 386),
    "k-odd": lambda d: _set_k(d, 5, 6),
    "lda-odd": lambda d: setattr(d, "lda", 7),
    "a-4-bytes": lambda d: setattr(d, "A", d.A + 4),
    "segments-0": lambda d: setattr(d, "n_seg", 0),
    "segments-7": lambda d: setattr(d, "n_seg", 7),
    "nsrc-0": lambda d: setattr(d.seg[0], "nsrc", 0),
    "nsrc-7": lambda d: setattr(d.seg[1], "nsrc", 7),
    "offset-odd": lambda d: d.seg[1].off.__setitem__(1, d.seg[1].off[1] + 1),
    "unsorted": _swap,
    "overlap": lambda d: setattr(d.seg[1], "col0", 3),
    "ld-not-k": lambda d: setattr(d.seg[0], "ld", 8),
    "ldc-short": lambda d: setattr(d, "ldc", d.N - 1),
}


@pytest.mark.parametrize("what", list(REFUSALS) + ["problems-5"])
def test_refused_arguments(what):
    L = launch_of("base", [BASE], 3, slack=4096)
    L.fresh()
    if what == "problems-5":
        one = L.descs()[0]
        arr = (_lib.FrontProb * 5)(*([one] * 5))
        rc = L.call(arr, 5)
    else:
        arr = L.descs()
        REFUSALS[what](arr[0])
        rc = L.call(arr, 1)
    assert rc == 1, "HMP_E_ARG"
    with pytest.raises(_lib.HydraMPError):
        _lib.check(rc)
    assert torch.isnan(L.c[0]).all(), "a refused call wrote"
    (c,) = L.run()
    check_projection("base", 0, c)


def test_refused_pack_arguments():
    lib = _lib.require_device()
    lay, refs, alone, params = pack_layout("heads")
    packed = torch.full((lay.n_packed,), NAN, device=DEV)

    def call(arr, n_params=params.numel(), n_packed=packed.numel(), route=0):
        return lib.hmp_pack_run(arr, len(lay.segs), route, params.data_ptr(), n_params, packed.data_ptr(), n_packed, None, None, _lib.stream_ptr())

    for route in (0, 1):
        assert call(pack_descs(lay), n_params=params.numel() - G - 6, route=route) == 1  # one float short of the last block's end
        assert call(pack_descs(lay), n_packed=packed.numel() - G - 1, route=route) == 1
        arr = pack_descs(lay)
        arr[0].kind = 4
        assert call(arr, route=route) == 1
        arr = pack_descs(lay)
        arr[1].rows_pad = arr[1].rows - 1
        assert call(arr, route=route) == 1
    assert call(pack_descs(lay), route=2) == 1
    torch.cuda.synchronize()
    assert torch.isnan(packed).all()
