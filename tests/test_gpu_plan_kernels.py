"""The graph-plan builder (csrc/plan.hip, csrc/plan_small.h) on every path, as the executor calls it: several edge types per
call, with and without t_pos, degf, uncleared scratch and graph offsets, through ``hmp_plan_build_many``.

Reference: tests/_plan_reference.py (numpy stable sorts; shares no code with the builder).  Outputs start as a sentinel and every
comparison is exact: ``rowptr`` / ``t_rowptr`` whole, ``eid`` / ``col`` / ``t_col`` / ``t_pos`` up to the kept count, ``degf`` bit
for bit (the library is built without fast-math: 1 / max(deg, 1) is one correctly rounded float32 division on both sides), and
the status word.  HMP_PLAN_SMALL=0 / 1 pins the multi-launch / single-launch build.  tests/test_plan_reference.py shows (without
a GPU) that every edge list below sits in the regime it is named after.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _plan_reference as R  # noqa: E402
from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402

DEV = "cuda:0"
SENT = -7
ARRAYS = ("rowptr", "col", "eid", "t_rowptr", "t_col", "t_pos")


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


class Buffers:
    """outputs + scratch of one job, sized for (E, n_src, n_dst); reusable for smaller edge lists of the same node counts"""

    def __init__(self, E, n_src, n_dst, zero_scratch=False):
        lib = _lib.require_device()
        i32 = dict(dtype=torch.int32, device=DEV)
        self.t = {"rowptr": torch.full((n_dst + 1,), SENT, **i32), "t_rowptr": torch.full((n_src + 1,), SENT, **i32)}
        for k in ("col", "eid", "t_col", "t_pos"):
            self.t[k] = torch.full((max(E, 1),), SENT, **i32)
        self.t["degf"] = torch.full((max(n_dst, 1),), float(SENT), dtype=torch.float32, device=DEV)
        nbytes = max(int(lib.hmp_plan_scratch_bytes(E, n_src, n_dst)), 16)
        # clear_first = 1 must cope with any content; clear_first = 0 is promised zeroed counters
        self.scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV) if zero_scratch else torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)

    def reset(self):
        for k, v in self.t.items():
            v.fill_(SENT)


def run_call(jobs, small, need_tpos=1, clear_first=1, offsets=True, bufs=None, monkeypatch=None):
    """one hmp_plan_build_many call; returns ([per-job {array: tensor}], status)"""
    lib = _lib.require_device()
    monkeypatch.setenv("HMP_PLAN_SMALL", str(small))
    bufs = bufs or [Buffers(j.E, j.n_src, j.n_dst) for j in jobs]
    keep = []
    arr = (_lib.PlanJob * max(len(jobs), 1))()
    for a, j, b in zip(arr, jobs, bufs):
        ei = _dev(j.ei, torch.int64)
        keep.append(ei)
        a.d_edge_index = ei.data_ptr() if j.E > 0 else None
        a.plan = _lib.Plan(j.n_src, j.n_dst, j.E, *(b.t[k].data_ptr() for k in ARRAYS))
        a.d_degf = b.t["degf"].data_ptr()
        if offsets and j.edge_ptr is not None:
            ptrs = [_dev(p, torch.int64) for p in (j.dst_ptr, j.src_ptr, j.edge_ptr)]
            keep += ptrs
            a.d_dst_ptr, a.d_src_ptr, a.d_edge_ptr = (p.data_ptr() for p in ptrs)
            a.n_graphs = j.edge_ptr.size - 1
        a.d_scratch = b.scratch.data_ptr()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib.hmp_plan_build_many(arr, len(jobs), need_tpos, clear_first, status.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    monkeypatch.delenv("HMP_PLAN_SMALL")
    return [b.t for b in bufs], int(status.item())


def first_diff(got, want):
    n = min(got.numel(), want.numel())
    d = torch.nonzero(got[:n] != want[:n]).flatten()
    return int(d[0]) if d.numel() else None


def same(got, want, what):
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} against {tuple(want.shape)}"
    if not torch.equal(got, want):
        i = first_diff(got, want)
        raise AssertionError(f"{what}: first difference at {i}: {got[i].item()} against {want[i].item()} ({int((got != want).sum())} of {got.numel()} differ)")


def check_job(j, t, need_tpos=1, what=""):
    """the arrays of one job against the host reference (computed here, once per job and call)"""
    r = R.reference(j)
    k = r["kept"]
    what = f"{what}{j.name}"
    same(t["rowptr"].cpu().long(), torch.from_numpy(r["rowptr"]), f"{what}: rowptr")
    same(t["t_rowptr"].cpu().long(), torch.from_numpy(r["t_rowptr"]), f"{what}: t_rowptr")
    for name in ("eid", "col", "t_col"):
        same(t[name].cpu().long()[:k], torch.from_numpy(r[name]), f"{what}: {name}")
    if need_tpos:
        same(t["t_pos"].cpu().long()[:k], torch.from_numpy(r["t_pos"]), f"{what}: t_pos")
    else:
        assert bool((t["t_pos"] == SENT).all()), f"{what}: t_pos written without need_tpos"
    same(t["degf"][:j.n_dst].cpu().view(torch.int32), torch.from_numpy(r["degf"]).view(torch.int32), f"{what}: degf (bits)")
    return r


def check_call(jobs, got, status, need_tpos=1, what=""):
    for i, (j, t) in enumerate(zip(jobs, got)):
        check_job(j, t, need_tpos, f"{what}job {i} ")
    assert status == R.call_status(jobs), f"{what}status {status}"


def agree(jobs, a, b, need_tpos=1):
    """two builds of the same call: every specified entry equal"""
    for j, x, y in zip(jobs, a, b):
        k = int(R.valid_mask(j).sum())
        for name in ("rowptr", "t_rowptr"):
            same(x[name], y[name], f"{j.name}: {name}")
        for name in ("eid", "col", "t_col") + (("t_pos",) if need_tpos else ()):
            same(x[name][:k], y[name][:k], f"{j.name}: {name}")
        same(x["degf"][:j.n_dst].view(torch.int32), y["degf"][:j.n_dst].view(torch.int32), f"{j.name}: degf (bits)")


# ---- multi-launch build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need_tpos", [1, 0])
@pytest.mark.parametrize("variant", range(len(R.SIX_VARIANTS)))
def test_six_jobs_in_one_call(variant, need_tpos, monkeypatch):
    """job boundaries inside and on wavefront edges, an empty job, a run of equal endpoints across every boundary, and the five
    orders: in-place (ordered) and ranked directions side by side in one launch"""
    jobs = R.six_jobs(variant)
    got, status = run_call(jobs, 0, need_tpos=need_tpos, monkeypatch=monkeypatch)
    check_call(jobs, got, status, need_tpos)
    assert status == 1  # the job with the out-of-range endpoint


@pytest.mark.parametrize("group_by", ["dst", "src"])
def test_runs_and_holes_at_chosen_lanes(group_by, monkeypatch):
    j = R.runs_and_holes(group_by)
    got, status = run_call([j], 0, monkeypatch=monkeypatch)
    check_call([j], got, status)
    assert status == 1


def test_rank_classes_in_neighbouring_row_groups(monkeypatch):
    jobs = R.rank_classes()
    got, status = run_call(jobs, 0, monkeypatch=monkeypatch)
    check_call(jobs, got, status)


@pytest.mark.parametrize("case", ["edges", "tops", "segments"])
def test_second_trips_of_the_grid_stride_loops(case, monkeypatch):
    jobs = {"edges": R.second_trip_edges, "tops": R.second_trip_tops, "segments": R.segment_edges}[case]()
    got, status = run_call(jobs, 0, monkeypatch=monkeypatch)
    check_call(jobs, got, status)


@pytest.mark.parametrize("modes", R.SCRATCH_MODES, ids=lambda m: "".join(map(str, m)))
def test_one_scratch_zeroed_once(modes, monkeypatch):
    """clear_first = 0: the counters are zero on entry because the last build left them zero, whichever build that was"""
    seq = R.scratch_sequence()
    b = Buffers(R.SCRATCH_CAP, R.SCRATCH_N_SRC, R.SCRATCH_N_DST, zero_scratch=True)
    n_cnt = R.counter_ints(R.SCRATCH_N_SRC, R.SCRATCH_N_DST)
    for step, (j, mode) in enumerate(zip(seq, modes)):
        b.reset()
        got, status = run_call([j], mode, clear_first=0, bufs=[b], monkeypatch=monkeypatch)
        check_call([j], got, status, what=f"build {step + 1} (HMP_PLAN_SMALL={mode}) ")
        counters = b.scratch.view(torch.int32)[:n_cnt]
        assert int(torch.count_nonzero(counters)) == 0, f"build {step + 1} (HMP_PLAN_SMALL={mode}) left counters behind"


# ---- single-launch build, and its agreement with the multi-launch build -----------------------------------------------------
@pytest.mark.parametrize("need_tpos", [1, 0])
@pytest.mark.parametrize("case", sorted(R.small_cases()))
def test_single_launch_build(case, need_tpos, monkeypatch):
    jobs = R.small_cases()[case]
    got, status = run_call(jobs, 1, need_tpos=need_tpos, monkeypatch=monkeypatch)
    check_call(jobs, got, status, need_tpos)
    multi, status0 = run_call(jobs, 0, need_tpos=need_tpos, monkeypatch=monkeypatch)
    assert status0 == status == 0
    agree(jobs, got, multi, need_tpos)


# ---- graph-sorted edge lists --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need_tpos", [1, 0])
@pytest.mark.parametrize("case", sorted(R.vouched_cases()))
def test_vouched_lists(case, need_tpos, monkeypatch):
    jobs = R.vouched_cases()[case]
    got, status = run_call(jobs, 1, need_tpos=need_tpos, monkeypatch=monkeypatch)
    assert status == 0
    check_call(jobs, got, status, need_tpos)
    plain, status = run_call(jobs, 1, need_tpos=need_tpos, offsets=False, monkeypatch=monkeypatch)
    assert status == 0
    agree(jobs, got, plain, need_tpos)
    multi, status = run_call(jobs, 0, need_tpos=need_tpos, monkeypatch=monkeypatch)  # offsets given and ignored
    assert status == 0
    agree(jobs, got, multi, need_tpos)


@pytest.mark.parametrize("case", sorted(R.wrongly_vouched()))
def test_wrong_vouching_is_flagged(case, monkeypatch):
    j = R.wrongly_vouched()[case]
    _, status = run_call([j], 1, monkeypatch=monkeypatch)
    assert status & R.STATUS_NOT_GRAPH_SORTED
    _, status = run_call([j.without_offsets()], 1, monkeypatch=monkeypatch)
    assert status == 0


@pytest.mark.parametrize("case", ["first", "middle", "last", "all"])
def test_vouched_list_with_an_out_of_range_endpoint_drops_it_cleanly(case, monkeypatch):
    """Valid offsets, one endpoint out of range: status bit 0 and the plan of the kept edges, as without the offsets.  A part
    starts its rows at its slice's first edge id, which counts the edges dropped in front of it; the build used to stop there.
    Measured on an MI355X before the last-arriving part rebuilt such a direction, three 200-row graphs, E = 1650: bad edge in
    graph 0: rowptr differs from index 200 on (401 of 601 entries one too large), rowptr[600] = 1650 against 1649 kept; in
    graph 1: from index 400 on (201 entries), rowptr[600] = 1650; in graph 2: nothing differs; one in each: from index 200 on,
    rowptr[600] = 1649 against 1647 kept.  Only builds and reads a plan."""
    j = R.vouched_out_of_range()[case]
    (got,), status = run_call([j], 1, monkeypatch=monkeypatch)
    r = R.reference(j)
    rp = got["rowptr"].cpu().long()
    print(f"{case}: E {j.E}, kept {r['kept']}, rowptr[n] {int(rp[-1])}, first differing rowptr index "
          f"{first_diff(rp, torch.from_numpy(r['rowptr']))}, entries that differ {int((rp != torch.from_numpy(r['rowptr'])).sum())}")
    assert status == R.STATUS_DROPPED
    check_job(j, got)
    (plain,), status = run_call([j.without_offsets()], 1, monkeypatch=monkeypatch)
    assert status == R.STATUS_DROPPED
    agree([j], [got], [plain])


# ---- through a net: the front-kernel role and the stand-alone link pass ---------------------------------------------------
class _DeviceArray:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (int(ptr), False), "version": 2}


def _read(ptr, n):
    if n == 0:
        return torch.zeros(0, dtype=torch.int64)
    return torch.as_tensor(_DeviceArray(ptr, n), device=DEV).cpu().long()


SAGE = dict(conv_block="GraphSAGE", hidden_dim=64, num_layers=3)
GAT = dict(conv_block="GAT", GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False])


@pytest.mark.parametrize("sliced", ["0", "1"])
@pytest.mark.parametrize("kind", ["sage", "gat"])
def test_plans_of_a_net_on_one_workspace(kind, sliced, monkeypatch):
    """forwards on 9, then 1, then 32 graphs through one net: every edge type's plan, read back with hmp_net_plan, is the
    reference's (t_pos only where the net builds it: GAT)"""
    monkeypatch.setenv("HMP_FUSE", "1")
    monkeypatch.setenv("HMP_PLAN_SLICED", sliced)
    torch.manual_seed(0)
    net = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, dropout=0.0, **(SAGE if kind == "sage" else GAT)).to(DEV).eval()
    lib = _lib.require_device()
    for n_graphs in (9, 1, 32):
        batch = workloads.config2_batch(n_graphs)
        net(batch.to(DEV))
        torch.cuda.synchronize()
        nat = net.native()
        assert nat.read_state()[1] == 0
        for e, et in enumerate(nat.edge_types):
            plan = _lib.Plan()
            _lib.check(lib.hmp_net_plan(nat._handle, e, C.byref(plan)))
            ei = batch[et].edge_index.numpy()
            j = R.job(ei[0], ei[1], batch[et[0]].x.size(0), batch[et[2]].x.size(0), name=f"{n_graphs} graphs {et[1]}")
            assert (plan.n_src, plan.n_dst, plan.n_edges) == (j.n_src, j.n_dst, j.E)
            r = R.reference(j)
            assert r["kept"] == j.E
            what = f"{kind}, {j.name}"
            same(_read(plan.d_rowptr, j.n_dst + 1), torch.from_numpy(r["rowptr"]), f"{what}: rowptr")
            same(_read(plan.d_t_rowptr, j.n_src + 1), torch.from_numpy(r["t_rowptr"]), f"{what}: t_rowptr")
            same(_read(plan.d_eid, j.E), torch.from_numpy(r["eid"]), f"{what}: eid")
            same(_read(plan.d_col, j.E), torch.from_numpy(r["col"]), f"{what}: col")
            same(_read(plan.d_t_col, j.E), torch.from_numpy(r["t_col"]), f"{what}: t_col")
            if kind == "gat":
                same(_read(plan.d_t_pos, j.E), torch.from_numpy(r["t_pos"]), f"{what}: t_pos")


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_argument_refusals(monkeypatch):
    lib = _lib.require_device()
    j = R.three_graphs()
    b = Buffers(j.E, j.n_src, j.n_dst)
    ei = _dev(j.ei, torch.int64)
    ptrs = [_dev(p, torch.int64) for p in (j.dst_ptr, j.src_ptr, j.edge_ptr)]

    def call(n=1, jobs=True, **over):
        a = (_lib.PlanJob * 1)()
        a[0].d_edge_index = ei.data_ptr()
        a[0].plan = _lib.Plan(j.n_src, j.n_dst, j.E, *(b.t[k].data_ptr() for k in ARRAYS))
        a[0].d_scratch = b.scratch.data_ptr()
        for k, v in over.items():
            if k in ARRAYS:
                setattr(a[0].plan, "d_" + k, v)
            else:
                setattr(a[0], k, v)
        return lib.hmp_plan_build_many(a if jobs else None, n, 1, 1, None, _lib.stream_ptr())

    assert call() == 0
    assert call(n=0, jobs=False) == 0
    for bad in (dict(n=-1), dict(n=_lib.MAX_EDGE_TYPES + 1), dict(jobs=False), dict(d_scratch=None), dict(col=None), dict(t_pos=None),
                dict(rowptr=None), dict(d_dst_ptr=ptrs[0].data_ptr(), n_graphs=3),
                dict(d_dst_ptr=ptrs[0].data_ptr(), d_edge_ptr=ptrs[2].data_ptr(), n_graphs=3),
                dict(d_src_ptr=ptrs[1].data_ptr(), d_edge_ptr=ptrs[2].data_ptr(), n_graphs=3)):
        assert call(**bad) == 1, bad  # HMP_E_ARG
    torch.cuda.synchronize()
