"""Host reference of the graph plan and the edge lists the plan-builder tests run (numpy only, no GPU, nothing shared with
csrc/plan.hip or csrc/plan_small.h).

``reference`` is the contract of include/hydra_mp.h section 1 for one job: edges with both endpoints in range, a stable sort by
destination (CSR) and by source (CSC), the CSR position of every CSC entry, ``1 / max(in-degree, 1)`` in float32 and the status
bits.  The case builders below place each edge list in one regime of the builder (a job boundary inside a wavefront, a run of
equal keys that begins at lane 63, a part of exactly PS_TMP edges, ...); tests/test_plan_reference.py recomputes every regime from
the edge lists and from the constants it reads out of the two source files, so a changed constant fails there instead of letting
a GPU case miss its branch.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hydra-gnn_amd", "csrc")

# the builder's constants as the case builders assume them (tests/test_plan_reference.py compares them with the sources)
K = dict(PS_ROWS=1024, PS_ROWS_SLICED=256, PS_TMP=12 * 1024, PS_RC=24, PS_UB=8, PS_MAX_EDGES=65536, SCAN_SEG=4096,
         PS_THREADS=1024, EDGE_GRID=2048, EDGE_BLOCK=256, RANK_GRID=8192, RANK_ROWS_PER_BLOCK=16, RANK_LANES=16, TOPS_CHUNK=1024,
         WAVE=64)
RC_EDGES = K["PS_RC"] * K["PS_THREADS"]             # largest edge type of a register-cached single-launch build
EDGE_TRIP = K["EDGE_GRID"] * K["EDGE_BLOCK"]        # edges one trip of the histogram / fill / link grids covers
RANK_TRIP = K["RANK_GRID"] * K["RANK_ROWS_PER_BLOCK"]  # rows one trip of the rank grid covers
STATUS_DROPPED, STATUS_NOT_GRAPH_SORTED = 1, 4


def read_constants() -> dict:
    """the same names as ``K``, read out of csrc/plan_small.h and csrc/plan.hip"""
    small = open(os.path.join(CSRC, "plan_small.h")).read()
    plan = open(os.path.join(CSRC, "plan.hip")).read()

    def const(text, name):
        m = re.search(r"constexpr\s+(?:int|int64_t)\s+%s\s*=\s*([0-9 *+]+);" % name, text)
        assert m, name
        return int(eval(m.group(1), {"__builtins__": {}}))

    def one(pattern, text, what):
        found = set(re.findall(pattern, text))
        assert len(found) == 1, f"{what}: {sorted(found)}"
        v = found.pop()
        if isinstance(v, tuple):
            assert len(set(v)) == 1, f"{what}: {v}"
            v = v[0]
        return int(v)

    out = {n: const(small, n) for n in ("PS_ROWS", "PS_ROWS_SLICED", "PS_TMP", "PS_RC", "PS_UB", "PS_MAX_EDGES")}
    out["SCAN_SEG"] = const(plan, "SCAN_SEG")
    out["PS_THREADS"] = one(r"__launch_bounds__\((\d+)\) void plan_small_kernel", plan, "threads of a single-launch part")
    assert re.search(r"emax <= \(int64_t\)PS_RC \* %d;" % out["PS_THREADS"], small), "register-cached bound"
    out["EDGE_GRID"] = one(r"cdiv\(E, \d+\) < (\d+) \? cdiv\(E, \d+\) : (\d+)", plan, "edge grid cap")
    out["EDGE_BLOCK"] = one(r"cdiv\(E, (\d+)\) < \d+ \? cdiv\(E, (\d+)\) : \d+", plan, "edge block")
    for kern in ("plan_hist_kernel", "plan_fill_kernel", "plan_link_kernel"):
        assert re.search(r"__launch_bounds__\(%d\) void %s\b" % (out["EDGE_BLOCK"], kern), plan), kern
    out["RANK_GRID"] = one(r"want > (\d+) \? (\d+) : want", plan, "rank grid cap")
    out["RANK_ROWS_PER_BLOCK"] = one(r"const int64_t want = cdiv\(rows, (\d+)\);", plan, "rank rows per block")
    m = re.search(r"void plan_rank_kernel\(.*?const int lane = threadIdx\.x & (\d+);\s*const int64_t grp = [^;]*>> (\d+);", plan, re.S)
    assert m, "rank kernel row groups"
    assert (1 << int(m.group(2))) == int(m.group(1)) + 1
    out["RANK_LANES"] = int(m.group(1)) + 1
    assert re.search(r"__launch_bounds__\(256\) void plan_rank_kernel", plan) and 256 // out["RANK_LANES"] == out["RANK_ROWS_PER_BLOCK"]
    out["TOPS_CHUNK"] = one(r"for \(int b0 = 0; b0 < nseg; b0 \+= (\d+)\)", plan, "segments per trip of the tops kernel")
    out["WAVE"] = one(r"const int lane = threadIdx\.x & (\d+);\s*const int pk = __shfl_up", plan, "wavefront of run_slot") + 1
    return out


# -----------------------------------------------------------------------------------------------------------------------
# the reference
# -----------------------------------------------------------------------------------------------------------------------
@dataclass
class Job:
    ei: np.ndarray                       # int64 [2, E]
    n_src: int
    n_dst: int
    dst_ptr: Optional[np.ndarray] = None  # int64 [n_graphs + 1] (all three or none)
    src_ptr: Optional[np.ndarray] = None
    edge_ptr: Optional[np.ndarray] = None
    name: str = ""

    @property
    def E(self) -> int:
        return int(self.ei.shape[1])

    def without_offsets(self) -> "Job":
        return Job(self.ei, self.n_src, self.n_dst, name=self.name)


def job(src, dst, n_src, n_dst, name="") -> Job:
    ei = np.stack([np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)])
    return Job(np.ascontiguousarray(ei), int(n_src), int(n_dst), name=name)


def valid_mask(j: Job) -> np.ndarray:
    s, d = j.ei
    return (s >= 0) & (s < j.n_src) & (d >= 0) & (d < j.n_dst)


def reference(j: Job) -> dict:
    s, d = j.ei
    ids = np.nonzero(valid_mask(j))[0].astype(np.int64)
    kept = int(ids.size)
    order = ids[np.argsort(d[ids], kind="stable")]
    t_order = ids[np.argsort(s[ids], kind="stable")]
    deg = np.zeros(j.n_dst, dtype=np.int64)
    np.add.at(deg, d[ids], 1)
    t_deg = np.zeros(j.n_src, dtype=np.int64)
    np.add.at(t_deg, s[ids], 1)
    pos_of = np.full(j.E, -1, dtype=np.int64)
    pos_of[order] = np.arange(kept, dtype=np.int64)
    return dict(kept=kept,
                rowptr=np.concatenate([[0], np.cumsum(deg)]).astype(np.int64),
                eid=order, col=s[order],
                t_rowptr=np.concatenate([[0], np.cumsum(t_deg)]).astype(np.int64),
                t_col=d[t_order], t_pos=pos_of[t_order],
                degf=np.float32(1) / np.maximum(deg, 1).astype(np.float32),
                status=STATUS_DROPPED if kept < j.E else 0)


def call_status(jobs: List[Job]) -> int:
    st = 0
    for j in jobs:
        st |= STATUS_DROPPED if int(valid_mask(j).sum()) < j.E else 0
    return st


def is_sorted(a) -> bool:
    a = np.asarray(a)
    return bool(np.all(a[1:] >= a[:-1]))


def run_lengths(keys):
    """[(start, length)] of the maximal runs of equal neighbouring keys"""
    keys = np.asarray(keys)
    if keys.size == 0:
        return []
    starts = np.concatenate([[0], np.nonzero(keys[1:] != keys[:-1])[0] + 1, [keys.size]])
    return [(int(a), int(b - a)) for a, b in zip(starts[:-1], starts[1:])]


def rand_job(rng, E, n_src, n_dst, name="") -> Job:
    return job(rng.integers(0, max(n_src, 1), E), rng.integers(0, max(n_dst, 1), E), n_src, n_dst, name)


# -----------------------------------------------------------------------------------------------------------------------
# multi-launch build: six jobs in one call
# -----------------------------------------------------------------------------------------------------------------------
# (edge counts, order of each job).  Variant 0 is the list as written down; with it the "dst" and "neither" orders fall on the
# empty and the one-edge job, so variant 1 deals the orders to the jobs that can show them, and variant 2 moves the job
# boundaries onto wavefront edges (flat edges 64, 128, 192).
SIX_VARIANTS = [
    ([37, 0, 100, 1, 64, 129], ["both", "dst", "src", "neither", "both_eq", "oor"]),
    ([37, 0, 100, 1, 64, 129], ["dst", "both", "neither", "src", "oor", "both_eq"]),
    ([64, 0, 64, 1, 63, 129], ["src", "both", "dst", "neither", "both_eq", "oor"]),
]


def _side_keys(rng, E, lo, hi, kind):
    """E keys in [lo, hi]: the first two are lo and the last two hi (E >= 4); kind: strict / equal (sorted) or random (not sorted)"""
    if E == 1:
        return np.array([lo], dtype=np.int64)
    assert E >= 4 and hi - lo - 1 >= E
    inner = np.arange(lo + 1, hi)
    if kind == "strict":
        mid = np.sort(rng.choice(inner, E - 4, replace=False))
    elif kind == "equal":
        mid = np.sort(rng.choice(inner[:: max(len(inner) // max(E // 8, 1), 1)], E - 4, replace=True))
    else:
        mid = rng.choice(inner, E - 4, replace=False)
        while is_sorted(mid):
            mid = rng.permutation(mid)
    return np.concatenate([[lo, lo], mid, [hi, hi]]).astype(np.int64)


def six_jobs(variant: int) -> List[Job]:
    counts, orders = SIX_VARIANTS[variant]
    rng = np.random.default_rng(600 + variant)
    kinds = {"both": ("strict", "strict"), "dst": ("random", "strict"), "src": ("strict", "random"), "neither": ("random", "random"),
             "both_eq": ("equal", "equal"), "oor": ("strict", "strict")}
    jobs, lo = [], (0, 0)
    for E, order in zip(counts, orders):
        if E == 0:
            jobs.append(job([], [], 0, 0, name=f"empty({order})"))
            continue
        hi = lo if E == 1 else (lo[0] + 2 * E + 5, lo[1] + 2 * E + 9)
        ks, kd = kinds[order]
        src, dst = _side_keys(rng, E, lo[0], hi[0], ks), _side_keys(rng, E, lo[1], hi[1], kd)
        n_src, n_dst = hi[0] + 3, hi[1] + 2
        if order == "oor" and E > 1:
            src[E // 2] = n_src  # one past the end
        jobs.append(job(src, dst, n_src, n_dst, name=order))
        lo = hi
    return jobs


# -----------------------------------------------------------------------------------------------------------------------
# multi-launch build: runs of equal keys and holes at chosen lanes
# -----------------------------------------------------------------------------------------------------------------------
# (start, length) of every run; lane = start % 64.  [63, 65) begins at lane 63 and ends at lane 0; [192, 257) ends at lane 0 too;
# [447, 452) begins at lane 63; 470 edges: the last wavefront holds 22
RUNS = [(0, 1), (1, 2), (3, 60), (63, 2), (65, 63), (128, 64), (192, 65), (257, 130), (387, 60), (447, 5), (452, 18)]
# holes (one endpoint out of range): head of the 130-run, inside it, at its lane 0, at its lane 63; head of a run at lane 0;
# and one whose KEY is out of range (head of [387, 447))
HOLES_OTHER = [257, 300, 320, 383, 128]
HOLE_KEY = 387


def runs_and_holes(group_by: str) -> Job:
    rng = np.random.default_rng(71 if group_by == "dst" else 72)
    n_key, n_other = 600, 50
    E = RUNS[-1][0] + RUNS[-1][1]
    ids = rng.permutation(n_key)[: len(RUNS)]  # grouped, not sorted: a key never comes back
    keys = np.concatenate([np.full(n, k, dtype=np.int64) for k, (_, n) in zip(ids, RUNS)])
    other = rng.integers(0, n_other, E).astype(np.int64)
    other[rng.random(E) < 0.3] = other[0]  # runs on the other side as well
    for i, h in enumerate(HOLES_OTHER):
        other[h] = n_other if i % 2 == 0 else -3
    keys[HOLE_KEY] = n_key
    src, dst = (other, keys) if group_by == "dst" else (keys, other)
    n_src, n_dst = (n_other, n_key) if group_by == "dst" else (n_key, n_other)
    return job(src, dst, n_src, n_dst, name=f"runs by {group_by}")


# -----------------------------------------------------------------------------------------------------------------------
# multi-launch build: the three classes of the rank kernel in neighbouring 16-lane groups
# -----------------------------------------------------------------------------------------------------------------------
RANK_DEGREES = [0, 1, 15, 16, 16, 17, 3, 32, 33, 2, 0, 64, 65, 200, 16, 1]
RANK_OTHER_ROWS = 52  # keeps the 16 rows of the second job's source side on a wavefront boundary of the flat row list


def rank_classes() -> List[Job]:
    rng = np.random.default_rng(16)
    keys = np.repeat(np.arange(16), RANK_DEGREES)
    a = rng.permutation(keys.size)
    b = rng.permutation(keys.size)
    other_a, other_b = rng.integers(0, RANK_OTHER_ROWS, keys.size), rng.integers(0, RANK_OTHER_ROWS, keys.size)
    return [job(other_a[a], keys[a], RANK_OTHER_ROWS, 16, name="degrees by dst"),
            job(keys[b], other_b[b], 16, RANK_OTHER_ROWS, name="degrees by src")]


# -----------------------------------------------------------------------------------------------------------------------
# multi-launch build: second trips of the grid-stride loops
# -----------------------------------------------------------------------------------------------------------------------
def second_trip_edges() -> List[Job]:
    return [rand_job(np.random.default_rng(2048), EDGE_TRIP + 77, 70_000, 140_000, name="edge and rank loops twice")]


TOPS_N_DST = K["TOPS_CHUNK"] * K["SCAN_SEG"] + 3
TOPS_ROWS = [0, K["SCAN_SEG"] - 1, K["SCAN_SEG"], K["TOPS_CHUNK"] * K["SCAN_SEG"] - 1, K["TOPS_CHUNK"] * K["SCAN_SEG"], TOPS_N_DST - 1]
TOPS_COUNTS = [1000, 700, 900, 800, 600, 1000]


def second_trip_tops() -> List[Job]:
    rng = np.random.default_rng(4096)
    dst = rng.permutation(np.repeat(np.array(TOPS_ROWS, dtype=np.int64), TOPS_COUNTS))
    return [job(rng.integers(0, K["SCAN_SEG"], dst.size), dst, K["SCAN_SEG"], TOPS_N_DST, name="tops carry")]


SEGMENT_ROWS = [1, K["SCAN_SEG"] - 1, K["SCAN_SEG"], K["SCAN_SEG"] + 1, 2 * K["SCAN_SEG"] + 1]


def segment_edges() -> List[Job]:
    rng = np.random.default_rng(8193)
    jobs = []
    for n in SEGMENT_ROWS:
        dst = np.concatenate([[0, n - 1, n - 1], rng.integers(0, n, 6)])
        src = np.concatenate([rng.integers(0, n, 6), [n - 1, 0, n - 1]])
        jobs.append(job(src, dst, n, n, name=f"{n} rows"))
    return jobs


# -----------------------------------------------------------------------------------------------------------------------
# one scratch, counters zeroed once
# -----------------------------------------------------------------------------------------------------------------------
SCRATCH_N_SRC, SCRATCH_N_DST, SCRATCH_CAP = 700, 900, 3000
SCRATCH_MODES = [[0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0], [0, 0, 1, 0, 0, 0]]  # HMP_PLAN_SMALL of the six builds


def scratch_sequence() -> List[Job]:
    rng = np.random.default_rng(6)
    ns, nd, cap = SCRATCH_N_SRC, SCRATCH_N_DST, SCRATCH_CAP
    a = rand_job(rng, cap, ns, nd, "unordered")
    b = job(np.sort(rng.integers(0, ns, cap)), np.sort(rng.integers(0, nd, cap)), ns, nd, "ordered")
    c = rand_job(rng, cap - 100, ns, nd, "out-of-range edges")
    holes = rng.choice(c.E, 60, replace=False)
    c.ei[0, holes[:20]] = ns
    c.ei[1, holes[20:40]] = -1
    c.ei[1, holes[40:]] = nd + 7
    d = rand_job(rng, 2000, ns, nd, "every edge out of range")
    d.ei[0, ::2] = ns
    d.ei[1, 1::2] = -2
    e = job([], [], ns, nd, "no edge")
    f = rand_job(rng, cap - 1, ns, nd, "unordered again")
    return [a, b, c, d, e, f]


def counter_ints(n_src: int, n_dst: int) -> int:
    a = lambda x: (x + 63) // 64 * 64  # noqa: E731
    return 2 * a(n_dst) + 2 * a(n_src)


# -----------------------------------------------------------------------------------------------------------------------
# single-launch build
# -----------------------------------------------------------------------------------------------------------------------
def _tiny(rng, E, name):
    return rand_job(rng, E, 7, 5, name)


def one_row_job(rng, E, name):
    """n_dst = 1: the destination side is ONE part that holds every edge"""
    return job(rng.integers(0, 2000, E), np.zeros(E, dtype=np.int64), 2000, 1, name)


def empty_rows_job():
    rng = np.random.default_rng(40)
    rows = np.array([r for r in range(40) if r not in (0, 7, 39)])
    return job(rng.integers(0, 3000, 13_000), rows[rng.integers(0, rows.size, 13_000)], 3000, 40, "rows 0, 7, 39 empty")


SMALL_ROW_COUNTS = [0, 1, K["PS_ROWS"], K["PS_ROWS"] + 1, 2 * K["PS_ROWS"] + 1]


def small_cases() -> dict:
    """name -> jobs of one call (HMP_PLAN_SMALL=1); every one also fits the multi-launch build"""
    rng = np.random.default_rng(24)
    big = rand_job(rng, RC_EDGES, 3000, 2500, "largest register-cached job")
    over = rand_job(rng, RC_EDGES + 1, 3000, 2500, "one edge past the register cache")
    at, past = one_row_job(rng, K["PS_TMP"], "part of PS_TMP edges"), one_row_job(rng, K["PS_TMP"] + 1, "part of PS_TMP + 1 edges")
    n_src = [5] + SMALL_ROW_COUNTS[:0:-1]
    rows = [job([], [], n_src[0], 0, "0 rows")] + [rand_job(rng, 2000, ns, nd, f"{nd} rows") for ns, nd in zip(n_src[1:], SMALL_ROW_COUNTS[1:])]
    return {
        "rc_alone": [big],
        "rc_companions": [_tiny(rng, 5, "tiny"), big, _tiny(rng, 1, "one edge"), job([], [], 3, 4, "no edge")],
        "streaming": [_tiny(rng, 5, "tiny"), over, _tiny(rng, 1, "one edge")],
        "slots_rc_lds": [at],
        "slots_rc_global": [past],
        "slots_streaming": [at, past],
        "empty_rows": [empty_rows_job()],
        "row_counts": rows,
    }


# -----------------------------------------------------------------------------------------------------------------------
# graph-sorted ("vouched") edge lists
# -----------------------------------------------------------------------------------------------------------------------
def collate(graphs, name="") -> Job:
    """graphs: [(n_src, n_dst, ei [2, E] in the graph's own numbering)] -> one job with the three offset arrays"""
    src_ptr = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    dst_ptr = np.concatenate([[0], np.cumsum([g[1] for g in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([np.asarray(g[2]).reshape(2, -1).shape[1] for g in graphs])]).astype(np.int64)
    parts = [np.asarray(g[2], dtype=np.int64).reshape(2, -1) + np.array([[src_ptr[i]], [dst_ptr[i]]]) for i, g in enumerate(graphs)]
    ei = np.ascontiguousarray(np.concatenate(parts, axis=1)) if parts else np.zeros((2, 0), dtype=np.int64)
    return Job(ei, int(src_ptr[-1]), int(dst_ptr[-1]), dst_ptr, src_ptr, edge_ptr, name)


def _graph(rng, n_src, n_dst, E):
    if n_src == 0 or n_dst == 0:
        E = 0
    return (n_src, n_dst, np.stack([rng.integers(0, max(n_src, 1), E), rng.integers(0, max(n_dst, 1), E)]).astype(np.int64))


def _split(rng, total, n):
    """n positive graph sizes that sum to total"""
    cuts = np.sort(rng.choice(np.arange(1, total), n - 1, replace=False))
    return np.diff(np.concatenate([[0], cuts, [total]])).tolist()


def three_graphs(seed=3) -> Job:
    rng = np.random.default_rng(seed)
    return collate([_graph(rng, 200, 200, 500 + 50 * g) for g in range(3)], "3 graphs of 200 rows")


def vouched_cases() -> dict:
    """name -> jobs of one call; jobs with and without offsets"""
    rng = np.random.default_rng(256)
    tiny = []
    for g in range(1300):
        nd, ns = int(rng.integers(1, 7)), int(rng.integers(0, 3))
        if g % 97 == 0:
            nd = 0
        tiny.append(_graph(rng, ns, nd, int(rng.integers(0, 2 * nd + 1))))
    counts = []
    for n_dst, n_src in [(255, 513), (256, 257), (257, 256), (513, 255)]:
        gs = [_graph(rng, a, b, int(rng.integers(0, 4 * b))) for a, b in zip(_split(rng, n_src, 4), _split(rng, n_dst, 4))]
        counts.append(collate(gs, f"{n_dst} x {n_src} rows"))
    return {
        "three": [three_graphs()],
        "one": [collate([_graph(rng, 300, 300, 2000)], "1 graph of 300 rows")],
        "tiny_1300": [collate(tiny, "1300 graphs of 0..6 rows")],
        "boundary_inside": [collate([_graph(rng, 300, 300, 900) for _ in range(5)], "5 graphs of 300 rows")],
        "row_counts": counts,
        "mixed": [three_graphs(5), rand_job(rng, 3000, 400, 300, "no offsets"), counts[1], rand_job(rng, 10, 3, 3, "no offsets, tiny"),
                  collate(tiny[:200], "200 tiny graphs")],
    }


def wrongly_vouched() -> dict:
    """name -> one job whose offsets do not describe its edge list (status bit 2; arrays unspecified)"""
    rng = np.random.default_rng(4)
    base = three_graphs()
    perm = Job(np.ascontiguousarray(base.ei[:, rng.permutation(base.E)]), base.n_src, base.n_dst, base.dst_ptr, base.src_ptr, base.edge_ptr,
               "permuted under the old offsets")
    short = Job(base.ei, base.n_src, base.n_dst, base.dst_ptr, base.src_ptr, base.edge_ptr.copy(), "last edge offset != E")
    short.edge_ptr[-1] -= 1
    rows = Job(base.ei, base.n_src, base.n_dst, base.dst_ptr.copy(), base.src_ptr.copy(), base.edge_ptr, "last row offset != n_rows")
    rows.dst_ptr[-1] += 1
    rows.src_ptr[-1] += 1
    return {"permuted": perm, "edge_offset": short, "row_offset": rows}


def vouched_out_of_range() -> dict:
    """valid offsets, one endpoint out of range in the first / a middle / the last graph (and in all three)"""
    out = {}
    for name, where in [("first", [0]), ("middle", [1]), ("last", [2]), ("all", [0, 1, 2])]:
        j = three_graphs()
        j.name = f"out-of-range edge in graph {where}"
        for g in where:
            e = int(j.edge_ptr[g] + (j.edge_ptr[g + 1] - j.edge_ptr[g]) // 2)
            if g == 1:
                j.ei[1, e] = -1
            else:
                j.ei[0, e] = j.n_src
        out[name] = j
    return out
