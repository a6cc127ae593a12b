"""The edge lists of tests/test_gpu_plan_kernels.py sit in the regimes they claim (no GPU).

Every regime is recomputed here from the edge list and from the constants of csrc/plan_small.h and csrc/plan.hip, read out of
the sources: a changed tile, cap or threshold fails this file instead of letting a GPU case miss its branch.  The reference
itself is checked on a hand-written graph."""
import numpy as np

import _plan_reference as R

K = R.K


def cdiv(a, b):
    return -(-a // b)


def test_constants_are_the_ones_the_case_builders_assume():
    assert R.read_constants() == K
    assert R.RC_EDGES == 24 * 1024 and R.EDGE_TRIP == 2048 * 256 and R.RANK_TRIP == 8192 * 16
    assert K["WAVE"] // K["RANK_LANES"] == 4  # rows per wavefront of the rank kernel


def test_reference_on_a_hand_written_graph():
    #            e: 0  1  2  3   4  5  6
    j = R.job(src=[2, 0, 2, 9, 1, 0, 2], dst=[1, 1, 0, 0, -1, 1, 0], n_src=3, n_dst=3)
    r = R.reference(j)
    assert r["kept"] == 5 and r["status"] == 1
    assert r["rowptr"].tolist() == [0, 2, 5, 5]
    assert r["eid"].tolist() == [2, 6, 0, 1, 5] and r["col"].tolist() == [2, 2, 2, 0, 0]
    assert r["t_rowptr"].tolist() == [0, 2, 2, 5]
    assert r["t_col"].tolist() == [1, 1, 1, 0, 0]          # edges 1, 5 (source 0), then 0, 2, 6 (source 2)
    assert r["t_pos"].tolist() == [3, 4, 2, 0, 1]
    assert r["degf"].dtype == np.float32 and r["degf"].tolist() == [0.5, np.float32(1) / np.float32(3), 1.0]
    e = R.reference(R.job([], [], 0, 0))
    assert e["kept"] == 0 and e["rowptr"].tolist() == [0] and e["t_rowptr"].tolist() == [0] and e["degf"].size == 0
    assert R.reference(R.job([0], [0], 1, 1))["status"] == 0


def _order(j):
    ok = bool(R.valid_mask(j).all())
    return ok and R.is_sorted(j.ei[1]), ok and R.is_sorted(j.ei[0])  # what plan_hist_kernel calls ordered by destination / source


def test_six_jobs_boundaries_orders_and_shared_endpoints():
    want_order = {"both": (True, True), "dst": (True, False), "src": (False, True), "neither": (False, False),
                  "both_eq": (True, True), "oor": (False, False)}
    starts = []
    for v, (counts, orders) in enumerate(R.SIX_VARIANTS):
        jobs = R.six_jobs(v)
        assert [j.E for j in jobs] == counts and len(jobs) == 6
        assert (jobs[1].n_src, jobs[1].n_dst) == (0, 0)
        starts.append(np.cumsum([0] + counts)[1:-1].tolist())
        live = [(j, o) for j, o in zip(jobs, orders) if j.E > 0]
        for j, o in live:
            if j.E >= 4:
                assert _order(j) == want_order[o], (v, o)
            if o == "both":
                assert j.E < 4 or (np.diff(j.ei[1][2:-2]) > 0).all() and (np.diff(j.ei[0][2:-2]) > 0).all()
            if o == "both_eq" and j.E >= 4:
                assert (np.diff(j.ei[1][2:-2]) == 0).any() and (np.diff(j.ei[0][2:-2]) == 0).any()
            if o == "oor" and j.E >= 4:
                bad = np.nonzero(~R.valid_mask(j))[0]
                assert bad.tolist() == [j.E // 2]
                keep = R.valid_mask(j)
                assert R.is_sorted(j.ei[0][keep]) and R.is_sorted(j.ei[1][keep])  # sorted but for that edge
        # a run of equal destination AND source ids spans every boundary between two jobs that hold edges
        for (a, _), (b, _) in zip(live[:-1], live[1:]):
            assert a.ei[:, -1].tolist() == b.ei[:, 0].tolist()
            if a.E >= 4:
                assert a.ei[:, -2].tolist() == a.ei[:, -1].tolist()
            if b.E >= 4:
                assert b.ei[:, 1].tolist() == b.ei[:, 0].tolist()
    assert starts[0] == [37, 37, 137, 138, 202]  # job 1 is empty: job 2 starts at flat edge 37, inside wavefront 0
    assert all(s % K["WAVE"] for s in starts[0])
    assert starts[2] == [64, 64, 128, 129, 192] and [s % K["WAVE"] for s in starts[2]] == [0, 0, 0, 1, 0]
    # every order is shown by a job of >= 4 edges in some variant
    shown = {o for v, (c, os_) in enumerate(R.SIX_VARIANTS) for e, o in zip(c, os_) if e >= 4}
    assert shown == set(want_order)


def test_runs_and_holes_sit_at_their_lanes():
    W = K["WAVE"]
    for group_by in ("dst", "src"):
        j = R.runs_and_holes(group_by)
        keys = j.ei[1] if group_by == "dst" else j.ei[0]
        clean = keys.copy()
        clean[R.HOLE_KEY] = clean[R.HOLE_KEY + 1]  # the run as written, before its head's key was pushed out of range
        runs = R.run_lengths(clean)
        assert runs == R.RUNS
        assert len({int(clean[s]) for s, _ in runs}) == len(runs) and not R.is_sorted(clean)  # grouped, not sorted
        lengths = {n for _, n in runs}
        assert {1, 2, W - 1, W, W + 1, 2 * W + 2} <= lengths
        assert any(s % W == W - 1 for s, n in runs if n > 1)                 # a run begins at lane 63
        assert any((s + n - 1) % W == 0 for s, n in runs if n > 1)           # a run ends at lane 0
        assert j.E % W == 22                                                # the last wavefront is partly live
        bad = np.nonzero(~R.valid_mask(j))[0].tolist()
        assert sorted(bad) == sorted(R.HOLES_OTHER + [R.HOLE_KEY])
        big = next((s, n) for s, n in runs if n == 2 * W + 2)
        inside = [h for h in bad if big[0] <= h < big[0] + big[1]]
        assert big[0] in inside                                             # at the run's head
        assert any(h % W == 0 for h in inside) and any(h % W == W - 1 for h in inside)
        assert any(h % W not in (0, W - 1) and h != big[0] for h in inside)  # strictly inside
        assert 0 < R.reference(j)["kept"] == j.E - len(bad)


def test_rank_classes_share_wavefronts():
    a, b = R.rank_classes()
    assert np.bincount(a.ei[1], minlength=16).tolist() == R.RANK_DEGREES
    assert np.bincount(b.ei[0], minlength=16).tolist() == R.RANK_DEGREES
    assert not R.is_sorted(a.ei[1]) and not R.is_sorted(b.ei[0])
    per_wave = K["WAVE"] // K["RANK_LANES"]
    groups = [R.RANK_DEGREES[i:i + per_wave] for i in range(0, 16, per_wave)]
    assert groups[1] == [16, 17, 3, 32]  # rows 4..7 of job 0
    cls = ["short" if max(g) <= K["RANK_LANES"] else "two" if max(g) <= 2 * K["RANK_LANES"] else "long" for g in groups]
    assert cls == ["short", "two", "long", "long"]
    assert any(d <= 16 for d in groups[2]) and any(16 < d <= 32 for d in groups[1])  # mixed classes inside one wavefront
    # flat row list of the call: (job 0, dst) (job 0, src) (job 1, dst) (job 1, src); the 16 degree rows start on a wavefront
    starts = np.cumsum([0, a.n_dst, a.n_src, b.n_dst]).tolist()
    assert starts[0] % per_wave == 0 and starts[3] % per_wave == 0


def test_second_trips_are_taken():
    (j,) = R.second_trip_edges()
    assert j.E == 2048 * 256 + 77 and (j.n_dst, j.n_src) == (140_000, 70_000)
    assert R.EDGE_TRIP < j.E < 2 * R.EDGE_TRIP and cdiv(j.E, K["EDGE_BLOCK"]) > K["EDGE_GRID"]
    assert j.n_dst + j.n_src > R.RANK_TRIP and j.n_dst > R.RANK_TRIP     # rows of both directions reach the second trip
    assert j.E > K["PS_MAX_EDGES"]
    (t,) = R.second_trip_tops()
    assert t.n_dst == 1024 * 4096 + 3 and t.n_src == 4096 and t.E == 5000
    assert cdiv(t.n_dst, K["SCAN_SEG"]) == K["TOPS_CHUNK"] + 1           # one segment past the first chunk of the tops kernel
    assert sorted(set(t.ei[1].tolist())) == [0, 4095, 4096, 1024 * 4096 - 1, 1024 * 4096, 1024 * 4096 + 2]
    segs = sorted({r // K["SCAN_SEG"] for r in t.ei[1].tolist()})
    assert segs == [0, 1, K["TOPS_CHUNK"] - 1, K["TOPS_CHUNK"]]
    assert [j.n_dst for j in R.segment_edges()] == [1, 4095, 4096, 4097, 8193]
    for j in R.segment_edges():
        assert {0, j.n_dst - 1} <= set(j.ei[1].tolist()) and {0, j.n_src - 1} <= set(j.ei[0].tolist()) and j.E == 9


def test_scratch_sequence():
    seq = R.scratch_sequence()
    ns, nd = R.SCRATCH_N_SRC, R.SCRATCH_N_DST
    assert all((j.n_src, j.n_dst) == (ns, nd) and j.E <= R.SCRATCH_CAP for j in seq) and seq[0].E == R.SCRATCH_CAP
    assert [_order(j) for j in seq[:2]] == [(False, False), (True, True)] and _order(seq[5]) == (False, False)
    kept = [R.reference(j)["kept"] for j in seq]
    assert kept[2] == seq[2].E - 60 and kept[3] == 0 and seq[3].E == 2000 and seq[4].E == 0 and kept[5] == seq[5].E
    assert R.counter_ints(ns, nd) == 2 * 704 + 2 * 960
    for modes in R.SCRATCH_MODES:
        assert len(modes) == 6 and set(modes) == {0, 1}
    # both builds run every step in some pattern; an ordered multi-launch build follows an unordered one on the same stamps
    assert all({m[i] for m in R.SCRATCH_MODES} == {0, 1} for i in range(6))
    assert R.SCRATCH_MODES[2][:2] == [0, 0]


def _parts(n_rows, rows_max):
    """(parts, rows per part) of one direction as plan_small_layout lays them out"""
    parts = cdiv(n_rows, rows_max) if n_rows > 0 else 1
    return parts, (cdiv(n_rows, parts) if n_rows > 0 else 1)


def _part_edges(j, direction, rows_max):
    """kept edges of every part of one direction"""
    n_rows = j.n_dst if direction == 0 else j.n_src
    parts, rpp = _parts(n_rows, rows_max)
    keys = j.ei[1 - direction][R.valid_mask(j)]
    return [int(((keys >= p * rpp) & (keys < min(n_rows, (p + 1) * rpp))).sum()) for p in range(parts)]


def test_single_launch_cases():
    cases = R.small_cases()

    def register_cached(jobs):
        return max(j.E for j in jobs) <= R.RC_EDGES

    assert [j.E for j in cases["rc_alone"]] == [24 * 1024] and register_cached(cases["rc_alone"])
    assert max(j.E for j in cases["rc_companions"]) == 24 * 1024 and register_cached(cases["rc_companions"])
    assert sorted(j.E for j in cases["rc_companions"]) == [0, 1, 5, 24 * 1024]
    assert max(j.E for j in cases["streaming"]) == 24 * 1024 + 1 and not register_cached(cases["streaming"])
    assert len(cases["streaming"]) == 3  # the tiny companions stream as well
    (at,), (past,) = cases["slots_rc_lds"], cases["slots_rc_global"]
    assert at.n_dst == past.n_dst == 1
    assert _part_edges(at, 0, K["PS_ROWS"]) == [12 * 1024] and _part_edges(past, 0, K["PS_ROWS"]) == [12 * 1024 + 1]  # 12 288 / 12 289
    assert _part_edges(at, 0, K["PS_ROWS"])[0] == K["PS_TMP"]
    assert max(_part_edges(at, 1, K["PS_ROWS"]) + _part_edges(past, 1, K["PS_ROWS"])) <= K["PS_TMP"]
    assert register_cached([at]) and register_cached([past]) and [j.E for j in cases["slots_streaming"]] == [at.E, past.E]
    # (the streaming form is chosen per call: PS_UB edges per thread and trip)
    assert cdiv(past.E, K["PS_UB"] * K["PS_THREADS"]) == 2
    (holes,) = cases["empty_rows"]
    assert holes.n_dst == 40 and holes.E == 13_000 > K["PS_TMP"]
    deg = np.bincount(holes.ei[1], minlength=40)
    assert [r for r in range(40) if deg[r] == 0] == [0, 7, 39]
    assert [j.n_dst for j in cases["row_counts"]] == [0, 1, 1024, 1025, 2049]
    assert [_parts(j.n_dst, K["PS_ROWS"])[0] for j in cases["row_counts"]] == [1, 1, 1, 2, 3]
    assert sorted(j.n_src for j in cases["row_counts"][1:]) == [1, 1024, 1025, 2049]
    for jobs in cases.values():
        assert sum(j.E for j in jobs) <= K["PS_MAX_EDGES"] and R.call_status(jobs) == 0


def _graph_sorted(j):
    """every edge lies inside the rows of the graph whose slice of the list holds it, and the offsets describe the batch"""
    if j.dst_ptr[-1] != j.n_dst or j.src_ptr[-1] != j.n_src or j.edge_ptr[-1] != j.E:
        return False
    g = np.searchsorted(j.edge_ptr, np.arange(j.E), side="right") - 1
    s, d = j.ei
    keep = R.valid_mask(j)
    return bool(((s >= j.src_ptr[g]) & (s < j.src_ptr[g + 1]) & (d >= j.dst_ptr[g]) & (d < j.dst_ptr[g + 1]))[keep].all())


def test_vouched_cases():
    cases = R.vouched_cases()
    S = K["PS_ROWS_SLICED"]
    for name, jobs in cases.items():
        assert R.call_status(jobs) == 0, name
        for j in jobs:
            if j.edge_ptr is not None:
                assert _graph_sorted(j), (name, j.name)
    (three,) = cases["three"]
    assert np.diff(three.dst_ptr).tolist() == [200, 200, 200] and three.dst_ptr.size == 4
    assert cases["one"][0].edge_ptr.size == 2
    (tiny,) = cases["tiny_1300"]
    rows, t_rows, edges = np.diff(tiny.dst_ptr), np.diff(tiny.src_ptr), np.diff(tiny.edge_ptr)
    assert rows.size == 1300 > K["PS_THREADS"] and set(rows.tolist()) == {0, 1, 2, 3, 4, 5, 6}
    assert (t_rows == 0).any() and (edges[(rows > 0) & (t_rows > 0)] == 0).any() and (edges > 0).any()
    assert _parts(tiny.n_dst, S)[0] > 4
    (inside,) = cases["boundary_inside"]
    parts, rpp = _parts(inside.n_dst, S)
    cuts = {p * rpp for p in range(1, parts)}
    assert cuts and not cuts & set(inside.dst_ptr.tolist())  # every part boundary falls inside a graph
    assert [(j.n_dst, j.n_src) for j in cases["row_counts"]] == [(255, 513), (256, 257), (257, 256), (513, 255)]
    assert [_parts(j.n_dst, S)[0] for j in cases["row_counts"]] == [1, 1, 2, 3]
    with_ptr = [j.edge_ptr is not None for j in cases["mixed"]]
    assert with_ptr == [True, False, True, False, True]
    # (one job with offsets makes the whole call stream: the register-cached form never reads slices)


def test_wrongly_vouched_cases_break_their_promise():
    w = R.wrongly_vouched()
    assert not _graph_sorted(w["permuted"]) and w["permuted"].edge_ptr[-1] == w["permuted"].E
    assert w["edge_offset"].edge_ptr[-1] == w["edge_offset"].E - 1
    assert w["row_offset"].dst_ptr[-1] == w["row_offset"].n_dst + 1 and w["row_offset"].src_ptr[-1] == w["row_offset"].n_src + 1
    assert _graph_sorted(R.three_graphs())  # the builders above changed copies


def test_vouched_out_of_range_cases():
    o = R.vouched_out_of_range()
    for name, graphs in [("first", [0]), ("middle", [1]), ("last", [2]), ("all", [0, 1, 2])]:
        j = o[name]
        bad = np.nonzero(~R.valid_mask(j))[0]
        g = (np.searchsorted(j.edge_ptr, bad, side="right") - 1).tolist()
        assert g == graphs and _graph_sorted(j)
        r = R.reference(j)
        assert r["status"] == 1 and r["kept"] == j.E - len(graphs) and r["rowptr"][-1] == r["kept"]
        # three parts of 200 rows per direction: each graph is one part, the later parts start behind the dropped edge
        assert _parts(j.n_dst, K["PS_ROWS_SLICED"]) == (3, 200)
