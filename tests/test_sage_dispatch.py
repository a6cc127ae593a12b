"""The SAGE aggregation cases of tests/test_gpu_sage_kernels.py, checked on the host (no GPU) through the dispatch mirror in
tests/_sage_regimes.py: together they launch every instantiation of agg_fwd_kernel / agg_bwd_kernel (GS x NV),
agg_proj_fwd_kernel / agg_bwd_dx_kernel (GS), the cross-entropy epilogue at every row-group width, 8-row tiles and none, and
the LDS-window kernels on chunks that fit and chunks that do not; the graphs carry the degree classes they promise."""
import numpy as np
import pytest

import _sage_regimes as R


@pytest.fixture(scope="module")
def launches():
    return R.case_launches()


def test_dispatch_cases_reach_every_instantiation(launches):
    by =lambda k: {(d["gs"], d["nv"]) for _, d in launches if d["kernel"] == k}
    assert by("agg_fwd_kernel") == R.AGG_SHAPES
    assert by("agg_bwd_kernel") == R.AGG_SHAPES
    assert {gs for gs, _ in by("agg_proj_fwd_kernel")} == R.PROJ_GS
    assert {gs for gs, _ in by("agg_bwd_dx_kernel")} == R.PROJ_GS
    # the cross entropy rides in the last aggregation at every row-group width: GS comes from the widest entry of that launch
    ce = {(c[1], d["gs"]) for c, d in launches if d["ce"]}
    assert ce == {(26, 8), (40, 16), (100, 32), (200, 64)}, ce
    assert not any(d["ce"] for c, d in launches if c[0] != "ce")
    # 8-row tiles in the plain and the fused kernels for the regime scene alone, none once the launch is past 3584 rows
    tiles = {c[1]: {(d["kernel"], d["tile8"]) for cc, d in launches if cc == c} for c, _ in launches if c[0] == "launch"}
    assert ("agg_fwd_kernel", True) in tiles[1] and ("agg_proj_fwd_kernel", True) in tiles[1] and ("agg_bwd_dx_kernel", True) in tiles[1]
    assert not any(t for _, t in tiles[10])


def test_fused_projection_edges_are_reached(launches):
    """hidden 48 / 208: pK not a multiple of 64 (the clamped last k trip); stacked pncols not a multiple of 16 (clamped columns)"""
    proj = [(c, d) for c, d in launches if d["kernel"] == "agg_proj_fwd_kernel"]
    pk = {k for _, d in proj for k in d["pK"].values()}
    assert {48, 208} <= pk and any(k % 64 for k in pk) and all(k % 16 == 0 for k in pk)
    assert any(n % 16 for _, d in proj for n in d["pncols"].values())
    assert all(c[1] <= 256 for c, _ in proj if c[0] == "hidden")
    # hidden > 256 never fuses: that is how NV = 2..4 reach agg_fwd_kernel / agg_bwd_kernel under HMP_FUSE=1 too
    for c, d in launches:
        if c[0] == "hidden" and c[1] > 256:
            assert d["kernel"] in ("agg_fwd_kernel", "agg_bwd_kernel", "agg_bwd_dx_kernel")
            if d["layer"] < 2:
                assert d["nv"] > 1 or d["kernel"] == "agg_bwd_dx_kernel"


def test_unsupported_width_is_outside_the_instantiations():
    assert R.pick_shape(R.fpad(1024)) == (64, 4)
    assert R.pick_shape(R.fpad(R.UNSUPPORTED_HIDDEN)) not in R.AGG_SHAPES


def test_segment_mean_cases_reach_every_shape_and_both_vector_widths():
    shapes = {s for c in R.SEGMENT_CASES for s in R.segment_shape(*c)}
    assert {(gs, nv) for gs, nv, _ in shapes} == R.AGG_SHAPES
    assert {v for _, _, v in shapes} == {1, 4}
    assert any(len(R.segment_shape(*c)) > 1 for c in R.SEGMENT_CASES)


def test_regime_batches_have_every_degree_class():
    for copies in R.LAUNCH_COPIES:
        R.check_sage_regimes(R.regime_batch(copies))


def test_regime_scene_pairs_and_launch_sizes():
    b = R.regime_batch()
    n, e = R.batch_sizes(b)
    assert R.small_launch(n.values()) and sum(n.values()) <= 16 * R.AGG_SMALL_TILES
    assert R.heavy(e[R.O2R], n["rooms"]) and R.heavy(e[R.R2O], n["rooms"])  # rooms: 8-row tiles forward and backward
    b10 = R.regime_batch(10)
    n10, _ = R.batch_sizes(b10)
    assert min(n10.values()) > 16 * R.AGG_SMALL_TILES and not R.xcd_mapping(sum(n10.values()))


def test_window_graph_has_chunks_over_capacity_in_both_directions():
    g = R.window_graph()
    fwd, bwd = R.check_window_graph(g)
    n = int(g["objects"].x.size(0))
    assert R.win_in(256, n, True) and R.win_out(n, [256])
    assert not R.win_in(256, int(g["rooms"].x.size(0)), True)
    print(f"window graph: forward chunks over {R.WIDCAP} ids: {int((fwd > R.WIDCAP).sum())} of {fwd.size} (max {int(fwd.max())}), "
          f"backward: {int((bwd > R.WIDCAP).sum())} (max {int(bwd.max())})")
    assert np.all(fwd > 0)
