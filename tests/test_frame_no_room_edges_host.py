"""``remove_room_edges=True`` in the native host stage of the frame pipeline (``hmp_frame_build_flags`` with
``HMP_FRAME_NO_ROOM_EDGES``; the reference's ``remove_room_edges_in_dsg``, ``mp3d_dataset.py:203-208``): on every case of
``_frame_cases`` the host stage equals, byte for byte, the host stage of the same frame with the room-room pairs deleted from
``edges`` by the test itself.  No GPU."""
import ctypes as C
import numpy as np
import pytest

import _frame_block as fb
import _frame_cases as fc
from hydra_gnn_amd import _lib, dsg

CASES = ["fixture", "special"] + fc.SIZES
MODES = {
    "typed": dict(),
    "typed_relpos": dict(relative_pos=True),
    "homogeneous": dict(homogeneous=True),
    "homogeneous_relpos": dict(homogeneous=True, relative_pos=True),
    "htree": dict(htree=True, clique_dim=6),
    "htree_homogeneous": dict(htree=True, clique_dim=6, homogeneous=True),
    "htree_relpos": dict(htree=True, clique_dim=9, htree_relative_pos=True),
    "htree_relpos_homogeneous": dict(htree=True, clique_dim=9, htree_relative_pos=True, homogeneous=True),
}
ROOMS = 4


def without_room_pairs(arrays):
    """the same frame with every edge between two room nodes deleted from ``edges``"""
    ids, layer, pos, bb_min, bb_max, label, edges = arrays
    layer_of = {int(i): int(l) for i, l in zip(ids, layer)}
    keep = np.array([not (layer_of.get(int(a)) == ROOMS and layer_of.get(int(b)) == ROOMS) for a, b in zip(edges[0], edges[1])], dtype=bool)
    return ids, layer, pos, bb_min, bb_max, label, np.ascontiguousarray(edges[:, keep])


def assert_same_stage(got, want):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), k
        else:
            assert got[k] == w, k


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_host_stage_equals_the_frame_without_its_room_pairs(case, mode):
    arrays, kw = fc.frame(case), MODES[mode]
    got = dsg.frame_host_stage(*arrays, sem_dim=0, remove_room_edges=True, **kw)
    assert_same_stage(got, dsg.frame_host_stage(*without_room_pairs(arrays), **kw))
    assert int(got["sizes"][_lib.FS_E_RR]) == 0 and got["rr_edges"].shape == (2, 0)
    plain = dsg.frame_host_stage(*arrays, **kw)
    if int(plain["sizes"][_lib.FS_E_RR]) > 0:  # the flag does something on a frame with room edges ...
        assert not np.array_equal(plain["block"], got["block"])
    else:  # ... and nothing on a frame without
        assert_same_stage(got, plain)
    assert_same_stage(dsg.frame_host_stage(*arrays, remove_room_edges=False, **kw), plain)  # the default is today's behaviour


def test_semantic_rows_ride_along():
    arrays = fc.frame("special")
    kw = dict(sem_dim=300, n_labels=fc.N_LABELS)
    assert_same_stage(dsg.frame_host_stage(*arrays, remove_room_edges=True, **kw), dsg.frame_host_stage(*without_room_pairs(arrays), **kw))


@pytest.mark.parametrize("form", [_lib.FB_COLLATED, _lib.FB_STORE])
@pytest.mark.parametrize("mode", list(MODES))
def test_batch_host_stage_on_three_frames(mode, form):
    frames = [fc.frame("special"), fc.frame((7, 2)), fc.frame((300, 3))]
    kw = MODES[mode]
    got = dsg.frame_batch_host_stage(frames, form=form, remove_room_edges=True, **kw)
    want = dsg.frame_batch_host_stage([without_room_pairs(f) for f in frames], form=form, **kw)
    assert sorted(got) == sorted(want)
    for k in ("sizes", "graph_of_frame", "node_ptr", "edge_ptr", "tensors", "block", "groups", "items"):
        assert np.array_equal(got[k], want[k]), k
    assert got["num_graphs"] == want["num_graphs"] == 3 and got["max_graph_nodes"] == want["max_graph_nodes"]
    for g, w in zip(got["frames"], want["frames"]):
        assert_same_stage(g, w)
    assert not np.array_equal(got["block"], dsg.frame_batch_host_stage(frames, form=form, **kw)["block"])


def test_a_batch_shares_the_flag_and_unknown_flags_are_refused():
    lib = _lib.load()
    arrays, n, m = dsg._frame_args(*fc.frame((7, 2)))
    a = dsg._frame_build(lib, arrays, n, m, fc.THRESHOLDS, False, 0, 0, 0, 0, False, remove_room_edges=True)
    b = dsg._frame_build(lib, arrays, n, m, fc.THRESHOLDS, False, 0, 0, 0, 0, False)
    try:
        with pytest.raises(_lib.HydraMPError):
            dsg._batch_build(lib, [a, b], _lib.FB_COLLATED, None)
    finally:
        lib.hmp_frame_destroy(a)
        lib.hmp_frame_destroy(b)
    ids, layer, pos, bb_min, bb_max, label, edges = arrays
    h = C.c_void_p()
    rc = lib.hmp_frame_build_flags(n, ids.ctypes.data, layer.ctypes.data, pos.ctypes.data, bb_min.ctypes.data, bb_max.ctypes.data,
                                   label.ctypes.data, m, edges.ctypes.data, 1.5, 2.0, 0.2, 0, 0, 0, 0, 0, 0, 2, C.byref(h))
    assert rc != 0 and b"unknown flag" in lib.hmp_last_error()


@pytest.mark.parametrize("mode", ["typed_relpos", "htree_relpos"])
def test_the_flag_is_clean_under_asan_and_ubsan(tmp_path, mode):
    """`make frame_check`, run with --flags: frame.cpp + htree.cpp + a program with its own main under -fsanitize=address,undefined (CPU only, the
    runtimes linked statically, nothing preloaded) on existing ``HMPF`` files, with the flag from the command line and without"""
    kw = {k: v for k, v in MODES[mode].items() if k != "homogeneous"}
    files = []
    for name in ("fixture", "special", (7, 2)):
        files.append(str(tmp_path / f"frame_{len(files)}.bin"))
        dsg.save_frame_file(files[-1], *fc.frame(name), **kw)
    out = fb.run_frame_check(["--flags"] + files + ["--no-room-edges"] + files)
    assert "flags 0: kept 62 dropped 3 rooms 5 oo 178 rr 1 " in out and "flags 1: kept 62 dropped 3 rooms 5 oo 178 rr 0 " in out
    assert out.count("batch no-room-edges") == 4 and "(homogeneous) flags 1" in out
