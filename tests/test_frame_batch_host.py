"""Host stage of frame batches (csrc/frame.cpp ``hmp_frame_batch_*``; include/hydra_mp.h section 14) without a device: the packed
block [group table | item table | sections] is executed with numpy, item by item, and every batched tensor is compared bit for bit
with ``data.collate`` / ``data.collate_homogeneous`` of the per-frame results of the existing path on the CPU (HMP_FB_COLLATED) and
with the arrays ``GraphStore.__init__`` cats (HMP_FB_STORE).  The two-level item lookup of ``frame_expand_batch_kernel`` is emulated
over the packed tables; capacity, refusals, empty batches and the stand-alone sanitizer program are covered as well."""
import numpy as np
import pytest

import _frame_batch_cases as bc
import _frame_block as fb
import _frame_cases as fc
from hydra_gnn_amd import _lib, dsg

LAYOUT_MODES = ["typed", "typed_htree", "homog", "homog_htree", "typed_relative_pos", "typed_sem300", "homog_htree_sem300"]
_GRAPHS = {}


def host(names, mode, form=_lib.FB_COLLATED, with_y=True):
    fr = bc.frames(names)
    return dsg.frame_batch_host_stage(fr, form=form, y=[bc.labels(a, i) for i, a in enumerate(fr)] if with_y else None,
                                      **bc.host_kwargs(mode))


def cpu_graphs(mode):
    """the existing path on every frame of the list, computed once per mode and left unchanged"""
    if mode not in _GRAPHS:
        fr = bc.frames()
        _GRAPHS[mode] = [bc.cpu_graph(a, mode, bc.labels(a, i)) for i, a in enumerate(fr)]
    return _GRAPHS[mode]


def run_block(r, mode):
    """({(store key or None, attribute): array}, written mask) of a batch block, executed with numpy"""
    sz = r["sizes"]
    table = fc.semantic_table().numpy() if bc.MODES[mode][3] else None
    fb.check_kinds(r["items"], fb.BATCH_KINDS)  # a batch holds no plain EDGE item
    arena, written = fb.expand(r["block"], r["items"], int(sz[_lib.FBS_ARENA_BYTES]), table)
    return fb.views(arena, r["tensors"], bc.MODES[mode][1], bc.MODES[mode][0]), written


def assert_tensors(got, want):
    assert sorted(map(str, got)) == sorted(map(str, want))
    for t, w in want.items():
        assert got[t].dtype == w.dtype and got[t].shape == w.shape and np.array_equal(got[t], w), t


@pytest.mark.parametrize("mode", LAYOUT_MODES)
def test_collated_block_equals_collate_of_the_single_frames(mode):
    r = host(bc.FRAME_NAMES, mode)
    graphs = cpu_graphs(mode)
    assert r["graph_of_frame"].tolist() == [0, 1, -1, 2, 3, 4] and r["num_graphs"] == 5
    assert [f["items"] == 0 for f in r["frames"]] == [g is None for g in graphs]
    want_batch = bc.collate([g for g in graphs if g is not None], bc.MODES[mode][0])
    got, written = run_block(r, mode)
    assert_tensors(got, bc.collated_arrays(want_batch, bc.MODES[mode][0]))
    # every byte of every tensor is written (exactly once: fb.expand), and nothing outside the tensors
    assert np.array_equal(fb.covered(written.size, r["tensors"], bc.MODES[mode][1], bc.MODES[mode][0]), written)
    if not bc.MODES[mode][0]:
        assert r["max_graph_nodes"] == want_batch.max_graph_nodes
        nodes, edges = dsg._node_type_names(bc.MODES[mode][1], False), dsg._edge_type_names(bc.MODES[mode][1], False)
        for k, t in enumerate(nodes):
            assert r["node_ptr"][k].tolist() == want_batch[t].ptr.tolist()
        for k, e in enumerate(edges):
            assert r["edge_ptr"][k].tolist() == want_batch[e].ptr.tolist()


@pytest.mark.parametrize("mode", LAYOUT_MODES)
def test_store_block_equals_what_graphstore_cats(mode):
    r = host(bc.FRAME_NAMES, mode, form=_lib.FB_STORE)
    graphs = [g for g in cpu_graphs(mode) if g is not None]
    homog, ht = bc.MODES[mode][:2]
    want = bc.store_arrays(graphs, homog)
    got, _ = run_block(r, mode)
    assert_tensors(got, want)
    assert not any(attr == "batch" for _, attr in got)
    for k, t in enumerate(dsg._node_type_names(ht, homog)):
        assert np.array_equal(r["node_ptr"][k], want[(t, "ptr")])
    for k, e in enumerate(dsg._edge_type_names(ht, homog)):
        assert np.array_equal(r["edge_ptr"][k], want[(e, "ptr")])


# name -> (frame names, mode, form, expected item count).  Item counts are K * (items of a frame) + (items of the batch), and no
# mode, form and K give exactly 65 (typed: even; H-tree: 29..55 per frame), so item 65 is covered twice: by the smallest batch
# that crosses item 64 (66 items) and by the first 65 items of that batch's tables, which are a complete table of their own
# (n_items = 65, n_blocks = the prefix word of item 65): what the kernel sees with one item in its second group.
FOUR = [(7, 2), "fixture", (1, 1), (65, 1)]
LOOKUP_CASES = {
    "below_64": ([(7, 2), "fixture"], "typed", _lib.FB_COLLATED, 2 * 16 + 6),
    "exactly_64": (FOUR, "homog", _lib.FB_COLLATED, 4 * 16),
    "item_65": (FOUR, "homog", _lib.FB_STORE, 65),  # 4 * 16 + 2 = 66, cut to 65
    "item_66": (FOUR, "homog", _lib.FB_STORE, 4 * 16 + 2),
    "four_groups": (bc.FRAME_NAMES, "typed_htree", _lib.FB_COLLATED, 5 * 39 + 21),
    "empty_tail_of_a_group": ([(1, 1)] * 6, "homog_htree", _lib.FB_COLLATED, 6 * 55),
}


@pytest.mark.parametrize("case", list(LOOKUP_CASES))
def test_two_level_lookup(case):
    names, mode, form, want_items = LOOKUP_CASES[case]
    r = host(names, mode, form)
    if case == "item_65":
        assert len(r["items"]) == 66
        r["sizes"][_lib.FBS_BLOCKS] = r["items"][65, _lib.FI_BLOCK0]
        r["items"] = r["items"][:65]
    items, groups, sz = r["items"], r["groups"], r["sizes"]
    n_items, n_blocks = len(items), int(sz[_lib.FBS_BLOCKS])
    assert n_items == want_items
    assert groups.size == -(-n_items // 64) == sz[_lib.FBS_GROUPS] and np.array_equal(groups, items[::64, _lib.FI_BLOCK0])
    # the prefix words: an item's word is the sum of the workgroups of the items before it
    blocks = fb.check_prefix(items, n_blocks)
    if case == "empty_tail_of_a_group":  # empty items at the end of a group, a non-empty one at the start of the next
        assert any(blocks[64 * g - 1] == 0 and blocks[64 * g] > 0 for g in range(1, groups.size)), blocks.reshape(-1)[:200]
    # every workgroup maps to a non-empty item; each item gets exactly its number of workgroups, in order
    found = [fb.lookup(groups, items, n_items, b) for b in range(n_blocks)]
    assert found == sorted(found) and all(blocks[i] > 0 for i in found)
    assert np.array_equal(np.bincount(found, minlength=n_items), blocks)
    # every section read and arena write lies inside its buffer and is aligned (checked by the numpy execution)
    got, written = run_block(r, mode)
    assert written.any() and sz[_lib.FBS_STAGING_BYTES] == r["block"].size
    header = ((groups.size * 4 + 15) & ~15) + ((len(host(names, mode, form)["items"]) * 48 + 15) & ~15)  # sections start behind both tables
    for it in items.tolist():
        secs = it[_lib.FI_S0:_lib.FI_S0 + 1] if it[_lib.FI_KIND] == _lib.FK_EDGE_SEG else it[_lib.FI_S0:_lib.FI_S3 + 1]
        assert all(s == -1 or (s % 16 == 0 and header <= s < r["block"].size) for s in secs), it
    assert all(dst % 16 == 0 for _, dst, _, _ in r["tensors"].tolist())


def test_capacity():
    """the largest number of (1, 1) typed baseline frames that fits 4096 items builds and packs; one more is refused"""
    per_frame, per_batch = 12 + 2, 2 + 4  # a frame's 12 tensors + its two `batch` segments; `ptr` of 2 node and 4 edge types
    k = (_lib.FRAME_BATCH_MAX_ITEMS - per_batch) // per_frame
    r = host([(1, 1)] * k, "typed", with_y=False)
    assert len(r["items"]) == k * per_frame + per_batch <= 4096 < (k + 1) * per_frame + per_batch
    assert r["groups"].size == 64 and r["num_graphs"] == k and r["block"].size == r["sizes"][_lib.FBS_STAGING_BYTES]
    found = [fb.lookup(r["groups"], r["items"], len(r["items"]), b) for b in (0, int(r["sizes"][_lib.FBS_BLOCKS]) - 1)]
    assert found[0] == 0 and found[1] == len(r["items"]) - 1
    with pytest.raises(_lib.HydraMPError, match="4096"):
        host([(1, 1)] * (k + 1), "typed", with_y=False)


def test_mixed_configurations_are_refused():
    lib = _lib.load()
    import ctypes as C

    handles = []
    try:
        for kw in (dict(), dict(htree=True, clique_dim=6), dict(relative_pos=True), dict(sem_dim=300, n_labels=fc.N_LABELS), dict(homogeneous=True),
                   dict(htree=True, clique_dim=8)):
            arrays, n, m = dsg._frame_args(*fc.frame((7, 2)))
            handles.append(dsg._frame_build(lib, arrays, n, m, fc.THRESHOLDS, kw.get("htree", False), kw.get("relative_pos", False),
                                            kw.get("sem_dim", 0), kw.get("n_labels", 0), kw.get("clique_dim"), kw.get("homogeneous", False)))
        for a, b in [(0, k) for k in range(1, 5)] + [(1, 5)]:
            hb = C.c_void_p()
            rc = lib.hmp_frame_batch_build(2, (C.c_void_p * 2)(handles[a], handles[b]), _lib.FB_COLLATED, None, C.byref(hb))
            assert rc == 1 and b"configurations" in lib.hmp_last_error(), (a, b)  # HMP_E_ARG
        hb = C.c_void_p()
        assert lib.hmp_frame_batch_build(2, (C.c_void_p * 2)(handles[0], handles[0]), 7, None, C.byref(hb)) == 1  # no such form
    finally:
        for h in handles:
            lib.hmp_frame_destroy(h)
    fr = bc.frames([(7, 2), (1, 1)])
    with pytest.raises(_lib.HydraMPError, match="label vectors"):
        dsg.frame_batch_host_stage(fr, y=[bc.labels(fr[0])])
    with pytest.raises(_lib.HydraMPError, match="labels"):
        dsg.frame_batch_host_stage(fr, y=[bc.labels(fr[0]), bc.labels(fr[0])])


@pytest.mark.parametrize("mode", ["typed", "homog_htree"])
def test_a_batch_of_only_empty_frames_has_no_items(mode):
    r = host(["no_room", "no_room"], mode)
    sz = r["sizes"]
    assert r["graph_of_frame"].tolist() == [-1, -1] and r["num_graphs"] == 0
    assert [int(sz[k]) for k in (_lib.FBS_ITEMS, _lib.FBS_GROUPS, _lib.FBS_BLOCKS, _lib.FBS_STAGING_BYTES, _lib.FBS_ARENA_BYTES)] == [0] * 5
    assert r["block"].size == 0 and len(r["items"]) == 0
    r = dsg.frame_batch_host_stage([], **bc.host_kwargs(mode))
    assert r["num_graphs"] == 0 and len(r["items"]) == 0


@pytest.mark.parametrize("mode", LAYOUT_MODES)
@pytest.mark.parametrize("name", ["fixture", (1, 1)], ids=str)
def test_a_one_frame_batch_equals_the_frame(name, mode):
    """the tensors of a one-frame batch, read from its block, are the single-frame block's, executed with the same numpy code
    through its own item table"""
    homog, ht = bc.MODES[mode][:2]
    r = host([name], mode, with_y=False)
    got, _ = run_block(r, mode)
    single = dsg.frame_host_stage(*bc.frame(name), **bc.host_kwargs(mode))
    table = fc.semantic_table().numpy() if bc.MODES[mode][3] else None
    fb.check_kinds(single["items"], fb.HOMOG_KINDS) if homog else fb.check_typed_frame(single["items"])
    arena, _ = fb.expand(single["block"], single["items"], int(single["sizes"][_lib.FS_ARENA_BYTES]), table)
    want = fb.views(arena, fb.tensor_rows(single["items"]), ht, homog)
    frame_tensors = {k: v for k, v in got.items() if k[1] not in ("batch", "ptr")}
    assert sorted(map(str, frame_tensors)) == sorted(map(str, want))
    for k, w in want.items():
        assert frame_tensors[k].dtype == w.dtype and np.array_equal(frame_tensors[k], w), k
    # what the batch adds: one graph
    for (_, attr), v in got.items():
        if attr == "batch":
            assert not v.any()
        elif attr == "ptr":
            assert v.size == 2 and v[0] == 0


def test_batch_host_stage_is_clean_under_asan_and_ubsan(tmp_path):
    """`make frame_check`, run with --batch: frame.cpp + htree.cpp + a program with its own main under -fsanitize=address,undefined (CPU only,
    the runtimes linked statically, nothing preloaded, nothing loaded into Python), run on the frame list: frame build, batch build,
    sizes, host arrays, pack and destroy, in both forms and both layouts, baseline and H-tree"""
    runs = []
    for ht in (False, True):
        files = []
        for i, arrays in enumerate(bc.frames()):
            path = str(tmp_path / f"frame_{int(ht)}_{i}.bin")
            dsg.save_frame_file(path, *arrays, htree=ht, sem_dim=0 if ht else 300, n_labels=0 if ht else fc.N_LABELS, clique_dim=6 if ht else 0)
            files.append(path)
        runs.append(files)
    for files in runs:
        assert fb.run_frame_check(["--batch"] + files).count("frames 6 graphs 5") == 4  # typed / homogeneous x collated / store
