"""The collation kernels of csrc/collate.hip on their own: ``collate_batch_kernel`` through ``hmp_collator_create`` /
``hmp_collator_run`` / ``hmp_collator_set_label_filter`` and the two older kernels through ``hmp_collate_rows`` /
``hmp_collate_edges``, driven with raw tensors (no ``GraphStore``).

Reference and case builders: tests/_collate_reference.py (numpy loops over the graphs of a selection; tests/test_collate_reference.py
holds it against ``data.collate`` on the CPU).  Collation moves bytes and adds integers, so every comparison is bit for bit.

Every destination lies inside a larger buffer filled with the byte ``SENT``: ``GUARD`` bytes in front, the capacity (a few rows more
than the batch needs) and ``GUARD`` bytes behind.  After a run the bytes of the batch equal the reference and every other byte of the
buffer still holds ``SENT``.  Every source array has a tail as long as its largest graph, so that a row search that picks a
neighbouring graph still reads inside the allocation (and fails the comparison).

What reaches which decision of the kernels:
  row classes     1 2 3 5 7 bytes: byte rows; 4 8 12 124 (31 units): narrow; 128 (32 units, the first wide width, where the
                  host's grid sizing changes too) 136 1224: wide, even, 8-byte copies; 132 1228: wide, odd, 4-byte
                  copies; 128 / 1224 with the source 4 bytes in and with the destination 4 bytes in: even widths on the 4-byte path
  workgroup cap   2048 workgroups cover 524 288 narrow rows / bytes / edges and 16 384 wide rows in one pass (4096 x 256 units, bytes
                  and edges for the older kernels); the cases are 37 rows above that
  table path      4 slots: B = 52 is 4 * 53 + 52 = 264 words (inline, the limit), B = 53 is 269 (ring)

The 31 | 32 unit boundary is read by the kernel's branch and by the host's grid sizing from one constant (CB_WIDE_UNITS).  Outputs
could not tell a disagreement: every loop of the kernel is grid-stride, so a 128-byte item that gets the other class's grid is
still copied completely, only with the wrong number of workgroups.  The 124 / 128 / 132 items hold each side's path to the
reference."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _collate_reference as R  # noqa: E402
from hydra_gnn_amd import _lib  # noqa: E402

DEV = "cuda:0"
SENT = 0xA5
GUARD = 64
G = 24  # graphs of a ragged dataset
ROW_BYTES = [1, 2, 3, 5, 7, 4, 8, 12, 124, 128, 132, 136, 1224, 1228]
E_ARG = "libhydra_mp error 1:"


def poisoned(nbytes):
    return torch.full((int(nbytes),), SENT, dtype=torch.uint8, device=DEV)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def all_sent(t):
    return bool((t == SENT).all())


def unit_of(it):
    """bytes per output row (an edge: both endpoints)"""
    return it.row_bytes if isinstance(it, R.RowItem) else 16


def upload_source(ds, it, offset=0):
    """the item's packed array ``offset`` bytes into an allocation, followed by a tail as long as its largest graph"""
    raw = it.data if isinstance(it, R.RowItem) else it.ei
    if raw is None:
        return None
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    tail = int(ds.counts(it.slot).max()) * unit_of(it)
    buf = poisoned(offset + raw.size + tail)
    buf[offset:offset + raw.size] = torch.from_numpy(raw).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[offset:]


class Collator:
    """a dataset of tests/_collate_reference.py on the device and its hmp_collator"""

    def __init__(self, ds, src_off=None, n_slots=None, n_items=None):
        self.lib = _lib.require_device()
        self.ds = ds
        src_off = src_off or {}
        self.ptr_dev = [to_dev(p) for p in ds.ptrs]
        self.src = [upload_source(ds, it, src_off.get(i, 0)) for i, it in enumerate(ds.items)]
        items = []
        for it, s in zip(ds.items, self.src):
            d_src = s.data_ptr() if s is not None else None
            if isinstance(it, R.RowItem):
                items.append(_lib.CollateItem(d_src, self.ptr_dev[it.slot].data_ptr(), 0, it.row_bytes, it.slot, 0, 0))
            else:
                e_total = 0 if it.ei is None else it.ei.shape[1]
                items.append(_lib.CollateItem(d_src, self.ptr_dev[it.slot].data_ptr(), e_total, 0, it.slot, it.slot_src, it.slot_dst))
        n_slots = len(ds.ptrs) if n_slots is None else n_slots
        n_items = len(items) if n_items is None else n_items
        items += [items[-1]] * (n_items - len(items))
        self._host_ptrs = [np.ascontiguousarray(p, dtype=np.int64) for p in ds.ptrs]
        self._host_ptrs += [self._host_ptrs[-1]] * (n_slots - len(self._host_ptrs))
        self._items = (_lib.CollateItem * n_items)(*items)
        self._slot_ptr = (C.c_void_p * n_slots)(*[p.ctypes.data for p in self._host_ptrs])
        self.h = C.c_void_p()
        _lib.check(self.lib.hmp_collator_create(n_slots, self._slot_ptr, ds.n_graphs, n_items, self._items, C.byref(self.h)))

    def set_filter(self, item, member, ignored):
        _lib.check(self.lib.hmp_collator_set_label_filter(self.h, item, member.data_ptr() if member is not None else None, ignored))

    def close(self):
        self.lib.hmp_collator_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Run:
    """one hmp_collator_run: fresh poisoned destinations, the launch, and (check) the comparison with the reference"""

    def __init__(self, col, sel, dst_off=None, stride=None, offsets=True, short=None, expected=None, slack=3):
        ds, self.col, self.sel = col.ds, col, [int(g) for g in sel]
        B = len(sel)
        ok_sel = [g for g in self.sel if 0 <= g < ds.n_graphs]  # a selection that will be refused: buffers sized by its valid part
        self.table, self.totals = R.offsets_ref(ds.ptrs, ok_sel)
        self.want = ds.expected(self.sel) if len(ok_sel) == B else [np.empty(0, np.uint8)] * len(ds.items)
        for i, w in (expected or {}).items():
            assert w.size == self.want[i].size
            self.want[i] = w
        dst_off = dst_off or {}
        self.bufs, self.lo = [], []
        caps = []
        for i, it in enumerate(ds.items):
            n_out = int(self.totals[it.slot])
            caps.append(n_out + slack)
            self.lo.append(GUARD + dst_off.get(i, 0))
            self.bufs.append(poisoned(self.lo[i] + caps[i] * unit_of(it) + GUARD))
            assert self.bufs[i].data_ptr() % 16 == 0
        if short is not None:  # the buffer is as large as ever, the caller claims one row less than the batch needs
            caps[short] = int(self.totals[ds.items[short].slot]) - 1
        self.stride = B + 1 if stride is None else stride
        n_slots = len(ds.ptrs)
        self.off_buf = poisoned(2 * GUARD + 8 * n_slots * max(self.stride, B + 1)) if offsets else None
        self.h_totals = (C.c_int64 * n_slots)(*([-7] * n_slots))
        d_dst = (C.c_void_p * len(caps))(*[b.data_ptr() + lo for b, lo in zip(self.bufs, self.lo)])
        sel32 = np.asarray(self.sel, dtype=np.int32)
        self.rc = col.lib.hmp_collator_run(col.h, sel32.ctypes.data, B, d_dst, (C.c_int64 * len(caps))(*caps), self.h_totals,
                                           self.off_buf.data_ptr() + GUARD if offsets else None, self.stride, _lib.stream_ptr())

    def offsets(self):
        return self.off_buf[GUARD:-GUARD].view(torch.int64)[:len(self.col.ds.ptrs) * self.stride].view(-1, self.stride)

    def check(self, what=""):
        _lib.check(self.rc)
        torch.cuda.synchronize()
        B = len(self.sel)
        assert list(self.h_totals) == self.totals.tolist(), what
        for i, (buf, lo, want) in enumerate(zip(self.bufs, self.lo, self.want)):
            assert torch.equal(buf[lo:lo + want.size], to_dev(want)), (what, i, self.col.ds.items[i])
            assert all_sent(buf[:lo]) and all_sent(buf[lo + want.size:]), (what, i, "wrote outside the batch's rows")
        if self.off_buf is not None:
            off = self.offsets()
            assert torch.equal(off[:, :B + 1], to_dev(self.table)), what
            assert all_sent(off[:, B + 1:].contiguous().view(torch.uint8)), (what, "padding columns of the offsets")
            assert all_sent(self.off_buf[:GUARD]) and all_sent(self.off_buf[GUARD + 8 * off.numel():]), what

    def check_refused(self):
        with pytest.raises(_lib.HydraMPError, match=E_ARG):
            _lib.check(self.rc)
        torch.cuda.synchronize()
        assert all(all_sent(b) for b in self.bufs) and (self.off_buf is None or all_sent(self.off_buf))


def selection_of(ds, slot, B, seed):
    """B graph ids with repeats; graphs that are empty in ``slot`` at the front, at the end and as a run in the middle"""
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, ds.n_graphs, size=B)
    empty = np.flatnonzero(ds.counts(slot) == 0)
    sel[0], sel[-1] = empty[0], empty[-1]
    if B >= 8:
        sel[B // 2:B // 2 + 3] = empty[1:4] if len(empty) >= 4 else empty[0]
    return sel.tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# collate_batch_kernel: every row class in one launch
# ---------------------------------------------------------------------------------------------------------------------------
def row_class_dataset():
    """18 row items over three node slots: ROW_BYTES, then the 128- and 1224-byte items with the source and with the destination
    4 bytes in"""
    sizes = ROW_BYTES + [128, 1224, 128, 1224]
    ds = R.make_dataset(17, G, [9, 6, 11], [(i % 3, rb) for i, rb in enumerate(sizes)])
    n = len(ROW_BYTES)
    return ds, {n: 4, n + 1: 4}, {n + 2: 4, n + 3: 4}


@pytest.fixture(scope="module")
def row_classes():
    ds, src_off, dst_off = row_class_dataset()
    with Collator(ds, src_off) as col:
        yield col, dst_off


@pytest.mark.parametrize("slot", [0, 1, 2])
@pytest.mark.parametrize("which", ["one", "repeats", "empty_edges_and_run", "only_empty"])
def test_batch_kernel_row_classes(row_classes, which, slot):
    col, dst_off = row_classes
    sel = R.ragged_selections(col.ds, slot, 5)[which]
    run = Run(col, sel, dst_off=dst_off)
    run.check((which, slot))
    if which == "only_empty":  # nothing of this slot, rows of the others
        assert run.totals[slot] == 0 and run.totals.sum() > 0
    else:
        assert run.totals[slot] > 0


def test_batch_kernel_row_classes_meet_all_four_alignments(row_classes):
    """the four cases the 8-byte test of a wide even row tells apart all occur: both aligned, source only, destination only (4 bytes
    in), and, for an odd width, every second row on a 4-byte address whatever the base"""
    col, dst_off = row_classes
    n = len(ROW_BYTES)
    for i in (n, n + 1):
        assert col.src[i].data_ptr() % 8 == 4 and col.src[ROW_BYTES.index(col.ds.items[i].row_bytes)].data_ptr() % 8 == 0
    run = Run(col, [1], dst_off=dst_off)
    for i in range(len(col.ds.items)):
        assert (run.bufs[i].data_ptr() + run.lo[i]) % 8 == (4 if i in dst_off else 0)
    assert (132 // 4) % 2 == 1 and (1228 // 4) % 2 == 1 and 124 // 4 == 31 and 128 // 4 == 32


# ---------------------------------------------------------------------------------------------------------------------------
# edge items
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_types():
    """two node slots, three edge slots (0 -> 0, 0 -> 1, 1 -> 0), x of both node types and a 12-byte edge_attr of each edge type"""
    ds = R.make_dataset(23, G, [8, 5], [(0, 20), (1, 8), (2, 12), (3, 12), (4, 12)], edge_items=[(0, 0, 13), (0, 1, 7), (1, 0, 9)])
    with Collator(ds) as col:
        yield col


@pytest.mark.parametrize("slot", [2, 3, 4])
@pytest.mark.parametrize("which", ["one", "repeats", "empty_edges_and_run", "only_empty"])
def test_batch_kernel_edge_items(edge_types, which, slot):
    col = edge_types
    ds = col.ds
    assert [(it.slot, it.slot_src, it.slot_dst) for it in ds.items[5:]] == [(2, 0, 0), (3, 0, 1), (4, 1, 0)]
    sel = R.ragged_selections(ds, slot, 9)[which]
    run = Run(col, sel)
    run.check((which, slot))
    if which == "empty_edges_and_run":  # the shifts are those of the selection: graphs without an edge still count their nodes
        assert any(ds.counts(slot)[g] == 0 and ds.counts(0)[g] > 0 for g in sel)


# ---------------------------------------------------------------------------------------------------------------------------
# the workgroup cap: a second pass of the grid-stride loops
# ---------------------------------------------------------------------------------------------------------------------------
def big_dataset(kind, per_graph, row_bytes=0, seed=3):
    """three graphs: a large one (selected repeatedly), an empty one and one of 37; one item of ``kind`` and a small 4-byte item on a
    slot of its own behind it (its workgroup comes after the capped ones)"""
    rng = np.random.default_rng(seed)
    big = np.array([per_graph, 0, 37], np.int64)
    small = np.array([5, 0, 3], np.int64)
    if kind == "edges":
        ec, ei = R.random_edges(rng, big, small, small)
        ds = R.Dataset(3, [R.ptr_of(small), R.ptr_of(ec)], [R.EdgeItem(1, 0, 0, ei)])
    else:
        ds = R.Dataset(3, [R.ptr_of(small), R.ptr_of(big)], [R.RowItem(1, row_bytes, R.random_rows(rng, big.sum(), row_bytes))])
    ds.items.append(R.RowItem(0, 4, R.random_rows(rng, small.sum(), 4)))
    return ds


BIG_SEL = [0] * 8 + [1, 2]

# (kind, rows or edges of the large graph, row bytes, what 2048 workgroups cover in one pass)
CAP_CASES = {
    "narrow": ("rows", 65536, 8, 2048 * 256),
    "wide": ("rows", 2048, 128, 2048 * 8),
    "bytes": ("rows", 21846, 3, 2048 * 256 // 3),
    "edges": ("edges", 65536, 0, 2048 * 256),
}


@pytest.mark.parametrize("name", list(CAP_CASES))
def test_batch_kernel_past_the_workgroup_cap(name):
    kind, per_graph, rb, one_pass = CAP_CASES[name]
    ds = big_dataset(kind, per_graph, rb)
    with Collator(ds) as col:
        run = Run(col, BIG_SEL)
        n_out = int(run.totals[1])
        assert one_pass < n_out <= one_pass + 64
        run.check(name)


# ---------------------------------------------------------------------------------------------------------------------------
# the older kernels: hmp_collate_rows / hmp_collate_edges
# ---------------------------------------------------------------------------------------------------------------------------
def run_old_rows(lib, ds, it, sel, src_off=0, dst_off=0):
    src = upload_source(ds, it, src_off)
    table, totals = R.offsets_ref(ds.ptrs, sel)
    n_out = int(totals[it.slot])
    want = R.collate_rows_ref(it.data, ds.ptrs[it.slot], sel).reshape(-1)
    lo = GUARD + dst_off
    buf = poisoned(lo + (n_out + 3) * it.row_bytes + GUARD)
    ptr, off, sel32 = to_dev(ds.ptrs[it.slot]), to_dev(table[it.slot]), to_dev(np.asarray(sel, np.int32))
    _lib.check(lib.hmp_collate_rows(src.data_ptr(), it.row_bytes, ptr.data_ptr(), sel32.data_ptr(), off.data_ptr(), len(sel), n_out,
                                    buf.data_ptr() + lo, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(buf[lo:lo + want.size], to_dev(want)), (it.row_bytes, sel)
    assert all_sent(buf[:lo]) and all_sent(buf[lo + want.size:]), (it.row_bytes, sel)
    return n_out


def run_old_edges(lib, ds, it, sel):
    src = upload_source(ds, it)
    table, totals = R.offsets_ref(ds.ptrs, sel)
    e_out = int(totals[it.slot])
    want = np.ascontiguousarray(R.collate_edges_ref(it.ei, ds.ptrs[it.slot], sel, ds.ptrs[it.slot_src], ds.ptrs[it.slot_dst]))
    want = want.view(np.uint8).reshape(-1)
    buf = poisoned(GUARD + (e_out + 3) * 16 + GUARD)
    ptr, sel32, tab = to_dev(ds.ptrs[it.slot]), to_dev(np.asarray(sel, np.int32)), to_dev(table)
    _lib.check(lib.hmp_collate_edges(src.data_ptr(), it.ei.shape[1], ptr.data_ptr(), sel32.data_ptr(), tab[it.slot].data_ptr(),
                                     tab[it.slot_src].data_ptr(), tab[it.slot_dst].data_ptr(), len(sel), e_out,
                                     buf.data_ptr() + GUARD, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(buf[GUARD:GUARD + want.size], to_dev(want)), sel
    assert all_sent(buf[:GUARD]) and all_sent(buf[GUARD + want.size:]), sel
    return e_out


@pytest.mark.parametrize("which", ["one", "repeats", "empty_edges_and_run", "only_empty"])
def test_older_kernels_ragged(which):
    lib = _lib.require_device()
    ds, src_off, dst_off = row_class_dataset()
    for i, it in enumerate(ds.items):
        sel = R.ragged_selections(ds, it.slot, 5)[which]
        n_out = run_old_rows(lib, ds, it, sel, src_off.get(i, 0), dst_off.get(i, 0))
        assert (n_out == 0) == (which == "only_empty")
    es = R.make_dataset(23, G, [8, 5], [], edge_items=[(0, 0, 13), (0, 1, 7), (1, 0, 9)])
    for it in es.items:
        run_old_edges(lib, es, it, R.ragged_selections(es, it.slot, 9)[which])


@pytest.mark.parametrize("name,kind,per_graph,rb", [("units", "rows", 65536, 8), ("bytes", "rows", 43691, 3), ("edges", "edges", 131072, 0)])
def test_older_kernels_past_the_grid_cap(name, kind, per_graph, rb):
    """4096 workgroups of 256 threads: more than 1 048 576 four-byte units, bytes, edges"""
    lib = _lib.require_device()
    ds = big_dataset(kind, per_graph, rb)
    it = ds.items[0]
    if kind == "edges":
        work = run_old_edges(lib, ds, it, BIG_SEL)
    else:
        work = run_old_rows(lib, ds, it, BIG_SEL) * (rb if rb & 3 else rb // 4)
    assert 4096 * 256 < work <= 4096 * 256 + 128


# ---------------------------------------------------------------------------------------------------------------------------
# the table path: inline | ring, the ring's life
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def four_slots():
    """two node slots, two edge slots; rows of every class and both edge lists"""
    ds = R.make_dataset(31, G, [6, 4], [(0, 1224), (0, 8), (1, 3), (1, 132), (2, 12)], edge_items=[(0, 1, 5), (1, 1, 4)])
    assert len(ds.ptrs) == 4
    return ds


@pytest.mark.parametrize("B,words", [(52, 264), (53, 269)])
def test_tables_inline_and_through_the_ring(four_slots, B, words):
    assert 4 * (B + 1) + B == words
    with Collator(four_slots) as col:
        Run(col, selection_of(four_slots, 0, B, B)).check(B)
        Run(col, selection_of(four_slots, 2, B, B + 1), stride=B + 7).check(B)


def test_ring_life(four_slots):
    """ten ring batches in flight (the ring has 8 slots), a batch more than twice as large (the ring is reallocated while in use),
    nine more at the old size; nothing waits between the launches of a group, so a slot rewritten too early would show"""
    B = 60
    assert 4 * (B + 1) + B > 264 and 4 * (131) + 130 > 2 * (4 * (B + 1) + B)
    with Collator(four_slots) as col:
        first = [Run(col, selection_of(four_slots, i % 4, B if i % 3 else B - 5, 100 + i)) for i in range(10)]
        for i, r in enumerate(first):
            r.check(("first", i))
        Run(col, selection_of(four_slots, 1, 130, 7)).check("regrow")
        later = [Run(col, selection_of(four_slots, i % 4, B, 200 + i)) for i in range(9)]
        for i, r in enumerate(later):
            r.check(("later", i))


@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("pad", [0, 6])
def test_offsets_out_and_totals(four_slots, B, pad):
    """off_out with offsets_stride = B + 1 and B + 7 (inline and ring): the table, untouched padding columns, the host totals"""
    with Collator(four_slots) as col:
        run = Run(col, selection_of(four_slots, 3, B, B + pad), stride=B + 1 + pad)
        run.check((B, pad))
        assert run.offsets().shape == (4, B + 1 + pad)


# ---------------------------------------------------------------------------------------------------------------------------
# empty items
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("B", [6, 70])
def test_items_of_a_slot_that_is_empty_everywhere(where, B):
    """such items have no source array (d_src = NULL), get no workgroup and write nothing; workgroup 0 belongs to the first item that
    has rows and still writes the offsets"""
    ds = R.make_dataset(41, G, [7, 5, 1], [(0, 12), (1, 1), (0, 128)], edge_items=[(0, 1, 6)], empty_slots=(2,))
    ds.ptrs.append(R.ptr_of(np.zeros(G, np.int64)))  # slot 4: an edge type no graph has
    full = ds.items
    gone_rows, gone_edges = R.RowItem(2, 8, None), R.EdgeItem(4, 2, 0, None)
    ds.items = {"first": [gone_rows] + full, "last": full + [gone_edges], "middle": full[:2] + [gone_edges, gone_rows] + full[2:]}[where]
    with Collator(ds) as col:
        for slot in (0, 3):
            run = Run(col, selection_of(ds, slot, B, B + slot))
            run.check((where, B, slot))
            assert run.totals[2] == 0 and run.totals[4] == 0 and run.totals[0] > 0


# ---------------------------------------------------------------------------------------------------------------------------
# the label filter
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignored", [25, -(1 << 63)])
@pytest.mark.parametrize("B", [7, 70])
def test_label_filter(ignored, B):
    rng = np.random.default_rng(5)
    ds = R.make_dataset(51, G, [9], [(0, 12), (0, 8), (0, 1)])
    labels, member = ds.items[1], ds.items[2]
    labels.data = np.ascontiguousarray(rng.integers(0, 25, size=labels.data.shape[0])).view(np.uint8).reshape(-1, 8)
    full = np.flatnonzero(ds.counts(0) >= 2)
    m = (rng.random(member.data.shape[0]) < 0.5).astype(np.uint8)
    p = ds.ptrs[0]
    m[p[full[0]]:p[full[0] + 1]] = 1  # a graph of members only
    m[p[full[1]]:p[full[1] + 1]] = 0  # a graph without a member
    m[p[full[2]]:p[full[2] + 1]][::2] = 1  # mixed
    m[p[full[2]] + 1:p[full[2] + 1]][::2] = 0
    member.data = m.reshape(-1, 1) * np.uint8(3)  # any non-zero byte is a member
    sel = selection_of(ds, 0, B, B)
    sel[1:4] = [int(g) for g in full[:3]]
    with Collator(ds) as col:
        col.set_filter(1, col.src[2], ignored)
        plain = ds.expected(sel)
        want = np.where(plain[2] != 0, plain[1].view(np.int64), np.int64(ignored))
        assert 0 < (want == ignored).sum() < want.size
        for _ in range(2):
            Run(col, sel, expected={1: want.view(np.uint8)}).check(("filtered", ignored))
        col.set_filter(-1, None, 0)
        Run(col, sel).check("plain copies again")


# ---------------------------------------------------------------------------------------------------------------------------
# a batch without a row
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 70])
def test_batch_in_which_no_item_has_a_row_still_writes_the_offsets(B):
    """slots 0 and 2 have items and are empty in every selected graph, slot 1 has rows and no item: no item gets a workgroup, and the
    offsets (zeros for 0 and 2, the running counts of 1) replace those of the batch before in the same buffer"""
    rng = np.random.default_rng(8)
    c0, c1 = np.array([0, 3, 0, 0, 2, 0], np.int64), np.array([4, 1, 0, 5, 2, 3], np.int64)
    ec, ei = R.random_edges(rng, np.array([0, 2, 0, 0, 3, 0], np.int64), c0, c1)
    ds = R.Dataset(6, [R.ptr_of(c0), R.ptr_of(c1), R.ptr_of(ec)],
                   [R.RowItem(0, 12, R.random_rows(rng, c0.sum(), 12)), R.RowItem(0, 1, R.random_rows(rng, c0.sum(), 1)), R.EdgeItem(2, 0, 1, ei)])
    empty_sel = [[0, 3, 5, 2, 0][b % 5] for b in range(B)]
    with Collator(ds) as col:
        before = Run(col, [[1, 4, 0, 4, 3][b % 5] for b in range(B)])
        before.check("before")
        run = Run(col, empty_sel)
        run.check("poisoned offsets")
        assert run.totals.tolist() == [0, int(c1[empty_sel].sum()), 0] and run.totals[1] > 0
        # the same selection into the offsets buffer of the batch before
        sel32 = np.asarray(empty_sel, dtype=np.int32)
        d_dst = (C.c_void_p * 3)(*[b.data_ptr() + GUARD for b in run.bufs])
        caps = (C.c_int64 * 3)(3, 3, 3)
        _lib.check(col.lib.hmp_collator_run(col.h, sel32.ctypes.data, B, d_dst, caps, run.h_totals, before.off_buf.data_ptr() + GUARD,
                                            B + 1, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(before.offsets(), to_dev(run.table))
        assert all(all_sent(b) for b in run.bufs)


def test_batch_without_a_row_on_poisoned_offsets():
    """the same through Run's own checks: a poisoned offsets buffer with padding columns"""
    ds = R.make_dataset(61, G, [5, 4], [(0, 8), (0, 2)], edge_items=[(0, 0, 3)])
    empty = np.flatnonzero((ds.counts(0) == 0) & (ds.counts(1) > 0))
    assert len(empty) >= 2
    with Collator(ds) as col:
        run = Run(col, [int(empty[0]), int(empty[1]), 0, int(empty[0])], stride=11)
        run.check()
        assert run.totals[0] == 0 and run.totals[2] == 0 and run.totals[1] > 0


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 70])
def test_refused_runs_write_nothing(four_slots, B):
    ds = four_slots
    sel = selection_of(ds, 0, B, 3)
    rich = np.flatnonzero(np.all([ds.counts(s) > 0 for s in range(4)], axis=0))  # every item has rows to be short of
    sel[1], sel[2] = int(rich[0]), int(rich[-1])
    with Collator(ds) as col:
        for bad in (-1, ds.n_graphs):
            for at in (0, B - 1):
                s = list(sel)
                s[at] = bad
                Run(col, s).check_refused()
        for short in range(len(ds.items)):
            run = Run(col, sel, short=short)
            assert run.totals[ds.items[short].slot] > 0
            run.check_refused()
        Run(col, sel, stride=B).check_refused()
        Run(col, sel).check("the collator still works")


def test_refused_filter_and_creation(four_slots):
    ds = four_slots
    with Collator(ds) as col:
        member = poisoned(int(ds.ptrs[0][-1]))
        for item in (0, 2, 4, 5, len(ds.items)):  # 1224-, 3- and 12-byte rows, an edge list, no such item
            with pytest.raises(_lib.HydraMPError, match=E_ARG):
                col.set_filter(item, member, 25)
        with pytest.raises(_lib.HydraMPError, match=E_ARG):
            col.set_filter(1, None, 25)
        Run(col, selection_of(ds, 0, 6, 1)).check("no filter was set")
    for kw in (dict(n_items=41), dict(n_slots=25)):
        with pytest.raises(_lib.HydraMPError, match=E_ARG):
            Collator(ds, **kw)
    with Collator(ds, n_items=40, n_slots=24) as col:  # the limits themselves are accepted
        assert col.h.value
