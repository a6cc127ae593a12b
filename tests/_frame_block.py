"""The numpy execution of a frame pipeline staging block, shared by the host tests (tests/test_frame_*host*.py): what the one launch
of ``hmp_frame_expand`` / ``hmp_frame_expand_batch`` is specified to write, item by item, for single frames and batches in every
mode.  ``expand`` executes every item kind once; ``views`` reads the result through the product's tensor table
(``dsg._TENSOR_TABLES``), so a comparison must take its EXPECTED tensors from the oracle object's own attributes, never from the
table.  Which kinds a mode may hold is the calling test's assertion (``check_kinds``).  Host tests only: ``run_frame_check`` builds
and runs the stand-alone sanitized driver."""
import os
import subprocess

import numpy as np

from hydra_gnn_amd import _lib, dsg

INT_MAX = 0x7FFFFFFF
TYPED_KINDS = {_lib.FK_FEAT, _lib.FK_POS, _lib.FK_I64, _lib.FK_EDGE, _lib.FK_EATTR, _lib.FK_CLIQUE}  # a typed single frame
HOMOG_KINDS = {_lib.FK_FEAT, _lib.FK_EATTR, _lib.FK_CLIQUE, _lib.FK_EDGE_SEG, _lib.FK_CONST}  # a homogeneous single frame
BATCH_KINDS = HOMOG_KINDS | {_lib.FK_POS, _lib.FK_I64}  # a batch holds no plain EDGE item
HTREL_KINDS = {_lib.FK_FEAT, _lib.FK_POS, _lib.FK_I64, _lib.FK_EDGE, _lib.FK_CLIQUE, _lib.FK_EDGE_SEG, _lib.FK_CONST, _lib.FK_EATTR_HT}  # no plain EATTR item


def check_kinds(items, allowed):
    kinds = set(items[:, _lib.FI_KIND].tolist())
    assert kinds <= allowed, sorted(kinds - allowed)


def check_typed_frame(items):
    """a typed single frame holds the six kinds of TYPED_KINDS, and a feature row is exactly as wide as its own columns (no padding)"""
    check_kinds(items, TYPED_KINDS)
    feat = items[items[:, _lib.FI_KIND] == _lib.FK_FEAT]
    assert (feat[:, _lib.FI_WIDTH] == feat[:, _lib.FI_P0] + 3 + feat[:, _lib.FI_P1]).all()


def section(block, off, dtype, count):
    """``count`` elements of ``dtype`` at byte ``off`` of the block: the only place that reads it"""
    nbytes = count * np.dtype(dtype).itemsize
    assert off >= 0 and off % 16 == 0 and off + nbytes <= block.size, (off, count, block.size)
    return block[off:off + nbytes].view(dtype)


def put(arena, written, dst, values):
    """``values`` at arena byte ``dst``: inside the arena, at a multiple of the element size, no byte written twice"""
    raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
    assert dst >= 0 and dst % values.dtype.itemsize == 0 and dst + raw.size <= arena.size, (dst, raw.size, arena.size)
    assert not written[dst:dst + raw.size].any()
    arena[dst:dst + raw.size] = raw
    written[dst:dst + raw.size] = True
    return written


def _ends(e, variant, n, col):
    if variant == 0:
        return e[col], e[n + col]
    if variant == 1:
        return (e[col], e[n + col]) if col < n else (e[col], e[col - n])
    if variant == 2:
        return e[n + col], e[col]
    return (e[col], col) if variant == 3 else (col, e[col])


def _edge_ends(block, s0, p0, p1, n_out):
    """int64 [n_out, 2]: (source, destination) of the first ``n_out`` columns of an edge section in variant ``p0``"""
    e = section(block, s0, np.int32, (2 if p0 <= 2 else 1) * p1)
    return np.array([_ends(e, p0, p1, c) for c in range(n_out)], dtype=np.int64).reshape(-1, 2)


def _clique_mean(ptr, mem, rpos, q):
    s = np.zeros(3, dtype=np.float32)
    for k in mem[ptr[q]:ptr[q + 1]]:  # ascending member order, float32
        s = s + rpos[k]
    return s / np.float32(max(int(ptr[q + 1] - ptr[q]), 1))


def _end_pos(block, desc, words, idx):
    """float32 [len(idx), 3]: the positions of nodes ``idx`` of one end of an EATTR_HT item (words = mode, pos, index / ptr, members:
    byte offsets relative to the descriptor at ``desc``)"""
    mode, r_pos, r_a, r_b = words
    if idx.size == 0:
        return np.zeros((0, 3), dtype=np.float32)
    assert r_pos != 0
    top = int(idx.max()) + 1
    if mode == _lib.FE_CLIQUE:
        assert r_a != 0 and r_b != 0
        ptr = section(block, desc + r_a, np.int32, top + 1)
        assert (np.diff(ptr) >= 0).all() and ptr[0] >= 0
        mem = section(block, desc + r_b, np.int32, int(ptr[-1]))
        rpos = section(block, desc + r_pos, np.float64, 3 * (int(mem.max()) + 1 if mem.size else 0)).reshape(-1, 3).astype(np.float32)
        mean = np.zeros((top, 3), dtype=np.float32)
        for q in np.unique(idx).tolist():
            mean[q] = _clique_mean(ptr, mem, rpos, q)
        return mean[idx]
    if mode == _lib.FE_GATHER:
        assert r_a != 0
        idx = section(block, desc + r_a, np.int32, top)[idx]
        assert idx.min() >= 0
    else:
        assert mode == _lib.FE_DIRECT
    return section(block, desc + r_pos, np.float64, 3 * (int(idx.max()) + 1)).reshape(-1, 3)[idx].astype(np.float32)


def _eattr_ht(block, item):
    kind, tensor, rows, width, dst, s0, s1, s2, s3, p0, p1, _ = item
    assert width == 3 and rows == p1 and s2 == -1 and s3 == -1
    if p0 == 0:  # as given
        e = section(block, s0, np.int32, 2 * p1)
        src, dst_ = e[:p1].astype(np.int64), e[p1:].astype(np.int64)
    else:  # (k, v[k])
        assert p0 == 4
        src, dst_ = np.arange(p1, dtype=np.int64), section(block, s0, np.int32, p1).astype(np.int64)
    assert (src >= 0).all() and (dst_ >= 0).all()
    d = section(block, s1, np.int32, 2 * _lib.FRAME_END_WORDS).tolist()
    return _end_pos(block, s1, d[_lib.FRAME_END_WORDS:], dst_) - _end_pos(block, s1, d[:_lib.FRAME_END_WORDS], src)


def expand(block, items, arena_bytes, table=None):
    """The arena (uint8) a launch over this block is specified to write, and the mask of written bytes.  Every section read is checked
    to lie inside the block and to be 16-byte aligned (``section``), every write to lie inside the arena at a multiple of its element
    size, and no byte is written twice (``put``).  ``table``: the semantic table of FEAT items with a semantic block."""
    arena = np.zeros(arena_bytes, dtype=np.uint8)
    written = np.zeros(arena_bytes, dtype=bool)
    for item in items.tolist():
        kind, tensor, rows, width, dst, s0, s1, s2, s3, p0, p1, _ = item
        if kind in (_lib.FK_FEAT, _lib.FK_POS, _lib.FK_I64):  # rows gathered through the index section S3 (none: in order)
            idx = section(block, s3, np.int32, rows) if s3 >= 0 else np.arange(rows, dtype=np.int32)
            n_src = int(idx.max()) + 1 if rows else 0
        else:  # no other kind gathers; an edge segment's S3 is its destination shift
            assert s3 == -1 or kind == _lib.FK_EDGE_SEG, item
        if kind == _lib.FK_FEAT:  # [position if P0 | size | table row if P1], zeros behind the type's own columns
            cols = [section(block, s0, np.float64, 3 * n_src).reshape(-1, 3)[idx]] if p0 else []
            cols.append(section(block, s1, np.float64, 3 * n_src).reshape(-1, 3)[idx])
            own = np.concatenate(cols, 1).astype(np.float32)
            if p1:
                own = np.concatenate([own, table[section(block, s2, np.int32, n_src)[idx]]], 1)
            assert own.shape == (rows, p0 + 3 + p1) and own.shape[1] <= width
            x = np.zeros((rows, width), dtype=np.float32)
            x[:, :own.shape[1]] = own
            put(arena, written, dst, x)
        elif kind == _lib.FK_POS:
            put(arena, written, dst, section(block, s0, np.float64, 3 * n_src).reshape(-1, 3)[idx].astype(np.float32))
        elif kind == _lib.FK_I64:
            put(arena, written, dst, section(block, s0, np.int32 if p0 == 4 else np.int64, n_src)[idx].astype(np.int64))
        elif kind in (_lib.FK_EDGE, _lib.FK_EDGE_SEG):  # a segment: its columns at pitch S1, shifted by S2 / S3
            ends = _edge_ends(block, s0, p0, p1, width)
            pitch, shift = (s1, (s2, s3)) if kind == _lib.FK_EDGE_SEG else (width, (0, 0))
            assert 0 <= width <= pitch
            put(arena, written, dst, ends[:, 0] + shift[0])
            put(arena, written, dst + 8 * pitch, ends[:, 1] + shift[1])
        elif kind == _lib.FK_EATTR:
            ends = _edge_ends(block, s0, p0, p1, rows)
            ps = section(block, s1, np.float64, 3 * (int(ends[:, 0].max()) + 1 if rows else 0)).reshape(-1, 3).astype(np.float32)
            pd = section(block, s2, np.float64, 3 * (int(ends[:, 1].max()) + 1 if rows else 0)).reshape(-1, 3).astype(np.float32)
            put(arena, written, dst, pd[ends[:, 1]] - ps[ends[:, 0]])
        elif kind == _lib.FK_EATTR_HT:
            put(arena, written, dst, _eattr_ht(block, item))
        elif kind == _lib.FK_CLIQUE:  # [mean of the member rooms' positions | zeros] without its first P0 columns
            assert p0 in (0, 3)
            ptr = section(block, s0, np.int32, rows + 1)
            mem = section(block, s1, np.int32, int(ptr[-1]))
            rpos = section(block, s2, np.float64, 3 * (int(mem.max()) + 1 if mem.size else 0)).reshape(-1, 3).astype(np.float32)
            x = np.zeros((rows, width + p0), dtype=np.float32)
            for q in range(rows):
                x[q, :3] = _clique_mean(ptr, mem, rpos, q)
            put(arena, written, dst, x[:, p0:])
        elif kind == _lib.FK_CONST:
            assert p1 in (1, 8)
            put(arena, written, dst, np.full(rows, p0, dtype=np.int64 if p1 == 8 else np.uint8))
        else:
            raise AssertionError(f"unknown item kind {kind}")
    return arena, written


def item_blocks(item):
    """workgroups of an item, from its own words (the rule of csrc/frame.cpp)"""
    kind, rows, width = item[_lib.FI_KIND], item[_lib.FI_ROWS], item[_lib.FI_WIDTH]
    if kind == _lib.FK_FEAT and width >= 32:
        return -(-rows // 4)
    if kind in (_lib.FK_EDGE, _lib.FK_EDGE_SEG):
        return -(-2 * width // 256)
    if kind in (_lib.FK_I64, _lib.FK_CONST):
        return -(-rows // 256)
    return -(-rows * (3 if kind in (_lib.FK_POS, _lib.FK_EATTR, _lib.FK_EATTR_HT) else width) // 256)


def check_prefix(items, n_blocks):
    """the workgroup prefix words are the running sum of the items' workgroups; returns the workgroups per item"""
    blocks = np.array([item_blocks(it) for it in items.tolist()])
    assert np.array_equal(items[:, _lib.FI_BLOCK0], np.concatenate([[0], np.cumsum(blocks)[:-1]])) and blocks.sum() == n_blocks
    return blocks


def lookup(groups, items, n_items, block):
    """the kernel's two-level item lookup for workgroup ``block``: two 64-lane loads, two ballots; tail lanes read INT_MAX"""
    lanes = np.arange(64)
    g0 = np.where(lanes < groups.size, groups[np.minimum(lanes, groups.size - 1)], INT_MAX)
    gi = int((g0 <= block).sum()) - 1
    assert gi >= 0 and bool(np.all((g0 <= block)[: gi + 1]))  # the ballot is a prefix: popcount - 1 is the last set lane
    it = gi * 64 + lanes
    b0 = np.where(it < n_items, items[np.minimum(it, n_items - 1), _lib.FI_BLOCK0], INT_MAX)
    hit = b0 <= block
    assert bool(np.all(hit[: int(hit.sum())]))
    return gi * 64 + int(hit.sum()) - 1


def tensor_rows(items):
    """The item table of a SINGLE frame as the rows of a batch's tensor table, ``[tensor, arena byte, rows, width]``: a tensor starts
    where its first item does, its segments' rows add up, and every segment carries the pitch of the whole (an edge segment in S1)"""
    geo = {}
    for kind, tensor, rows, width, dst, _, s1, *_ in items.tolist():
        pitch = s1 if kind == _lib.FK_EDGE_SEG else width
        row = geo.setdefault(tensor, [tensor, dst, 0, pitch])
        assert row[3] == pitch, "one pitch per tensor"
        row[2] += rows if kind != _lib.FK_EDGE_SEG else 0
    return list(geo.values())


def _extents(rows, htree, homogeneous):
    """(store key or None, attribute, arena byte, numpy dtype, shape) of every tensor ``rows`` lists, by the product's tensor table"""
    table = dsg._TENSOR_TABLES[bool(htree), bool(homogeneous)]
    layout = {dsg._F32: lambda n, w: (np.float32, (n, w)), dsg._EDGE: lambda n, w: (np.int64, (2, w)),
              dsg._I64: lambda n, w: (np.int64, (n,)), dsg._BOOL: lambda n, w: (np.bool_, (n,))}
    for t, dst, n, w in np.asarray(rows).reshape(-1, 4).tolist():
        key, attr, cls = table[t]
        assert cls in layout, (t, key, attr)  # a number the mode defines
        yield (key, attr, dst) + layout[cls](n, w)


def views(arena, rows, htree, homogeneous):
    """{(store key or None, attribute): array} of the tensors ``rows`` lists (a batch's tensor table, or ``tensor_rows`` of a single
    frame), read from an arena through the product's tensor table; every tensor starts 16-byte aligned and has a name of its own"""
    out = {}
    for key, attr, dst, dtype, shape in _extents(rows, htree, homogeneous):
        assert dst % 16 == 0 and (key, attr) not in out, (dst, key, attr)
        out[(key, attr)] = arena[dst:dst + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
    return out


def covered(arena_bytes, rows, htree, homogeneous):
    """mask of the arena bytes that belong to a tensor of ``rows``"""
    mask = np.zeros(arena_bytes, dtype=bool)
    for _, _, dst, dtype, shape in _extents(rows, htree, homogeneous):
        mask[dst:dst + int(np.prod(shape)) * np.dtype(dtype).itemsize] = True
    return mask


def run_frame_check(args):
    """`make frame_check` (csrc/frame_check.cpp: frame.cpp + htree.cpp + a program with its own main under
    -fsanitize=address,undefined; CPU only, the runtimes linked statically, nothing preloaded, nothing loaded into Python), run with
    ``args``; asserts a clean exit and returns what it printed"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydra-gnn_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "frame_check"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(csrc, "build", "frame_check")] + list(args), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "FRAME-CHECK-OK" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout
