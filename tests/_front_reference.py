"""Float64 restatement of the two unit-tested roles of the small-batch front launch (csrc/front.hip) and of the stand-alone pack
(csrc/optim.hip pack_launch, csrc/device_fns.h pack_lane), with the case tables and buffer layouts of tests/test_gpu_front_kernels.py.
numpy only; shares no code with the kernels.  tests/test_front_reference.py checks it against dense algebra on the CPU and proves,
from constants read out of the sources, that the projection cases reach the paths they are named after.

Projection: C = A[:, :K] @ B.T, row c of B = sum_q params[off_q + (c - col0) * ld : ... + K] inside a segment's rows, zero elsewhere.
Pack: the four kinds of the comment block above PackSeg in csrc/kernels.h; the transposed image of a PACK_SUM segment stores element
(r, c) at row c, column col(col_t + r), where col moves the digits of k = 16 b + 4 u + q to 16 b + 4 q + u.

Every operand lives inside a NaN-filled allocation, so a read outside what the descriptors name poisons a result and a write
outside what a segment owns destroys a guard NaN."""
import os
import re
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hydra-gnn_amd", "csrc")

PACK_SUM, PACK_HEADS, PACK_ATTDOT, PACK_ATTDOT_T = range(4)
GUARD = 8   # NaN floats in front of and behind every operand
U32 = 2.0 ** -24  # unit roundoff of float32


def constants():
    """the launch geometry, read out of the sources"""
    front = open(os.path.join(CSRC, "front.hip")).read()
    kern = open(os.path.join(CSRC, "kernels.h")).read()
    net = open(os.path.join(CSRC, "net.hip")).read()
    dev = open(os.path.join(CSRC, "device_fns.h")).read()

    def const(text, name):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*([0-9 *+]+);" % name, text)
        assert m, name
        return int(eval(m.group(1), {"__builtins__": {}}))

    def one(pattern, text, what):
        found = set(re.findall(pattern, text))
        assert len(found) == 1, f"{what}: {sorted(found)}"
        return found.pop()

    out = {n: const(front, n) for n in ("FT", "FBK", "FSTAGES")}
    out.update({n: const(kern, n) for n in ("FR_MAX_PROB", "FR_MAX_SEG", "FR_MAX_SRC", "SEG_MAX", "GAT_HMAX", "GAT_MAX_EDIM", "AGG_MAX_IN")})
    a, b = one(r"const int nk = min\(max\(klen - kg \* (\d+), 0\), (\d+)\);", front, "k steps of a K-group")
    assert a == b
    out["KG"] = int(a)  # columns of a stage that one K-group multiplies
    assert one(r"const int kg = w >> (\d+),", front, "K-group of a wave") == "2" and re.search(r"__launch_bounds__\(1024\) void front_kernel", front)
    out["GROUPS"] = 1024 // 64 // 4
    assert out["GROUPS"] * out["KG"] == out["FBK"]
    assert re.search(r"if \(nk == %d\) \{" % out["KG"], front), "the batched form takes full groups only"
    cases = [int(x) for x in re.findall(r"case (\d+): front_gemm_tile<VEC, \1>", front)]
    assert re.search(r"default: front_gemm_tile<VEC, FR_MAX_SRC>", front)
    out["NSRC_CASES"] = sorted(cases)
    out["KMIN"] = int(one(r"P\.K >= (\d+) && P\.K <= FSTAGES \* FBK && \(P\.K & 1\) == 0", front, "K limits"))
    assert re.search(r"int vec = \(\(pa & 15\) == 0 && \(P\.lda & 3\) == 0\) \? 4 : 2;", front)
    assert re.search(r"if \(S\.ld & 3\) vec = 2;", front) and re.search(r"if \(S\.off\[q\] & 3\) vec = 2;", front)
    out["PACK_ITEMS_FRONT"] = int(one(r"for \(int it = 0; it < items; it \+= (\d+), \+\+nb\)", net, "items per pack block of the front launch"))
    out["PACK_ITEMS_LAUNCH"] = int(one(r"\(blk - sb\.start\[si\]\) \* (\d+) \+ \(int\)\(threadIdx\.x >> 6\)", dev, "items per block of pack_launch"))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# projection
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Proj:
    """one projection problem; segs: (col0, rows, nsrc).  a_shift: floats between a 16-byte aligned address and A; off2: the
    last source of the first segment starts at an offset = 2 mod 4 (every other block starts at a multiple of 4)"""
    name: str
    K: int
    M: int
    segs: Tuple[Tuple[int, int, int], ...]
    lda: Optional[int] = None
    N: Optional[int] = None
    ldc_pad: int = 0
    a_shift: int = 0
    off2: bool = False

    @property
    def ld_a(self):
        return self.K if self.lda is None else self.lda

    @property
    def n(self):
        return self.segs[-1][0] + self.segs[-1][1] if self.N is None else self.N

    @property
    def ldc(self):
        return self.n + self.ldc_pad


ROWS = (1, 63, 64, 65, 130)
K_LIST = (4, 6, 30, 126, 128, 130, 160, 192, 224, 254, 256, 258, 306, 308, 382, 384)
K_EXTRA = (90,)  # a last stage that ends inside K-group 2 (none of the widths above does)


def proj_cases():
    cs = []
    for i, K in enumerate(K_LIST + K_EXTRA):  # one segment of two sources, 33 columns; natural alignment: vector 4 where K % 4 == 0
        cs.append(Proj(f"k{K}", K, ROWS[i % 5], ((0, 33, 2),), ldc_pad=4 * (i & 1)))
    cs.append(Proj("k306-lda308", 306, 65, ((0, 33, 2),), lda=308))
    cs.append(Proj("k128-a8", 128, 63, ((0, 33, 2),), a_shift=2))
    cs.append(Proj("k128-off2", 128, 64, ((0, 33, 2),), off2=True))
    cs.append(Proj("k384-a8", 384, 65, ((0, 33, 2),), a_shift=2))
    cs.append(Proj("k256-lda258", 256, 1, ((0, 33, 2),), lda=258))
    for n in range(1, 7):
        cs.append(Proj(f"nsrc{n}", 30 if n & 1 else 130, ROWS[n % 5], ((0, 20, n),)))
    cs.append(Proj("nsrc4-k306", 306, 64, ((0, 20, 4),)))
    cs.append(Proj("nsrc5-k308", 308, 65, ((0, 20, 5),)))
    cs.append(Proj("nsrc1+5", 306, 63, ((0, 10, 1), (10, 12, 5))))
    cs.append(Proj("nsrc5+1", 128, 130, ((0, 10, 5), (10, 12, 1))))
    cs.append(Proj("gap", 126, 65, ((0, 30, 1), (32, 20, 2))))
    cs.append(Proj("straddle", 306, 65, ((0, 40, 1), (40, 40, 2), (80, 40, 3))))
    cs.append(Proj("six-segs", 160, 130, ((0, 8, 1), (8, 8, 2), (16, 8, 1), (24, 8, 3), (32, 8, 1), (40, 8, 2))))
    cs.append(Proj("n-past", 30, 64, ((0, 20, 2),), N=22))
    cs.append(Proj("ldc-pad", 306, 130, ((0, 70, 2),), ldc_pad=4))
    cs.append(Proj("n1", 6, 63, ((0, 1, 1),)))
    cs.append(Proj("n1-m1", 384, 1, ((0, 1, 3),)))
    cs.append(Proj("n65", 258, 65, ((0, 65, 2),)))
    return cs


def multi_cases():
    """four problems of one launch: different K, vector width, sources and tile counts; a one-tile problem between multi-tile ones"""
    return [Proj("m0", 306, 130, ((0, 40, 1), (40, 30, 2))), Proj("m1", 256, 1, ((0, 33, 1),)),
            Proj("m2", 6, 65, ((0, 40, 5),), ldc_pad=4), Proj("m3", 384, 63, ((0, 65, 3),))]


@dataclass
class ProjLayout:
    case: Proj
    a_buf: np.ndarray      # NaN-filled float32 allocation; A starts at a0
    a0: int
    c_rows: int            # rows of the C allocation behind its guard (M + 2: the rows past M must stay NaN)
    offs: list = field(default_factory=list)  # per segment: the float offsets of its sources

    @property
    def A(self):
        p = self.case
        return self.a_buf[self.a0:self.a0 + p.M * p.ld_a].reshape(p.M, p.ld_a)[:, :p.K]


def lay_out_proj(cases, seed):
    """one launch: a shared parameter buffer and one A allocation per problem.  Blocks are as build_front forms them: ld = K."""
    rng = np.random.default_rng(seed)
    blocks, cur, lays = [], GUARD, []
    for p in cases:
        a_buf = np.full(2 * GUARD + p.a_shift + p.M * p.ld_a, np.nan, np.float32)
        a0 = GUARD + p.a_shift
        a = a_buf[a0:a0 + p.M * p.ld_a].reshape(p.M, p.ld_a)
        a[:, :p.K] = rng.standard_normal((p.M, p.K), dtype=np.float32)
        lay = ProjLayout(p, a_buf, a0, p.M + 2)
        for si, (col0, rows, nsrc) in enumerate(p.segs):
            offs = []
            for q in range(nsrc):
                cur = (cur + 3) // 4 * 4
                if p.off2 and si == 0 and q == nsrc - 1:
                    cur += 2
                offs.append(cur)
                blocks.append((cur, rng.standard_normal(rows * p.K, dtype=np.float32)))
                cur += rows * p.K + 6
            lay.offs.append(offs)
        lays.append(lay)
    params = np.full(cur + GUARD, np.nan, np.float32)
    for off, v in blocks:
        params[off:off + v.size] = v
    return params, lays


def proj_regime(lay, c):
    """what front_launch and the tile make of a problem: the load width, the stages, the k steps of each K-group in the last
    stage and the source-count instantiation"""
    p = lay.case
    vec = 4 if (p.a_shift % 4 == 0 and p.ld_a % 4 == 0 and p.K % 4 == 0 and all(o % 4 == 0 for offs in lay.offs for o in offs)) else 2
    n_stage = -(-p.K // c["FBK"])
    klen = p.K - (n_stage - 1) * c["FBK"]
    nk = [min(max(klen - g * c["KG"], 0), c["KG"]) for g in range(c["GROUPS"])]
    mx = max(s[2] for s in p.segs)
    return dict(vec=vec, n_stage=n_stage, klen=klen, nk=nk, max_nsrc=mx, inst=mx if mx in c["NSRC_CASES"] else c["FR_MAX_SRC"],
                tiles=(-(-p.M // c["FT"]), -(-p.n // c["FT"])))


def proj_reference(lay, params):
    """(C, bound operand |A| @ sum_q |W_q|.T, live columns) in float64"""
    p = lay.case
    B = np.zeros((p.n, p.K))
    Babs = np.zeros((p.n, p.K))
    live = np.zeros(p.n, bool)
    for (col0, rows, nsrc), offs in zip(p.segs, lay.offs):
        for r in range(rows):
            if col0 + r >= p.n:
                break
            live[col0 + r] = True
            for off in offs:
                w = params[off + r * p.K:off + r * p.K + p.K].astype(np.float64)
                B[col0 + r] += w
                Babs[col0 + r] += np.abs(w)
    A = lay.A.astype(np.float64)
    return A @ B.T, np.abs(A) @ Babs.T, live


# ---------------------------------------------------------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------------------------------------------------------
def image_col(k):
    """column of the transposed image that holds stacked row k = 16 b + 4 u + q: 16 b + 4 q + u"""
    b, rem = divmod(k, 16)
    u, q = divmod(rem, 4)
    return 16 * b + 4 * q + u


@dataclass(frozen=True)
class Seg:
    """one pack segment without its offsets.  img: key of the transposed image it shares with the other segments of its stack"""
    kind: int
    rows: int
    rows_pad: int
    cols: int
    ld_dst: int
    nsrc: int = 1
    H: int = 0
    C: int = 0
    Cp: int = 0
    img: Optional[str] = None
    ld_dst_t: int = 0
    col_t: int = 0
    pad_t: int = 0

    @property
    def ld_src(self):  # parameters are dense: == cols, except the [H * C][edge_dim] weight of PACK_ATTDOT_T
        return self.rows if self.kind == PACK_ATTDOT_T else self.cols

    @property
    def items(self):
        return self.rows_pad * (-(-self.ld_dst // 64))


def _sum(rows, rows_pad, cols, ld_dst, nsrc, **kw):
    return Seg(PACK_SUM, rows, rows_pad, cols, ld_dst, nsrc, **kw)


def _heads(H, C, Cp, cols, ld_dst, extra=0):
    return Seg(PACK_HEADS, H * Cp, H * Cp + extra, cols, ld_dst, 1, H, C, Cp)


def _attdot(H, C, cols, ld_dst, rows_pad=None):
    return Seg(PACK_ATTDOT, H, (H + 3) // 4 * 4 if rows_pad is None else rows_pad, cols, ld_dst, 1, H, C, C)


def _attdot_t(D, H, C, rows_pad=None, ld_dst=8):
    # a net pads to GAT_MAX_EDIM = 4 rows and forms no edge dimension above it; 6 is the kernel's own range, padded to 8
    return Seg(PACK_ATTDOT_T, D, (D + 3) // 4 * 4 if rows_pad is None else rows_pad, H, ld_dst, 1, H, C, C)


def pack_tables():
    t = {}
    t["sum"] = [
        _sum(5, 8, 70, 72, 1), _sum(8, 8, 6, 8, 2), _sum(3, 4, 70, 72, 6), _sum(1, 1, 26, 28, 3),
        # stack a: two segments, the second starts at row 8 (no multiple of 16) and pads the image (pad_t == its rows_pad)
        _sum(5, 8, 70, 72, 1, img="a", ld_dst_t=16, col_t=0), _sum(3, 4, 70, 72, 2, img="a", ld_dst_t=16, col_t=8, pad_t=4),
        _sum(4, 4, 6, 8, 6, img="b", ld_dst_t=16, col_t=0, pad_t=12),    # pad_t > rows_pad
        _sum(10, 12, 70, 72, 2, img="c", ld_dst_t=16, col_t=0, pad_t=4),  # pad_t < rows_pad
        # stack d: the second segment starts at row 20, inside a block of 16
        _sum(18, 20, 6, 8, 1, img="d", ld_dst_t=32, col_t=0), _sum(7, 8, 6, 8, 2, img="d", ld_dst_t=32, col_t=20, pad_t=4),
    ]
    t["heads"] = [_heads(1, 4, 4, 6, 8), _heads(3, 5, 8, 70, 72), _heads(4, 26, 28, 6, 8), _heads(3, 5, 8, 6, 8, extra=4),
                  _heads(4, 26, 28, 70, 72, extra=4)]
    t["attdot"] = ([_attdot(1, C, 306, 308) for C in (1, 7, 8, 9, 17, 64)] + [_attdot(4, C, 6, 8) for C in (1, 7, 8, 9, 17, 64)] +
                   [_attdot(4, 9, 306, 308), _attdot(1, 17, 6, 8)])
    t["attdot_t"] = [_attdot_t(D, H, C) for D in (3, 6) for H in (1, 3, 4) for C in (5, 16)]
    # 40 small segments of mixed kinds; no item count is a multiple of 4 (idle waves in every last block of both routes)
    mixed = []
    for i in range(10):
        rp = (1, 3, 5, 7, 9, 17, 21, 1, 5, 9)[i]
        two = i % 3 == 1
        mixed.append(_sum(max(rp - (i & 1), 1), rp, 70 if two else 6, 72 if two else 8, 1 + i % 6))
        hp = (1 + i % 3) * 5 + (i & 1)  # rows_pad of the heads segment: above H * Cp in every other one
        mixed.append(Seg(PACK_HEADS, (1 + i % 3) * 5, hp + (hp % 4 == 0), 6, 8, 1, 1 + i % 3, 3 + (i & 1), 5))
        mixed.append(_attdot(1 + i % 4, (1, 7, 8, 9, 17)[i % 5], 70 if i & 1 else 6, 72 if i & 1 else 8, rows_pad=5 if i & 1 else 7))
        mixed.append(_attdot_t(3 if i & 1 else 6, 1 + i % 4, 5 if i & 2 else 16, rows_pad=6 if i & 1 else 7))
    t["mixed40"] = mixed
    return t


@dataclass
class PackLayout:
    segs: list             # Seg
    desc: list             # per segment: dict(dst, att, src[list], dst_t)
    params: np.ndarray
    n_packed: int


def lay_out_pack(segs, seed):
    """parameter blocks and packed regions of a table, each between NaN guards; a stack's segments share one image"""
    rng = np.random.default_rng(seed)
    blocks, cur, pk, desc, images = [], GUARD, GUARD, [], {}

    def block(n):
        nonlocal cur
        off = cur
        blocks.append((off, rng.standard_normal(n, dtype=np.float32)))
        cur += n + 5
        return off

    for s in segs:
        d = dict(att=0, dst_t=0)
        if s.kind == PACK_SUM:
            d["src"] = [block(s.rows * s.cols) for _ in range(s.nsrc)]
        else:
            if s.kind != PACK_HEADS:
                d["att"] = block(s.H * s.C)
            d["src"] = [block(s.H * s.C * s.ld_src)]
        d["dst"] = pk
        pk += s.rows_pad * s.ld_dst + GUARD
        if s.img is not None:
            if s.img not in images:
                images[s.img] = pk
                pk += s.ld_dst * s.ld_dst_t + GUARD
            d["dst_t"] = images[s.img]
        desc.append(d)
    params = np.full(cur + GUARD, np.nan, np.float32)
    for off, v in blocks:
        params[off:off + v.size] = v
    return PackLayout(list(segs), desc, params, pk)


def pack_segment_reference(s, d, params):
    """what one segment leaves behind:
      own     flat indices [rows_pad][ld_dst] of the block it writes (all of it)
      val     float64 values there; bound: 0 where the value is exact, else gamma_C * sum_c |a_c w_c|
      exact   float32 values where the kernel has no freedom (PACK_SUM: the left-to-right float32 sum; PACK_HEADS: a copy), else None
      img     flat indices, same shape, of each element's copy in the transposed image (None without image)
      img_zero  flat indices of the image's padding this segment zeroes"""
    R, L = s.rows_pad, s.ld_dst
    own = d["dst"] + np.arange(R)[:, None] * L + np.arange(L)[None, :]
    val = np.zeros((R, L))
    bound = np.zeros((R, L))
    exact = None

    def mat(off, rows, ld, cols):
        return np.stack([params[off + r * ld:off + r * ld + cols] for r in range(rows)]) if rows else np.zeros((0, cols), np.float32)

    if s.kind == PACK_SUM:
        acc = np.zeros((s.rows, s.cols), np.float32)
        for off in d["src"][:s.nsrc]:
            acc = (acc + mat(off, s.rows, s.ld_src, s.cols)).astype(np.float32)
            val[:s.rows, :s.cols] += mat(off, s.rows, s.ld_src, s.cols).astype(np.float64)
        exact = np.zeros((R, L), np.float32)
        exact[:s.rows, :s.cols] = acc
    elif s.kind == PACK_HEADS:
        W = mat(d["src"][0], s.H * s.C, s.ld_src, s.cols)
        exact = np.zeros((R, L), np.float32)
        for h in range(s.H):
            for c in range(s.C):
                exact[h * s.Cp + c, :s.cols] = W[h * s.C + c]
        val = exact.astype(np.float64)
    else:
        gamma = s.C * U32 / (1 - s.C * U32)
        att = params[d["att"]:d["att"] + s.H * s.C].astype(np.float64)
        width = s.cols if s.kind == PACK_ATTDOT else s.rows
        W = mat(d["src"][0], s.H * s.C, s.ld_src, width).astype(np.float64)
        for h in range(s.H):
            terms = att[h * s.C:(h + 1) * s.C, None] * W[h * s.C:(h + 1) * s.C]  # [C][width]
            if s.kind == PACK_ATTDOT:
                val[h, :width] = terms.sum(0)
                bound[h, :width] = gamma * np.abs(terms).sum(0)
            else:
                val[:width, h] = terms.sum(0)
                bound[:width, h] = gamma * np.abs(terms).sum(0)
    img = img_zero = None
    if s.ld_dst_t > 0:
        cols = np.array([image_col(s.col_t + r) for r in range(R)])
        img = d["dst_t"] + np.arange(L)[None, :] * s.ld_dst_t + cols[:, None]
        pad = np.array([image_col(s.col_t + R + p) for p in range(s.pad_t)], dtype=np.int64)
        img_zero = (d["dst_t"] + np.arange(L)[:, None] * s.ld_dst_t + pad[None, :]).ravel()
    return dict(own=own, val=val, bound=bound, exact=exact, img=img, img_zero=img_zero)


def pack_reference(lay):
    """per-segment references and the mask of the packed buffer that no segment may touch"""
    refs = [pack_segment_reference(s, d, lay.params) for s, d in zip(lay.segs, lay.desc)]
    alone = np.ones(lay.n_packed, bool)
    for r in refs:
        for k in ("own", "img", "img_zero"):
            if r[k] is not None and r[k].size:
                assert r[k].min() >= 0 and r[k].max() < lay.n_packed
                alone[r[k].ravel()] = False
    return refs, alone
