"""tests/_front_reference.py against dense algebra, and the reach of the case tables of tests/test_gpu_front_kernels.py, proved
from the constants of csrc/front.hip (no GPU)."""
import numpy as np
import pytest
import torch

import _front_reference as R

CONST = R.constants()


# ---- the reference against dense algebra ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gap", "straddle", "nsrc1+5", "n-past"])
def test_projection_reference_is_the_product_with_an_explicit_stacked_matrix(name):
    case = next(c for c in R.proj_cases() if c.name == name)
    params, (lay,) = R.lay_out_proj([case], 3)
    C, bound, live = R.proj_reference(lay, params)
    P = torch.from_numpy(params).double()
    B = torch.zeros(case.n, case.K, dtype=torch.float64)
    for (col0, rows, nsrc), offs in zip(case.segs, lay.offs):
        assert len(offs) == nsrc
        for off in offs:
            W = P[off:off + rows * case.K].reshape(rows, case.K)  # a dense [rows][K] parameter
            keep = min(rows, case.n - col0)
            B[col0:col0 + keep] += W[:keep]
    A = torch.from_numpy(np.ascontiguousarray(lay.A)).double()
    assert not torch.isnan(A).any() and not torch.isnan(B).any()
    np.testing.assert_allclose(C, (A @ B.T).numpy(), rtol=0, atol=1e-12)
    assert (bound >= np.abs(C) - 1e-12).all()
    dead = ~live
    assert (C[:, dead] == 0).all() and (bound[:, dead] == 0).all()
    if name == "gap":
        assert list(np.nonzero(dead)[0]) == [30, 31]
    if name == "n-past":
        assert list(np.nonzero(dead)[0]) == [20, 21]


def test_projection_layout_keeps_every_operand_between_guards():
    for case in R.proj_cases() + R.multi_cases():
        params, (lay,) = R.lay_out_proj([case], 1)
        assert np.isnan(params[:R.GUARD]).all() and np.isnan(params[-R.GUARD:]).all()
        live = np.zeros(params.size, bool)
        for (col0, rows, nsrc), offs in zip(case.segs, lay.offs):
            for off in offs:
                assert off % 2 == 0 and not live[off:off + rows * case.K].any()
                live[off:off + rows * case.K] = True
        assert (np.isnan(params) == ~live).all()
        a = lay.a_buf[lay.a0:lay.a0 + case.M * case.ld_a].reshape(case.M, case.ld_a)
        assert not np.isnan(a[:, :case.K]).any() and np.isnan(a[:, case.K:]).all()
        assert np.isnan(lay.a_buf[:lay.a0]).all() and np.isnan(lay.a_buf[lay.a0 + a.size:]).all()
        # as build_front forms them: sorted, disjoint segments of 1 .. FR_MAX_SRC sources
        assert 1 <= len(case.segs) <= CONST["FR_MAX_SEG"]
        end = 0
        for col0, rows, nsrc in case.segs:
            assert col0 >= end and rows >= 1 and 1 <= nsrc <= CONST["FR_MAX_SRC"]
            end = col0 + rows


def test_image_column_rule():
    cols = [R.image_col(k) for k in range(64)]
    assert sorted(cols) == list(range(64))  # a permutation inside each block of 16
    assert cols[:16] == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
    for k in range(64):
        assert cols[k] // 16 == k // 16
        assert R.image_col(cols[k]) == k  # swapping two base-4 digits twice


@pytest.mark.parametrize("table", ["sum", "heads", "attdot", "attdot_t"])
def test_pack_reference_against_dense_algebra(table):
    lay = R.lay_out_pack(R.pack_tables()[table], 5)
    refs, alone = R.pack_reference(lay)
    P = torch.from_numpy(lay.params).double()
    images = {}
    for s, d, r in zip(lay.segs, lay.desc, refs):
        assert r["own"].shape == (s.rows_pad, s.ld_dst) and not np.isnan(r["val"]).any()
        want = torch.zeros(s.rows_pad, s.ld_dst, dtype=torch.float64)
        if s.kind == R.PACK_SUM:
            for off in d["src"]:
                want[:s.rows, :s.cols] += P[off:off + s.rows * s.cols].reshape(s.rows, s.cols)
            np.testing.assert_allclose(r["exact"], want.numpy(), rtol=0, atol=s.nsrc * 2.0 ** -22)
        elif s.kind == R.PACK_HEADS:
            W = P[d["src"][0]:d["src"][0] + s.H * s.C * s.cols].reshape(s.H, s.C, s.cols)
            want[:s.H * s.Cp].reshape(s.H, s.Cp, s.ld_dst)[:, :s.C, :s.cols] = W
            assert (r["exact"].astype(np.float64) == want.numpy()).all()
        elif s.kind == R.PACK_ATTDOT:
            att = P[d["att"]:d["att"] + s.H * s.C].reshape(s.H, s.C)
            W = P[d["src"][0]:d["src"][0] + s.H * s.C * s.cols].reshape(s.H, s.C, s.cols)
            want[:s.H, :s.cols] = torch.einsum("hc,hcf->hf", att, W)
            np.testing.assert_array_less(np.abs(want.numpy()), r["bound"] / (s.C * R.U32) * 1.0000001 + 1e-300)
        else:
            att = P[d["att"]:d["att"] + s.H * s.C].reshape(s.H, s.C)
            W = P[d["src"][0]:d["src"][0] + s.H * s.C * s.rows].reshape(s.H, s.C, s.rows)
            want[:s.rows, :s.H] = torch.einsum("hc,hcd->dh", att, W)
        np.testing.assert_allclose(r["val"], want.numpy(), rtol=0, atol=1e-12)
        if s.kind in (R.PACK_SUM, R.PACK_HEADS):
            assert (r["bound"] == 0).all()
        else:
            assert ((r["bound"] > 0) == (want.numpy() != 0)).all()
        if s.img is not None:
            images.setdefault(s.img, []).append((s, d, r, want))
    # the image of a stack: a plain transpose of the stacked operand, then the digit rule on its columns
    for key, members in images.items():
        s0, d0 = members[0][0], members[0][1]
        stack = torch.zeros(s0.ld_dst_t, s0.ld_dst, dtype=torch.float64)
        for s, d, r, want in members:
            stack[s.col_t:s.col_t + s.rows_pad] = want
        plain = stack.T.numpy()  # [ld_dst][ld_dst_t]
        image = np.full(lay.n_packed, np.nan)
        for s, d, r, want in members:
            image[r["img"].ravel()] = r["val"].ravel()
            image[r["img_zero"]] = 0.0
        got = image[d0["dst_t"]:d0["dst_t"] + s0.ld_dst * s0.ld_dst_t].reshape(s0.ld_dst, s0.ld_dst_t)
        assert not np.isnan(got).any(), "the stack's segments cover the whole image"
        for k in range(s0.ld_dst_t):
            b, u, q = k // 16, k // 4 % 4, k % 4
            assert (got[:, 16 * b + 4 * q + u] == plain[:, k]).all()
    # every packed region lies between guards
    assert alone[:R.GUARD].all() and alone[-R.GUARD:].all()
    owned = sum(r[k].size for r in refs for k in ("own", "img", "img_zero") if r[k] is not None)
    assert owned == int((~alone).sum()), "no element has two owners"


# ---- what the case tables reach ---------------------------------------------------------------------------------------------
def _regimes():
    out = {}
    for case in R.proj_cases():
        params, (lay,) = R.lay_out_proj([case], 1)
        out[case.name] = (case, R.proj_regime(lay, CONST))
    return out


def test_projection_cases_reach_every_listed_path():
    c = CONST
    assert (c["FT"], c["FBK"], c["FSTAGES"], c["KG"], c["GROUPS"], c["KMIN"]) == (64, 128, 3, 32, 4, 4)
    assert c["NSRC_CASES"] == [1, 2, 3] and c["FR_MAX_SRC"] == 6 and c["FR_MAX_SEG"] == 6 and c["FR_MAX_PROB"] == 4
    reg = _regimes()
    ks = {case.K for case, _ in reg.values()}
    assert set(R.K_LIST) <= ks
    for K in R.K_LIST:
        assert c["KMIN"] <= K <= c["FSTAGES"] * c["FBK"] and K % 2 == 0
    # load width: both, and 16 bytes at K = 308 / 128 / 384; 8 bytes at K % 4 == 0 by A's address, by lda and by an offset
    assert reg["k308"][1]["vec"] == reg["k128"][1]["vec"] == reg["k384"][1]["vec"] == 4
    assert reg["k306"][1]["vec"] == reg["k306-lda308"][1]["vec"] == 2
    for n in ("k128-a8", "k128-off2", "k384-a8", "k256-lda258"):
        assert reg[n][0].K % 4 == 0 and reg[n][1]["vec"] == 2, n
    assert reg["k306-lda308"][0].ld_a == 308 and reg["k306"][0].ld_a == 306
    # stages
    assert {r["n_stage"] for _, r in reg.values()} == {1, 2, 3}
    assert {r["klen"] for _, r in reg.values()} >= {2, 32, 64, 96, 126, 128}
    assert reg["k130"][1]["klen"] == reg["k258"][1]["klen"] == 2
    # a last stage of exactly FBK columns after 0, 1 and 2 full ones; the batched form in K-groups 2 and 3 of a last stage
    for n, st in (("k128", 1), ("k256", 2), ("k384", 3)):
        assert reg[n][1]["n_stage"] == st and reg[n][1]["nk"] == [32, 32, 32, 32]
    # every K-group takes the batched (nk == 32) and the ragged (0 < nk < 32) form in some last stage, for both load widths
    for vec in (2, 4):
        for g in range(c["GROUPS"]):
            nks = {r["nk"][g] for _, r in reg.values() if r["vec"] == vec}
            assert c["KG"] in nks and 0 in nks | ({0} if g == 0 else set()), (vec, g)
    for g in range(c["GROUPS"]):
        nks = {r["nk"][g] for _, r in reg.values()}
        assert any(0 < v < c["KG"] for v in nks), g
    # sources
    assert {r["max_nsrc"] for _, r in reg.values()} == {1, 2, 3, 4, 5, 6}
    assert {r["inst"] for _, r in reg.values()} == {1, 2, 3, 6}
    for n in ("nsrc4", "nsrc5", "nsrc4-k306", "nsrc5-k308", "nsrc1+5", "nsrc5+1"):
        assert reg[n][1]["inst"] == c["FR_MAX_SRC"] > reg[n][1]["max_nsrc"], n
    assert [s[2] for s in reg["nsrc1+5"][0].segs] == [1, 5]
    # columns and rows
    assert len(reg["six-segs"][0].segs) == c["FR_MAX_SEG"]
    assert reg["straddle"][1]["tiles"][1] == 2 and any(col0 < c["FT"] < col0 + rows for col0, rows, _ in reg["straddle"][0].segs)
    assert reg["n65"][1]["tiles"][1] == 2 and reg["n1"][0].n == 1
    assert {case.M for case, _ in reg.values()} == set(R.ROWS)
    assert any(case.M == 1 for case, _ in reg.values()) and {r["tiles"][0] for _, r in reg.values()} == {1, 2, 3}
    assert any(case.ldc_pad == 4 for case, _ in reg.values()) and any(case.ldc_pad == 0 for case, _ in reg.values())


def test_multi_problem_launch_mixes_what_it_claims():
    cases = R.multi_cases()
    assert len(cases) == CONST["FR_MAX_PROB"]
    params, lays = R.lay_out_proj(cases, 1)
    regs = [R.proj_regime(lay, CONST) for lay in lays]
    assert {r["vec"] for r in regs} == {2, 4} and len({r["n_stage"] for r in regs}) == 3 and len({r["inst"] for r in regs}) >= 3
    tiles = [r["tiles"][0] * r["tiles"][1] for r in regs]
    assert tiles[1] == 1 and tiles[0] > 1 and tiles[2] > 1 and tiles[3] > 1


def test_pack_tables_hold_the_listed_cases():
    t = R.pack_tables()
    c = CONST
    sums = t["sum"]
    assert {s.nsrc for s in sums} >= {1, 2, 6} and any(s.rows < s.rows_pad for s in sums)
    assert any((s.cols, s.ld_dst) == (70, 72) for s in sums) and any((s.cols, s.ld_dst) == (6, 8) for s in sums)
    imgs = [s for s in sums if s.img is not None]
    assert imgs and any(s.img is None for s in sums)
    assert any(s.pad_t == 0 for s in imgs) and any(0 < s.pad_t < s.rows_pad for s in imgs) and any(s.pad_t > s.rows_pad for s in imgs)
    assert any(s.col_t % 16 for s in imgs)
    assert {(s.H, s.C, s.Cp) for s in t["heads"]} == {(1, 4, 4), (3, 5, 8), (4, 26, 28)}
    assert any(s.rows_pad > s.H * s.Cp for s in t["heads"])
    assert {s.C for s in t["attdot"]} == {1, 7, 8, 9, 17, 64} and {s.H for s in t["attdot"]} == {1, 4}
    assert {s.cols for s in t["attdot"]} == {6, 306}
    assert {(s.rows, s.H, s.C) for s in t["attdot_t"]} == {(d, h, cc) for d in (3, 6) for h in (1, 3, 4) for cc in (5, 16)}
    for s in t["attdot_t"]:
        assert s.rows_pad == c["GAT_MAX_EDIM"] or s.rows > c["GAT_MAX_EDIM"]
        assert s.ld_dst == c["GAT_HMAX"]
    mixed = t["mixed40"]
    assert len(mixed) == 40 <= c["SEG_MAX"] and {s.kind for s in mixed} == {0, 1, 2, 3}
    assert (c["PACK_ITEMS_LAUNCH"], c["PACK_ITEMS_FRONT"]) == (4, 16)
    for s in mixed:  # idle waves in the last block of every segment, on both routes
        assert s.items % c["PACK_ITEMS_LAUNCH"] and s.items % c["PACK_ITEMS_FRONT"]
    assert sum(s.items > c["PACK_ITEMS_FRONT"] for s in mixed) >= 3  # map entries with a first item > 0
    for table in t.values():
        for s in table:
            assert s.rows <= s.rows_pad and s.cols <= s.ld_dst and s.nsrc <= c["AGG_MAX_IN"]
