"""The float64 reference of tests/_tail_reference.py against torch.nn.functional (cross_entropy, linear) and torch.argmax on small
random cases, so that the reference the GPU tests trust is not wrong in the same way as a kernel: the formulas here are written
a second time, row by row, with the library's own operators."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _tail_reference import (ACT_ELU, ACT_NONE, ACT_RELU, head_members, linear_heads_reference, pool_csr_csc, tail_reference,
                             within, yardstick)

IGN = 7
ACTS = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_ELU: F.elu}


def _case(n, width, seed, p):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, width + 3, generator=g, dtype=torch.float64)
    z[torch.rand(n, width + 3, generator=g) < 0.1] = 0.0
    keep = (torch.rand(n, width + 3, generator=g) >= p).to(torch.uint8)
    return g, z, keep


def _labels(g, n, classes):
    lab = torch.randint(0, classes, (n,), generator=g)
    if n > 4:
        lab[1] = IGN
        lab[2] = -3
        lab[3] = classes
    mask = torch.rand(n, generator=g) < 0.8
    return lab, mask


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_ELU])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("classes", [1, 5, 9])
def test_tail_reference_unpooled(classes, p, act):
    n = 23
    g, z, keep = _case(n, classes, 100 * classes + act, p)
    lab, mask = _labels(g, n, classes)
    r = tail_reference(z, classes, act, keep, p, lab, mask, IGN)
    zl = z[:, :classes].clone().requires_grad_(True)
    y = ACTS[act](zl) * (keep[:, :classes].double() / (1 - p) if p > 0 else 1.0)
    use = mask & (lab != IGN) & (lab >= 0) & (lab < classes)
    per_row = F.cross_entropy(y, lab.clamp(0, classes - 1), reduction="none")
    (per_row * use).sum().backward()
    torch.testing.assert_close(r["loss"], (per_row * use).sum().detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["row_loss"], (per_row * use).detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["row_valid"], use.double())
    torch.testing.assert_close(r["dz"], zl.grad, rtol=1e-12, atol=1e-12)
    assert r["bad"] == int(mask[2]) + int(mask[3])
    pred = torch.argmax(y.detach(), dim=1)
    # torch.argmax returns the first maximum on the CPU; ties exist (ReLU zeros, dropped columns)
    assert torch.equal(r["pred"], pred)
    assert r["total"] == int(mask.sum()) and r["correct"] == int((mask & (pred == lab)).sum())


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_ELU])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_tail_reference_pooled_with_empty_rows_and_shared_leaves(p, act):
    classes, n_leaves, n_pool = 6, 11, 7
    g, z, keep = _case(n_leaves, classes, 31 + act, p)
    # pooled row 0: three leaves, 1: one leaf, 2: EMPTY, 3: two leaves (leaf 4 a second time), 4: EMPTY, 5: leaf 4 again, 6: one leaf;
    # leaves 8 .. 10 have no pool edge
    edges = [(0, 0), (4, 3), (1, 0), (2, 1), (5, 3), (3, 0), (4, 5), (6, 6), (4, 0)]
    rowptr, col, t_rowptr, t_col = pool_csr_csc(n_pool, n_leaves, edges)
    assert rowptr.tolist() == [0, 4, 5, 5, 7, 7, 8, 9] and col.tolist() == [0, 1, 3, 4, 2, 4, 5, 4, 6]
    assert t_rowptr.tolist() == [0, 1, 2, 3, 4, 7, 8, 9, 9, 9, 9, 9] and t_col.tolist() == [0, 0, 1, 0, 3, 5, 0, 3, 6]
    lab, mask = _labels(g, n_pool, classes)
    lab[4] = 2  # an empty row that counts: its logits are all 0
    mask[4] = True
    r = tail_reference(z, classes, act, keep, p, lab, mask, IGN, pool=(rowptr, col))
    zl = z[:, :classes].clone().requires_grad_(True)
    y = ACTS[act](zl) * (keep[:, :classes].double() / (1 - p) if p > 0 else 1.0)
    rows = []
    for v in range(n_pool):  # the mean, row by row
        leaves = [leaf for leaf, row in edges if row == v]
        rows.append(torch.stack([y[leaf] for leaf in leaves]).mean(dim=0) if leaves else torch.zeros(classes, dtype=torch.float64))
    rows = torch.stack(rows)
    use = mask & (lab != IGN) & (lab >= 0) & (lab < classes)
    loss = F.cross_entropy(rows[use], lab[use], reduction="sum")
    loss.backward()
    torch.testing.assert_close(r["loss"], loss.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["dz"], zl.grad, rtol=1e-12, atol=1e-12)
    assert float(r["dz"][8:].abs().max()) == 0.0  # leaves without a pool edge
    torch.testing.assert_close(r["row_loss"][4], torch.log(torch.tensor(float(classes), dtype=torch.float64)))
    assert int(r["pred"][2]) == 0 and int(r["pred"][4]) == 0  # an empty row predicts 0
    assert torch.equal(r["pred"], torch.argmax(rows.detach(), dim=1))
    assert r["total"] == int(mask.sum()) and r["correct"] == int((mask & (r["pred"] == lab)).sum())


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_ELU])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("members", ["both_null", "second_null", "both_given"])
def test_linear_heads_reference(members, p, act):
    n, Fw, C0, C1 = 29, 10, 4, 6
    g, z, keep = _case(n, Fw, 77 + act, p)
    W = [torch.randn(C, Fw, generator=g, dtype=torch.float64) for C in (C0, C1)]
    b = [torch.randn(C, generator=g, dtype=torch.float64) for C in (C0, C1)]
    lab = torch.randint(0, C0, (n,), generator=g)
    lab[1], lab[2], lab[3] = IGN, -1, C0  # C0 is a valid label of head 1 and an invalid one of head 0
    mask = torch.rand(n, generator=g) < 0.8
    mask[:8] = True
    m0 = m1 = None
    if members != "both_null":
        m0 = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
    if members == "both_given":
        m1 = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
        m0[4], m1[4] = 1, 1  # a row in both heads
        m0[5], m1[5] = 0, 0  # a row in neither
        m0[3], m1[3] = 1, 1
    r = linear_heads_reference(z, Fw, W[0], b[0], W[1], b[1], act, keep, p, lab, mask, m0, m1, IGN)
    mem = head_members(n, m0, m1)
    if members == "both_null":
        assert bool(mem[0].all()) and not bool(mem[1].any())
    if members == "second_null":
        assert torch.equal(mem[1], ~mem[0])
    zl = z[:, :Fw].clone().requires_grad_(True)
    Wl = [w.clone().requires_grad_(True) for w in W]
    bl = [x.clone().requires_grad_(True) for x in b]
    y = ACTS[act](zl) * (keep[:, :Fw].double() / (1 - p) if p > 0 else 1.0)
    total, row_valid, bad = 0.0, torch.zeros(n, dtype=torch.float64), 0
    for h, C in enumerate((C0, C1)):
        logits = F.linear(y, Wl[h], bl[h])
        live = mem[h] & mask & (lab != IGN)
        use = live & (lab >= 0) & (lab < C)
        bad += int((live & ~use).sum())
        if bool(use.any()):
            total = total + F.cross_entropy(logits[use], lab[use], reduction="sum")
        row_valid += use.double()
        pred = torch.argmax(logits.detach(), dim=1)
        counted = mem[h] & mask
        assert r["total"][h] == int(counted.sum()) and r["correct"][h] == int((counted & (pred == lab)).sum())
    total.backward()
    assert r["bad"] == bad
    torch.testing.assert_close(r["loss"], total.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["row_loss"].sum(), total.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["row_valid"], row_valid)
    torch.testing.assert_close(r["dz"], zl.grad, rtol=1e-12, atol=1e-12)
    for h in range(2):
        want_w = Wl[h].grad if Wl[h].grad is not None else torch.zeros_like(W[h])
        want_b = bl[h].grad if bl[h].grad is not None else torch.zeros_like(b[h])
        torch.testing.assert_close(r["dW"][h], want_w, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(r["db"][h], want_b, rtol=1e-12, atol=1e-12)
    if members == "both_given":
        assert float(r["row_valid"][4]) == 2.0 and float(r["row_valid"][5]) == 0.0 and float(r["dz"][5].abs().max()) == 0.0
        assert float(r["row_valid"][3]) == 1.0 and r["bad"] >= 1  # label C0: head 1 takes it, head 0 reports it
    if members == "both_null":
        assert float(r["dW"][1].abs().max()) == 0.0 and float(r["db"][1].abs().max()) == 0.0


def test_first_maximum_on_ties():
    z = torch.tensor([[1.0, 3.0, 3.0, 2.0], [-1.0, -2.0, 5.0, 5.0], [0.0, -0.0, 0.0, -1.0]], dtype=torch.float64)
    r = tail_reference(z, 4, ACT_NONE, None, 0.0, torch.tensor([1, 3, 0]), None, IGN)
    assert r["pred"].tolist() == [1, 2, 0] and r["correct"] == 2 and r["total"] == 3
    assert r["gap"].tolist() == [0.0, 0.0, 0.0]
    r = tail_reference(z, 4, ACT_RELU, None, 0.0, torch.tensor([1, 3, 0]), None, IGN)  # ReLU makes row 2 an all-zero tie
    assert r["pred"].tolist() == [1, 2, 0]


def test_float32_yardstick_and_within():
    g, z, keep = _case(200, 40, 5, 0.25)
    lab, mask = _labels(g, 200, 40)
    r64 = tail_reference(z.float(), 40, ACT_ELU, keep, 0.25, lab, mask, IGN)
    r32 = tail_reference(z.float(), 40, ACT_ELU, keep, 0.25, lab, mask, IGN, dtype=torch.float32)
    assert r32["dz"].dtype == torch.float32
    yard = yardstick(r32["dz"], r64["dz"])
    assert 0 < yard[0] < 1e-5 and 0 < yard[1] < 1e-3
    assert within(r32["dz"], r64["dz"], yard)[0]  # the yardstick passes its own bar
    wrong = r64["dz"].clone()
    wrong[17, 3] += 1e-4
    ok, msg = within(wrong, r64["dz"], yard)
    assert not ok and "1 of" in msg
    nan = r64["dz"].clone()
    nan[0, 0] = float("nan")
    assert not within(nan, r64["dz"], yard)[0]
    assert within(r64["dz"], r64["dz"], (0.0, 0.0))[0]
    assert np.isclose(yardstick(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.5], dtype=torch.float64))[1], 0.2)


def test_signed_sums_are_held_to_the_absolute_yardstick_only():
    g = torch.Generator().manual_seed(9)
    ref = torch.randn(64, 64, generator=g, dtype=torch.float64)
    ref[3, 3] = 2e-5  # a nearly cancelled element
    f32 = ref + 1e-6 * torch.randn(64, 64, generator=g, dtype=torch.float64)
    f32[3, 3] = ref[3, 3] + 1e-8
    yard = yardstick(f32, ref)
    got = ref.clone()
    got[3, 3] += 2e-6  # an absolute error like every other element's, a relative error of 10 %
    assert not within(got, ref, yard)[0] and within(got, ref, yard, signed_sum=True)[0]
    got[5, 5] += 5 * yard[0]
    assert not within(got, ref, yard, signed_sum=True)[0]
