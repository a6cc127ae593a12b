"""The dropout generator on the device against the numpy restatement (tests/_dropout_reference.py, written from the generator's
statement in include/hydra_mp.h and tied to the host side of csrc/common.h bit for bit by tests/test_dropout_reference.py).

Every training-mode parity test replays the engine's masks through hmp_dropout_mask, which proves that the draw sites agree with
the export; here the export itself, and one draw site directly, are compared with the restatement:
  * hmp_dropout_mask == keep_mask, torch.equal, at single-quad, ragged (F % 4 != 0), multi-block and grid-stride shapes (the launch
    has at most 2048 x 256 threads, one per quad: [8200, 256] is 524 800 quads), for every p of the CPU test's list and seeds, steps
    and streams at the ends of their ranges; the bytes behind each mask stay as they were; empty shapes write nothing;
  * hmp_bias_act_drop_fwd (csrc/homog.hip, the homogeneous models' epilogue) on x = 1 with ReLU and row pitches above F: y != 0 is
    the restatement's mask, kept values are 1.f / (1.f - p) exactly, dropped ones -0.0, the pitch gap and the bytes behind y
    untouched; [16390, 258] (1 065 350 quads) passes that launch's 4096 x 256 threads;
  * masks of seeds s and s + 2^32 differ in every quad element.
"""
import numpy as np
import pytest
import torch

import _dropout_reference as ref

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 0xA5
N_GUARD = 64

P_LIST = [0.0, 1e-6, 2.0**-16, 1.5 * 2.0**-16, np.float32(0.1), 0.25, 0.3, 0.5, 0.999, np.nextafter(np.float32(1), np.float32(0))]
# (seed, step, stream): small, zero, a seed of high word 1, a model-sized seed with the largest step, the largest seed and stream
TRIPLES = [(1234, 1, 3), (0, 0, 0), (2**32, 1, 8), (2**61 + 5, 2**32 - 1, 71), (2**64 - 1, 7, 2**32 - 1)]


def device_mask(seed, step, stream, p, n, F) -> torch.Tensor:
    """hmp_dropout_mask into a guard-filled buffer: the whole buffer, [n * F + N_GUARD] uint8, on the host"""
    lib = _lib.require_device()
    buf = torch.full((n * F + N_GUARD,), GUARD, dtype=torch.uint8, device=DEV)
    _lib.check(lib.hmp_dropout_mask(seed, step, stream, float(p), n, F, buf.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("n,F", [(1, 1), (3, 5), (7, 4), (33, 130), (129, 306), (8200, 256)])
def test_export_equals_restatement(n, F):
    qpr = (F + 3) >> 2
    q = np.arange(n * qpr, dtype=np.int64)
    for seed, step, stream in TRIPLES:
        draws = ref.draws(seed, step, stream, q).reshape(n, qpr * 4)[:, :F]  # the draws do not depend on p
        for p in P_LIST:
            want = draws >= np.uint32(ref.thresh(p) >> 16)
            got = device_mask(seed, step, stream, p, n, F)
            assert torch.all(got[n * F:] == GUARD), (seed, step, stream, float(p))
            assert torch.equal(got[:n * F].view(n, F), torch.from_numpy(want.astype(np.uint8))), (seed, step, stream, float(p))
    # the vectorised path above is the restatement's own keep_mask
    assert np.array_equal(want, ref.keep_mask(seed, step, stream, p, n, F))


def test_thresholds_on_the_device():
    """p below 2^-16 drops nothing; the float below 1 keeps exactly the elements whose draw is 65535"""
    n, F = 8192, 64  # 2^19 draws: 12 of them are 65535 and 8 are 0 at this site
    for p in P_LIST[:2]:
        assert int(device_mask(9, 1, 0, p, n, F)[:n * F].sum()) == n * F
    d = ref.draws(9, 1, 0, np.arange(n * F // 4)).reshape(n, F)
    assert int((d == 65535).sum()) > 0 and int((d == 0).sum()) > 0  # both rules below have something to show
    got = device_mask(9, 1, 0, P_LIST[-1], n, F)[:n * F].view(n, F).numpy()
    assert np.array_equal(got != 0, d == 65535)
    got = device_mask(9, 1, 0, 2.0**-16, n, F)[:n * F].view(n, F).numpy()
    assert np.array_equal(got != 0, d != 0)


@pytest.mark.parametrize("n,F", [(0, 64), (5, 0), (0, 0)])
def test_empty_shapes_write_nothing(n, F):
    assert torch.all(device_mask(1234, 1, 3, 0.25, n, F) == GUARD)


@pytest.mark.parametrize("n,F,pad_x,pad_y", [(33, 15, 2, 5), (129, 130, 7, 1), (5000, 64, 4, 8), (16390, 258, 2, 3)])
def test_draw_site_equals_restatement(n, F, pad_x, pad_y):
    lib = _lib.require_device()
    ldx, ldy = F + pad_x, F + pad_y
    x = torch.ones(n, ldx, device=DEV)
    x[:, F:] = float("nan")  # the pitch gap of x is not read
    for (seed, step, stream), p in zip(TRIPLES, [0.25, np.float32(0.1), 0.5, 0.3, 0.999]):
        pf = np.float32(p)
        scale = np.float32(1) / (np.float32(1) - pf)  # the header's 1.f / (1.f - p)
        assert scale == np.float32(1.0 / (1.0 - float(pf)))  # ... which for these p is the rounded exact quotient too
        y = torch.full((n * ldy + N_GUARD,), 7.0, device=DEV)
        _lib.check(lib.hmp_bias_act_drop_fwd(x.data_ptr(), ldx, n, F, None, _lib.ACT_RELU, float(pf), seed, step, stream, y.data_ptr(), ldy,
                                             _lib.stream_ptr()))
        torch.cuda.synchronize()
        yh = y.cpu()
        assert torch.all(yh[n * ldy:] == 7.0)
        yh = yh[:n * ldy].view(n, ldy)
        assert torch.all(yh[:, F:] == 7.0)
        got = yh[:, :F].numpy()
        keep = ref.keep_mask(seed, step, stream, pf, n, F)
        assert np.array_equal(got != 0, keep), (seed, step, stream, float(pf))
        assert np.all(got[keep] == scale), (float(pf), float(scale))
        assert np.all(got[~keep].view(np.uint32) == 0x80000000)  # a dropped element is stored as -0.0


def test_both_seed_words_reach_every_quad_element():
    n, F = 256, 64
    for s in (1234, 2**61 + 5):
        a = device_mask(s, 1, 3, 0.25, n, F)[:n * F].view(n, F // 4, 4)
        b = device_mask((s + 2**32) % 2**64, 1, 3, 0.25, n, F)[:n * F].view(n, F // 4, 4)
        agree = (a == b).double().mean((0, 1))
        # independent masks agree at 0.75^2 + 0.25^2 = 0.625 with a binomial sd of 0.0076 over 4096 quads: 6 sd
        assert torch.all((agree - 0.625).abs() < 6 * 0.0076), agree.tolist()
