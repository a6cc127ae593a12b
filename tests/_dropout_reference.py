"""The dropout generator in numpy, written from its statement above hmp_dropout_mask in include/hydra_mp.h (not from csrc/common.h).

uint32 arithmetic throughout (numpy arrays of dtype uint32 wrap modulo 2^32 without warnings).  tests/test_dropout_reference.py
ties it bit for bit to the C++ (tools/drop_check.cpp) and checks its statistics; tests/test_gpu_dropout_generator.py compares the
device export and a draw site with it."""
import numpy as np

U32 = np.uint32
_M32 = 0xFFFFFFFF

STREAM_MUL = 0x9E3779B1
STEP_MUL = 0x85EBCA77
B_ADD = 0x9E3779B9
B_QMUL = 0xC2B2AE3D


def _u32(x) -> np.ndarray:
    """x (python int, or array of non-negative ints) modulo 2^32 as a uint32 array"""
    if isinstance(x, np.ndarray):
        return (x.astype(np.uint64) & np.uint64(_M32)).astype(U32)
    return np.asarray(int(x) & _M32, dtype=np.uint64).astype(U32)


def hash32(x: np.ndarray) -> np.ndarray:
    x = np.array(x, dtype=U32, copy=True)
    x ^= x >> U32(16)
    x *= U32(0x7FEB352D)
    x ^= x >> U32(15)
    x *= U32(0x846CA68B)
    x ^= x >> U32(16)
    return x


def key_word(seed: int, step: int, stream: int) -> np.ndarray:
    k0, k1 = _u32(seed), _u32(int(seed) >> 32)
    return k0 ^ (_u32(stream) * U32(STREAM_MUL)) ^ (_u32(step) * U32(STEP_MUL)) ^ hash32(k1)


def words(seed: int, step: int, stream: int, q) -> tuple:
    """the raw word pair (a, b) of the quads q (any integers: the counter is q modulo 2^32), two uint32 arrays of q's shape"""
    q = _u32(np.asarray(q))
    k1 = _u32(int(seed) >> 32)
    a = hash32(q ^ key_word(seed, step, stream))
    b = hash32((a + U32(B_ADD)) ^ k1 ^ (q * U32(B_QMUL)))
    return a, b


def thresh(p) -> int:
    """the 32-bit threshold of the C float p"""
    t = float(np.float32(p)) * 4294967296.0  # float32 -> double is exact, and so is the product by a power of two
    return int(min(max(t, 0.0), 4294967295.0))  # int() truncates


def draws(seed: int, step: int, stream: int, q) -> np.ndarray:
    """the four 16-bit draws of each quad: uint32 [..., 4]"""
    a, b = words(seed, step, stream, q)
    return np.stack([a & U32(0xFFFF), a >> U32(16), b & U32(0xFFFF), b >> U32(16)], axis=-1)


def keep_quads(seed: int, step: int, stream: int, p, q) -> np.ndarray:
    """keep flags of the four elements of each quad: bool [..., 4]"""
    return draws(seed, step, stream, q) >= U32(thresh(p) >> 16)


def keep_bits(seed: int, step: int, stream: int, p, q) -> np.ndarray:
    """the same packed, element j in bit j: uint32 of q's shape"""
    k = keep_quads(seed, step, stream, p, q).astype(U32)
    return k[..., 0] | (k[..., 1] << U32(1)) | (k[..., 2] << U32(2)) | (k[..., 3] << U32(3))


def keep_mask(seed: int, step: int, stream: int, p, n_rows: int, F: int) -> np.ndarray:
    """hmp_dropout_mask(seed, step, stream, p, n_rows, F): bool [n_rows, F]"""
    qpr = (F + 3) >> 2
    q = np.arange(n_rows, dtype=np.int64)[:, None] * qpr + np.arange(qpr, dtype=np.int64)[None, :]
    return keep_quads(seed, step, stream, p, q).reshape(n_rows, qpr * 4)[:, :F].copy()


def keep_prob(p) -> float:
    """the probability with which an element is kept: draws are uniform on 0 .. 65535"""
    return 1.0 - (thresh(p) >> 16) / 65536.0
