"""What the bf16x6 tests share (tests/test_bf16x6.py without a GPU, tests/test_gpu_gemm_bf16x6.py with one): a numpy restatement of the
arithmetic `csrc/ntx_gemm_bf16x6.hip` documents, the operand sets of normal values both files use, and the one error measure and float32
floor both are judged by.

THE ARITHMETIC.  v = v0 + v1 + v2 with v0 = bf16_rne(v), v1 = bf16_rne(v - v0), v2 = bf16_rne(v - v0 - v1), the subtractions in float32;
the six products of order <= 2 as float32 matrix products, added in float32 smallest first: a0b2, a1b1, a2b0, a0b1, a1b0, a0b0.

THE MEASURE.  Row-wise: max over the rows i of max_j |x - ref|[i] / max_j |ref|[i], ref the float64 product -- a row of A scaled by 1e-9 counts
as much as a row of O(1).  THE FLOOR of an operand set is numpy's float32 product of the same operands, measured the same way; the bar of both
files is 2 floors (the kernel may be as wrong as float32 rounding makes any float32 product, and a little: its order of summation is another)."""

import numpy as np

F = np.float32
ORDER = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))      # smallest first
FLOORS = 2.0


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), as float32; finite values"""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F).reshape(np.shape(x))


def split3(x):
    x = np.asarray(x, F)
    v0 = bf16_rne(x)
    r1 = (x - v0).astype(F)
    v1 = bf16_rne(r1)
    r2 = (r1 - v1).astype(F)
    return v0, v1, bf16_rne(r2)


def emulate(A, B, leave_out=None):
    """The documented arithmetic on A [M][K], B [K][N]; `leave_out`: one (i, j) of ORDER that is not added"""
    a, b = split3(A), split3(B)
    y = np.zeros((A.shape[0], B.shape[1]), F)
    for i, j in ORDER:
        if (i, j) != leave_out:
            y = (y + (a[i] @ b[j]).astype(F)).astype(F)
    return y


def rowwise(x, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.max(np.abs(np.asarray(x, np.float64) - ref), axis=1) / np.max(np.abs(ref), axis=1)))


def floor32(A, B):
    """numpy's float32 product of the same operands against float64"""
    return rowwise(A.astype(F) @ B.astype(F), A.astype(np.float64) @ B.astype(np.float64))


def activations(rng, shape):
    """O(1) and half of them zero, as behind a ReLU"""
    return (np.maximum(rng.standard_normal(shape), 0) * rng.standard_normal(shape)).astype(F)


def operand_sets():
    """{name: (A' [M][K] as the product reads it, B [K][N], a_kcontig, n_split, k_chunk)} -- A' is what is multiplied; the dW form stores its transpose.
      o1         O(1) activations times glorot-scale weights, k-contiguous
      cotangents the same with A's rows scaled by 10**U(-9, -3): the cotangents of a mean loss, k-contiguous (the dX form)
      dw         the dW form: A [K][M] activations, B's rows (one per sample) scaled the same way, K = 4096 in two ranges of 2048"""
    rng = np.random.default_rng(2024)
    M, K, N = 200, 256, 130
    W = (rng.standard_normal((K, N)) * 0.1).astype(F)
    A1 = activations(rng, (M, K))
    A2 = (activations(rng, (M, K)) * 10.0 ** rng.uniform(-9, -3, (M, 1))).astype(F)
    Kd, Md, Nd = 4096, 130, 130
    X = np.maximum(rng.standard_normal((Kd, Md)), 0).astype(F)
    G = (rng.standard_normal((Kd, Nd)) * 10.0 ** rng.uniform(-9, -3, (Kd, 1))).astype(F)
    return {"o1": (A1, W, 1, 1, K), "cotangents": (A2, W, 1, 1, K), "dw": (np.ascontiguousarray(X.T), G, 0, 2, 2048)}


def ranges(name):
    """[(A' rows x its range of K, B's range)] of an operand set: one pair per K range"""
    A, B, _, n_split, k_chunk = operand_sets()[name]
    return [(A[:, z * k_chunk:(z + 1) * k_chunk], B[z * k_chunk:(z + 1) * k_chunk]) for z in range(n_split)]
