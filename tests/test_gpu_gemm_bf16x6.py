"""Every path of the bf16x6 contraction (`csrc/ntx_gemm_bf16x6.hip`) through `ntx_gemm_bf16x6_ex`, on the plan of tests/test_gpu_gemm.py
(whose buffers, sentinels and restated epilogue this file imports).  `-m gpu`.

  * integer operands from {-2 .. 2}, K <= 2048: exact in the first bf16 term (the other two are 0), every product and partial sum exact in
    float32 -- the result has to EQUAL numpy's integer product.  The bar for placement, bounds, offsets, the K split and the cut of M;
  * normal operands (tests/bf16x6_common.py's sets): the row-wise error against float64 within 2 float32 floors -- numpy's float32 product of
    the same operands, measured the same way -- and within the project's 2e-6 sqrt(K).  tests/test_bf16x6.py shows on the CPU that the
    documented arithmetic meets this bar and that it misses it with any one of the six products left out;
  * what works on the finished accumulator (bias, ReLU, mask, accumulate) BIT-equal to the float32 restatement of the epilogue on this
    kernel's plain product; a range of a split to the unsplit call on its rows; the column sums to `ntx_gemm_f32_ex`'s on the same B.

Sentinels around every output, NaN in the padding of operand rows and in one row behind the last.  Measured ratios and times:
profiles/bf16x6/notes.md."""

import numpy as np
import pytest

from tests import bf16x6_common as x6
from tests.test_gpu_gemm import (GEOMETRIES, OPTIONS, SENTINEL, Dev, bits, epilogue_inputs, epilogue_restated, integers, operand, out_buffer, pad4, split_out)
from tests.test_gpu_gemm import gemm_ex as gemm_f32_ex

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
TK = 16                                  # the kernel's panel depth: one step of v_mfma_f32_32x32x16_bf16


def dev():
    return torch.device("cuda", 0)


def bar(K):
    return 2e-6 * np.sqrt(K)


def gemm_ex(A, lda, ak, B, ldb, C, ldc, M, N, K, bias=None, relu=0, mask=None, ldmask=0, accumulate=0, n_split=1, k_chunk=0, split_stride=0, colsum=None,
            a_at=0, b_at=0, c_at=0):
    """The raw return code of ntx_gemm_bf16x6_ex (the null stream); operands are `Dev`s (or None), `*_at` an offset in floats into A, B and C."""
    from nerf_tex_amd import _lib
    p = lambda d, at=0: d.ptr(at) if d is not None else None
    torch.cuda.synchronize()
    with torch.cuda.device(dev()):
        rc = _lib.lib.ntx_gemm_bf16x6_ex(p(A, a_at), lda, ak, p(B, b_at), ldb, p(C, c_at), ldc, M, N, K, p(bias), relu, p(mask), ldmask, accumulate, n_split, k_chunk, split_stride,
                                         p(colsum))
    torch.cuda.synchronize()
    return rc


def run(*a, **kw):
    from nerf_tex_amd import _lib
    _lib.check(gemm_ex(*a, **kw))


# ---------------------------------------------------------------------------------------------------------------- a. pipeline regimes and K tails
KS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113)       # one panel less one .. seven panels plus one


@pytest.mark.parametrize("alignment", ["aligned", "lda_odd", "pointers_off_by_a_float"])
@pytest.mark.parametrize("ak", [1, 0])
def test_pipeline_regimes_and_k_tails(ak, alignment):
    """130 x 132: one interior tile (the bounds-free pipeline on whole panels, the bounds-checked one on the K tail) and edge tiles in both
    directions.  1 - 3 panels run the tail loop alone, 4 - 5 the body unrolled by two once, 6 - 7 twice.  Integer operands: equal."""
    M, N = 130, 132
    rng = np.random.default_rng(100 * ak + len(alignment))
    off = 1 if alignment == "pointers_off_by_a_float" else 0
    for K in KS:
        A = integers(rng, (M, K) if ak else (K, M)); B = integers(rng, (K, N))
        lda = pad4(A.shape[1]) + 4 + (alignment == "lda_odd"); ldb = pad4(N) + 4; ldc = N + 3
        dA, dB, dC = operand(A, lda, off), operand(B, ldb, off), out_buffer(M, ldc)
        assert (dA.ptr() % 16 == 0) == (off == 0)
        run(dA, lda, ak, dB, ldb, dC, ldc, M, N, K)
        got, rest = split_out(dC.get(), M, N, ldc)
        want = ((A if ak else A.T).astype(np.int64) @ B.astype(np.int64)).astype(F)
        assert np.array_equal(got[0], want), f"K = {K}"
        assert (rest == SENTINEL).all(), f"K = {K}"


@pytest.mark.parametrize("ak", [1, 0])
@pytest.mark.parametrize("M,N,K", [(130, 130, 40), (300, 130, 40), (100, 90, 2048), (129, 128, 33), (128, 129, 33), (70, 3, 50), (1, 130, 50)],
                         ids=["130x130x40", "three_row_tiles", "inside_a_tile_k2048", "m_one_past", "n_one_past", "three_columns", "one_row"])
def test_output_geometries(M, N, K, ak):
    """Inside a tile, M / N one past a tile, N = 3 (three of four waves without columns), M = 1, three row tiles; integer operands: equal."""
    rng = np.random.default_rng(M * 7 + N + K + ak)
    A = integers(rng, (M, K) if ak else (K, M)); B = integers(rng, (K, N))
    lda, ldb, ldc = pad4(A.shape[1]) + 4, pad4(N) + 4, N + 3
    dA, dB, dC = operand(A, lda), operand(B, ldb), out_buffer(M, ldc)
    run(dA, lda, ak, dB, ldb, dC, ldc, M, N, K)
    got, rest = split_out(dC.get(), M, N, ldc)
    assert np.array_equal(got[0], ((A if ak else A.T).astype(np.int64) @ B.astype(np.int64)).astype(F))
    assert (rest == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- b. normal operands
def product(name):
    """The kernel's results of an operand set, one per K range, with the sentinels checked"""
    A, B, ak, n_split, k_chunk = x6.operand_sets()[name]
    M, K = A.shape
    N = B.shape[1]
    stored = A if ak else np.ascontiguousarray(A.T)
    lda, ldb, ldc = pad4(stored.shape[1]) + 4, pad4(N) + 4, N + 3
    stride = (M + 1) * ldc + 5
    dA, dB, dC = operand(stored, lda), operand(B, ldb), out_buffer(M, ldc, n_split, stride)
    run(dA, lda, ak, dB, ldb, dC, ldc, M, N, K, n_split=n_split, k_chunk=k_chunk, split_stride=stride)
    got, rest = split_out(dC.get(), M, N, ldc, n_split, stride)
    assert (rest == SENTINEL).all()
    return got


@pytest.mark.parametrize("name", ["o1", "cotangents", "dw"])
def test_normal_operands_within_two_float32_floors(name):
    """O(1) operands; A's rows scaled by 10**U(-9, -3) (k-contiguous, the dX form); the dW form with B's rows scaled so, K = 4096 in two ranges
    of 2048.  Row-wise against float64: within 2 floors and within 2e-6 sqrt(K).  Every figure is printed before it is gated."""
    got = product(name)
    for z, (Az, Bz) in enumerate(x6.ranges(name)):
        ref = Az.astype(np.float64) @ Bz.astype(np.float64)
        err, floor = x6.rowwise(got[z], ref), x6.floor32(Az, Bz)
        print(f"X6ERR {name} range {z}: K {Az.shape[1]} err {err:.3e} floor {floor:.3e} ratio {err / floor:.2f} (bars: {x6.FLOORS:.0f} floors, {bar(Az.shape[1]):.2e})")
        assert np.isfinite(got[z]).all()
        assert err <= x6.FLOORS * floor, (err, floor)
        assert err <= bar(Az.shape[1])


# ---------------------------------------------------------------------------------------------------------------- c. the epilogue
EPI_M, EPI_N, EPI_K = 130, 130, 40


def epilogue_run(geometry):
    """{options: result [M][N]} of all 16 option sets at one output geometry (tests/test_gpu_gemm.py's, through this kernel)"""
    M, N, K = EPI_M, EPI_N, EPI_K
    ldc, c_off, ldmask, m_off = GEOMETRIES[geometry]
    A, B, bias, old, mask = epilogue_inputs()
    dA, dB, dbias = operand(A, pad4(K) + 4), operand(B, pad4(N) + 4), Dev(bias)
    dmask = operand(mask, ldmask, m_off)
    out = {}
    for opt in OPTIONS:
        use_bias, relu, use_mask, acc = opt
        dC = out_buffer(M, ldc, off=c_off)
        if acc:
            start = np.full((M + 2, ldc), SENTINEL, F); start[:M, :N] = old
            dC.t[dC.off:] = torch.from_numpy(start.ravel())
        run(dA, pad4(K) + 4, 1, dB, pad4(N) + 4, dC, ldc, M, N, K, bias=dbias if use_bias else None, relu=relu, mask=dmask if use_mask else None, ldmask=ldmask if use_mask else 0,
            accumulate=acc)
        got, rest = split_out(dC.get(), M, N, ldc)
        assert (rest == SENTINEL).all(), f"{geometry} {opt}"
        out[opt] = got[0]
    return out


@pytest.fixture(scope="module")
def epilogue_whole():
    return epilogue_run("whole")


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_epilogue_options_at_every_output_geometry(geometry, epilogue_whole):
    """bias x ReLU x mask (values {1.5, 1e-30, 0, -0, -2, NaN}) x accumulate at 130 x 130 x 40, the 8-byte epilogue and each of the four ways to
    miss it: bit-equal to the float32 restatement on this kernel's plain product, the same bits at every geometry."""
    A, B, bias, old, mask = epilogue_inputs()
    got = epilogue_whole if geometry == "whole" else epilogue_run(geometry)
    plain = got[(0, 0, 0, 0)]
    ref = A.astype(np.float64) @ B.astype(np.float64)
    err, floor = x6.rowwise(plain, ref), x6.floor32(A, B)
    print(f"X6ERR epilogue {geometry}: plain product err {err:.3e} floor {floor:.3e} ratio {err / floor:.2f}")
    assert err <= x6.FLOORS * floor and err <= bar(EPI_K)
    for opt in OPTIONS:
        use_bias, relu, use_mask, acc = opt
        want = epilogue_restated(plain, bias if use_bias else None, relu, mask if use_mask else None, old if acc else None)
        assert np.array_equal(bits(got[opt]), bits(want)), f"{geometry} {opt}: not the restated epilogue"
        assert np.array_equal(bits(got[opt]), bits(epilogue_whole[opt])), f"{geometry} {opt}: other bits than the 8-byte epilogue"


# ---------------------------------------------------------------------------------------------------------------- d. the K split, placement, column sums
def split_case(M, N, n_split, K, k_chunk, integer, seed):
    """One split call in the dW form beside its ranges: each range bit-equal to the unsplit call on its rows, the column sums to ntx_gemm_f32_ex's"""
    rng = np.random.default_rng(seed)
    draw = (lambda s: integers(rng, s)) if integer else (lambda s: rng.normal(size=s).astype(F))
    A, B = draw((K, M)), draw((K, N))
    lda, ldb, ldc = pad4(M) + 4, pad4(N) + 4, N + 3
    stride = (M + 1) * ldc + 5
    dA, dB = operand(A, lda), operand(B, ldb)
    dC, dS = out_buffer(M, ldc, n_split, stride), Dev(np.full(n_split * N + 7, SENTINEL, F))
    run(dA, lda, 0, dB, ldb, dC, ldc, M, N, K, n_split=n_split, k_chunk=k_chunk, split_stride=stride, colsum=dS)
    got, rest = split_out(dC.get(), M, N, ldc, n_split, stride)
    sums = dS.get()
    assert (rest == SENTINEL).all() and (sums[n_split * N:] == SENTINEL).all()
    sums = sums[:n_split * N].reshape(n_split, N)
    fC, fS = out_buffer(M, ldc, n_split, stride), Dev(np.full(n_split * N + 7, SENTINEL, F))          # the f32 kernel on the same B
    assert gemm_f32_ex(dA, lda, 0, dB, ldb, fC, ldc, M, N, K, n_split=n_split, k_chunk=k_chunk, split_stride=stride, colsum=fS) == 0
    assert np.array_equal(bits(sums), bits(fS.get()[:n_split * N].reshape(n_split, N))), "column sums: other bits than ntx_gemm_f32_ex's"
    worst = 0.0
    for z in range(n_split):
        lo, hi = z * k_chunk, min((z + 1) * k_chunk, K)
        Az, Bz = A[lo:hi], B[lo:hi]
        if integer:
            assert np.array_equal(got[z], (Az.T.astype(np.int64) @ Bz.astype(np.int64)).astype(F)), f"range {z}"
            assert np.array_equal(sums[z], Bz.astype(np.int64).sum(0).astype(F)), f"column sums of range {z}"
            continue
        one = out_buffer(M, ldc)
        run(dA, lda, 0, dB, ldb, one, ldc, M, N, hi - lo, a_at=lo * lda, b_at=lo * ldb)
        alone, rest = split_out(one.get(), M, N, ldc)
        assert (rest == SENTINEL).all()
        assert np.array_equal(bits(got[z]), bits(alone[0])), f"range {z} is not the unsplit product of its rows"
        worst = max(worst, x6.rowwise(got[z], Az.T.astype(np.float64) @ Bz.astype(np.float64)))
    assert worst <= bar(k_chunk)
    return worst


def split_ks(n_split, k_chunk=48):
    return (n_split * k_chunk, n_split * k_chunk - 1, n_split * k_chunk - 17)           # the last range whole, one element short, ending in a partial panel


@pytest.mark.parametrize("integer", [False, True], ids=["normal", "integer"])
@pytest.mark.parametrize("M,N", [(300, 130), (200, 3)], ids=["three_row_tiles", "three_columns"])
@pytest.mark.parametrize("n_split", [2, 7, 8, 9, 16])
def test_k_split_partials_and_column_sums(n_split, M, N, integer):
    """The dW form, ranges of 48: 8 and 16 ranges take gemm_place's XCD-major numbering, the others the plain one.  M = 300: only the first of
    three row tiles writes a range's column sums.  N = 3: three of a tile's four waves have no columns."""
    worst = 0.0
    for K in split_ks(n_split):
        worst = max(worst, split_case(M, N, n_split, K, 48, integer, seed=n_split * 1000 + K + M + N))
    if not integer:
        print(f"X6ERR split n_split {n_split} {M} x {N}: partials row-wise {worst:.3e} (bar {bar(48):.3e})")


# ---------------------------------------------------------------------------------------------------------------- e. the cut of M into launches
def test_m_beyond_one_launch():
    """M = 65 535 x 128 + 129: a second launch of two row tiles whose A and C start at row 65 535 x 128.  N = 3, K = 5; integer operands."""
    M, N, K = 65535 * 128 + 129, 3, 5
    rng = np.random.default_rng(1)
    A = rng.integers(-2, 3, size=(M, K), dtype=np.int8).astype(F); B = integers(rng, (K, N))
    lda, ldb, ldc = K, 4, 4
    want = A @ B
    dA, dB, dC = Dev(A), operand(B, ldb), Dev(np.full((M + 2, ldc), SENTINEL, F))
    run(dA, lda, 1, dB, ldb, dC, ldc, M, N, K)
    got = dC.get().reshape(M + 2, ldc)
    assert np.array_equal(got[:M, :N], want)
    assert (got[:M, N:] == SENTINEL).all() and (got[M:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- f. refusals
def test_every_refusal_writes_nothing():
    """NTX_E_INVALID before the first launch for each argument ntx_gemm_f32_ex refuses; C and the column sums keep their sentinels."""
    from nerf_tex_amd import _lib
    M, N, K, n_split, kc = 40, 20, 96, 2, 48
    rng = np.random.default_rng(0)
    At, Ak, B = integers(rng, (K, M)), integers(rng, (M, K)), integers(rng, (K, N))
    lda_t, lda_k, ldb, ldc = M + 4, K + 4, N + 4, N + 3
    stride = (M + 1) * ldc
    dAt, dAk, dB, dmask, dbias = operand(At, lda_t), operand(Ak, lda_k), operand(B, ldb), operand(np.ones((M, N), F), N + 1), Dev(np.ones(N, F))
    dC, dS = out_buffer(M, ldc, n_split, stride), Dev(np.full(n_split * N + 7, SENTINEL, F))
    good_t = dict(A=dAt, lda=lda_t, ak=0, B=dB, ldb=ldb, C=dC, ldc=ldc, M=M, N=N, K=K, bias=dbias, relu=1, mask=dmask, ldmask=N + 1, accumulate=0, n_split=n_split, k_chunk=kc,
                  split_stride=stride, colsum=dS)
    good_k = dict(good_t, A=dAk, lda=lda_k, ak=1, colsum=None)
    big = 2 ** 31 - 1
    cases = [("A is NULL", good_t, dict(A=None)), ("B is NULL", good_t, dict(B=None)), ("C is NULL", good_t, dict(C=None)),
             ("M = 0", good_t, dict(M=0)), ("N = 0", good_t, dict(N=0)), ("K = 0", good_t, dict(K=0, n_split=1)), ("M < 0", good_t, dict(M=-1)),
             ("lda < M, A [K][M]", good_t, dict(lda=M - 1)), ("lda < K, A [M][K]", good_k, dict(lda=K - 1)), ("ldb < N", good_t, dict(ldb=N - 1)), ("ldc < N", good_t, dict(ldc=N - 1)),
             ("ldmask < N", good_t, dict(ldmask=N - 1)), ("ldmask < N, A [M][K]", good_k, dict(ldmask=0)),
             ("n_split = 0", good_t, dict(n_split=0)), ("n_split < 0", good_t, dict(n_split=-3)), ("n_split = 65536", good_t, dict(n_split=65536, k_chunk=1, K=65536)),
             ("k_chunk = 0", good_t, dict(k_chunk=0)), ("k_chunk < 0", good_t, dict(k_chunk=-48)),
             ("K beyond the last range", good_t, dict(K=n_split * kc + 1)), ("K leaves the last range empty", good_t, dict(K=(n_split - 1) * kc)),
             ("n_split k_chunk beyond an int", good_t, dict(n_split=65535, k_chunk=big)),
             ("split_stride short of a result", good_t, dict(split_stride=(M - 1) * ldc + N - 1)), ("split_stride = 0", good_t, dict(split_stride=0)),
             ("split_stride < 0", good_t, dict(split_stride=-stride)),
             ("colsum with A [M][K]", good_k, dict(colsum=dS)), ("colsum with A [M][K], unsplit", good_k, dict(colsum=dS, n_split=1))]
    for name, good, change in cases:
        rc = gemm_ex(**dict(good, **change))
        assert rc == _lib.NTX_E_INVALID, f"{name}: returned {rc}"
        assert (dC.get() == SENTINEL).all() and (dS.get() == SENTINEL).all(), f"{name}: wrote something"
    for good in (good_t, good_k):                                                        # and what they were changed from is taken
        run(**good)
        got, rest = split_out(dC.get(), M, N, ldc, n_split, stride)
        A = At.T if good is good_t else Ak
        for z in range(n_split):
            assert np.array_equal(got[z], np.maximum(A[:, z * kc:(z + 1) * kc] @ B[z * kc:(z + 1) * kc] + 1, 0))
        assert (rest == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- g. NaN
def test_a_nan_row_of_a_stays_in_its_row_of_c():
    """A NaN in one row of A: that row of C is NaN in every column, every other row is bit for bit what it is without it."""
    M, N, K, row = 130, 130, 40, 70
    rng = np.random.default_rng(11)
    A, B = rng.normal(size=(M, K)).astype(F), rng.normal(size=(K, N)).astype(F)
    bad = A.copy(); bad[row, 3] = np.nan
    lda, ldb, ldc = pad4(K) + 4, pad4(N) + 4, N + 4
    dB, res = operand(B, ldb), []
    for X in (A, bad):
        dC = out_buffer(M, ldc)
        run(operand(X, lda), lda, 1, dB, ldb, dC, ldc, M, N, K)
        got, rest = split_out(dC.get(), M, N, ldc)
        assert (rest == SENTINEL).all()
        res.append(got[0])
    clean, got = res
    others = np.arange(M) != row
    assert np.isfinite(clean).all() and np.array_equal(bits(got[others]), bits(clean[others]))
    assert np.isnan(got[row]).all()
