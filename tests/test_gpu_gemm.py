"""Every path of the f32 contraction behind the layer-by-layer trainer (`csrc/ntx_gemm.hip`), through `ntx_gemm_f32_ex`, the launcher's whole
argument list at the C ABI.  `-m gpu`.

Two kinds of input, two kinds of bar:
  * integer-valued operands from {-2 .. 2} with K <= 2048: every product and partial sum is exact in float32, so the result cannot depend on the
    order of the sum and has to EQUAL numpy's integer product.  The bar for placement, bounds, offsets and the cut of M into launches;
  * normal operands: rel-Linf <= 2e-6 sqrt(K) of the float64 product (the bar of tests/test_gpu_train.py::test_gemm_kernel_against_float64;
    sqrt(k_chunk) for one range of a split).  Where an option only works on the finished accumulator -- bias, ReLU, mask, accumulate -- the
    result has to be BIT-equal to a float32 restatement of the epilogue on the plain product of the same operands; a range of a split to the
    unsplit call on that range's rows; a column sum to a float32 restatement of the kernel's order.

Every output buffer is filled with a sentinel first and is wider and longer than the result (and a split's partials lie further apart than they
are long); what the call must not write has to hold the sentinel afterwards.  Operand rows are padded with NaN, with a NaN row behind the last:
a read past K, M or N that reached the product would show.  Measured errors and times: profiles/gemm_paths/notes.md."""

import itertools

import numpy as np
import pytest

from tests.train_common import rel_linf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
SENTINEL = F(-12345.5)                  # no integer, and nothing a product of a few hundred normal terms comes to
TK, TM = 16, 128                        # the kernel's panel depth and tile height


def dev():
    return torch.device("cuda", 0)


def pad4(n):
    return (n + 3) // 4 * 4


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def bar(K):
    return 2e-6 * np.sqrt(K)


class Dev:
    """A float32 device buffer whose first element sits `off` floats behind an allocation (torch's are 256-byte aligned): `off` = 1 is a
    pointer off 16 and off 8 bytes."""

    def __init__(self, flat, off=0):
        flat = np.ascontiguousarray(flat, dtype=F).ravel()
        self.off, self.n = off, flat.size
        self.t = torch.empty(off + flat.size, dtype=torch.float32, device=dev())
        assert self.t.data_ptr() % 16 == 0
        self.t[off:] = torch.from_numpy(flat)

    def ptr(self, at=0):
        return self.t.data_ptr() + 4 * (self.off + at)

    def get(self):
        return self.t[self.off:].cpu().numpy()


def operand(X, ld, off=0):
    """Rows of `X` at stride `ld`, NaN in the padding and in one more row."""
    rows, cols = X.shape
    assert ld >= cols
    buf = np.full((rows + 1, ld), np.nan, F)
    buf[:rows, :cols] = X
    return Dev(buf, off)


def gemm_ex(A, lda, ak, B, ldb, C, ldc, M, N, K, bias=None, relu=0, mask=None, ldmask=0, accumulate=0, n_split=1, k_chunk=0, split_stride=0, colsum=None,
            a_at=0, b_at=0, c_at=0):
    """The raw return code of ntx_gemm_f32_ex; operands are `Dev`s (or None), `*_at` an offset in floats into A, B and C."""
    from nerf_tex_amd import _lib
    p = lambda d, at=0: d.ptr(at) if d is not None else None
    with torch.cuda.device(dev()):
        rc = _lib.lib.ntx_gemm_f32_ex(p(A, a_at), lda, ak, p(B, b_at), ldb, p(C, c_at), ldc, M, N, K, p(bias), relu, p(mask), ldmask, accumulate, n_split, k_chunk, split_stride,
                                      p(colsum), torch.cuda.current_stream(dev()).cuda_stream)
    torch.cuda.synchronize()
    return rc


def run(*a, **kw):
    from nerf_tex_amd import _lib
    _lib.check(gemm_ex(*a, **kw))


def out_buffer(M, ldc, n_split=1, split_stride=0, off=0):
    """Sentinels for `n_split` results of M rows at stride ldc, `split_stride` apart, and two rows more."""
    return Dev(np.full((n_split - 1) * split_stride + (M + 2) * ldc, SENTINEL, F), off)


def split_out(flat, M, N, ldc, n_split=1, split_stride=0):
    """(results [n_split][M][N], everything else of the buffer)"""
    idx = (np.arange(n_split)[:, None, None] * split_stride + np.arange(M)[None, :, None] * ldc + np.arange(N)[None, None, :])
    rest = np.ones(flat.size, bool)
    rest[idx.ravel()] = False
    return flat[idx], flat[rest]


def integers(rng, shape):
    return rng.integers(-2, 3, size=shape).astype(F)


def product64(A, B, ak):
    A = A.astype(np.float64)
    return (A if ak else A.T) @ B.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- a. pipeline regimes and K tails
KS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 81, 96, 97)       # 1 .. 7 panels of 16, each count with and without a partial last one


@pytest.mark.parametrize("alignment", ["aligned", "lda_odd", "pointers_off_by_a_float"])
@pytest.mark.parametrize("ak", [1, 0])
def test_pipeline_regimes_and_k_tails(ak, alignment):
    """130 x 132: one interior tile (the bounds-free pipeline on whole panels, then the bounds-checked one on the K tail) and edge tiles in both
    directions (bounds-checked throughout).  1 - 3 panels run the tail loop alone, 4 - 5 the body unrolled by two once, 6 - 7 twice.  With an odd
    lda or pointers off 16 bytes nothing goes by 16-byte loads.  Integer operands: equal to the integer product."""
    M, N = 130, 132
    rng = np.random.default_rng(100 * ak + len(alignment))
    off = 1 if alignment == "pointers_off_by_a_float" else 0
    for K in KS:
        A = integers(rng, (M, K) if ak else (K, M)); B = integers(rng, (K, N))
        lda = pad4(A.shape[1]) + 4 + (alignment == "lda_odd"); ldb = pad4(N) + 4; ldc = N + 3
        assert lda % 2 == (alignment == "lda_odd") and ldb % 4 == 0
        dA, dB, dC = operand(A, lda, off), operand(B, ldb, off), out_buffer(M, ldc)
        assert (dA.ptr() % 16 == 0) == (off == 0)
        run(dA, lda, ak, dB, ldb, dC, ldc, M, N, K)
        got, rest = split_out(dC.get(), M, N, ldc)
        want = ((A if ak else A.T).astype(np.int64) @ B.astype(np.int64)).astype(F)
        assert np.array_equal(got[0], want), f"K = {K}"
        assert (rest == SENTINEL).all(), f"K = {K}"


# ---------------------------------------------------------------------------------------------------------------- b. the epilogue
EPI_M, EPI_N, EPI_K = 130, 130, 40
#                 ldc, C off, ldmask, mask off
GEOMETRIES = {"whole": (134, 0, 132, 0),                       # the interior tile stores and reads 8 bytes at a time
              "ldc_odd": (133, 0, 132, 0),
              "c_off_by_a_float": (134, 1, 132, 0),
              "ldmask_odd": (134, 0, 133, 0),
              "mask_off_by_a_float": (134, 0, 132, 1)}
OPTIONS = list(itertools.product((0, 1), repeat=4))            # bias, relu, mask, accumulate


def epilogue_inputs():
    rng = np.random.default_rng(7)
    M, N, K = EPI_M, EPI_N, EPI_K
    A, B = rng.normal(size=(M, K)).astype(F), rng.normal(size=(K, N)).astype(F)
    bias, old = rng.normal(size=N).astype(F), rng.normal(size=(M, N)).astype(F)              # what `accumulate` finds in C: data, not zeros
    mask = rng.choice(np.asarray([1.5, 1e-30, 0.0, -0.0, -2.0, np.nan], F), size=(M, N))     # kept where mask > 0: NaN drops
    return A, B, bias, old, mask


def epilogue_restated(plain, bias, relu, mask, old):
    """csrc/ntx_gemm.hip's epilogue in float32, in its order: acc (+ what C held) + bias (0.0f without one), ReLU as v > 0 ? v : 0, then the mask"""
    v = plain.astype(F)
    if old is not None:
        v = v + old
    v = v + (bias[None] if bias is not None else F(0))
    with np.errstate(invalid="ignore"):
        if relu:
            v = np.where(v > 0, v, F(0))
        if mask is not None:
            v = np.where(mask > 0, v, F(0))
    assert v.dtype == F
    return v


def epilogue_run(geometry):
    """{options: result [M][N]} of all 16 option sets at one output geometry; the sentinels are checked here"""
    M, N, K = EPI_M, EPI_N, EPI_K
    ldc, c_off, ldmask, m_off = GEOMETRIES[geometry]
    A, B, bias, old, mask = epilogue_inputs()
    dA, dB, dbias = operand(A, pad4(K) + 4), operand(B, pad4(N) + 4), Dev(bias)
    dmask = operand(mask, ldmask, m_off)
    out = {}
    for opt in OPTIONS:
        use_bias, relu, use_mask, acc = opt
        dC = out_buffer(M, ldc, off=c_off)
        assert dC.ptr() % 8 == 4 * c_off and dmask.ptr() % 8 == 4 * m_off
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
    """bias x ReLU x mask x accumulate at 130 x 130 x 40: the interior tile takes the 8-byte epilogue only when ldc and ldmask are even and C
    and mask sit on 8 bytes; each of the four ways to miss that sends it down the scalar path the edge tiles always take.  Every option set:
    bit-equal to the float32 restatement on the plain product, and the same bits at every geometry.  The plain product: the float64 bar."""
    A, B, bias, old, mask = epilogue_inputs()
    got = epilogue_whole if geometry == "whole" else epilogue_run(geometry)
    plain = got[(0, 0, 0, 0)]
    err = rel_linf(plain, product64(A, B, 1))
    print(f"epilogue {geometry}: plain product rel-Linf {err:.3e} (bar {bar(EPI_K):.3e})")
    assert err <= bar(EPI_K)
    for opt in OPTIONS:
        use_bias, relu, use_mask, acc = opt
        want = epilogue_restated(plain, bias if use_bias else None, relu, mask if use_mask else None, old if acc else None)
        assert np.array_equal(bits(got[opt]), bits(want)), f"{geometry} {opt}: not the restated epilogue"
        assert np.array_equal(bits(got[opt]), bits(epilogue_whole[opt])), f"{geometry} {opt}: other bits than the 8-byte epilogue"
    with np.errstate(invalid="ignore"):
        kept = mask > 0
    assert kept.any() and (~kept).any() and (got[(0, 0, 1, 0)][~kept] == 0).all() and (got[(0, 0, 1, 0)][kept] != 0).all()


# ---------------------------------------------------------------------------------------------------------------- c. the K split, placement, column sums
def colsum_restated(Bz):
    """The kernel's order for the column sums of one range's rows Bz [k][N]: panel row r = 0 .. 15 adds its elements B[16 p + r] over the
    panels p in ascending order (0.0f where the range has ended), then the 16 rows are added in ascending order; float32 throughout."""
    k, N = Bz.shape
    panels = (k + TK - 1) // TK
    padded = np.zeros((panels * TK, N), F); padded[:k] = Bz
    rows = np.zeros((TK, N), F)
    for p in range(panels):
        rows = rows + padded[p * TK:(p + 1) * TK]
    total = np.zeros(N, F)
    for r in range(TK):
        total = total + rows[r]
    return total


def split_case(M, N, n_split, K, k_chunk, integer, seed):
    """One split call in the dW form (A [K][M]) beside its ranges; returns the measured errors (partials, column sums) of normal operands"""
    rng = np.random.default_rng(seed)
    draw = (lambda s: integers(rng, s)) if integer else (lambda s: rng.normal(size=s).astype(F))
    A, B = draw((K, M)), draw((K, N))
    lda, ldb, ldc = pad4(M) + 4, pad4(N) + 4, N + 3
    stride = (M + 1) * ldc + 5                                                           # a gap between two ranges' partials
    dA, dB = operand(A, lda), operand(B, ldb)
    dC, dS = out_buffer(M, ldc, n_split, stride), Dev(np.full(n_split * N + 7, SENTINEL, F))
    run(dA, lda, 0, dB, ldb, dC, ldc, M, N, K, n_split=n_split, k_chunk=k_chunk, split_stride=stride, colsum=dS)
    got, rest = split_out(dC.get(), M, N, ldc, n_split, stride)
    sums = dS.get()
    assert (rest == SENTINEL).all() and (sums[n_split * N:] == SENTINEL).all()
    sums = sums[:n_split * N].reshape(n_split, N)
    e_part = e_sum = 0.0
    for z in range(n_split):
        lo, hi = z * k_chunk, min((z + 1) * k_chunk, K)
        Az, Bz = A[lo:hi], B[lo:hi]
        if integer:
            assert np.array_equal(got[z], (Az.T.astype(np.int64) @ Bz.astype(np.int64)).astype(F)), f"range {z}"
            assert np.array_equal(sums[z], Bz.astype(np.int64).sum(0).astype(F)), f"column sums of range {z}"
            continue
        one = out_buffer(M, ldc)                                                         # the same rows, unsplit: the panels start at the same places
        run(dA, lda, 0, dB, ldb, one, ldc, M, N, hi - lo, a_at=lo * lda, b_at=lo * ldb)
        alone, rest = split_out(one.get(), M, N, ldc)
        assert (rest == SENTINEL).all()
        assert np.array_equal(bits(got[z]), bits(alone[0])), f"range {z} is not the unsplit product of its rows"
        assert np.array_equal(bits(sums[z]), bits(colsum_restated(Bz))), f"column sums of range {z} are not the kernel's order restated"
        e_part = max(e_part, rel_linf(got[z], product64(Az, Bz, 0)))
        e_sum = max(e_sum, rel_linf(sums[z], Bz.astype(np.float64).sum(0)))
    if not integer:
        assert e_part <= bar(k_chunk) and e_sum <= bar(k_chunk), (e_part, e_sum, bar(k_chunk))
    return e_part, e_sum


def split_ks(n_split, k_chunk=48):
    return (n_split * k_chunk, n_split * k_chunk - 1, n_split * k_chunk - 17)           # the last range whole, one element short, ending in a partial panel


@pytest.mark.parametrize("integer", [False, True], ids=["normal", "integer"])
@pytest.mark.parametrize("n_split", [2, 7, 8, 9, 16, 24])
def test_k_split_partials_and_column_sums(n_split, integer):
    """The dW form at 200 x 130 (2 x 2 tiles), ranges of 48: a number of ranges that is a multiple of 8 takes gemm_place's XCD-major numbering
    (one and several rounds of 8), any other the plain one.  Normal operands: every partial bit-identical to the unsplit call on its rows, every
    column sum to the restated order, both inside the float64 bar.  Integer operands: equal to the integer products and sums."""
    worst = (0.0, 0.0)
    for K in split_ks(n_split):
        worst = max(worst, split_case(200, 130, n_split, K, 48, integer, seed=n_split * 1000 + K))
    if not integer:
        print(f"split n_split {n_split}: partials rel-Linf {worst[0]:.3e}, column sums {worst[1]:.3e} (bar {bar(48):.3e})")


@pytest.mark.parametrize("integer", [False, True], ids=["normal", "integer"])
@pytest.mark.parametrize("M,N", [(300, 130), (200, 3)], ids=["three_row_tiles", "three_columns"])
@pytest.mark.parametrize("n_split", [8, 9])
def test_k_split_three_row_tiles_and_three_columns(n_split, M, N, integer):
    """M = 300: only the first of three row tiles writes a range's column sums, which still have to be whole.  N = 3: three of a tile's four
    waves have no columns."""
    worst = (0.0, 0.0)
    for K in split_ks(n_split):
        worst = max(worst, split_case(M, N, n_split, K, 48, integer, seed=n_split * 1000 + K + M + N))
    if not integer:
        print(f"split n_split {n_split} {M} x {N}: partials rel-Linf {worst[0]:.3e}, column sums {worst[1]:.3e} (bar {bar(48):.3e})")


@pytest.mark.parametrize("n_split", [3, 8])
@pytest.mark.parametrize("k_chunk", [16, 18])
def test_k_split_of_k_contiguous_rows(k_chunk, n_split):
    """A [M][K] with a split: range z starts at column z k_chunk of A's rows, which for k_chunk = 18 is off 16 bytes in every other range
    although lda, ldb and both pointers are aligned -- the launcher has to take that into `aligned`.  Integer operands."""
    M, N = 130, 132
    rng = np.random.default_rng(k_chunk * 10 + n_split)
    for K in (n_split * k_chunk, n_split * k_chunk - 1):
        A, B = integers(rng, (M, K)), integers(rng, (K, N))
        lda, ldb, ldc = pad4(K) + 4, pad4(N) + 4, N + 3
        stride = (M + 1) * ldc + 5
        dA, dB, dC = operand(A, lda), operand(B, ldb), out_buffer(M, ldc, n_split, stride)
        run(dA, lda, 1, dB, ldb, dC, ldc, M, N, K, n_split=n_split, k_chunk=k_chunk, split_stride=stride)
        got, rest = split_out(dC.get(), M, N, ldc, n_split, stride)
        assert (rest == SENTINEL).all()
        for z in range(n_split):
            lo, hi = z * k_chunk, min((z + 1) * k_chunk, K)
            assert np.array_equal(got[z], (A[:, lo:hi].astype(np.int64) @ B[lo:hi].astype(np.int64)).astype(F)), f"K = {K}, range {z}"


# ---------------------------------------------------------------------------------------------------------------- d. the cut of M into launches
CUT = 65535 * TM                         # rows of the first launch: row tiles are a grid dimension, 65 535 at the most


@pytest.mark.parametrize("ak,epilogue", [(1, False), (0, False), (1, True)], ids=["k_contiguous", "transposed", "k_contiguous_mask_accumulate"])
def test_m_beyond_one_launch(ak, epilogue):
    """M = 65 535 x 128 + 129: a second launch of two row tiles whose A, C and mask start at row 65 535 x 128.  N = 3, K = 5: one panel a tile.
    Integer operands (the mask from {1, 0, -1}, what C held from {-2 .. 2}): every row equal to the integer result."""
    M, N, K = CUT + 129, 3, 5
    rng = np.random.default_rng(ak + 2 * epilogue)
    A = rng.integers(-2, 3, size=(M, K) if ak else (K, M), dtype=np.int8).astype(F); B = integers(rng, (K, N))
    lda, ldb, ldc, ldmask = A.shape[1], 4, 4, 5
    want = (A if ak else A.T) @ B                                                        # exact in float32: sums of five integers
    dA, dB = Dev(A), operand(B, ldb)
    start = np.full((M + 2, ldc), SENTINEL, F)
    dmask = None
    if epilogue:
        old = rng.integers(-2, 3, size=(M, N), dtype=np.int8).astype(F); mask = rng.integers(-1, 2, size=(M, N), dtype=np.int8).astype(F)
        start[:M, :N] = old
        want = np.where(mask > 0, want + old, F(0))
        mbuf = np.full((M, ldmask), 1, F); mbuf[:, :N] = mask
        dmask = Dev(mbuf)
    dC = Dev(start)
    run(dA, lda, ak, dB, ldb, dC, ldc, M, N, K, mask=dmask, ldmask=ldmask if epilogue else 0, accumulate=int(epilogue))
    got = dC.get().reshape(M + 2, ldc)
    for row in (0, CUT - 1, CUT, M - 1):
        assert np.array_equal(got[row, :N], want[row]), f"row {row}"
    assert np.array_equal(got[:M, :N], want)
    assert (got[:M, N:] == SENTINEL).all() and (got[M:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- e. refusals
def test_every_refusal_writes_nothing():
    """NTX_E_INVALID before the first launch for each argument the entry refuses; C and the column sums keep their sentinels."""
    from nerf_tex_amd import _lib
    M, N, K, n_split, kc = 40, 20, 96, 2, 48
    rng = np.random.default_rng(0)
    At, Ak, B = integers(rng, (K, M)), integers(rng, (M, K)), integers(rng, (K, N))      # the dW form and the k-contiguous one
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


# ---------------------------------------------------------------------------------------------------------------- f. non-finite values
def nonfinite_case(relu):
    M, N, K, row = 130, 130, 40, 70
    rng = np.random.default_rng(11)
    A, B = rng.normal(size=(M, K)).astype(F), rng.normal(size=(K, N)).astype(F)
    bad = A.copy(); bad[row, 3] = np.nan; bad[row, 21] = np.inf
    lda, ldb, ldc = pad4(K) + 4, pad4(N) + 4, N + 4
    dB, res = operand(B, ldb), []
    for X in (A, bad):
        dC = out_buffer(M, ldc)
        run(operand(X, lda), lda, 1, dB, ldb, dC, ldc, M, N, K, relu=relu)
        got, rest = split_out(dC.get(), M, N, ldc)
        assert (rest == SENTINEL).all()
        res.append(got[0])
    clean, got = res
    others = np.arange(M) != row
    assert np.isfinite(clean).all() and np.array_equal(bits(got[others]), bits(clean[others]))       # no other row moves a bit
    return got[row]


def test_a_nonfinite_row_of_a_stays_in_its_row_of_c():
    """A NaN and an inf in one row of A, no ReLU: that row of C is non-finite in every column, every other row is what it is without them."""
    assert not np.isfinite(nonfinite_case(relu=0)).any()


def test_relu_epilogue_turns_nan_into_zero_present_behaviour():
    """PINS WHAT THE KERNEL DOES TODAY, not what it should do: the epilogue's `v > 0 ? v : 0` sends NaN to 0, where the reference's tf.nn.relu
    keeps it (and the render kernels propagate it).  A row of A with a NaN therefore leaves a ReLU layer as a row of exact zeros: a non-finite
    input to a layer-by-layer training step is not reported."""
    assert (bits(nonfinite_case(relu=1)) == 0).all()
