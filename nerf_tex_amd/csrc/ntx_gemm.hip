// ntx_gemm.hip -- the general f32 contraction on the matrix cores: one Dense layer and pass of the layer-by-layer training step
// (ntx_backend_flex.hip) and ntx_gemm_f32 / ntx_gemm_f32_ex on caller buffers, all through one launcher.  Since it cuts the rows into launches of at most
// 65 535 tiles, ntx_gemm_f32 also takes an M beyond 65 535 x 128 rows, which used to fail at launch.  gfx950 only.
//   C[i][j] = sum_p A'(i, p) B(p, j) for i < M, j < N, p < K, with B[p * ldb + j] and
//   A'(i, p) = A_KCONTIG ? A[i * lda + p] : A[p * lda + i]
// A workgroup (4 waves) owns a 128 x 128 tile of C, a wave a 64 x 64 quarter of it = 2 x 2 MFMA tiles of 32 x 32 (64 accumulator registers).  K advances a panel (16) at a time: the next
// 128 x 16 / 16 x 128 panels are fetched into registers (16-byte loads when the panel lies inside the matrices and the rows are 16-byte
// aligned, element by element with bounds otherwise) while the current ones, already in LDS as As[p][i] / Bs[p][j], feed the MFMAs; one
// barrier per panel (double buffered).  The f32 MFMA shares the vector ALUs' lanes, so every VALU instruction of the loop
// costs MFMA time: hence the vector loads and the branch-free interior path.
// GemmArgs::precision = NTX_PRECISION_BF16X6 sends the same tiles, grid and arguments to the second body, ntx_gemm_bf16x6.hip (six bf16 products
// on the 16-bit MFMAs); what the two bodies share -- the epilogue, the column sums' ordered tail, the tile numbering -- is ntx_gemm_device.h.
#include <algorithm>
#include <type_traits>
#include "ntx_gemm_device.h"   // fetch_run, gemm_epilogue, gemm_colsum_sum, gemm_place: shared with the bf16x6 body
namespace ntx_train {
// TN_: columns of the workgroup's tile (128 or 256: two or four 64-wide waves across), TK_: depth of a panel; a wave always owns 64 x 64
template <bool A_KCONTIG, int TN_, int TK_>
__device__ __forceinline__ void gemm_body(const GemmArgs &g, int bx, int by, int bz) {
    constexpr int THREADS = TN_ * 2, WCOLS = TN_ / 64, LROWA = TM + 4, LROWB_ = TN_ + 4;
    constexpr int FA = TM * TK_ / THREADS;          // floats of the A panel a thread carries
    constexpr int FB = TN_ * TK_ / THREADS;         // ... of the B panel
    constexpr int TPR = THREADS / TK_;              // threads along a panel row (B, and A when its rows run along i)
    static_assert(FA % 4 == 0 && FB % 4 == 0 && FA * (THREADS / TM) == TK_ && TPR * FB == TN_ && TPR * FA == TM, "panel split");
    __shared__ __attribute__((aligned(16))) float As[2][TK_][LROWA], Bs[2][TK_][LROWB_];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j0 = bx * TN_, i0 = by * TM;
    const int k_begin = bz * g.k_chunk;
    const int k_end = k_begin + g.k_chunk < g.K ? k_begin + g.k_chunk : g.K;
    float *C = g.C + (size_t)bz * (size_t)g.split_stride;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
    // two panels are in flight from memory at any time: the registers of panel kt + 2 are being filled while panel kt + 1 goes from its
    // registers into LDS and panel kt feeds the MFMAs
    float ra[2][FA], rb[2][FB], cs[FB];
#pragma unroll
    for (int q = 0; q < FB; ++q) cs[q] = 0.0f;
    const bool want_colsum = !A_KCONTIG && g.colsum != nullptr && by == 0;
    const bool inner = g.aligned && i0 + TM <= g.M && j0 + TN_ <= g.N;          // the tile lies inside A' and B: only the K end of a panel can stick out
    // thread -> its run of the A panel (k-contiguous rows A[i][p]: row t % 128, FA elements from (t / 128) * FA; rows along i, A[p][i]: panel row
    // t / TPR, FA elements from (t % TPR) * FA) and of the B panel (B[p][j]: panel row t / TPR, FB elements from (t % TPR) * FB)
    const int a_row = A_KCONTIG ? (int)(threadIdx.x % TM) : (int)(threadIdx.x / TPR), a_off = A_KCONTIG ? (int)(threadIdx.x / TM) * FA : (int)(threadIdx.x % TPR) * FA;
    const int b_row = (int)(threadIdx.x / TPR), b_off = (int)(threadIdx.x % TPR) * FB;
    auto fetch = [&](int k0, float *fa, float *fb) {                  // with bounds: a run that lies inside still comes by 16-byte loads
        const bool al = g.aligned != 0;
        if (A_KCONTIG) fetch_run<FA, false>(g.A + (size_t)(i0 + a_row) * g.lda + k0 + a_off, i0 + a_row < g.M, k0 + a_off, k_end, fa, al);
        else fetch_run<FA, false>(g.A + (size_t)(k0 + a_row) * g.lda + i0 + a_off, k0 + a_row < k_end, i0 + a_off, g.M, fa, al);
        fetch_run<FB, false>(g.B + (size_t)(k0 + b_row) * g.ldb + j0 + b_off, k0 + b_row < k_end, j0 + b_off, g.N, fb, al);
    };
    auto stash = [&](int buf, const float *fa, const float *fb) {
        if (want_colsum) {
#pragma unroll
            for (int q = 0; q < FB; ++q) cs[q] += fb[q];
        }
        if (A_KCONTIG) {
#pragma unroll
            for (int q = 0; q < FA; ++q) As[buf][a_off + q][a_row] = fa[q];
        } else {
            f32x4 *d = reinterpret_cast<f32x4 *>(&As[buf][a_row][a_off]);
#pragma unroll
            for (int q = 0; q < FA / 4; ++q) d[q] = f32x4{fa[4 * q], fa[4 * q + 1], fa[4 * q + 2], fa[4 * q + 3]};
        }
        f32x4 *d = reinterpret_cast<f32x4 *>(&Bs[buf][b_row][b_off]);
#pragma unroll
        for (int q = 0; q < FB / 4; ++q) d[q] = f32x4{fb[4 * q], fb[4 * q + 1], fb[4 * q + 2], fb[4 * q + 3]};
    };
    const int n_panels = (k_end - k_begin + TK_ - 1) / TK_;
    const int n_full = inner ? (k_end - k_begin) / TK_ : 0;            // panels the bounds-free pipeline takes; the rest (a K tail, edge tiles) go one by one
    // a wave's 64 x 64 quarter as 2 x 2 MFMA tiles that INTERLEAVE: tile (a, b) = its rows 2 m + a, its columns 2 n + b -- a lane's two A
    // (two B) operands of a k-step then sit side by side in LDS (one 8-byte read each) and its results pair up into 8-byte stores
    const int wi = (wave / WCOLS) * 64 + 2 * (lane & 31), wj = (wave % WCOLS) * 64 + 2 * (lane & 31), kh = lane >> 5;
    const bool wave_live = j0 + (wave % WCOLS) * 64 < g.N;       // a narrow matrix leaves some of the tile's waves without columns
    // the MFMAs of one panel in LDS[buf].  The operands of k-step s + 1 are asked for BEFORE the four MFMAs of step s are issued (the
    // scheduling barriers keep the compiler from sinking the reads back down to their use, which leaves the matrix pipe idle for an LDS
    // round trip every step)
    auto compute = [&](int buf) {
        if (!wave_live) return;
        f32x2 av[2], bv[2];
        av[0] = *reinterpret_cast<const f32x2 *>(&As[buf][kh][wi]); bv[0] = *reinterpret_cast<const f32x2 *>(&Bs[buf][kh][wj]);
#pragma unroll
        for (int st = 0; st < TK_ / 2; ++st) {
            const int c = st & 1, n = c ^ 1;
            if (st + 1 < TK_ / 2) {
                const int kk = 2 * (st + 1) + kh;
                av[n] = *reinterpret_cast<const f32x2 *>(&As[buf][kk][wi]); bv[n] = *reinterpret_cast<const f32x2 *>(&Bs[buf][kk][wj]);
            }
            __builtin_amdgcn_sched_barrier(0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c].x, bv[c].x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c].x, bv[c].y, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c].y, bv[c].x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c].y, bv[c].y, acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto fetch_fast = [&](int k0, float *fa, float *fb) {
        const float *ga = A_KCONTIG ? g.A + (size_t)(i0 + a_row) * g.lda + k0 + a_off : g.A + (size_t)(k0 + a_row) * g.lda + i0 + a_off;
        fetch_run<FA, true>(ga, true, 0, 0, fa);
        fetch_run<FB, true>(g.B + (size_t)(k0 + b_row) * g.ldb + j0 + b_off, true, 0, 0, fb);
    };
    // Two panels are in flight from memory at any time: panel kt feeds the MFMAs from LDS, panel kt + 1 waits in one register set for its
    // turn to go into LDS, panel kt + 2 is on its way into the other.  With the bounds-free loads the steady-state loop has no branch around
    // a load, so the wait in front of the LDS stores covers panel kt + 1 only (s_waitcnt vmcnt(loads of one panel)), not the panel just
    // asked for.  Panels [first, last) of this workgroup's K range.
    auto pipeline = [&](auto fast_tag, int first, int last) {
        constexpr bool FAST = decltype(fast_tag)::value;
        auto get = [&](int kt, float *fa, float *fb) { if (FAST) fetch_fast(k_begin + kt * TK_, fa, fb); else fetch(k_begin + kt * TK_, fa, fb); };
        if (first >= last) return;
        get(first, ra[0], rb[0]); stash(0, ra[0], rb[0]);
        if (first + 1 < last) get(first + 1, ra[1], rb[1]);
        __syncthreads();
        int kt = first;                                               // LDS buffer of panel kt = (kt - first) & 1
        for (; kt + 3 < last; kt += 2) {
            get(kt + 2, ra[0], rb[0]); compute(0); stash(1, ra[1], rb[1]); __syncthreads();
            get(kt + 3, ra[1], rb[1]); compute(1); stash(0, ra[0], rb[0]); __syncthreads();
        }
        for (; kt < last; ++kt) {                                     // the last two or three panels: nothing left to ask for behind them
            const int buf = (kt - first) & 1;
            if (kt + 2 < last) { if (buf) get(kt + 2, ra[1], rb[1]); else get(kt + 2, ra[0], rb[0]); }
            compute(buf);
            if (kt + 1 < last) { if (buf) stash(0, ra[0], rb[0]); else stash(1, ra[1], rb[1]); }
            __syncthreads();
        }
    };
    pipeline(std::true_type{}, 0, n_full);
    pipeline(std::false_type{}, n_full, n_panels);                    // a K tail; every panel of a tile on the matrix's edge
    gemm_epilogue<TN_>(g, C, acc, i0, j0, wave, lane);
    if (want_colsum) {                                        // the panel rows a column was spread over, added up in a fixed order
        float (*red)[LROWB_] = Bs[0];
#pragma unroll
        for (int q = 0; q < FB; ++q) red[b_row][b_off + q] = cs[q];
        gemm_colsum_sum<TN_, TK_, LROWB_>(g, red, j0, bz);
    }
}

template <bool A_KCONTIG, int TN_, int TK_, int WAVES_PER_EU = 2>
__global__ __launch_bounds__(TN_ * 2) __attribute__((amdgpu_waves_per_eu(WAVES_PER_EU, 8))) void gemm_kernel(GemmArgs g) {
    int bx, by, bz;
    gemm_place(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), gridDim.x, gridDim.y, gridDim.z, bx, by, bz);
    gemm_body<A_KCONTIG, TN_, TK_>(g, bx, by, bz);
}

void launch_gemm(hipStream_t st, bool a_kcontig, GemmArgs g, int n_split) {
    if (n_split == 1) g.k_chunk = g.K;
    g.aligned = (g.lda % 4 == 0) && (g.ldb % 4 == 0) && (((uintptr_t)g.A | (uintptr_t)g.B) % 16 == 0);
    if (a_kcontig && n_split > 1 && g.k_chunk % 4 != 0) g.aligned = 0;      // range z starts z * k_chunk floats into A's rows (the dW form starts at whole rows)
    const long long rows_max = 65535LL * TM, M = g.M;
    for (long long r0 = 0; r0 < M; r0 += rows_max) {
        GemmArgs h = g;
        h.A = g.A + (a_kcontig ? (size_t)r0 * g.lda : (size_t)r0); h.C = g.C + (size_t)r0 * g.ldc; h.M = (int)std::min<long long>(rows_max, M - r0);
        if (g.mask) h.mask = g.mask + (size_t)r0 * g.ldmask;
        const dim3 grid((h.N + 127) / 128, (h.M + TM - 1) / TM, (unsigned)n_split);
        if (g.precision == NTX_PRECISION_BF16X6) launch_gemm_bf16x6(st, a_kcontig, h, grid);      // the same tiles, grid and arguments: the second body
        else if (a_kcontig) hipLaunchKernelGGL((gemm_kernel<true, 128, 16>), grid, dim3(256), 0, st, h);
        else hipLaunchKernelGGL((gemm_kernel<false, 128, 16>), grid, dim3(256), 0, st, h);
    }
}
}   // namespace ntx_train

/* The contraction on caller buffers (DEVICE): C[M][N] = op(A) . op(B) (+ bias) (ReLU), op = identity or transpose as
 * a_kcontig / b_kcontig say (see gemm_kernel).  For tests and benches of the kernel itself. */
extern "C" int ntx_gemm_f32(const float *A, int lda, int a_kcontig, const float *B, int ldb, int b_kcontig, float *C, int ldc, int M, int N, int K, const float *bias, int relu,
                            ntx_stream stream) {
    if (!A || !B || !C || M < 1 || N < 1 || K < 1) return ntx_set_error(NTX_E_INVALID, "bad GEMM arguments");
    ntx_train::GemmArgs g{}; g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.bias = bias; g.relu = relu;
    if (b_kcontig) return ntx_set_error(NTX_E_UNSUPPORTED, "B must be [K][N]");
    ntx_train::launch_gemm((hipStream_t)stream, a_kcontig != 0, g);
    TRAIN_TRY(hipGetLastError());
    return NTX_OK;
}

/* The launcher's whole argument list on caller buffers (DEVICE): every field of GemmArgs and the K split, see include/nerftex.h.  Every
 * refusal comes before the first launch.  For tests and benches of the kernel itself; precision: the body (ntx_precision). */
static int gemm_ex(int precision, const float *A, int lda, int a_kcontig, const float *B, int ldb, float *C, int ldc, int M, int N, int K, const float *bias, int relu,
                   const float *mask, int ldmask, int accumulate, int n_split, int k_chunk, int64_t split_stride, float *colsum, ntx_stream stream) {
    if (!A || !B || !C || M < 1 || N < 1 || K < 1) return ntx_set_error(NTX_E_INVALID, "bad GEMM arguments");
    if (lda < (a_kcontig ? K : M) || ldb < N || ldc < N || (mask && ldmask < N)) return ntx_set_error(NTX_E_INVALID, "a leading dimension is smaller than its row");
    if (n_split < 1 || n_split > 65535) return ntx_set_error(NTX_E_INVALID, "n_split must be 1 .. 65535");
    if (n_split > 1) {
        if (k_chunk < 1 || (long long)K <= (long long)(n_split - 1) * k_chunk || (long long)K > (long long)n_split * k_chunk)
            return ntx_set_error(NTX_E_INVALID, "K must end inside the last of n_split ranges of k_chunk");
        if ((long long)split_stride < (long long)(M - 1) * ldc + N) return ntx_set_error(NTX_E_INVALID, "split_stride is shorter than one result");
    }
    if (colsum && a_kcontig) return ntx_set_error(NTX_E_INVALID, "column sums are taken in the form A [K][M] only");
    ntx_train::GemmArgs g{}; g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.bias = bias; g.relu = relu;
    g.mask = mask; g.ldmask = ldmask; g.accumulate = accumulate; g.k_chunk = k_chunk; g.split_stride = n_split > 1 ? (long long)split_stride : 0; g.colsum = colsum;
    g.precision = precision;
    ntx_train::launch_gemm((hipStream_t)stream, a_kcontig != 0, g, n_split);
    TRAIN_TRY(hipGetLastError());
    return NTX_OK;
}
extern "C" int ntx_gemm_f32_ex(const float *A, int lda, int a_kcontig, const float *B, int ldb, float *C, int ldc, int M, int N, int K, const float *bias, int relu,
                               const float *mask, int ldmask, int accumulate, int n_split, int k_chunk, int64_t split_stride, float *colsum, ntx_stream stream) {
    return gemm_ex(NTX_PRECISION_F32, A, lda, a_kcontig, B, ldb, C, ldc, M, N, K, bias, relu, mask, ldmask, accumulate, n_split, k_chunk, split_stride, colsum, stream);
}
/* ... and through the bf16x6 body (ntx_gemm_bf16x6.hip), on the null stream: the same refusals, the same order */
extern "C" int ntx_gemm_bf16x6_ex(const float *A, int lda, int a_kcontig, const float *B, int ldb, float *C, int ldc, int M, int N, int K, const float *bias, int relu,
                                  const float *mask, int ldmask, int accumulate, int n_split, int k_chunk, int64_t split_stride, float *colsum) {
    return gemm_ex(NTX_PRECISION_BF16X6, A, lda, a_kcontig, B, ldb, C, ldc, M, N, K, bias, relu, mask, ldmask, accumulate, n_split, k_chunk, split_stride, colsum, nullptr);
}
