// ntx_gemm_bf16x6.hip -- the contraction of ntx_gemm.hip on the 16-bit matrix cores, float32-grade: the second body behind launch_gemm
// (GemmArgs::precision = NTX_PRECISION_BF16X6), same contract, same tiles, same grid.  gfx950 only.
//   C[i][j] = sum_p A'(i, p) B(p, j),  A'(i, p) = A_KCONTIG ? A[i * lda + p] : A[p * lda + i],  B[p * ldb + j]
// THE ARITHMETIC.  Both operands stay float32 in memory.  On the way from registers into LDS every value is split into three bf16 terms,
//   v0 = bf16_rne(v),  v1 = bf16_rne(v - v0),  v2 = bf16_rne(v - v0 - v1)          (the subtractions in float32: both are exact)
// and the six products of order <= 2 are taken by v_mfma_f32_32x32x16_bf16 into float32: a0b2, a1b1, a2b0, a0b1, a1b0 -- the small ones, in
// this order, into one accumulator -- and a0b0 into another; the two are added once, behind the last panel, small + large.  A product of two
// bf16 values is exact in float32, v0 + v1 + v2 carries 24 mantissa bits, and bf16 has float32's exponents: what is lost is the three
// products of order 3 and 4 (2^-24 relative and below) and the accumulator's roundings, at every scale of the operands -- no loss scaling,
// no amax pass (tests/bf16x6_common.py restates it in numpy).
// NON-FINITE AND HUGE VALUES.  A NaN in a row of A stays in that row of C (a row of C reads one row of A').  An Inf operand may come out as
// NaN in its row (columns, for B): v - v0 = inf - inf.  A finite value beyond bf16's largest finite one (|v| > 3.3895e38 rounds up) turns
// Inf in v0 and then behaves like an Inf operand.  Subnormal terms are taken as the MFMA takes them.
// STRUCTURE.  A workgroup (4 waves) owns a 128 x 128 tile, a wave a 64 x 64 quarter = 2 x 2 interleaved MFMA tiles, as in ntx_gemm.hip, so
// the epilogue and the column sums are that file's (ntx_gemm_device.h).  K advances a panel of 16 = one MFMA step.  A thread carries one
// RUN of 8 consecutive k of one row of A' and of one column of B -- exactly a lane's operand of the MFMA (lane l: A[row l & 31][k = 8 (l >> 5)
// + 0..7], B[k = ...][col l & 31]) -- so a run is split in registers and stored with one 16-byte write per term, and read with one 16-byte
// read per term and tile.  k-contiguous A comes by two 16-byte loads a run; A [K][M] and B [K][N] by eight 4-byte loads, each coalesced
// across the wave (64 neighbouring floats of one row), which need no alignment.  Two panels are in flight from memory while a third feeds
// the MFMAs (double-buffered LDS, one barrier a panel): 24 MFMAs a wave and panel, the split on the VALU beside them.
// LDS: [buffer][term][k-half][slot] of 16 bytes for A and for B; row / column e of the tile sits at slot (e >> 6) * 72 + (e & 1) * 36 +
// ((e & 63) >> 1): the 32 rows of an interleaved MFMA tile are neighbours (a wave's read is 32 x 16 contiguous bytes a k-half, free of bank
// conflicts), and the two tiles 36 slots apart (8 neighbouring threads write two runs of 64 bytes into different halves of the 128-byte
// bank row).  2 x 3 x 2 x 144 x 16 B = 27 648 B each, 55 296 B a workgroup.
#include <type_traits>
#include "ntx_gemm_device.h"
namespace ntx_train {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int X6_HALF = 144;                     // slots of a k-half: 2 quarters x (2 tiles x 32 + 2 x 4 of padding)

// a run of 8 floats as its three bf16 terms
__device__ __forceinline__ void split3(const float *v, bf16x8 &t0, bf16x8 &t1, bf16x8 &t2) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const __bf16 h0 = (__bf16)v[q];
        const float r1 = v[q] - (float)h0;
        const __bf16 h1 = (__bf16)r1;
        const float r2 = r1 - (float)h1;
        t0[q] = h0; t1[q] = h1; t2[q] = (__bf16)r2;
    }
}
__device__ __forceinline__ int x6_slot(int e) { return (e >> 6) * 72 + (e & 1) * 36 + ((e & 63) >> 1); }

template <bool A_KCONTIG>
__device__ __forceinline__ void gemm_x6_body(const GemmArgs &g, int bx, int by, int bz) {
    constexpr int TN_ = 128, TK_ = 16, LRED = TN_ + 4;
    __shared__ __attribute__((aligned(16))) bf16x8 As[2][3][2][X6_HALF], Bs[2][3][2][X6_HALF];
    static_assert(sizeof(Bs) >= sizeof(float) * TK_ * LRED, "the column sums' scratch lies in Bs");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j0 = bx * TN_, i0 = by * TM;
    const int k_begin = bz * g.k_chunk;
    const int k_end = k_begin + g.k_chunk < g.K ? k_begin + g.k_chunk : g.K;
    float *C = g.C + (size_t)bz * (size_t)g.split_stride;
    f32x16 hi[2][2], lo[2][2];                   // a0b0; the five smaller products
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) { hi[a][b][r] = 0.0f; lo[a][b][r] = 0.0f; }
    float ra[2][8], rb[2][8], cs[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) cs[q] = 0.0f;
    const bool want_colsum = !A_KCONTIG && g.colsum != nullptr && by == 0;
    // the tile lies inside A' and B: only the K end of a panel can stick out (k-contiguous A: and its rows take 16-byte loads)
    const bool inner = i0 + TM <= g.M && j0 + TN_ <= g.N && (!A_KCONTIG || g.aligned);
    // thread -> row e of A' / column e of B within the tile, and the k-half (8 consecutive k) of the panel it carries of both
    const int e = (int)(threadIdx.x & 127), half = (int)(threadIdx.x >> 7);
    const int slot = x6_slot(e);
    const float *a_base = A_KCONTIG ? g.A + (size_t)(i0 + e) * g.lda + 8 * half : g.A + (size_t)(8 * half) * g.lda + i0 + e;
    const float *b_base = g.B + (size_t)(8 * half) * g.ldb + j0 + e;
    auto fetch = [&](auto fast_tag, int k0, float *fa, float *fb) {
        constexpr bool FAST = decltype(fast_tag)::value;
        const int kf = k0 + 8 * half;                                 // the run's first k
        if (A_KCONTIG) fetch_run<8, FAST>(a_base + k0, i0 + e < g.M, kf, k_end, fa, g.aligned != 0);
        else {
            const float *ga = a_base + (size_t)k0 * g.lda;
#pragma unroll
            for (int q = 0; q < 8; ++q) fa[q] = (FAST || (kf + q < k_end && i0 + e < g.M)) ? ga[(size_t)q * g.lda] : 0.0f;
        }
        const float *gb = b_base + (size_t)k0 * g.ldb;
#pragma unroll
        for (int q = 0; q < 8; ++q) fb[q] = (FAST || (kf + q < k_end && j0 + e < g.N)) ? gb[(size_t)q * g.ldb] : 0.0f;
    };
    auto stash = [&](int buf, const float *fa, const float *fb) {
        if (want_colsum) {                                            // the float32 values, per panel row k % 16, in ascending k: ntx_gemm.hip's order
#pragma unroll
            for (int q = 0; q < 8; ++q) cs[q] += fb[q];
        }
        bf16x8 t0, t1, t2;
        split3(fa, t0, t1, t2);
        As[buf][0][half][slot] = t0; As[buf][1][half][slot] = t1; As[buf][2][half][slot] = t2;
        split3(fb, t0, t1, t2);
        Bs[buf][0][half][slot] = t0; Bs[buf][1][half][slot] = t1; Bs[buf][2][half][slot] = t2;
    };
    const int n_panels = (k_end - k_begin + TK_ - 1) / TK_;
    const int n_full = inner ? (k_end - k_begin) / TK_ : 0;            // panels the bounds-free pipeline takes; the rest (a K tail, edge tiles) go with bounds
    const int kh = lane >> 5;
    const int sa = (wave >> 1) * 72 + (lane & 31), sb = (wave & 1) * 72 + (lane & 31);      // the wave's quarter; tile a / b: 36 slots on
    const bool wave_live = j0 + (wave & 1) * 64 < g.N;           // a narrow matrix leaves some of the tile's waves without columns
    auto compute = [&](int buf) {
        if (!wave_live) return;
        bf16x8 av[3][2], bv[3][2];
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int a = 0; a < 2; ++a) { av[t][a] = As[buf][t][kh][sa + 36 * a]; bv[t][a] = Bs[buf][t][kh][sb + 36 * a]; }
        constexpr int order[5][2] = {{0, 2}, {1, 1}, {2, 0}, {0, 1}, {1, 0}};      // smallest first
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) lo[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[order[p][0]][a], bv[order[p][1]][b], lo[a][b], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) hi[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[0][a], bv[0][b], hi[a][b], 0, 0, 0);
    };
    // panel kt feeds the MFMAs from LDS, panel kt + 1 waits in one register set for its turn to go into LDS, panel kt + 2 is on its way
    // into the other (ntx_gemm.hip's pipeline).  Panels [first, last) of this workgroup's K range.
    auto pipeline = [&](auto fast_tag, int first, int last) {
        auto get = [&](int kt, float *fa, float *fb) { fetch(fast_tag, k_begin + kt * TK_, fa, fb); };
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
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = lo[a][b][r] + hi[a][b][r];
    gemm_epilogue<TN_>(g, C, acc, i0, j0, wave, lane);
    if (want_colsum) {
        float (*red)[LRED] = reinterpret_cast<float (*)[LRED]>(&Bs[0][0][0][0]);      // (every wave is behind the last panel's barrier)
#pragma unroll
        for (int q = 0; q < 8; ++q) red[8 * half + q][e] = cs[q];
        gemm_colsum_sum<TN_, TK_, LRED>(g, red, j0, bz);
    }
}

template <bool A_KCONTIG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) void gemm_bf16x6_kernel(GemmArgs g) {
    int bx, by, bz;
    gemm_place(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), gridDim.x, gridDim.y, gridDim.z, bx, by, bz);
    gemm_x6_body<A_KCONTIG>(g, bx, by, bz);
}

void launch_gemm_bf16x6(hipStream_t st, bool a_kcontig, const GemmArgs &g, dim3 grid) {
    if (a_kcontig) hipLaunchKernelGGL(gemm_bf16x6_kernel<true>, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(gemm_bf16x6_kernel<false>, grid, dim3(256), 0, st, g);
}
}   // namespace ntx_train
