// ntx_gemm_device.h -- what the bodies of the contraction share on the device (ntx_gemm.hip: float32 MFMAs; ntx_gemm_bf16x6.hip: three bf16
// terms an operand on the 16-bit MFMAs): the loads of a run of a row, the epilogue on a wave's finished 64 x 64 quarter, the ordered sum
// behind the column sums, and the numbering of the tiles.  Both MFMA shapes leave C in the same registers, so one epilogue serves both.
#pragma once
#include "ntx_trainer.h"
#include "ntx_train_device.h"   // f32x2, f32x4, f32x16
namespace ntx_train {
constexpr int TM = 128;

// n consecutive floats of a row into registers: 16-byte loads, or one by one under a bound
template <int n, bool FAST>
__device__ __forceinline__ void fetch_run(const float *g, bool row_ok, int first, int bound, float *r, bool aligned_ok = false) {
    if (FAST) {
        const f32x4 *v = reinterpret_cast<const f32x4 *>(g);
#pragma unroll
        for (int q = 0; q < n / 4; ++q) { const f32x4 x = v[q]; r[4 * q] = x.x; r[4 * q + 1] = x.y; r[4 * q + 2] = x.z; r[4 * q + 3] = x.w; }
    } else if (row_ok && first + n <= bound && aligned_ok) {         // the run lies inside: vector loads here too
        const f32x4 *v = reinterpret_cast<const f32x4 *>(g);
#pragma unroll
        for (int q = 0; q < n / 4; ++q) { const f32x4 x = v[q]; r[4 * q] = x.x; r[4 * q + 1] = x.y; r[4 * q + 2] = x.z; r[4 * q + 3] = x.w; }
    } else {
#pragma unroll
        for (int q = 0; q < n; ++q) r[q] = (row_ok && first + q < bound) ? g[q] : 0.0f;
    }
}

// The epilogue on a wave's 64 x 64 quarter of the tile at (i0, j0), as 2 x 2 MFMA tiles that INTERLEAVE: tile (a, b) = the quarter's rows
// 2 m + a, its columns 2 n + b.  D of a 32 x 32 tile: lane l, register r  <->  tile row m = 8 (r >> 2) + (r & 3) + 4 (l >> 5), tile column
// n = l & 31; with the interleaved tiles that is row 2 m + a, columns 2 n and 2 n + 1 (b = 0, 1): one 8-byte access per (a, r).
// C[i][j] = acc (+ what was there) + bias[j]; ReLU; 0 where !(mask > 0)
template <int TN_>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs &g, float *C, const f32x16 (&acc)[2][2], int i0, int j0, int wave, int lane) {
    constexpr int WCOLS = TN_ / 64;
    const int kh = lane >> 5;
    const bool whole = i0 + TM <= g.M && j0 + TN_ <= g.N && (g.ldc % 2 == 0) && (!g.mask || g.ldmask % 2 == 0) && ((uintptr_t)C % 8 == 0) && ((uintptr_t)g.mask % 8 == 0);
    const int j = j0 + (wave % WCOLS) * 64 + 2 * (lane & 31);
    const float bj0 = (g.bias && j < g.N) ? g.bias[j] : 0.0f, bj1 = (g.bias && j + 1 < g.N) ? g.bias[j + 1] : 0.0f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + (wave / WCOLS) * 64 + 2 * (8 * (r >> 2) + (r & 3) + 4 * kh) + a;
            float v0 = acc[a][0][r], v1 = acc[a][1][r];
            float *c = C + (size_t)i * g.ldc + j;
            if (whole) {
                f32x2 *c2 = reinterpret_cast<f32x2 *>(c);
                if (g.accumulate) { const f32x2 o = *c2; v0 += o.x; v1 += o.y; }
                v0 += bj0; v1 += bj1;
                if (g.relu) { v0 = v0 > 0.0f ? v0 : 0.0f; v1 = v1 > 0.0f ? v1 : 0.0f; }
                if (g.mask) { const f32x2 mk = *reinterpret_cast<const f32x2 *>(g.mask + (size_t)i * g.ldmask + j); if (!(mk.x > 0.0f)) v0 = 0.0f; if (!(mk.y > 0.0f)) v1 = 0.0f; }
                *c2 = f32x2{v0, v1};
            } else if (i < g.M) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if (j + b >= g.N) continue;
                    float v = b ? v1 : v0;
                    if (g.accumulate) v = v + c[b];
                    v = v + (b ? bj1 : bj0);
                    if (g.relu) v = v > 0.0f ? v : 0.0f;
                    if (g.mask && !(g.mask[(size_t)i * g.ldmask + j + b] > 0.0f)) v = 0.0f;
                    c[b] = v;
                }
            }
        }
}

// the column sums' last step: red[q][j] holds column j's sum over the panel rows q, q + TK_, ... of the range, each added up in ascending
// order by the thread that carried them; here the TK_ of them are added in ascending q.  (The threads have stored to red; this waits for them.)
template <int TN_, int TK_, int LROW>
__device__ __forceinline__ void gemm_colsum_sum(const GemmArgs &g, const float (*red)[LROW], int j0, int bz) {
    __syncthreads();
    if ((int)threadIdx.x < TN_ && j0 + (int)threadIdx.x < g.N) {
        float sum = 0.0f;
        for (int q = 0; q < TK_; ++q) sum += red[q][threadIdx.x];
        g.colsum[(size_t)bz * g.N + j0 + threadIdx.x] = sum;
    }
}

// Which tile of which K range.  The tiles of ONE range read the same panels of A and B: workgroups are dealt to the 8 XCDs round-robin by
// their linear number, each XCD has its own L2 -- so a range's tiles are given numbers that land on one XCD, next to each other in time,
// and the panels come from HBM once instead of once per tile (dW of a 256 x 256 layer: 999 MB a launch at 3.8 TB/s before, for 537 MB of
// operands).  lin: the workgroup's number within its problem; nx x ny tiles, nz ranges (a multiple of 8, or the plain order is kept).
__device__ __forceinline__ void gemm_place(int lin, int nx, int ny, int nz, int &bx, int &by, int &bz) {
    const int tiles = nx * ny;
    if (nz % 8 == 0) {
        const int xcd = lin & 7, slot = lin >> 3, tile = slot % tiles;
        bz = (slot / tiles) * 8 + xcd; bx = tile % nx; by = tile / nx;
    } else { bx = lin % nx; by = (lin / nx) % ny; bz = lin / tiles; }
}
// ntx_gemm_bf16x6.hip: one launch of the bf16x6 body on a grid the launcher (ntx_gemm.hip) has cut
void launch_gemm_bf16x6(hipStream_t st, bool a_kcontig, const GemmArgs &g, dim3 grid);
}   // namespace ntx_train
