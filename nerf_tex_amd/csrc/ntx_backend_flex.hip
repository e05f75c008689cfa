// ntx_backend_flex.hip -- the layer-by-layer backend of a training step (ntx_trainer_create_flex, ntx_trainer_create_flex_ex): any Nerf /
// ParamNerf the flex render family takes (other depths, widths, skips, color_depth; through the _ex entry also param_depth > 0) on row-major
// activations -- flex_encode_kernel, one contraction (ntx_gemm.hip) per Dense layer and pass, the narrow heads on flex_head_*_kernel, a
// parameter branch's output into the concatenations by flex_branch_copy_kernel; where it is asked for (ntx_trainer_enable_param_gradients), dL/d params:
// one more term per reader of the parameter features, then flex_param_fold_kernel / flex_param_rows_kernel.  An instanced step
// (ntx_train_forward_instanced) is the same network on the compact rows of the in-patch samples: flex_encode_samples_kernel in front,
// flex_param_samples_kernel behind.  Where it is asked for (ntx_trainer_enable_input_gradients), dL/d rays_o, rays_d and -- of an instanced
// step -- dL/d pts, rays_d_map: one more term per reader of FF(xyz) / FF(dir), then flex_ray_fold_kernel / flex_input_samples_kernel.
// The handle, the composite, the loss and Adam are ntx_trainer.hip's.  gfx950 only.
#include <algorithm>
#include "ntx_trainer.h"
#include "ntx_encode.h"
namespace ntx_train {
// ---------------------------------------------------------------------------------------------------------------------------
// The small kernels of the layer-by-layer step (ntx_trainer_create_flex): any Nerf / ParamNerf the flex render family takes, one
// gemm_kernel per Dense layer and pass on plain row-major buffers.  A concatenation is a buffer [encoding | hidden] whose two parts
// are written in place: the encoder writes a map at the front of every buffer that starts with it, the layer in front writes behind it.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int FLEX_MAX_DEPTH = 24, FLEX_MAX_COLOR = 4, FLEX_MAX_DST = FLEX_MAX_DEPTH + 1;
constexpr int FLEX_SPLIT = 2048;                       // samples per partial sum of a weight gradient: a function of nothing, so a step's sums do not depend on the trainer's capacity
struct FlexDst { float *p; int ld; };                  // where a map goes: row m starts at p + m * ld
struct FlexEncodeArgs {
    StepRays r; int Kp, Kd;                            // features the encoder writes per map: FF(xyz) and FF(that map's parameters)
    FlexDst pos[FLEX_MAX_DST], dir; int n_pos_dst;
    FlexDst geo_in, app_in;                            // p != NULL: a parameter branch (model.py:88-101) takes that map's parameter features as its input rows
    float *dists;
};
// ntx_encode.h's values as rows [sample][feature]: thread per sample and feature, blockIdx.y = the map
__global__ __launch_bounds__(256) void flex_encode_kernel(FlexEncodeArgs args) {
    const StepRays &a = args.r;
    const int part = blockIdx.y, K = part == 0 ? args.Kp : args.Kd;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.M() * K) return;
    const long long m = e / K, ray = m / a.S;
    const int f = (int)(e - m * K), s = (int)(m - ray * a.S);
    const RayCtx rc = ray_ctx(a.rays_d, a.params, a.rays_per_param_row, ray, a.n_geo + a.n_app);
    const float *zray = a.z + (size_t)ray * a.S;
    bool hit;
    const float z = depth_of(zray[s], hit);
    const int K3 = fourier_width(3, part == 0 ? a.pos_freq : a.dir_freq);
    const bool xyz = f < K3;
    const float v = fourier_row(xyz ? f : f - K3, xyz ? 3 : (part == 0 ? a.n_geo : a.n_app), [&](int c) -> float {
        if (!xyz) return blurred_param(rc.pr, part == 0 ? c : a.n_geo + c, a.blur_idx, hit, a.cone, ray, z);     // model.py:88-93, 96-101
        return part == 0 ? rc.point(a.rays_o[3 * ray + c], c, z) : rc.dir(c);
    });
    const FlexDst &branch = part == 0 ? args.geo_in : args.app_in;
    if (!xyz && branch.p) branch.p[(size_t)m * branch.ld + (f - K3)] = v;                      // the branch's output goes behind FF(xyz) instead: flex_branch_copy_kernel
    else if (part == 0) for (int i = 0; i < args.n_pos_dst; ++i) args.pos[i].p[(size_t)m * args.pos[i].ld + f] = v;
    else {
        args.dir.p[(size_t)m * args.dir.ld + f] = v;
        if (f == 0) args.dists[(size_t)ray * a.S + s] = sample_dist(zray, s, a.S, z, hit, rc.dn);
    }
}

// The same rows for an instanced step (ntx_train_forward_instanced): row i of every destination is live sample m = live[i] of the
// instancer's buffers -- position pts[m], direction rays_d_map[m] as given (renderer.py:265-272 hands it on un-normalised), parameters
// params_map[m], blur_idx's times cone_scale t / patch_scale (:259-263).  Thread per compact row and feature, blockIdx.y = the map; the
// values are ntx_encode.h's fourier_row, as the render side's.  Only live samples are read; the distances stay the caller's.
struct FlexEncodeSamplesArgs {
    StepSamples s; int Kp, Kd;
    FlexDst pos[FLEX_MAX_DST], dir; int n_pos_dst;
    FlexDst geo_in, app_in;
};
__global__ __launch_bounds__(256) void flex_encode_samples_kernel(FlexEncodeSamplesArgs args) {
    const StepSamples &a = args.s;
    const int part = blockIdx.y, K = part == 0 ? args.Kp : args.Kd, P = a.n_geo + a.n_app;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n_live * K) return;
    const long long i = e / K, m = a.live[i], ray = m / a.S;
    const int f = (int)(e - i * K);
    const int K3 = fourier_width(3, part == 0 ? a.pos_freq : a.dir_freq);
    const bool xyz = f < K3;
    const float v = fourier_row(xyz ? f : f - K3, xyz ? 3 : (part == 0 ? a.n_geo : a.n_app), [&](int c) -> float {
        if (xyz) return (part == 0 ? a.pts : a.rays_d_map)[3 * m + c];
        const int col = part == 0 ? c : a.n_geo + c;
        const float p = a.params_map[(size_t)m * P + col];
        return col == a.blur_idx ? p * a.blur_scale(m, ray) : p;
    });
    const FlexDst &branch = part == 0 ? args.geo_in : args.app_in;
    if (!xyz && branch.p) branch.p[(size_t)i * branch.ld + (f - K3)] = v;
    else if (part == 0) for (int q = 0; q < args.n_pos_dst; ++q) args.pos[q].p[(size_t)i * args.pos[q].ld + f] = v;
    else args.dir.p[(size_t)i * args.dir.ld + f] = v;
}

// The output of a parameter branch's last layer, src[m][c] for c < width, behind the FF(xyz) columns of every buffer that starts with the map
// (model.py:93, 101): dst[i].p[m][off + c].  Read once, written n_dst times; thread per element, consecutive threads along the row.  off is
// 63 / 27 at the configs' bands, so the destinations are not 16-byte aligned: dwords
struct FlexBranchCopyArgs { const float *src; int lds, width, off, n_dst; FlexDst dst[FLEX_MAX_DST]; long long M; };
__global__ __launch_bounds__(256) void flex_branch_copy_kernel(FlexBranchCopyArgs a) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.M * a.width) return;
    const long long m = e / a.width; const int c = (int)(e - m * a.width);
    const float v = a.src[(size_t)m * a.lds + c];
    for (int i = 0; i < a.n_dst; ++i) a.dst[i].p[(size_t)m * a.dst[i].ld + a.off + c] = v;
}

// A narrow head (density: 1 column, colour: 3): out[m][c] = b[c] + sum_k X[m][k] W[k][c], K <= 256.  A wave per row, the row's sum
// in the fixed order of the lanes' butterfly.
template <int NOUT>
__global__ __launch_bounds__(256) void flex_head_kernel(const float *__restrict__ X, int ldx, int K, const float *__restrict__ W, const float *__restrict__ b,
                                                        float *__restrict__ out, long long M) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * 4;
    float w[NOUT][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < NOUT; ++c) w[c][q] = lane + 64 * q < K ? W[(lane + 64 * q) * NOUT + c] : 0.0f;
    for (long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); m < M; m += n_waves) {
        float acc[NOUT];
#pragma unroll
        for (int c = 0; c < NOUT; ++c) acc[c] = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x = lane + 64 * q < K ? X[(size_t)m * ldx + lane + 64 * q] : 0.0f;
#pragma unroll
            for (int c = 0; c < NOUT; ++c) acc[c] = fmaf(x, w[c][q], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < NOUT; ++c) { acc[c] = wave_sumf(acc[c]); if (lane == 0) out[(size_t)m * NOUT + c] = acc[c] + b[c]; }
    }
}
// ... its weight gradient over one range of FLEX_SPLIT samples: partial[z][k][c] = sum_m X[m][k] dgrad[m][c0 + c], behind it the bias's
// partial[z][K][c] = sum_m dgrad[m][c0 + c].  1024 threads = G groups of KK >= K threads (KK a power of two >= 64): group g takes the
// range's samples g, g + G, ... in ascending order, thread k of it column k; the groups' sums are added in ascending g through LDS -- an order
// that K and the step's sample count fix.  reduce_batch_kernel adds the ranges up.
template <int NOUT>
__global__ __launch_bounds__(1024) void flex_head_wgrad_kernel(const float *__restrict__ X, int ldx, int K, int KK, const float *__restrict__ dgrad, int c0, long long M,
                                                               float *__restrict__ partial) {
    __shared__ float red[1024 * NOUT], redb[16 * NOUT];
    const int k = threadIdx.x & (KK - 1), g = threadIdx.x / KK, G = 1024 / KK;
    const long long m0 = (long long)blockIdx.x * FLEX_SPLIT, m1 = m0 + FLEX_SPLIT < M ? m0 + FLEX_SPLIT : M;
    float acc[NOUT], bs[NOUT];
#pragma unroll
    for (int c = 0; c < NOUT; ++c) acc[c] = bs[c] = 0.0f;
#pragma unroll 4
    for (long long m = m0 + g; m < m1; m += G) {
        const float x = k < K ? X[(size_t)m * ldx + k] : 0.0f;
#pragma unroll
        for (int c = 0; c < NOUT; ++c) { const float d = dgrad[4 * m + c0 + c]; acc[c] = fmaf(x, d, acc[c]); bs[c] += d; }
    }
#pragma unroll
    for (int c = 0; c < NOUT; ++c) { red[threadIdx.x * NOUT + c] = acc[c]; if (k == 0) redb[g * NOUT + c] = bs[c]; }
    __syncthreads();
    float *p = partial + (size_t)blockIdx.x * ((size_t)K * NOUT + NOUT);
    if (g == 0 && k < K) {
#pragma unroll
        for (int c = 0; c < NOUT; ++c) { float sum = 0.0f; for (int q = 0; q < G; ++q) sum += red[(q * KK + k) * NOUT + c]; p[k * NOUT + c] = sum; }
    }
    if (threadIdx.x < NOUT) { float sum = 0.0f; for (int q = 0; q < G; ++q) sum += redb[q * NOUT + threadIdx.x]; p[K * NOUT + threadIdx.x] = sum; }
}
// ... and the gradient at its input: G[m][k] = sum_c dgrad[m][c0 + c] W[k][c], kept where act[m][k] > 0 (act NULL: everywhere)
template <int NOUT>
__global__ __launch_bounds__(256) void flex_head_dx_kernel(const float *__restrict__ dgrad, int c0, const float *__restrict__ W, int K, const float *__restrict__ act,
                                                           int ldact, float *__restrict__ G, int ldg, long long M) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * K) return;
    const long long m = e / K; const int k = (int)(e - m * K);
    float v = 0.0f;
#pragma unroll
    for (int c = 0; c < NOUT; ++c) v = fmaf(dgrad[4 * m + c0 + c], W[k * NOUT + c], v);
    if (act && !(act[(size_t)m * ldact + k] > 0.0f)) v = 0.0f;
    G[(size_t)m * ldg + k] = v;
}
// The hidden rows of every kernel transposed, once a step: wt[dst + j * hid + r] = w[src + r * out + j] -- the [K][N] operand of
// dX = dY . W^T (the encoding rows of a layer behind a concatenation take no gradient further and are left out)
struct FlexTSeg { long long src, dst, first, count; int hid, out; };
__global__ void flex_transpose_kernel(const float *__restrict__ w, float *__restrict__ wt, const FlexTSeg *__restrict__ seg, int n_seg, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg[mid].first <= e) lo = mid; else hi = mid - 1; }
    const FlexTSeg &s = seg[lo];
    const long long o = e - s.first;
    if (o >= s.count) return;
    const int j = (int)(o / s.hid), r = (int)(o - (long long)j * s.hid);
    wt[s.dst + o] = w[s.src + (size_t)r * s.out + j];
}

// ---------------------------------------------------------------------------------------------------------------------------
// dL/d params (ntx_trainer_enable_param_gradients).  The way back leaves the gradient at the parameter FEATURES of every sample,
// PG_geo[M][ld_geo] / PG_app[M][ld_app] in the rows of FourierFeatures(parameters); the fold takes a sample's row through the encoder's
// derivative -- the identity row plus, per band, slope(sin row) and slope(cos row) at the value x the encoder fed (blurred_param), times the
// sample's cone_scale z for blur_idx (renderer.py:155-158) -- and adds the samples of a ray: a wave per ray, lane l the samples l, l + 64, ...
// in ascending order, then the lanes' butterfly.  A wave's 64 samples are 64 consecutive rows of PG, one contiguous range: every line it
// fetches is used whole over the loop along the row.  A sample of a ray that misses (z not finite) is SELECTED to 0, never multiplied:
// its cone_scale may be NaN.  flex_param_rows_kernel then adds the rays of a parameter row in ascending ray order: neither sum depends on the
// grid or on the trainer's capacity.
// ---------------------------------------------------------------------------------------------------------------------------
struct FlexFoldArgs { StepRays r; const float *pg_geo, *pg_app; int ld_geo, ld_app; float *ray_pg; };      // ray_pg [n_rays][P], geometry columns first
__global__ __launch_bounds__(256) void flex_param_fold_kernel(FlexFoldArgs args) {
    const StepRays &a = args.r;
    const int lane = threadIdx.x & 63, P = a.n_geo + a.n_app;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    const RayCtx rc = ray_ctx(a.rays_d, a.params, a.rays_per_param_row, ray, P);
    const float *zray = a.z + (size_t)ray * a.S;
    for (int c = 0; c < P; ++c) {
        const bool geo = c < a.n_geo;
        const int D = geo ? a.n_geo : a.n_app, cc = geo ? c : c - a.n_geo, ld = geo ? args.ld_geo : args.ld_app;
        const float *pg = (geo ? args.pg_geo : args.pg_app) + (size_t)ray * a.S * ld;
        float acc = 0.0f;
        for (int s = lane; s < a.S; s += 64) {
            bool hit;
            const float z = depth_of(zray[s], hit);
            const float x = blurred_param(rc.pr, c, a.blur_idx, hit, a.cone, ray, z);
            const float *row = pg + (size_t)s * ld;
            float v = row[cc];
            for (int f = 0; f < a.param_freq; ++f) {
                v = fmaf(fourier_slope(x, f, 0), row[fourier_row_of(D, f, 0, cc)], v);
                v = fmaf(fourier_slope(x, f, 1), row[fourier_row_of(D, f, 1, cc)], v);
            }
            if (c == a.blur_idx && hit) v *= a.cone[ray] * z;
            acc += hit ? v : 0.0f;
        }
        acc = wave_sumf(acc);
        if (lane == 0) args.ray_pg[(size_t)ray * P + c] = acc;
    }
}
// param_grad[row][c] = the sum of ray_pg[r][c] over the row's rays r = row * rays_per_param_row ..., ascending (the last row may be short)
__global__ __launch_bounds__(256) void flex_param_rows_kernel(const float *__restrict__ ray_pg, long long n_rays, long long rays_per_param_row, int P, long long rows,
                                                              float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * P) return;
    const long long row = e / P, r0 = row * rays_per_param_row, r1 = r0 + rays_per_param_row < n_rays ? r0 + rays_per_param_row : n_rays;
    const int c = (int)(e - row * P);
    float sum = 0.0f;
#pragma unroll 8
    for (long long r = r0; r < r1; ++r) sum += ray_pg[(size_t)r * P + c];
    out[e] = sum;
}
// The fold of an instanced step: nothing is added up -- every sample has parameters of its own (params_map), so out[m][c] is live sample m's
// row of PG (compact row row_of[m]) through the same derivative, times cone_scale t / patch_scale for blur_idx; a sample that is not live
// is written as 0 and nothing of it is read.  Thread per (sample, parameter).
struct FlexSampleFoldArgs { StepSamples s; const float *pg_geo, *pg_app; int ld_geo, ld_app; float *out; };       // out [N][S][P], geometry columns first
__global__ __launch_bounds__(256) void flex_param_samples_kernel(FlexSampleFoldArgs args) {
    const StepSamples &a = args.s;
    const int P = a.n_geo + a.n_app;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.M() * P) return;
    const long long m = e / P;
    const int c = (int)(e - m * P), row_i = a.row_of[m];
    float v = 0.0f;
    if (row_i >= 0) {
        const bool geo = c < a.n_geo;
        const int D = geo ? a.n_geo : a.n_app, cc = geo ? c : c - a.n_geo, ld = geo ? args.ld_geo : args.ld_app;
        const float *row = (geo ? args.pg_geo : args.pg_app) + (size_t)row_i * ld;
        const float scale = c == a.blur_idx ? a.blur_scale(m, m / a.S) : 1.0f;
        const float p = a.params_map[(size_t)m * P + c], x = c == a.blur_idx ? p * scale : p;
        v = row[cc];
        for (int f = 0; f < a.param_freq; ++f) {
            v = fmaf(fourier_slope(x, f, 0), row[fourier_row_of(D, f, 0, cc)], v);
            v = fmaf(fourier_slope(x, f, 1), row[fourier_row_of(D, f, 1, cc)], v);
        }
        if (c == a.blur_idx) v *= scale;
    }
    args.out[e] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// dL/d rays_o, rays_d and dL/d pts, rays_d_map (ntx_trainer_enable_input_gradients).  The way back leaves the gradient at the FF(xyz) rows
// and the FF(dir) rows of every sample, IG_pos[M][ld_pos] / IG_dir[M][ld_dir]; a row goes through the encoder's derivative to a 3-vector --
// component c: the identity row plus, per band, slope(sin row) and slope(cos row) at the value x_c the encoder fed (RayCtx::point /
// RayCtx::dir) --, a_s for the position and b_s for the direction.  The sample depths are constants (renderer.py:129).
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fourier_back3(const float *row, int L, int c, float x) {
    float v = row[c];
    for (int f = 0; f < L; ++f) {
        v = fmaf(fourier_slope(x, f, 0), row[fourier_row_of(3, f, 0, c)], v);
        v = fmaf(fourier_slope(x, f, 1), row[fourier_row_of(3, f, 1, c)], v);
    }
    return v;
}
// The ray fold of a plain step, flex_param_fold_kernel's sibling: a wave per ray, lane l the samples l, l + 64, ... in ascending order, then
// the lanes' butterfly; a wave's 64 samples are 64 consecutive rows of IG_pos and of IG_dir.  With n = d / |d| and B = sum_s b_s:
//     d_rays_o = sum_s a_s,    d_rays_d = sum_s z_s a_s + (B - n (n . B)) / |d| + n dL/d|d|
// dL/d|d| is the composite's dists = dz |d| (renderer.py:180): dL/d dist_s dist_s = dL/d sigma_s relu(sigma_s + noise_s), and dgrad[s][3]
// is 0 where that ReLU is closed, so dL/d|d| = (sum_s dgrad[s][3] (sigma_s + noise_s)) / |d|.  A sample of a ray that misses (z not finite)
// is SELECTED to 0, and so are both rows of a ray without a sample that hits: its cone_scale and its cotangent may be anything.  No sum
// depends on the grid or on the trainer's capacity.
struct FlexRayFoldArgs { StepRays r; const float *ig_pos, *ig_dir; int ld_pos, ld_dir; const float *dgrad, *sigma, *noise; float *d_rays_o, *d_rays_d; };
__global__ __launch_bounds__(256) void flex_ray_fold_kernel(FlexRayFoldArgs args) {
    const StepRays &a = args.r;
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    const RayCtx rc = ray_ctx(a.rays_d, a.params, a.rays_per_param_row, ray, a.n_geo + a.n_app);
    const float *zray = a.z + (size_t)ray * a.S;
    const float o[3] = {a.rays_o[3 * ray], a.rays_o[3 * ray + 1], a.rays_o[3 * ray + 2]};
    const float *gp = args.ig_pos + (size_t)ray * a.S * args.ld_pos, *gd = args.ig_dir + (size_t)ray * a.S * args.ld_dir;
    const size_t m0 = (size_t)ray * a.S;
    float sa[3] = {0.0f, 0.0f, 0.0f}, sza[3] = {0.0f, 0.0f, 0.0f}, sb[3] = {0.0f, 0.0f, 0.0f}, q = 0.0f;
    bool any = false;
    for (int s = lane; s < a.S; s += 64) {
        bool hit;
        const float z = depth_of(zray[s], hit);
        any = any || hit;
        const float *prow = gp + (size_t)s * args.ld_pos, *drow = gd + (size_t)s * args.ld_dir;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float av = fourier_back3(prow, a.pos_freq, c, rc.point(o[c], c, z));
            const float bv = fourier_back3(drow, a.dir_freq, c, rc.dir(c));
            sa[c] += hit ? av : 0.0f; sza[c] += hit ? z * av : 0.0f; sb[c] += hit ? bv : 0.0f;
        }
        const float sg = args.noise ? args.sigma[m0 + s] + args.noise[m0 + s] : args.sigma[m0 + s];
        const float dq = args.dgrad[4 * (m0 + s) + 3] * sg;
        q += hit ? dq : 0.0f;
    }
    any = __any(any) != 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { sa[c] = wave_sumf(sa[c]); sza[c] = wave_sumf(sza[c]); sb[c] = wave_sumf(sb[c]); }
    q = wave_sumf(q);
    if (lane < 3) {
        const float n[3] = {rc.dir(0), rc.dir(1), rc.dir(2)};
        const float nb = (n[0] * sb[0] + n[1] * sb[1]) + n[2] * sb[2], dlen = q / rc.dn;
        const float go = lane == 0 ? sa[0] : lane == 1 ? sa[1] : sa[2];
        const float gz = lane == 0 ? sza[0] : lane == 1 ? sza[1] : sza[2], gb = lane == 0 ? sb[0] : lane == 1 ? sb[1] : sb[2];
        const float nc = lane == 0 ? n[0] : lane == 1 ? n[1] : n[2];
        const float gd3 = (gz + (gb - nc * nb) / rc.dn) + nc * dlen;
        args.d_rays_o[3 * ray + lane] = any ? go : 0.0f;
        args.d_rays_d[3 * ray + lane] = any ? gd3 : 0.0f;
    }
}
// The same of an instanced step, flex_param_samples_kernel's sibling: nothing is added up -- d_pts[m] = a and d_dirs[m] = b of live sample m's
// compact row (the direction is fed as given: no normalisation term; dists are the caller's: no |d| term); a sample that is not live is
// written as 0 and nothing of it is read.  Thread per (sample, component): 0..2 the position's, 3..5 the direction's.
struct FlexSampleInputArgs { StepSamples s; const float *ig_pos, *ig_dir; int ld_pos, ld_dir; float *d_pts, *d_dirs; };
__global__ __launch_bounds__(256) void flex_input_samples_kernel(FlexSampleInputArgs args) {
    const StepSamples &a = args.s;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.M() * 6) return;
    const long long m = e / 6;
    const int k = (int)(e - m * 6), c = k < 3 ? k : k - 3, row_i = a.row_of[m];
    float v = 0.0f;
    if (row_i >= 0) {
        if (k < 3) v = fourier_back3(args.ig_pos + (size_t)row_i * args.ld_pos, a.pos_freq, c, a.pts[3 * m + c]);
        else v = fourier_back3(args.ig_dir + (size_t)row_i * args.ld_dir, a.dir_freq, c, a.rays_d_map[3 * m + c]);
    }
    (k < 3 ? args.d_pts : args.d_dirs)[3 * m + c] = v;
}
}   // namespace ntx_train
namespace {
using namespace ntx_train;
// A Dense layer with an activation buffer of its own: trunk 0 .. depth-1, the feature layer, the colour layers, the colour half layer
// (model.py:104-122).  Its input X is the buffer of the layer in front -- [encoding | hidden] where a concatenation lies between them
// (a skip: pos_map, model.py:107-108; the feature layer: dir_map, :115) --, its output goes to Y = its own buffer behind the encoding
// columns of the concatenation that follows it.
struct FlexLayer {
    int in = 0, out = 0, enc = 0, src = -1, relu = 0;   // enc: the leading input rows that are an encoding (no gradient further); src: the layer whose output the others are
    size_t w = 0, b = 0;                                // offsets into the Keras-order blob
    const float *X = nullptr; int ldx = 0;
    float *Y = nullptr; int ldy = 0;
    long long wt = -1;                                  // its transposed hidden rows [out][in - enc] in FlexBackend::wt
    long long bwt = -1;                                 // a consumer of a parameter branch: its transposed branch rows [out][param_width] in FlexBackend::wt
    long long pwt = -1;                                 // parameter gradients on: a reader of parameter features, its transposed feature rows [out][n_in]; a branch's layer 0, its kernel whole
    long long xwt = -1;                                 // input gradients on: a reader of pos_map / dir_map, its transposed FF(xyz) / FF(dir) rows [out][K3]
};
// A parameter branch (model.py:88-93 geometry, 96-101 appearance): param_depth Dense(param_width, relu) layers on FF(parameters), per sample
// (with blur_idx on one of its parameters the input differs from sample to sample).  Layer j's X is the input buffer / layer j - 1's Y; every Y
// is a buffer of its own [M][pad4(param_width)]: the ReLU mask on the way back.  Its consumers read copies of the last Y in their own rows.
struct FlexBranch {
    std::vector<FlexLayer> layers;
    float *in = nullptr; int ld_in = 0, n_in = 0, off = 0;      // the input rows [M][ld_in], n_in features; off: the columns of FF(xyz) in front of it in a map
    int consumers_met = 0;                                      // of the current way back
    bool exists() const { return !layers.empty(); }
};

struct FlexBackend : Backend {
    ntx_trainer *t = nullptr;
    std::vector<FlexLayer> layers;
    std::vector<int> relu_layers;                       // the oracle's mask order: trunk, colour hidden layers, colour half
    TLayer rgb{}, alpha{};
    int last_trunk = 0, half = 0;                       // indices into layers
    FlexBranch geo, app; int pw = 0, ldb = 0;           // the parameter branches, param_width and the rows of their buffers
    int Kp = 0, Kd = 0, enc_Kp = 0, enc_Kd = 0;         // features of pos_map / dir_map as the layers see them; as the encoder writes them (the same without branches)
    int ldg = 0;
    float *G[2] = {nullptr, nullptr};                   // the gradient at a layer's output, ping-pong
    float *BG[2] = {nullptr, nullptr};                  // ... at a branch layer's output [M][ldb] (param_width may be larger than width)
    float *wt = nullptr; FlexTSeg *tseg = nullptr; int n_tseg = 0; long long t_total = 0;
    std::vector<FlexTSeg> segs;                         // the table on the host: enable_param_gradients appends to it
    float *PG[2] = {nullptr, nullptr}; int ldpg[2] = {0, 0}, pg_met[2] = {0, 0};      // the gradient at the geometry / appearance parameter features [M][pad4(n_in)]; readers met on this way back
    float *ray_pg = nullptr;                            // [cap_rays][P]: a ray's samples folded and added
    float *IG[2] = {nullptr, nullptr}; int ldig[2] = {0, 0}, ig_met[2] = {0, 0}, K3[2] = {0, 0};       // the gradient at the FF(xyz) / FF(dir) rows [M][pad4(K3)]; readers met on this way back
    float *partial = nullptr, *colsum = nullptr;        // [n_split][in * out], [n_split][out] of the layer whose weight gradient is being taken
    FlexDst pos_dst[FLEX_MAX_DST]; int n_pos_dst = 0; FlexDst dir_dst{};
    size_t plan(const ntx_model_desc *d, int param_depth, int param_width);
    void place();
    void branch_forward(const FlexBranch &b, const FlexDst *dst, int n_dst, long long M, hipStream_t st);
    void branch_term(FlexBranch &b, const FlexLayer &consumer, const float *dY, long long M, hipStream_t st);
    void branch_backward(const FlexBranch &b, long long M, int n_split, hipStream_t st);
    void param_term(int group, long long pwt, int n_in, const float *dY, int lddy, int K, long long M, hipStream_t st);
    void seg(long long &slot, size_t src, int rows, int out);
    int enable_param_gradients() override;
    int enable_input_gradients() override;
    void input_term(int group, const FlexLayer &l, const float *dY, long long M, hipStream_t st);
    void reduce(hipStream_t st, int n_split, const float *part, long long count, size_t out, const float *bias_partial, long long bias_count, size_t bias_out);
    void network_forward(long long M, hipStream_t st);                      // the rows are encoded: branches, layers, heads on M rows
    void network_backward(long long M, hipStream_t st);                     // dgrad [M][4] -> the weight gradients, the gradient at the parameter features
    int forward(const StepRays &r, hipStream_t st) override;
    int backward(const StepRays &r, hipStream_t st) override;
    int takes_samples() override { return NTX_OK; }
    int forward_samples(const StepSamples &s, hipStream_t st) override;
    int backward_samples(const StepSamples &s, float *sample_pg, hipStream_t st) override;
    int activation(int layer, int64_t n_samples_total, float *out_host) override;
};

// the layers of the architecture in forward order with their places in the Keras-order blob (ntx_arch.h: view_blob); returns the blob's floats
size_t FlexBackend::plan(const ntx_model_desc *d, int param_depth, int param_width) {
    ntx_model_desc_ex x{};                                                   // (the handle keeps the base struct and the two fields behind it: put together again for flex_arch_of)
    x.base = *d; x.param_depth = param_depth; x.param_width = param_width;
    if (param_depth > 0) x.base.kind = NTX_MODEL_PARAMNERF_EX;
    const ntx::Dims dm = ntx::dims_of(d);
    const ntx::BlobView n = ntx::view_blob(param_depth > 0 ? ntx::flex_arch_of(&x.base) : ntx::trunk_arch_of(d), dm);
    const int depth = (int)n.trunk.size(), cd = (int)n.colour.size();
    Kp = n.pos_map; Kd = n.dir_map; enc_Kp = ntx::pos_map_m(dm, 0); enc_Kd = ntx::dir_map_m(dm);
    pw = param_depth > 0 ? param_width : 0;
    auto branch = [&](FlexBranch &b, const std::vector<TLayer> &ls, int n_act, int off) {
        for (const TLayer &t : ls) { FlexLayer l; l.in = t.in; l.out = t.out; l.relu = 1; l.w = t.w; l.b = t.b; b.layers.push_back(l); }
        b.n_in = ntx::par_emb_m(n_act, dm); b.off = off;
    };
    branch(geo, n.pgeo, dm.g, ntx::pos_emb_m(dm, 0)); branch(app, n.papp, dm.a, ntx::dir_emb_m(dm));
    auto add = [&](const TLayer &t, int enc, int src, int relu) {
        FlexLayer l; l.in = t.in; l.out = t.out; l.enc = enc; l.src = src; l.relu = relu; l.w = t.w; l.b = t.b;
        layers.push_back(l);
        if (relu) relu_layers.push_back((int)layers.size() - 1);
    };
    for (int i = 0; i < depth; ++i) add(n.trunk[i], i == 0 ? n.pos_map : n.trunk[i].in - d->width, i - 1, 1);   // enc: pos_map, also where a skip concatenates it (model.py:107-108)
    last_trunk = depth - 1;
    add(n.feature, 0, depth - 1, 0);                                         // the feature layer: no activation (model.py:114)
    for (int i = 0; i < cd; ++i) add(n.colour[i], i == 0 ? n.dir_map : 0, depth + i, 1);
    add(n.c2, cd > 0 ? 0 : n.dir_map, depth + cd, 1);                        // :122
    half = (int)layers.size() - 1;
    rgb = n.rgb; alpha = n.alpha;
    return n.count;
}

// a buffer per layer, [the encoding of the concatenation behind it | its output], rows padded to 16 bytes; the first layer reads pos_map.
// Then the branches' buffers, the gradients' ping-pongs, the weight gradients' partial sums and the transposed kernels with their table
void FlexBackend::place() {
    DeviceMemory &mem = t->mem;
    const ntx_model_desc &d = t->desc;
    const long long M = t->cap;
    const unsigned skips = ntx::trunk_skips(&d);
    float *pos = nullptr;
    mem.alloc(&pos, (size_t)M * pad4(Kp));
    pos_dst[n_pos_dst++] = FlexDst{pos, pad4(Kp)};
    std::vector<float *> base(layers.size(), nullptr);
    size_t most_dw = 1024;                                                 // (the heads' partial sums: at most 128 x 3 + 3 floats a range)
    for (size_t i = 0; i < layers.size(); ++i) {
        FlexLayer &l = layers[i];
        const int front = (int)i < d.depth ? (((skips >> i) & 1u) ? Kp : 0) : ((int)i == d.depth ? Kd : 0);
        l.ldy = pad4(front + l.out);
        mem.alloc(&base[i], (size_t)M * l.ldy);
        l.Y = base[i] ? base[i] + front : nullptr;
        if ((int)i < d.depth && front) pos_dst[n_pos_dst++] = FlexDst{base[i], l.ldy};
        if ((int)i == d.depth) dir_dst = FlexDst{base[i], l.ldy};
        if (i == 0) { l.X = pos; l.ldx = pad4(Kp); }
        else { l.X = base[l.src]; l.ldx = layers[l.src].ldy; }                              // (the whole row: encoding columns first, as the kernel's rows are)
        most_dw = std::max(most_dw, (size_t)l.in * l.out);
    }
    ldg = pad4(d.width);
    mem.alloc(&G[0], (size_t)M * ldg); mem.alloc(&G[1], (size_t)M * ldg);
    ldb = pad4(pw);
    for (FlexBranch *b : {&geo, &app}) {
        if (!b->exists()) continue;
        b->ld_in = pad4(b->n_in);
        mem.alloc(&b->in, (size_t)M * b->ld_in);
        for (size_t j = 0; j < b->layers.size(); ++j) {
            FlexLayer &l = b->layers[j];
            l.ldy = ldb; mem.alloc(&l.Y, (size_t)M * ldb);
            if (j == 0) { l.X = b->in; l.ldx = b->ld_in; } else { l.X = b->layers[j - 1].Y; l.ldx = ldb; }
            most_dw = std::max(most_dw, (size_t)l.in * l.out);
        }
    }
    if (geo.exists() || app.exists()) { mem.alloc(&BG[0], (size_t)M * ldb); mem.alloc(&BG[1], (size_t)M * ldb); }
    const size_t splits = (size_t)((M + FLEX_SPLIT - 1) / FLEX_SPLIT);
    mem.alloc(&partial, splits * most_dw); mem.alloc(&colsum, splits * 256);
    long long at = 0;
    for (size_t i = 1; i < layers.size(); ++i) {
        FlexLayer &l = layers[i];
        const int hid = l.in - l.enc;
        l.wt = at;
        segs.push_back(FlexTSeg{(long long)(l.w + (size_t)l.enc * l.out), at, at, (long long)hid * l.out, hid, l.out});
        at += ((long long)hid * l.out + 3) / 4 * 4;
    }
    t_total = at;
    // ... and the branch rows of the kernels that read a branch's output (behind the FF(xyz) rows of the map), the kernels of the branches'
    // own hidden layers whole
    for (size_t i = 0; i < layers.size(); ++i) {
        FlexLayer &l = layers[i];
        const bool pos_in = (int)i < d.depth && l.enc > 0, dir_in = (int)i == d.depth + 1;     // layers that read pos_map / dir_map
        if (pos_in && geo.exists()) seg(l.bwt, l.w + (size_t)geo.off * l.out, pw, l.out);
        if (dir_in && app.exists()) seg(l.bwt, l.w + (size_t)app.off * l.out, pw, l.out);
    }
    for (FlexBranch *b : {&geo, &app})
        for (size_t j = 1; j < b->layers.size(); ++j) seg(b->layers[j].wt, b->layers[j].w, b->layers[j].in, b->layers[j].out);
    n_tseg = (int)segs.size();
    mem.alloc(&wt, (size_t)t_total);
    mem.upload(&tseg, segs, "segment");
}
// one more segment behind the table's last: rows [src / out ...) of a kernel [.][out], transposed to [out][rows]
void FlexBackend::seg(long long &slot, size_t src, int rows, int out) {
    slot = t_total;
    segs.push_back(FlexTSeg{(long long)src, t_total, t_total, (long long)rows * out, rows, out});
    t_total += ((long long)rows * out + 3) / 4 * 4;
}
// What dL/d params needs, placed at the first enable for the trainer's capacity: the feature gradients, a ray's and a row's sums, and the
// transposed parameter-feature rows of every reader (without branches: trunk layer 0 and the layers behind a skip read the geometry
// features, the first layer that reads dir_map the appearance features; with branches: the branch's layer 0 reads them) as NEW segments
// behind the table's last, so the places of the others in wt -- and a handle that never enables this -- stay as they are
int FlexBackend::enable_param_gradients() {
    if (t->P == 0) return ntx_set_error(NTX_E_INVALID, "parameter gradients: the model has no parameters (a Nerf, n_parameters [0, 0]); the layer-by-layer trainer of a "
                                        "ParamNerf takes them (ntx_trainer_create_flex, ntx_trainer_create_flex_ex)");
    if (ray_pg) return NTX_OK;
    DeviceMemory &mem = t->mem;
    const ntx_model_desc &d = t->desc;
    TRAIN_TRY(hipSetDevice(t->device));
    FlexBranch *br[2] = {&geo, &app};
    for (int k = 0; k < 2; ++k) {
        if (br[k]->n_in == 0) continue;
        ldpg[k] = pad4(br[k]->n_in);
        mem.alloc(&PG[k], (size_t)t->cap * ldpg[k]);
        if (br[k]->exists()) { FlexLayer &l = br[k]->layers[0]; seg(l.pwt, l.w, l.in, l.out); continue; }
        for (size_t i = 0; i < layers.size(); ++i) {
            FlexLayer &l = layers[i];
            const bool reads = k == 0 ? (int)i < d.depth && l.enc > 0 : (int)i == d.depth + 1;
            if (reads) seg(l.pwt, l.w + (size_t)br[k]->off * l.out, br[k]->n_in, l.out);
        }
    }
    mem.alloc(&ray_pg, (size_t)t->cap_rays * t->P); mem.alloc(&t->param_grad, (size_t)t->cap_rays * t->P);
    float *old_wt = wt; FlexTSeg *old_seg = tseg;
    n_tseg = (int)segs.size();
    mem.alloc(&wt, (size_t)t_total);                                         // (every forward pass fills it again)
    mem.upload(&tseg, segs, "segment");
    if (mem.rc == NTX_OK) { mem.release(old_wt); mem.release(old_seg); }
    return mem.rc;
}

// What dL/d rays and sample points needs, placed at the first enable for the trainer's capacity: the gradients at the FF(xyz) and FF(dir)
// rows, a plain step's two results, and the transposed first K3 rows of every reader's kernel (trunk layer 0 and the layers behind a skip read
// FF(xyz), the first layer that reads dir_map FF(dir); with or without branches) as NEW segments behind the table's last, as above
int FlexBackend::enable_input_gradients() {
    if (IG[0]) return NTX_OK;
    DeviceMemory &mem = t->mem;
    const ntx_model_desc &d = t->desc;
    TRAIN_TRY(hipSetDevice(t->device));
    K3[0] = 3 * (1 + 2 * d.pos_freq); K3[1] = 3 * (1 + 2 * d.dir_freq);
    for (int k = 0; k < 2; ++k) {
        ldig[k] = pad4(K3[k]);
        mem.alloc(&IG[k], (size_t)t->cap * ldig[k]);
        for (size_t i = 0; i < layers.size(); ++i) {
            FlexLayer &l = layers[i];
            const bool reads = k == 0 ? (int)i < d.depth && l.enc > 0 : (int)i == d.depth + 1;
            if (reads) seg(l.xwt, l.w, K3[k], l.out);
        }
    }
    mem.alloc(&t->d_rays_o, (size_t)t->cap_rays * 3); mem.alloc(&t->d_rays_d, (size_t)t->cap_rays * 3);
    float *old_wt = wt; FlexTSeg *old_seg = tseg;
    n_tseg = (int)segs.size();
    mem.alloc(&wt, (size_t)t_total);                                         // (every forward pass fills it again)
    mem.upload(&tseg, segs, "segment");
    if (mem.rc == NTX_OK) { mem.release(old_wt); mem.release(old_seg); }
    return mem.rc;
}

// a branch's layers, then its last output into the concatenations that hold the map
void FlexBackend::branch_forward(const FlexBranch &b, const FlexDst *dst, int n_dst, long long M, hipStream_t st) {
    const float *W = t->w;
    for (const FlexLayer &l : b.layers) {
        GemmArgs g{}; g.A = l.X; g.lda = l.ldx; g.B = W + l.w; g.ldb = l.out; g.C = l.Y; g.ldc = l.ldy; g.M = (int)M; g.N = l.out; g.K = l.in; g.bias = W + l.b; g.relu = 1;
        g.precision = t->precision; launch_gemm(st, true, g);
    }
    const FlexLayer &last = b.layers.back();
    FlexBranchCopyArgs c{}; c.src = last.Y; c.lds = last.ldy; c.width = pw; c.off = b.off; c.n_dst = n_dst; c.M = M;
    for (int i = 0; i < n_dst; ++i) c.dst[i] = dst[i];
    hipLaunchKernelGGL(flex_branch_copy_kernel, dim3((unsigned)((M * pw + 255) / 256)), dim3(256), 0, st, c);
}

int FlexBackend::forward(const StepRays &r, hipStream_t st) {
    const long long M = r.M();
    const float *W = t->w;
    hipLaunchKernelGGL(flex_transpose_kernel, dim3((unsigned)((t_total + 255) / 256)), dim3(256), 0, st, W, wt, tseg, n_tseg, t_total);
    {
        FlexEncodeArgs e{}; e.r = r; e.Kp = enc_Kp; e.Kd = enc_Kd; e.n_pos_dst = n_pos_dst; e.dir = dir_dst; e.dists = t->dists;
        for (int i = 0; i < n_pos_dst; ++i) e.pos[i] = pos_dst[i];
        if (geo.exists()) e.geo_in = FlexDst{geo.in, geo.ld_in};
        if (app.exists()) e.app_in = FlexDst{app.in, app.ld_in};
        const long long most = M * std::max(enc_Kp, enc_Kd);
        hipLaunchKernelGGL(flex_encode_kernel, dim3((unsigned)((most + 255) / 256), 2), dim3(256), 0, st, e);
    }
    network_forward(M, st);
    return NTX_OK;
}
// An instanced step: the same network on the n_live compact rows of the step's live samples (none: nothing is launched)
int FlexBackend::forward_samples(const StepSamples &s, hipStream_t st) {
    const long long M = s.n_live;
    if (M == 0) return NTX_OK;
    hipLaunchKernelGGL(flex_transpose_kernel, dim3((unsigned)((t_total + 255) / 256)), dim3(256), 0, st, t->w, wt, tseg, n_tseg, t_total);
    FlexEncodeSamplesArgs e{}; e.s = s; e.Kp = enc_Kp; e.Kd = enc_Kd; e.n_pos_dst = n_pos_dst; e.dir = dir_dst;
    for (int i = 0; i < n_pos_dst; ++i) e.pos[i] = pos_dst[i];
    if (geo.exists()) e.geo_in = FlexDst{geo.in, geo.ld_in};
    if (app.exists()) e.app_in = FlexDst{app.in, app.ld_in};
    const long long most = M * std::max(enc_Kp, enc_Kd);
    hipLaunchKernelGGL(flex_encode_samples_kernel, dim3((unsigned)((most + 255) / 256), 2), dim3(256), 0, st, e);
    network_forward(M, st);
    return NTX_OK;
}
void FlexBackend::network_forward(long long M, hipStream_t st) {
    const float *W = t->w;
    if (geo.exists()) branch_forward(geo, pos_dst, n_pos_dst, M, st);        // model.py:88-93: in front of trunk layer 0
    for (size_t i = 0; i < layers.size(); ++i) {                             // a contraction per layer, every output kept
        const FlexLayer &l = layers[i];
        if ((int)i == t->desc.depth + 1 && app.exists()) branch_forward(app, &dir_dst, 1, M, st);      // :96-101: in front of the first layer that reads dir_map
        GemmArgs g{}; g.A = l.X; g.lda = l.ldx; g.B = W + l.w; g.ldb = l.out; g.C = l.Y; g.ldc = l.ldy; g.M = (int)M; g.N = l.out; g.K = l.in; g.bias = W + l.b; g.relu = l.relu;
        g.precision = t->precision; launch_gemm(st, true, g);
    }
    const unsigned head_grid = (unsigned)std::min<long long>((M + 3) / 4, (long long)t->cus * 8);
    const FlexLayer &lt = layers[last_trunk], &lh = layers[half];
    hipLaunchKernelGGL(flex_head_kernel<1>, dim3(head_grid), dim3(256), 0, st, lt.Y, lt.ldy, lt.out, W + alpha.w, W + alpha.b, t->sigma, M);      // model.py:111
    hipLaunchKernelGGL(flex_head_kernel<3>, dim3(head_grid), dim3(256), 0, st, lh.Y, lh.ldy, lh.out, W + rgb.w, W + rgb.b, t->raw_rgb, M);        // :123
}

// the way back from the composite's adjoint dgrad [M][4]: per layer, last to first, dW = X^T . dY over ranges of FLEX_SPLIT samples added in
// ascending order, then dX = (dY . W[hidden rows]^T) where the stored activation in front is > 0
void FlexBackend::reduce(hipStream_t st, int n_split, const float *part, long long count, size_t out, const float *bias_partial, long long bias_count, size_t bias_out) {
    ReduceBatch rb{};
    rb.job[0] = ReduceJob{part, n_split, count, count, 0, t->grad + out, 0};
    rb.n = 1;
    if (bias_partial) { rb.job[1] = ReduceJob{bias_partial, n_split, bias_count, bias_count, 0, t->grad + bias_out, (count + 255) / 256 * 256}; rb.n = 2; }
    launch_reduce(st, rb);
}
// A consumer's term of the gradient at a branch's output: BG[0] (+)= dY . W_consumer[branch rows]^T, kept where the branch's last ReLU was
// open.  The contraction masks after it accumulates, and what it masks is the same in every term, so masking each equals masking the sum.
void FlexBackend::branch_term(FlexBranch &b, const FlexLayer &consumer, const float *dY, long long M, hipStream_t st) {
    const FlexLayer &last = b.layers.back();
    GemmArgs g{}; g.A = dY; g.lda = ldg; g.B = wt + consumer.bwt; g.ldb = pw; g.C = BG[0]; g.ldc = ldb; g.M = (int)M; g.N = pw; g.K = consumer.out;
    g.accumulate = b.consumers_met++ > 0; g.mask = last.Y; g.ldmask = last.ldy;
    g.precision = t->precision; launch_gemm(st, true, g);
}
// A reader's term of the gradient at a group's parameter features (0 geometry, 1 appearance): PG (+)= dY . W[feature rows]^T, the readers in
// the order the way back meets them
void FlexBackend::param_term(int group, long long pwt, int n_in, const float *dY, int lddy, int K, long long M, hipStream_t st) {
    GemmArgs g{}; g.A = dY; g.lda = lddy; g.B = wt + pwt; g.ldb = n_in; g.C = PG[group]; g.ldc = ldpg[group]; g.M = (int)M; g.N = n_in; g.K = K;
    g.accumulate = pg_met[group]++ > 0;
    g.precision = t->precision; launch_gemm(st, true, g);
}
// A reader's term of the gradient at the FF(xyz) rows (group 0) or the FF(dir) rows (1): IG (+)= dY . W[first K3 rows]^T, in the same order
void FlexBackend::input_term(int group, const FlexLayer &l, const float *dY, long long M, hipStream_t st) {
    GemmArgs g{}; g.A = dY; g.lda = ldg; g.B = wt + l.xwt; g.ldb = K3[group]; g.C = IG[group]; g.ldc = ldig[group]; g.M = (int)M; g.N = K3[group]; g.K = l.out;
    g.accumulate = ig_met[group]++ > 0;
    g.precision = t->precision; launch_gemm(st, true, g);
}
// ... and from there through the branch, as through the trunk: dW / db per layer over ranges of FLEX_SPLIT samples, dX masked by the layer in
// front; nothing behind the first layer (the inputs are not trained)
void FlexBackend::branch_backward(const FlexBranch &b, long long M, int n_split, hipStream_t st) {
    int cur = 0;
    for (int j = (int)b.layers.size() - 1; j >= 0; --j) {
        const FlexLayer &l = b.layers[j];
        const float *dY = BG[cur];
        if (t->takes_weight_gradients()) {
            GemmArgs g{}; g.A = l.X; g.lda = l.ldx; g.B = dY; g.ldb = ldb; g.C = partial; g.ldc = l.out; g.M = l.in; g.N = l.out; g.K = (int)M;
            g.k_chunk = FLEX_SPLIT; g.split_stride = (long long)l.in * l.out; g.colsum = colsum;
            g.precision = t->precision; launch_gemm(st, false, g, n_split);
            reduce(st, n_split, partial, (long long)l.in * l.out, l.w, colsum, l.out, l.b);
        }
        if (j == 0) {                                                        // behind the first layer lie the parameter features: dY_0 . W_0^T where dL/d params is asked for
            if (t->pg_mode != 0) param_term(&b == &geo ? 0 : 1, l.pwt, l.in, dY, ldb, l.out, M, st);
            break;
        }
        const FlexLayer &s = b.layers[j - 1];
        GemmArgs x{}; x.A = dY; x.lda = ldb; x.B = wt + l.wt; x.ldb = l.in; x.C = BG[cur ^ 1]; x.ldc = ldb; x.M = (int)M; x.N = l.in; x.K = l.out;
        x.mask = s.Y; x.ldmask = s.ldy;
        x.precision = t->precision; launch_gemm(st, true, x);
        cur ^= 1;
    }
}

int FlexBackend::backward(const StepRays &r, hipStream_t st) {
    network_backward(r.M(), st);
    // the features' gradient through the encoder, a ray's samples, a row's rays
    if (t->pg_mode != 0) launch_param_fold(st, r, PG[0], PG[1], ldpg[0], ldpg[1], ray_pg, t->P, t->param_grad);
    // the FF(xyz) / FF(dir) rows' gradient through the encoder, a ray's samples
    if (t->ig_mode != 0) launch_ray_fold(st, r, IG[0], IG[1], ldig[0], ldig[1], t->dgrad, t->sigma, t->step_noise, t->d_rays_o, t->d_rays_d);
    return NTX_OK;
}
// An instanced step's way back over its n_live rows.  Without a live sample nothing is contracted: every weight gradient is exactly 0 (mode
// 2 leaves the buffer alone, as ever), and the per-sample parameter gradients are zeros.
int FlexBackend::backward_samples(const StepSamples &s, float *sample_pg, hipStream_t st) {
    if (s.n_live > 0) network_backward(s.n_live, st);
    else if (t->takes_weight_gradients()) TRAIN_TRY(hipMemsetAsync(t->grad, 0, t->n_weights * sizeof(float), st));
    if (t->pg_mode != 0) launch_param_samples(st, s, PG[0], PG[1], ldpg[0], ldpg[1], t->P, sample_pg);
    if (t->ig_mode != 0) launch_input_samples(st, s, IG[0], IG[1], ldig[0], ldig[1], t->d_pts, t->d_dirs);      // (no live sample: every row_of is -1, both results are zeros)
    return NTX_OK;
}
void FlexBackend::network_backward(long long M, hipStream_t st) {
    const float *W = t->w;
    const int n_split = (int)((M + FLEX_SPLIT - 1) / FLEX_SPLIT);
    auto reduce = [&](const float *part, long long count, size_t out, const float *bias_partial, long long bias_count, size_t bias_out) {
        this->reduce(st, n_split, part, count, out, bias_partial, bias_count, bias_out);
    };
    geo.consumers_met = app.consumers_met = 0; pg_met[0] = pg_met[1] = 0; ig_met[0] = ig_met[1] = 0;
    const bool wgrad = t->takes_weight_gradients(), pgrad = t->pg_mode != 0;   // either mode 2: no weight gradient is taken or reduced
    const FlexLayer &lt = layers[last_trunk], &lh = layers[half];
    const unsigned ew = 256;
    // the colour head (model.py:123): kernel and bias lie side by side in the blob, as in a range's partial sums
    auto pow2 = [](int k) { int p = 64; while (p < k) p *= 2; return p; };
    if (wgrad) {
        hipLaunchKernelGGL(flex_head_wgrad_kernel<3>, dim3((unsigned)n_split), dim3(1024), 0, st, lh.Y, lh.ldy, lh.out, pow2(lh.out), t->dgrad, 0, M, partial);
        reduce(partial, (long long)lh.out * 3 + 3, rgb.w, nullptr, 0, 0);
    }
    int cur = 0;
    hipLaunchKernelGGL(flex_head_dx_kernel<3>, dim3((unsigned)((M * lh.out + ew - 1) / ew)), dim3(ew), 0, st, t->dgrad, 0, W + rgb.w, lh.out, lh.Y, lh.ldy, G[cur], ldg, M);
    for (int i = (int)layers.size() - 1; i >= 0; --i) {
        const FlexLayer &l = layers[i];
        const float *dY = G[cur];
        if (wgrad) {   // dW_i and db_i
            GemmArgs g{}; g.A = l.X; g.lda = l.ldx; g.B = dY; g.ldb = ldg; g.C = partial; g.ldc = l.out; g.M = l.in; g.N = l.out; g.K = (int)M;
            g.k_chunk = FLEX_SPLIT; g.split_stride = (long long)l.in * l.out; g.colsum = colsum;
            g.precision = t->precision; launch_gemm(st, false, g, n_split);
            reduce(partial, (long long)l.in * l.out, l.w, colsum, l.out, l.b);
        }
        if (l.bwt >= 0) {                                                    // a reader of a branch's output: its term, in the order this loop meets the readers
            const bool trunk = i <= last_trunk;
            FlexBranch &b = trunk ? geo : app;
            branch_term(b, l, dY, M, st);
            if (!trunk || i == 0) branch_backward(b, M, n_split, st);        // the appearance branch has one reader; trunk layer 0 is the geometry branch's last
        } else if (pgrad && l.pwt >= 0) {                                    // a reader of parameter features: its term, in the same order
            const int group = i <= last_trunk ? 0 : 1;
            param_term(group, l.pwt, (group == 0 ? geo : app).n_in, dY, ldg, l.out, M, st);
        }
        if (t->ig_mode != 0 && l.xwt >= 0) input_term(i <= last_trunk ? 0 : 1, l, dY, M, st);      // a reader of FF(xyz) / FF(dir): its term, in the same order
        if (i == 0) break;
        const FlexLayer &s = layers[l.src];
        float *dX = G[cur ^ 1];
        int accumulate = 0;
        if (l.src == last_trunk) {                                           // the density head hangs on the same output (model.py:111): its rank-1 term first
            if (wgrad) {
                hipLaunchKernelGGL(flex_head_wgrad_kernel<1>, dim3((unsigned)n_split), dim3(1024), 0, st, lt.Y, lt.ldy, lt.out, pow2(lt.out), t->dgrad, 3, M, partial);
                reduce(partial, (long long)lt.out + 1, alpha.w, nullptr, 0, 0);
            }
            hipLaunchKernelGGL(flex_head_dx_kernel<1>, dim3((unsigned)((M * lt.out + ew - 1) / ew)), dim3(ew), 0, st, t->dgrad, 3, W + alpha.w, lt.out, (const float *)nullptr, 0, dX,
                               ldg, M);
            accumulate = 1;
        }
        GemmArgs g{}; g.A = dY; g.lda = ldg; g.B = wt + l.wt; g.ldb = l.in - l.enc; g.C = dX; g.ldc = ldg; g.M = (int)M; g.N = l.in - l.enc; g.K = l.out;
        g.accumulate = accumulate;
        if (s.relu) { g.mask = s.Y; g.ldmask = s.ldy; }
        g.precision = t->precision; launch_gemm(st, true, g);
        cur ^= 1;
    }
}

int FlexBackend::activation(int layer, int64_t n_samples_total, float *out_host) {              // row-major buffers: a strided copy
    const float *from = nullptr; int width = 0, ld = 0;
    if (layer >= 0 && layer < (int)relu_layers.size()) { const FlexLayer &l = layers[relu_layers[layer]]; from = l.Y; width = l.out; ld = l.ldy; }
    else if (layer >= 32 && layer < 32 + (int)geo.layers.size()) { const FlexLayer &l = geo.layers[layer - 32]; from = l.Y; width = l.out; ld = l.ldy; }
    else if (layer >= 48 && layer < 48 + (int)app.layers.size()) { const FlexLayer &l = app.layers[layer - 48]; from = l.Y; width = l.out; ld = l.ldy; }
    else if (layer == 64) { from = t->sigma; width = ld = 1; }
    else if (layer == 65) { from = t->raw_rgb; width = ld = 3; }
    else if (layer == 30) { from = t->dgrad; width = ld = 4; }
    else return ntx_set_error(NTX_E_INVALID, "layer %d (0 .. %d: the ReLU layers in the order trunk, colour layers, colour half; 32 + j / 48 + j: layer j of the geometry / "
                              "appearance branch, where the model has it; 64 the raw density, 65 the raw colour, 30 the composite's adjoint)", layer, (int)relu_layers.size() - 1);
    TRAIN_TRY(hipSetDevice(t->device));
    TRAIN_TRY(hipDeviceSynchronize());
    TRAIN_TRY(hipMemcpy2D(out_host, (size_t)width * sizeof(float), from, (size_t)ld * sizeof(float), (size_t)width * sizeof(float), (size_t)n_samples_total, hipMemcpyDeviceToHost));
    return NTX_OK;
}
}   // namespace
namespace ntx_train {
// the architectures the flex render family takes (ntx_arch.h: find_variant): without parameter branches (ntx_trainer_create_flex), or --
// branches: desc is an ntx_model_desc_ex -- with them, within the render side's limits (ntx_trainer_create_flex_ex)
int flex_check(const ntx_model_desc *desc, TrainDims *dims, bool branches) {
    const bool nerf = desc->kind == NTX_MODEL_NERF;
    if (branches && desc->kind != NTX_MODEL_PARAMNERF_EX)
        return ntx_set_error(NTX_E_UNSUPPORTED, "training: model kind %d (ntx_trainer_create_flex_ex takes an ntx_model_desc_ex, kind NTX_MODEL_PARAMNERF_EX)", desc->kind);
    if (desc->kind != NTX_MODEL_PARAMNERF && desc->kind != NTX_MODEL_NERF && desc->kind != NTX_MODEL_PARAMNERF_EX) return ntx_set_error(NTX_E_UNSUPPORTED, "training: model kind %d", desc->kind);
    if (!branches && desc->kind == NTX_MODEL_PARAMNERF_EX && desc->n_geo + desc->n_app > 0 && reinterpret_cast<const ntx_model_desc_ex *>(desc)->param_depth != 0)
        return ntx_set_error(NTX_E_UNSUPPORTED, "training: parameter branches (param_depth > 0) train through ntx_trainer_create_flex_ex");
    if (desc->pos_encoding != NTX_POS_FOURIER || desc->n_pos != 3)
        return ntx_set_error(NTX_E_UNSUPPORTED, "the layer-by-layer trainer takes Fourier features on n_pos 3 (an IPE model trains in the 8 x 256 / skips [4] / color_depth 1 shape: ntx_trainer_create)");
    const int n_geo = nerf ? 0 : desc->n_geo, n_app = nerf ? 0 : desc->n_app, cd = nerf ? 0 : desc->color_depth;
    if (desc->depth < 1 || desc->depth > FLEX_MAX_DEPTH || desc->width < 2 || desc->width > 256 || cd < 0 || cd > FLEX_MAX_COLOR)
        return ntx_set_error(NTX_E_UNSUPPORTED, "training: depth %d width %d color_depth %d (built: depth 1..%d, width 2..256, color_depth 0..%d)", desc->depth, desc->width, cd,
                             FLEX_MAX_DEPTH, FLEX_MAX_COLOR);
    if ((desc->skip >= 0 && !(desc->skip & NTX_SKIP_MASK) && desc->skip >= 30) || ((ntx::skip_mask_of(desc) >> (desc->depth - 1)) & 1u))
        return ntx_set_error(NTX_E_UNSUPPORTED, "training: a skip behind the last trunk layer (it widens the density head and the feature layer, model.py:107-114) is not built");
    if (n_geo < 0 || n_geo > 4 || n_app < 0 || n_app > 8 || desc->pos_freq < 0 || desc->pos_freq > 10 || desc->dir_freq < 0 || desc->dir_freq > 4 ||
        (n_geo + n_app > 0 && (desc->param_freq < 0 || desc->param_freq > 4)))
        return ntx_set_error(NTX_E_UNSUPPORTED, "training: n_parameters [%d,%d] / band counts %d %d %d (built: [g<=4, a<=8], bands <= 10 / 4 / 4)", n_geo, n_app, desc->pos_freq,
                             desc->dir_freq, desc->param_freq);
    int pd = 0, pw = 0;
    if (branches) {
        const ntx_model_desc_ex *ex = reinterpret_cast<const ntx_model_desc_ex *>(desc);
        if (ex->param_depth < 0 || ex->param_depth > ntx::FLEX_MAX_PARAM_DEPTH || (ex->param_depth > 0 && (ex->param_width < 2 || ex->param_width > 2 * ntx::BRANCH_K)))
            return ntx_set_error(NTX_E_UNSUPPORTED, "training: param_depth %d param_width %d (built: param_depth 0..%d, param_width 2..%d)", ex->param_depth, ex->param_width,
                                 ntx::FLEX_MAX_PARAM_DEPTH, 2 * ntx::BRANCH_K);
        pd = n_geo + n_app > 0 ? ex->param_depth : 0;                        // a model without parameters has no branches (model.py:88, 96)
        pw = pd > 0 ? ex->param_width : 0;
    }
    const int pfq = n_geo + n_app > 0 ? desc->param_freq : 0;
    dims->desc = *desc; dims->desc.n_geo = n_geo; dims->desc.n_app = n_app; dims->desc.param_freq = pfq; dims->ipe = false;
    if (branches) dims->desc.kind = NTX_MODEL_PARAMNERF;                     // (the handle's copy is the base struct alone: nothing may look behind it)
    dims->param_depth = pd; dims->param_width = pw;
    FlexBackend plan;
    dims->n_weights = plan.plan(desc, pd, pw);
    dims->Kp = plan.Kp; dims->Kd = plan.Kd;
    return NTX_OK;
}

void launch_param_fold(hipStream_t st, const StepRays &r, const float *pg_geo, const float *pg_app, int ld_geo, int ld_app, float *ray_pg, int P, float *param_grad) {
    const long long rows = (r.n_rays + r.rays_per_param_row - 1) / r.rays_per_param_row;
    FlexFoldArgs f{}; f.r = r; f.pg_geo = pg_geo; f.pg_app = pg_app; f.ld_geo = ld_geo; f.ld_app = ld_app; f.ray_pg = ray_pg;
    hipLaunchKernelGGL(flex_param_fold_kernel, dim3((unsigned)((r.n_rays + 3) / 4)), dim3(256), 0, st, f);
    hipLaunchKernelGGL(flex_param_rows_kernel, dim3((unsigned)((rows * P + 255) / 256)), dim3(256), 0, st, ray_pg, r.n_rays, r.rays_per_param_row, P, rows, param_grad);
}
void launch_ray_fold(hipStream_t st, const StepRays &r, const float *ig_pos, const float *ig_dir, int ld_pos, int ld_dir, const float *dgrad, const float *sigma,
                     const float *noise, float *d_rays_o, float *d_rays_d) {
    FlexRayFoldArgs f{}; f.r = r; f.ig_pos = ig_pos; f.ig_dir = ig_dir; f.ld_pos = ld_pos; f.ld_dir = ld_dir; f.dgrad = dgrad; f.sigma = sigma;
    f.noise = noise; f.d_rays_o = d_rays_o; f.d_rays_d = d_rays_d;
    hipLaunchKernelGGL(flex_ray_fold_kernel, dim3((unsigned)((r.n_rays + 3) / 4)), dim3(256), 0, st, f);
}
void launch_param_samples(hipStream_t st, const StepSamples &s, const float *pg_geo, const float *pg_app, int ld_geo, int ld_app, int P, float *out) {
    FlexSampleFoldArgs f{}; f.s = s; f.pg_geo = pg_geo; f.pg_app = pg_app; f.ld_geo = ld_geo; f.ld_app = ld_app; f.out = out;
    hipLaunchKernelGGL(flex_param_samples_kernel, dim3((unsigned)((s.M() * P + 255) / 256)), dim3(256), 0, st, f);
}
void launch_input_samples(hipStream_t st, const StepSamples &s, const float *ig_pos, const float *ig_dir, int ld_pos, int ld_dir, float *d_pts, float *d_dirs) {
    FlexSampleInputArgs f{}; f.s = s; f.ig_pos = ig_pos; f.ig_dir = ig_dir; f.ld_pos = ld_pos; f.ld_dir = ld_dir; f.d_pts = d_pts; f.d_dirs = d_dirs;
    hipLaunchKernelGGL(flex_input_samples_kernel, dim3((unsigned)((s.M() * 6 + 255) / 256)), dim3(256), 0, st, f);
}

int flex_backend_create(ntx_trainer *t) {
    FlexBackend *f = new FlexBackend();
    t->backend = f; f->t = t;
    f->plan(&t->desc, t->param_depth, t->param_width);
    f->place();
    return t->mem.rc;
}
}   // namespace ntx_train
