// ntx_ray_losses.hip -- losses along a ray on the compositing weights: ntx_ray_distortion, the distortion regulariser of mip-NeRF 360 in its
// O(S) form and its gradient at the weights, and ntx_ray_interlevel, the interlevel (proposal) loss of the same paper between a fine and a
// proposal histogram and its gradients at both sets of weights (the formulas: include/nerftex.h, at the entries).  One unit of its own: no
// context, no trainer, no header of the render or training kernels.  gfx950 only.  -ffp-contract=off: nothing below is fused.
#include "ntx_entry.h"

namespace {
constexpr int RAYS_PER_BLOCK = 4;   // a wave per ray

struct DistortionArgs {
    const float *w, *z, *widths, *live, *ray_scale;   // [N][S], [N][S], NULL or [N][S], NULL or [N][S], NULL or [N]
    float *loss, *grad;                               // NULL or [N], NULL or [N][S]
    long long n_rays; int S;
};

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// inclusive sums over the 64 lanes of a chunk, of the weights and of the weighted depths together: lane l ends with the sum of lanes 0 .. l,
// added in the order the doubling steps fix
__device__ __forceinline__ void chunk_scan(int lane, float &W, float &M) {
    for (int o = 1; o < 64; o <<= 1) {
        const float wo = __shfl_up(W, o), mo = __shfl_up(M, o);
        if (lane >= o) { W += wo; M += mo; }
    }
}

// What one lane holds of one chunk: sample s = s0 + lane of the ray, selected to w = 0, m = 0, delta = 0 where it is not live (nothing of a
// dead sample is multiplied: the sparse instancer leaves those rows unwritten).
struct Sample { bool lv; float w, z, delta; };
__device__ __forceinline__ Sample load_sample(const DistortionArgs &a, size_t row, int s) {
    Sample x{false, 0.0f, 0.0f, 0.0f};
    if (s >= a.S) return x;
    const float z = a.z[row + s];
    x.lv = __builtin_isfinite(z) && (a.live ? a.live[row + s] > 0.0f : true);
    if (!x.lv) return x;
    x.w = a.w[row + s]; x.z = z;
    if (a.widths) x.delta = a.widths[row + s];
    else if (a.S > 1) {                                 // the composite's: the last width is the one before it; 0 where the neighbour is not finite
        const float d = s + 1 < a.S ? a.z[row + s + 1] - z : z - a.z[row + s - 1];
        x.delta = __builtin_isfinite(d) ? d : 0.0f;
    }
    return x;
}

__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void ray_distortion_kernel(DistortionArgs a) {
    const int lane = threadIdx.x & 63, S = a.S;
    for (long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6); ray < a.n_rays; ray += (long long)gridDim.x * RAYS_PER_BLOCK) {
        const size_t row = (size_t)ray * S;
        // pass 1: the depth of the first live sample, and the totals of w and w m (m = z - z_first) as the carries pass 2 will end with
        bool found = false;
        float z_first = 0.0f, W_tot = 0.0f, M_tot = 0.0f;
        for (int s0 = 0; s0 < S; s0 += 64) {
            const Sample x = load_sample(a, row, s0 + lane);
            const unsigned long long alive = __ballot(x.lv);
            if (alive == 0) continue;                       // (wave-uniform)
            if (!found) { z_first = __shfl(x.z, __ffsll((long long)alive) - 1); found = true; }
            float W = x.w, M = x.lv ? x.w * (x.z - z_first) : 0.0f;
            chunk_scan(lane, W, M);
            W_tot += __shfl(W, 63); M_tot += __shfl(M, 63);
        }
        if (!found) {                                       // no live sample: 0 and a zero row, whatever ray_scale holds
            if (a.loss && lane == 0) a.loss[ray] = 0.0f;
            if (a.grad) for (int s = lane; s < S; s += 64) a.grad[row + s] = 0.0f;
            continue;
        }
        const float scale = a.ray_scale ? a.ray_scale[ray] : 1.0f;
        // pass 2 (the row comes from L2): exclusive prefix sums by chunk with carries; the suffix sums are the totals less the inclusive ones
        float W_carry = 0.0f, M_carry = 0.0f, pair = 0.0f, self = 0.0f;
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const Sample x = load_sample(a, row, s);
            if (__ballot(x.lv) == 0) {                      // nothing live in the chunk: the carries stand
                if (a.grad && s < S) a.grad[row + s] = 0.0f;
                continue;
            }
            const float m = x.lv ? x.z - z_first : 0.0f;
            float W = x.w, M = x.lv ? x.w * m : 0.0f;
            chunk_scan(lane, W, M);
            float W_ex = __shfl_up(W, 1), M_ex = __shfl_up(M, 1);
            if (lane == 0) { W_ex = 0.0f; M_ex = 0.0f; }
            const float W_lt = W_carry + W_ex, M_lt = M_carry + M_ex;           // sums over the samples in front of s
            const float W_gt = W_tot - (W_carry + W), M_gt = M_tot - (M_carry + M);   // ... and behind it
            const float before = m * W_lt - M_lt;                              // sum_{j<s} w_j (z_s - z_j)
            const float behind = M_gt - m * W_gt;                              // sum_{j>s} w_j (z_j - z_s)
            if (x.lv) {
                pair += x.w * before;
                self += (x.w * x.w) * x.delta;
            }
            if (a.grad && s < S) a.grad[row + s] = x.lv ? scale * (2.0f * (before + behind) + (2.0f / 3.0f) * (x.w * x.delta)) : 0.0f;
            W_carry += __shfl(W, 63); M_carry += __shfl(M, 63);
        }
        if (a.loss) {
            const float L = 2.0f * wave_sum(pair) + (1.0f / 3.0f) * wave_sum(self);
            if (lane == 0) a.loss[ray] = scale * L;
        }
    }
}
// ---- the interlevel loss (include/nerftex.h at ntx_ray_interlevel has the formula) ----------------------------------------------------------
struct InterlevelArgs {
    const float *w, *z, *wp, *zp, *ray_scale;         // [N][S], [N][S], [N][Sp], [N][Sp], NULL or [N]
    float *loss, *grad_prop, *grad_fine;              // NULL or [N], NULL or [N][Sp], NULL or [N][S]
    long long n_rays; int S, Sp; float eps;
};

// the end of interval k of a row of n depths: the next depth ITSELF, and the last width repeated behind the last one (k < n)
__device__ __forceinline__ float interval_end(const float *row, int k, int n) {
    if (k + 1 < n) return row[k + 1];
    const float zl = row[k];
    return n > 1 ? zl + (zl - row[k - 1]) : zl;
}
// #{k < n : end_k <= x} and #{k < n : row_k < x}: both predicates are monotone in k (the row is nondecreasing), at most 13 steps each
__device__ __forceinline__ int count_ends_le(const float *row, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (interval_end(row, mid, n) <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int count_starts_lt(const float *row, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A wave per ray; q of the ray's fine samples passes from pass A to pass B through the wave's own S floats of LDS (sized on the host:
// RAYS_PER_BLOCK * S * 4 bytes, 64 KB at the limit).  The searched rows come from L1 / L2.
__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void ray_interlevel_kernel(InterlevelArgs a) {
    extern __shared__ float q_lds[];
    const int lane = threadIdx.x & 63, S = a.S, Sp = a.Sp;
    float *q_row = q_lds + (size_t)(threadIdx.x >> 6) * S;
    for (long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6); ray < a.n_rays; ray += (long long)gridDim.x * RAYS_PER_BLOCK) {
        const float *z = a.z + (size_t)ray * S, *w = a.w + (size_t)ray * S;
        const float *zp = a.zp + (size_t)ray * Sp, *wp = a.wp + (size_t)ray * Sp;
        // live iff every depth of both sets is finite
        bool bad = false;
        for (int s = lane; s < S; s += 64) bad |= !__builtin_isfinite(z[s]);
        for (int s = lane; s < Sp; s += 64) bad |= !__builtin_isfinite(zp[s]);
        if (__ballot(bad) != 0) {                           // (wave-uniform) 0 and two zero rows, whatever ray_scale and the weights hold
            if (a.loss && lane == 0) a.loss[ray] = 0.0f;
            if (a.grad_fine) for (int s = lane; s < S; s += 64) a.grad_fine[(size_t)ray * S + s] = 0.0f;
            if (a.grad_prop) for (int s = lane; s < Sp; s += 64) a.grad_prop[(size_t)ray * Sp + s] = 0.0f;
            continue;
        }
        const float scale = a.ray_scale ? a.ray_scale[ray] : 1.0f;
        // pass A: fine samples across the lanes; the proposal weights a sample's interval overlaps, added directly in increasing j
        float acc = 0.0f;
        for (int i = lane; i < S; i += 64) {
            const float ai = z[i], bi = interval_end(z, i, S), wi = w[i];
            const int lo = count_ends_le(zp, Sp, ai), hi = count_starts_lt(zp, Sp, bi);   // 0 <= lo, hi <= Sp
            float bound = 0.0f;
            for (int j = lo; j < hi; ++j) bound += wp[j];
            const float d = wi - bound, r = d > 0.0f ? d : 0.0f, q = r / (wi + a.eps);
            acc += r * q;
            q_row[i] = q;
            if (a.grad_fine) a.grad_fine[(size_t)ray * S + i] = scale * (q * (2.0f - q));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // q_row: written and read by this wave alone
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // pass B: proposal samples across the lanes; q of the fine samples an interval overlaps, added directly in increasing i
        if (a.grad_prop) {
            for (int j = lane; j < Sp; j += 64) {
                const float aj = zp[j], bj = interval_end(zp, j, Sp);
                const int lo = count_ends_le(z, S, aj), hi = count_starts_lt(z, S, bj);   // 0 <= lo, hi <= S
                float sum = 0.0f;
                for (int i = lo; i < hi; ++i) sum += q_row[i];
                a.grad_prop[(size_t)ray * Sp + j] = scale * (0.0f - 2.0f * sum);
            }
        }
        if (a.loss) {
            const float L = wave_sum(acc);
            if (lane == 0) a.loss[ray] = scale * L;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the next ray of this wave writes q_row again
        __builtin_amdgcn_wave_barrier();
    }
}
}  // namespace

extern "C" int ntx_ray_distortion(const float *weights, const float *z_vals, const float *widths, const float *live, const float *ray_scale, int64_t n_rays, int n_samples,
                                  float *loss_out, float *grad_out, void *stream) {
    if (!weights || !z_vals) return ntx_set_error(NTX_E_INVALID, "weights or z_vals is NULL");
    if (!loss_out && !grad_out) return ntx_set_error(NTX_E_INVALID, "loss_out and grad_out are both NULL");
    if (n_samples < 1 || n_samples > 4096) return ntx_set_error(NTX_E_INVALID, "n_samples %d outside [1, 4096]", n_samples);
    if (n_rays < 0 || n_rays > 0x7fffffff) return ntx_set_error(NTX_E_INVALID, "n_rays %lld outside [0, 2^31)", (long long)n_rays);
    if (live && !widths) return ntx_set_error(NTX_E_INVALID, "live without widths: the difference of neighbouring depths would read samples that are not live");
    if (n_rays == 0) return NTX_OK;
    DistortionArgs a{};
    a.w = weights; a.z = z_vals; a.widths = widths; a.live = live; a.ray_scale = ray_scale;
    a.loss = loss_out; a.grad = grad_out;
    a.n_rays = n_rays; a.S = n_samples;
    int64_t nb = (n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK;
    if (nb > 256 * 8) nb = 256 * 8;   // 8 workgroups per CU, grid-stride over rays
    ray_distortion_kernel<<<dim3((unsigned)nb), dim3(64 * RAYS_PER_BLOCK), 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

extern "C" int ntx_ray_interlevel(const float *weights, const float *z_vals, int n_samples, const float *weights_prop, const float *z_prop, int n_prop,
                                  const float *ray_scale, float eps, int64_t n_rays, float *loss_out, float *grad_prop_out, float *grad_fine_out, void *stream) {
    if (!weights || !z_vals || !weights_prop || !z_prop) return ntx_set_error(NTX_E_INVALID, "weights, z_vals, weights_prop or z_prop is NULL");
    if (!loss_out && !grad_prop_out && !grad_fine_out) return ntx_set_error(NTX_E_INVALID, "loss_out, grad_prop_out and grad_fine_out are all NULL");
    if (n_samples < 1 || n_samples > 4096) return ntx_set_error(NTX_E_INVALID, "n_samples %d outside [1, 4096]", n_samples);
    if (n_prop < 1 || n_prop > 4096) return ntx_set_error(NTX_E_INVALID, "n_prop %d outside [1, 4096]", n_prop);
    if (n_rays < 0 || n_rays > 0x7fffffff) return ntx_set_error(NTX_E_INVALID, "n_rays %lld outside [0, 2^31)", (long long)n_rays);
    if (!(eps > 0.0f) || !__builtin_isfinite(eps)) return ntx_set_error(NTX_E_INVALID, "eps must be finite and > 0");
    if (n_rays == 0) return NTX_OK;
    InterlevelArgs a{};
    a.w = weights; a.z = z_vals; a.wp = weights_prop; a.zp = z_prop; a.ray_scale = ray_scale;
    a.loss = loss_out; a.grad_prop = grad_prop_out; a.grad_fine = grad_fine_out;
    a.n_rays = n_rays; a.S = n_samples; a.Sp = n_prop; a.eps = eps;
    int64_t nb = (n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK;
    if (nb > 256 * 8) nb = 256 * 8;   // grid-stride over rays
    const size_t lds = (size_t)RAYS_PER_BLOCK * (size_t)n_samples * sizeof(float);   // q of four rays: 64 KB at S = 4096, two workgroups a CU
    ray_interlevel_kernel<<<dim3((unsigned)nb), dim3(64 * RAYS_PER_BLOCK), lds, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}
