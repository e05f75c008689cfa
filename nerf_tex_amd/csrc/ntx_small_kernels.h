// ntx_small_kernels.h -- the bandwidth-bound stand-alone kernels (composite, ray generation, Fourier
// features) and the small kernels of the context's entries.  Included by ntx_standalone.hip only, which launches every one of them; the
// MFMA kernels are in ntx_device.h / ntx_variant.hip.
#pragma once

#include "ntx_device.h"

namespace ntx {

// ---------------------------------------------------------------------------------------------
// stand-alone composite: one wave64 per ray, lane = sample, chunks of 64 with carry
// ---------------------------------------------------------------------------------------------
struct CompositeArgs {
    const float *color, *sigma, *z, *rays_d;
    float *color_out, *alpha_out, *weights_out;
    int64_t n_rays;
    int n_samples;
    uint32_t flags;
    float bkgd[3];
};

__global__ __launch_bounds__(256) void composite_kernel(CompositeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int S = a.n_samples;
    for (int64_t ray = wave; ray < a.n_rays; ray += nwaves) {
        const float dx = a.rays_d[3 * ray], dy = a.rays_d[3 * ray + 1], dz = a.rays_d[3 * ray + 2];
        const float dnorm = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
        const float *zr = a.z + ray * S;
        RayAccum ra{1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int base = 0; base < S; base += 64) {
            const int i = base + lane;
            const bool valid = i < S;
            const int ic = valid ? i : S - 1;
            const float z = zr[ic];
            const float zn = zr[ic < S - 1 ? ic + 1 : ic - 1];
            const float dist = (ic < S - 1 ? zn - z : z - zn) * dnorm;
            const float sg = a.sigma[ray * S + ic];
            float raw[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) raw[k] = a.color[(ray * S + ic) * 3 + k];
            composite_step<64>(ra, sg, raw, dist, valid, a.flags, lane,
                               a.weights_out ? a.weights_out + ray * S + ic : nullptr);
        }
        float out[4] = {ra.c0, ra.c1, ra.c2, ra.a};
        if (a.flags & NTX_FLAG_COMPOSITE_BKGD) {
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = out[k] + (1.0f - ra.a) * a.bkgd[k];
        }
        if (lane == 0) {
            a.color_out[3 * ray + 0] = out[0]; a.color_out[3 * ray + 1] = out[1];
            a.color_out[3 * ray + 2] = out[2]; a.alpha_out[ray] = out[3];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// ray generation (pixel_sampler.py:14-15, ray_sampler.py:23-48, proxy.py:13-35)
// ---------------------------------------------------------------------------------------------
struct RaygenConsts {                 // what every ray of a launch shares beside its camera
    float b0[3], b1[3];
    float half_w, half_h, near_t, far_t;
    int mode;
};

struct RaygenArgs {
    float c2w[16];
    RaygenConsts k;                   // b0 / b1, half_w / half_h, near_t / far_t, mode
    float focal;
    int width;
    int64_t pixel0, n;
    int64_t run_length, run_stride;   // local ray k = pixel pixel0 + (k / run_length) * run_stride + k % run_length
    const float *loc;                 // NULL, or image_plane_loc [n,2] = (row, col) of every ray as float32 (any pixel sampler)
    float *rays_o, *rays_d, *t, *cone;
};

// proxy.AABB.__call__ (proxy.py:13-35) for one ray; comparisons written exactly as tf.where does them so NaNs fall the same way
NTX_DEV void aabb_t(const float (&ro)[3], const float (&rd)[3], const float (&b0)[3], const float (&b1)[3], float &t0, float &t1) {
    float tmax = 0.0f, tmin = 0.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float inv = 1.0f / rd[r];
        const float ta = (b0[r] - ro[r]) * inv, tb = (b1[r] - ro[r]) * inv;
        const float lo = ta < tb ? ta : tb;
        const float hi = ta > tb ? ta : tb;
        if (r == 0) { tmax = lo; tmin = hi; }
        else {
            // reduce_max / reduce_min propagate NaN
            tmax = (lo != lo || tmax != tmax) ? __builtin_nanf("") : (lo > tmax ? lo : tmax);
            tmin = (hi != hi || tmin != tmin) ? __builtin_nanf("") : (hi < tmin ? hi : tmin);
        }
    }
    const bool hit = tmax < tmin;
    t0 = hit ? tmax : __builtin_inff();
    t1 = hit ? tmin : __builtin_inff();
}

// ray_sampler.rays_from_camera (ray_sampler.py:39-48) + Proxy (:32-37) / Frustum (:15-21) for ONE ray at the image-plane location (li, lj) =
// (row, col): the one statement of the generator's float32 arithmetic, shared by raygen_kernel (a camera in the kernel's arguments) and
// raygen_posed_kernel (cameras in device memory).  m: the top three rows of c2w, row-major with a row stride of 4.
NTX_DEV void raygen_ray(const float *m, float focal, const RaygenConsts &c, float li, float lj, int64_t k, float *rays_o, float *rays_d, float *t, float *cone_out) {
    const float d0 = (lj + 0.5f - c.half_w) / focal;                         // ray_sampler.py:41
    const float d1 = -(li + 0.5f - c.half_h) / focal;
    const float d2 = -1.0f;
    float rd[3], ro[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        rd[r] = (d0 * m[4 * r + 0] + d1 * m[4 * r + 1]) + d2 * m[4 * r + 2];   // :42
        ro[r] = m[4 * r + 3];                                                    // :43
    }
    const float nxy = __builtin_sqrtf(d0 * d0 + d1 * d1);
    const float nrm = __builtin_sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    const float cone = cosf(atanf(nxy)) / nrm / focal;                          // :46
    float t0, t1;
    if (c.mode == 0) {
        const float n = __builtin_sqrtf((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2]);  // :34
#pragma unroll
        for (int r = 0; r < 3; ++r) rd[r] = rd[r] / n;
        aabb_t(ro, rd, c.b0, c.b1, t0, t1);
    } else {
        t0 = c.near_t; t1 = c.far_t;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) { rays_o[3 * k + r] = ro[r]; rays_d[3 * k + r] = rd[r]; }
    t[2 * k] = t0; t[2 * k + 1] = t1;
    cone_out[k] = cone;
}

__global__ __launch_bounds__(256) void raygen_kernel(RaygenArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    float li, lj;                                                             // (row, col)
    if (a.loc) { li = a.loc[2 * k]; lj = a.loc[2 * k + 1]; }                  // the caller's image_plane_loc (ray_sampler.py:39)
    else {                                                                    // pixel_sampler.Full
        const int64_t pix = a.pixel0 + (k / a.run_length) * a.run_stride + k % a.run_length;
        li = (float)(pix / a.width); lj = (float)(pix % a.width);
    }
    raygen_ray(a.c2w, a.focal, a.k, li, lj, k, a.rays_o, a.rays_d, a.t, a.cone);
}

// ---------------------------------------------------------------------------------------------
// rays of a BATCH of cameras that live on the device (ntx_generate_rays_posed) and the adjoint of that map (ntx_generate_rays_posed_adjoint):
// ray k belongs to pose k / rays_per_pose.  poses [n_poses][3][4] (the top three rows of c2w, a row stride of 4 as in RaygenArgs::c2w),
// focal [n_poses].  The forward is raygen_ray per thread.
// ---------------------------------------------------------------------------------------------
struct RaygenPosedArgs {
    RaygenConsts k;
    const float *poses, *focal, *loc;
    int64_t n, rays_per_pose;
    float *rays_o, *rays_d, *t, *cone;
};

__global__ __launch_bounds__(256) void raygen_posed_kernel(RaygenPosedArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    const int64_t p = k / a.rays_per_pose;
    raygen_ray(a.poses + 12 * p, a.focal[p], a.k, a.loc[2 * k], a.loc[2 * k + 1], k, a.rays_o, a.rays_d, a.t, a.cone);
}

// The adjoint: ONE workgroup of POSED_ADJ_THREADS per pose.  Thread i adds the terms of the pose's rays i, i + POSED_ADJ_THREADS, ... in
// ascending order into 13 partial sums (dR 3x3, dT 3, the focal's sum), a butterfly adds the 64 lanes of a wave, a binary tree in LDS the
// waves: the order is a function of the pose's OWN ray count alone -- bit-reproducible, independent of n_poses, of the pose's place in the
// batch and of the grid; no atomics.  dc = (d0, d1, -1), v = R dc as the forward forms them (the same float32 expressions):
//     mode 0: g_v = (g_d - n (n . g_d)) / |v|, n = v / |v|;   mode 1: g_v = g_d
//     dR[r][c] += g_v[r] dc[c];   dT[r] += g_o[r];   s += g_v . (d0 R[:,0] + d1 R[:,1]);   d_focal = -(s / f)
// t and cone_scale are constants.  A ray whose g_d is exactly zero adds exact zeros whatever its direction is.
constexpr int POSED_ADJ_THREADS = 1024;
constexpr int POSED_ADJ_SUMS = 13;

struct RaygenPosedAdjointArgs {
    const float *poses, *focal, *loc, *d_rays_o, *d_rays_d;
    float half_w, half_h;
    int mode;
    int64_t n, rays_per_pose;
    float *d_poses, *d_focal;
};

__global__ __launch_bounds__(POSED_ADJ_THREADS) void raygen_posed_adjoint_kernel(RaygenPosedAdjointArgs a) {
    __shared__ float part[POSED_ADJ_THREADS / 64][POSED_ADJ_SUMS];
    const int64_t p = blockIdx.x;
    const int64_t first = p * a.rays_per_pose;
    const int64_t left = a.n - first;
    const int64_t count = left < a.rays_per_pose ? (left > 0 ? left : 0) : a.rays_per_pose;
    const float *m = a.poses + 12 * p;
    const float f = a.focal[p];
    float R[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = m[4 * r + c];
    float acc[POSED_ADJ_SUMS];
#pragma unroll
    for (int j = 0; j < POSED_ADJ_SUMS; ++j) acc[j] = 0.0f;
    for (int64_t i = threadIdx.x; i < count; i += POSED_ADJ_THREADS) {
        const int64_t k = first + i;
        const float li = a.loc[2 * k], lj = a.loc[2 * k + 1];
        const float go[3] = {a.d_rays_o[3 * k], a.d_rays_o[3 * k + 1], a.d_rays_o[3 * k + 2]};
        const float gd[3] = {a.d_rays_d[3 * k], a.d_rays_d[3 * k + 1], a.d_rays_d[3 * k + 2]};
        const float dc[3] = {(lj + 0.5f - a.half_w) / f, -(li + 0.5f - a.half_h) / f, -1.0f};
        float gv[3] = {gd[0], gd[1], gd[2]};
        const bool zero = gd[0] == 0.0f && gd[1] == 0.0f && gd[2] == 0.0f;
        if (a.mode == 0 && !zero) {
            float v[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) v[r] = (dc[0] * R[r][0] + dc[1] * R[r][1]) + dc[2] * R[r][2];
            const float len = __builtin_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            const float nv[3] = {v[0] / len, v[1] / len, v[2] / len};
            const float dot = (nv[0] * gd[0] + nv[1] * gd[1]) + nv[2] * gd[2];
#pragma unroll
            for (int r = 0; r < 3; ++r) gv[r] = (gd[r] - nv[r] * dot) / len;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[3 * r + c] += gv[r] * dc[c];
            acc[9 + r] += go[r];
        }
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < 3; ++r) s += gv[r] * (dc[0] * R[r][0] + dc[1] * R[r][1]);
        acc[12] += s;
    }
#pragma unroll
    for (int j = 0; j < POSED_ADJ_SUMS; ++j)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[j] += __shfl_xor(acc[j], d, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < POSED_ADJ_SUMS; ++j) part[wv][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < POSED_ADJ_SUMS) {
        const int j = threadIdx.x;
        float w[POSED_ADJ_THREADS / 64];
#pragma unroll
        for (int q = 0; q < POSED_ADJ_THREADS / 64; ++q) w[q] = part[q][j];
#pragma unroll
        for (int h = POSED_ADJ_THREADS / 128; h >= 1; h >>= 1)
#pragma unroll
            for (int q = 0; q < h; ++q) w[q] += w[q + h];
        if (j < 9) a.d_poses[12 * p + 4 * (j / 3) + j % 3] = w[0];
        else if (j < 12) a.d_poses[12 * p + 4 * (j - 9) + 3] = w[0];
        else a.d_focal[p] = w[0] == 0.0f ? 0.0f : -(w[0] / f);                  // (a zero sum gives +0, not -(0 / f) = -0)
    }
}

// proxy.AABB.__call__ on the caller's own rays (proxy.py:13-35): thread per ray
__global__ __launch_bounds__(256) void aabb_kernel(const float *rays_o, const float *rays_d, int64_t n, float b00, float b01, float b02,
                                                   float b10, float b11, float b12, float *t) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float ro[3] = {rays_o[3 * k], rays_o[3 * k + 1], rays_o[3 * k + 2]}, rd[3] = {rays_d[3 * k], rays_d[3 * k + 1], rays_d[3 * k + 2]};
    const float b0[3] = {b00, b01, b02}, b1[3] = {b10, b11, b12};
    float t0, t1;
    aabb_t(ro, rd, b0, b1, t0, t1);
    t[2 * k] = t0; t[2 * k + 1] = t1;
}

// ---------------------------------------------------------------------------------------------
// FourierFeatures alone (layer.py:8-23): thread per (row, component)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fourier_kernel(const float *x, int64_t m, int d, int nf, float *out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m * d) return;
    const int64_t row = k / d;
    const int c = (int)(k % d);
    const float v = x[k];
    float *o = out + row * (int64_t)(d * (1 + 2 * nf));
    o[c] = v;
    float f = 1.0f;
    for (int i = 0; i < nf; ++i) {
        // sin_q's three-step reduction holds its 1.5 ulp out to |x| = 2^17 (tests/kernel_emulation.py has the table); this entry point takes
        // n_freq <= 30 and any x, so beyond that the device library's sinf / cosf (full-range reduction) evaluate the band
        const float y = f * v;
        const bool far = !(__builtin_fabsf(y) < 0x1p17f);
        o[d + 2 * i * d + c] = far ? sinf(y) : sin_q(y, 0);
        o[d + (2 * i + 1) * d + c] = far ? cosf(y) : sin_q(y, 1);
        f *= 2.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// image epilogue (logger.py:128-144, util/interpolate.py:68-82): separable gaussian taps, stride = factor,
// TensorFlow 'SAME' zero padding, un-premultiply, optional uint8.  One thread per output pixel.
// ---------------------------------------------------------------------------------------------
constexpr int MAX_EPILOGUE_TAPS = 48;

struct EpilogueArgs {
    const float *rgba;
    float *out_f32;
    uint8_t *out_u8;
    int h, w, oh, ow, factor, taps, pad_top, pad_left;
    int unpremultiply;
    float k1[MAX_EPILOGUE_TAPS];   // normalised 1-D gaussian: the 2-D kernel is k1[i]*k1[j]
};

__global__ __launch_bounds__(256) void epilogue_kernel(EpilogueArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.oh * a.ow) return;
    const int oy = idx / a.ow, ox = idx % a.ow;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (a.factor > 1) {
        for (int i = 0; i < a.taps; ++i) {
            const int y = oy * a.factor + i - a.pad_top;
            if (y < 0 || y >= a.h) continue;
            for (int j = 0; j < a.taps; ++j) {
                const int x = ox * a.factor + j - a.pad_left;
                if (x < 0 || x >= a.w) continue;
                const float wgt = a.k1[i] * a.k1[j];
                const f32x4 p = reinterpret_cast<const f32x4 *>(a.rgba)[(int64_t)y * a.w + x];
                acc[0] = __builtin_fmaf(wgt, p.x, acc[0]); acc[1] = __builtin_fmaf(wgt, p.y, acc[1]);
                acc[2] = __builtin_fmaf(wgt, p.z, acc[2]); acc[3] = __builtin_fmaf(wgt, p.w, acc[3]);
            }
        }
    } else {
        const f32x4 p = reinterpret_cast<const f32x4 *>(a.rgba)[idx];
        acc[0] = p.x; acc[1] = p.y; acc[2] = p.z; acc[3] = p.w;
    }
    if (a.unpremultiply) {   // logger.py:133-135
        const float d = acc[3] + 1e-5f;
        acc[0] = acc[0] / d; acc[1] = acc[1] / d; acc[2] = acc[2] / d;
    }
    if (a.out_f32) reinterpret_cast<f32x4 *>(a.out_f32)[idx] = f32x4{acc[0], acc[1], acc[2], acc[3]};
    if (a.out_u8) {          // tf.image.convert_image_dtype: saturate(x * 255.5), truncated
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = acc[c] * 255.5f;
            v = v != v ? 0.0f : __builtin_fminf(__builtin_fmaxf(v, 0.0f), 255.0f);
            a.out_u8[4 * (int64_t)idx + c] = (uint8_t)v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// hierarchical sampling (renderer.py:125-130 + sample_pdf 589-617): per ray, invert the CDF of the coarse
// weights at n_imp positions and merge the new depths into the sorted coarse ones.  One wave per ray.
// ---------------------------------------------------------------------------------------------
constexpr int MAX_PDF_SAMPLES = 512;   // coarse samples and importance samples each

struct SamplePdfArgs {
    const float *t, *z_vals, *weights, *u;
    float *z_out;
    int64_t n_rays;
    int n_samples, n_imp;
    float delta, delta_u;   // float32 steps of tf.linspace(0,1,S) and tf.linspace(0,1,n_imp)
    uint32_t flags, seed_lo, seed_hi;   // NTX_FLAG_PERTURB: the coarse depths carry the jitter of the render kernel
    uint32_t idx_run;                   // ... keyed by the ray's global index (RenderArgs)
    int64_t idx0, idx_stride;
};

__global__ __launch_bounds__(256) void sample_pdf_kernel(SamplePdfArgs a) {
    __shared__ float cdf_all[4][MAX_PDF_SAMPLES], bins_all[4][MAX_PDF_SAMPLES], vals_all[4][2 * MAX_PDF_SAMPLES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *cdf = cdf_all[wv], *bins = bins_all[wv], *vals = vals_all[wv];
    const int64_t wave = (int64_t)blockIdx.x * 4 + wv, nwaves = (int64_t)gridDim.x * 4;
    const int S = a.n_samples, NI = a.n_imp, NB = S - 1, NT = S + NI;
    for (int64_t ray = wave; ray < a.n_rays; ray += nwaves) {
        const float t0 = a.t[2 * ray], t1 = a.t[2 * ray + 1];
        float *zo = a.z_out + ray * NT;
        if (t0 == __builtin_inff()) {   // culled ray: no weights exist; the fused kernel never reads its depths
            for (int i = lane; i < NT; i += 64) zo[i] = 0.0f;
            continue;
        }
        auto z_at = [&](int i) -> float {
            if (a.z_vals) return a.z_vals[ray * S + i];
            if (a.flags & NTX_FLAG_PERTURB)
                return z_jittered(a.delta, global_index(a.idx0, a.idx_run, a.idx_stride, ray), i, t0, t1, S, a.seed_lo, a.seed_hi);
            return z_lin(a.delta, i, t0, t1, S);
        };
        const float *w = a.weights + ray * S;
        // pdf over the S-2 interior weights (+1e-5), cdf with a leading 0: S-1 entries; bins = S-1 midpoints
        float part = 0.0f;
        for (int i = lane; i < S - 2; i += 64) part += w[i + 1] + 1e-5f;
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
        const float total = part;
        float carry = 0.0f;
        for (int base = 0; base < S - 2; base += 64) {
            const int i = base + lane;
            float p = i < S - 2 ? (w[i + 1] + 1e-5f) / total : 0.0f;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const float v = __shfl_up(p, d, 64);
                if (lane >= d) p += v;
            }
            if (i < S - 2) cdf[i + 1] = carry + p;
            carry += __shfl(p, 63, 64);
        }
        if (lane == 0) cdf[0] = 0.0f;
        for (int i = lane; i < NB; i += 64) bins[i] = 0.5f * (z_at(i + 1) + z_at(i));
        for (int i = lane; i < S; i += 64) vals[i] = z_at(i);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < NI; k += 64) {
            const float u = a.u ? a.u[ray * NI + k] : (k == 0 ? 0.0f : (k == NI - 1 ? 1.0f : a.delta_u * (float)k));
            int lo = 0, hi = NB;                       // searchsorted(cdf, u, side='right')
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
            }
            const int below = lo - 1 > 0 ? lo - 1 : 0, above = lo < NB - 1 ? lo : NB - 1;
            float denom = cdf[above] - cdf[below];
            if (denom < 1e-5f) denom = 1.0f;
            const float tt = (u - cdf[below]) / denom;
            vals[S + k] = bins[below] + tt * (bins[above] - bins[below]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // tf.sort(concat[z_vals, z_samples]) (renderer.py:130).  With the deterministic u (an increasing linspace) the
        // samples come out non-decreasing like the coarse depths, so the sort is a MERGE: the rank of coarse value i is
        // i + #{samples < v}, of sample k it is k + #{coarse <= v} (equal values are interchangeable) -- one binary search
        // instead of NT comparisons per value.  Checked, not assumed: any inversion in either run takes the general path.
        bool ordered = true;
        for (int i = lane; i < NT - 1; i += 64)
            if (i != S - 1 && !(vals[i] <= vals[i + 1])) ordered = false;
        if (__ballot(!ordered) == 0ull) {
            for (int i = lane; i < NT; i += 64) {
                const float v = vals[i];
                const bool coarse = i < S;
                const float *other = coarse ? vals + S : vals;
                int lo = 0, hi = coarse ? NI : S;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const bool before = coarse ? other[mid] < v : other[mid] <= v;
                    if (before) lo = mid + 1; else hi = mid;
                }
                zo[(coarse ? i : i - S) + lo] = v;
            }
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        // unsorted u: rank of every value = #smaller + #equal-with-lower-index
        for (int i = lane; i < NT; i += 64) {
            const float v = vals[i];
            int rank = 0;
            for (int jx = 0; jx < NT; ++jx) {
                const float o = vals[jx];
                rank += (o < v) || (o == v && jx < i);
            }
            zo[rank] = v;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------
// hit-ray compaction, first step of ntx_render_rays at both precisions: rays culled by the proxy (t0 == inf,
// renderer.py:58-67) get their final value here (0, or the background colour: renderer.py:81-86); the indices of the
// others are appended to hit_list (the order across workgroups is irrelevant, results are stored per ray).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compact_hits_kernel(const float *t, int64_t n_rays, int32_t *hit_list, int32_t *hit_count,
                                                           float *color_out, float *alpha_out, uint32_t flags, float b0, float b1, float b2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < n_rays;
    const bool hit = in && !(t[2 * i] == __builtin_inff());   // NaN counts as a hit, as in render_kernel
    // block-aggregated append: ranks within the wave by ballot, wave offsets through LDS, ONE atomic per workgroup
    // (640 000 rays = 2 500 atomics on the one counter instead of 10 000)
    __shared__ int wave_count[4], block_base;
    const uint64_t m = __ballot(hit);
    const int wv = threadIdx.x >> 6;
    if (lane == 0) wave_count[wv] = (int)__builtin_popcountll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
        block_base = total ? atomicAdd(hit_count, total) : 0;
    }
    __syncthreads();
    int base = block_base;
    for (int k = 0; k < wv; ++k) base += wave_count[k];
    if (hit) hit_list[base + (int)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
    if (in && !hit) {
        const bool bk = (flags & NTX_FLAG_COMPOSITE_BKGD) != 0;
        color_out[3 * i + 0] = bk ? b0 : 0.0f; color_out[3 * i + 1] = bk ? b1 : 0.0f; color_out[3 * i + 2] = bk ? b2 : 0.0f;
        alpha_out[i] = 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// ray order of the instanced kernels: longest first.  The rays of a chunk cost 0 .. S/32 network batches each and the
// waves take them off a shared counter; with ~16 rays per wave the kernel ends one average ray after its mean finishing
// time (5.7 % of the carpet_instanced workload, measured by quadrupling the chunk).  Handing the rays out in DESCENDING
// cost (a counting sort on the number of in-patch samples, 512 bins) leaves only the cheapest rays for the end.
// inst_count: one wave per ray, counts dists > 0 (hit rays), the row read with 16-byte loads that are all in flight at once;
// inst_order: ONE workgroup -- histogram, exclusive scan from the costliest bin down and scatter, all on LDS atomics (round 2
// used global atomics, ~16 000 of them on ~20 addresses, one L2 round trip each: 110 + 53 us of a 19.5 ms call; now ~25 us in
// all), and it zeroes the hand-out counter of the main kernel.  The order inside a bin is whatever the atomics make it;
// results do not depend on it (instance_kernel: position-independent composite).
// ---------------------------------------------------------------------------------------------
constexpr int INST_BINS = 512;
NTX_DEV int inst_bin(int count) { const int b = count >> 3; return INST_BINS - 1 - (b < INST_BINS ? b : INST_BINS - 1); }   // bin 0 = costliest

__global__ __launch_bounds__(256) void inst_count_kernel(const float *__restrict__ dists, const uint8_t *__restrict__ hit, int64_t n_rays, int S,
                                                         int32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    int n = 0;
    if (hit[ray]) {
        const float *drow = dists + ray * S;
        if ((S & 3) == 0 && (reinterpret_cast<uintptr_t>(dists) & 15) == 0) {
            const f32x4 *d4 = reinterpret_cast<const f32x4 *>(drow);
            const int q = S >> 2;
            for (int i0 = 0; i0 < q; i0 += 256) {   // 4 loads of 16 bytes in flight per lane = 4 KiB per wave and step
                f32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int i = i0 + 64 * u + lane; v[u] = i < q ? d4[i] : f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
#pragma unroll
                for (int u = 0; u < 4; ++u) n += (v[u][0] > 0.0f) + (v[u][1] > 0.0f) + (v[u][2] > 0.0f) + (v[u][3] > 0.0f);
            }
        } else {
            for (int i = lane; i < S; i += 64) n += drow[i] > 0.0f ? 1 : 0;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    }
    if (lane == 0) count[ray] = n;
}

// The hand-out of the float32 instance kernel is in CHUNKS of the cost order (ntx_device.h: bundles of rays share what is paid per
// claim): 4 rays, 2 or 1.  inst_order_kernel also says where: a chunk may cost at most HALF of a wave's average share of the work
// (a chunk of the costliest rays that is a whole share leaves its wave behind for good: +12 % at 8 rays per wave, measured), and the
// hand-out ends in pairs and then single rays, the last tb = 3 rays per wave single, the last ta = 6 not in fours, so that the ragged end
// stays one cheap ray's worth.  chunk_tab = {r1, q0, q1, p1}: ranks [0, r1) single, [r1, q0) pairs, [q0, q1) fours, [q1, p1) pairs,
// [p1, n) single.  (Counts are known per bin of 8: the bin a limit falls into counts as above it.)
constexpr int INST_ORDER_THREADS = 1024;
__global__ __launch_bounds__(INST_ORDER_THREADS) void inst_order_kernel(const int32_t *__restrict__ count, int64_t n_rays, int32_t *__restrict__ order,
                                                                        int32_t *__restrict__ work_counter, int n_waves, int ta, int tb,
                                                                        int32_t *__restrict__ chunk_tab) {
    __shared__ int32_t v[INST_BINS], off[INST_BINS];
    __shared__ unsigned long long total;
    const int i = threadIdx.x;
    if (i < INST_BINS) v[i] = 0;
    if (i == 0) { *work_counter = 0; total = 0ull; }   // the main kernel's hand-out starts from 0
    __syncthreads();
    unsigned long long mine = 0ull;
    for (int64_t r = i; r < n_rays; r += INST_ORDER_THREADS) { const int c = count[r]; mine += (unsigned long long)c; atomicAdd(&v[inst_bin(c)], 1); }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((i & 63) == 0) atomicAdd(&total, mine);
    __syncthreads();
    if (i < INST_BINS) off[i] = v[i];
    __syncthreads();
    for (int d = 1; d < INST_BINS; d <<= 1) {          // inclusive scan over the bins, costliest first
        int32_t add = 0;
        if (i < INST_BINS && i >= d) add = off[i - d];
        __syncthreads();
        if (i < INST_BINS) off[i] += add;
        __syncthreads();
    }
    if (i == 0) {
        const int64_t n = n_rays, w = n_waves > 0 ? n_waves : 1;
        const int64_t half_share = (int64_t)(total / (unsigned long long)(2 * w));     // samples
        int64_t r1 = n, r2 = n;                                                        // ta < 0: single rays throughout
        if (ta >= 0) {
            r1 = off[inst_bin((int)(half_share / 2 < 0x7fffffff ? half_share / 2 : 0x7fffffff))];   // ranks below: a pair would cost more than half a share
            r2 = off[inst_bin((int)(half_share / 4 < 0x7fffffff ? half_share / 4 : 0x7fffffff))];   // ... a four
        }
        auto clamp = [](int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : x > hi ? hi : x; };
        int64_t p1 = clamp(n - tb * w, r1, n);
        int64_t q1 = clamp(n - ta * w, r1, p1);
        int64_t q0 = clamp(r2 > r1 ? r2 : r1, r1, q1);
        q0 = r1 + ((q0 - r1 + 1) & ~(int64_t)1); if (q0 > q1) q0 = r1 + ((q1 - r1) & ~(int64_t)1);   // whole pairs in front of the fours
        q1 = q0 + ((q1 - q0) & ~(int64_t)3);
        p1 = q1 + ((p1 - q1) & ~(int64_t)1);
        chunk_tab[0] = (int32_t)r1; chunk_tab[1] = (int32_t)q0; chunk_tab[2] = (int32_t)q1; chunk_tab[3] = (int32_t)p1;
    }
    if (i < INST_BINS) v[i] = off[i] - v[i];           // exclusive: the first place of bin i
    __syncthreads();
    for (int64_t r = i; r < n_rays; r += INST_ORDER_THREADS) order[atomicAdd(&v[inst_bin(count[r])], 1)] = (int32_t)r;
}

// ---------------------------------------------------------------------------------------------
// sample depths alone (renderer.py:101-111 / 374-383): the z_vals the fused kernels place internally, for parity
// tests and for callers that want them.  Thread per (ray, point).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_depths_kernel(const float *t, int64_t n_rays, int npts, float delta, uint32_t flags,
                                                            uint32_t seed_lo, uint32_t seed_hi, int64_t idx0, uint32_t idx_run,
                                                            int64_t idx_stride, float *z_out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_rays * npts) return;
    const int64_t ray = k / npts;
    const int i = (int)(k % npts);
    const float t0 = t[2 * ray], t1 = t[2 * ray + 1];
    z_out[k] = (flags & NTX_FLAG_PERTURB) ? z_jittered(delta, global_index(idx0, idx_run, idx_stride, ray), i, t0, t1, npts, seed_lo, seed_hi)
                                          : z_lin(delta, i, t0, t1, npts);
}

// packed[i] = idx[i] >= 0 ? w[idx[i]] : konst[i]: the weight image remade where the weights are
__global__ void gather_weights_kernel(const float *__restrict__ w, const int32_t *__restrict__ idx, const float *__restrict__ konst, size_t n, float *__restrict__ packed) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t g = idx[i];
    packed[i] = g >= 0 ? w[g] : konst[i];
}

// noise_out[ray][i] = raw_noise_std * N(0,1): the very draws the render kernels add to the density (ntx_device.h normal01)
__global__ __launch_bounds__(256) void sample_noise_kernel(int64_t n_rays, int npts, float noise_std, uint32_t seed_lo, uint32_t seed_hi, int64_t idx0,
                                                           uint32_t idx_run, int64_t idx_stride, float *noise_out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_rays * npts) return;
    const int64_t ray = k / npts;
    noise_out[k] = noise_std * normal01(global_index(idx0, idx_run, idx_stride, ray), (int)(k % npts), seed_lo, seed_hi);
}

}  // namespace ntx
