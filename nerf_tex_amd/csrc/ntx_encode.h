// ntx_encode.h -- what a training step's encoders compute, each formula once: the ray and its parameter row (renderer.py:98, :155-158, :386),
// the rows of layer.FourierFeatures (layer.py:14-23), the distances between samples (renderer.py:174-180, :441-444) and the O-layout index.
// The chain's encoders (a wave per 32 samples), the chain's per-ray direction row and the layer-by-layer encoder (a thread per sample and
// feature) differ in which thread takes which value and where it goes; every value comes from here, so they agree bit for bit.  gfx950 only.
#pragma once
#include "ntx_device.h"   // ntx::sin_q
namespace ntx_train {
// O layout: a block of 32 samples x `tiles` tiles of 32 rows; element (row, sample p of the block) -- the weight gradients' A operands
// (ntx_train_device.h).  The composite's narrow tile (tiles = 1, rows 0 .. 3) and the host's decode of a kept activation read the same index.
__host__ __device__ constexpr size_t o_index(long long blk, int tiles, int row, int p) {
    return (((size_t)blk * tiles + (row >> 5)) * 4 + (p >> 3)) * 256 + ((row & 31) + 32 * ((p >> 2) & 1)) * 4 + (p & 3);
}

// A ray: its un-normalised direction, |d|, and its row of `width` parameters (rays_per_param_row consecutive rays share one)
struct RayCtx {
    float d[3], dn; const float *pr;
    __device__ __forceinline__ float dcomp(int c) const { return c == 0 ? d[0] : c == 1 ? d[1] : d[2]; }       // (selects: no indexed register array)
    __device__ __forceinline__ float dir(int c) const { return dcomp(c) / dn; }                                  // renderer.py:98
    __device__ __forceinline__ float point(float o_c, int c, float z) const { return o_c + dcomp(c) * z; }      // :114: component c of the sample point, o_c the origin's
};
__device__ __forceinline__ RayCtx ray_ctx(const float *rays_d, const float *params, long long rays_per_param_row, long long ray, int width) {
    RayCtx r; r.d[0] = rays_d[3 * ray]; r.d[1] = rays_d[3 * ray + 1]; r.d[2] = rays_d[3 * ray + 2];
    r.dn = sqrtf((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]);
    r.pr = params + (size_t)(ray / rays_per_param_row) * (width > 0 ? width : 1);
    return r;
}
// A ray that misses the proxy (t = inf: the reference's Renderer.__call__ filters it out and scatters 0 / the background back, renderer.py:58-86)
// stays in the batch with depth 0 and distances 0: every alpha of it is 1 - exp(-sigma 0) = 0, so it composites to exactly 0 / the background,
// no gradient flows into or out of its rows, and the loss still counts it among its rays
__device__ __forceinline__ float depth_of(float zr, bool &hit) { hit = isfinite(zr); return hit ? zr : 0.0f; }
// Renderer: parameter c of a sample, blur_idx's scaled by the sample's footprint (:155-158; a missing ray's cone scale may be anything)
__device__ __forceinline__ float blurred_param(const float *pr, int c, int blur_idx, bool hit, const float *cone, long long ray, float z) {
    return c == blur_idx ? (hit ? pr[c] * (cone[ray] * z) : 0.0f) : pr[c];
}
// MipRenderer: the rows hold P + 1 values, the model sees the P beside column `splice` (:386); splice < 0: the rows as they are
__device__ __forceinline__ float spliced_param(const float *pr, int k, int splice) { return pr[splice < 0 || k < splice ? k : k + 1]; }

// FourierFeatures(x[0 .. D), L) = [x | sin(2^0 x) | cos(2^0 x) | sin(2^1 x) | ...], every block D wide: the value of (band, h = 0 sin / 1 cos),
// the row it lands on, and row r as a function of r
__device__ __forceinline__ float fourier_value(float x, int band, int h) { return ntx::sin_q(ldexpf(1.0f, band) * x, h); }
// ... and its slope d/dx: 2^band cos(2^band x) for the sine row, -2^band sin(2^band x) for the cosine row -- on the same sin_q the value
// came from (the way back from the parameter features to the parameters: ntx_trainer_enable_param_gradients)
__device__ __forceinline__ float fourier_slope(float x, int band, int h) {
    const float w = ldexpf(1.0f, band), s = ntx::sin_q(w * x, 1 - h);
    return h ? -(w * s) : w * s;
}
__device__ __forceinline__ int fourier_row_of(int D, int band, int h, int c) { return D + 2 * D * band + h * D + c; }
template <class X>
__device__ __forceinline__ float fourier_row(int r, int D, X x) {
    if (r < D) return x(r);
    const int q = r - D, band = q / (2 * D), hc = q - band * 2 * D, h = hc / D, c = hc - h * D;
    return fourier_value(x(c), band, h);
}
__device__ __forceinline__ int fourier_width(int D, int L) { return D * (1 + 2 * L); }

// dists of sample s: z[s+1] - z[s], the last one repeated (zray: the ray's S depths, z: sample s's), or the width of the mip segment
// [e0, e1] with no copy of the last one; times |rays_d|, and 0 on a ray that misses
__device__ __forceinline__ float sample_dist(const float *zray, int s, int S, float z, bool hit, float dn) {
    const float zn = s + 1 < S ? zray[s + 1] : 0.0f;
    const float dist = s + 1 < S ? zn - z : (S > 1 ? z - zray[s - 1] : 0.0f);
    return hit ? dist * dn : 0.0f;
}
__device__ __forceinline__ float segment_dist(float e0, float e1, bool hit, float dn) { return hit ? (e1 - e0) * dn : 0.0f; }
}   // namespace ntx_train
