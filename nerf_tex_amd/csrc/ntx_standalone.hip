// ntx_standalone.hip -- the entries of the C ABI that need no context: ray generation, the proxy intersection, Fourier features, the composite,
// the samplers and the image epilogue -- and every launch from ntx_small_kernels.h, those of the context's entries (nerftex.hip) included.  gfx950 only.
#include <cstring>
#include "ntx_entry.h"
#include "ntx_small_kernels.h"

using namespace ntx;

// what the rays of one launch share beside their camera
static RaygenConsts raygen_consts(int height, int width, int mode, const float *b0, const float *b1, float near_t, float far_t) {
    RaygenConsts k{};
    if (mode == 0) { memcpy(k.b0, b0, sizeof(k.b0)); memcpy(k.b1, b1, sizeof(k.b1)); }
    k.half_w = (float)(.5 * width);   // `.5 * width` is evaluated by python, then cast (ray_sampler.py:41)
    k.half_h = (float)(.5 * height);
    k.near_t = near_t; k.far_t = far_t;
    k.mode = mode;
    return k;
}

// the generator's launch for n rays: pixels pixel0 .. in runs (loc NULL), or the image-plane locations loc[n][2]
static int launch_raygen(const float *c2w, int height, int width, float focal, int64_t pixel0, int64_t n, int64_t run_length, int64_t run_stride, const float *loc, int mode,
                         const float *b0, const float *b1, float near_t, float far_t, float *rays_o, float *rays_d, float *t, float *cone_scale, ntx_stream stream) {
    RaygenArgs a{};
    memcpy(a.c2w, c2w, sizeof(a.c2w));
    a.k = raygen_consts(height, width, mode, b0, b1, near_t, far_t);
    a.focal = focal;
    a.width = width;
    a.pixel0 = pixel0; a.n = n;
    a.run_length = run_length; a.run_stride = run_stride;
    a.loc = loc;
    a.rays_o = rays_o; a.rays_d = rays_d; a.t = t; a.cone = cone_scale;
    raygen_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

namespace ntx {
void launch_gather_weights(hipStream_t st, const float *w, const int32_t *idx, const float *konst, size_t n, float *packed) {
    gather_weights_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(w, idx, konst, n, packed);
}
void launch_compact_hits(hipStream_t st, const float *t, int64_t n_rays, int32_t *hit_list, int32_t *hit_count, float *color_out, float *alpha_out, uint32_t flags,
                         const float *bkgd) {
    compact_hits_kernel<<<dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st>>>(t, n_rays, hit_list, hit_count, color_out, alpha_out, flags, bkgd[0], bkgd[1], bkgd[2]);
}
void launch_inst_order(hipStream_t st, const float *dists, const uint8_t *hit, int64_t n_rays, int n_samples, int32_t *count, int32_t *order, int32_t *work_counter,
                       int n_waves, int ta, int tb, int32_t *chunk_tab) {
    inst_count_kernel<<<dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, st>>>(dists, hit, n_rays, n_samples, count);
    inst_order_kernel<<<dim3(1), dim3(INST_ORDER_THREADS), 0, st>>>(count, n_rays, order, work_counter, n_waves, ta, tb, chunk_tab);
}
}  // namespace ntx

extern "C" {

int ntx_generate_rays_strided(const float *c2w, int height, int width, float focal, int64_t pixel0, int64_t n_pixels,
                              int64_t run_length, int64_t run_stride, int mode, const float *b0, const float *b1,
                              float near_t, float far_t, float *rays_o, float *rays_d, float *t, float *cone_scale,
                              ntx_stream stream) {
    if (!c2w || !rays_o || !rays_d || !t || !cone_scale) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (height <= 0 || width <= 0 || n_pixels < 0 || pixel0 < 0 || run_length < 1 || run_stride < run_length)
        return ntx_set_error(NTX_E_INVALID, "bad pixel set: pixel0 %lld n %lld run_length %lld run_stride %lld", (long long)pixel0,
                    (long long)n_pixels, (long long)run_length, (long long)run_stride);
    if (n_pixels > 0) {
        const int64_t last = pixel0 + ((n_pixels - 1) / run_length) * run_stride + (n_pixels - 1) % run_length;
        if (last >= (int64_t)height * width)
            return ntx_set_error(NTX_E_INVALID, "pixel set [%lld .. %lld] outside %dx%d", (long long)pixel0, (long long)last, height, width);
    }
    if (mode != 0 && mode != 1) return ntx_set_error(NTX_E_INVALID, "mode must be 0 (Proxy/AABB) or 1 (Frustum)");
    if (mode == 0 && (!b0 || !b1)) return ntx_set_error(NTX_E_INVALID, "AABB bounds are NULL");
    if (n_pixels == 0) return NTX_OK;
    return launch_raygen(c2w, height, width, focal, pixel0, n_pixels, run_length, run_stride, nullptr, mode, b0, b1, near_t, far_t, rays_o, rays_d, t, cone_scale, stream);
}

int ntx_generate_rays_at(const float *c2w, int height, int width, float focal, const float *image_plane_loc, int64_t n_rays, int mode,
                         const float *b0, const float *b1, float near_t, float far_t, float *rays_o, float *rays_d, float *t,
                         float *cone_scale, ntx_stream stream) {
    if (!c2w || !rays_o || !rays_d || !t || !cone_scale) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (height <= 0 || width <= 0 || n_rays < 0) return ntx_set_error(NTX_E_INVALID, "bad shape %dx%d, n_rays %lld", height, width, (long long)n_rays);
    if (mode != 0 && mode != 1) return ntx_set_error(NTX_E_INVALID, "mode must be 0 (Proxy/AABB) or 1 (Frustum)");
    if (mode == 0 && (!b0 || !b1)) return ntx_set_error(NTX_E_INVALID, "AABB bounds are NULL");
    if (n_rays == 0) return NTX_OK;
    if (!image_plane_loc) return ntx_set_error(NTX_E_INVALID, "image_plane_loc is NULL");
    return launch_raygen(c2w, height, width, focal, 0, n_rays, 1, 1, image_plane_loc, mode, b0, b1, near_t, far_t, rays_o, rays_d, t, cone_scale, stream);
}

// the argument checks the two posed entries share: the cameras, the image size and the split of the rays over the poses
static int check_posed(const float *poses, const float *focal, int64_t n_poses, int height, int width, const float *image_plane_loc, int64_t n_rays, int64_t rays_per_pose,
                       int mode) {
    if (!poses || !focal || !image_plane_loc) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (height <= 0 || width <= 0 || n_rays < 0) return ntx_set_error(NTX_E_INVALID, "bad shape %dx%d, n_rays %lld", height, width, (long long)n_rays);
    if (mode != 0 && mode != 1) return ntx_set_error(NTX_E_INVALID, "mode must be 0 (Proxy/AABB) or 1 (Frustum)");
    if (n_poses < 1 || n_poses > 0x7fffffff || rays_per_pose < 1)
        return ntx_set_error(NTX_E_INVALID, "n_poses %lld outside [1, 2^31), or rays_per_pose %lld < 1", (long long)n_poses, (long long)rays_per_pose);
    if (n_rays > 0 && (n_rays - 1) / rays_per_pose + 1 != n_poses)
        return ntx_set_error(NTX_E_INVALID, "%lld rays at %lld per pose are %lld poses, not %lld", (long long)n_rays, (long long)rays_per_pose,
                             (long long)((n_rays - 1) / rays_per_pose + 1), (long long)n_poses);
    return NTX_OK;
}

int ntx_generate_rays_posed(const float *poses, const float *focal, int64_t n_poses, int height, int width, const float *image_plane_loc, int64_t n_rays,
                            int64_t rays_per_pose, int mode, const float *b0, const float *b1, float near_t, float far_t, float *rays_o, float *rays_d, float *t,
                            float *cone_scale, void *stream) {
    if (!rays_o || !rays_d || !t || !cone_scale) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (int rc = check_posed(poses, focal, n_poses, height, width, image_plane_loc, n_rays, rays_per_pose, mode)) return rc;
    if (mode == 0 && (!b0 || !b1)) return ntx_set_error(NTX_E_INVALID, "AABB bounds are NULL");
    if (n_rays == 0) return NTX_OK;
    RaygenPosedArgs a{};
    a.k = raygen_consts(height, width, mode, b0, b1, near_t, far_t);
    a.poses = poses; a.focal = focal; a.loc = image_plane_loc;
    a.n = n_rays; a.rays_per_pose = rays_per_pose;
    a.rays_o = rays_o; a.rays_d = rays_d; a.t = t; a.cone = cone_scale;
    raygen_posed_kernel<<<dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_generate_rays_posed_adjoint(const float *poses, const float *focal, int64_t n_poses, int height, int width, const float *image_plane_loc, int64_t n_rays,
                                    int64_t rays_per_pose, int mode, const float *d_rays_o, const float *d_rays_d, float *d_poses, float *d_focal, void *stream) {
    if (!d_rays_o || !d_rays_d || !d_poses || !d_focal) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (int rc = check_posed(poses, focal, n_poses, height, width, image_plane_loc, n_rays, rays_per_pose, mode)) return rc;
    RaygenPosedAdjointArgs a{};
    a.poses = poses; a.focal = focal; a.loc = image_plane_loc; a.d_rays_o = d_rays_o; a.d_rays_d = d_rays_d;
    a.half_w = (float)(.5 * width); a.half_h = (float)(.5 * height);
    a.mode = mode;
    a.n = n_rays; a.rays_per_pose = rays_per_pose;
    a.d_poses = d_poses; a.d_focal = d_focal;
    raygen_posed_adjoint_kernel<<<dim3((unsigned)n_poses), dim3(POSED_ADJ_THREADS), 0, (hipStream_t)stream>>>(a);   // n_rays = 0: zeros for every pose
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_generate_rays(const float *c2w, int height, int width, float focal, int64_t pixel0, int64_t n_pixels,
                      int mode, const float *b0, const float *b1, float near_t, float far_t, float *rays_o,
                      float *rays_d, float *t, float *cone_scale, ntx_stream stream) {
    const int64_t run = n_pixels > 0 ? n_pixels : 1;
    return ntx_generate_rays_strided(c2w, height, width, focal, pixel0, n_pixels, run, run, mode, b0, b1, near_t, far_t, rays_o,
                                     rays_d, t, cone_scale, stream);
}

int ntx_aabb_intersect(const float *rays_o, const float *rays_d, int64_t n_rays, const float *b0, const float *b1, float *t,
                       ntx_stream stream) {
    if (n_rays < 0) return ntx_set_error(NTX_E_INVALID, "n_rays < 0");
    if (!b0 || !b1) return ntx_set_error(NTX_E_INVALID, "AABB bounds are NULL");
    if (n_rays == 0) return NTX_OK;
    if (!rays_o || !rays_d || !t) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    aabb_kernel<<<dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(rays_o, rays_d, n_rays, b0[0], b0[1], b0[2],
                                                                                                b1[0], b1[1], b1[2], t);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_fourier_features(const float *x, int64_t m, int d, int n_freq, float *out, ntx_stream stream) {
    if (m < 0 || d <= 0 || n_freq < 0 || n_freq > 30) return ntx_set_error(NTX_E_INVALID, "bad shape m=%lld d=%d n_freq=%d", (long long)m, d, n_freq);
    if (m == 0) return NTX_OK;
    if (!x || !out) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    const int64_t nb = (m * d + 255) / 256;
    fourier_kernel<<<dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream>>>(x, m, d, n_freq, out);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_composite(const float *color, const float *sigma, const float *z_vals, const float *rays_d, int64_t n_rays,
                  int n_samples, uint32_t flags, const float *bkgd, float *color_out, float *alpha_out,
                  float *weights_out, ntx_stream stream) {
    if (n_rays < 0) return ntx_set_error(NTX_E_INVALID, "n_rays < 0");
    if (n_samples < 2) return ntx_set_error(NTX_E_INVALID, "n_samples must be >= 2 (renderer.py:174-177 needs a previous step)");
    if (n_rays == 0) return NTX_OK;
    if (!color || !sigma || !z_vals || !rays_d || !color_out || !alpha_out) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    CompositeArgs a{};
    a.color = color; a.sigma = sigma; a.z = z_vals; a.rays_d = rays_d;
    a.color_out = color_out; a.alpha_out = alpha_out; a.weights_out = weights_out;
    a.n_rays = n_rays; a.n_samples = n_samples; a.flags = flags;
    for (int k = 0; k < 3; ++k) a.bkgd[k] = bkgd ? bkgd[k] : 1.0f;
    int64_t nb = (n_rays + 3) / 4;
    if (nb > 256 * 8) nb = 256 * 8;   // 8 workgroups per CU, grid-stride over rays
    composite_kernel<<<dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_sample_depths(const float *t, int64_t n_rays, int n_points, uint32_t flags, uint64_t perturb_seed,
                      const ntx_render_opts *opts, float *z_out, ntx_stream stream) {
    if (n_rays < 0) return ntx_set_error(NTX_E_INVALID, "n_rays < 0");
    if (n_points < 2) return ntx_set_error(NTX_E_INVALID, "n_points must be >= 2");
    IndexMap im;
    if (int rc = index_map_of(opts, &im)) return rc;
    if (n_rays > 0x7fffffff) return ntx_set_error(NTX_E_INVALID, "n_rays %lld exceeds int32", (long long)n_rays);
    if (n_rays == 0) return NTX_OK;
    if (!t || !z_out) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    const int64_t n = n_rays * n_points;
    sample_depths_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        t, n_rays, n_points, 1.0f / (float)(n_points - 1), flags, (uint32_t)perturb_seed, (uint32_t)(perturb_seed >> 32), im.idx0, im.run,
        im.stride, z_out);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_sample_noise(int64_t n_rays, int n_points, uint64_t seed, const ntx_render_opts *opts, float *noise_out, ntx_stream stream) {
    if (n_rays < 0 || n_points < 1) return ntx_set_error(NTX_E_INVALID, "n_rays < 0 or n_points < 1");
    IndexMap im;
    if (int rc = index_map_of(opts, &im)) return rc;
    float noise_std = 0.0f;
    if (int rc = noise_of(opts, NTX_FLAG_RAW_NOISE, &noise_std)) return rc;
    if (n_rays > 0x7fffffff) return ntx_set_error(NTX_E_INVALID, "n_rays %lld exceeds int32", (long long)n_rays);
    if (n_rays == 0) return NTX_OK;
    if (!noise_out) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    const int64_t n = n_rays * n_points;
    sample_noise_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(n_rays, n_points, noise_std, (uint32_t)seed, (uint32_t)(seed >> 32), im.idx0,
                                                                                                   im.run, im.stride, noise_out);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_sample_pdf(const float *t, const float *z_vals, const float *weights, const float *u, int64_t n_rays,
                   int n_samples, int n_importance, uint32_t flags, uint64_t perturb_seed, const ntx_render_opts *opts, float *z_out,
                   ntx_stream stream) {
    if (n_rays < 0) return ntx_set_error(NTX_E_INVALID, "n_rays < 0");
    IndexMap im;
    if (int rc = index_map_of(opts, &im)) return rc;
    if (n_rays > 0x7fffffff) return ntx_set_error(NTX_E_INVALID, "n_rays %lld exceeds int32", (long long)n_rays);
    if (n_samples < 3 || n_samples > MAX_PDF_SAMPLES) return ntx_set_error(NTX_E_INVALID, "n_samples %d outside [3,%d]", n_samples, MAX_PDF_SAMPLES);
    if (n_importance < 1 || n_importance > MAX_PDF_SAMPLES) return ntx_set_error(NTX_E_INVALID, "n_importance %d outside [1,%d]", n_importance, MAX_PDF_SAMPLES);
    if (n_rays == 0) return NTX_OK;
    if (!t || !weights || !z_out) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    SamplePdfArgs a{};
    a.t = t; a.z_vals = z_vals; a.weights = weights; a.u = u; a.z_out = z_out;
    a.n_rays = n_rays; a.n_samples = n_samples; a.n_imp = n_importance;
    a.delta = 1.0f / (float)(n_samples - 1);
    a.delta_u = n_importance > 1 ? 1.0f / (float)(n_importance - 1) : 0.0f;
    a.flags = flags; a.seed_lo = (uint32_t)perturb_seed; a.seed_hi = (uint32_t)(perturb_seed >> 32);
    a.idx0 = im.idx0; a.idx_run = im.run; a.idx_stride = im.stride;
    int64_t nb = (n_rays + 3) / 4;
    if (nb > 256 * 8) nb = 256 * 8;
    sample_pdf_kernel<<<dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_image_epilogue(const float *rgba, int height, int width, int downsampling_factor, int unpremultiply,
                       float *out_f32, uint8_t *out_u8, ntx_stream stream) {
    if (!rgba || (!out_f32 && !out_u8)) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (height <= 0 || width <= 0) return ntx_set_error(NTX_E_INVALID, "bad image size %dx%d", height, width);
    const int f = downsampling_factor;
    if (f < 1 || f * 3 > MAX_EPILOGUE_TAPS) return ntx_set_error(NTX_E_INVALID, "downsampling_factor %d outside [1,%d]", f, MAX_EPILOGUE_TAPS / 3);
    EpilogueArgs a{};
    a.rgba = rgba; a.out_f32 = out_f32; a.out_u8 = out_u8;
    a.h = height; a.w = width; a.factor = f; a.unpremultiply = unpremultiply;
    a.oh = (height + f - 1) / f; a.ow = (width + f - 1) / f;
    if (f > 1) {
        const float stdv = (float)(f * .5);                     // filtered_downsample(std=.5): factor * std
        const int K = (int)(f * .5 * 6);                        // interpolate.py:81
        a.taps = K;
        float sum = 0.0f;
        for (int i = 0; i < K; ++i) {                           // interpolate.py:71-72 (+0.5 shift for even sizes)
            const float x = (float)(-(K - 1) / 2.0 + i) + (K % 2 == 0 ? 0.5f : 0.0f);
            const float q = x / stdv;
            a.k1[i] = expf(-.5f * (q * q));
            sum += a.k1[i];
        }
        for (int i = 0; i < K; ++i) a.k1[i] /= sum;             // (k1 (x) k1) / sum(k1 (x) k1) = (k1/S) (x) (k1/S)
        const int ph = (a.oh - 1) * f + K - height, pw = (a.ow - 1) * f + K - width;   // TF 'SAME'
        a.pad_top = (ph > 0 ? ph : 0) / 2; a.pad_left = (pw > 0 ? pw : 0) / 2;
    }
    const int n = a.oh * a.ow;
    epilogue_kernel<<<dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return NTX_OK;
}

}  // extern "C"
