// ntx_trainer.hip -- one training step of the reference on the GPU: network/train.py:49-70 (GradientTape over Renderer.__call__, a loss of
// network/loss.py:6-59, Adam under ExponentialDecay).  This file is what every architecture shares: the handle behind ntx_trainer_* and its
// create, the step's skeleton (depths, noise, the backend's forward, composite + loss, the backend's backward), and the kernels around the
// network: composite_loss_kernel (renderer.py:170-213 per ray, the ray's term of the loss and the adjoint of both), reduce_batch_kernel (the
// weight gradients' partial sums added in a fixed order: a step is bit-reproducible), adam_kernel (train.py:49-52).  The same step cut in
// two at the predictions, for a loss the caller evaluates (ntx_train_forward / ntx_train_backward): composite_forward_kernel and
// composite_adjoint_kernel.  And the same pair for the instanced render (ntx_train_forward_instanced: InstanceRenderer's tail,
// renderer.py:247-354): the compaction of the in-patch samples (live_*_kernel), inst_composite_forward_kernel and
// inst_composite_adjoint_kernel, the network on the compact rows.  All five composite kernels are made of the device pieces of
// ntx_composite.h -- ray_transmittance, ray_forward, ray_adjoint, each formula once -- over a view of the ray (WholeRay / InstancedRay).
// The network between the encoded rays and the composite is a backend's (ntx_trainer.h): the 8 x 256 chain of ntx_backend_chain.hip behind
// ntx_trainer_create, the layer-by-layer step of ntx_backend_flex.hip behind ntx_trainer_create_flex / _flex_ex.  Inference fuses the whole network into
// one kernel because nothing of it has to survive (ntx_device.h); a training step has to keep every layer's activations for the weight
// gradients, and with 288 GB of HBM they are simply stored, once each.  Everything is float32 with float32 accumulation, like the
// reference's TensorFlow graph.  gfx950 only.
#include <cmath>
#include "ntx_composite.h"
namespace ntx_train {
__global__ void reduce_batch_kernel(ReduceBatch b) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int j = 0;
    while (j + 1 < b.n && g >= b.job[j + 1].first) ++j;
    const ReduceJob &r = b.job[j];
    const long long e = g - r.first;
    if (e >= r.count) return;
    // four running sums over z = 0, 4, 8 ... / 1, 5, ... / ..., combined at the end: a fixed order, four loads in flight
    float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    auto at = [&](int z) { const float *p = r.partial + (size_t)z * r.stride + e; return r.pair > 0 ? p[0] + p[r.pair] : p[0]; };
    int z = 0;
    for (; z + 4 <= r.n_split; z += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s4[q] += at(z + q);
    }
    for (int q = 0; z < r.n_split; ++z, ++q) s4[q] += at(z);
    r.out[e] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
}
void launch_reduce(hipStream_t st, const ReduceBatch &b) {
    const long long total = b.job[b.n - 1].first + (b.job[b.n - 1].count + 255) / 256 * 256;
    hipLaunchKernelGGL(reduce_batch_kernel, dim3((unsigned)(total / 256)), dim3(256), 0, st, b);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The five composite kernels: 256 threads, a wave per ray, the wave's el and T in two LDS rows.  Each formula is ntx_composite.h's, stated
// there once for a whole ray (WholeRay: map_model_output, renderer.py:170-213) and a ray of an instanced step (InstancedRay:
// renderer.py:318-354); a kernel keeps what is its own.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void loss_term(int fn, float t, float p, float inv_n, float &value, float &grad) {
    if (fn == NTX_LOSS_MSE) { const float e = t - p; value = e * e * inv_n; grad = -2.0f * e * inv_n; }          // loss.py:51-54
    else {                                                                                                        // smape, eps 1e-2 (:56-59)
        const float e = t - p, den = (t + p) + 1e-2f, ae = fabsf(e);
        const float sgn = e > 0.0f ? 1.0f : (e < 0.0f ? -1.0f : 0.0f);
        value = ae / den * inv_n; grad = (-sgn / den - ae / (den * den)) * inv_n;
    }
}
// the tail of the last block of 32 samples: no gradient (the threads of one workgroup)
__device__ __forceinline__ void zero_dhead_tail(const CompositeArgs &a) {
    const long long end = (a.M + 31) / 32 * 32;
    for (long long m = a.M + threadIdx.x; m < end; m += 256)
        for (int r = 0; r < 4; ++r) a.dhead[dhead_at(m, r)] = 0.0f;
}
// the fused step's composite: the forward, the ray's terms of the loss and their derivatives (loss.py:6-49: both losses are means over the
// rays, so a ray's gradient needs nothing of the others), the adjoint
__global__ __launch_bounds__(256) void composite_loss_kernel(CompositeArgs a) {
    __shared__ float sh_a[4][MAX_TRAIN_SAMPLES], sh_T[4][MAX_TRAIN_SAMPLES];
    fetch_args(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0) zero_dhead_tail(a);
    const int ray = blockIdx.x * 4 + wave;
    if (ray >= a.n_rays) return;
    float *el = sh_a[wave], *T = sh_T[wave];
    const WholeRay v(a, ray);
    float cp[3], A;
    ray_forward(v, a, lane, el, T, cp, A);
    float dC[3], dA = 0.0f, total = 0.0f;
    {
        const float inv_c = 1.0f / (float)(a.n_rays * 3), inv_a = 1.0f / (float)a.n_rays;
        float mask = 1.0f;
        if (a.kind == NTX_LOSS_ALPHA && a.filter_color_loss) mask = a.use_hard_mask ? (a.alpha_true[ray] > 0.0f ? 1.0f : 0.0f) : a.alpha_true[ray];   // :29-35
        for (int c = 0; c < 3; ++c) {
            float val, gr;
            loss_term(a.loss_fn, a.color_true[3 * ray + c] * mask, cp[c] * mask, inv_c, val, gr);
            total += val; dC[c] = gr * mask;
        }
        if (a.kind == NTX_LOSS_ALPHA) { float val; loss_term(a.alpha_loss_fn, a.alpha_true[ray], A, inv_a, val, dA); total += a.gamma * val; dA *= a.gamma; }   // :38
    }
    store_prediction(a, ray, lane, cp, A);
    if (lane == 0) a.ray_loss[ray] = total;
    ray_adjoint(v, a, lane, el, T, dC, dA, nullptr);
}
// ntx_train_forward's composite: the forward alone -- the predictions (and the weights a coarse pass hands on); nothing of the loss, no gradient
__global__ __launch_bounds__(256) void composite_forward_kernel(CompositeArgs a) {
    __shared__ float sh_a[4][MAX_TRAIN_SAMPLES], sh_T[4][MAX_TRAIN_SAMPLES];
    fetch_args(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ray = blockIdx.x * 4 + wave;
    if (ray >= a.n_rays) return;
    float c[3], A;
    ray_forward(WholeRay(a, ray), a, lane, sh_a[wave], sh_T[wave], c, A);
    store_prediction(a, ray, lane, c, A);
}
// ntx_train_backward's composite: el and T again from what the pending forward left (sigma, dists, noise, raw_rgb), then the adjoint from the
// caller's cotangents d_color [N][3] and d_alpha [N] (NULL: 0).  A ray whose depths are not finite has dists 0 throughout: it composites to
// nothing, and its gradient is 0 whatever its cotangent holds (inf and NaN included) -- by selecting a zero cotangent for it, so that the
// adjoint runs on the same numbers as with the cotangent zeroed by the caller, never by a product with what may not be finite.  d_weights:
// NULL, or [N][S] = dL/d weights (ntx_trainer_weight_cotangent); such a ray selects none of it either.
__global__ __launch_bounds__(256) void composite_adjoint_kernel(CompositeArgs a, const float *__restrict__ d_color, const float *__restrict__ d_alpha,
                                                                const float *__restrict__ d_weights) {
    __shared__ float sh_a[4][MAX_TRAIN_SAMPLES], sh_T[4][MAX_TRAIN_SAMPLES];
    fetch_args(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0) zero_dhead_tail(a);
    const int ray = blockIdx.x * 4 + wave;
    if (ray >= a.n_rays) return;
    float *el = sh_a[wave], *T = sh_T[wave];
    const WholeRay v(a, ray);
    (void)ray_transmittance(v, lane, el, T);
    bool live = false;
    for (int s = lane; s < a.S; s += 64) live = live || v.ds[s] != 0.0f;
    live = __any(live) != 0;
    float dC[3];
    for (int c = 0; c < 3; ++c) dC[c] = live ? d_color[3 * ray + c] : 0.0f;
    const float dA = live && d_alpha ? d_alpha[ray] : 0.0f;
    ray_adjoint(v, a, lane, el, T, dC, dA, live ? d_weights : nullptr);
}
// ntx_train_forward_instanced's composite, the network's raw outputs in compact rows.  A ray with hit == 0 is 0 / 0 and its weights are 0.
__global__ __launch_bounds__(256) void inst_composite_forward_kernel(InstCompositeArgs a) {
    __shared__ float sh_a[4][MAX_TRAIN_SAMPLES], sh_T[4][MAX_TRAIN_SAMPLES];
    fetch_args(a);
    const StepSamples &p = a.s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * 4 + wave;
    if (ray >= p.n_rays) return;
    float c[3] = {0.0f, 0.0f, 0.0f}, A = 0.0f;
    if (!p.hit[ray]) { if (a.weights) for (int s = lane; s < p.S; s += 64) a.weights[ray * p.S + s] = 0.0f; }
    else ray_forward(InstancedRay(a, ray), a, lane, sh_a[wave], sh_T[wave], c, A);
    store_prediction(a, ray, lane, c, A);
}
// Its adjoint from the caller's cotangents, to dgrad[row] of the live samples.  A ray with hit == 0 has no live sample: nothing of it is
// written whatever its cotangent holds, which is not even read.  d_weights: NULL, or [N][S] = dL/d weights of the S samples.
__global__ __launch_bounds__(256) void inst_composite_adjoint_kernel(InstCompositeArgs a, const float *__restrict__ d_color, const float *__restrict__ d_alpha,
                                                                     const float *__restrict__ d_weights) {
    __shared__ float sh_a[4][MAX_TRAIN_SAMPLES], sh_T[4][MAX_TRAIN_SAMPLES];
    fetch_args(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * 4 + wave;
    if (ray >= a.s.n_rays || !a.s.hit[ray]) return;
    float *el = sh_a[wave], *T = sh_T[wave];
    const InstancedRay v(a, ray);
    (void)ray_transmittance(v, lane, el, T);
    const float dC[3] = {d_color[3 * ray], d_color[3 * ray + 1], d_color[3 * ray + 2]};
    ray_adjoint(v, a, lane, el, T, dC, d_alpha ? d_alpha[ray] : 0.0f, d_weights);
}
// ---------------------------------------------------------------------------------------------------------------------------
// The instanced step (ntx_train_forward_instanced): InstanceRenderer.evaluate_model + map_model_output (renderer.py:247-354) with the
// network on the live samples alone.  Sample m = ray * S + s is live iff hit[ray] != 0 && dists[m] > 0 (:284-288).
// The compaction numbers the live samples in ascending m by a prefix sum in two levels and no atomic: live_count_kernel counts a ray's
// live samples (wave per ray), live_scan_kernel turns the counts into each ray's first row (one workgroup, every thread a contiguous range
// of rays, the threads' sums scanned in LDS) and leaves the total, live_rows_kernel numbers a ray's samples behind its first row (wave per
// ray, a ballot per 64 samples): live[row] = m, row_of[m] = row or -1.  The order is a function of hit and dists alone.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void live_count_kernel(const float *__restrict__ dists, const uint8_t *__restrict__ hit, long long n_rays, int S, int *__restrict__ ray_live) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    int n = 0;
    if (hit[ray]) for (int s = lane; s < S; s += 64) n += dists[(size_t)ray * S + s] > 0.0f ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) ray_live[ray] = n;
}
// ray_live[r] (counts) -> the exclusive sum over the rays in front of r, in place; *n_live = the total
__global__ __launch_bounds__(1024) void live_scan_kernel(int *__restrict__ ray_live, long long n_rays, long long *__restrict__ n_live) {
    __shared__ int sums[1024];
    const long long per = (n_rays + 1023) / 1024, r0 = (long long)threadIdx.x * per, r1 = r0 + per < n_rays ? r0 + per : n_rays;
    int mine = 0;
    for (long long r = r0; r < r1; ++r) mine += ray_live[r];
    sums[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                                       // inclusive scan of the threads' sums
        const int v = (int)threadIdx.x >= o ? sums[threadIdx.x - o] : 0;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    int base = sums[threadIdx.x] - mine;
    for (long long r = r0; r < r1; ++r) { const int c = ray_live[r]; ray_live[r] = base; base += c; }
    if (threadIdx.x == 1023) *n_live = sums[1023];
}
__global__ __launch_bounds__(256) void live_rows_kernel(const float *__restrict__ dists, const uint8_t *__restrict__ hit, long long n_rays, int S,
                                                        const int *__restrict__ ray_first, int *__restrict__ live, int *__restrict__ row_of) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const bool h = hit[ray] != 0;
    int base = ray_first[ray];
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const long long m = ray * S + s;
        const bool lv = h && s < S && dists[m] > 0.0f;
        const unsigned long long b = __ballot(lv);
        const int row = base + __popcll(b & ((1ull << lane) - 1ull));
        if (s < S) row_of[m] = lv ? row : -1;
        if (lv) live[row] = (int)m;
        base += __popcll(b);
    }
}
// the loss: the rays' terms added up by one workgroup in a fixed order
__global__ __launch_bounds__(1024) void loss_sum_kernel(const float *__restrict__ ray_loss, int n_rays, float *__restrict__ loss) {
    __shared__ float red[1024];
    float total = 0.0f;
    for (int r = threadIdx.x; r < n_rays; r += blockDim.x) total += ray_loss[r];
    red[threadIdx.x] = total;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) *loss = red[0];
}

// tf.keras.optimizers.Adam (TF 2.4, non-amsgrad): m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
// w -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps), t = iterations + 1; lr from ExponentialDecay (train.py:49-52) on the host
__global__ void adam_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, long long n, float lr_t, float b1,
                            float b2, float eps) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float ge = g[e];
    const float me = m[e] + (ge - m[e]) * (1.0f - b1);
    const float ve = v[e] + (ge * ge - v[e]) * (1.0f - b2);
    m[e] = me; v[e] = ve;
    w[e] = w[e] - (me * lr_t) / (sqrtf(ve) + eps);
}
}   // namespace ntx_train

using namespace ntx_train;
// The create entries (kind 0: the chain, 1: layer by layer, 2: layer by layer with parameter branches): the architecture check first (trainer_class_for in train.py asks with max_rays = 0 and counts on NTX_E_UNSUPPORTED
// before NTX_E_INVALID, and on no device being asked for before either), then the sizes, the device, the handle with the buffers and weights
// every backend needs, and the backend.
static int trainer_create(int kind, const ntx_model_desc *desc, const float *weights, size_t n_floats, int device, int64_t max_rays, int max_samples_per_ray, ntx_trainer **out) {
    if (!out) return ntx_set_error(NTX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!desc || !weights) return ntx_set_error(NTX_E_INVALID, "desc / weights is NULL");
    const bool flex = kind != 0;
    TrainDims dm{};
    int rc = flex ? flex_check(desc, &dm, kind == 2) : chain_check(desc, &dm);
    if (rc != NTX_OK) return rc;
    if (max_rays < 1 || max_samples_per_ray < 2 || max_samples_per_ray > MAX_TRAIN_SAMPLES || max_rays * (int64_t)max_samples_per_ray > (int64_t)1 << 30)
        return ntx_set_error(NTX_E_INVALID, "max_rays / max_samples_per_ray out of range (samples per ray <= %d)", MAX_TRAIN_SAMPLES);
    const size_t p = dm.n_weights;
    auto count_ok = [&]() { return n_floats == p ? NTX_OK : ntx_set_error(NTX_E_INVALID, "weights: %zu floats, the model has %zu", n_floats, p); };
    if (flex && (rc = count_ok()) != NTX_OK) return rc;          // the layer-by-layer entry says so before it asks for a device, the chain's after
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ntx_set_error(NTX_E_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return ntx_set_error(NTX_E_INVALID, "device %d out of range [0,%d)", device, ndev);
    if (!flex && (rc = count_ok()) != NTX_OK) return rc;
    ntx_trainer *t = new ntx_trainer();
    t->device = device; t->desc = dm.desc; t->ipe = dm.ipe; t->P = dm.desc.n_geo + dm.desc.n_app; t->Kp = dm.Kp; t->Kd = dm.Kd; t->n_weights = p;
    t->param_depth = dm.param_depth; t->param_width = dm.param_width; t->flex = flex;
    const long long M = (long long)max_rays * max_samples_per_ray, NB = (M + 31) / 32;
    t->cap = M; t->cap_rays = max_rays; t->cap_blocks = NB;
    DeviceMemory &mem = t->mem;
    if (hipSetDevice(device) != hipSuccess) mem.rc = ntx_set_error(NTX_E_HIP, "hipSetDevice(%d) failed", device);
    else { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) t->cus = n; }
    mem.alloc(&t->w, p); mem.alloc(&t->grad, p, true); mem.alloc(&t->adam_m, p, true); mem.alloc(&t->adam_v, p, true);
    mem.alloc(&t->sigma, (size_t)M); mem.alloc(&t->raw_rgb, (size_t)M * 3); mem.alloc(&t->dists, (size_t)M); mem.alloc(&t->noise, (size_t)M);
    mem.alloc(&t->z, (size_t)(M + max_rays));                                                   // (a mip step's S + 1 segment edges a ray)
    mem.alloc(&t->dgrad, (size_t)NB * 32 * 4); mem.alloc(&t->dhead, (size_t)NB * 1024, true);   // rows 4 .. 31 of the heads' dY tile stay zero
    mem.alloc(&t->color, (size_t)max_rays * 3); mem.alloc(&t->alpha_out, (size_t)max_rays); mem.alloc(&t->ray_loss, (size_t)max_rays); mem.alloc(&t->loss, 1);
    if (mem.rc == NTX_OK && hipMemcpy(t->w, weights, p * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) mem.rc = ntx_set_error(NTX_E_HIP, "weight upload failed");
    rc = flex ? flex_backend_create(t) : chain_backend_create(t);
    if (rc != NTX_OK) { delete t; return rc; }                                                  // (frees what was made)
    *out = t;
    return NTX_OK;
}

extern "C" {
int ntx_trainer_create(const ntx_model_desc *desc, const float *weights, size_t n_floats, int device, int64_t max_rays, int max_samples_per_ray, ntx_trainer **out) {
    return trainer_create(0, desc, weights, n_floats, device, max_rays, max_samples_per_ray, out);
}

int ntx_trainer_create_flex(const ntx_model_desc *desc, const float *weights, size_t n_floats, int device, int64_t max_rays, int max_samples_per_ray, ntx_trainer **out) {
    return trainer_create(1, desc, weights, n_floats, device, max_rays, max_samples_per_ray, out);
}
int ntx_trainer_create_flex_ex(const ntx_model_desc_ex *desc, const float *weights, size_t n_floats, int device, int64_t max_rays, int max_samples_per_ray, ntx_trainer **out) {
    return trainer_create(2, desc ? &desc->base : nullptr, weights, n_floats, device, max_rays, max_samples_per_ray, out);
}
int ntx_trainer_destroy(ntx_trainer *t) { delete t; return NTX_OK; }
size_t ntx_trainer_weight_count(const ntx_trainer *t) { return t ? t->n_weights : 0; }

// one of the handle's four vectors to the host or from it
static int trainer_copy(ntx_trainer *t, int what, float *to_host, const float *from_host, size_t n_floats) {
    if (!t || (!to_host && !from_host)) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    if (n_floats != t->n_weights) return ntx_set_error(NTX_E_INVALID, "%zu floats %s, the model has %zu", n_floats, to_host ? "asked" : "given", t->n_weights);
    float *v = what == NTX_TRAINER_WEIGHTS ? t->w : what == NTX_TRAINER_GRADIENTS ? t->grad : what == NTX_TRAINER_ADAM_M ? t->adam_m : what == NTX_TRAINER_ADAM_V ? t->adam_v : nullptr;
    if (!v) return ntx_set_error(NTX_E_INVALID, "what = %d", what);
    TRAIN_TRY(hipSetDevice(t->device));
    TRAIN_TRY(hipDeviceSynchronize());
    TRAIN_TRY(to_host ? hipMemcpy(to_host, v, n_floats * sizeof(float), hipMemcpyDeviceToHost) : hipMemcpy(v, from_host, n_floats * sizeof(float), hipMemcpyHostToDevice));
    return NTX_OK;
}
int ntx_trainer_get(ntx_trainer *t, int what, float *out_host, size_t n_floats) { return trainer_copy(t, what, out_host, nullptr, n_floats); }
int ntx_trainer_set(ntx_trainer *t, int what, const float *values_host, size_t n_floats) { return trainer_copy(t, what, nullptr, values_host, n_floats); }
int ntx_trainer_set_weights(ntx_trainer *t, const float *weights_host, size_t n_floats) { return ntx_trainer_set(t, NTX_TRAINER_WEIGHTS, weights_host, n_floats); }

int ntx_trainer_activation(ntx_trainer *t, int layer, int64_t n_samples_total, float *out_host) {
    if (!t || !out_host) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    if (n_samples_total < 1 || n_samples_total > t->cap) return ntx_set_error(NTX_E_INVALID, "n_samples_total out of range");
    return t->backend->activation(layer, n_samples_total, out_host);
}

int ntx_trainer_set_iterations(ntx_trainer *t, int64_t iterations) {
    if (!t || iterations < 0) return ntx_set_error(NTX_E_INVALID, "trainer is NULL or iterations < 0");
    t->adam_iterations = iterations;
    return NTX_OK;
}

// The arithmetic of the layer-by-layer backend's contractions from the next step on; everything else of a step is float32 either way
int ntx_trainer_set_precision(ntx_trainer *t, int precision) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    if (precision == NTX_PRECISION_FP16X3)
        return ntx_set_error(NTX_E_UNSUPPORTED, "training in fp16x3: the cotangents of a mean loss lie below the range of an IEEE half; NTX_PRECISION_BF16X6 keeps float32's exponents");
    if (precision != NTX_PRECISION_F32 && precision != NTX_PRECISION_BF16X6) return ntx_set_error(NTX_E_INVALID, "precision %d (NTX_PRECISION_F32 or NTX_PRECISION_BF16X6)", precision);
    if (!t->flex || t->ipe)
        return ntx_set_error(NTX_E_UNSUPPORTED, "a precision: the fused chain (ntx_trainer_create) runs on its own float32 kernels; the layer-by-layer trainer takes the same "
                             "model in NTX_PRECISION_BF16X6 (ntx_trainer_create_flex, ntx_trainer_create_flex_ex)");
    if (t->pending.open) return ntx_set_error(NTX_E_INVALID, "a forward is pending: its ntx_train_backward runs in the precision of the forward; set the precision between steps");
    t->precision = precision;
    return NTX_OK;
}
int ntx_trainer_precision(const ntx_trainer *t) { return t ? t->precision : -1; }

int ntx_trainer_composite_weights(ntx_trainer *t, float *weights_dev) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    if (t->ipe && weights_dev) return ntx_set_error(NTX_E_UNSUPPORTED, "an IPE trainer has no importance pass (MipRenderer: renderer.py:403-404)");
    t->weights_out = weights_dev;
    return NTX_OK;
}
int ntx_trainer_weight_cotangent(ntx_trainer *t, const float *d_weights_dev) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    if (t->ipe) return ntx_set_error(NTX_E_UNSUPPORTED, "an IPE trainer hands out no composite weights (ntx_trainer_composite_weights), so it takes no cotangent of them");
    if (!t->pending.open) return ntx_set_error(NTX_E_INVALID, "no forward is pending: the weight cotangent belongs to the next ntx_train_backward of a pending ntx_train_forward / "
                                               "ntx_train_forward_instanced");
    t->pending.d_weights = d_weights_dev;                                                       // (NULL: none)
    return NTX_OK;
}
namespace ntx_train {
__global__ void add_kernel(float *__restrict__ dst, const float *__restrict__ src, long long n) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) dst[e] += src[e];
}
}   // namespace ntx_train

// mode 2 of ntx_trainer_enable_param_gradients takes no weight gradient: what would use one says so (as does mode 2 of
// ntx_trainer_enable_input_gradients)
static int no_weight_gradients(const ntx_trainer *t, const char *who) {
    if (t->ig_mode == 2)
        return ntx_set_error(NTX_E_INVALID, "%s: the trainer takes input gradients only (ntx_trainer_enable_input_gradients mode 2), its weight gradient is not this "
                             "step's; set mode 0 or 1 first", who);
    return t->pg_mode == 2 ? ntx_set_error(NTX_E_INVALID, "%s: the trainer takes parameter gradients only (ntx_trainer_enable_param_gradients mode 2), its weight gradient is "
                                           "not this step's; set mode 0 or 1 first", who) : NTX_OK;
}

int ntx_trainer_stash_gradients(ntx_trainer *t, int op, ntx_stream stream) {
    if (!t || (op != 0 && op != 1)) return ntx_set_error(NTX_E_INVALID, "trainer is NULL or op is not 0 (keep) / 1 (add back)");
    if (int rc = no_weight_gradients(t, "ntx_trainer_stash_gradients")) return rc;
    TRAIN_TRY(hipSetDevice(t->device));
    if (!t->stash) {
        if (op == 1) return ntx_set_error(NTX_E_INVALID, "no gradient was kept");
        if (t->mem.alloc(&t->stash, t->n_weights) != NTX_OK) return t->mem.rc;
    }
    if (op == 0) TRAIN_TRY(hipMemcpyAsync(t->stash, t->grad, t->n_weights * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else hipLaunchKernelGGL(ntx_train::add_kernel, dim3((unsigned)((t->n_weights + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t->grad, t->stash, (long long)t->n_weights);
    TRAIN_TRY(hipGetLastError());
    return NTX_OK;
}

int ntx_trainer_device_weights(ntx_trainer *t, const float **weights_dev) {
    if (!t || !weights_dev) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    *weights_dev = t->w;
    return NTX_OK;
}

int ntx_trainer_allreduce_gradients(ntx_trainer *t, ntx_comm *comm, ntx_stream stream) {
    if (!t || !comm) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    if (int rc = no_weight_gradients(t, "ntx_trainer_allreduce_gradients")) return rc;
    return ntx_allreduce_mean_f32(comm, t->grad, t->n_weights, stream);
}

// What the entries of a step share.  step_check: the rays and sizes of a step against the handle.  step_network: depths, noise and the
// backend's forward (every activation kept); leaves the step's rays and the noise its composite takes (NULL without NTX_FLAG_RAW_NOISE).
// composite_args: the composite's arguments less the loss and the cotangents.
static int step_check(const ntx_trainer *t, const float *rays_o, const float *rays_d, const float *tnear_far, const float *params, const float *cone_scale, int64_t n_rays,
                      int n_samples, int blur_idx, const float *z_vals) {
    const int P_in = t->P + (t->ipe ? 1 : 0);                                               // the MipRenderer's rows still hold the blur parameter
    if (!rays_o || !rays_d || (!tnear_far && !z_vals) || (P_in > 0 && !params)) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (n_rays < 1 || n_rays > t->cap_rays || n_samples < 2 || (long long)n_rays * n_samples > t->cap) return ntx_set_error(NTX_E_INVALID, "n_rays x n_samples beyond what the trainer was created for");
    if (n_samples > MAX_TRAIN_SAMPLES) return ntx_set_error(NTX_E_INVALID, "n_samples > %d", MAX_TRAIN_SAMPLES);
    if (blur_idx >= P_in || (blur_idx >= 0 && !cone_scale) || (t->ipe && blur_idx < 0)) return ntx_set_error(NTX_E_INVALID, "bad blur_idx / cone_scale");
    return NTX_OK;
}
static int step_network(ntx_trainer *t, const float *rays_o, const float *rays_d, const float *tnear_far, const float *params, int64_t rays_per_param_row,
                        const float *cone_scale, int64_t n_rays, int n_samples, int blur_idx, uint32_t flags, uint64_t perturb_seed, const ntx_render_opts *opts,
                        const float *z_vals, ntx_stream stream, StepRays *rays, const float **noise) {
    if (rays_per_param_row < 1) rays_per_param_row = 1;
    TRAIN_TRY(hipSetDevice(t->device));
    const int S = n_samples;
    const float *z = z_vals;                                                                    // [N][S], or the S + 1 segment edges of a mip step
    if (!z) {
        int rc = ntx_sample_depths(tnear_far, n_rays, t->ipe ? S + 1 : S, flags & NTX_FLAG_PERTURB, perturb_seed, opts, t->z, stream);     // renderer.py:101-111, 374-383
        if (rc != NTX_OK) return rc;
        z = t->z;
    }
    *noise = nullptr;
    if (flags & NTX_FLAG_RAW_NOISE) {                                                           // renderer.py:190-192
        int rc = ntx_sample_noise(n_rays, S, perturb_seed, opts, t->noise, stream);
        if (rc != NTX_OK) return rc;
        *noise = t->noise;
    }
    t->step_noise = *noise;
    const ntx_model_desc &d = t->desc;
    *rays = StepRays{rays_o, rays_d, z, params, cone_scale, rays_per_param_row, n_rays, S, blur_idx, d.n_geo, d.n_app, d.pos_freq, d.dir_freq, d.param_freq};
    return t->backend->forward(*rays, (hipStream_t)stream);
}
// what both composites' arguments share: the raw outputs, the flags' options, the background (default 1), the predictions (default: the
// handle's buffers), the registered weights (ntx_trainer_composite_weights: a forward's; the backwards set NULL) and dgrad
static void composite_common(const ntx_trainer *t, uint32_t flags, const float *bkgd, float *color_pred, float *alpha_pred, CompositeCommon *c) {
    c->raw_rgb = t->raw_rgb; c->sigma = t->sigma; c->map_exr = (flags & NTX_FLAG_MAP_EXR) ? 1 : 0; c->composite_bkgd = (flags & NTX_FLAG_COMPOSITE_BKGD) ? 1 : 0;
    for (int k = 0; k < 3; ++k) c->bkgd[k] = bkgd ? bkgd[k] : 1.0f;
    c->color = color_pred ? color_pred : t->color; c->alpha = alpha_pred ? alpha_pred : t->alpha_out; c->weights = t->weights_out; c->dgrad = t->dgrad;
}
// what a step left for the gradient getters, under the modes that are on: a plain step's parameter rows and rays (smp_rays = 0), or an
// instanced step's rays x S of per-sample gradients (rows = rays = 0) -- each kind of getter refuses the other kind's step
static void step_left(ntx_trainer *t, long long rows, long long rays, long long smp_rays, int smp_S) {
    if (t->pg_mode != 0) { t->pg_rows = rows; t->spg_rays = smp_rays; t->spg_S = smp_S; }
    if (t->ig_mode != 0) { t->ig_rays = rays; t->ig_smp_rays = smp_rays; t->ig_S = smp_S; }
}
static void plain_step_left(ntx_trainer *t, const StepRays &rays) { step_left(t, (rays.n_rays + rays.rays_per_param_row - 1) / rays.rays_per_param_row, rays.n_rays, 0, 0); }
static CompositeArgs composite_args(const ntx_trainer *t, const StepRays &rays, const float *noise, uint32_t flags, const float *bkgd, float *color_pred, float *alpha_pred) {
    CompositeArgs c{};
    composite_common(t, flags, bkgd, color_pred, alpha_pred, &c);
    c.dists = t->dists; c.noise = noise; c.n_rays = (int)rays.n_rays; c.S = rays.S; c.ray_loss = t->ray_loss; c.dhead = t->dhead; c.M = rays.M();
    return c;
}

// ... of an instanced step, and its second half: the adjoint over the pending samples, the backend's way back over the compact rows and --
// under ntx_trainer_enable_param_gradients -- the per-sample dL/d params (placed at the first such step, for the capacity)
static InstCompositeArgs inst_composite_args(const ntx_trainer *t, const StepSamples &s, uint32_t flags, const float *bkgd, float *color_pred, float *alpha_pred) {
    InstCompositeArgs c{};
    composite_common(t, flags, bkgd, color_pred, alpha_pred, &c);
    c.s = s;
    return c;
}
static int backward_instanced(ntx_trainer *t, const float *d_color, const float *d_alpha, const float *d_weights, hipStream_t st) {
    const StepSamples &s = t->pending.smp;
    if (t->pg_mode != 0 && !t->sample_pg && t->mem.alloc(&t->sample_pg, (size_t)t->cap * t->P) != NTX_OK) return t->mem.rc;
    if (t->ig_mode != 0 && !t->d_pts) {
        t->mem.alloc(&t->d_pts, (size_t)t->cap * 3); t->mem.alloc(&t->d_dirs, (size_t)t->cap * 3);
        if (t->mem.rc != NTX_OK) return t->mem.rc;
    }
    InstCompositeArgs c = inst_composite_args(t, s, t->pending.flags, t->pending.bkgd, nullptr, nullptr);
    c.weights = nullptr;                                                                        // the adjoint alone: nothing of the forward is written again
    if (s.n_live > 0) hipLaunchKernelGGL(inst_composite_adjoint_kernel, dim3((unsigned)((s.n_rays + 3) / 4)), dim3(256), 0, st, c, d_color, d_alpha, d_weights);
    int rc = t->backend->backward_samples(s, t->sample_pg, st);
    if (rc != NTX_OK) return rc;
    TRAIN_TRY(hipGetLastError());
    step_left(t, 0, 0, s.n_rays, s.S);
    return NTX_OK;
}

int ntx_train_step_gradients(ntx_trainer *t, const float *rays_o, const float *rays_d, const float *tnear_far, const float *params, int64_t rays_per_param_row,
                             const float *cone_scale, int64_t n_rays, int n_samples, int blur_idx, uint32_t flags, const float *bkgd, uint64_t perturb_seed,
                             const ntx_render_opts *opts, const float *z_vals, const float *color_true, const float *alpha_true, const ntx_loss_desc *loss,
                             float *color_pred, float *alpha_pred, float *loss_out, ntx_stream stream) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    t->pending.open = false; t->pending.d_weights = nullptr;                                    // a forward left open is not this step's, nor is its weight cotangent
    if (!color_true || !loss) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (int rc = step_check(t, rays_o, rays_d, tnear_far, params, cone_scale, n_rays, n_samples, blur_idx, z_vals)) return rc;
    if (loss->size < sizeof(ntx_loss_desc) || (loss->kind != NTX_LOSS_NERF && loss->kind != NTX_LOSS_ALPHA) || (loss->loss_fn != NTX_LOSS_MSE && loss->loss_fn != NTX_LOSS_SMAPE) ||
        (loss->alpha_loss_fn != NTX_LOSS_MSE && loss->alpha_loss_fn != NTX_LOSS_SMAPE))
        return ntx_set_error(NTX_E_INVALID, "bad ntx_loss_desc");
    if (loss->kind == NTX_LOSS_ALPHA && !alpha_true) return ntx_set_error(NTX_E_INVALID, "AlphaLoss needs alpha_true");
    hipStream_t st = (hipStream_t)stream;
    StepRays rays{};
    const float *noise = nullptr;
    int rc = step_network(t, rays_o, rays_d, tnear_far, params, rays_per_param_row, cone_scale, n_rays, n_samples, blur_idx, flags, perturb_seed, opts, z_vals, stream, &rays, &noise);
    if (rc != NTX_OK) return rc;
    // ---- the composite, the loss (loss.py) and their adjoint ------------------------------------------------------------------------
    CompositeArgs c = composite_args(t, rays, noise, flags, bkgd, color_pred, alpha_pred);
    c.color_true = color_true; c.alpha_true = alpha_true; c.kind = loss->kind; c.loss_fn = loss->loss_fn; c.alpha_loss_fn = loss->alpha_loss_fn;
    c.filter_color_loss = loss->filter_color_loss; c.use_hard_mask = loss->use_hard_mask; c.gamma = loss->gamma;
    hipLaunchKernelGGL(composite_loss_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, st, c);
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(1024), 0, st, t->ray_loss, (int)n_rays, loss_out ? loss_out : t->loss);
    rc = t->backend->backward(rays, st);
    if (rc != NTX_OK) return rc;
    TRAIN_TRY(hipGetLastError());
    plain_step_left(t, rays);
    return NTX_OK;
}

int ntx_train_forward(ntx_trainer *t, const float *rays_o, const float *rays_d, const float *tnear_far, const float *params, int64_t rays_per_param_row,
                      const float *cone_scale, int64_t n_rays, int n_samples, int blur_idx, uint32_t flags, const float *bkgd, uint64_t perturb_seed,
                      const ntx_render_opts *opts, const float *z_vals, float *color_pred, float *alpha_pred, ntx_stream stream) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    t->pending.open = false; t->pending.d_weights = nullptr;                                    // a new forward replaces the one left open (and drops its weight cotangent)
    if (int rc = step_check(t, rays_o, rays_d, tnear_far, params, cone_scale, n_rays, n_samples, blur_idx, z_vals)) return rc;
    StepRays rays{};
    const float *noise = nullptr;
    int rc = step_network(t, rays_o, rays_d, tnear_far, params, rays_per_param_row, cone_scale, n_rays, n_samples, blur_idx, flags, perturb_seed, opts, z_vals, stream, &rays, &noise);
    if (rc != NTX_OK) return rc;
    const CompositeArgs c = composite_args(t, rays, noise, flags, bkgd, color_pred, alpha_pred);
    hipLaunchKernelGGL(composite_forward_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream, c);
    TRAIN_TRY(hipGetLastError());
    t->pending.rays = rays; t->pending.flags = flags; t->pending.noise = noise; t->pending.samples = false;
    for (int k = 0; k < 3; ++k) t->pending.bkgd[k] = c.bkgd[k];
    t->pending.open = true;
    return NTX_OK;
}

int ntx_train_backward(ntx_trainer *t, const float *d_color, const float *d_alpha, ntx_stream stream) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    if (!t->pending.open) return ntx_set_error(NTX_E_INVALID, "no ntx_train_forward is pending (one ntx_train_backward per forward; ntx_train_step_gradients closes it too)");
    if (!d_color) return ntx_set_error(NTX_E_INVALID, "d_color is NULL");
    t->pending.open = false;
    const float *d_weights = t->pending.d_weights;                                              // ntx_trainer_weight_cotangent's, used once
    t->pending.d_weights = nullptr;
    TRAIN_TRY(hipSetDevice(t->device));
    if (t->pending.samples) return backward_instanced(t, d_color, d_alpha, d_weights, (hipStream_t)stream);
    const StepRays &rays = t->pending.rays;
    CompositeArgs c = composite_args(t, rays, t->pending.noise, t->pending.flags, t->pending.bkgd, nullptr, nullptr);
    c.weights = nullptr;                                                                        // the adjoint alone: nothing of the forward is written again
    t->step_noise = t->pending.noise;
    hipLaunchKernelGGL(composite_adjoint_kernel, dim3((unsigned)((rays.n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream, c, d_color, d_alpha, d_weights);
    int rc = t->backend->backward(rays, (hipStream_t)stream);
    if (rc != NTX_OK) return rc;
    TRAIN_TRY(hipGetLastError());
    plain_step_left(t, rays);
    return NTX_OK;
}

int ntx_train_forward_instanced(ntx_trainer *t, const float *rays_d_map, const float *pts, const float *t_map, const float *dists, const float *color_last,
                                const float *alpha_last, const float *alpha_weight, const uint8_t *hit, const float *params_map, const float *cone_scale, int64_t n_rays,
                                int n_samples, int blur_idx, float patch_scale, float density_scale, uint32_t flags, const float *bkgd, float *color_pred, float *alpha_pred,
                                int64_t *n_live_out, ntx_stream stream) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    t->pending.open = false; t->pending.d_weights = nullptr;                                    // a new forward of either kind replaces the one left open
    if (int rc = t->backend->takes_samples()) return rc;
    if (!rays_d_map || !pts || !dists || !color_last || !alpha_last || !hit || (t->P > 0 && !params_map)) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (n_samples < 1 || n_samples > MAX_TRAIN_SAMPLES) return ntx_set_error(NTX_E_INVALID, "n_samples outside 1 .. %d", MAX_TRAIN_SAMPLES);
    if (n_rays < 1 || n_rays > t->cap_rays || (long long)n_rays * n_samples > t->cap) return ntx_set_error(NTX_E_INVALID, "n_rays x n_samples beyond what the trainer was created for");
    if (!(patch_scale > 0.0f)) return ntx_set_error(NTX_E_INVALID, "patch_scale must be > 0");
    if (blur_idx >= t->P || (blur_idx >= 0 && (!cone_scale || !t_map))) return ntx_set_error(NTX_E_INVALID, "bad blur_idx / cone_scale / t_map");
    if (flags & (NTX_FLAG_PERTURB | NTX_FLAG_RAW_NOISE))
        return ntx_set_error(NTX_E_INVALID, "NTX_FLAG_PERTURB / NTX_FLAG_RAW_NOISE: the instancer places the samples, and the density noise of an instanced step is not built");
    hipStream_t st = (hipStream_t)stream;
    TRAIN_TRY(hipSetDevice(t->device));
    if (int rc = t->place_sample_maps()) return rc;                                             // the first instanced step places its maps, for the capacity
    const unsigned ray_grid = (unsigned)((n_rays + 3) / 4);
    hipLaunchKernelGGL(live_count_kernel, dim3(ray_grid), dim3(256), 0, st, dists, hit, (long long)n_rays, n_samples, t->ray_live);
    hipLaunchKernelGGL(live_scan_kernel, dim3(1), dim3(1024), 0, st, t->ray_live, (long long)n_rays, t->n_live_dev);
    hipLaunchKernelGGL(live_rows_kernel, dim3(ray_grid), dim3(256), 0, st, dists, hit, (long long)n_rays, n_samples, t->ray_live, t->live, t->row_of);
    long long n_live = 0;                                                                       // the launches are sized on the host: the step's one synchronisation
    TRAIN_TRY(hipMemcpyAsync(&n_live, t->n_live_dev, sizeof(n_live), hipMemcpyDeviceToHost, st));
    TRAIN_TRY(hipStreamSynchronize(st));
    if (n_live < 0 || n_live > (long long)n_rays * n_samples) return ntx_set_error(NTX_E_HIP, "the compaction counted %lld live samples of %lld", n_live, (long long)n_rays * n_samples);
    if (n_live_out) *n_live_out = n_live;
    const ntx_model_desc &d = t->desc;
    StepSamples s{rays_d_map, pts, t_map, dists, color_last, alpha_last, alpha_weight, hit, params_map, cone_scale, n_rays, n_samples, blur_idx, d.n_geo, d.n_app, d.pos_freq,
                  d.dir_freq, d.param_freq, patch_scale, density_scale, t->live, t->row_of, n_live};
    int rc = t->backend->forward_samples(s, st);
    if (rc != NTX_OK) return rc;
    const InstCompositeArgs c = inst_composite_args(t, s, flags, bkgd, color_pred, alpha_pred);
    hipLaunchKernelGGL(inst_composite_forward_kernel, dim3(ray_grid), dim3(256), 0, st, c);
    TRAIN_TRY(hipGetLastError());
    t->pending.smp = s; t->pending.flags = flags; t->pending.noise = nullptr; t->pending.samples = true;
    for (int k = 0; k < 3; ++k) t->pending.bkgd[k] = c.bkgd[k];
    t->pending.open = true;
    return NTX_OK;
}

int ntx_trainer_enable_instanced(ntx_trainer *t) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    return t->backend->enable_samples();                                                        // the chain places its maps once; a layer-by-layer handle takes samples as it is
}

int ntx_trainer_sample_param_gradients(ntx_trainer *t, const float **grad_dev, int64_t *n_rays, int *n_samples, int *n_params) {
    if (!t || !grad_dev || !n_rays || !n_samples || !n_params) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    if (t->pg_mode == 0 || t->spg_rays == 0) return ntx_set_error(NTX_E_INVALID, "no per-sample parameter gradients: %s", t->pg_mode == 0 ? "ntx_trainer_enable_param_gradients is off" :
                                                                  "the last step since they were enabled was not an instanced one (ntx_trainer_param_gradients has a plain step's)");
    *grad_dev = t->sample_pg; *n_rays = t->spg_rays; *n_samples = t->spg_S; *n_params = t->P;
    return NTX_OK;
}

int ntx_trainer_enable_param_gradients(ntx_trainer *t, int mode) {
    if (!t || mode < 0 || mode > 2) return ntx_set_error(NTX_E_INVALID, "trainer is NULL or mode is not 0 (off) / 1 (with the weight gradients) / 2 (parameters only)");
    if (mode != 0) {
        int rc = t->backend->enable_param_gradients();                                          // the chain refuses; the layer-by-layer backend places its buffers once
        if (rc != NTX_OK) return rc;
    } else { t->pg_rows = 0; t->spg_rays = 0; }
    t->pg_mode = mode;
    return NTX_OK;
}

int ntx_trainer_param_gradients(ntx_trainer *t, const float **grad_dev, int64_t *rows, int *n_params) {
    if (!t || !grad_dev || !rows || !n_params) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    if (t->pg_mode == 0 || t->pg_rows == 0) return ntx_set_error(NTX_E_INVALID, "no parameter gradients: %s", t->pg_mode == 0 ? "ntx_trainer_enable_param_gradients is off" :
                                                                 (t->spg_rays ? "the last step was an instanced one (ntx_trainer_sample_param_gradients has its per-sample gradients)" :
                                                                  "no step has run since they were enabled"));
    *grad_dev = t->param_grad; *rows = t->pg_rows; *n_params = t->P;
    return NTX_OK;
}

int ntx_trainer_enable_input_gradients(ntx_trainer *t, int mode) {
    if (!t || mode < 0 || mode > 2) return ntx_set_error(NTX_E_INVALID, "trainer is NULL or mode is not 0 (off) / 1 (with the weight gradients) / 2 (inputs only)");
    if (mode != 0) {
        int rc = t->backend->enable_input_gradients();                                          // the chain refuses; the layer-by-layer backend places its buffers once
        if (rc != NTX_OK) return rc;
    } else { t->ig_rays = 0; t->ig_smp_rays = 0; }
    if (mode != t->ig_mode) t->pending.open = false;                                           // (the first enable re-places the transposed weights a pending forward filled)
    t->ig_mode = mode;
    return NTX_OK;
}

int ntx_trainer_enable_gradients(ntx_trainer *t, int param_mode, int input_mode) {
    if (!t || param_mode < 0 || param_mode > 2 || input_mode < 0 || input_mode > 2)
        return ntx_set_error(NTX_E_INVALID, "trainer is NULL or a mode is not 0 (off) / 1 (beside the weight gradients) / 2 (without them)");
    if (param_mode != 0 && t->P == 0)
        return ntx_set_error(NTX_E_INVALID, "parameter gradients: the model has no parameters (a Nerf, n_parameters [0, 0])");
    int rc = t->backend->enable_gradients(param_mode, input_mode);              // refuses before it places anything; places once
    if (rc != NTX_OK) return rc;
    if (param_mode == 0) { t->pg_rows = 0; t->spg_rays = 0; }
    if (input_mode == 0) { t->ig_rays = 0; t->ig_smp_rays = 0; }
    if (param_mode != t->pg_mode || input_mode != t->ig_mode) t->pending.open = false;      // set the modes before the forward
    t->pg_mode = param_mode; t->ig_mode = input_mode;
    return NTX_OK;
}

int ntx_trainer_ray_gradients(ntx_trainer *t, const float **d_rays_o, const float **d_rays_d, int64_t *n_rays) {
    if (!t || !d_rays_o || !d_rays_d || !n_rays) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    if (t->ig_mode == 0 || t->ig_rays == 0) return ntx_set_error(NTX_E_INVALID, "no ray gradients: %s", t->ig_mode == 0 ? "ntx_trainer_enable_input_gradients is off" :
                                                                 (t->ig_smp_rays ? "the last step was an instanced one (ntx_trainer_sample_input_gradients has its per-sample gradients)" :
                                                                  "no step has run since they were enabled"));
    *d_rays_o = t->d_rays_o; *d_rays_d = t->d_rays_d; *n_rays = t->ig_rays;
    return NTX_OK;
}

int ntx_trainer_sample_input_gradients(ntx_trainer *t, const float **d_pts, const float **d_dirs, int64_t *n_rays, int *n_samples) {
    if (!t || !d_pts || !d_dirs || !n_rays || !n_samples) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    if (t->ig_mode == 0 || t->ig_smp_rays == 0) return ntx_set_error(NTX_E_INVALID, "no per-sample input gradients: %s", t->ig_mode == 0 ? "ntx_trainer_enable_input_gradients is off" :
                                                                     "the last step since they were enabled was not an instanced one (ntx_trainer_ray_gradients has a plain step's)");
    *d_pts = t->d_pts; *d_dirs = t->d_dirs; *n_rays = t->ig_smp_rays; *n_samples = t->ig_S;
    return NTX_OK;
}

int ntx_trainer_adam_step(ntx_trainer *t, float lrate, float lrate_decay_steps, float lrate_decay_rate, float beta_1, float beta_2, float epsilon, ntx_stream stream) {
    if (!t) return ntx_set_error(NTX_E_INVALID, "trainer is NULL");
    if (int rc = no_weight_gradients(t, "ntx_trainer_adam_step")) return rc;
    TRAIN_TRY(hipSetDevice(t->device));
    const double step = (double)t->adam_iterations;
    double lr = lrate;
    if (lrate_decay_steps > 0) lr = (double)lrate * std::pow((double)lrate_decay_rate, step / (double)lrate_decay_steps);      // ExponentialDecay, staircase off
    const double tt = step + 1.0;
    const float lr_t = (float)((double)(float)lr * std::sqrt(1.0 - std::pow((double)beta_2, tt)) / (1.0 - std::pow((double)beta_1, tt)));
    hipLaunchKernelGGL(ntx_train::adam_kernel, dim3((unsigned)((t->n_weights + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t->w, t->grad, t->adam_m, t->adam_v,
                       (long long)t->n_weights, lr_t, beta_1, beta_2, epsilon);
    t->adam_iterations += 1;
    TRAIN_TRY(hipGetLastError());
    return NTX_OK;
}

int64_t ntx_trainer_iterations(const ntx_trainer *t) { return t ? t->adam_iterations : -1; }
}   // extern "C"
