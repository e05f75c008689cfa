// nerftex.hip -- the context of libnerftex_hip.so and the entries of the C ABI (include/nerftex.h) that run a model's network: kernel dispatch,
// ntx_create .. ntx_destroy, ntx_mlp_forward, ntx_render_rays, ntx_render_instanced.  Reading a model descriptor is ntx_arch.h's, packing the
// weights ntx_pack.cpp's, the entries without a context ntx_standalone.hip's.  gfx950 only.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ntx_entry.h"
#include "ntx_pack.h"
#include "ntx_device.h"

using namespace ntx;

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

// every unit of the library reports through this; not part of the public ABI
extern "C" __attribute__((visibility("hidden"))) int ntx_set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// context
// ---------------------------------------------------------------------------------------------
struct ntx_ctx {
    int variant = 0;
    int device = 0;
    int n_cus = 0;
    int n_wgs = 0;
    float *packed = nullptr;        // device: stream | tail | aux
    size_t stream_floats = 0;       // incl. tail
    size_t n_packed = 0;
    ntx_model_desc_ex descx{};      // (the base descriptor, and param_depth / param_width when kind = NTX_MODEL_PARAMNERF_EX)
    uint16_t *packed16 = nullptr;   // device: fp16x3 stream; shares the f32 aux block
    size_t packed16_bytes = 0;
    uint16_t *packed16i = nullptr;  // device: fp16x3 stream of the kernels with per-sample directions (C1 with its direction segment); ParamNerf only
    size_t packed16i_bytes = 0;
    int32_t *hit_list = nullptr;    // device scratch of ntx_render_rays: compacted hit-ray indices, sized by ntx_reserve
    size_t hit_cap = 0;
    int32_t *hit_count = nullptr;   // device int32[8]: [0] number of hit rays, [1] work counter of the instance kernel, [2..5] its chunk table (inst_order_kernel)
    bool hoist_dir = true;          // false when NERFTEX_NO_DIR_HOIST is set at ntx_create (A/B knob for tests: same bits either way)
    uint16_t *inst_sidx = nullptr;  // device scratch of ntx_render_instanced: per wave, the execution list of its bundle of rays in flight (8.5 KiB each)
    // ntx_set_weights_device: where every float of the packed image comes from -- an index into the weight blob, or -1 and a constant
    int32_t *gather_idx = nullptr; float *gather_const = nullptr;
    bool x3_stale = false;   // the fp16x3 images were not remade by the last ntx_set_weights_device
};

// The big kernels of each model family live in their own translation units (ntx_variant.hip / ntx_variant_x3.hip
// compiled with -DNTX_VARIANT=k, the hoisted render kernels with -DNTX_HOIST=1|2) so that the build parallelises; this file
// only dispatches to them through one table.
namespace ntx {
#define NTX_DECL(k)                                                                  \
    hipError_t launch_render_v##k(int n_wgs, RenderArgs &a, hipStream_t st);         \
    hipError_t launch_mlp_v##k(int n_wgs, MlpArgs &a, hipStream_t st);               \
    hipError_t launch_instance_v##k(int n_wgs, InstanceArgs &a, hipStream_t st);     \
    hipError_t launch_render_hoist_v##k(int n_wgs, RenderArgs &a, hipStream_t st);   \
    hipError_t launch_render_hoist2_v##k(int n_wgs, RenderArgs &a, hipStream_t st);  \
    hipError_t launch_render_hoist3_v##k(int n_wgs, RenderArgs &a, hipStream_t st);  \
    hipError_t launch_render_x3_v##k(int n_wgs, RenderArgs &a, hipStream_t st);      \
    hipError_t launch_mlp_x3_v##k(int n_wgs, MlpArgs &a, hipStream_t st);            \
    hipError_t launch_instance_x3_v##k(int n_wgs, InstanceArgs &a, hipStream_t st);
NTX_DECL(0) NTX_DECL(1) NTX_DECL(2) NTX_DECL(3) NTX_DECL(4) NTX_DECL(5) NTX_DECL(6) NTX_DECL(7)
#undef NTX_DECL
}  // namespace ntx

struct Launchers {
    hipError_t (*render)(int, RenderArgs &, hipStream_t);
    hipError_t (*render_hoist)(int, RenderArgs &, hipStream_t);   // NULL: plain Nerf has no per-ray direction segment to hoist out of C1
    hipError_t (*render_hoist2)(int, RenderArgs &, hipStream_t);  // + the geometry-parameter blocks of L0 / L5 per ray; NULL: not built for the family
    hipError_t (*render_hoist3)(int, RenderArgs &, hipStream_t);  // + all of them but parameter 0's (blur_idx = 0); NULL: not built
    hipError_t (*mlp)(int, MlpArgs &, hipStream_t);
    hipError_t (*instance)(int, InstanceArgs &, hipStream_t);
    hipError_t (*render_x3)(int, RenderArgs &, hipStream_t);
    hipError_t (*mlp_x3)(int, MlpArgs &, hipStream_t);
    hipError_t (*instance_x3)(int, InstanceArgs &, hipStream_t);
};
#define NTX_ROW(k, hoist, hoist2, hoist3) {launch_render_v##k, hoist, hoist2, hoist3, launch_mlp_v##k, launch_instance_v##k, launch_render_x3_v##k, launch_mlp_x3_v##k, launch_instance_x3_v##k}
static const Launchers kLaunch[] = {   // indexed like kVariants
    NTX_ROW(0, launch_render_hoist_v0, launch_render_hoist2_v0, nullptr),
#ifndef NTX_DEV_ONLY_CARPET   // development builds link only the carpet family (compile time)
    NTX_ROW(1, launch_render_hoist_v1, launch_render_hoist2_v1, nullptr), NTX_ROW(2, launch_render_hoist_v2, nullptr, launch_render_hoist3_v2),
    NTX_ROW(3, nullptr, nullptr, nullptr), NTX_ROW(4, launch_render_hoist_v4, nullptr, nullptr), NTX_ROW(5, launch_render_hoist_v5, nullptr, nullptr),
    {launch_render_v6, nullptr, nullptr, nullptr, launch_mlp_v6, launch_instance_v6, nullptr, nullptr, nullptr},   // flex: float32, everything per sample
    {launch_render_v7, nullptr, nullptr, nullptr, launch_mlp_v7, launch_instance_v7, nullptr, nullptr, nullptr},   // flex with parameter branches
#else
    {}, {}, {}, {}, {}, {}, {},
#endif
};
#undef NTX_ROW
template <class Fn, class Args>
static hipError_t launch(Fn fn, const ntx_ctx *c, Args &a, hipStream_t st) {
    return fn ? fn(c->n_wgs, a, st) : hipErrorNotSupported;
}

// parameter slots of the kernel family <- columns of the caller's parameter rows (identity for the tuned families; the
// generic family has GEN_NGEO + GEN_NAPP slots and feeds 0 into those the model does not have)
template <class Args>
static void fill_param_map(const ntx_ctx *c, Args &a) {
    const Variant &v = kVariants[c->variant];
    const Dims m = dims_of(&c->descx.base);
    a.np_in = m.g + m.a + v.ipe;
    for (int k = 0; k < MAX_PARAM_SLOTS; ++k) a.pmap[k] = -1;
    for (int k = 0; k < v.n_geo && k < MAX_PARAM_SLOTS; ++k) a.pmap[k] = k < m.g ? (int8_t)k : (int8_t)-1;
    for (int j = 0; j < v.n_app && v.n_geo + j < MAX_PARAM_SLOTS; ++j) a.pmap[v.n_geo + j] = j < m.a ? (int8_t)(m.g + j) : (int8_t)-1;
}
// blur_idx (a column of the caller's rows) -> the slot the kernel compares with
static int blur_slot(const ntx_ctx *c, int blur_idx) {
    const Variant &v = kVariants[c->variant];
    const Dims m = dims_of(&c->descx.base);
    if (blur_idx < 0 || !v.gen) return blur_idx;
    return blur_idx < m.g ? blur_idx : v.n_geo + (blur_idx - m.g);
}

// NTX_FLAG_FP16X3 on this context: the family has the kernels, and the images are those of the weights
static int admit_fp16x3(const ntx_ctx *c, uint32_t flags) {
    if (!(flags & NTX_FLAG_FP16X3)) return NTX_OK;
    if (int rc = no_fp16x3(kVariants[c->variant])) return rc;
    if (c->x3_stale)
        return ntx_set_error(NTX_E_UNSUPPORTED, "the fp16x3 images are stale: the weights last came from device memory (ntx_set_weights_device remakes the float32 image only); "
                                                "ntx_set_weights remakes all of them");
    return NTX_OK;
}
// the float32 image: stream and aux block
template <class Args>
static void fill_stream(const ntx_ctx *c, Args &a) {
    a.wstream = reinterpret_cast<const f32x4 *>(c->packed);
    a.stream_bytes = (uint32_t)(c->stream_floats * sizeof(float));
    a.aux = c->packed + c->stream_floats;
}
// the fp16x3 stream of a kernel whose directions are per sample: ParamNerf uses the stream that keeps C1's direction segment; plain
// Nerf's one stream has it in C2 anyway
template <class Args>
static void use_fp16x3_dir_stream(const ntx_ctx *c, Args &a) {
    const int cd = kVariants[c->variant].cd;
    a.wstream = reinterpret_cast<const f32x4 *>(cd ? c->packed16i : c->packed16);
    a.stream_bytes = (uint32_t)(cd ? c->packed16i_bytes : c->packed16_bytes);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int ntx_abi_version(void) { return NTX_ABI_VERSION; }
const char *ntx_last_error(void) { return g_err; }

int ntx_create(const ntx_model_desc *desc, const float *weights_host, size_t n_floats, int device, ntx_ctx **out) {
    if (!out) return ntx_set_error(NTX_E_INVALID, "out is NULL");
    *out = nullptr;
    const int v = find_variant(desc);
    if (v < 0) return unsupported(desc);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ntx_set_error(NTX_E_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return ntx_set_error(NTX_E_INVALID, "device %d out of range [0,%d)", device, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ntx_set_error(NTX_E_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    ntx_ctx *c = new ntx_ctx();
    auto drop = [&](int rc) { ntx_destroy(c); *out = nullptr; return rc; };   // a failure from here on: the message stands, the context goes
    auto alloc = [](auto **p, size_t bytes) {
        const hipError_t e = hipMalloc((void **)p, bytes);
        return e == hipSuccess ? NTX_OK : ntx_set_error(NTX_E_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    };
    c->variant = v;
    c->device = device;
    c->n_cus = prop.multiProcessorCount;
    c->n_wgs = prop.multiProcessorCount;   // one 4-wave workgroup per CU: each wave owns a SIMD's register file
    if (desc->kind == NTX_MODEL_PARAMNERF_EX) c->descx = *reinterpret_cast<const ntx_model_desc_ex *>(desc);
    else c->descx.base = *desc;
    c->n_packed = packed_floats_of(v, desc);
    c->stream_floats = c->n_packed - aux_floats_of_variant(v);
    c->hoist_dir = getenv("NERFTEX_NO_DIR_HOIST") == nullptr;
    if (int rc = alloc(&c->packed, c->n_packed * sizeof(float))) return drop(rc);
    if (!kVariants[v].flex) {   // (the flex family has float32 kernels only)
        c->packed16_bytes = packed16_bytes(kVariants[v]);
        if (int rc = alloc(&c->packed16, c->packed16_bytes)) return drop(rc);
    }
    if (c->packed16 && kVariants[v].cd) {
        c->packed16i_bytes = packed16_bytes(kVariants[v], 1);
        if (int rc = alloc(&c->packed16i, c->packed16i_bytes)) return drop(rc);
    }
    *out = c;
    // all the device scratch the entry points will ever use: allocated here (and by ntx_reserve), never per call
    if (hipMalloc((void **)&c->hit_count, 8 * sizeof(int32_t)) != hipSuccess) return drop(ntx_set_error(NTX_E_HIP, "hipMalloc(hit_count)"));
    if (hipMalloc((void **)&c->inst_sidx, (size_t)c->n_wgs * 4 * INST_EXEC_CAP * sizeof(uint16_t)) != hipSuccess) return drop(ntx_set_error(NTX_E_HIP, "hipMalloc(inst_sidx)"));
    if (int rc = ntx_reserve(c, NTX_DEFAULT_MAX_RAYS)) return drop(rc);
    if (weights_host) {
        if (int rc = ntx_set_weights(c, weights_host, n_floats)) return drop(rc);
    } else if (kVariants[v].flex) {   // all-zero weights, but the image carries the architecture
        const std::vector<float> zeros(view_blob_of(v, desc).count, 0.0f);
        if (int rc = ntx_set_weights(c, zeros.data(), zeros.size())) return drop(rc);
    } else {
        auto zero = [&]() {
            HIP_TRY(hipMemset(c->packed, 0, c->n_packed * sizeof(float)));
            if (c->packed16) HIP_TRY(hipMemset(c->packed16, 0, c->packed16_bytes));
            if (c->packed16i) HIP_TRY(hipMemset(c->packed16i, 0, c->packed16i_bytes));
            return (int)NTX_OK;
        };
        if (int rc = zero()) return drop(rc);
    }
    return NTX_OK;
}

int ntx_reserve(ntx_ctx *ctx, int64_t max_rays) {
    if (!ctx) return ntx_set_error(NTX_E_INVALID, "ctx is NULL");
    if (max_rays < 0 || max_rays > 0x7fffffff) return ntx_set_error(NTX_E_INVALID, "max_rays %lld outside [0, 2^31)", (long long)max_rays);
    if ((size_t)max_rays == ctx->hit_cap && (ctx->hit_list || max_rays == 0)) return NTX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());   // a launch may still be walking the old list
    if (ctx->hit_list) HIP_TRY(hipFree(ctx->hit_list));
    ctx->hit_list = nullptr; ctx->hit_cap = 0;
    // ntx_render_rays: hit_list[max_rays]; ntx_render_instanced: order[max_rays] | count[max_rays]
    if (max_rays > 0) HIP_TRY(hipMalloc((void **)&ctx->hit_list, (size_t)max_rays * 2 * sizeof(int32_t)));
    ctx->hit_cap = (size_t)max_rays;
    return NTX_OK;
}

int ntx_set_weights_device(ntx_ctx *ctx, const float *weights_dev, size_t n_floats, ntx_stream stream) {
    if (!ctx || !weights_dev) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    const size_t want = view_blob_of(ctx->variant, &ctx->descx.base).count;
    if (n_floats != want) return ntx_set_error(NTX_E_INVALID, "weight blob has %zu floats, model needs %zu", n_floats, want);
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->gather_idx) {
        // The packer only PLACES weights (and a few constants: the flex family's descriptor, zero padding).  Packing two blobs of the weights'
        // own numbers -- i + 1 and 2 (i + 1), exact in float32 below 2^23 -- tells every packed float's source: doubled = weight i, equal = constant.
        if (n_floats >= (size_t)1 << 22) return ntx_set_error(NTX_E_UNSUPPORTED, "ntx_set_weights_device: the model has more than 2^22 weights");
        std::vector<float> b1(n_floats), b2(n_floats), p1(ctx->n_packed), p2(ctx->n_packed);
        for (size_t i = 0; i < n_floats; ++i) { b1[i] = (float)(i + 1); b2[i] = (float)(2 * (i + 1)); }
        int rc = ntx_pack_weights(&ctx->descx.base, b1.data(), n_floats, p1.data(), p1.size());
        if (rc == NTX_OK) rc = ntx_pack_weights(&ctx->descx.base, b2.data(), n_floats, p2.data(), p2.size());
        if (rc != NTX_OK) return rc;
        std::vector<int32_t> idx(ctx->n_packed);
        for (size_t i = 0; i < ctx->n_packed; ++i) {
            const float a = p1[i], b = p2[i];
            if (a >= 1.0f && a <= (float)n_floats && b == 2.0f * a && a == std::floor(a)) idx[i] = (int32_t)a - 1;
            else if (memcmp(&a, &b, sizeof(float)) == 0) idx[i] = -1;
            else return ntx_set_error(NTX_E_UNSUPPORTED, "ntx_set_weights_device: packed float %zu is neither a weight nor a constant", i);
        }
        HIP_TRY(hipMalloc((void **)&ctx->gather_idx, ctx->n_packed * sizeof(int32_t)));
        HIP_TRY(hipMalloc((void **)&ctx->gather_const, ctx->n_packed * sizeof(float)));
        HIP_TRY(hipMemcpy(ctx->gather_idx, idx.data(), ctx->n_packed * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->gather_const, p1.data(), ctx->n_packed * sizeof(float), hipMemcpyHostToDevice));
    }
    launch_gather_weights((hipStream_t)stream, weights_dev, ctx->gather_idx, ctx->gather_const, ctx->n_packed, ctx->packed);
    HIP_TRY(hipGetLastError());
    ctx->x3_stale = ctx->packed16 != nullptr;
    return NTX_OK;
}

int ntx_set_weights(ntx_ctx *ctx, const float *weights_host, size_t n_floats) {
    if (!ctx || !weights_host) return ntx_set_error(NTX_E_INVALID, "NULL argument");
    std::vector<float> packed(ctx->n_packed);
    const int rc = ntx_pack_weights(&ctx->descx.base, weights_host, n_floats, packed.data(), packed.size());
    if (rc != NTX_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());   // a launch on any stream may still be reading the images (a blocking copy waits for the null stream alone)
    HIP_TRY(hipMemcpy(ctx->packed, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
    if (ctx->packed16) {
        std::vector<uint16_t> p16(ctx->packed16_bytes / 2);
        pack16(kVariants[ctx->variant], dims_of(&ctx->descx.base), weights_host, p16.data());
        HIP_TRY(hipMemcpy(ctx->packed16, p16.data(), ctx->packed16_bytes, hipMemcpyHostToDevice));
    }
    if (ctx->packed16i) {
        std::vector<uint16_t> p16(ctx->packed16i_bytes / 2);
        pack16(kVariants[ctx->variant], dims_of(&ctx->descx.base), weights_host, p16.data(), 1);
        HIP_TRY(hipMemcpy(ctx->packed16i, p16.data(), ctx->packed16i_bytes, hipMemcpyHostToDevice));
    }
    ctx->x3_stale = false;
    return NTX_OK;
}

int ntx_destroy(ntx_ctx *ctx) {
    if (!ctx) return NTX_OK;
    if (ctx->packed) (void)hipFree(ctx->packed);
    if (ctx->packed16) (void)hipFree(ctx->packed16);
    if (ctx->packed16i) (void)hipFree(ctx->packed16i);
    if (ctx->hit_list) (void)hipFree(ctx->hit_list);
    if (ctx->hit_count) (void)hipFree(ctx->hit_count);
    if (ctx->inst_sidx) (void)hipFree(ctx->inst_sidx);
    if (ctx->gather_idx) (void)hipFree(ctx->gather_idx);
    if (ctx->gather_const) (void)hipFree(ctx->gather_const);
    delete ctx;
    return NTX_OK;
}

int ntx_kernel_info(ntx_ctx *ctx, int *n_workgroups, int *threads_per_workgroup, int *n_cus) {
    if (!ctx) return ntx_set_error(NTX_E_INVALID, "ctx is NULL");
    if (n_workgroups) *n_workgroups = ctx->n_wgs;
    if (threads_per_workgroup) *threads_per_workgroup = 256;
    if (n_cus) *n_cus = ctx->n_cus;
    return NTX_OK;
}

int ntx_mlp_forward(ntx_ctx *ctx, const float *pos, const float *dirs, const float *params, int64_t m, uint32_t flags,
                    float *color_out, float *sigma_out, ntx_stream stream) {
    if (!ctx) return ntx_set_error(NTX_E_INVALID, "ctx is NULL");
    if (m < 0) return ntx_set_error(NTX_E_INVALID, "m < 0");
    if (flags & ~NTX_FLAG_FP16X3) return ntx_set_error(NTX_E_INVALID, "ntx_mlp_forward takes NTX_FLAG_FP16X3 or 0, got 0x%x", flags);
    if (m == 0) return NTX_OK;
    if (int rc = admit_fp16x3(ctx, flags)) return rc;
    const Dims dm_ = dims_of(&ctx->descx.base);
    if (!pos || !dirs || !color_out || !sigma_out || (!params && dm_.g + dm_.a > 0))
        return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    HIP_TRY(hipSetDevice(ctx->device));   // the launch goes to the context's device whatever the caller's current one is
    MlpArgs a{};
    fill_stream(ctx, a);
    a.pos = pos; a.dirs = dirs; a.params = params;
    a.color_out = color_out; a.sigma_out = sigma_out;
    a.m = m;
    fill_param_map(ctx, a);
    if (flags & NTX_FLAG_FP16X3) {
        use_fp16x3_dir_stream(ctx, a);
        HIP_TRY(launch(kLaunch[ctx->variant].mlp_x3, ctx, a, (hipStream_t)stream));
        return NTX_OK;
    }
    HIP_TRY(launch(kLaunch[ctx->variant].mlp, ctx, a, (hipStream_t)stream));
    return NTX_OK;
}

int ntx_render_rays(ntx_ctx *ctx, const float *rays_o, const float *rays_d, const float *t, const float *params,
                    int64_t rays_per_param_row, const float *cone_scale, int64_t n_rays, int n_samples, int blur_idx,
                    uint32_t flags, const float *bkgd, const float *z_vals, uint64_t perturb_seed, const ntx_render_opts *opts,
                    float *color_out, float *alpha_out, float *weights_out, int32_t *status_flag, ntx_stream stream) {
    // every check comes before the first launch: a call that fails has written nothing
    if (!ctx) return ntx_set_error(NTX_E_INVALID, "ctx is NULL");
    if (n_rays < 0) return ntx_set_error(NTX_E_INVALID, "n_rays < 0");
    if (n_samples < 2) return ntx_set_error(NTX_E_INVALID, "n_samples must be >= 2 (renderer.py:174-177 needs a previous step)");
    if (n_rays == 0) return NTX_OK;
    const Variant &v = kVariants[ctx->variant];
    if (int rc = admit_fp16x3(ctx, flags)) return rc;
    const Dims dm_ = dims_of(&ctx->descx.base);
    const int np = dm_.g + dm_.a + v.ipe;   // parameters per row at the ABI (mip: incl. the spliced-out blur parameter)
    if (!rays_o || !rays_d || !t || !color_out || !alpha_out || (!params && np > 0))
        return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (rays_per_param_row < 1) return ntx_set_error(NTX_E_INVALID, "rays_per_param_row must be >= 1");
    if (blur_idx < -1 || blur_idx >= np) return ntx_set_error(NTX_E_INVALID, "blur_idx %d outside [-1,%d)", blur_idx, np);
    if (v.ipe && blur_idx < 0) return ntx_set_error(NTX_E_INVALID, "an IPE (mip) model needs blur_idx: the cone radius parameter (renderer.py:385)");
    if (blur_idx >= 0 && !cone_scale) return ntx_set_error(NTX_E_INVALID, "blur_idx set but cone_scale is NULL");
    if ((size_t)n_rays > ctx->hit_cap)
        return ntx_set_error(NTX_E_INVALID, "n_rays %lld exceeds the %zu rays this context reserved; call ntx_reserve first", (long long)n_rays, ctx->hit_cap);
    IndexMap im;
    float noise_std;
    if (int rc = index_map_of(opts, &im)) return rc;
    if (int rc = noise_of(opts, flags, &noise_std)) return rc;
    const bool x3 = (flags & NTX_FLAG_FP16X3) != 0;
    // the per-ray direction vector is valid unless the blur scaling hits an APPEARANCE parameter per sample (renderer.py:155-158)
    const bool dir_const = v.cd && (blur_idx < 0 || blur_idx < dm_.g || v.ipe);
    if (x3 && v.cd && !dir_const)
        return ntx_set_error(NTX_E_UNSUPPORTED, "fp16x3: blur_idx %d scales an appearance parameter per sample; use float32", blur_idx);
    RenderArgs a{};
    fill_stream(ctx, a);
    a.rays_o = rays_o; a.rays_d = rays_d; a.t = t; a.params = params; a.cone = cone_scale; a.z_vals = z_vals;
    a.color_out = color_out; a.alpha_out = alpha_out; a.weights_out = weights_out; a.status = status_flag;
    a.n_rays = n_rays; a.rays_per_row = rays_per_param_row;
    a.n_samples = n_samples; a.blur_idx = blur_slot(ctx, blur_idx); a.flags = flags;
    fill_param_map(ctx, a);
    a.delta = (1.0f - 0.0f) / (float)(n_samples - 1 + v.ipe);   // mip: S+1 segment edges (renderer.py:374)
    a.seed_lo = (uint32_t)perturb_seed; a.seed_hi = (uint32_t)(perturb_seed >> 32);
    a.raw_noise_std = noise_std; a.idx0 = im.idx0; a.idx_run = im.run; a.idx_stride = im.stride;
    for (int k = 0; k < 3; ++k) a.bkgd[k] = bkgd ? bkgd[k] : 1.0f;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    // Hit-ray compaction: culled rays get their final value here, the render kernel walks the list.  The list lives in the
    // context, so launches on one context must be stream-ordered.
    HIP_TRY(hipMemsetAsync(ctx->hit_count, 0, sizeof(int32_t), st));
    launch_compact_hits(st, t, n_rays, ctx->hit_list, ctx->hit_count, color_out, alpha_out, flags, a.bkgd);
    HIP_TRY(hipGetLastError());
    a.hit_list = ctx->hit_list; a.hit_count = ctx->hit_count;
    const Launchers &L = kLaunch[ctx->variant];
    if (x3) {
        // ParamNerf: C1's direction segment always enters as the per-ray vector dir_block computes in float32 from the float32 stream
        a.dir_wstream = a.wstream; a.dir_stream_bytes = a.stream_bytes;
        a.wstream = reinterpret_cast<const f32x4 *>(ctx->packed16);
        a.stream_bytes = (uint32_t)ctx->packed16_bytes;
        HIP_TRY(launch(L.render_x3, ctx, a, st));
        return NTX_OK;
    }
    // float32: direction features and appearance parameters are per-ray constants (renderer.py:152-154): the HOIST kernel
    // evaluates the colour layer's direction segment once per ray (dir_block) instead of once per sample -- same bits
    // -- and without a blur_idx the geometry parameters are per-ray constants as well: HOIST = 2 also starts L0 and L5 from
    // per-ray rows (bias + the geometry block of their position segments)
    // -- and with blur_idx = 0 all of them but parameter 0's: HOIST = 3 (its block comes last in the layout)
    if (ctx->hoist_dir && dir_const && blur_idx < 0 && L.render_hoist2) HIP_TRY(launch(L.render_hoist2, ctx, a, st));
    else if (ctx->hoist_dir && dir_const && blur_idx == 0 && dm_.g >= 2 && L.render_hoist3) HIP_TRY(launch(L.render_hoist3, ctx, a, st));
    else if (ctx->hoist_dir && dir_const && L.render_hoist) HIP_TRY(launch(L.render_hoist, ctx, a, st));
    else HIP_TRY(launch(L.render, ctx, a, st));
    return NTX_OK;
}

int ntx_render_instanced(ntx_ctx *ctx, const float *rays_d_map, const float *pts, const float *t, const float *dists,
                         const float *color_last, const float *alpha_last, const float *alpha_weight,
                         const int32_t *instance_id, const uint8_t *hit, const float *params_map, const float *cone_scale,
                         int64_t n_rays, int n_samples, int blur_idx, float patch_scale, float density_scale,
                         uint32_t flags, const float *bkgd, const float *instance_color, const ntx_render_opts *opts,
                         float *color_out, float *alpha_out, int32_t *status_flag, ntx_stream stream) {
    if (!ctx) return ntx_set_error(NTX_E_INVALID, "ctx is NULL");
    if (n_rays < 0) return ntx_set_error(NTX_E_INVALID, "n_rays < 0");
    if (n_samples < 1 || n_samples > MAX_INSTANCE_SAMPLES)
        return ntx_set_error(NTX_E_INVALID, "n_samples %d outside [1,%d]", n_samples, MAX_INSTANCE_SAMPLES);
    if (n_rays == 0) return NTX_OK;
    const Variant &v = kVariants[ctx->variant];
    if (int rc = admit_fp16x3(ctx, flags)) return rc;
    const Dims dm_ = dims_of(&ctx->descx.base);
    const int np = dm_.g + dm_.a + v.ipe;
    if (v.ipe && (blur_idx < 0 || !t)) return ntx_set_error(NTX_E_INVALID, "an IPE (mip) model needs blur_idx and t (renderer.py:511, 575)");
    if (!rays_d_map || !pts || !dists || !color_last || !alpha_last || !hit || !color_out || !alpha_out ||
        (!params_map && np > 0))
        return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    if (blur_idx < -1 || blur_idx >= np) return ntx_set_error(NTX_E_INVALID, "blur_idx %d outside [-1,%d)", blur_idx, np);
    if (blur_idx >= 0 && (!cone_scale || !t)) return ntx_set_error(NTX_E_INVALID, "blur_idx set but cone_scale / t is NULL");
    if (instance_color && !instance_id) return ntx_set_error(NTX_E_INVALID, "instance_color given without instance_id");
    if (!(patch_scale > 0.0f)) return ntx_set_error(NTX_E_INVALID, "patch_scale must be > 0");
    if (flags & NTX_FLAG_PERTURB) return ntx_set_error(NTX_E_INVALID, "NTX_FLAG_PERTURB: the instancer places the samples of this path, there is nothing to jitter");
    IndexMap im;
    float noise_std;
    if (int rc = index_map_of(opts, &im)) return rc;
    if (int rc = noise_of(opts, flags, &noise_std)) return rc;
    InstanceArgs a{};
    a.raw_noise_std = noise_std; a.idx0 = im.idx0; a.idx_run = im.run; a.idx_stride = im.stride;
    a.seed_lo = opts ? (uint32_t)opts->noise_seed : 0u; a.seed_hi = opts ? (uint32_t)(opts->noise_seed >> 32) : 0u;
    a.run_hoist = ctx->hoist_dir ? 1 : 0;
    if (const char *dbg = getenv("NERFTEX_DEBUG_RUNS")) a.run_hoist = atoi(dbg);   // development: ntx_device.h instance_kernel
    a.sidx_scratch = ctx->inst_sidx;
    fill_stream(ctx, a);
    a.rays_d_map = rays_d_map; a.pts = pts; a.t = t; a.dists = dists; a.color_last = color_last;
    a.alpha_last = alpha_last; a.alpha_weight = alpha_weight; a.params_map = params_map; a.cone = cone_scale;
    a.instance_color = instance_color; a.instance_id = instance_id; a.hit = hit;
    a.color_out = color_out; a.alpha_out = alpha_out; a.status = status_flag;
    a.n_rays = n_rays; a.n_samples = n_samples; a.blur_idx = blur_slot(ctx, blur_idx); a.flags = flags;
    fill_param_map(ctx, a);
    a.patch_scale = patch_scale; a.density_scale = density_scale;
    for (int k = 0; k < 3; ++k) a.bkgd[k] = bkgd ? bkgd[k] : 1.0f;
    if (n_rays > 0x7fffffff) return ntx_set_error(NTX_E_INVALID, "n_rays %lld exceeds int32", (long long)n_rays);
    // dynamic ray hand-out: a device counter owned by the context (stream-ordered use, like the other scratch)
    if ((size_t)n_rays > ctx->hit_cap)
        return ntx_set_error(NTX_E_INVALID, "n_rays %lld exceeds the %zu rays this context reserved; call ntx_reserve first", (long long)n_rays, ctx->hit_cap);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    a.work_counter = ctx->hit_count + 1;   // [0] hits of ntx_render_rays, [1] this counter (inst_order_kernel zeroes it)
    {   // hand the rays out costliest first (ntx_small_kernels.h: inst_*_kernel); scratch reserved in the context
        int32_t *order = ctx->hit_list, *count = ctx->hit_list + ctx->hit_cap;
        // chunks of the hand-out (float32 kernel): the last ta rays per wave not in fours, the last tb single; development knobs in
        // NERFTEX_DEBUG_RUNS: bit 3 = single rays throughout, bits 8-12 / 16-20 = ta / tb
        int ta = 6, tb = 3;
        if ((a.run_hoist >> 8) & 31) ta = (a.run_hoist >> 8) & 31;
        if ((a.run_hoist >> 16) & 31) tb = (a.run_hoist >> 16) & 31;
        if (a.run_hoist & 8) ta = -1;
        a.chunk_tab = ctx->hit_count + 2;
        launch_inst_order(st, dists, hit, n_rays, n_samples, count, order, a.work_counter, ctx->n_wgs * 4, ta, tb, ctx->hit_count + 2);
        HIP_TRY(hipGetLastError());
        a.order = order; a.count = count;
    }
    if (flags & NTX_FLAG_FP16X3) {
        use_fp16x3_dir_stream(ctx, a);
        HIP_TRY(launch(kLaunch[ctx->variant].instance_x3, ctx, a, (hipStream_t)stream));
        return NTX_OK;
    }
    HIP_TRY(launch(kLaunch[ctx->variant].instance, ctx, a, (hipStream_t)stream));
    return NTX_OK;
}

}  // extern "C"
