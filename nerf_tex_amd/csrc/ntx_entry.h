// ntx_entry.h -- what the units with entries of the C ABI share (nerftex.hip: the context; ntx_standalone.hip: the entries without one): the
// error return of a HIP call, the options every sampling entry reads, and the launchers of the small kernels the context's entries use (no
// relocatable device code: a kernel is launched by a host function of the unit that defines it, and ntx_small_kernels.h is in one unit).
#pragma once
#include "nerftex.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

extern "C" int ntx_set_error(int code, const char *fmt, ...);   // nerftex.hip: the per-thread message behind ntx_last_error()
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return ntx_set_error(NTX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace ntx {
// ntx_render_opts (ABI v3) -> the generator's ray index map; identity when opts is NULL or the map is all zero
struct IndexMap {
    int64_t idx0, stride;
    uint32_t run;
};
inline int index_map_of(const ntx_render_opts *o, IndexMap *m) {
    *m = IndexMap{0, 0, 0xffffffffu};
    if (!o) return NTX_OK;
    if (o->size < NTX_RENDER_OPTS_V3_SIZE) return ntx_set_error(NTX_E_INVALID, "ntx_render_opts.size %u < %u: set it to sizeof(ntx_render_opts)", o->size, NTX_RENDER_OPTS_V3_SIZE);
    if (o->ray_index0 == 0 && o->ray_run_length == 0 && o->ray_run_stride == 0) return NTX_OK;
    if (o->ray_index0 < 0 || o->ray_run_length < 1 || o->ray_run_stride < o->ray_run_length)
        return ntx_set_error(NTX_E_INVALID, "bad ray index map: index0 %lld run_length %lld run_stride %lld", (long long)o->ray_index0,
                             (long long)o->ray_run_length, (long long)o->ray_run_stride);
    m->idx0 = o->ray_index0; m->stride = o->ray_run_stride;
    m->run = o->ray_run_length > 0xffffffffLL ? 0xffffffffu : (uint32_t)o->ray_run_length;   // local rays are < 2^31: one run then
    return NTX_OK;
}
inline int noise_of(const ntx_render_opts *o, uint32_t flags, float *std_out) {
    *std_out = 0.0f;
    if (!(flags & NTX_FLAG_RAW_NOISE)) return NTX_OK;
    if (!o) return ntx_set_error(NTX_E_INVALID, "NTX_FLAG_RAW_NOISE needs ntx_render_opts.raw_noise_std");
    if (!(o->raw_noise_std >= 0.0f) || std::isinf(o->raw_noise_std)) return ntx_set_error(NTX_E_INVALID, "raw_noise_std must be finite and >= 0");
    *std_out = o->raw_noise_std;
    return NTX_OK;
}

// ntx_standalone.hip, for the context's entries (the caller asks hipGetLastError)
void launch_gather_weights(hipStream_t st, const float *w, const int32_t *idx, const float *konst, size_t n, float *packed);   // ntx_set_weights_device
void launch_compact_hits(hipStream_t st, const float *t, int64_t n_rays, int32_t *hit_list, int32_t *hit_count, float *color_out, float *alpha_out, uint32_t flags,
                         const float *bkgd);                                                                                    // ntx_render_rays
// ntx_render_instanced: count the in-patch samples of every ray, then order the rays costliest first and set the hand-out's chunk table
void launch_inst_order(hipStream_t st, const float *dists, const uint8_t *hit, int64_t n_rays, int n_samples, int32_t *count, int32_t *order, int32_t *work_counter,
                       int n_waves, int ta, int tb, int32_t *chunk_tab);
}  // namespace ntx
