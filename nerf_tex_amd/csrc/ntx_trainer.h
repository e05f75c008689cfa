// ntx_trainer.h -- what the units of a training step share on the host: the handle behind ntx_trainer_* (ntx_trainer.hip), the interface of
// its two backends (ntx_backend_chain.hip: the 8 x 256 chain on ntx_train_device.h's kernels; ntx_backend_flex.hip: any other architecture
// layer by layer, parameter branches included), the owner of its device memory, and the launchers of the kernels more than one unit uses (no relocatable device code: a
// kernel is launched by a host function of the unit that defines it).
#pragma once
#include "ntx_arch.h"   // the model's dimensions and the one view of its blob; ntx_set_error
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#define TRAIN_TRY(expr)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return ntx_set_error(NTX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
namespace ntx_train {
constexpr int MAX_TRAIN_SAMPLES = 1024;                // samples per ray (the composite kernels hold a ray in LDS)
// Every device allocation of a handle and its backend: what is on the list is freed with the handle, and nothing else is.  The first failure
// sticks (rc): the allocations behind it are skipped, so a create runs through and looks at rc once.
struct DeviceMemory {
    std::vector<void *> ptrs; int rc = NTX_OK;
    template <class T>
    int alloc(T **d, size_t n, bool zero = false) {
        if (rc != NTX_OK) return rc;
        const size_t bytes = (n ? n : 1) * sizeof(T);
        if (hipMalloc((void **)d, bytes) != hipSuccess) return rc = ntx_set_error(NTX_E_HIP, "hipMalloc of %zu bytes failed", bytes);
        ptrs.push_back(*d);
        if (zero && hipMemset(*d, 0, bytes) != hipSuccess) return rc = ntx_set_error(NTX_E_HIP, "hipMemset failed");
        return rc;
    }
    template <class T>
    int upload(T **d, const std::vector<T> &host, const char *what) {      // a table the kernels read
        if (alloc(d, host.size()) == NTX_OK && hipMemcpy(*d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            rc = ntx_set_error(NTX_E_HIP, "%s table upload failed", what);
        return rc;
    }
    void release(void *p) {                                                  // one allocation given back early (hipFree waits for what is in flight)
        for (size_t i = 0; i < ptrs.size(); ++i) if (ptrs[i] == p) { (void)hipFree(p); ptrs.erase(ptrs.begin() + i); return; }
    }
    ~DeviceMemory() { for (void *p : ptrs) (void)hipFree(p); }
};

// the rays of one step and the model's encodings, as the backends' encoders take them (host and device)
struct StepRays {
    const float *rays_o, *rays_d, *z, *params, *cone; long long rays_per_param_row, n_rays; int S, blur_idx, n_geo, n_app, pos_freq, dir_freq, param_freq;
    __host__ __device__ long long M() const { return n_rays * S; }
    int n_blocks() const { return (int)((M() + 31) / 32); }       // blocks of 32 samples
};
// The samples of one instanced step (ntx_train_forward_instanced): the instancer's buffers as the caller handed them, and the compaction of
// the step -- sample m = ray * S + s is LIVE iff hit[ray] != 0 && dists[m] > 0; the live samples numbered in ascending m are the rows the
// network runs on: live[row] = m, row_of[m] = row or -1.  Nothing of pts / rays_d_map / t_map / alpha_weight / params_map is read at a
// sample that is not live.
struct StepSamples {
    const float *rays_d_map, *pts, *t_map, *dists, *color_last, *alpha_last, *alpha_weight; const uint8_t *hit; const float *params_map, *cone;
    long long n_rays; int S, blur_idx, n_geo, n_app, pos_freq, dir_freq, param_freq; float patch_scale, density_scale;
    const int *live, *row_of; long long n_live;
    __host__ __device__ long long M() const { return n_rays * S; }
    // column c of a live sample's parameters as the network sees it: blur_idx's times the sample's footprint (renderer.py:259-263)
    __device__ __forceinline__ float blur_scale(long long m, long long ray) const { return cone[ray] * t_map[m] / patch_scale; }
};
// The network between the encoded rays and the composite.  forward leaves sigma, raw_rgb and dists in the handle's buffers and keeps what the
// way back needs; backward takes the handle's dgrad (and its O-layout copy dhead) to the handle's grad -- right behind the forward
// (ntx_train_step_gradients) or later from the same StepRays (ntx_train_backward: the caller keeps the rays' buffers alive until then).
struct Backend {
    virtual ~Backend() {}                                                            // (its device buffers are on the handle's list)
    virtual int forward(const StepRays &r, hipStream_t st) = 0;
    virtual int backward(const StepRays &r, hipStream_t st) = 0;
    virtual int activation(int layer, int64_t n_samples_total, float *out_host) = 0;   // ntx_trainer_activation, the arguments checked
    // ntx_train_forward_instanced: the network on the n_live compact rows of a StepSamples -- forward leaves sigma [n_live] and raw_rgb
    // [n_live][3]; backward takes dgrad [n_live][4] to the handle's grad and, where asked for, the per-sample dL/d params to sample_pg [N][S][P]
    // (takes_samples: asked before anything of the step is launched)
    virtual int takes_samples() {
        return ntx_set_error(NTX_E_UNSUPPORTED, "an instanced step: the fused chain (ntx_trainer_create) runs on whole rays; the layer-by-layer trainer takes the "
                             "same model on the in-patch samples (ntx_trainer_create_flex, ntx_trainer_create_flex_ex)");
    }
    // ntx_trainer_enable_instanced: a backend that takes samples only once it is asked to (the chain) places what it needs, once; the
    // layer-by-layer backend takes them as it is
    virtual int enable_samples() { return takes_samples(); }
    virtual int forward_samples(const StepSamples &, hipStream_t) { return takes_samples(); }
    virtual int backward_samples(const StepSamples &, float *, hipStream_t) { return takes_samples(); }
    // ntx_trainer_enable_param_gradients, mode 1 / 2 on a model with parameters: places what dL/d params needs (once); the handle keeps the mode
    virtual int enable_param_gradients() {
        return ntx_set_error(NTX_E_UNSUPPORTED, "parameter gradients: the fused chain (ntx_trainer_create) stops at the encoded inputs; the layer-by-layer "
                             "trainer takes the same model (ntx_trainer_create_flex, ntx_trainer_create_flex_ex)");
    }
    // ntx_trainer_enable_input_gradients, mode 1 / 2: places what dL/d rays_o, rays_d (a plain step) and dL/d pts, rays_d_map (an instanced
    // one) need (once); the handle keeps the mode
    virtual int enable_input_gradients() {
        return ntx_set_error(NTX_E_UNSUPPORTED, "input gradients: the fused chain (ntx_trainer_create) stops at the encoded inputs; the layer-by-layer "
                             "trainer takes the same model (ntx_trainer_create_flex, ntx_trainer_create_flex_ex)");
    }
    // ntx_trainer_enable_gradients, both modes at once and checked (0 .. 2; param_mode 0 on a model without parameters): places what the
    // non-zero ones need (once) and refuses before anything is placed; the handle keeps the modes.  The chain's way in
    virtual int enable_gradients(int param_mode, int input_mode) {
        if (param_mode != 0) { const int rc = enable_param_gradients(); if (rc != NTX_OK) return rc; }
        return input_mode != 0 ? enable_input_gradients() : NTX_OK;
    }
};
// what an entry's architecture check makes of a descriptor
struct TrainDims { ntx_model_desc desc; int Kp, Kd; bool ipe; size_t n_weights; int param_depth, param_width; };   // param_*: the branches the model HAS (0 without parameters)
using TLayer = ntx::BlobLayer;                    // offsets into the Keras-order blob (kernel [in][out], then bias)
}   // namespace ntx_train

struct ntx_trainer {
    int device = 0, cus = 256;
    ntx_model_desc desc{};
    int param_depth = 0, param_width = 0;      // the parameter branches of an extended descriptor (ntx_trainer_create_flex_ex): the base struct has no room for them
    int Kp = 0, Kd = 0, P = 0;                 // features of pos_map / dir_map, parameters the model sees
    bool ipe = false; size_t n_weights = 0;    // ipe: an IntegratedPositionalEncoding model, a MipRenderer step
    bool flex = false;                         // the layer-by-layer backend (kinds 1 and 2 of the create entries)
    int precision = 0;                         // ntx_trainer_set_precision: the contractions of the layer-by-layer backend (NTX_PRECISION_F32 or _BF16X6)
    long long cap = 0, cap_blocks = 0, cap_rays = 0;   // samples (blocks of 32 samples, rays) the buffers hold
    float *w = nullptr, *grad = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    float *stash = nullptr;                    // a second gradient (ntx_trainer_stash_gradients)
    float *sigma = nullptr, *raw_rgb = nullptr, *z = nullptr, *dists = nullptr, *noise = nullptr;
    float *dgrad = nullptr, *dhead = nullptr;  // the composite's adjoint [M][4], and the same as one O-layout tile per block (the chain's narrow heads' dY)
    float *color = nullptr, *alpha_out = nullptr, *ray_loss = nullptr, *loss = nullptr;
    float *weights_out = nullptr;              // caller's [N][S] buffer for the composite's weights of the next steps, or NULL
    int pg_mode = 0;                           // ntx_trainer_enable_param_gradients: 0 off, 1 dL/d params beside the weight gradients, 2 dL/d params alone
    float *param_grad = nullptr;               // [rows][P] of the last step (the backend places it at the first enable), pg_rows = 0: no step yet
    long long pg_rows = 0;
    // an instanced step (ntx_train_forward_instanced), placed at the first one for the trainer's capacity: the compaction's maps and scan
    // workspace, and -- at the first instanced backward under pg_mode 1 / 2 -- the per-sample dL/d params [N][S][P] (spg_rays = 0: no such step yet)
    int *live = nullptr, *row_of = nullptr, *ray_live = nullptr; long long *n_live_dev = nullptr;
    float *sample_pg = nullptr; long long spg_rays = 0; int spg_S = 0;
    // ntx_trainer_enable_input_gradients: 0 off, 1 dL/d rays and sample points beside the weight gradients, 2 without them.  d_rays_o / d_rays_d
    // [cap_rays][3] of the last plain step (the backend places them at the first enable; ig_rays = 0: no such step yet), d_pts / d_dirs [cap][3]
    // of the last instanced one (placed at the first instanced backward under the mode; ig_smp_rays = 0: no such step yet)
    int ig_mode = 0;
    float *d_rays_o = nullptr, *d_rays_d = nullptr, *d_pts = nullptr, *d_dirs = nullptr;
    long long ig_rays = 0, ig_smp_rays = 0; int ig_S = 0;
    const float *step_noise = nullptr;         // the density noise of the step whose way back runs (NULL without NTX_FLAG_RAW_NOISE): the ray fold's |d| term reads it
    // the compaction's maps and scan workspace, for the capacity: at the first instanced step, or at ntx_trainer_enable_instanced
    int place_sample_maps() {
        if (live) return mem.rc;                           // (a failed allocation sticks in mem.rc)
        mem.alloc(&live, (size_t)cap); mem.alloc(&row_of, (size_t)cap); mem.alloc(&ray_live, (size_t)cap_rays); mem.alloc(&n_live_dev, 1);
        return mem.rc;
    }
    bool takes_weight_gradients() const { return pg_mode != 2 && ig_mode != 2; }   // the weight gradient is taken unless EITHER mode is 2
    long long adam_iterations = 0;
    // ntx_train_forward's step until its ntx_train_backward: the caller's rays (alive and unchanged until then), what the composite was run with;
    // samples: the step is ntx_train_forward_instanced's, and smp holds the caller's buffers instead of rays
    struct Pending { bool open = false, samples = false; ntx_train::StepRays rays{}; ntx_train::StepSamples smp{}; uint32_t flags = 0; float bkgd[3] = {1.0f, 1.0f, 1.0f};
                     const float *noise = nullptr;
                     const float *d_weights = nullptr; } pending;   // d_weights: ntx_trainer_weight_cotangent's [N][S] for the pending step's backward, or NULL
    ntx_train::Backend *backend = nullptr;
    ntx_train::DeviceMemory mem;               // (destroyed after the body below has run)
    ~ntx_trainer() { (void)hipSetDevice(device); delete backend; }
};
namespace ntx_train {
// ntx_backend_chain.hip / ntx_backend_flex.hip: the entry's architecture check (no device is asked for), and the backend of a handle whose
// common buffers exist (allocations go through t->mem; the caller looks at t->mem.rc)
int chain_check(const ntx_model_desc *desc, TrainDims *dims);
int chain_backend_create(ntx_trainer *t);
int flex_check(const ntx_model_desc *desc, TrainDims *dims, bool branches = false);   // branches: ntx_trainer_create_flex_ex's domain (desc is an ntx_model_desc_ex)
int flex_backend_create(ntx_trainer *t);
// ntx_gemm.hip: C[i][j] = sum_p A'(i, p) B[p * ldb + j], A'(i, p) = a_kcontig ? A[i * lda + p] : A[p * lda + i]
struct GemmArgs {
    const float *A; int lda; const float *B; int ldb; float *C; int ldc;
    int M, N, K;
    const float *bias;               // NULL or [N]: added to every row
    const float *mask; int ldmask;   // NULL, or C[i][j] is kept only where mask[i * ldmask + j] > 0 (the ReLU of a stored activation)
    int relu, accumulate;            // C = max(C, 0);  C += what was there
    int k_chunk; long long split_stride;   // blockIdx.z = z covers p in [z * k_chunk, (z + 1) * k_chunk) and writes to C + z * split_stride
    float *colsum;                   // NULL, or [n_split][N]: the column sums of B over each split's rows (the bias gradient rides along with dW)
    int aligned;                     // every row of A and B starts on a 16-byte boundary (the launcher's)
    int precision = 0;               // ntx_precision: NTX_PRECISION_F32 (the f32 MFMA body) or NTX_PRECISION_BF16X6 (ntx_gemm_bf16x6.hip), same contract
};
// n_split = 1: the whole of K in one range (k_chunk = K); more: the dW form, the caller's k_chunk and split_stride.  Any M: 65 535 row tiles a launch
void launch_gemm(hipStream_t st, bool a_kcontig, GemmArgs g, int n_split = 1);
// ntx_trainer.hip: out[e] = sum_z partial[z][e] (+ the second half of a bias's pair), z ascending: the fixed order that makes a step
// reproducible.  Several results in one launch; a job's elements are numbered from first (multiples of 256: a block belongs to one job)
constexpr int MAX_REDUCE_BATCH = 32;
struct ReduceJob { const float *partial; int n_split; long long stride, count, pair; float *out; long long first; };   // pair > 0: element e of a split is partial[e] + partial[pair + e]
struct ReduceBatch { ReduceJob job[MAX_REDUCE_BATCH]; int n; };
void launch_reduce(hipStream_t st, const ReduceBatch &b);
// ntx_backend_flex.hip: the two folds behind the gradient at the encoded inputs (flex_param_fold_kernel + flex_param_rows_kernel;
// flex_ray_fold_kernel), for both backends.  pg_geo / pg_app: the gradient at the geometry / appearance parameter features of every sample, rows
// of ld_geo / ld_app floats; ig_pos / ig_dir: at the FF(xyz) / FF(dir) rows
void launch_param_fold(hipStream_t st, const StepRays &r, const float *pg_geo, const float *pg_app, int ld_geo, int ld_app, float *ray_pg, int P, float *param_grad);
void launch_ray_fold(hipStream_t st, const StepRays &r, const float *ig_pos, const float *ig_dir, int ld_pos, int ld_dir, const float *dgrad, const float *sigma,
                     const float *noise, float *d_rays_o, float *d_rays_d);
// ... and the two per-sample folds of an instanced step (flex_param_samples_kernel -> out [N][S][P]; flex_input_samples_kernel -> d_pts,
// d_dirs [N][S][3]): the same rows, read at row_of[m]
void launch_param_samples(hipStream_t st, const StepSamples &s, const float *pg_geo, const float *pg_app, int ld_geo, int ld_app, int P, float *out);
void launch_input_samples(hipStream_t st, const StepSamples &s, const float *ig_pos, const float *ig_dir, int ld_pos, int ld_dir, float *d_pts, float *d_dirs);
inline int pad4(int n) { return (n + 3) & ~3; }      // a row of n floats padded to 16 bytes
__device__ __forceinline__ float wave_sumf(float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
}   // namespace ntx_train
