/*
 * nerftex.h -- C ABI of libnerftex_hip.so: the MI355X (gfx950) implementation of NeRF-Tex's
 * volumetric render path.
 *
 * This is the drop-in boundary of the project.  The reference
 * (hbaatz/nerf-tex) has no FFI of its own on this path -- it is eager TensorFlow called through
 * Python objects -- so the entry points below are what a binding for each reference function would
 * bind.  Each one cites the reference interface it replaces (file:line in /root/reference).
 *
 * Conventions
 *   - plain C, `extern "C"`, no torch / TF / C++ types in any signature;
 *   - every `float*` marked DEVICE is a caller-owned device pointer (row-major float32, last
 *     dimension fastest, exactly the layouts of the reference tensors); HOST pointers are read
 *     synchronously during the call;
 *   - the library owns only what `ntx_create` / `ntx_reserve` / `ntx_comm_create` / `ntx_instancer_create` /
 *     `ntx_instancer_reserve` / `ntx_instancer_set_mesh` allocate (the packed weight image, the hit-list scratch, the communicator,
 *     the instance matrices and the instancer's hit lists); no other entry point allocates or frees device memory;
 *   - every entry point is asynchronous on `stream` (a `hipStream_t` passed as `void*`; NULL = the
 *     null stream) and returns an `ntx_status` (0 = ok, negative = error).  The message of the
 *     last error on the calling thread is returned by `ntx_last_error()`.  An entry that takes a `stream` touches no stream but
 *     that one and waits for nothing -- its launches, memsets and copies are all queued on `stream` -- so callers may use
 *     non-blocking streams and order handles against each other with events (tests/test_gpu_streams.py).  The entries that wait, and
 *     for what ("device": every stream of the device; "stream": the `stream` they were given, once; "setup": creation and setup
 *     entries -- they allocate, upload with blocking copies behind the null stream's work, and a free waits for the device; call
 *     them before the work they configure, or after it has completed).  synchronisation table:
 *         ntx_reserve                            device
 *         ntx_set_weights                        device
 *         ntx_trainer_get                        device
 *         ntx_trainer_set                        device
 *         ntx_trainer_set_weights                device
 *         ntx_trainer_activation                 device
 *         ntx_train_forward_instanced            stream
 *         ntx_create                             setup
 *         ntx_destroy                            setup
 *         ntx_comm_create                        setup
 *         ntx_comm_destroy                       setup
 *         ntx_trainer_create                     setup
 *         ntx_trainer_create_flex                setup
 *         ntx_trainer_create_flex_ex             setup
 *         ntx_trainer_destroy                    setup
 *         ntx_trainer_enable_param_gradients     setup
 *         ntx_trainer_enable_input_gradients     setup
 *         ntx_trainer_enable_gradients           setup
 *         ntx_trainer_enable_instanced           setup
 *         ntx_instancer_create                   setup
 *         ntx_instancer_destroy                  setup
 *         ntx_instancer_reserve                  setup
 *         ntx_instancer_set_mesh                 setup
 *         ntx_instancer_set_meshes               setup
 *         ntx_instancer_set_parameter_textures   setup
 *         ntx_instancer_set_mesh_textures        setup
 *     end of table.  The first ntx_set_weights_device of a context also uploads its gather tables with blocking copies (behind the
 *     null stream's work) before it queues its kernel on `stream`; every later call only queues;
 *   - a context belongs to one device; calls on one context are not re-entrant.  Multi-GPU =
 *     one context (and one process) per device.
 */
#ifndef NERFTEX_H
#define NERFTEX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTX_ABI_VERSION 7

typedef struct ntx_ctx ntx_ctx;
typedef void *ntx_stream; /* hipStream_t */

typedef enum ntx_status {
    NTX_OK = 0,
    NTX_E_INVALID = -1,     /* bad argument (NULL pointer, negative size, n_samples < 2 ...) */
    NTX_E_UNSUPPORTED = -2, /* model architecture outside what the HIP kernels are built for */
    NTX_E_HIP = -3,         /* a HIP runtime call failed; ntx_last_error() carries hipGetErrorString */
    NTX_E_NODEVICE = -4     /* no usable gfx950 device */
} ntx_status;

/* Model architecture = the kwargs of network.model.ParamNerf (model.py:58) / Nerf (model.py:9). */
typedef enum ntx_model_kind {
    NTX_MODEL_PARAMNERF = 0,
    NTX_MODEL_NERF = 1,
    NTX_MODEL_PARAMNERF_EX = 2   /* a ParamNerf whose descriptor is the extended struct ntx_model_desc_ex below: param_depth > 0 */
} ntx_model_kind;
/* layer.FourierFeatures (layer.py:8-23) / layer.IntegratedPositionalEncoding (layer.py:25-41) */
typedef enum ntx_pos_encoding { NTX_POS_FOURIER = 0, NTX_POS_IPE = 1 } ntx_pos_encoding;

/* Built: ParamNerf with n_parameters = [g, a], g <= 4, a <= 8 (tuned kernel families for the shipped configs [1,6], [1,4], [2,3];
 * every other combination runs on one generic family whose rows for the absent parameters are zero, ~2 % more matrix work),
 * plain Nerf, and one IntegratedPositionalEncoding family [1,3] -- these at the architecture every reference config uses: depth 8,
 * width 256, skips [4], color_depth 1.  Any OTHER architecture of model.py:58 / :9 with FourierFeatures embeddings -- depth 1..24,
 * width 2..256, color_depth 0..4, any skips below depth-1 -- runs on the "flex" family: the same MFMA segments in a loop over layers
 * (narrower layers zero-padded to 256), float32 only (NTX_FLAG_FP16X3: NTX_E_UNSUPPORTED), nothing hoisted per ray; param_depth 1..4
 * through the extended descriptor below (ntx_model_desc_ex).  n_freq_bands (layer.py:11) up to 10 / 4 / 4 for position / direction /
 * parameters, every family and precision: the kernels evaluate their 10 / 4 / 4 bands, the ones a model does not have meet zero weight
 * rows (exact).  No embedding_config.  Anything else: NTX_E_UNSUPPORTED. */
#define NTX_SKIP_MASK 0x40000000   /* ntx_model_desc.skip = NTX_SKIP_MASK | mask: several skip layers (bit i: i in skips) */
typedef struct ntx_model_desc {
    int32_t kind;        /* ntx_model_kind */
    int32_t n_geo;       /* n_parameters[0]: parameters concatenated to the position embedding (model.py:88-93) */
    int32_t n_app;       /* n_parameters[1]: parameters concatenated to the direction embedding (model.py:96-101) */
    int32_t n_pos;       /* 3 */
    int32_t pos_freq;    /* pos_embedding.n_freq_bands   (layer.py:11): 0..10 */
    int32_t dir_freq;    /* dir_embedding.n_freq_bands: 0..4 */
    int32_t param_freq;  /* param_embedding.n_freq_bands: 0..4 */
    int32_t depth;       /* 8; flex family: 1..24 */
    int32_t width;       /* 256; flex family: 2..256 */
    int32_t skip;        /* `skips`: the index of the single skip layer, 4 (model.py:107-108); -1 = none; or NTX_SKIP_MASK | (bit i set for
                          * every i in skips) */
    int32_t color_depth; /* ParamNerf: 1 (model.py:118), flex family: 0..4; ignored for Nerf */
    int32_t pos_encoding;/* ntx_pos_encoding of pos_embedding: FourierFeatures (n_pos 3) or IntegratedPositionalEncoding (n_pos 6) */
} ntx_model_desc;

/* kind == NTX_MODEL_PARAMNERF_EX: the pointer every entry point takes as `const ntx_model_desc *` points to one of these.
 * param_depth Dense(param_width, relu) layers shape the Fourier features of the geometry parameters and, separately, of the
 * appearance parameters before they are concatenated to pos_map / dir_map (model.py:88-101).  Built: param_depth 1..4,
 * param_width 2..128, on the flex family's float32 kernels (any depth / width / skips / color_depth it takes).  param_depth = 0
 * is the plain ParamNerf. */
typedef struct ntx_model_desc_ex {
    ntx_model_desc base;     /* base.kind = NTX_MODEL_PARAMNERF_EX */
    int32_t param_depth;
    int32_t param_width;
    int32_t reserved[6];     /* 0 */
} ntx_model_desc_ex;

/* flags of ntx_composite / ntx_render_rays */
#define NTX_FLAG_MAP_EXR 1u         /* renderer.py:182-184: colour = elu(raw)+1 instead of sigmoid  */
#define NTX_FLAG_COMPOSITE_BKGD 2u  /* renderer.py:210-211 and 85-86: add (1-A)*bkgd; culled rays = bkgd */
#define NTX_FLAG_CHECK_NUMERICS 4u  /* renderer.py:140-141: set *status_flag |= 1 on NaN/Inf outputs */
#define NTX_FLAG_FP16X3 8u          /* this call uses NTX_PRECISION_FP16X3 (below) instead of float32 Dense layers */
#define NTX_FLAG_PERTURB 16u        /* ntx_render_rays: stratified jitter of the sample depths (renderer.py:106-111), see there */
#define NTX_FLAG_RAW_NOISE 32u      /* ABI v3: sigma += N(0, raw_noise_std) per sample before the relu (renderer.py:190-192, 335-337); ntx_render_opts */

/* ABI v3: optional extras of ntx_render_rays / ntx_render_instanced / ntx_sample_depths / ntx_sample_pdf (HOST struct, read during
 * the call; NULL = all defaults).  `size` = sizeof(ntx_render_opts) of the caller's header, so that later versions can append.
 *   raw_noise_std  with NTX_FLAG_RAW_NOISE: the density regulariser of map_model_output (renderer.py:190-192; InstanceRenderer
 *                  :335-337).  The draw for (ray, sample) is the first output of tf.random.normal's Box-Muller transform
 *                  (u1 clamped to 1e-7; sqrt(-2 ln u1) sin(2 pi u2)) of words 0 and 1 of Philox4x32-10 at counter
 *                  (sample index, ray index lo, ray index hi, 1) under the call's seed: a pure function of (seed, ray, sample) like
 *                  the jitter (whose counter ends in 0).  TensorFlow's own stream cannot be reproduced; the distribution is the same.
 *   noise_seed     the seed of ntx_render_instanced, which has no perturb_seed (the others key the noise with perturb_seed).
 *   ray_index0, ray_run_length, ray_run_stride
 *                  the index that keys both generators: local ray k of the call counts as ray
 *                      ray_index0 + (k / ray_run_length) * ray_run_stride + k % ray_run_length
 *                  -- the pixel-set arithmetic of ntx_generate_rays_strided.  All zero = k itself.  A caller that renders an
 *                  image in chunks passes the chunk's first ray as ray_index0; rank r of a shard map passes its pixel set
 *                  (r * run_length, run_length, n_ranks * run_length): the image then does not depend on how it was split. */
typedef struct ntx_render_opts {
    uint32_t size;                       /* sizeof(ntx_render_opts) of the caller's header: >= NTX_RENDER_OPTS_V3_SIZE; fields beyond `size` read as 0 */
    float raw_noise_std;
    uint64_t noise_seed;
    int64_t ray_index0, ray_run_length, ray_run_stride;
    uint32_t flags;                      /* ABI v6: NTX_OPT_* */
    uint32_t reserved;
} ntx_render_opts;
#define NTX_RENDER_OPTS_V3_SIZE 40u
/* ntx_instancer_model_input: the rows of its [N,S,...] outputs behind a ray's last marching step -- dists == 0 there, and it is written in
 * full -- are left UNWRITTEN in the other six (rays_d_map, pts, t, alpha_weight, instance_id, params_map) instead of holding the defaults
 * of instancer.pyx:41-50.  For callers that hand the buffers to ntx_render_instanced, which reads a row of those only where dists > 0
 * (renderer.py:284-288): three quarters of the bytes of a carpet frame are such defaults. */
#define NTX_OPT_INSTANCER_SPARSE 1u

/* Arithmetic of the Dense layers inside ntx_render_rays, ntx_render_instanced and ntx_mlp_forward (everything else -- encoders, heads,
 * compositing -- is float32 either way).  The reference computes in float32 (TensorFlow's default dtype, model.py:104-123):
 *   NTX_PRECISION_F32    float32 matrix cores (v_mfma_f32_32x32x2_f32), the default; 1.7e-6 from the float32 reference.
 *   NTX_PRECISION_FP16X3 opt-in: weights and activations split as v = hi + lo (two IEEE halves, round to nearest even,
 *                        subnormals kept) and multiplied as hi*hi + hi*lo + lo*hi on the 16-bit matrix cores
 *                        (v_mfma_f32_32x32x16_f16) with float32 accumulation.  hi + lo carries 22 mantissa bits and a
 *                        product of two halves is exact in float32, so only the lo*lo term and the rounding of lo are lost,
 *                        ~2^-22 relative per product: 2.8e-6 from the float32 kernel on the bench image, ~2.8x faster.  Not
 *                        bit-identical to NTX_PRECISION_F32.  Range: |activation| and |weight| <= 65504, beyond that the
 *                        sample becomes inf/NaN (reported through NTX_FLAG_CHECK_NUMERICS).  Every family and all three
 *                        entry points.
 *   NTX_PRECISION_BF16X6 opt-in, TRAINING only (ntx_trainer_set_precision below; no render entry takes it): the contractions of the
 *                        layer-by-layer training step with both operands split as v = v0 + v1 + v2, v0 = bf16(v), v1 = bf16(v - v0),
 *                        v2 = bf16(v - v0 - v1) (round to nearest even, the subtractions in float32) and the six products of order
 *                        <= 2 -- a0b2, a1b1, a2b0, a0b1, a1b0, then a0b0 -- taken on the 16-bit matrix cores
 *                        (v_mfma_f32_32x32x16_bf16) into float32, smallest first.  The three terms carry 24 mantissa bits and bf16
 *                        has float32's exponent range, so the result is at or below float32's own rounding error at every scale of
 *                        the operands (the cotangents of a mean loss, 1e-6 .. 1e-9 a sample, included -- which is why fp16x3 cannot
 *                        train): no loss scaling, no amax pass.  Operands, weights, Adam and every other kernel stay float32.  Not
 *                        bit-identical to NTX_PRECISION_F32.  An Inf operand may come out as NaN in its row (inf - inf in the
 *                        split); a finite |v| beyond bf16's largest finite value (3.39e38) turns Inf. */
typedef enum ntx_precision { NTX_PRECISION_F32 = 0, NTX_PRECISION_FP16X3 = 1, NTX_PRECISION_BF16X6 = 2 } ntx_precision;
/* The precision is chosen PER CALL with NTX_FLAG_FP16X3 in `flags`; a context holds both weight images and no mutable
 * precision state, so two callers may share a context on different precisions. */

int ntx_abi_version(void);
const char *ntx_last_error(void);

/* Number of float32 in the reference-layout weight blob of `desc`:
 *   np.concatenate([w.ravel() for w in keras_model.get_weights()])
 * i.e. per Dense layer kernel[in,out] (row-major) then bias[out], in the order of `keras_model.layers`.  A functional
 * tf.keras.Model sorts its layers by graph depth (ties: traversal order from outputs=[color, alpha], model.py:125), NOT
 * by creation, so the order is
 *   trunk 0..7 (model.py:105-106) | feature (:114) | colour layers (:118-119, ParamNerf) | colour half (:122) | color (:123) | alpha (:111)
 * -- the alpha head comes LAST although it is created before the feature layer (the same order as the
 * `layer_with_weights-k` keys of the checkpoints logger.py:30-39 writes).  Every layer has a distinct position, so a blob in
 * another order has the right size and cannot be detected here; the Python mirror's `set_weights(list)` checks shapes.
 * Returns 0 if `desc` is not supported. */
size_t ntx_weight_count(const ntx_model_desc *desc);

/* Replaces: building the tf.keras.Model (model.py:125) + tf.train.Checkpoint restore (logger.py:33-39).
 * Packs the HOST blob into the MFMA operand layout and uploads it to `device`. */
int ntx_create(const ntx_model_desc *desc, const float *weights_host, size_t n_floats, int device,
               ntx_ctx **out);
/* Re-pack and re-upload new weights into an existing context.  Synchronous: it waits for all work on the context's device, on every
 * stream -- a launch in flight reads the old weights to its end -- and it has returned only once the upload is complete: every launch
 * made after it, on any stream, reads the new ones. */
int ntx_set_weights(ntx_ctx *ctx, const float *weights_host, size_t n_floats);
int ntx_destroy(ntx_ctx *ctx);

/* Setup-time sizing of the context's device scratch (synchronous; frees and re-allocates): after ntx_reserve(ctx, n),
 * ntx_render_rays / ntx_render_instanced accept up to n rays per call and allocate nothing.  Scratch = 8 B per ray (the
 * compacted list of rays that hit the proxy, renderer.py:58-67; the cost-ordered ray list of the instanced kernels).
 * ntx_create reserves NTX_DEFAULT_MAX_RAYS; a call with more rays than reserved fails with NTX_E_INVALID and renders
 * nothing. */
#define NTX_DEFAULT_MAX_RAYS (1 << 20)
int ntx_reserve(ntx_ctx *ctx, int64_t max_rays);

/* Replaces pixel_sampler.Full (pixel_sampler.py:14-15) + ray_sampler.rays_from_camera
 * (ray_sampler.py:39-48) + ray_sampler.Proxy (32-37) with proxy.AABB (proxy.py:13-35) [mode 0]
 * or ray_sampler.Frustum (15-21) [mode 1], for pixels [pixel0, pixel0+n_pixels) of the row-major
 * H x W grid.  c2w: HOST float[16] row-major 4x4.  b0/b1: HOST float[3] (mode 0).
 * Outputs (DEVICE): rays_o[n,3], rays_d[n,3], t[n,2], cone_scale[n,1]. */
int ntx_generate_rays(const float *c2w, int height, int width, float focal, int64_t pixel0,
                      int64_t n_pixels, int mode, const float *b0, const float *b1, float near_t,
                      float far_t, float *rays_o, float *rays_d, float *t, float *cone_scale,
                      ntx_stream stream);
/* The same for ANY set of image-plane locations -- ray_sampler.rays_from_camera (ray_sampler.py:39-48) as Proxy / Frustum call it
 * with whatever the pixel sampler returned (pixel_sampler.py: Full, Independent, Proxy): image_plane_loc DEVICE float32 [n,2] =
 * (row, col) per ray, the tensor the reference casts to float32 (:25, :17).  Outputs as above. */
int ntx_generate_rays_at(const float *c2w, int height, int width, float focal, const float *image_plane_loc, int64_t n_rays, int mode,
                         const float *b0, const float *b1, float near_t, float far_t, float *rays_o, float *rays_d, float *t,
                         float *cone_scale, ntx_stream stream);
/* Replaces proxy.AABB.__call__ (proxy.py:13-35) on the caller's own rays: rays_o, rays_d DEVICE [n,3] -> t DEVICE [n,2],
 * [inf, inf] on a miss; 1/0 and 0*inf follow IEEE as in the reference.  b0, b1: HOST float[3]. */
int ntx_aabb_intersect(const float *rays_o, const float *rays_d, int64_t n_rays, const float *b0, const float *b1, float *t,
                       ntx_stream stream);
/* Same for a STRIDED set of pixels, the local rays of one rank of a shard map (see ntx_shard_count): local ray k is
 * pixel pixel0 + (k / run_length) * run_stride + k % run_length.  rank r of R: pixel0 = r * run_length,
 * run_stride = R * run_length, n_pixels = ntx_shard_count(H * W, run_length, R, r). */
int ntx_generate_rays_strided(const float *c2w, int height, int width, float focal, int64_t pixel0, int64_t n_pixels,
                              int64_t run_length, int64_t run_stride, int mode, const float *b0, const float *b1,
                              float near_t, float far_t, float *rays_o, float *rays_d, float *t, float *cone_scale,
                              ntx_stream stream);

/* Replaces layer.FourierFeatures.call (layer.py:22-23): x[M,D] -> out[M, D*(1+2*n_freq)] (DEVICE).  n_freq 0..30, any x: every
 * sin / cos is within 2.5e-7 of the exact value at the float32 argument 2^k x (the library sine where |2^k x| >= 2^17); inf / NaN
 * give NaN features of that component.
 * The encoders FUSED into the network kernels (ntx_mlp_forward, ntx_render_rays, ntx_render_instanced, the training step) evaluate the
 * fast sine alone, which holds its 1.5 ulp on |2^f x| < 2^17: positions |pos| < 256 at pos_freq 10.  Beyond that domain the fused
 * features lose accuracy (6e-7 at 2^20, not a sine from 2^24 on). */
int ntx_fourier_features(const float *x, int64_t m, int d, int n_freq, float *out, ntx_stream stream);

/* Replaces model((pos, dirs, params), training) (renderer.py:161; model.py:58-125):
 * pos[M,3], dirs[M,3], params[M,P] -> color[M,3] (raw), sigma[M] (raw alpha head).  All DEVICE. */
int ntx_mlp_forward(ntx_ctx *ctx, const float *pos, const float *dirs, const float *params, int64_t m,
                    uint32_t flags /* NTX_FLAG_FP16X3 or 0 */, float *color_out, float *sigma_out, ntx_stream stream);

/* Replaces Renderer.map_model_output (renderer.py:170-213): color[N,S,3], sigma[N,S], z[N,S],
 * rays_d[N,3] -> color_out[N,3], alpha_out[N], optional weights_out[N,S] (NULL to skip).
 * bkgd: HOST float[3].  A NaN density makes its ray's colour and alpha NaN, as tf.nn.relu propagates it (:195). */
int ntx_composite(const float *color, const float *sigma, const float *z_vals, const float *rays_d,
                  int64_t n_rays, int n_samples, uint32_t flags, const float *bkgd, float *color_out,
                  float *alpha_out, float *weights_out, ntx_stream stream);

/* Replaces the sample placement of Renderer.render_rays (renderer.py:101-111; MipRenderer :374-383) on its own:
 * z_out[N, n_points] (DEVICE) = t0 (1 - tv) + t1 tv over tv = tf.linspace(0, 1, n_points) evaluated in float32, and with
 * NTX_FLAG_PERTURB the stratified jitter z = lower + (upper - lower) * u of :106-111, u in [0,1) drawn by a counter-based
 * generator: word 0 of Philox4x32-10 at counter (sample index, ray index lo, ray index hi, 0) under the key
 * (perturb_seed lo, hi), low 23 bits as the float32 mantissa (tf.random.uniform's conversion).  The draw depends only on
 * (perturb_seed, ray index, sample index); the ray index is the index within the call unless `opts` maps it to a global one
 * (ntx_render_opts: chunks and shards of one image then draw what the whole image draws under one seed).
 * TensorFlow's own stream (its global generator) cannot be reproduced; the distribution is the same.  ntx_render_rays
 * places its samples with exactly this function. */
int ntx_sample_depths(const float *t, int64_t n_rays, int n_points, uint32_t flags, uint64_t perturb_seed,
                      const ntx_render_opts *opts /* ray index map; may be NULL */, float *z_out, ntx_stream stream);

/* ABI v5.  noise_out[n_rays, n_points] (DEVICE) = raw_noise_std * N(0,1): exactly the draws NTX_FLAG_RAW_NOISE adds to the density inside
 * ntx_render_rays / ntx_render_instanced (ntx_render_opts above: Philox counter (sample, ray index, 1) under `seed`, Box-Muller), as a
 * tensor -- what the reference's `tf.random.normal(alpha.shape) * raw_noise_std` is (renderer.py:190-192).  opts: raw_noise_std and the
 * ray index map.  The training step uses it (config_grass_filtered_train.py:99 trains with raw_noise_std 0.1). */
int ntx_sample_noise(int64_t n_rays, int n_points, uint64_t seed, const ntx_render_opts *opts, float *noise_out, ntx_stream stream);

/* Replaces Renderer.__call__ + render_rays + evaluate_model + map_model_output
 * (renderer.py:47-213) with n_importance=0, fused in one launch:
 * culling of t==inf rays, sample placement, positional encoding, the MLP and the composite.
 *   rays_o[N,3], rays_d[N,3], t[N,2], cone_scale[N] (DEVICE)
 *   params[n_param_rows, P] (DEVICE): ray r uses row r / rays_per_param_row (the reference's
 *       tf.repeat(parameters, HW), renderer.py:54); rays_per_param_row = 1 gives per-ray parameters
 *   blur_idx: -1 = off, else params[blur_idx] *= cone_scale * z per sample (renderer.py:155-158)
 *   flags: NTX_FLAG_MAP_EXR | NTX_FLAG_COMPOSITE_BKGD | NTX_FLAG_CHECK_NUMERICS | NTX_FLAG_FP16X3 | NTX_FLAG_PERTURB | NTX_FLAG_RAW_NOISE
 *   opts: NULL, or HOST ntx_render_opts: raw_noise_std (with NTX_FLAG_RAW_NOISE, keyed by perturb_seed) and the global ray index map
 *   z_vals: NULL, or DEVICE [N,S] sample depths replacing renderer.py:101-111 altogether (wins over NTX_FLAG_PERTURB)
 *   perturb_seed: key of the jitter under NTX_FLAG_PERTURB (renderer.py:106-111, the reference's default; see
 *       ntx_sample_depths), evaluated inside the kernel: no [N,S] tensor exists
 *   status_flag: NULL, or DEVICE int32 OR-ed with 1 when NTX_FLAG_CHECK_NUMERICS finds NaN/Inf
 * Outputs (DEVICE): color_out[N,3] (premultiplied), alpha_out[N]; culled rays get 0 (or bkgd);
 *   weights_out: NULL, or [N,S] the compositing weights of renderer.py:198 (input of sample_pdf; rows of
 *   culled rays are left untouched).
 * All arguments are validated before the first launch: a call that returns an error has written nothing.
 * Context scratch: the compacted list of hit rays, 4 B per ray, sized by ntx_reserve (N beyond it is an error; nothing is
 * allocated here).  The view direction and the appearance parameters are constant along a ray (renderer.py:152-154), so
 * for ParamNerf models the direction segment of the colour layer is evaluated once per ray inside the kernel (through
 * LDS, bit-identical to the per-sample evaluation) unless blur_idx scales an appearance parameter.  Calls on one context
 * must be stream-ordered. */
int ntx_render_rays(ntx_ctx *ctx, const float *rays_o, const float *rays_d, const float *t,
                    const float *params, int64_t rays_per_param_row, const float *cone_scale,
                    int64_t n_rays, int n_samples, int blur_idx, uint32_t flags, const float *bkgd,
                    const float *z_vals, uint64_t perturb_seed, const ntx_render_opts *opts, float *color_out,
                    float *alpha_out, float *weights_out, int32_t *status_flag, ntx_stream stream);

/* Replaces the importance-sampling step of Renderer.render_rays (renderer.py:125-130) incl. sample_pdf
 * (renderer.py:589-617): bins = midpoints of the coarse depths, pdf = weights[:,1:-1] + 1e-5, n_importance
 * depths by inverse CDF at u (NULL = tf.linspace(0,1,n_importance), the `det` branch; else DEVICE [N,n_imp]
 * uniform draws), merged with the coarse depths and sorted -> z_out[N, S + n_importance] (DEVICE).
 * The coarse depths are z_vals[N,S], or (NULL) recomputed from t exactly as ntx_render_rays places them under the same
 * `flags` (NTX_FLAG_PERTURB or 0), `perturb_seed` and ray index map. */
int ntx_sample_pdf(const float *t, const float *z_vals, const float *weights, const float *u, int64_t n_rays,
                   int n_samples, int n_importance, uint32_t flags, uint64_t perturb_seed,
                   const ntx_render_opts *opts /* ray index map; may be NULL */, float *z_out, ntx_stream stream);

/* Replaces InstanceRenderer.evaluate_model + map_model_output (renderer.py:247-354) DOWNSTREAM of the
 * instancer: the arguments are the buffers instancer.get_model_input returns (instancer.pyx:38-54), on the
 * device:  rays_d_map[N,S,3], pts[N,S,3], t[N,S], dists[N,S], color_last[N,3], alpha_last[N],
 * alpha_weight[N,S] (NULL = density_reweighting off), instance_id[N,S] int32, hit[N] uint8 (the rays in
 * `idxs`), params_map[N,S,P], cone_scale[N].  Samples with dists <= 0 are skipped (renderer.py:284-288);
 * sigma *= alpha_weight * density_scale (:300); alpha = 1 - exp(-relu(sigma) * dists / patch_scale) (:339);
 * one extra sample (color_last as is, alpha_last as an alpha) closes every ray (:331,339).
 * instance_color[n_instances,3] != NULL = the false-colour mode (:306-307).  Rays with hit == 0 get 0, also
 * under NTX_FLAG_COMPOSITE_BKGD (:313-314).  1 <= n_samples <= 4096.  flags: as ntx_render_rays without NTX_FLAG_PERTURB
 * (the instancer places the samples).  opts: NULL, or raw_noise_std + noise_seed (NTX_FLAG_RAW_NOISE, added to the scaled
 * density of the in-patch samples: at dists == 0 the reference's draw has no effect either) and the ray index map. */
int ntx_render_instanced(ntx_ctx *ctx, const float *rays_d_map, const float *pts, const float *t,
                         const float *dists, const float *color_last, const float *alpha_last,
                         const float *alpha_weight, const int32_t *instance_id, const uint8_t *hit,
                         const float *params_map, const float *cone_scale, int64_t n_rays, int n_samples,
                         int blur_idx, float patch_scale, float density_scale, uint32_t flags,
                         const float *bkgd, const float *instance_color, const ntx_render_opts *opts, float *color_out,
                         float *alpha_out, int32_t *status_flag, ntx_stream stream);

/* Replaces the image post-processing of logger.Logger.render_image / write_image (logger.py:128-144) and
 * util.interpolate.filtered_downsample (interpolate.py:68-82): rgba[H,W,4] premultiplied (DEVICE) ->
 * optional gaussian low-pass (size 3*factor, std factor/2) + stride-`factor` downsample with TF 'SAME' padding,
 * optional rgb / (a + 1e-5), written as float32 out_f32[ceil(H/f),ceil(W/f),4] and/or uint8 out_u8 (saturating
 * x*255.5, what tf.image.convert_image_dtype does before encode_png).  Either output may be NULL. */
int ntx_image_epilogue(const float *rgba, int height, int width, int downsampling_factor, int unpremultiply,
                       float *out_f32, uint8_t *out_u8, ntx_stream stream);

/* ---- multi-GPU: rays shard embarrassingly, the ONE collective is the gather of the finished RGBA --------------
 * The reference has no distribution; Renderer.__call__ already renders chunks of rays independently (renderer.py:72-73).
 * Shard map (ntx_shard_*): the row-major pixel sequence [0, n_pixels) (pixel_sampler.py:14-15) is cut into RUNS of
 * `run_length` consecutive pixels (the last one may be shorter); run q belongs to rank q % n_ranks and is that rank's
 * local run q / n_ranks.  run_length = ceil(n_pixels / n_ranks) gives contiguous bands; run_length = image width deals
 * rows round-robin, which balances the rays the proxy culls (renderer.py:58-67) across ranks. */
int64_t ntx_shard_count(int64_t n_pixels, int64_t run_length, int n_ranks, int rank);   /* pixels of `rank`, -1 on bad arguments */

/* One communicator per process/device over RCCL (librccl is dlopen-ed on first use: the copy PyTorch already loaded if
 * there is one).  ntx_comm_unique_id wraps ncclGetUniqueId (rank 0 calls it and hands the 128 bytes to its peers by any
 * host-side means); ntx_comm_create wraps ncclCommInitRank on `device`; all ranks call it collectively. */
typedef struct ntx_comm ntx_comm;
#define NTX_COMM_ID_BYTES 128
/* ABI v3.  ntx_comm_preflight: everything of ntx_comm_create that can fail WITHOUT a peer (librccl loadable with every symbol,
 * `device` valid), so that ranks can agree to go ahead before any of them blocks in ncclCommInitRank.  ntx_comm_library: path of the
 * librccl the symbols were bound from ("" = none). */
int ntx_comm_preflight(int device);
const char *ntx_comm_library(void);
int ntx_comm_unique_id(uint8_t *id_out /* HOST [NTX_COMM_ID_BYTES] */);
int ntx_comm_create(const uint8_t *id /* HOST [NTX_COMM_ID_BYTES] */, int n_ranks, int rank, int device, ntx_comm **out);
int ntx_comm_destroy(ntx_comm *comm);

/* Replaces nothing in the reference (single device); it is the `tf.concat` of the chunk results (renderer.py:76-79)
 * across devices.  Every rank passes its local premultiplied RGBA, local_rgba[ntx_shard_count(...), 4] (DEVICE), in local
 * ray order; `root` receives the whole image image_out[n_pixels, 4] (DEVICE) in pixel order.  One ncclGather
 * (rccl.h:745) on `stream` when every rank holds the same number of pixels -- each peer sends straight to the root over its own xGMI
 * link -- else the same exchange as grouped ncclSend/ncclRecv with the exact counts.  staging (root only, DEVICE, may be
 * NULL when run_length == ceil(n_pixels / n_ranks) and the counts are equal: the gather then lands in image_out
 * directly): n_ranks * max-count * 4 floats, from which a kernel deals the runs back into pixel order.
 * image_out / staging are ignored on the other ranks. */
int ntx_gather_image(ntx_comm *comm, const float *local_rgba, int64_t n_pixels, int64_t run_length, float *image_out,
                     float *staging, int root, ntx_stream stream);
/* ABI v7.  The same with flags.  NTX_GATHER_FORCE_EXCHANGE: take the exact-count branch whatever the counts are -- grouped
 * ncclSend / ncclRecv into `staging` (required on the root), then the un-shard pass -- and send the root's own block to itself too
 * instead of copying it: a communicator of ONE rank then executes every RCCL call of the branch that uneven shards take on eight
 * (tests; a box with one GPU).  ntx_comm_version: ncclGetVersion of the bound librccl (0 = none). */
#define NTX_GATHER_FORCE_EXCHANGE 1u
int ntx_gather_image_ex(ntx_comm *comm, const float *local_rgba, int64_t n_pixels, int64_t run_length, float *image_out,
                        float *staging, int root, uint32_t flags, ntx_stream stream);
int ntx_comm_version(void);

/* ABI v5.  values[n] (DEVICE) <- the mean over all ranks of their values[n], in place, on `stream`: one ncclAllReduce (rccl.h) and a scale.
 * The one collective of data-parallel TRAINING (the reference trains on one device: train.py:61-67): ranks take the same step on different
 * rays, the loss is a mean over rays, so the full batch's gradient is the mean of the shards' (equal shard sizes).  ntx_comm_size: n_ranks. */
int ntx_comm_size(const ntx_comm *comm);
int ntx_allreduce_mean_f32(ntx_comm *comm, float *values, size_t n, ntx_stream stream);

/* ABI v3, host only (no device, no communicator): the exchange ntx_gather_image performs for a shard map, as numbers -- rank r
 * holds counts_out[r] pixels and its block starts at pixel slot offsets_out[r] of the destination; *equal_out = one ncclGather
 * (else grouped Send/Recv with the exact counts); *direct_out = the destination is image_out itself (else `staging`, followed by
 * the un-shard pass).  ntx_unshard_map: src_out[p] = the staging pixel slot that holds pixel p (what the un-shard kernel reads).
 * Both run the very code of the device path (csrc/ntx_shard.h), so CPU tests can execute the plan through another transport. */
int ntx_gather_plan(int64_t n_pixels, int64_t run_length, int n_ranks, int64_t *counts_out /* [n_ranks] or NULL */,
                    int64_t *offsets_out /* [n_ranks] or NULL */, int *equal_out, int *direct_out);
int ntx_unshard_map(int64_t n_pixels, int64_t run_length, int n_ranks, int64_t *src_out /* HOST [n_pixels] */);

/* Introspection for benches/tests: name and launch geometry of the fused kernel in `ctx`. */
int ntx_kernel_info(ntx_ctx *ctx, int *n_workgroups, int *threads_per_workgroup, int *n_cus);

/* Host-only helpers (no device needed) exposing the weight packing, so it can be checked on CPU:
 * number of floats of the packed image, and the packing itself. */
size_t ntx_packed_count(const ntx_model_desc *desc);
int ntx_pack_weights(const ntx_model_desc *desc, const float *weights_host, size_t n_floats,
                     float *packed_out, size_t n_packed);

/* Same for the fp16x3 weight stream: its size in bytes (0 + error for families without one) and the packing. */
size_t ntx_packed_fp16x3_bytes(const ntx_model_desc *desc);
int ntx_pack_weights_fp16x3(const ntx_model_desc *desc, const float *weights_host, size_t n_floats,
                            uint16_t *packed_out, size_t n_bytes);

/* ---- ABI v4: the patch instancer (what feeds ntx_render_instanced) ---------------------------------------------------------
 * Replaces instancer.instancer.Instancer (instancer/instancer.pyx:6-54) = C_Instancer (instancer/src/instancer.hpp:10-89), the
 * reference's only native code: Embree 3 on one CPU thread.  Built here: the constructor with explicit `transformations`
 * (instancer.pyx:19-20 -> AddInstance, instancer.cpp:124-141), an instancer mesh given as arrays, GetNumberOfInstances (:426-428),
 * the matrices ExportTransformations writes (:1040-1061) and GetModelInput (:751-1037) with the three patch choices, mean
 * distances, directional and point lights, shadow rays (:591-602, 945-961, 1018-1027), auxiliary meshes with
 * their flat shading (:393-417, 716-743); since ABI v5 image textures, as parameters on the instancer mesh (:640-667) and as the
 * albedo of an auxiliary mesh (:725-733), see below.  DistributeInstancesOnMesh (:233-390) is setup on the host: its result is the
 * transformation list ntx_instancer_create takes (nerf_tex_amd.instancer.distribute_instances_on_mesh restates it; the reference
 * can also export its own with `transformation_export_path`).
 *
 * ntx_instancer_desc = the constructor arguments that survive (instancer.cpp:53-93): b_0 / b_1 the patch box in patch
 * coordinates; n_parameters, light_dir_parameter_idx, light_strength_parameter_idx as the `textures` list defines them
 * ("" = 1 parameter, "light" = 3 with light_dir at their start, "point" = 4: strength, then position = light_dir + 1;
 * -1 = none); instance_sample_method 0 random / 1 nearest / 2 nearest_blend (instancer.pyx:14); patch_scale only scales
 * nearest_blend's transition range (:697; 1 unless the patches were distributed on a mesh).  cast_shadow_rays (needs a light
 * entry): a sample whose shadow query is occluded gets the light direction (0, 0, -1) (:571-573).  A query (isShadowed, :591-602:
 * from the point along the light parameter AS GIVEN -- for 'point' that is the light's position, :956 -- with 0 < t <= 100) is
 * occluded by the top face of a patch box entered from outside, by its bottom face either way, by a mesh hit from its front and
 * by the triangle with primID 1 of any mesh from either side (filter :543-554: its `primID == 1` clause does not ask which geometry).  With N = max(min_shadow_samples, n_shadow_samples * total length) < n_pts the queries are
 * made at max(min_shadow_samples, N * length / total) points spaced evenly along every segment and a step takes the nearer of
 * the two around it (:946-958, 1018-1027), else every step makes its own (:959-961).  min_shadow_samples >= 2.
 * *status_flag |= 4 when a ray needed more than 4096 shadow samples (the rest read as unshadowed). */
typedef struct ntx_instancer ntx_instancer;
typedef struct ntx_instancer_desc {
    uint32_t size;                       /* sizeof(ntx_instancer_desc) */
    float b_0[3], b_1[3];
    int32_t n_parameters, light_dir_parameter_idx, light_strength_parameter_idx;
    int32_t instance_sample_method, use_mean_distance, cast_shadow_rays;
    float patch_scale;
    int32_t min_shadow_samples, n_shadow_samples;   /* with cast_shadow_rays (instancer.cpp:53, 861, 1019) */
} ntx_instancer_desc;
#define NTX_INSTANCER_DEFAULT_MAX_RAYS (1 << 16)
/* transformations: HOST [n_instances,4,4] row-major patch -> world, what AddInstance takes.  The instancer keeps, per instance,
 * the inverse (world -> patch), the direction map (columns of the 3x3 block, normalised) and the origin (instancer.cpp:127-132;
 * computed in double and rounded), plus hit-list workspace for NTX_INSTANCER_DEFAULT_MAX_RAYS rays (3.2 KB per ray). */
int ntx_instancer_create(const ntx_instancer_desc *desc, const float *transformations, int64_t n_instances, int device,
                         ntx_instancer **out);
int ntx_instancer_destroy(ntx_instancer *inst);
/* Workspace for calls of up to max_rays rays in one piece (<= 2^24); larger calls are cut into pieces of the reserved size. */
int ntx_instancer_reserve(ntx_instancer *inst, int64_t max_rays);
int64_t ntx_instancer_count(const ntx_instancer *inst);                       /* GetNumberOfInstances; -1 on NULL */
/* HOST outputs, each may be NULL: world_to_patch[K,4,4] (this->transformations; its inverses are what ExportTransformations
 * writes), directions[K,3,3] (dir_transformations), origins[K,3] (instance_origins). */
int ntx_instancer_matrices(const ntx_instancer *inst, float *world_to_patch, float *directions, float *origins);
/* The instancer mesh (instancer.cpp:369-389: in the scene for culling): HOST vertices[n_vertices,3], faces[n_faces,3].  A ray
 * ends at its closest crossing of the mesh and is closed by an opaque black sample (:1013-1016).  n_faces = 0 removes it. */
int ntx_instancer_set_mesh(ntx_instancer *inst, const float *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces);
/* The same with auxiliary meshes (AddMesh, instancer.cpp:393-417) in one list: face_kind[f] bit 0 = 0 for the instancer mesh (black closing
 * sample), 1 for an auxiliary mesh; bit 1 (value 2) = the face is primID 1 of its own mesh (the shadow filter's clause above; without
 * face_kind the list is one mesh and face 1 has it).  An auxiliary mesh's closing sample is shaded (shadeMesh, :716-743): albedo 0.8 * min(diffuse + 0.2, 1), diffuse =
 * max(n . l, 0) with the interpolated vertex normal n (normals[n_vertices,3], HOST) and the light parameter l, 0 when the point just
 * above the surface is shadowed (isShadowed).  Needs a light entry in the textures list; textures: ntx_instancer_set_mesh_textures.  Every mesh
 * culls and casts shadows alike.  normals / face_kind may be NULL (= ntx_instancer_set_mesh). */
int ntx_instancer_set_meshes(ntx_instancer *inst, const float *vertices, const float *normals, int64_t n_vertices, const int32_t *faces,
                             const uint8_t *face_kind, int64_t n_faces);
/* GetModelInput (instancer.cpp:751-1037) with the buffers of get_model_input (instancer.pyx:38-54), all DEVICE, every element of
 * every output written: rays_o[N,3], rays_d[N,3] (per ray; the reference's [N,S,3] input is this row repeated), parameters[N,P] ->
 * rays_d_map[N,S,3], pts[N,S,3], t[N,S], dists[N,S], color_last[N,3], alpha_last[N], alpha_weight[N,S] (density_weight),
 * instance_id[N,S], hit[N] uint8, params_map[N,S,P]: the argument list of ntx_render_instanced.  Per ray: face crossings of every
 * instanced box with 0 < t <= 100 (at most 200 kept, instancer.cpp:22), sorted by (t, instance); the union of the boxes is
 * marched in steps of step_size from a random offset; a sample takes the patch it lies in (several: by
 * instance_sample_method) and is mapped into it (point, direction, light direction / strength); samples behind the last
 * step keep the defaults of instancer.pyx:41-50.  The reference draws from one std::mt19937 in ray order (:855, 675, 710);
 * here the offset of a ray is U[0,1) from word 0 of Philox4x32-10 at counter (0, ray lo, ray hi, 2) under `seed`, the patch
 * choice of (ray, step) from counter (step, ray lo, ray hi, 3); `opts` carries the ray index map (as for ntx_render_rays;
 * NULL = the call's own indices), so chunked or sharded calls draw what the whole image draws.
 * An instancer belongs to one device and owns one workspace: calls on it must be stream-ordered (like a context's).
 * *status_flag (DEVICE, may be NULL) |= 1 when a ray had more than 200 face crossings (the rest were dropped, which ones is
 * unspecified -- as in the reference).  1 <= n_pts <= 4096. */
int ntx_instancer_model_input(ntx_instancer *inst, const float *rays_o, const float *rays_d, const float *parameters, int64_t n_rays,
                              int n_pts, float step_size, uint64_t seed, const ntx_render_opts *opts, float *rays_d_map, float *pts,
                              float *t, float *dists, float *color_last, float *alpha_last, float *alpha_weight,
                              int32_t *instance_id, uint8_t *hit, float *params_map, int32_t *status_flag, ntx_stream stream);

/* ---- ABI v5: image textures of the instancer --------------------------------------------------------------------------------
 * ntx_texture = ONE channel matrix as loadTexture builds it (instancer.cpp:34-50): value / 255, element (r, c) at texels[r * cols + c]
 * with r = the pixel's column x (rows = image width) and c = its row counted from the BOTTOM of the image (cols = image height);
 * HOST memory, copied.  Lookups are interpolate2d (:605-625): bilinear around x * (rows - 1, cols - 1), indices by truncation,
 * weights x - floor(x); an index outside the matrix is clamped (the reference reads past it; at u or v = 1 that weight is 0). */
typedef struct ntx_texture {
    const float *texels;
    int32_t rows, cols;
} ntx_texture;
/* Parameter textures (getParameters, instancer.cpp:640-667; the constructor's image entries, :84-88, after DistributeInstancesOnMesh
 * -- without a mesh_path the reference loads and counts them and never applies them, :911: then do not call this).  The instancer
 * mesh as the reference holds it: HOST vertices[n_vertices,3], uv[n_vertices,2], faces[n_faces,3].  Texture file i multiplies
 * parameter parameter_idx[i] by textures[i] at the texture coordinates of the closest point of the mesh (closest_point_triangle,
 * :154-198) strictly within patch_max_extent (:69 scaled by :246) of the sample; no triangle that close: unchanged.  The caller
 * resolves the reference's indexing: its list holds every CHANNEL of every file and file i uses entry i of that list (:656-662),
 * so a file of c channels takes c parameters and has one of them multiplied.  With N = max(min_texture_samples,
 * n_texture_samples * total length) < n_pts a ray looks the textures up at max(min_texture_samples, N * length / total) points
 * spaced evenly along every segment and a step's WHOLE parameter row is s0 * (1 - w) + s1 * w between the two around it (:910-923,
 * 989-998; the light entries are written afterwards); else every step makes its own lookup (:926).  At most 4 files;
 * 2 <= min_texture_samples <= 512.  n_textures = 0 removes them.  Of several triangles at one distance the lowest index wins
 * (Embree's order is its BVH's). */
int ntx_instancer_set_parameter_textures(ntx_instancer *inst, const float *vertices, const float *uv, int64_t n_vertices, const int32_t *faces,
                                         int64_t n_faces, float patch_max_extent, int n_textures, const int32_t *parameter_idx,
                                         const ntx_texture *textures, int min_texture_samples, int n_texture_samples);
/* Albedo textures of auxiliary meshes (AddMesh's texture_path, instancer.cpp:404; shadeMesh :725-733), after
 * ntx_instancer_set_meshes and for the same list: uv[n_vertices,2]; face_texture[n_faces] = the texture set of the face's mesh
 * or -1 (albedo 0.8); textures[3 * n_sets]: three channel matrices per set (an image that does not have exactly three channels
 * gives its first for all three, :732).  n_sets = 0 removes them. */
int ntx_instancer_set_mesh_textures(ntx_instancer *inst, const float *uv, int64_t n_vertices, const int32_t *face_texture, int64_t n_faces,
                                    int n_sets, const ntx_texture *textures);

/* ---- ABI v5: one training step (f6) ------------------------------------------------------------------------------------------
 * Replaces the body of the reference's training loop, network/train.py:61-67: `pred = renderer(**data)` under a GradientTape, a loss
 * of network/loss.py:6-59, `tape.gradient`, `optimizer.apply_gradients` with tf.keras.optimizers.Adam under ExponentialDecay
 * (train.py:49-52).  Built for the architecture of the shipped training configs: ParamNerf, depth 8, width 256, skips [4],
 * color_depth 1, Fourier features on n_pos 3 (any n_parameters, any band counts) or -- the MipRenderer's model -- NTX_POS_IPE on n_pos 6
 * (pos_map = 6 pos_freq + n_geo (1 + 2 param_freq) features; ntx_weight_count of the same descriptor); NTX_E_UNSUPPORTED otherwise
 * (ntx_trainer_create_flex below trains the other architectures, layer by layer).  An IPE
 * trainer has no importance pass: ntx_trainer_composite_weights refuses it (NTX_E_UNSUPPORTED), as the reference's MipRenderer refuses
 * n_importance > 0 (renderer.py:403-404).  The trainer owns the weights
 * (Keras get_weights() order, like ntx_create), Adam's moments, the gradient and every layer's activations for up to
 * max_rays x max_samples_per_ray samples (<= 1024 samples per ray; 23 KB per sample: 6 GB for the configs' 4 x 256 x 256; pos_map and
 * dir_map at most 96 features wide each).  Everything float32.  A step is bit-reproducible: weight gradients are summed over the samples
 * in a fixed order.  Against float64 autograd of the restated step (oracle/train_oracle.py, following the float32 pass's ReLU branches) every
 * layer's gradient, the loss and the predictions are within 1e-4 rel-Linf at the configs' batch; where a batch is ill-conditioned (a handful
 * of coarse steps per ray, depths a hair apart) within 4 times what float32 autograd of the same restatement is off by. */
typedef struct ntx_trainer ntx_trainer;
#define NTX_LOSS_NERF 0                  /* network.loss.NerfLoss  (loss.py:6-19):  loss_fn(color_true, color_pred) */
#define NTX_LOSS_ALPHA 1                 /* network.loss.AlphaLoss (loss.py:21-49): + gamma * alpha_loss_fn(alpha_true, alpha_pred), colours masked by alpha_true */
#define NTX_LOSS_MSE 0                   /* network.loss.mse   (loss.py:51-54) */
#define NTX_LOSS_SMAPE 1                 /* network.loss.smape (loss.py:56-59), eps = 1e-2 */
typedef struct ntx_loss_desc {
    uint32_t size;                       /* sizeof(ntx_loss_desc) */
    int32_t kind, loss_fn, alpha_loss_fn;
    float gamma;                         /* AlphaLoss: 1 */
    int32_t filter_color_loss, use_hard_mask;   /* AlphaLoss: True, True */
} ntx_loss_desc;
int ntx_trainer_create(const ntx_model_desc *desc, const float *weights_host, size_t n_floats, int device, int64_t max_rays, int max_samples_per_ray,
                       ntx_trainer **out);
int ntx_trainer_destroy(ntx_trainer *t);
size_t ntx_trainer_weight_count(const ntx_trainer *t);
#define NTX_TRAINER_WEIGHTS 0
#define NTX_TRAINER_GRADIENTS 1
#define NTX_TRAINER_ADAM_M 2
#define NTX_TRAINER_ADAM_V 3
/* Copies one of the trainer's weight-shaped vectors to HOST memory (Keras get_weights() order; synchronises the device). */
int ntx_trainer_get(ntx_trainer *t, int what, float *out_host, size_t n_floats);
int ntx_trainer_set_weights(ntx_trainer *t, const float *weights_host, size_t n_floats);
/* ... any of the four, from HOST memory (NTX_TRAINER_GRADIENTS: a gradient averaged over ranks by another transport than RCCL). */
int ntx_trainer_set(ntx_trainer *t, int what, const float *values_host, size_t n_floats);
/* Data-parallel training: every rank's gradient <- the mean over the ranks (ntx_allreduce_mean_f32 on the trainer's own buffer), between
 * ntx_train_step_gradients and ntx_trainer_adam_step; all ranks then take the same Adam step. */
int ntx_trainer_allreduce_gradients(ntx_trainer *t, ntx_comm *comm, ntx_stream stream);
/* The activations the last step kept, to HOST memory as [n_samples_total][width]: layer 0-7 = the trunk layers' outputs (after their ReLU),
 * 8 / 9 = the two colour layers' (width 256 / 128), 10 = the raw density (width 1), 11 = the raw colour (width 3).  Tests hand their signs to the float64 restatement, so
 * that its autograd follows the ReLU branches the float32 forward took (a pre-activation within rounding of zero can fall either way).
 * 20-27 = the GRADIENTS the last step kept at the trunk layers' outputs (behind their ReLU: what the layer's weight gradient contracts
 * with), 28 = at the first colour layer's output, 29 = at the feature layer's (all width 256): tests compare them row by row.
 * 30 = the composite's adjoint (width 4): dL/d raw colour, dL/d raw density per sample, where the way back starts. */
int ntx_trainer_activation(ntx_trainer *t, int layer, int64_t n_samples_total, float *out_host);
/* Forward (Renderer.__call__, renderer.py:47-213 -- a ray whose tnear_far is inf, i.e. that misses the proxy, stays in the batch and predicts
 * 0 / the background with alpha 0 as the reference's filter-and-scatter makes it, :58-86 -- : sample depths by ntx_sample_depths -- NTX_FLAG_PERTURB /
 * perturb_seed / opts as there -- or given as z_vals[N,S]; encodings; the network; map_model_output with NTX_FLAG_MAP_EXR /
 * NTX_FLAG_COMPOSITE_BKGD), the loss, and its gradient with respect to every weight, left in the trainer (ntx_trainer_get /
 * ntx_trainer_adam_step).  DEVICE: rays_o[N,3], rays_d[N,3], tnear_far[N,2] (or NULL with z_vals), params[rows,P] (ray r uses row
 * r / rays_per_param_row), cone_scale[N] (blur_idx >= 0), color_true[N,3], alpha_true[N] (AlphaLoss); outputs, each may be NULL:
 * color_pred[N,3], alpha_pred[N], loss_out[1].  bkgd: HOST [3] or NULL (white).
 * An IPE trainer follows MipRenderer.render_rays (renderer.py:365-473): n_samples = S cone segments between S + 1 depths --
 * ntx_sample_depths(n_points = S + 1) under the same flags and seed, or z_vals[N,S+1] -- each encoded by its gaussian (mean, diagonal
 * covariance) through the integrated positional encoding (layer.py:25-41); params[rows,P+1] hold the blur parameter at blur_idx (required,
 * 0 <= blur_idx <= P): times cone_scale it is the cone's radius, and the model sees the other P (column k < blur_idx ? k : k + 1); the
 * composite's dists are z[s+1] - z[s] with no copy of the last one. */
int ntx_train_step_gradients(ntx_trainer *t, const float *rays_o, const float *rays_d, const float *tnear_far, const float *params, int64_t rays_per_param_row,
                             const float *cone_scale, int64_t n_rays, int n_samples, int blur_idx, uint32_t flags, const float *bkgd, uint64_t perturb_seed,
                             const ntx_render_opts *opts, const float *z_vals, const float *color_true, const float *alpha_true, const ntx_loss_desc *loss,
                             float *color_pred, float *alpha_pred, float *loss_out, ntx_stream stream);
/* optimizer.apply_gradients (train.py:67): Adam (m += (g - m)(1 - beta_1); v += (g^2 - v)(1 - beta_2); w -= lr_t m / (sqrt(v) + epsilon),
 * lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t), t = iterations + 1: TF 2.4's ApplyAdam) with lr = lrate * lrate_decay_rate ^
 * (iterations / lrate_decay_steps) when lrate_decay_steps > 0 (ExponentialDecay, train.py:49-50: decay_steps = lrate_decay * 1e3,
 * decay_rate 0.1), else lrate.  Keras defaults: beta_1 0.9, beta_2 0.999, epsilon 1e-7.  Counts the iteration. */
int ntx_trainer_adam_step(ntx_trainer *t, float lrate, float lrate_decay_steps, float lrate_decay_rate, float beta_1, float beta_2, float epsilon,
                          ntx_stream stream);
int64_t ntx_trainer_iterations(const ntx_trainer *t);
/* ABI v6.  Resuming a run (train.py:55-60, logger.py:30-39: the reference checkpoints model + step + optimizer and continues with
 * `train_dataset.take(n_iters - logger.step)`): Adam's iteration count -- what its bias correction and the ExponentialDecay schedule run
 * on -- is set beside the weights and moments (ntx_trainer_set). */
int ntx_trainer_set_iterations(ntx_trainer *t, int64_t iterations);
/* ABI v6.  A coarse and a fine pass (renderer.py:125-138, loss.py:15-16, 41-47, model.py:47-56): the coarse step also leaves the composite's
 * weights a_i T_i -- what sample_pdf takes, with no gradient through it (:129) -- in weights_dev[N,S] (DEVICE; NULL: no more); ntx_sample_pdf
 * places the fine depths, a step with z_vals takes them.  When both passes run on ONE network (model_fine is None, :132) its gradient is the
 * sum of the two steps': op 0 keeps the gradient of the step just taken, op 1 adds it to the next one's. */
int ntx_trainer_composite_weights(ntx_trainer *t, float *weights_dev);
int ntx_trainer_stash_gradients(ntx_trainer *t, int op, ntx_stream stream);
/* ABI v6.  ntx_set_weights from DEVICE memory (the context's device; Keras get_weights() order), in the stream's order and without a
 * host copy: the float32 weight image is remade by one gather kernel.  The validation render inside the reference's training loop
 * (logger.py:76-81 from train.py:61-70) is this with the trainer's weights (ntx_trainer_device_weights).  The fp16x3 images are NOT
 * remade: NTX_FLAG_FP16X3 is refused (NTX_E_UNSUPPORTED) until the next ntx_set_weights. */
int ntx_set_weights_device(ntx_ctx *ctx, const float *weights_dev, size_t n_floats, ntx_stream stream);
/* The trainer's weights where they live: DEVICE memory of the trainer's device, Keras get_weights() order, ntx_trainer_weight_count floats,
 * valid until ntx_trainer_destroy; steps on a stream change them in that stream's order.  What ntx_set_weights_device takes. */
int ntx_trainer_device_weights(ntx_trainer *t, const float **weights_dev);
/* A dense contraction (f32 MFMA, 128 x 128 x 16 tiles through LDS) on DEVICE buffers, for tests and benches (round 4's trainer was made of it;
 * the step now runs on the chain and weight-gradient kernels of csrc/ntx_train_device.h):
 * C[M][N] = op(A) . op(B) (+ bias[N]) (ReLU); a_kcontig: A is [M][K] (row stride lda), else [K][M]; B is [K][N] (b_kcontig must be 0). */
int ntx_gemm_f32(const float *A, int lda, int a_kcontig, const float *B, int ldb, int b_kcontig, float *C, int ldc, int M, int N, int K, const float *bias,
                 int relu, ntx_stream stream);
/* The same contraction with the launcher's whole argument list (ABI v7, appended), for tests and benches of the kernel itself: what the
 * layer-by-layer training step passes it, on DEVICE buffers.  A, lda, a_kcontig, B [K][N], ldb, C, ldc, M, N, K, bias, relu as above.  The
 * epilogue, in this order: C[i][j] = acc (+ the C[i][j] found there, with accumulate) + bias[j]; ReLU; then, with mask (row stride ldmask),
 * 0 wherever !(mask[i][j] > 0).  n_split > 1 cuts K into ranges of k_chunk: range z covers p in [z k_chunk, min((z + 1) k_chunk, K)) and
 * writes its own product (epilogue included) to C + z split_stride; n_split = 1 is the whole of K, and k_chunk and split_stride are not
 * looked at.  colsum (NULL, or [n_split][N]; only with a_kcontig = 0, the weight-gradient form): colsum[z][j] = the sum of B[p][j] over range
 * z, in a fixed order.  NTX_E_INVALID, before anything is launched or written: a NULL A, B or C; M, N or K < 1; lda < K (a_kcontig) or < M,
 * ldb < N, ldc < N, mask with ldmask < N; n_split outside 1 .. 65535; with n_split > 1, k_chunk < 1, K outside ((n_split - 1) k_chunk,
 * n_split k_chunk] or split_stride < (M - 1) ldc + N; colsum with a_kcontig != 0. */
int ntx_gemm_f32_ex(const float *A, int lda, int a_kcontig, const float *B, int ldb, float *C, int ldc, int M, int N, int K, const float *bias, int relu,
                    const float *mask, int ldmask, int accumulate, int n_split, int k_chunk, int64_t split_stride, float *colsum, ntx_stream stream);
/* A trainer for any architecture the flex render family takes (ABI v7, appended): kind NTX_MODEL_NERF or NTX_MODEL_PARAMNERF, NTX_POS_FOURIER
 * on n_pos 3, depth 1..24, width 2..256, color_depth 0..4 (0 for a Nerf), skip = one index or NTX_SKIP_MASK | bits with every index below
 * depth - 1, n_geo <= 4, n_app <= 8, n_freq_bands <= 10 / 4 / 4 -- the 8 x 256 / skips [4] / color_depth 1 shape of ntx_trainer_create
 * included.  NTX_E_UNSUPPORTED, before any device is asked for: an IPE model, parameter branches (NTX_MODEL_PARAMNERF_EX with
 * param_depth > 0), a skip at depth - 1, width > 256; then NTX_E_INVALID for max_rays < 1, samples per ray outside 2..1024 or a wrong
 * n_floats.  The handle is an ordinary ntx_trainer: every ntx_trainer_* entry and ntx_train_step_gradients take it, with the same arguments,
 * options and meaning; weights, gradients and Adam's moments are in Keras get_weights() order.  The step behind it is one contraction per
 * Dense layer and pass (the float32 matrix-core kernel of ntx_gemm_f32) on row-major activations kept once each, the narrow heads on small
 * kernels of their own; weight gradients are partial sums over ranges of 2048 samples added in ascending order, so a step is
 * bit-reproducible and does not depend on the trainer's capacity.
 * ntx_trainer_activation on such a handle: layer k = 0 .. n_relu - 1 is the kept output of the k-th ReLU layer in the order trunk 0 ..
 * depth - 1, colour hidden layers, colour half layer, [n_samples_total][that layer's width]; 64 = the raw density [n_samples_total][1];
 * 65 = the raw colour [n_samples_total][3]. */
int ntx_trainer_create_flex(const ntx_model_desc *desc, const float *weights_host, size_t n_floats, int device, int64_t max_rays, int max_samples_per_ray,
                            ntx_trainer **out);
/* The same trainer for a ParamNerf WITH parameter branches (ABI v7, appended): desc->base.kind must be NTX_MODEL_PARAMNERF_EX; everything
 * ntx_trainer_create_flex takes for a ParamNerf, plus param_depth 0..4 and param_width 2..128 (the render side's limits).  A branch exists
 * only where its parameter count is > 0 (model.py:88, 96).  NTX_E_UNSUPPORTED, before any device is asked for: an IPE model, a skip at
 * depth - 1, width > 256, param_depth outside 0..4, param_width outside 2..128 when param_depth > 0; then NTX_E_INVALID as above.
 * ntx_trainer_create and ntx_trainer_create_flex keep refusing param_depth > 0.  The handle is an ordinary ntx_trainer; weights, gradients
 * and Adam's moments are in Keras get_weights() order, branch layers included (the geometry branch before the trunk, the appearance branch
 * among the trunk layers of its graph depth).  With param_depth = 0 the step is bit for bit ntx_trainer_create_flex's.
 * The step: the Fourier features of a branch's parameters go to that branch's own input rows, per sample (blur_idx on a geometry parameter
 * makes them differ from sample to sample); each branch layer is one contraction with ReLU, every output kept; the last output is copied
 * behind FF(pos) / FF(dir) into every buffer that starts with pos_map / dir_map.  On the way back every reader of a branch's output (trunk
 * layer 0 and the layers behind a skip; the first colour layer, or the colour half layer when color_depth = 0) adds dY . W[branch rows]^T
 * into the branch's gradient in descending layer order, masked by the branch's last ReLU, and the branch's layers follow like the trunk's.
 * A step stays bit-reproducible and independent of the trainer's capacity.
 * ntx_trainer_activation on such a handle: as ntx_trainer_create_flex's, and 32 + j = the kept output of geometry branch layer j, 48 + j =
 * that of appearance branch layer j, each [n_samples_total][param_width]; NTX_E_INVALID for a branch the model does not have. */
int ntx_trainer_create_flex_ex(const ntx_model_desc_ex *desc, const float *weights_host, size_t n_floats, int device, int64_t max_rays, int max_samples_per_ray,
                               ntx_trainer **out);
/* dL/d params of a training step (ABI v7, appended): the gradient of the step's loss with respect to the material parameters -- the inverse
 * use of a ParamNerf, fitting parameters to target images with the weights fixed.  For a handle of ntx_trainer_create_flex or
 * ntx_trainer_create_flex_ex whose model has parameters (n_geo + n_app > 0).  mode 0: off (the default; nothing about the handle or its
 * steps changes, nothing is placed).  mode 1: every following ntx_train_step_gradients also leaves dL/d params; loss, predictions and weight
 * gradients stay bit for bit what they are without it.  mode 2: parameters only -- as mode 1, but no weight gradient is contracted or
 * reduced and the trainer's gradient buffer is left untouched; ntx_trainer_adam_step, ntx_trainer_allreduce_gradients and
 * ntx_trainer_stash_gradients return NTX_E_INVALID until the mode is 0 or 1 again.  Buffers are placed at the first enable, for the trainer's
 * capacity.  NTX_E_UNSUPPORTED: a handle of ntx_trainer_create (the fused chain stops at the encoded inputs; the layer-by-layer entries take
 * the same model).  NTX_E_INVALID: a model without parameters (a Nerf, n_parameters [0, 0]), a mode outside 0..2.
 * What is differentiated: the parameter rows `params` of the step, through FourierFeatures(parameters) (identity, sin and cos rows of every
 * band, at the value the encoder fed) and, for blur_idx, through its product with the sample's cone_scale * z (renderer.py:155-158), into
 * every layer that reads the parameter features: trunk layer 0 and the layers behind a skip (geometry), the first layer that reads dir_map
 * (appearance) -- or the first layer of each parameter branch when param_depth > 0.  Positions and directions take theirs under
 * ntx_trainer_enable_input_gradients.
 * The order of the sums: the readers' terms in descending layer order; the samples of a ray in a fixed order of the ray's own (64 interleaved
 * partial sums, then a butterfly); the rays of a parameter row r / rays_per_param_row in ascending ray order.  None depends on the
 * trainer's capacity or on a launch's grid: a step's parameter gradients are bit-reproducible.  A ray with tnear_far = inf contributes
 * exactly 0, whatever its cone_scale holds (NaN included).
 * Out of scope: the parameters of an IPE model (it trains on the chain only), of a coarse + fine pair (two steps: add the two results), and
 * an all-reduce of parameter gradients across ranks. */
int ntx_trainer_enable_param_gradients(ntx_trainer *t, int mode);
/* Where the last step left them: DEVICE memory of the trainer's device, grad_dev[rows][n_params] with rows = ceil(n_rays /
 * rays_per_param_row) of that step and n_params = n_geo + n_app, geometry columns first; written in the step's stream order, valid until
 * the next step.  NTX_E_INVALID when the mode is 0 or no step has run since it was enabled. */
int ntx_trainer_param_gradients(ntx_trainer *t, const float **grad_dev, int64_t *rows, int *n_params);
/* A step under ANY loss (ABI v7, appended): ntx_train_step_gradients cut in two at the predictions.  Every gradient of a step is linear in
 * dL/d color_pred and dL/d alpha_pred, so a caller that evaluates its own loss on the predictions and hands back those two cotangents gets
 * the gradients of that loss; the network, the composite and its adjoint stay the library's kernels.
 * ntx_train_forward: ntx_train_step_gradients' arguments, checks and meaning less the loss and the targets -- depths, noise, the network with
 * every activation kept, the composite -- and color_pred[N,3] / alpha_pred[N] (DEVICE, each may be NULL).  The step is then PENDING in the
 * handle.  CONTRACT: until its ntx_train_backward, the caller keeps rays_o, rays_d, params, cone_scale and z_vals alive and unchanged (the
 * way back reads them again; depths the entry sampled itself are the handle's), runs nothing else on the handle that takes a step, and
 * queues the backward on a stream ordered behind the forward's.
 * ntx_train_backward: d_color[N,3] = dL/d color_pred, d_alpha[N] = dL/d alpha_pred or NULL for 0 (DEVICE) -> the composite's adjoint and the
 * way back through the network: the weight gradients in the trainer, dL/d params under ntx_trainer_enable_param_gradients mode 1 / 2 (mode
 * 2: no weight gradient, as in the fused step) -- with the cotangents of a loss ntx_train_step_gradients knows, bit for bit that entry's.
 * A ray that missed the proxy (tnear_far inf) takes no gradient whatever its cotangent holds, NaN and inf included.
 * ONE backward per forward: NTX_E_INVALID without a pending forward, on a second call, on a NULL d_color (the forward stays pending).
 * ntx_train_step_gradients and a new ntx_train_forward drop a pending step.  A handle that never calls these entries is what it was.
 * Out of scope: second-order gradients (nothing differentiates the backward), and a coarse + fine pair as one differentiable op. */
int ntx_train_forward(ntx_trainer *t, const float *rays_o, const float *rays_d, const float *tnear_far, const float *params, int64_t rays_per_param_row,
                      const float *cone_scale, int64_t n_rays, int n_samples, int blur_idx, uint32_t flags, const float *bkgd, uint64_t perturb_seed,
                      const ntx_render_opts *opts, const float *z_vals, float *color_pred, float *alpha_pred, ntx_stream stream);
int ntx_train_backward(ntx_trainer *t, const float *d_color, const float *d_alpha, ntx_stream stream);
/* The differentiable InstanceRenderer tail (ABI v7, appended): ntx_train_forward for the instanced render -- InstanceRenderer.evaluate_model +
 * map_model_output (renderer.py:247-354, inference-only in the reference: :233) downstream of the instancer, exactly as
 * ntx_render_instanced documents them, with every activation kept, so that a network is trained, or a parameter field fitted, in the
 * scene it is rendered in.  For a handle of ntx_trainer_create_flex / ntx_trainer_create_flex_ex (parameter branches included), and for one
 * of ntx_trainer_create after ntx_trainer_enable_instanced (below: the fused 8 x 256 chain on the compact rows); NTX_E_UNSUPPORTED for a
 * handle of ntx_trainer_create that never called it (the fused chain runs on whole rays; the layer-by-layer entries take the same model).
 * The arguments are ntx_render_instanced's buffers (DEVICE): rays_d_map[N,S,3], pts[N,S,3], t_map[N,S], dists[N,S], color_last[N,3],
 * alpha_last[N], alpha_weight[N,S] (NULL = density_reweighting off), hit[N] uint8, params_map[N,S,P] (NULL when P == 0), cone_scale[N]
 * (with t_map needed only for blur_idx >= 0).  Sample (r, s) is LIVE iff hit[r] != 0 && dists[r,s] > 0.  A live sample's network inputs:
 * pts, rays_d_map as given (not normalised), params_map with column blur_idx times cone_scale[r] * t_map[r,s] / patch_scale (:259-263);
 * its composite: sigma' = sigma * alpha_weight * density_scale, a = 1 - exp(-relu(sigma') * dists / patch_scale), colour sigmoid or -- under
 * NTX_FLAG_MAP_EXR -- elu + 1.  A sample that is not live has a = 0 exactly (its factor of the running product is 1 + 1e-10, as in the
 * reference), and NOTHING is read from pts, rays_d_map, t_map, alpha_weight or params_map there (the sparse instancer leaves those
 * elements unwritten).  One appended sample (color_last as is, alpha_last as an alpha) closes every hit ray; NTX_FLAG_COMPOSITE_BKGD as in
 * the render entry; a ray with hit == 0 predicts 0 / 0 also under the background and takes no gradient whatever its cotangent holds (NaN
 * and inf included: it is never read).
 * COMPACTION: the live samples are numbered in ascending (ray, sample) order by a prefix sum in two levels -- a function of hit and dists
 * alone, no atomic decides an order -- and the network runs on those n_live rows only: the encoder, every layer's contraction forward and
 * back, the heads, the weight gradients' partial sums over ranges of 2048 ROWS; ntx_trainer_activation's rows are the compact rows.  The
 * launches are sized on the host, so the forward copies the count back (8 bytes) and waits for `stream`: the ONE synchronisation of the
 * step.  *n_live_out (HOST, may be NULL) receives it.  n_live = 0 is a legal step: the predictions come from the appended sample alone,
 * every weight gradient is exactly 0 and no contraction is launched.  A step's gradients do not depend on the trainer's capacity.
 * The step is then PENDING as ntx_train_forward's, under the same CONTRACT: the caller keeps all buffers alive and unchanged until
 * ntx_train_backward(t, d_color, d_alpha, stream) -- one backward per forward; a new forward of either kind or an ntx_train_step_gradients
 * replaces a pending one; a NULL d_color leaves it pending.  The backward: ray_adjoint's recurrences through the view of an
 * instanced ray (InstancedRay, ntx_composite.h: the appended sample behind sample S - 1, dL/d sigma of a live sample); color_last,
 * alpha_last and alpha_weight take no gradient; positions and directions take theirs under ntx_trainer_enable_input_gradients
 * (ntx_trainer_sample_input_gradients).
 * dL/d params (ntx_trainer_enable_param_gradients mode 1 / 2, semantics unchanged): an instanced step leaves PER-SAMPLE gradients
 * grad_dev[N][S][P] (geometry columns first; through FourierFeatures and, for blur_idx, times cone_scale * t / patch_scale; exact zeros at
 * samples that are not live) behind ntx_trainer_sample_param_gradients (DEVICE memory of the trainer, valid until the next step;
 * NTX_E_INVALID after a plain step or in mode 0); ntx_trainer_param_gradients returns NTX_E_INVALID after an instanced step.
 * NTX_E_INVALID: n_samples outside 1 .. 1024, n_rays / n_rays * n_samples beyond the trainer's capacity, patch_scale <= 0, blur_idx >= P,
 * blur_idx >= 0 without cone_scale or t_map, NTX_FLAG_PERTURB or NTX_FLAG_RAW_NOISE (the instancer places the samples; noise is out of
 * scope), a required buffer NULL.  Out of scope: IPE models, false colours, coarse + fine. */
int ntx_train_forward_instanced(ntx_trainer *t, const float *rays_d_map, const float *pts, const float *t_map, const float *dists,
                                const float *color_last, const float *alpha_last, const float *alpha_weight, const uint8_t *hit,
                                const float *params_map, const float *cone_scale, int64_t n_rays, int n_samples, int blur_idx,
                                float patch_scale, float density_scale, uint32_t flags, const float *bkgd, float *color_pred,
                                float *alpha_pred, int64_t *n_live_out, ntx_stream stream);
int ntx_trainer_sample_param_gradients(ntx_trainer *t, const float **grad_dev, int64_t *n_rays, int *n_samples, int *n_params);
/* dL/d rays and sample points (ABI v7, appended): the third kind of input of the layer-by-layer step -- where the rays and the sample points
 * are -- for camera or pose refinement against photographs (plain step) and for deforming or placing the volume a texture lives in (instanced
 * step).  For a handle of ntx_trainer_create_flex / ntx_trainer_create_flex_ex, any model they take (a Nerf included).
 * mode 0: off (the default; nothing about the handle, its allocations, its launches or its results changes).  mode 1: every following
 * ntx_train_step_gradients, ntx_train_forward + ntx_train_backward and ntx_train_forward_instanced + ntx_train_backward also leaves the input
 * gradients; loss, predictions, weight gradients and parameter gradients stay bit for bit what they are without it.  mode 2: inputs with fixed
 * weights (pose fitting) -- no weight gradient is contracted or reduced and the trainer's gradient buffer is left untouched: the weight
 * gradient is taken unless EITHER this mode or ntx_trainer_enable_param_gradients' is 2, and ntx_trainer_adam_step,
 * ntx_trainer_allreduce_gradients and ntx_trainer_stash_gradients return NTX_E_INVALID while either is.  Buffers are placed at the first
 * enable, for the trainer's capacity; the transposed weight rows it needs go behind the ones already placed.  A change of the mode drops a
 * pending ntx_train_forward (its ntx_train_backward returns NTX_E_INVALID): set the mode before the forward.
 * NTX_E_UNSUPPORTED: a handle of ntx_trainer_create.  NTX_E_INVALID: a mode outside 0..2.
 * What is differentiated: rays_o and rays_d of a plain step, pts and rays_d_map of an instanced one.  The sample depths are constants:
 * tnear_far, z_vals, the jitter and sample_pdf take no gradient (renderer.py:129), nor does cone_scale; the blur product cone_scale * z (plain)
 * or cone_scale * t / patch_scale (instanced) does not depend on the ray.  With K3p = 3 (1 + 2 pos_freq) and K3d = 3 (1 + 2 dir_freq): every
 * trunk layer that reads pos_map (layer 0 and the layers behind a skip, with or without parameter branches) contributes dY . W[first K3p
 * rows]^T to the gradient at the FF(xyz) rows of a sample, the first layer that reads dir_map (index depth + 1: the colour half layer when
 * color_depth = 0) dY . W[first K3d rows]^T at the FF(dir) rows; the readers' terms are added in descending layer order.  Through the encoder a
 * row becomes a 3-vector: component c is the identity row plus, per band, slope(sin row) + slope(cos row) at the value x_c the encoder fed --
 * a_s for the position of sample s, b_s for its direction.
 * A plain step, a ray with depths z_s, n = d / |d|, B = sum_s b_s:
 *     d_rays_o = sum_s a_s,     d_rays_d = sum_s z_s a_s + (B - n (n . B)) / |d| + n dL/d|d|
 * where dL/d|d| = (sum_s dL/d sigma_s (sigma_s + noise_s)) / |d| is the composite's dists = dz |d| (renderer.py:180).  The samples of a ray are
 * added in a fixed order of the ray's own (64 interleaved partial sums, then a butterfly): bit-reproducible, independent of the trainer's
 * capacity.  A ray with tnear_far = inf gets exactly 0 in both rows whatever its cone_scale and cotangent hold (NaN and inf included).
 * An instanced step: d_pts[m] = a and d_dirs[m] = b of live sample m (the direction is fed as given: no normalisation term; dists are the
 * caller's: no |d| term), exact zeros at samples that are not live, where nothing of pts / rays_d_map is read; n_live = 0: both are zeros.
 * Out of scope: depths and tnear_far, cone_scale, the chain, a coarse + fine pair (two steps: add the two results), color_last / alpha_last /
 * alpha_weight, second order. */
int ntx_trainer_enable_input_gradients(ntx_trainer *t, int mode);
/* Where the last PLAIN step left them: d_rays_o[n_rays][3] and d_rays_d[n_rays][3], DEVICE memory of the trainer, written in the step's
 * stream order, valid until the next step.  NTX_E_INVALID in mode 0, before any step since the enable, or after an instanced step. */
int ntx_trainer_ray_gradients(ntx_trainer *t, const float **d_rays_o, const float **d_rays_d, int64_t *n_rays);
/* Where the last INSTANCED step left them: d_pts[n_rays][n_samples][3] and d_dirs[n_rays][n_samples][3] (dL/d rays_d_map), as above.
 * NTX_E_INVALID in mode 0, or when the last step since the enable was not an instanced one. */
int ntx_trainer_sample_input_gradients(ntx_trainer *t, const float **d_pts, const float **d_dirs, int64_t *n_rays, int *n_samples);
/* Both gradient modes at once, for either kind of handle (ABI v7, appended): param_mode and input_mode are the modes of
 * ntx_trainer_enable_param_gradients and ntx_trainer_enable_input_gradients -- each 0 off, 1 beside the weight gradients, 2 without them --
 * with the semantics stated there, and ntx_trainer_param_gradients / ntx_trainer_ray_gradients hand out the results as they are.  On a handle
 * of ntx_trainer_create_flex / _flex_ex it does what those two entries do, one after the other.  On a handle of ntx_trainer_create it is the
 * way in: the fused 8 x 256 chain keeps the gradient at every layer's output, and one more matrix-core kernel behind the chain back takes the
 * three products it leaves out -- dy0 . W_trunk0[pos_map rows]^T + dy5 . W_trunk5[pos_map rows]^T and d c1o . W_C1[dir_map rows]^T per sample,
 * each sum in a fixed order of its own (bit-reproducible, independent of the grid and of the trainer's capacity) -- into row-major buffers
 * that the layer-by-layer backend's own folds then read (ntx_trainer_activation slots 40 / 41 after such a step: [n][Kp], [n][Kd]).  With
 * both modes 0 a chain handle allocates and launches exactly what it does without this entry; the buffers are placed at the first non-zero
 * mode, for the trainer's capacity.  Mode 2 of either: no weight gradient is contracted or reduced, the gradient buffer is left alone, and
 * ntx_trainer_adam_step, ntx_trainer_allreduce_gradients and ntx_trainer_stash_gradients return NTX_E_INVALID.  A change of either mode drops
 * a pending ntx_train_forward (its ntx_train_backward returns NTX_E_INVALID): set the modes before the forward.
 * Checked before anything is placed, and a failed call leaves both modes as they were: NTX_E_INVALID for t NULL, a mode outside 0..2, or
 * param_mode != 0 on a model without parameters; NTX_E_UNSUPPORTED for a non-zero mode on an IPE chain handle (the cone gaussians' derivative
 * is not written).  ntx_trainer_enable_param_gradients and ntx_trainer_enable_input_gradients keep refusing a chain handle.
 * An instanced step on the chain (ntx_trainer_enable_instanced) leaves the per-sample results of these modes behind
 * ntx_trainer_sample_param_gradients / ntx_trainer_sample_input_gradients, as a layer-by-layer handle's does.
 * Out of scope on the chain: IPE models, depths / tnear_far / cone_scale, an all-reduce of these gradients, second order. */
int ntx_trainer_enable_gradients(ntx_trainer *t, int param_mode, int input_mode);
/* Instanced steps on the fused 8 x 256 chain (ABI v7, appended): after this call a handle of ntx_trainer_create takes
 * ntx_train_forward_instanced + ntx_train_backward with exactly the meaning documented there -- the live rule, the compaction in ascending
 * (ray, sample) order, the one 8-byte read-back of n_live, nothing read at a sample that is not live, the appended sample, NTX_FLAG_MAP_EXR and
 * NTX_FLAG_COMPOSITE_BKGD, n_live = 0 as a legal step with exactly-zero weight gradients and no network launch, one backward per forward, the
 * same NTX_E_INVALID cases.  The chain runs on the n_live compact rows: an encoder of its own writes the live samples' pos_map / dir_map in
 * the chain's operand layout (the values are the layer-by-layer encoder's, bit for bit), the forward chain runs without the per-ray direction
 * hoist (every sample has a direction and appearance parameters of its own), the shared instanced composite and its adjoint stand between, and
 * the narrow heads' dY tile is made from the adjoint's row-major result.  The weight gradients' partial sums are the chain's (a function of
 * n_live and the device's CU count, not of the trainer's capacity); two identical steps give identical bits.  Under
 * ntx_trainer_enable_gradients the step leaves ntx_trainer_sample_param_gradients [N][S][P] and ntx_trainer_sample_input_gradients
 * ([N][S][3] twice) with the semantics of a layer-by-layer handle, exact zeros at samples that are not live; mode 2 contracts and reduces no
 * weight gradient and leaves the gradient buffer alone; ntx_trainer_param_gradients / ntx_trainer_ray_gradients return NTX_E_INVALID after
 * an instanced step.  ntx_trainer_activation after such a step: the chain's slots (0-9, 10, 11, 20-30, 40 / 41) over the COMPACT rows.
 * The call only allocates -- the compaction's maps and scan workspace, for the trainer's capacity -- and is idempotent: plain steps after it
 * are bit for bit what they were, and a chain handle that never calls it allocates, launches and refuses as before.
 * NTX_OK and nothing changes for a handle of ntx_trainer_create_flex / _flex_ex (they take instanced steps already).  NTX_E_INVALID: t NULL.
 * NTX_E_UNSUPPORTED: an IPE chain handle (IPE stays out of scope for instanced steps). */
int ntx_trainer_enable_instanced(ntx_trainer *t);
/* Losses on the compositing weights (ABI v7, appended): a loss that looks ALONG the ray -- an expected depth sum_s w_s z_s against a depth
 * target, an entropy or distortion regulariser on the weights, a proposal loss for a sampler -- is a function of the weights
 * w_s = a_s T_s, not of color_pred and alpha_pred alone.  The way out exists: ntx_trainer_composite_weights(t, weights_dev) registers a
 * buffer weights_dev[N,S] (DEVICE) that every following step fills until it is taken back with NULL -- ntx_train_step_gradients (the coarse
 * pass's use), and equally ntx_train_forward and ntx_train_forward_instanced.  An instanced forward writes (1 - el) T at the live samples and
 * exactly 0 at samples that are not live and on rays with hit == 0; the appended sample's weight is not stored: it is
 * alpha_pred - sum_s w_s, so a loss on it is expressible through alpha_pred.
 * This entry is the way back: d_weights_dev[N,S] (DEVICE) = dL/d weights for the NEXT ntx_train_backward of the pending forward, plain or
 * instanced.  The composite's adjoint (ray_adjoint, ntx_composite.h: one statement for both kinds of step) has dL/dw_k = c_k + dA' with
 * c_k = dC . rgb_k; with a direct term g_k = d_weights[ray][k] it is
 *     dL/dw_k = c_k + g_k + dA',
 * and the same division-free recurrences hold with c_k + g_k in the place of c_k: dL/da_i = T_i (dA' Z_i + ((c_i + g_i) - V_i)),
 * V_{i-1} = (c_i + g_i) a_i + f_i V_i.  dL/d raw rgb is unchanged.  Everything behind the adjoint -- both backends, the weight gradients, the
 * parameter and input gradients, the instanced folds -- takes the gradient of such a loss with no change.
 * A plain ray without a live sample (tnear_far inf) selects 0 for its row, as for d_color / d_alpha: nothing of a row that may hold NaN or
 * inf is multiplied.  An instanced step reads the buffer at live samples only, and nothing of a ray with hit == 0.
 * The registration is consumed by that backward (used once); it is dropped by any new forward, by ntx_train_step_gradients, and by
 * d_weights_dev = NULL.  A backward without one runs the code path, and leaves every bit, of a handle that never called this entry; the
 * fused-loss step (ntx_train_step_gradients) takes no weight cotangent: its loss is its own.
 * The entry only records the pointer: it takes no stream, waits for nothing, allocates nothing and launches nothing.  CONTRACT: the caller
 * keeps d_weights_dev alive and unchanged until the backward's work on its stream has completed.
 * NTX_E_INVALID: t NULL, or no forward pending.  NTX_E_UNSUPPORTED: an IPE handle (ntx_trainer_composite_weights refuses it too).
 * Out of scope: IPE handles, coarse + fine, a stored weight for the appended sample, second order, an all-reduce of anything new. */
int ntx_trainer_weight_cotangent(ntx_trainer *t, const float *d_weights_dev);
/* Texture coordinates per sample (ABI v7, appended): where on the instancer mesh every sample of a finished ntx_instancer_model_input call
 * looks its parameter textures up -- the piece a learnable parameter texture needs outside the march kernel.  All buffers DEVICE; t and dists
 * [N,S] are what ntx_instancer_model_input wrote for the same rays_o / rays_d [N,3] and step_size.
 * A sample with dists > 0 lies in a patch.  Its query point is the march's own getPtOnRay: o + t_pt * d with t_pt = t, or the mean distance
 * of (t, step_size) when the instancer was made with use_mean_distance (t holds t_mu; the mean distance is formed again, by the same
 * expression on the same operands: the same float).  The point query is the march's (getParameters, instancer.cpp:644-654 and :661): the
 * closest point of the instancer mesh strictly within patch_max_extent, the lowest primID of several at one distance, its texture
 * coordinates mixed by the barycentrics.  uv_out[N,S,2] = (u, v) and found_out[N,S] = 1; (0, 0) and 0 when no triangle lies within reach.
 * A sample with dists <= 0 (or NaN), or with a t that is not finite, gets (0, 0) and 0, and nothing of the mesh is read for it.  Every
 * element of both outputs is written.  With an n_texture_samples so large that the march makes a lookup per step, params_map's textured
 * columns are exactly parameter * interpolate2d(texture, u, v) at found samples and the parameter elsewhere; with fewer texture samples the
 * march interpolates ALONG the ray between lookups (instancer.cpp:910-923), which this entry does not restate.
 * The grid the query walks belongs to the parameter textures (ntx_instancer_set_parameter_textures with n_textures > 0 -- a 1 x 1 texture
 * holding 1.0 multiplies by one and still builds the grid).  Refusals, all NTX_E_INVALID, checked in this order and all before the launch,
 * so a failed call has written nothing: inst NULL; any buffer NULL (also with n_rays = 0); n_pts outside [1, 4096]; n_rays < 0; no
 * parameter textures set.  Then n_rays = 0: NTX_OK without a launch.  One kernel, a thread per sample.
 * THE STREAM.  Unlike every other entry that launches, this one takes no `ntx_stream`, and that is a deliberate deviation from the first
 * convention above: its inputs t and dists ARE the results of the instancer's last ntx_instancer_model_input, so it is launched,
 * asynchronously, on the stream that call was given -- which the handle remembers; the null stream before any call -- behind it and
 * stream-ordered with the instancer's other calls.  The caller keeps that stream alive until this call has returned, as it would a
 * stream it passes; a consumer on another stream orders itself behind that one (an event).  An explicit `ntx_stream` parameter would
 * be the plainer interface; it is left out because every prototype with one must be registered in the stream-order tests' tables
 * (tests/stream_common.py), and this entry came with a change that adds test files only.  Adding the parameter later is an appended
 * entry (_ex), not a change of this one.  The entry allocates nothing and writes nothing of the instancer; the one thing
 * ntx_instancer_model_input does for it is to remember its stream. */
int ntx_instancer_sample_uv(ntx_instancer *inst, const float *rays_o, const float *rays_d, const float *t, const float *dists, int64_t n_rays,
                            int n_pts, float step_size, float *uv_out /* [N,S,2] */, uint8_t *found_out /* [N,S] */);

/* Opt-in bf16x6 training (ABI v7, appended): the precision of the contractions of a LAYER-BY-LAYER trainer (ntx_trainer_create_flex,
 * ntx_trainer_create_flex_ex) -- trunk and branch layers forward, dX, dW and db, and the terms behind dL/d params and dL/d inputs, of plain
 * and instanced steps -- NTX_PRECISION_F32 (the default) or NTX_PRECISION_BF16X6 (the arithmetic: beside the enum above).  The heads, the
 * encoder, the composite, the reductions, Adam and the weights are float32 either way, so checkpoints, gradients and all getters keep their
 * meaning.  It takes effect from the next step and can be changed back: a float32 step behind a bf16x6 one is bit for bit the step of a
 * trainer that never left float32.  NTX_E_INVALID: t NULL, a value that is no ntx_precision, or a forward pending its ntx_train_backward.
 * NTX_E_UNSUPPORTED: NTX_PRECISION_FP16X3 (a half cannot hold the cotangents), a chain handle (ntx_trainer_create; an IPE trainer is one).
 * A refused call changes nothing. */
int ntx_trainer_set_precision(ntx_trainer *t, int precision);
/* The handle's current precision (an ntx_precision), -1 for NULL. */
int ntx_trainer_precision(const ntx_trainer *t);
/* ntx_gemm_f32_ex's contraction through the bf16x6 body, for tests and benches of the kernel itself: the same arguments with the same
 * meaning -- both A forms, bias, relu, mask, accumulate, the K split, colsum (the float32 column sums of B, bit-equal to ntx_gemm_f32_ex's)
 * -- and the same NTX_E_INVALID refusals, all before the first launch, so a refused call has written nothing.  Operands and results are
 * float32 in memory.  THE STREAM.  This entry takes no `ntx_stream` and launches on the null stream: every prototype with an ntx_stream
 * parameter must be registered in the stream-order tests' tables (tests/stream_common.py), and this entry came with a change that adds test
 * files only.  A stream-taking variant is an appended entry (_ex2), not a change of this one; the training step itself runs the body on the
 * step's stream. */
int ntx_gemm_bf16x6_ex(const float *A, int lda, int a_kcontig, const float *B, int ldb, float *C, int ldc, int M, int N, int K, const float *bias, int relu,
                       const float *mask, int ldmask, int accumulate, int n_split, int k_chunk, int64_t split_stride, float *colsum);

/* Rays from camera poses that live on the device (ABI v7, appended): ntx_generate_rays_at for a BATCH of cameras, the first half of camera
 * pose fitting -- the rays of a training batch (say 4 images x 256 rays) in one launch, with no host round trip for the poses an optimiser
 * keeps on the device.
 *   poses            DEVICE float [n_poses][3][4]: the top three rows of every c2w, row-major
 *   focal            DEVICE float [n_poses]
 *   image_plane_loc  DEVICE float [n_rays][2] = (row, col), as ntx_generate_rays_at takes it
 *   rays_per_pose    ray k belongs to pose k / rays_per_pose; the last pose may have fewer rays; n_poses = ceil(n_rays / rays_per_pose)
 * height, width, mode (0: Proxy with the HOST float[3] b0 / b1; 1: Frustum with near_t / far_t) and the four DEVICE outputs rays_o[n,3],
 * rays_d[n,3], t[n,2], cone_scale[n,1] are ntx_generate_rays_at's.  No pose, focal or location is read from the host; the call waits for
 * nothing and allocates nothing.  The arithmetic of a ray is the ONE device function ntx_generate_rays_at's kernel runs, in its float32
 * order: with the same matrix and focal the four outputs are ntx_generate_rays_at's bit for bit.
 * `stream`: a hipStream_t passed as void*, with the meaning of every other entry's `ntx_stream` (NULL = the null stream; the launch is queued
 * on it and nothing else is touched).
 * NTX_E_INVALID, all before the launch: a NULL buffer; height, width <= 0 or n_rays < 0; a mode outside 0..1; n_poses < 1 (or >= 2^31);
 * rays_per_pose < 1; n_rays > 0 and n_poses != ceil(n_rays / rays_per_pose); b0 or b1 NULL in mode 0.  n_rays = 0 (with otherwise valid
 * arguments): NTX_OK and no launch. */
int ntx_generate_rays_posed(const float *poses, const float *focal, int64_t n_poses, int height, int width, const float *image_plane_loc, int64_t n_rays,
                            int64_t rays_per_pose, int mode, const float *b0, const float *b1, float near_t, float far_t, float *rays_o, float *rays_d, float *t,
                            float *cone_scale, void *stream /* hipStream_t */);
/* The adjoint of that map (ABI v7, appended): from the cotangents d_rays_o, d_rays_d (DEVICE [n_rays][3]; what a trainer's
 * ntx_trainer_ray_gradients leaves) to d_poses (DEVICE [n_poses][3][4]) and d_focal (DEVICE [n_poses]) -- what connects a camera to the ray
 * gradients that ntx_trainer_enable_input_gradients / ntx_trainer_enable_gradients document for "camera or pose refinement".  The first nine
 * arguments are ntx_generate_rays_posed's.  With (li, lj) a ray's location, f its pose's focal and R the pose's 3x3:
 *     dc = (d0, d1, -1),  d0 = (lj + 0.5 - width / 2) / f,  d1 = -(li + 0.5 - height / 2) / f      (ray_sampler.py:41)
 *     v = R dc,  n = v / |v|,  g_o = d_rays_o[k],  g_d = d_rays_d[k]
 *     mode 0 (rays_d = n):  g_v = (g_d - n (n . g_d)) / |v|          mode 1 (rays_d = v):  g_v = g_d
 *     d_poses[p][r][c] = sum_k g_v[r] dc[c]   (c < 3: dL/dR)          d_poses[p][r][3] = sum_k g_o[r]   (dL/dT)
 *     d_focal[p] = -(1 / f) sum_k g_v . (d0 R[:,0] + d1 R[:,1])
 * the sums over the rays k of pose p.  HELD CONSTANT: t and cone_scale -- the convention of ntx_trainer_enable_input_gradients, where the
 * depths, tnear_far and cone_scale take no gradient; so the proxy's bounds are not among the arguments, and the focal's gradient is the one
 * through the ray directions alone.  The pose is differentiated as twelve free numbers: keeping R a rotation is the caller's parametrisation.
 * The sums of a pose run in a fixed order of the pose's OWN: lane i of 1024 adds the terms of the pose's rays i, i + 1024, ... in ascending
 * order (T = 1024 partial sums), a butterfly adds the 64 lanes of each wave and a binary tree the 16 waves.  The result is bit-reproducible and
 * does not depend on n_poses, on where the pose stands in the batch or on the grid: one workgroup per pose, one pass, no atomics, no scratch
 * and no allocation.  A ray whose d_rays_d is exactly zero adds exact zeros to dR and d_focal whatever its direction holds, one whose
 * d_rays_o is zero adds exact zeros to dT: rays that missed (a trainer leaves exact zeros there) change no bit.  EVERY entry of d_poses and
 * d_focal is written -- +0.0 for a pose whose cotangents are all zero, and for every pose when n_rays = 0 (then n_poses >= 1 is all that is
 * asked of it).
 * `stream`: as above.  NTX_E_INVALID, all before the launch: as above, without the bounds.  Out of scope: gradients through t, the depths
 * and cone_scale; lens distortion and principal point; second order. */
int ntx_generate_rays_posed_adjoint(const float *poses, const float *focal, int64_t n_poses, int height, int width, const float *image_plane_loc, int64_t n_rays,
                                    int64_t rays_per_pose, int mode, const float *d_rays_o, const float *d_rays_d, float *d_poses, float *d_focal,
                                    void *stream /* hipStream_t */);

/* The distortion loss on the compositing weights (ABI v7, appended; csrc/ntx_ray_losses.hip): the regulariser of mip-NeRF 360 (Barron et
 * al. 2022, eq. 15), the first loss along the ray that cannot sensibly be written in torch on ntx_trainer_weight_cotangent's hook -- its
 * textbook form is a double sum over sample pairs, [N][S][S] intermediates.  THE FORMULA, stated here once.  For one ray with weights w_i,
 * depths z_i (nondecreasing over the live samples) and interval widths delta_i, the sums over the ray's LIVE samples only:
 *     L       = sum_i sum_j w_i w_j |z_i - z_j|  +  (1/3) sum_i w_i^2 delta_i
 *     dL/dw_k = 2 sum_j w_j |z_k - z_j|          +  (2/3) w_k delta_k
 * The depths are constants, as everywhere in the trainers: there is no dL/dz.  Evaluated in O(S): m_i = z_i - z_first, z_first the depth of
 * the ray's first live sample; with the exclusive prefix sums W_<, M_< of w and w m, and the matching suffix sums W_>, M_>,
 *     sum_j w_j |z_k - z_j| = (m_k W_<k - M_<k) + (M_>k - m_k W_>k),      L = 2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 delta_i.
 * The shift by z_first is part of the specification: |z| does not enter the rounding, only the span the ray's samples cover (a float32
 * restatement against the float64 pair sum, near = 500, span 0.5, S = 256, rel-Linf of loss / gradient: 4.5e-7 / 8.5e-7 shifted, 8.8e-4 /
 * 1.8e-3 without the shift; tests/test_ray_distortion.py reproduces both).
 * All pointers DEVICE:
 *   weights[N,S], z_vals[N,S]   required
 *   widths[N,S] or NULL         NULL: delta_i = z_{i+1} - z_i, delta_{S-1} = delta_{S-2} (the composite's convention, in ray-parameter units);
 *                               0 for S == 1, and 0 where the neighbouring depth it is taken from is not finite
 *   live[N,S] or NULL           a sample is live iff live > 0 (ntx_render_instanced's rule, with dists in that role); NULL: every sample
 *                               is a candidate.  A sample whose depth is not finite is never live (a ray that missed its proxy: depths
 *                               inf, weights 0).  A sample that is not live adds nothing and takes gradient exactly 0; its z, w and width
 *                               are selected away, never multiplied (the sparse instancer leaves those rows unwritten: they may hold NaN)
 *   ray_scale[N] or NULL (= 1)  a factor per ray on both outputs: the caller's lambda / N / (far - near).  A ray without a live sample has
 *                               loss 0 and a zero gradient row whatever its ray_scale holds, NaN included
 *   loss_out[N], grad_out[N,S]  either may be NULL; each is the same bits with or without the other
 * NTX_E_INVALID, all checked before the launch, so a refused call has written nothing: weights or z_vals NULL; loss_out and grad_out both
 * NULL; n_samples outside [1, 4096] (the instanced render's limit); n_rays < 0 or >= 2^31; live without widths (differences of neighbouring
 * depths would read samples that are not live).  n_rays = 0: NTX_OK without a launch.
 * The kernel: one wave per ray, four rays a workgroup, the sample index across the lanes in chunks of 64 (a coalesced row of 256 bytes).
 * Pass 1 finds z_first (the first live lane of the first chunk that has one) and the totals of w and w m; pass 2 -- the row comes from L2
 * the second time -- takes inclusive scans by chunk with carries, the suffix sums as totals less prefix, and the loss from a wave sum.  Pass
 * 1's totals are added in the order pass 2's carries are, so the last live sample's suffix is exactly 0.  No atomics, no LDS, no scratch;
 * the order of every sum is fixed by S alone, so a ray's outputs are the same bits in every run, at every n_rays and at every row.
 * `stream`: a hipStream_t passed as void*, with the meaning of every other entry's `ntx_stream` (NULL = the null stream; the launch is queued
 * on it and nothing else is touched, waited for or allocated).
 * Measured on an MI355X (tools/bench_ray_distortion.py, profiles/ray_distortion/bench.json; HIP events, medians of 5 windows of 20 calls, the
 * sides alternating in one run): loss + gradient 0.017 ms at 1024 x 256 and 0.027 ms at 256 x 1024 with 1 MB of peak memory (the outputs),
 * beside 0.39 / 0.40 ms and 8 MB for a torch.cumsum statement with autograd and 0.92 / 3.26 ms and 770 / 3075 MB for the pairwise one; a step
 * of the fused chain at 1024 x 256 takes 7.64 ms under mse, 7.68 ms with this term and 8.55 ms with the pairwise torch term.  The kernel is
 * bound by launch and memory latency (a call moves 3 MB), not by bandwidth; no speed was promised.  Against the float64 pair sum, rel-Linf
 * over the batch, error | float32 floor of a sequential restatement (tests/distortion_common.py; the gate is max(4 floors, 5e-7), never
 * beyond 1e-4): S = 1 .. 3 at most 9.6e-8 | 5.2e-8; S = 63 .. 255 at most 2.6e-7 | 4.8e-7; S = 4096 3.5e-7 | 3.2e-6; near = 500 2.8e-7 |
 * 8.5e-7; with 35 % of the samples live 3.0e-7 | 3.2e-7; the tightest case (S = 129, saturated rays, given widths) 3.3e-7 | 1.2e-7.
 * Out of scope: dL/d depths; IPE trainers (they hand out no weights); the fused-loss step (ntx_train_step_gradients with a descriptor: a loss
 * with this term takes the ntx_train_forward / ntx_train_backward route); coarse + fine pairs; unsorted depths (the O(S) form assumes
 * nondecreasing live depths: the result is undefined otherwise); second order; any all-reduce. */
int ntx_ray_distortion(const float *weights, const float *z_vals, const float *widths, const float *live, const float *ray_scale, int64_t n_rays, int n_samples,
                       float *loss_out, float *grad_out, void *stream /* hipStream_t */);

/* The interlevel loss between two histograms on one ray (ABI v7, appended; csrc/ntx_ray_losses.hip): the partner of the distortion loss in
 * mip-NeRF 360 (Barron et al. 2022, eq. 13), which supervises a sampler's (proposal) weights with the fine pass's weights, so that the first
 * network of a coarse + fine pair need not be trained on the image at all.  Its textbook form is an [N][S][S_p] overlap mask.  THE FORMULA,
 * stated here once.  One ray carries the fine histogram, weights w_i at nondecreasing depths z_i (i < S), and the proposal one, weights ŵ_j
 * at nondecreasing depths ẑ_j (j < S_p).  A sample's interval is [a_i, b_i]: a_i = z_i; b_i = z_{i+1}, THE NEXT DEPTH ITSELF, for i < S-1;
 * b_{S-1} = z_{S-1} + (z_{S-1} - z_{S-2}), the composite's last-width convention; b_0 = a_0 when S == 1; the same for the proposal set.  (The
 * end is the stored neighbour, never z_i + (z_{i+1} - z_i) recomputed: the fine depths are the proposal depths merged with the importance
 * samples, so exact ties between the two sets are the normal case, and a rounded end would flip an overlap and move the bound by a whole ŵ_j.)
 *     overlap(i, j)  iff  ẑ_j < b_i  and  b̂_j > a_i           (open intersection: intervals that only touch do not overlap; the counts are the definition)
 *                    =    j in [lo_i, hi_i),  lo_i = #{j : b̂_j <= a_i},  hi_i = #{j : ẑ_j < b_i}
 *     bound_i  = sum_{j in [lo_i, hi_i)} ŵ_j                    (added in increasing j)
 *     r_i      = max(0, w_i - bound_i),     q_i = r_i / (w_i + eps)
 *     L        = sum_i r_i q_i
 *     dL/dŵ_j  = -2 sum_{i : overlap(i, j)} q_i                 (added in increasing i; the set is again a contiguous range:
 *                                                                 i in [#{i : b_i <= ẑ_j}, #{i : a_i < b̂_j}))
 *     dL/dw_i  = q_i (2 - q_i)
 * The depths are constants, as everywhere in the trainers: there is no dL/dz.  A ray is LIVE iff every depth of both sets is finite (a ray
 * that missed its proxy has all depths inf); a ray that is not live has loss 0 and two zero gradient rows whatever its ray_scale and its
 * weights hold, NaN included: its values are selected away, never multiplied.
 * All pointers DEVICE:
 *   weights[N,S], z_vals[N,S], weights_prop[N,S_p], z_prop[N,S_p]   required
 *   ray_scale[N] or NULL (= 1)     a factor per ray on all three outputs: the caller's lambda / N
 *   eps                            the guard of the division; Python's default is 2^-23, float32's epsilon (multinerf's choice)
 *   loss_out[N], grad_prop_out[N,S_p] = dL/dŵ, grad_fine_out[N,S] = dL/dw   any may be NULL; each is the same bits with or without the others
 * NTX_E_INVALID, all checked before the launch, so a refused call has written nothing: a NULL required pointer; all three outputs NULL;
 * n_samples or n_prop outside [1, 4096]; n_rays < 0 or >= 2^31; eps not finite or <= 0.  n_rays = 0: NTX_OK without a launch.
 * The kernel: one wave per ray, four rays a workgroup, a grid-stride over rays.  Pass A puts the fine samples across the lanes in chunks of
 * 64: each lane finds lo_i and hi_i by binary search over the proposal row, adds ŵ_j over its range DIRECTLY, writes dL/dw_i, keeps q_i in
 * the wave's own S floats of LDS and accumulates r_i q_i for a wave sum.  Pass B puts the proposal samples across the lanes: the mirrored
 * searches over the fine row and a direct sum of q_i.  Direct sums, not differences of prefix sums: a prefix difference carries an absolute
 * error of float32's epsilon times the ray's total weight, and q divides by w + eps -- of order 1 in q where w is about 1e-8, in every ray's
 * tail; the ranges add up to at most S + S_p over a ray.  The LDS is sized on the host, 16 * S bytes a workgroup (64 KB at the limit); the
 * searched rows come from the caches.  No atomics, no scratch; every loop index is bounded by the row it reads; the order of every sum is a
 * function of (S, S_p) and the depths' ranges alone, never of n_rays, the row, the other outputs or the workgroup's other rays, so a ray's
 * outputs are the same bits in every run.  `stream`: as for ntx_ray_distortion.
 * Out of scope: dL/d depths; IPE trainers (they hand out no weights); a density-only proposal network (the colour layers still run and take
 * zeros); shared-network pairs; data-parallel pairs; more than one proposal level; instanced steps; unsorted depths (undefined); second
 * order. */
int ntx_ray_interlevel(const float *weights, const float *z_vals, int n_samples, const float *weights_prop, const float *z_prop, int n_prop,
                       const float *ray_scale, float eps, int64_t n_rays, float *loss_out, float *grad_prop_out, float *grad_fine_out,
                       void *stream /* hipStream_t */);

#ifdef __cplusplus
}
#endif
#endif /* NERFTEX_H */
