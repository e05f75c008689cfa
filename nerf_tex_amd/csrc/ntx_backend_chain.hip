// ntx_backend_chain.hip -- the chain backend of a training step (ntx_trainer_create): the ParamNerf architecture of the shipped training
// configs (8 x 256, skip 4, color_depth 1; configs/config_carpet_train.py: 4 images x 256 rays x 256 samples = 262 144 samples a step).
// Every layer's activations are stored once, and the network is three passes on the f32 matrix cores (ntx_train_device.h, one object
// each from ntx_train_chain.hip: fwd_chain_kernel with a block's activations in registers from layer to layer, dx_chain_kernel back through
// the layers masked by the forward pass's ReLU bits, dw_kernel for every layer's dW = X^T . dY in one launch) between this file's kernels:
//   pack_kernel     the weights move every step: the forward and the transposed weight streams and the aux block (biases, narrow heads)
//   encode_kernel   sample points and the encodings of position / direction / parameters (ntx_encode.h): the first layer's and the two
//                   concatenations' inputs, in the row order the chain reads and in the operand order the weight gradients read
//   dirrow_kernel   the colour layer's direction segment once per ray, where a ray's samples share it
//   encode_samples_kernel, dhead_rows_kernel   an instanced step (ntx_trainer_enable_instanced): the same operands from the instancer's buffers
//                   over the compact rows of the live samples, and the narrow heads' dY tile from the shared composite adjoint's row-major dgrad
//   feat_grad_kernel  where dL/d params or dL/d rays is asked for (ntx_trainer_enable_gradients): the gradient at pos_map and dir_map, the three
//                   products the chain back leaves out, on the f32 matrix cores; ntx_backend_flex.hip's folds take it from there
// The handle, the composite, the loss, the partial sums' reduction and Adam are ntx_trainer.hip's.  gfx950 only.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "ntx_trainer.h"
#include "ntx_train_device.h"
#include "ntx_encode.h"
namespace ntx_train {
// ---------------------------------------------------------------------------------------------------------------------------
// the weights as the chains stream them (ntx_train_device.h), made once a step.  A segment of a stream: records (k-step s, tile group g) of
// 64 lanes x 4 floats, component c of lane (f, kh) = Wsrc[row(s, kh)][32 (4 g + c) + f] with Wsrc[k][col] = src[k * sk + col * sc]; rows
// beyond K (padding k-steps, the odd half of a last k-step) and columns beyond ncols are zero.  The aux block's pieces ride along.
// ---------------------------------------------------------------------------------------------------------------------------
enum { PACK_HIDDEN = 0, PACK_LINEAR = 1, PACK_AUX_ROW = 2, PACK_AUX_RGB = 3, PACK_COPY = 4 };
struct PackSeg {
    const float *src; long long sk, sc;
    int mode;                 // PACK_HIDDEN: row(s, kh) = hidden_row(s, kh) (the k-steps of a layer whose input is a lane's registers); PACK_LINEAR: 2 s + kh
    int K, ncols, nt;         // rows / columns that exist; tiles of the layer (4 or 8)
    float *dst; long long first, count;   // where it goes; the segment's first float in the launch's index space and how many
};
struct PackArgs { const PackSeg *seg; int n_seg; long long total; };
__global__ void pack_kernel(PackArgs a) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.total) return;
    int lo = 0, hi = a.n_seg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.seg[mid].first <= e) lo = mid; else hi = mid - 1; }
    const PackSeg &p = a.seg[lo];
    const long long o = e - p.first;
    float v = 0.0f;
    if (p.mode == PACK_COPY) v = p.src[o];
    else if (p.mode == PACK_AUX_ROW) {                   // [half][128]: value V of half h <-> feature hidden_row(V, h)
        const int h = (int)(o >> 7) & 1, V = (int)(o & 127), k = hidden_row(V, h);
        v = k < p.K ? p.src[k * p.sk] : 0.0f;
    } else if (p.mode == PACK_AUX_RGB) {                 // [3][half][64]
        const int c = (int)(o >> 7), h = (int)(o >> 6) & 1, V = (int)(o & 63);
        v = p.src[hidden_row(V, h) * 3 + c];
    } else {
        const int c = (int)(o & 3), lane = (int)((o >> 2) & 63);
        const long long rec = o >> 8;
        const int G = p.nt / 4, g = (int)(rec % G), s = (int)(rec / G);
        const int f = lane & 31, kh = lane >> 5;
        const int k = p.mode == PACK_HIDDEN ? hidden_row(s, kh) : 2 * s + kh, col = 32 * (4 * g + c) + f;
        if (k < p.K && col < p.ncols) v = p.src[k * p.sk + col * p.sc];
    }
    p.dst[o] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// encoder: layer.FourierFeatures (layer.py:8-23) of position [+ geometry parameters] and of direction [+ appearance parameters]
// (model.py:77-101), the sample points of renderer.py:98-114 and the blur product of :155-158.  One wave per block of 32 samples and map:
// lane (n, h) evaluates sin (h = 0) or cos (h = 1) of its sample with ONE function (ntx_device.h sin_q, the render kernels' own) and writes
// rows of 32 samples in O layout: the weight gradients' A operands, and what the chain gathers its B operands from.
// ---------------------------------------------------------------------------------------------------------------------------
struct EncodeArgs {
    StepRays r;
    float *posO; int ptiles;             // rows 0 .. Kp: pos_map; the rest of the ptiles * 32 rows stays zero
    float *dirO; int dtiles;
    float *dists;                        // [N][S]: z[i+1] - z[i], the last one repeated, times |rays_d| (renderer.py:174-180)
};
// IPE: the MipRenderer (renderer.py:365-444) and an IntegratedPositionalEncoding model (layer.py:25-41): sample s is the cone segment
// between edges z[s] and z[s+1] of the ray's S + 1 depths (z is [N][S+1]), encoded as the gaussian of cone_moments / cone_cov (ntx_device.h,
// the render kernel's own) with radius params[blur_idx] * cone_scale; the blur parameter is spliced out of the rows of P + 1 values and the model
// sees the other P.  pos_map = [sin(2^f mean_c) exp(-4^f cov_c / 2) for f, c band-major | the same with cos] | FourierFeatures(geometry
// parameters).  A ray that misses the proxy encodes mean = o, cov = 0 (finite rows) with dists 0: like the Fourier path's, it composites to
// 0 / the background and no gradient flows through its rows.
template <bool IPE>
__global__ __launch_bounds__(64) void encode_kernel(EncodeArgs args) {
    const StepRays &a = args.r;
    const int lane = threadIdx.x, n = lane & 31, h = lane >> 5, blk = blockIdx.x, part = blockIdx.y;
    const long long m = (long long)blk * 32 + n;
    const bool valid = m < a.M();
    const int ray = valid ? (int)(m / a.S) : 0, s = valid ? (int)(m - (long long)ray * a.S) : 0;
    const int P = a.n_geo + a.n_app;
    const RayCtx rc = ray_ctx(a.rays_d, a.params, a.rays_per_param_row, ray, IPE ? P + 1 : P);
    const float *zray = a.z + (size_t)ray * (IPE ? a.S + 1 : a.S);
    const float e0 = zray[s], e1 = IPE ? zray[s + 1] : 0.0f;
    bool hit;
    const float z = depth_of(e0, hit);                                                       // (the Fourier path's)
    if (IPE) hit = hit && isfinite(e1);
    auto param = [&](int c) { return IPE ? spliced_param(rc.pr, c, a.blur_idx) : blurred_param(rc.pr, c, a.blur_idx, hit, a.cone, ray, z); };
    float *O = part == 0 ? args.posO : args.dirO;
    const int tiles = part == 0 ? args.ptiles : args.dtiles;
    auto put = [&](int row, float v) { O[o_index(blk, tiles, row, n)] = valid ? v : 0.0f; };      // the tail of the last block: finite, and no gradient comes back
    auto fourier = [&](int r0, int D, int L, auto x) {                                      // lane (n, h): x itself, and one of sin / cos of every band
        if (h == 0) for (int c = 0; c < D; ++c) put(r0 + c, x(c));
        for (int f = 0; f < L; ++f)
            for (int c = 0; c < D; ++c) put(r0 + fourier_row_of(D, f, h, c), fourier_value(x(c), f, h));
    };
    if (part == 0) {
        int geo0;                                                                           // the row the geometry parameters' features start at
        if (IPE) {
            float mean[3] = {a.rays_o[3 * ray], a.rays_o[3 * ray + 1], a.rays_o[3 * ray + 2]}, cov[3] = {0.0f, 0.0f, 0.0f};
            if (hit) {                                                                          // renderer.py:411-437
                float t_mean, t_var, r_var;
                ntx::cone_moments((e0 + e1) / 2.0f, (e1 - e0) / 2.0f, rc.pr[a.blur_idx] * a.cone[ray], t_mean, t_var, r_var);
                for (int c = 0; c < 3; ++c) mean[c] = mean[c] + rc.d[c] * t_mean;
                ntx::cone_cov(t_var, r_var, rc.d, cov);
            }
            const int L = a.pos_freq;
            for (int f = 0; f < L; ++f)                                                             // layer.py:33-41: row h 3L + 3f + c
                for (int c = 0; c < 3; ++c)
                    put(h * 3 * L + 3 * f + c, ntx::sin_q(mean[c] * ldexpf(1.0f, f), h) * expf(-0.5f * (cov[c] * ldexpf(1.0f, 2 * f))));
            geo0 = 6 * L;
        } else {
            const float o[3] = {a.rays_o[3 * ray], a.rays_o[3 * ray + 1], a.rays_o[3 * ray + 2]};       // (read once: the stores in between may alias)
            fourier(0, 3, a.pos_freq, [&](int c) { return rc.point(o[c], c, z); });
            geo0 = fourier_width(3, a.pos_freq);
        }
        if (a.n_geo > 0) fourier(geo0, a.n_geo, a.param_freq, [&](int c) { return param(c); });          // model.py:88-93
    } else {
        fourier(0, 3, a.dir_freq, [&](int c) { return rc.dir(c); });
        if (a.n_app > 0) fourier(fourier_width(3, a.dir_freq), a.n_app, a.param_freq, [&](int c) { return param(a.n_geo + c); });   // model.py:96-101
        if (valid && h == 0) args.dists[(size_t)ray * a.S + s] = IPE ? segment_dist(e0, e1, hit, rc.dn) : sample_dist(zray, s, a.S, z, hit, rc.dn);
    }
}

// The same operands for an instanced step (ntx_train_forward_instanced): compact row blk * 32 + n is live sample m = live[row] of the
// instancer's buffers -- pos_map = FourierFeatures(pts[m]) | FourierFeatures(geometry parameters), dir_map = FourierFeatures(rays_d_map[m]) |
// FourierFeatures(appearance parameters): the direction as given (renderer.py:265-272 hands it on un-normalised), the parameters params_map[m]
// with column blur_idx times cone_scale t / patch_scale (:259-263).  Lane (n, h) as in encode_kernel, every value ntx_encode.h's: the features
// flex_encode_samples_kernel feeds, bit for bit.  The tail of the last block is written as zeros; a lane of the tail reads nothing -- not
// live[] beyond n_live, nor anything of the caller's, which is read at live samples alone.  The distances stay the caller's.
struct EncodeSamplesArgs { StepSamples s; float *posO; int ptiles; float *dirO; int dtiles; };
__global__ __launch_bounds__(64) void encode_samples_kernel(EncodeSamplesArgs args) {
    const StepSamples &a = args.s;
    const int lane = threadIdx.x, n = lane & 31, h = lane >> 5, blk = blockIdx.x, part = blockIdx.y;
    const long long row = (long long)blk * 32 + n;
    const bool valid = row < a.n_live;
    const long long m = valid ? a.live[row] : 0, ray = m / a.S;
    const int P = a.n_geo + a.n_app;
    auto param = [&](int col) {
        if (!valid) return 0.0f;
        const float p = a.params_map[(size_t)m * P + col];
        return col == a.blur_idx ? p * a.blur_scale(m, ray) : p;
    };
    float *O = part == 0 ? args.posO : args.dirO;
    const int tiles = part == 0 ? args.ptiles : args.dtiles;
    auto put = [&](int r, float v) { O[o_index(blk, tiles, r, n)] = valid ? v : 0.0f; };
    auto fourier = [&](int r0, int D, int L, auto x) {
        if (h == 0) for (int c = 0; c < D; ++c) put(r0 + c, x(c));
        for (int f = 0; f < L; ++f)
            for (int c = 0; c < D; ++c) put(r0 + fourier_row_of(D, f, h, c), fourier_value(x(c), f, h));
    };
    const float *xyz = part == 0 ? a.pts : a.rays_d_map;
    const float x3[3] = {valid ? xyz[3 * m] : 0.0f, valid ? xyz[3 * m + 1] : 0.0f, valid ? xyz[3 * m + 2] : 0.0f};
    const int L3 = part == 0 ? a.pos_freq : a.dir_freq, D = part == 0 ? a.n_geo : a.n_app, c0 = part == 0 ? 0 : a.n_geo;
    fourier(0, 3, L3, [&](int c) { return c == 0 ? x3[0] : c == 1 ? x3[1] : x3[2]; });
    if (D > 0) fourier(fourier_width(3, L3), D, a.param_freq, [&](int c) { return param(c0 + c); });
}
// ... and the narrow heads' dY of its way back: inst_composite_adjoint_kernel (ntx_trainer.hip, the layer-by-layer step's too) leaves the
// row-major dgrad [n_live][4] alone; the weight gradients read rows 0 .. 3 of one O-layout tile per block (dhead_at).  Thread per row of
// the n_live rows' blocks, the tail of the last block as zeros; rows 4 .. 31 of the tile are never written: zero as at allocation.
__global__ __launch_bounds__(256) void dhead_rows_kernel(const float *__restrict__ dgrad, long long n_live, float *__restrict__ dhead) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= (n_live + 31) / 32 * 32) return;
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4 g = m < n_live ? *reinterpret_cast<const f32x4 *>(dgrad + 4 * m) : zero;
    dhead[o_index(m >> 5, 1, 0, (int)(m & 31))] = g.x; dhead[o_index(m >> 5, 1, 1, (int)(m & 31))] = g.y;
    dhead[o_index(m >> 5, 1, 2, (int)(m & 31))] = g.z; dhead[o_index(m >> 5, 1, 3, (int)(m & 31))] = g.w;
}

// The colour layer's direction segment once per ray (fwd_chain_kernel's HOIST builds): row[f] = bias_C1[f] + sum_k dir_map[k] W_C1[k][f] over
// the Kd rows of dir_map = FourierFeatures(direction) | FourierFeatures(appearance parameters) (model.py:96-101, 115), written in the
// accumulators' order [ray][half h][16 T + 4 g + c] for feature 32 T + 8 g + 4 h + c.  Workgroup per ray, thread per output feature.
// splice >= 0 (the MipRenderer): the parameter rows hold P + 1 values and model parameter k is column k < splice ? k : k + 1 (ntx_encode.h spliced_param).
struct DirRowArgs {
    StepRays r; int Kd, splice;
    const float *w, *bias;                     // W_C1 [Kd + 256][256] (its first Kd rows), bias_C1 [256]
    float *rows;
};
__global__ __launch_bounds__(256) void dirrow_kernel(DirRowArgs a) {
    __shared__ float feat[8 * MAX_PB_GROUPS];
    const int ray = blockIdx.x, f = threadIdx.x;
    const RayCtx r = ray_ctx(a.r.rays_d, a.r.params, a.r.rays_per_param_row, ray, a.r.n_geo + a.r.n_app + (a.splice >= 0 ? 1 : 0));
    if (f < a.Kd) {                                                                             // row f of dir_map, as encode_kernel lays it out
        const int K3 = fourier_width(3, a.r.dir_freq);
        const bool xyz = f < K3;
        feat[f] = fourier_row(xyz ? f : f - K3, xyz ? 3 : a.r.n_app, [&](int c) { return xyz ? r.dir(c) : spliced_param(r.pr, a.r.n_geo + c, a.splice); });   // model.py:96-101
    }
    __syncthreads();
    float acc = a.bias[f];
    for (int k = 0; k < a.Kd; ++k) acc = fmaf(feat[k], a.w[(size_t)k * 256 + f], acc);
    const int T = f >> 5, g = (f >> 3) & 3, h = (f >> 2) & 1, c = f & 3;
    a.rows[(size_t)ray * 256 + h * 128 + 16 * T + 4 * g + c] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The gradient at the encoded inputs (ntx_trainer_enable_gradients): the three products the chain back leaves out -- dX of trunk layer 0, the
// skip layer's pos_map rows, C1's dir_map rows --
//     G[m][j] = sum over the terms (dY, W) of sum_o dY[m][o] W[j][o],     j < K
// G_pos: (dy0, W_trunk0), (dy5, W_trunk5), K = Kp;  G_dir: (dc1o, W_c1), K = Kd.  dY: the kept O-layout gradients (256 rows), W: the first K
// rows of the layer's kernel in the Keras-order blob, row j contiguous over o.  Output row-major [M][ld], ld = K padded to 4 (the padding
// columns are written as zeros): what flex_param_fold_kernel / flex_ray_fold_kernel read.
// A wave per block of 32 samples on v_mfma_f32_32x32x2_f32, transposed like the chains: G^T[j, sample] = W[j, o] . dY^T[o, sample], NT tiles
// of 32 rows j.  A operand: lane (j, kh) loads 16 bytes W[j][8 q + 4 kh + (0..3)] = four k-steps; B operand: lane (n, kh) gathers dwords
// dY[row 8 q + 4 kh + c][sample n] of the O-layout block -- the very addresses dx_chain_kernel's lane (n, kh) stored its value V = 4 q + c
// to (o_lane_bytes + o_value_bytes).  Rows j >= K lie beyond the weight resource's end and read as 0.  D of a tile: lane (n, h) holds rows
// 8 g + 4 h + (0..3) in registers 4 g .. 4 g + 3: four consecutive j of sample n, one 16-byte store.  Rows m >= M are not written.
// The order of a sum: from 0, the terms in the order given, within a term k-step V = 0 .. 127 ascending, within a k-step feature
// hidden_row(V, 0) then hidden_row(V, 1) (the MFMA's k = 0, 1): one fmaf chain per output, whatever the grid and the trainer's capacity.
// No atomics.  The grid is persistent (ChainBackend::feat_grid): wave w takes the blocks w, w + n_waves, ...
// ---------------------------------------------------------------------------------------------------------------------------
struct FeatGradArgs {
    const float *dY[2], *W[2]; int n_terms;   // a term's dY: O layout, 8 tiles a block; W: [K][256]
    int K, ld; long long M;
    float *G;                                  // [M][ld]
};
template <int NT>
__global__ __launch_bounds__(256) void feat_grad_kernel(FeatGradArgs a) {
    const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), nwaves = gridDim.x * 4;
    const int n_blocks = (int)((a.M + 31) >> 5);
    const uint32_t voff_y = o_lane_bytes(lane);
    uint32_t voff_w[NT];
    static_for<NT>([&](auto T) { constexpr int t = T; voff_w[t] = (uint32_t)(32 * t + n) * 1024u + (uint32_t)h * 16u; });
    for (int blk = wave; blk < n_blocks; blk += nwaves) {
        f32x16 acc[NT];
        static_for<NT>([&](auto T) { acc[T] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; });
        for (int term = 0; term < a.n_terms; ++term) {
            const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.W[term], (long long)a.K * 1024);
            const __amdgpu_buffer_rsrc_t ry = make_rsrc(a.dY[term] + (size_t)blk * 8 * 1024, 8 * 4096);
            // groups of four 16-byte steps (16 k-steps = one tile of dY's rows), one group ahead of the MFMAs
            f32x4 wa[2][4][NT]; float yb[2][16];
            auto fetch = [&](auto BUF, int grp) {
                constexpr int buf = BUF;
                static_for<4>([&](auto Q) {
                    constexpr int q = Q;
                    static_for<NT>([&](auto T) {
                        wa[buf][q][T] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, voff_w[T], (uint32_t)(4 * grp + q) * 32u, 0)); });
                    static_for<4>([&](auto Cc) {
                        constexpr int c = Cc;
                        yb[buf][4 * q + c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, voff_y, (uint32_t)grp * 4096u + o_value_bytes(4 * q + c), 0)); });
                });
            };
            auto compute = [&](auto BUF) {
                constexpr int buf = BUF;
                static_for<4>([&](auto Q) { static_for<4>([&](auto Cc) { static_for<NT>([&](auto T) {
                    constexpr int q = Q, c = Cc;
                    acc[T] = mfma32(wa[buf][q][T][c], yb[buf][4 * q + c], acc[T]);
                }); }); });
            };
            // (unconditional fetches, as in dw_piece: behind the last group it is asked for again and not used)
            fetch(std::integral_constant<int, 0>{}, 0);
            for (int grp = 0; grp < 8; grp += 2) {
                fetch(std::integral_constant<int, 1>{}, grp + 1);
                compute(std::integral_constant<int, 0>{});
                fetch(std::integral_constant<int, 0>{}, grp + 2 < 8 ? grp + 2 : grp + 1);
                compute(std::integral_constant<int, 1>{});
            }
        }
        const long long m = (long long)blk * 32 + n;
        if (m < a.M) {
            float *row = a.G + (size_t)m * a.ld;
            static_for<NT>([&](auto T) { static_for<4>([&](auto Gq) {
                constexpr int t = T, g = Gq;
                const int j = 32 * t + 8 * g + 4 * h;
                if (j < a.ld) *reinterpret_cast<f32x4 *>(row + j) = f32x4{acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]};
            }); });
        }
    }
}

}   // namespace ntx_train
namespace {
using namespace ntx_train;
struct ChainBackend : Backend {
    ntx_trainer *t = nullptr;
    int ptiles = 0, dtiles = 0, PS = 0, DS = 0, fwd_variant = 0;   // pos_map / dir_map: tiles of 32 rows of their buffers, k-steps of their segments; the forward chain's build
    TLayer trunk[8], feature, c1, c2, rgb, alpha;
    float *wfwd = nullptr, *wdx = nullptr, *aux = nullptr; size_t fwd_floats = 0, dx_floats = 0;      // what pack_kernel makes of the weights once a step: the two streams and the aux block
    PackSeg *pack_seg = nullptr; int n_pack = 0; long long pack_total = 0;
    float *posO = nullptr, *dirO = nullptr;               // forward: the encoded inputs and every layer's output (O layout), the ReLU bits
    float *act = nullptr; long long act_stride = 0;       // eleven matrices act + i * act_stride: h0 .. h7, feature, c1o, c2o
    unsigned int *bits = nullptr; long long bits_stride = 0;   // ten: h0 .. h7, c1o, c2o
    float *dirrow = nullptr;                   // [max_rays][256]: the colour layer's direction segment per ray (dirrow_kernel)
    float *gout = nullptr; long long gout_stride = 0;     // backward: the gradient at every layer's output (O layout: d c2o, d c1o, d feature, dy7 .. dy0)
    DwJob *jobs = nullptr; int n_jobs = 0; long long total_cost = 0;      // the weight gradients' jobs (ntx_train_device.h), their costs per block added up
    std::vector<DwJob> jobs_host; std::vector<int> reduce_job;      // reduce_job[i]: the job whose slots reduction i adds up
    float *dw_partial = nullptr; ReduceBatch reduce{};     // (n_split per step)
    float *G_pos = nullptr, *G_dir = nullptr; int ld_pos = 0, ld_dir = 0;      // ntx_trainer_enable_gradients: the gradient at pos_map / dir_map [cap][pad4(Kp / Kd)] (feat_grad_kernel)
    float *ray_pg = nullptr;                   // [cap_rays][P]: a ray's samples folded and added
    float *act_at(int i) const { return act + (size_t)i * act_stride; }
    float *gout_at(int i) const { return gout + (size_t)i * gout_stride; }
    bool samples_on = false;                   // ntx_trainer_enable_instanced: the handle takes instanced steps
    static int blocks_of(long long rows) { return (int)((rows + 31) / 32); }
    unsigned chain_grid(long long rows) const { return (unsigned)std::min<long long>(t->cus, (blocks_of(rows) + 3) / 4); }      // persistent: a workgroup of four waves per CU
    unsigned feat_grid(long long rows) const { return (unsigned)std::min<long long>(2 * (long long)t->cus, (blocks_of(rows) + 3) / 4); }   // persistent: two workgroups of four waves per CU
    size_t plan_layers(const ntx_model_desc &d, bool ipe);
    void build_pack();
    void build_dw_jobs();
    int forward(const StepRays &r, hipStream_t st) override;
    int backward(const StepRays &r, hipStream_t st) override;
    void launch_pack(hipStream_t st);
    FwdArgs fwd_args(long long M) const;
    void backward_network(long long M, hipStream_t st);
    void backward_weights(int n_blocks, hipStream_t st);
    int takes_samples() override { return samples_on ? NTX_OK : Backend::takes_samples(); }
    int enable_samples() override;
    int forward_samples(const StepSamples &s, hipStream_t st) override;
    int backward_samples(const StepSamples &s, float *sample_pg, hipStream_t st) override;
    int enable_gradients(int param_mode, int input_mode) override;
    void launch_feat_grad(hipStream_t st, unsigned grid, int tiles, const FeatGradArgs &a);
    int activation(int layer, int64_t n_samples_total, float *out_host) override;
};

// the forward chain's build for the model's segment lengths, or the longest one (the streams are then padded with zero rows), and the layers'
// places in the Keras-order blob; returns the blob's floats
size_t ChainBackend::plan_layers(const ntx_model_desc &d, bool ipe) {
    const ntx::BlobView n = ntx::view_blob(ntx::tuned_arch(1), ntx::dims_of(&d), ipe);
    const int Kp = n.pos_map, Kd = n.dir_map;
    ptiles = (Kp + 31) / 32; dtiles = (Kd + 31) / 32;
    const int psg = ((Kp + 1) / 2 + 3) / 4, dsg = ((Kd + 1) / 2 + 3) / 4;
    fwd_variant = 3;                                     // the smallest build that holds both segments
    for (int v = 2; v >= 0; --v)
        if (FWD_VARIANTS[v][0] >= psg && FWD_VARIANTS[v][1] >= dsg &&
            FWD_VARIANTS[v][0] + FWD_VARIANTS[v][1] <= FWD_VARIANTS[fwd_variant][0] + FWD_VARIANTS[fwd_variant][1]) fwd_variant = v;
    PS = 4 * FWD_VARIANTS[fwd_variant][0]; DS = 4 * FWD_VARIANTS[fwd_variant][1];
    std::copy(n.trunk.begin(), n.trunk.end(), trunk);
    feature = n.feature; c1 = n.colour[0]; c2 = n.c2; rgb = n.rgb; alpha = n.alpha;
    return n.count;
}

// the two weight streams and the aux block: what lies where, and what pack_kernel gathers it from
void ChainBackend::build_pack() {
    const int Kp = t->Kp, Kd = t->Kd;
    enum { FWD = 0, DX = 1, AUX = 2 };
    std::vector<PackSeg> segs; std::vector<int> base_of;                   // a segment's dst is an offset into buffer base_of[] until the buffers exist
    size_t floats[2] = {0, 0};
    long long first = 0;
    auto push = [&](PackSeg s, int base, size_t at, long long count) {
        s.count = count; s.first = first; s.dst = (float *)(uintptr_t)(at * sizeof(float));
        first += count; segs.push_back(s); base_of.push_back(base);
    };
    auto seg = [&](const float *src, long long sk, long long sc, int mode, int K, int ncols, int nt, int stream, int nsteps) {
        PackSeg s{}; s.src = src; s.sk = sk; s.sc = sc; s.mode = mode; s.K = K; s.ncols = ncols; s.nt = nt;
        const int ring = stream == DX ? DX_RING : RING;                                   // a segment is whole turns of its chain's ring
        const long long recs = ((long long)nsteps * (nt / 4) + ring - 1) / ring * ring;
        push(s, stream, floats[stream], recs * 256); floats[stream] += (size_t)recs * 256;
    };
    const float *W = t->w;
    // forward (model.py:104-123): W_l[k][col] row-major, k in the order of the layer's input
    auto fwd_hidden = [&](const TLayer &l, int row0, int nt) { seg(W + l.w + (size_t)row0 * l.out, l.out, 1, PACK_HIDDEN, 256, l.out, nt, FWD, 128); };
    auto fwd_linear = [&](const TLayer &l, int K, int nsteps) { seg(W + l.w, l.out, 1, PACK_LINEAR, K, l.out, 8, FWD, nsteps); };
    fwd_linear(trunk[0], Kp, PS);
    for (int i = 1; i < 8; ++i) {
        if (i == 5) { fwd_linear(trunk[5], Kp, PS); fwd_hidden(trunk[5], Kp, 8); }
        else fwd_hidden(trunk[i], 0, 8);
    }
    fwd_hidden(feature, 0, 8);
    fwd_linear(c1, Kd, DS); fwd_hidden(c1, Kd, 8);
    fwd_hidden(c2, 0, 4);
    const size_t n_fwd_segs = segs.size();
    // backward: row(s, kh) runs over the layer's OUTPUTS (what the lane holds of dY), the columns over its inputs: Wsrc[k][col] = W_l[col][k]
    auto dx_hidden = [&](const TLayer &l, int row0, int K, int nsteps) { seg(W + l.w + (size_t)row0 * l.out, 1, l.out, PACK_HIDDEN, K, 256, 8, DX, nsteps); };
    seg(W + rgb.w, 1, 3, PACK_LINEAR, 3, 128, 4, DX, 2);                      // d c2o = d raw . W_rgb^T
    dx_hidden(c2, 0, 128, 64);                                                // d c1o = d c2o . W_c2^T
    dx_hidden(c1, Kd, 256, 128);                                              // d feature = d c1o . W_c1[the feature rows]^T
    dx_hidden(feature, 0, 256, 128);                                          // d h7 = d feature . W_feature^T
    seg(W + alpha.w, 1, 1, PACK_LINEAR, 1, 256, 8, DX, 1);                    //        + d_sigma (x) W_alpha (model.py:111)
    for (int i = 7; i >= 1; --i) dx_hidden(trunk[i], i == 5 ? Kp : 0, 256, 128);  // d h(i-1) = dy_i . W_i^T (the skip's position rows take no gradient further)
    // a stream ends with its first RING records again
    auto tail = [&](size_t of, int stream) { const long long count = (long long)(stream == DX ? DX_RING : RING) * 256; push(segs[of], stream, floats[stream], count); floats[stream] += (size_t)count; };
    tail(0, FWD); tail(n_fwd_segs, DX);
    // aux: biases of the eleven layers in accumulator order, the density head's weights and bias, the colour head's
    auto aux_seg = [&](const float *src, int mode, int K, long long count, size_t at) { PackSeg s{}; s.src = src; s.sk = 1; s.mode = mode; s.K = K; push(s, AUX, at, count); };
    for (int i = 0; i < 8; ++i) aux_seg(W + trunk[i].b, PACK_AUX_ROW, 256, 256, AUX_BIAS + (size_t)i * 256);
    aux_seg(W + feature.b, PACK_AUX_ROW, 256, 256, AUX_BIAS + 8 * 256); aux_seg(W + c1.b, PACK_AUX_ROW, 256, 256, AUX_BIAS + 9 * 256);
    aux_seg(W + c2.b, PACK_AUX_ROW, 128, 256, AUX_BIAS + 10 * 256);
    aux_seg(W + alpha.w, PACK_AUX_ROW, 256, 256, AUX_ALPHA_W); aux_seg(W + alpha.b, PACK_COPY, 1, 1, AUX_ALPHA_B);
    aux_seg(W + rgb.w, PACK_AUX_RGB, 128, 384, AUX_RGB_W); aux_seg(W + rgb.b, PACK_COPY, 3, 3, AUX_RGB_B);
    pack_total = first; n_pack = (int)segs.size(); fwd_floats = floats[FWD]; dx_floats = floats[DX];
    t->mem.alloc(&wfwd, fwd_floats); t->mem.alloc(&wdx, dx_floats); t->mem.alloc(&aux, AUX_FLOATS, true);
    float *const base[3] = {wfwd, wdx, aux};
    for (size_t i = 0; i < segs.size(); ++i) segs[i].dst = (float *)((char *)base[base_of[i]] + (uintptr_t)segs[i].dst);
    t->mem.upload(&pack_seg, segs, "segment");
}

// the weight gradients' jobs: dW_l = X_l^T . dY_l, X_l = the O-layout input of layer l, dY_l = the gradient at its output.  A job =
// four waves side by side on the same blocks of samples (ntx_train_device.h); a slot of its partial sums holds the matrices its waves write
void ChainBackend::build_dw_jobs() {
    const int Kp = t->Kp, Kd = t->Kd;
    std::vector<DwJob> &jobs = jobs_host;
    struct RJ { int job; long long at, count, pair; size_t out; };
    std::vector<RJ> rjobs;
    auto new_job = [&]() { DwJob j{}; for (DwWave &w : j.w) w.shape = -1; jobs.push_back(j); return (int)jobs.size() - 1; };
    // a matrix of the job's slot: the [K][N] kernel gradient, behind it (g_bias >= 0) the [2][N] halves of the bias gradient
    auto matrix = [&](int j, int K, int N, size_t g_kernel, long long g_bias, long long *at_bias) {
        const long long at = jobs[j].slot_floats;
        jobs[j].slot_floats += (long long)K * N;
        rjobs.push_back(RJ{j, at, (long long)K * N, 0, g_kernel});
        *at_bias = -1;
        if (g_bias >= 0) { *at_bias = jobs[j].slot_floats; jobs[j].slot_floats += 2 * N; rjobs.push_back(RJ{j, *at_bias, N, N, (size_t)g_bias}); }
        return at;
    };
    auto wave = [&](int j, int w, int shape, const float *A, int rtA, int a0, const float *B, int rtB, int b0, long long at, int K, int N, int c_lo, long long at_bias) {
        DwWave &d = jobs[j].w[w];
        d.A = A; d.rtA = rtA; d.a0 = a0; d.B = B; d.rtB = rtB; d.b0 = b0; d.shape = shape; d.out = at; d.ldc = N; d.row0 = a0 * 32; d.rows_valid = K;
        d.col0 = b0 * 32; d.c_lo = c_lo; d.c_hi = c_lo + N; d.bias_out = a0 == 0 ? at_bias : -1;
        // a block's cost in MFMAs of the full shape: 16 k-steps x 16 tiles = 256; the narrower shapes load more per MFMA (7 tiles for 12, 5 for 4) and
        // run 3 % / 6 % behind their MFMA counts (192, 64): measured per block with the kernel's clock probe (-DNTX_TRAIN_CLOCKS)
        const int cost = shape == 0 ? 256 : shape == 1 ? 198 : 68;
        if (cost > jobs[j].cost) jobs[j].cost = cost;
    };
    // a 256 x 256 layer: wave w takes X tiles 4 (w >> 1) .., dY tiles 4 (w & 1) ..
    auto layer_job = [&](const float *X, const float *dY, size_t g_kernel, size_t g_bias) {
        const int j = new_job(); long long ab; const long long at = matrix(j, 256, 256, g_kernel, (long long)g_bias, &ab);
        for (int w = 0; w < 4; ++w) wave(j, w, 0, X, 8, 4 * (w >> 1), dY, 8, 4 * (w & 1), at, 256, 256, 0, ab);
    };
    for (int i = 7; i >= 1; --i) layer_job(act_at(i - 1), gout_at(10 - i), trunk[i].w + (size_t)(i == 5 ? Kp : 0) * 256, trunk[i].b);    // trunk 7 .. 1 (the skip: its h4 rows)
    layer_job(act_at(7), gout_at(2), feature.w, feature.b);                         // feature layer: X = h7
    layer_job(act_at(8), gout_at(1), c1.w + (size_t)Kd * 256, c1.b);                // C1: the feature rows of X = [dir_map | feature]
    {   // the position rows: trunk 0 (X = pos_map) and the skip (X = [pos_map | h4]); up to three tiles of rows x two halves of the columns
        const int j = new_job(); long long ab0, ab5;
        const long long at0 = matrix(j, Kp, 256, trunk[0].w, (long long)trunk[0].b, &ab0), at5 = matrix(j, Kp, 256, trunk[5].w, -1, &ab5);
        for (int w = 0; w < 2; ++w) { wave(j, w, 1, posO, ptiles, 0, gout_at(10), 8, 4 * w, at0, Kp, 256, 0, ab0); wave(j, 2 + w, 1, posO, ptiles, 0, gout_at(5), 8, 4 * w, at5, Kp, 256, 0, ab5); }
    }
    {   // C1's direction rows (X = dir_map) beside C2 (X = c1o, dY 128 wide)
        const int j = new_job(); long long abd, ab2;
        const long long atd = matrix(j, Kd, 256, c1.w, -1, &abd), at2 = matrix(j, 256, 128, c2.w, (long long)c2.b, &ab2);
        for (int w = 0; w < 2; ++w) { wave(j, w, 1, dirO, dtiles, 0, gout_at(1), 8, 4 * w, atd, Kd, 256, 0, abd); wave(j, 2 + w, 0, act_at(9), 8, 4 * w, gout_at(0), 4, 0, at2, 256, 128, 0, ab2); }
    }
    {   // the narrow heads: X = c2o against d raw (columns 0-2 of the heads' tile), X = h7 against d sigma (column 3)
        const int j = new_job(); long long abr, aba;
        const long long atr = matrix(j, 128, 3, rgb.w, (long long)rgb.b, &abr), ata = matrix(j, 256, 1, alpha.w, (long long)alpha.b, &aba);
        wave(j, 0, 2, act_at(10), 4, 0, t->dhead, 1, 0, atr, 128, 3, 0, abr);
        for (int w = 0; w < 2; ++w) wave(j, 1 + w, 2, act_at(7), 8, 4 * w, t->dhead, 1, 0, ata, 256, 1, 3, aba);
    }
    n_jobs = (int)jobs.size();
    size_t partial_floats = 0;
    for (DwJob &j : jobs) total_cost += j.cost;
    for (DwJob &j : jobs) {                                  // a job fills at most its share of the workgroups' slots (+ the two it may share with its neighbours)
        const long long slots = ((long long)j.cost * t->cus + total_cost - 1) / total_cost + 2;
        j.first_float = (long long)partial_floats; partial_floats += (size_t)(slots * j.slot_floats);
    }
    t->mem.alloc(&dw_partial, partial_floats);
    t->mem.upload(&this->jobs, jobs, "job");
    if (t->mem.rc == NTX_OK && (int)rjobs.size() > MAX_REDUCE_BATCH) t->mem.rc = ntx_set_error(NTX_E_INVALID, "trainer: too many weight gradients for one launch");
    long long rfirst = 0;
    for (size_t i = 0; i < rjobs.size() && t->mem.rc == NTX_OK; ++i) {
        ReduceJob &r = reduce.job[reduce.n++];
        const DwJob &j = jobs[rjobs[i].job];
        r.partial = dw_partial + j.first_float + rjobs[i].at; r.n_split = 0; r.stride = j.slot_floats; r.count = rjobs[i].count; r.pair = rjobs[i].pair;
        r.out = t->grad + rjobs[i].out; r.first = rfirst;
        rfirst += (rjobs[i].count + 255) / 256 * 256;
        reduce_job.push_back(rjobs[i].job);
    }
}

void ChainBackend::launch_pack(hipStream_t st) {
    const PackArgs pa{pack_seg, n_pack, pack_total};
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((pack_total + 255) / 256)), dim3(256), 0, st, pa);
}
// the forward chain's arguments on M rows, less the direction hoist's
FwdArgs ChainBackend::fwd_args(long long M) const {
    FwdArgs f{}; f.stream = wfwd; f.stream_bytes = (uint32_t)(fwd_floats * sizeof(float)); f.aux = aux; f.M = M;
    f.ptiles = ptiles; f.dtiles = dtiles; f.pos = posO; f.dir = dirO;
    f.act = act; f.act_stride = act_stride; f.bits = bits; f.bits_stride = bits_stride;
    f.sigma = t->sigma; f.raw_rgb = t->raw_rgb;
    return f;
}
int ChainBackend::forward(const StepRays &r, hipStream_t st) {
    launch_pack(st);
    EncodeArgs e{}; e.r = r; e.posO = posO; e.ptiles = ptiles; e.dirO = dirO; e.dtiles = dtiles; e.dists = t->dists;
    if (t->ipe) hipLaunchKernelGGL(encode_kernel<true>, dim3((unsigned)r.n_blocks(), 2), dim3(64), 0, st, e);
    else hipLaunchKernelGGL(encode_kernel<false>, dim3((unsigned)r.n_blocks(), 2), dim3(64), 0, st, e);
    FwdArgs f = fwd_args(r.M());
    // the direction segment of the colour layer per ray instead of per sample -- unless blur_idx scales an APPEARANCE parameter per sample
    // (renderer.py:155-158) or a block of 32 samples can lie in two rays (S no multiple of 32).  Under the MipRenderer the parameters are
    // per-ray constants whatever blur_idx is (the blur is the cone's radius)
    const bool hoist = (t->ipe || r.blur_idx < 0 || r.blur_idx < r.n_geo) && r.S % 32 == 0 && getenv("NERFTEX_TRAIN_NO_DIR_HOIST") == nullptr;
    if (hoist) {
        DirRowArgs dr{}; dr.r = r; dr.Kd = t->Kd; dr.w = t->w + c1.w; dr.bias = t->w + c1.b; dr.rows = dirrow; dr.splice = t->ipe ? r.blur_idx : -1;
        hipLaunchKernelGGL(dirrow_kernel, dim3((unsigned)r.n_rays), dim3(256), 0, st, dr);
    }
    f.dirrow = dirrow; f.n_rays = (int)r.n_rays; f.S = r.S;
    launch_fwd_chain(fwd_variant, hoist, st, chain_grid(r.M()), f);
    return NTX_OK;
}
// An instanced step: the same chain on the n_live compact rows of the step's live samples (none: nothing is launched).  Every sample has a
// direction and appearance parameters of its own (rays_d_map, params_map), so the colour layer's direction segment is per sample: the build
// without the hoist, the one S % 32 != 0 and an appearance blur_idx already run
int ChainBackend::forward_samples(const StepSamples &s, hipStream_t st) {
    if (int rc = takes_samples()) return rc;
    const long long M = s.n_live;
    if (M == 0) return NTX_OK;
    launch_pack(st);
    EncodeSamplesArgs e{}; e.s = s; e.posO = posO; e.ptiles = ptiles; e.dirO = dirO; e.dtiles = dtiles;
    hipLaunchKernelGGL(encode_samples_kernel, dim3((unsigned)blocks_of(M), 2), dim3(64), 0, st, e);
    FwdArgs f = fwd_args(M);
    f.dirrow = dirrow; f.n_rays = (int)s.n_rays; f.S = s.S;                  // (not read without the hoist)
    launch_fwd_chain(fwd_variant, false, st, chain_grid(M), f);
    return NTX_OK;
}

#ifdef NTX_TRAIN_CLOCKS
// development (tools/dev/README.md): every workgroup's pieces of the weight gradients' launch, in 100 MHz ticks from the earliest start, into
// the file NERFTEX_DW_CLOCKS names: the buffer dw_kernel writes them to (NULL when the variable is not set), and the dump behind the launch
unsigned long long *dw_clocks_buffer(long long G, int n_jobs, hipStream_t st) {
    static unsigned long long *clocks = nullptr;
    const size_t nck = (size_t)G * (2 + 3 * n_jobs);
    if (!getenv("NERFTEX_DW_CLOCKS")) return nullptr;
    if (!clocks) (void)hipMalloc((void **)&clocks, nck * sizeof(unsigned long long));
    (void)hipMemsetAsync(clocks, 0, nck * sizeof(unsigned long long), st);
    return clocks;
}
void dump_dw_clocks(const unsigned long long *clocks, long long G, const std::vector<DwJob> &jobs, hipStream_t st) {
    const int n_jobs = (int)jobs.size();
    const size_t nck = (size_t)G * (2 + 3 * n_jobs);
    std::vector<unsigned long long> h(nck);
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(h.data(), clocks, nck * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    unsigned long long t0 = ~0ull;
    for (long long g = 0; g < G; ++g) t0 = std::min(t0, h[g * (2 + 3 * n_jobs)]);
    FILE *f = fopen(getenv("NERFTEX_DW_CLOCKS"), "w");
    if (!f) return;
    for (long long g = 0; g < G; ++g) {
        const unsigned long long *c = &h[g * (2 + 3 * n_jobs)];
        fprintf(f, "%lld %llu %llu", g, c[0] - t0, c[1] - t0);
        for (int j = 0; j < n_jobs; ++j) if (c[4 + 3 * j]) fprintf(f, "  j%d cost %d blocks %llu %llu-%llu", j, jobs[j].cost, c[2 + 3 * j], c[3 + 3 * j] - t0, c[4 + 3 * j] - t0);
        fprintf(f, "\n");
    }
    fclose(f);
}
#endif

// the way back over M rows from the handle's dgrad [M][4] and its O-layout copy dhead: the chain back, the gradient at the encoded inputs
// where a mode asks for it, the weight gradients
void ChainBackend::backward_network(long long M, hipStream_t st) {
    DxArgs x{}; x.stream = wdx; x.stream_bytes = (uint32_t)(dx_floats * sizeof(float)); x.M = M; x.dgrad = t->dgrad;
    x.out = gout; x.out_stride = gout_stride; x.bits = bits; x.bits_stride = bits_stride;
    launch_dx_chain(st, chain_grid(M), x);
    if (t->pg_mode != 0 || t->ig_mode != 0) {                                // the gradient at pos_map and at dir_map, all Kp / Kd columns whichever mode asked
        FeatGradArgs p{}; p.dY[0] = gout_at(10); p.W[0] = t->w + trunk[0].w; p.dY[1] = gout_at(5); p.W[1] = t->w + trunk[5].w; p.n_terms = 2;
        p.K = t->Kp; p.ld = ld_pos; p.M = M; p.G = G_pos;
        launch_feat_grad(st, feat_grid(M), ptiles, p);
        FeatGradArgs d{}; d.dY[0] = gout_at(1); d.W[0] = t->w + c1.w; d.n_terms = 1; d.K = t->Kd; d.ld = ld_dir; d.M = M; d.G = G_dir;
        launch_feat_grad(st, feat_grid(M), dtiles, d);
    }
    if (t->takes_weight_gradients()) backward_weights(blocks_of(M), st);     // either mode 2: no weight gradient is taken or reduced
}
int ChainBackend::backward(const StepRays &r, hipStream_t st) {
    backward_network(r.M(), st);
    // the folds of the layer-by-layer backend: the parameter features' and the FF(xyz) / FF(dir) rows' gradient through the encoder
    if (t->pg_mode != 0) {
        const ntx_model_desc &m = t->desc;
        launch_param_fold(st, r, G_pos + 3 * (1 + 2 * m.pos_freq), G_dir + 3 * (1 + 2 * m.dir_freq), ld_pos, ld_dir, ray_pg, t->P, t->param_grad);
    }
    if (t->ig_mode != 0) launch_ray_fold(st, r, G_pos, G_dir, ld_pos, ld_dir, t->dgrad, t->sigma, t->step_noise, t->d_rays_o, t->d_rays_d);
    return NTX_OK;
}
// An instanced step's way back over its n_live rows, from the shared composite adjoint's dgrad.  Without a live sample nothing is contracted:
// every weight gradient is exactly 0 (mode 2 leaves the buffer alone, as ever), and the per-sample gradients are zeros.  The per-sample folds
// are the layer-by-layer backend's, on feat_grad_kernel's rows at row_of[m]
int ChainBackend::backward_samples(const StepSamples &s, float *sample_pg, hipStream_t st) {
    if (int rc = takes_samples()) return rc;
    const long long M = s.n_live;
    if (M > 0) {
        hipLaunchKernelGGL(dhead_rows_kernel, dim3((unsigned)((blocks_of(M) * 32 + 255) / 256)), dim3(256), 0, st, t->dgrad, M, t->dhead);
        backward_network(M, st);
    } else if (t->takes_weight_gradients()) TRAIN_TRY(hipMemsetAsync(t->grad, 0, t->n_weights * sizeof(float), st));
    const ntx_model_desc &m = t->desc;
    if (t->pg_mode != 0) launch_param_samples(st, s, G_pos + 3 * (1 + 2 * m.pos_freq), G_dir + 3 * (1 + 2 * m.dir_freq), ld_pos, ld_dir, t->P, sample_pg);
    if (t->ig_mode != 0) launch_input_samples(st, s, G_pos, G_dir, ld_pos, ld_dir, t->d_pts, t->d_dirs);
    return NTX_OK;
}
// ntx_trainer_enable_instanced: what an instanced step needs beyond the plain one's buffers is the compaction's maps and scan workspace, placed
// here for the trainer's capacity (the encoded inputs, the activations and the heads' tile are the plain step's, whose capacity covers any
// n_live).  A handle that never asks has none of it and refuses the step as before
int ChainBackend::enable_samples() {
    if (t->ipe) return ntx_set_error(NTX_E_UNSUPPORTED, "an instanced step of an IPE model: the instanced render has no cone segments (out of scope, as on the layer-by-layer trainer)");
    if (samples_on) return NTX_OK;
    TRAIN_TRY(hipSetDevice(t->device));
    if (int rc = t->place_sample_maps()) return rc;
    samples_on = true;
    return NTX_OK;
}
void ChainBackend::backward_weights(int n_blocks, hipStream_t st) {
    // every layer's dW = X^T . dY and db = the column sums of dY in one launch of one workgroup per CU, each with an equal share of the work ...
    DwArgs d{}; d.jobs = jobs; d.n_jobs = n_jobs; d.n_blocks = n_blocks; d.total_cost = total_cost; d.partial = dw_partial;
    const long long G = t->cus, W = total_cost * n_blocks;
#ifdef NTX_TRAIN_CLOCKS
    d.clocks = dw_clocks_buffer(G, n_jobs, st);
#endif
    launch_dw(st, (unsigned)G, d);
#ifdef NTX_TRAIN_CLOCKS
    if (d.clocks) dump_dw_clocks(d.clocks, G, jobs_host, st);
#endif
    // ... and the slots every job filled added up in a fixed order
    ReduceBatch rb = reduce;
    std::vector<int> slots(n_jobs);
    long long start = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const long long span = (long long)jobs_host[j].cost * n_blocks;
        slots[j] = (int)(dw_last_g(G, W, start, span) - dw_first_g(G, W, start) + 1);
        start += span;
    }
    for (int i = 0; i < rb.n; ++i) rb.job[i].n_split = slots[reduce_job[i]];
    launch_reduce(st, rb);
}

void ChainBackend::launch_feat_grad(hipStream_t st, unsigned grid, int tiles, const FeatGradArgs &a) {
    if (tiles <= 1) hipLaunchKernelGGL(feat_grad_kernel<1>, dim3(grid), dim3(256), 0, st, a);
    else if (tiles == 2) hipLaunchKernelGGL(feat_grad_kernel<2>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(feat_grad_kernel<3>, dim3(grid), dim3(256), 0, st, a);
}

// What dL/d params and dL/d rays need on the chain, placed at the first enable for the trainer's capacity: the gradient at the encoded
// inputs, a ray's and a row's parameter sums, the two ray results.  A handle that never enables anything has none of it
int ChainBackend::enable_gradients(int param_mode, int input_mode) {
    if (param_mode == 0 && input_mode == 0) return NTX_OK;
    if (t->ipe) return ntx_set_error(NTX_E_UNSUPPORTED, "parameter / input gradients of an IPE model on the fused chain: the cone gaussians' derivative is not written");
    if (G_pos) return NTX_OK;
    DeviceMemory &mem = t->mem;
    TRAIN_TRY(hipSetDevice(t->device));
    ld_pos = pad4(t->Kp); ld_dir = pad4(t->Kd);
    mem.alloc(&G_dir, (size_t)t->cap * ld_dir);
    mem.alloc(&ray_pg, (size_t)t->cap_rays * t->P); mem.alloc(&t->param_grad, (size_t)t->cap_rays * t->P);
    mem.alloc(&t->d_rays_o, (size_t)t->cap_rays * 3); mem.alloc(&t->d_rays_d, (size_t)t->cap_rays * 3);
    mem.alloc(&G_pos, (size_t)t->cap * ld_pos);                              // (last: it is the mark that all of it is placed)
    return mem.rc;
}

int ChainBackend::activation(int layer, int64_t n_samples_total, float *out_host) {
    const float *src = nullptr; int tiles = 8;
    if (layer >= 0 && layer < 8) src = act_at(layer);
    else if (layer == 8) src = act_at(9);
    else if (layer == 9) { src = act_at(10); tiles = 4; }
    else if (layer == 10) src = t->sigma;
    else if (layer >= 20 && layer < 28) src = gout_at(10 - (layer - 20));
    else if (layer == 28) src = gout_at(1);
    else if (layer == 29) src = gout_at(2);
    else if (layer == 11) src = t->raw_rgb;
    else if (layer == 30) src = t->dgrad;
    else if ((layer == 40 || layer == 41) && G_pos && ((t->pg_mode != 0 && (t->pg_rows > 0 || t->spg_rays > 0)) || (t->ig_mode != 0 && (t->ig_rays > 0 || t->ig_smp_rays > 0)))) src = layer == 40 ? G_pos : G_dir;
    else return ntx_set_error(NTX_E_INVALID, "layer %d (0-7 trunk, 8 / 9 the colour layers, 10 the density, 11 the raw colour; 20-29 the kept gradients, 30 the composite's adjoint; "
                              "40 / 41 the gradient at pos_map / dir_map of a step under ntx_trainer_enable_gradients)", layer);
    TRAIN_TRY(hipSetDevice(t->device));
    TRAIN_TRY(hipDeviceSynchronize());
    if (layer == 40 || layer == 41) {                                        // row-major [n][pad4(K)] -> [n][K]
        const int K = layer == 40 ? t->Kp : t->Kd, ld = layer == 40 ? ld_pos : ld_dir;
        TRAIN_TRY(hipMemcpy2D(out_host, (size_t)K * sizeof(float), src, (size_t)ld * sizeof(float), (size_t)K * sizeof(float), (size_t)n_samples_total, hipMemcpyDeviceToHost));
        return NTX_OK;
    }
    if (layer == 10 || layer == 11 || layer == 30) {
        const size_t width = layer == 10 ? 1 : (layer == 11 ? 3 : 4);
        TRAIN_TRY(hipMemcpy(out_host, src, (size_t)n_samples_total * width * sizeof(float), hipMemcpyDeviceToHost)); return NTX_OK;
    }
    // O layout -> [sample][feature]
    const long long nb = (n_samples_total + 31) / 32;
    std::vector<float> tmp((size_t)nb * tiles * 1024);
    TRAIN_TRY(hipMemcpy(tmp.data(), src, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
    const int width = tiles * 32;
    for (long long m = 0; m < n_samples_total; ++m)
        for (int row = 0; row < width; ++row) out_host[(size_t)m * width + row] = tmp[o_index(m >> 5, tiles, row, (int)(m & 31))];
    return NTX_OK;
}
}   // namespace
namespace ntx_train {
template <int K, bool HOIST> void launch_fwd_variant(hipStream_t st, unsigned grid, const FwdArgs &a);      // ntx_train_chain.hip, one object each
void launch_fwd_chain(int variant, bool hoist, hipStream_t st, unsigned grid, const FwdArgs &a) {
    static void (*const launch[8])(hipStream_t, unsigned, const FwdArgs &) = {launch_fwd_variant<0, false>, launch_fwd_variant<0, true>, launch_fwd_variant<1, false>, launch_fwd_variant<1, true>,
                                                                               launch_fwd_variant<2, false>, launch_fwd_variant<2, true>, launch_fwd_variant<3, false>, launch_fwd_variant<3, true>};
    launch[variant * 2 + (hoist ? 1 : 0)](st, grid, a);
}

int chain_check(const ntx_model_desc *desc, TrainDims *dims) {
    const bool ipe = desc->pos_encoding == NTX_POS_IPE && desc->n_pos == 6;        // MipRenderer + IntegratedPositionalEncoding (renderer.py:356-473)
    if (desc->kind != NTX_MODEL_PARAMNERF || desc->depth != 8 || desc->width != 256 || desc->skip != 4 || desc->color_depth != 1 ||
        !((desc->pos_encoding == NTX_POS_FOURIER && desc->n_pos == 3) || ipe))
        return ntx_set_error(NTX_E_UNSUPPORTED, "training is built for the ParamNerf architecture of the shipped training configs (depth 8, width 256, skips [4], color_depth 1, "
                                                "Fourier features on n_pos 3 or IPE on n_pos 6); other architectures train through ntx_trainer_create_flex");
    if (desc->n_geo < 0 || desc->n_app < 0 || desc->n_geo + desc->n_app > 16) return ntx_set_error(NTX_E_INVALID, "n_parameters out of range");
    if (desc->pos_freq < 0 || desc->dir_freq < 0 || desc->param_freq < 0) return ntx_set_error(NTX_E_INVALID, "negative band count");
    const int Kp = ntx::pos_map_m(ntx::dims_of(desc), ipe), Kd = ntx::dir_map_m(ntx::dims_of(desc));
    if (Kp > 8 * MAX_PB_GROUPS || Kd > 8 * MAX_PB_GROUPS)
        return ntx_set_error(NTX_E_UNSUPPORTED, "training: pos_map (%d) / dir_map (%d) wider than %d features (the chain holds a block's encoded inputs in registers)", Kp, Kd,
                             8 * MAX_PB_GROUPS);
    dims->desc = *desc; dims->Kp = Kp; dims->Kd = Kd; dims->ipe = ipe; dims->n_weights = ChainBackend().plan_layers(*desc, ipe);
    return NTX_OK;
}

int chain_backend_create(ntx_trainer *t) {
    ChainBackend *c = new ChainBackend();
    t->backend = c; c->t = t;
    c->plan_layers(t->desc, t->ipe);
    DeviceMemory &mem = t->mem;
    const long long NB = t->cap_blocks;
    // rows of the encoded inputs beyond Kp / Kd meet zero weights and are never written: they have to be finite
    mem.alloc(&c->posO, (size_t)NB * c->ptiles * 1024, true); mem.alloc(&c->dirO, (size_t)NB * c->dtiles * 1024, true);
    c->act_stride = c->gout_stride = NB * 8 * 1024; c->bits_stride = NB * 256;
    mem.alloc(&c->act, (size_t)c->act_stride * 11); mem.alloc(&c->bits, (size_t)c->bits_stride * 10); mem.alloc(&c->gout, (size_t)c->gout_stride * 11);
    mem.alloc(&c->dirrow, (size_t)t->cap_rays * 256);
    c->build_pack();
    c->build_dw_jobs();
    return mem.rc;
}
}   // namespace ntx_train
