// ntx_composite.h -- the volume-rendering composite of a training step (map_model_output, renderer.py:170-213, and InstanceRenderer's tail,
// renderer.py:318-354) and its adjoint, each formula stated once: ray_transmittance, ray_forward and ray_adjoint, templated on a RAY VIEW that
// supplies what differs between a whole ray of a plain step (WholeRay) and a ray of an instanced step (InstancedRay).  The five composite
// kernels of ntx_trainer.hip are made of these pieces.  A wave per ray, lane l holds samples l, l + 64, ...; el and T are the wave's two LDS
// rows of MAX_TRAIN_SAMPLES floats.  -ffp-contract=off: every fmaf below is meant, and nothing else is fused.
#pragma once
#include "ntx_trainer.h"
#include "ntx_encode.h"   // o_index
#include "ntx_device.h"   // f32x4
namespace ntx_train {
using ntx::f32x4;
// what both kinds of composite take, filled in one place on the host (composite_common)
struct CompositeCommon {
    const float *raw_rgb, *sigma;              // the network's raw outputs: [N][S][3], [N][S] of a plain step, [n_live][3], [n_live] in compact rows of an instanced one
    int map_exr, composite_bkgd; float bkgd[3];
    float *color, *alpha;                      // [N][3], [N]: the predictions
    float *weights;                            // NULL, or [N][S]: the composite's weights a_s T_s (what the importance sampler takes, renderer.py:127-128; the way
                                               // out for a loss on them); an instanced step's exactly 0 where a sample is not live and on a ray with hit == 0
    float *dgrad;                              // [M][4] ([n_live][4] in compact row order): dL/d raw rgb, dL/d sigma per sample (the way back starts from these)
};
struct CompositeArgs : CompositeCommon {
    const float *dists;                        // [N][S]
    const float *noise;                        // NULL, or [N][S]: raw_noise_std * N(0,1), added to the density before its ReLU (renderer.py:190-195)
    int n_rays, S;
    const float *color_true, *alpha_true;
    int kind, loss_fn, alpha_loss_fn, filter_color_loss, use_hard_mask; float gamma;
    float *ray_loss;                           // [N]: each ray's share of the loss
    float *dhead;                              // dgrad again as one O-layout tile per block of 32 samples (rows 0-2, 3): the narrow heads' dY
    long long M;
};
// The instanced composite: the network's raw outputs in compact rows, everything else in the caller's [N][S] buffers (StepSamples).  A ray with
// hit == 0 is 0 / 0, also under the background (:313-314): the kernels leave before they form a view of it.
struct InstCompositeArgs : CompositeCommon { StepSamples s; };

// The first statement of each composite kernel.  A wave reads its kernel arguments through the scalar cache, a line of 64 bytes at a time,
// as its code first needs them: the ray-index test waits for one line, the el fill for the next, and each new line is a round trip in front
// of all work -- 0.3 - 0.5 us of kernels of 10 us (profiles/composite_unify/timing.md: the parent's kernels happened to touch every line in
// their first wait, the shared pieces at first did not).  Naming one word of every line here makes the first wait fetch them together,
// wherever the fields lie; the values themselves are not used.
template <class Args> NTX_DEV void fetch_args(const Args &a) {
    const int *w = reinterpret_cast<const int *>(&a);
#pragma unroll
    for (size_t i = 0; i < sizeof(Args) / sizeof(int); i += 16) asm volatile("" ::"s"(w[i]));
}
NTX_DEV float rgb_of(float raw, int map_exr) {
    if (map_exr) return raw > 0.0f ? raw + 1.0f : expf(raw);                                   // elu + 1 (:184-185)
    return 1.0f / (1.0f + expf(-raw));                                                         // sigmoid (:187)
}
NTX_DEV size_t dhead_at(long long m, int row) { return o_index(m >> 5, 1, row, (int)(m & 31)); }

// ---- the two ray views ---------------------------------------------------------------------------------------------------------------------
// A view is built once per ray in front of the loops, so the ray's constants stay in registers across the stores.
// A plain step's ray: every sample is the network's (live() is a constant, the branches on it fold away), in [ray][s] order; nothing lies
// behind the ray's end, so the adjoint's carries stay at Z = 1, V = 0 and nothing is added to C or A.
struct WholeRay {
    const float *sg, *ds, *nz, *rr; float *weights, *dgrad, *dhead; long long m0; int S;
    NTX_DEV WholeRay(const CompositeArgs &a, int ray)
        : sg(a.sigma + (size_t)ray * a.S), ds(a.dists + (size_t)ray * a.S), nz(a.noise ? a.noise + (size_t)ray * a.S : nullptr), rr(a.raw_rgb + (size_t)ray * a.S * 3),
          weights(a.weights), dgrad(a.dgrad), dhead(a.dhead), m0((long long)ray * a.S), S(a.S) {}
    NTX_DEV int row(int s) const { return s; }                                                       // where sample s's raw outputs are
    static NTX_DEV bool live(int) { return true; }                                                   // whether it went through the network
    NTX_DEV float density(int s, int) const { return nz ? sg[s] + nz[s] : sg[s]; }                   // what enters the ReLU (:190-195)
    NTX_DEV float exponent(float r, int s) const { return -r * ds[s]; }                              // exp's argument, r = relu(density)
    NTX_DEV const float *raw(int row) const { return rr + 3 * row; }                                 // the three raw colours
    NTX_DEV float dsigma(int s, float d_a, float e) const { return d_a * ds[s] * e; }           // dL/d sigma where density > 0: da/dsigma = dist exp(-sigma dist)
    NTX_DEV void store(int s, int, const float (&g)[4]) const {                                      // where the four gradients go
        const long long m = m0 + s;
        *reinterpret_cast<f32x4 *>(dgrad + 4 * m) = f32x4{g[0], g[1], g[2], g[3]};
        for (int r = 0; r < 4; ++r) dhead[dhead_at(m, r)] = g[r];
    }
    NTX_DEV void close_forward(float (&)[3], float &, float) const {}                                // what lies behind sample S - 1: nothing
    NTX_DEV void close_adjoint(const float (&)[3], float &, float &) const {}
};
// An instanced step's ray with hit != 0.  Sample m = ray * S + s is live iff row_of[m] >= 0; a live sample: sigma' = sigma * alpha_weight *
// density_scale (:300; alpha_weight NULL: 1), a = 1 - exp(-relu(sigma') dists / patch_scale) (:339), its gradients to dgrad[row] alone.  A
// sample that is not live has a = 0 exactly.  One appended sample (color_last as is, alpha_last as an alpha) closes the ray (:331, :339):
// its weight wl = alpha_last * (the product of all S factors) is added to C and A (it is alpha_pred - sum_s w_s and is not stored), and the
// adjoint's carries start behind it, at V = (dC . color_last) alpha_last and Z = ((1 - alpha_last) + 1e-10) - 1e-10.  It has no stored weight
// and takes no weight cotangent.
struct InstancedRay {
    const int *rows; const float *sg, *ds, *aw, *rr, *color_last; float *weights, *dgrad; float al, patch_scale, density_scale; long long m0; int S;
    NTX_DEV InstancedRay(const InstCompositeArgs &a, long long ray)
        : rows(a.s.row_of + ray * a.s.S), sg(a.sigma), ds(a.s.dists + ray * a.s.S), aw(a.s.alpha_weight), rr(a.raw_rgb),
          color_last(a.s.color_last + 3 * ray), weights(a.weights), dgrad(a.dgrad), al(a.s.alpha_last[ray]), patch_scale(a.s.patch_scale),
          density_scale(a.s.density_scale), m0(ray * a.s.S), S(a.s.S) {}
    NTX_DEV int row(int s) const { return rows[s]; }
    static NTX_DEV bool live(int row) { return row >= 0; }
    NTX_DEV float density(int s, int row) const { return sg[row] * (aw ? aw[m0 + s] : 1.0f) * density_scale; }
    NTX_DEV float exponent(float r, int s) const { return -r * ds[s] / patch_scale; }
    NTX_DEV const float *raw(int row) const { return rr + 3 * (size_t)row; }
    NTX_DEV float dsigma(int s, float d_a, float e) const { return d_a * (ds[s] / patch_scale) * e * (aw ? aw[m0 + s] : 1.0f) * density_scale; }
    NTX_DEV void store(int, int row, const float (&g)[4]) const { *reinterpret_cast<f32x4 *>(dgrad + 4 * (size_t)row) = f32x4{g[0], g[1], g[2], g[3]}; }
    NTX_DEV void close_forward(float (&c)[3], float &A, float T_last) const {
        const float wl = al * T_last;
        A += wl;
        for (int k = 0; k < 3; ++k) c[k] += wl * color_last[k];
    }
    NTX_DEV void close_adjoint(const float (&dC)[3], float &Z, float &V) const {
        V = ((dC[0] * color_last[0] + dC[1] * color_last[1]) + dC[2] * color_last[2]) * al;
        Z = ((1.0f - al) + 1e-10f) - 1e-10f;
    }
};

// ---- the formulas, once ------------------------------------------------------------------------------------------------------------------
// el[s] = exp(-relu(density) length), 1 at a sample that is not live, and T[s], the exclusive running product, in the wave's two LDS rows.
// Returns the product of all S factors: the transmittance behind sample S - 1.
template <class View> NTX_DEV float ray_transmittance(const View &v, int lane, float *el, float *T) {
    const int S = v.S;
    // a_s = 1 - el[s] (:195), and the factor of the running product, (1 - a_s) + 1e-10 (:198), is taken as el[s] + 1e-10 -- the value of the
    // reference's expression without the float32 round trip through 1 - (1 - e), which on a saturated sample (e ~ 1e-6) leaves 1 - a with two
    // digits: the ray's transmittance, and with it every gradient behind the sample, would carry that error
    for (int s = lane; s < S; s += 64) {
        const int row = v.row(s);
        float e = 1.0f;
        if (View::live(row)) { const float d = v.density(s, row); const float r = d > 0.0f ? d : 0.0f; e = expf(v.exponent(r, s)); }
        el[s] = e;
    }
    __builtin_amdgcn_wave_barrier();
    // exclusive running product of (1 - a) + 1e-10, sequential like tf.math.cumprod (:198): chunks of 64 with a carry
    float carry = 1.0f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        float f = s < S ? el[s] + 1e-10f : 1.0f, incl = f;
        for (int o = 1; o < 64; o <<= 1) { const float w = __shfl_up(incl, o); if (lane >= o) incl *= w; }
        float excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 1.0f;
        if (s < S) T[s] = carry * excl;
        carry *= __shfl(incl, 63);
    }
    __builtin_amdgcn_wave_barrier();
    return carry;
}
// The forward of a ray: el and T, then the ray's colour c and opacity A (every lane ends with them) and the optional weights w_s = a_s T_s --
// exactly 0 at a sample that is not live.
template <class View> NTX_DEV void ray_forward(const View &v, const CompositeCommon &a, int lane, float *el, float *T, float (&c)[3], float &A) {
    const float T_last = ray_transmittance(v, lane, el, T);
    c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f; A = 0.0f;
    for (int s = lane; s < v.S; s += 64) {
        const int row = v.row(s);
        if (!View::live(row)) { if (v.weights) v.weights[v.m0 + s] = 0.0f; continue; }                 // a = 0: no weight
        const float *raw = v.raw(row);
        const float w = (1.0f - el[s]) * T[s];
        for (int k = 0; k < 3; ++k) c[k] += w * rgb_of(raw[k], a.map_exr);
        A += w;
        if (v.weights) v.weights[v.m0 + s] = w;
    }
    c[0] = wave_sumf(c[0]); c[1] = wave_sumf(c[1]); c[2] = wave_sumf(c[2]); A = wave_sumf(A);
    v.close_forward(c, A, T_last);
    if (a.composite_bkgd) for (int k = 0; k < 3; ++k) c[k] += (1.0f - A) * a.bkgd[k];           // :210-211, :351-352
}
NTX_DEV void store_prediction(const CompositeCommon &a, long long ray, int lane, const float (&c)[3], float A) {
    if (lane == 0) { a.color[3 * ray] = c[0]; a.color[3 * ray + 1] = c[1]; a.color[3 * ray + 2] = c[2]; a.alpha[ray] = A; }
}
// The adjoint of a ray's composite from dC = dL/d color_pred and dA = dL/d alpha_pred (el and T as ray_transmittance left them), to the
// view's store.
//     C = sum w rgb (+ (1 - A) bkgd), A = sum w, w_i = a_i T_i, T_i = prod_{j<i} f_j, f_j = (1 - a_j) + 1e-10.  With
// dL/dw_k = c_k + dA' (c_k = dC . rgb_k, dA' = dA - dC . bkgd):
//     dL/da_i = T_i (dA' Z_i + (c_i - V_i)),
//     V_i = sum_{k>i} c_k a_k prod_{i<j<k} f_j   (the colour composited behind sample i, along dC):   V_{i-1} = c_i a_i + f_i V_i,  V_{S-1} = 0
//     Z_i = 1 - sum_{k>i} a_k prod_{i<j<k} f_j   (what is left of the ray behind sample i):            Z_{i-1} = f_i Z_i - 1e-10,   Z_{S-1} = 1
// (V_{S-1}, Z_{S-1}: the view's close_adjoint where something lies behind the ray's end.)
// Nothing is divided and the opacity term is never formed as a difference of two sums.  tf.math.cumprod's own gradient
// (TF 2.4 math_grad.py _CumprodGrad: cumsum(out * grad, reverse) / x) is the same derivative as a quotient by f_i, which on a saturated
// sample (f_i -> 1e-10) loses the digits the forward product kept, and "dA' (1 - sum)" loses them again when the ray saturates BEHIND
// sample i (round 5's kernel did both: profiles/r05/soak_train_seed3.txt, case 297).
// A chunk of 64 samples is a suffix scan of the affine maps X -> b_i + f_i X (composed pairwise), carried from chunk to chunk back to front.
// A sample that is not live is the map X -> -1e-10 + (1 + 1e-10) X for Z and the identity's for V (Bv exactly 0), and writes nothing.
// A loss on the weights themselves (gw = dL/d w [N][S], or NULL): dL/dw_k = c_k + g_k + dA', and everything above holds with c_k + g_k in
// the place of c_k -- in c_i - V_i and in V_{i-1} = (c_i + g_i) a_i + f_i V_i; dL/d raw rgb = w dC rgb' has no such term.  gw is read at live
// samples only.  With gw NULL nothing is added (no + 0.0f): the fused step and a backward without a weight cotangent keep their bits.  Like
// every optional array gw is indexed from its base at m0 + s: a per-ray pointer would turn the scalar test for NULL into a vector one.
template <class View> NTX_DEV void ray_adjoint(const View &v, const CompositeCommon &a, int lane, const float *el, const float *T, const float (&dC)[3], float dA,
                                                                   const float *gw) {
    const int S = v.S;
    if (a.composite_bkgd) dA -= (dC[0] * a.bkgd[0] + dC[1] * a.bkgd[1]) + dC[2] * a.bkgd[2];
    float Z_carry = 1.0f, V_carry = 0.0f;                  // Z, V of the last sample of the current chunk (nothing lies behind a whole ray's end)
    v.close_adjoint(dC, Z_carry, V_carry);
    for (int s0 = ((S - 1) / 64) * 64; s0 >= 0; s0 -= 64) {
        const int s = s0 + lane;
        const int row = s < S ? v.row(s) : -1;
        const bool lv = s < S && View::live(row);
        float cs = 0.0f, rgb[3] = {0.0f, 0.0f, 0.0f}, e = 1.0f;
        float F = 1.0f, Bz = 0.0f, Bv = 0.0f;              // the identity for the lanes past the ray's end
        if (s < S) {
            e = el[s];
            if (lv) {
                const float *raw = v.raw(row);
                for (int c = 0; c < 3; ++c) rgb[c] = rgb_of(raw[c], a.map_exr);
                cs = (dC[0] * rgb[0] + dC[1] * rgb[1]) + dC[2] * rgb[2];
                if (gw) cs += gw[v.m0 + s];
            }
            F = e + 1e-10f; Bz = -1e-10f; Bv = lv ? cs * (1.0f - e) : 0.0f;
        }
        // inclusive suffix composition: lane l ends with the maps of samples l .. 63 of the chunk composed, X_{l-1} = B + F X_63
        for (int o = 1; o < 64; o <<= 1) {
            const float Fo = __shfl_down(F, o), Bzo = __shfl_down(Bz, o), Bvo = __shfl_down(Bv, o);
            if (lane + o < 64) { Bz = fmaf(F, Bzo, Bz); Bv = fmaf(F, Bvo, Bv); F *= Fo; }
        }
        float Fn = __shfl_down(F, 1), Bzn = __shfl_down(Bz, 1), Bvn = __shfl_down(Bv, 1);   // the lanes strictly behind this one
        if (lane == 63) { Fn = 1.0f; Bzn = 0.0f; Bvn = 0.0f; }
        const float Z = fmaf(Fn, Z_carry, Bzn), V = fmaf(Fn, V_carry, Bvn);
        if (lv) {
            const float *raw = v.raw(row);                 // (read again: keeping the three values across the scan costs more than the loads)
            const float w = (1.0f - e) * T[s];
            const float d_a = T[s] * fmaf(dA, Z, cs - V);
            const float sig = v.density(s, row);
            float gr[4];
            for (int c = 0; c < 3; ++c) {
                const float drgb = a.map_exr ? (raw[c] > 0.0f ? 1.0f : expf(raw[c])) : rgb[c] * (1.0f - rgb[c]);
                gr[c] = w * dC[c] * drgb;
            }
            gr[3] = sig > 0.0f ? v.dsigma(s, d_a, e) : 0.0f;
            v.store(s, row, gr);
        }
        const float F0 = __shfl(F, 0);
        Z_carry = fmaf(F0, Z_carry, __shfl(Bz, 0)); V_carry = fmaf(F0, V_carry, __shfl(Bv, 0));
    }
}
}   // namespace ntx_train
