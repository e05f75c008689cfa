// ntx_arch.h -- everything that reads an ntx_model_desc, for the host units of the library (the packers, the context, the trainers): which
// kernel family a model runs on, the widths and rows of its own encodings, and the one view of its weight blob in Keras' get_weights()
// order.  Plain C++17: no HIP, nothing but the ABI header and ntx_layout.h.
#pragma once
#include "nerftex.h"
#include "ntx_layout.h"

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <vector>

extern "C" int ntx_set_error(int code, const char *fmt, ...);   // nerftex.hip: the per-thread message behind ntx_last_error()

namespace ntx {
// ---------------------------------------------------------------------------------------------
// supported architectures = the kernels instantiated in ntx_variant.hip / ntx_variant_x3.hip
// ---------------------------------------------------------------------------------------------
struct Variant {
    int n_geo, n_app, cd, ipe;   // the kernel family's layout (for the generic family: its parameter SLOTS)
    int gen;
    int flex;                    // the architecture is read from the model descriptor (ntx_layout.h "flex family")
};
inline constexpr Variant kVariants[] = {
    {1, 6, 1, 0, 0},   // carpet          (configs/config_carpet_render.py:59-72)
    {1, 4, 1, 0, 0},   // grass, fur, plush
    {2, 3, 1, 0, 0},   // grass_filtered
    {0, 0, 0, 0, 0},   // plain Nerf      (model.py:9-45)
    {1, 3, 1, 1, 0},   // mip variant of grass_filtered: IPE on (mean, cov), blur parameter spliced out (renderer.py:385-386)
    {GEN_NGEO, GEN_NAPP, 1, 0, 1},   // generic: any other ParamNerf n_parameters = [g <= 4, a <= 8]; absent parameters = zero rows
    {GEN_NGEO, GEN_NAPP, 1, 0, 1, 1},   // flex: any depth <= 24, width <= 256, skips, color_depth <= 4 (model.py:58), float32 kernels only
    {GEN_NGEO, GEN_NAPP, 1, 0, 1, 2},   // flex with param_depth 1..4: Dense(param_width <= 128) layers on the parameter features (model.py:88-101)
};
constexpr int kFlexVariant = 6, kFlexParamVariant = 7;
static_assert(NTX_SKIP_MASK == (unsigned)NTX_SKIP_MASK_BIT, "skip encoding of the ABI header and of ntx_layout.h");

// the model's own parameter counts (the generic family has more slots than the model has parameters)
struct Dims {
    int g, a;
    int pf, df, qf;   // n_freq_bands of the model's position / direction / parameter embeddings (layer.py:11)
};
inline Dims dims_of(const ntx_model_desc *d) {
    const bool nerf = d->kind == NTX_MODEL_NERF;
    return Dims{nerf ? 0 : d->n_geo, nerf ? 0 : d->n_app, d->pos_freq, d->dir_freq, nerf || d->n_geo + d->n_app <= 0 ? PAR_FREQ : d->param_freq};
}
// FEWER frequency bands than the kernels' 10 / 4 / 4 (FourierFeatures(n_freq_bands), layer.py:8-23): the kernels evaluate all of
// theirs, the packers give the bands the model does not have zero weight rows -- exact, like the parameters the generic family does
// not have.  Widths of the model's own encodings, and the model's row for row r of a 10/4/4 model's map (-1: no such band).
inline int par_emb_m(int n_act, Dims m) { return n_act * (1 + 2 * m.qf); }
inline int pos_emb_m(Dims m, int ipe) { return ipe ? 6 * m.pf : 3 * (1 + 2 * m.pf); }
inline int dir_emb_m(Dims m) { return 3 * (1 + 2 * m.df); }
inline int pos_map_m(Dims m, int ipe) { return pos_emb_m(m, ipe) + par_emb_m(m.g, m); }
inline int dir_map_m(Dims m) { return dir_emb_m(m) + par_emb_m(m.a, m); }
inline int par_row_m(int idx, int n_act, int qf) {        // idx into [p (n_act) | sin f0, cos f0 (n_act each) | ...] of 4 bands
    if (idx < n_act) return idx;
    return (idx - n_act) / (2 * n_act) < qf ? idx : -1;
}
inline int pos_row_m(int r, Dims m, int ipe) {
    if (r < 0) return r;
    const int full = pos_emb_dim(ipe);
    if (r >= full) { const int q = par_row_m(r - full, m.g, m.qf); return q < 0 ? -1 : pos_emb_m(m, ipe) + q; }
    if (ipe) { const int h = r / (3 * POS_FREQ), q = r % (3 * POS_FREQ); return q / 3 < m.pf ? h * 3 * m.pf + q : -1; }
    return r < 3 || (r - 3) / 6 < m.pf ? r : -1;
}
inline int dir_row_m(int r, Dims m) {
    if (r < 0) return r;
    const int full = 3 * (1 + 2 * DIR_FREQ);
    if (r >= full) { const int q = par_row_m(r - full, m.a, m.qf); return q < 0 ? -1 : dir_emb_m(m) + q; }
    return r < 3 || (r - 3) / 6 < m.df ? r : -1;
}

// the model's `skips` as a mask of layer indices: ntx_model_desc.skip is one index (-1: none) or NTX_SKIP_MASK | mask
inline unsigned skip_mask_of(const ntx_model_desc *d) {
    if (d->skip < 0) return 0u;
    if (d->skip & NTX_SKIP_MASK) return (unsigned)d->skip & (NTX_SKIP_MASK - 1u);
    return d->skip < 30 ? 1u << d->skip : 0u;
}
// ... those that fire: `i in skips` never does for i >= depth (model.py:107); i = depth - 1 is refused in find_variant
inline unsigned trunk_skips(const ntx_model_desc *d) { return skip_mask_of(d) & ((1u << (d->depth > 1 ? d->depth - 1 : 0)) - 1u); }
// param_depth / param_width of the model: fields of the extended descriptor (kind NTX_MODEL_PARAMNERF_EX); a model without
// parameters has no branches whatever param_depth says (model.py:88, 96).  These two and flex_arch_of read BEHIND the base struct when
// kind says so: d must then point into a whole ntx_model_desc_ex (the caller's, or the context's copy), never at a copy of the base alone
inline int param_depth_of(const ntx_model_desc *d) {
    if (d->kind != NTX_MODEL_PARAMNERF_EX || d->n_geo + d->n_app <= 0) return 0;
    return reinterpret_cast<const ntx_model_desc_ex *>(d)->param_depth;
}
inline int param_width_of(const ntx_model_desc *d) {
    return d->kind == NTX_MODEL_PARAMNERF_EX ? reinterpret_cast<const ntx_model_desc_ex *>(d)->param_width : 0;
}
// the architecture without parameter branches: the base struct's fields only (what the trainers build, which refuse branches)
inline FlexArch trunk_arch_of(const ntx_model_desc *d) {
    return FlexArch{d->depth, d->width, d->kind == NTX_MODEL_NERF ? 0 : d->color_depth, trunk_skips(d), 0, 0, 0, 0};
}
inline FlexArch flex_arch_of(const ntx_model_desc *d) {
    FlexArch f = trunk_arch_of(d);
    f.param_depth = param_depth_of(d);
    if (f.param_depth > 0) { f.param_width = param_width_of(d); f.has_geo = d->n_geo > 0; f.has_app = d->n_app > 0; }
    return f;
}
inline bool default_arch(const ntx_model_desc *d) {
    const bool nerf = d->kind == NTX_MODEL_NERF;
    return d->depth == DEPTH && d->width == WIDTH && d->skip == SKIP && (nerf || d->color_depth == 1) && param_depth_of(d) == 0;
}
// the architecture of the tuned and generic families (default_arch), colour layer or not
inline FlexArch tuned_arch(int cd) { return FlexArch{DEPTH, WIDTH, cd, 1u << SKIP, 0, 0, 0, 0}; }

inline int find_variant(const ntx_model_desc *d) {
    if (!d) return -1;
    const int ipe = d->pos_encoding == NTX_POS_IPE;
    if (d->pos_encoding != NTX_POS_FOURIER && d->pos_encoding != NTX_POS_IPE) return -1;
    if (d->n_pos != (ipe ? 6 : 3) || d->pos_freq < 0 || d->pos_freq > POS_FREQ || d->dir_freq < 0 || d->dir_freq > DIR_FREQ) return -1;
    if (d->kind != NTX_MODEL_PARAMNERF && d->kind != NTX_MODEL_NERF && d->kind != NTX_MODEL_PARAMNERF_EX) return -1;
    const bool nerf = d->kind == NTX_MODEL_NERF;
    const int g = nerf ? 0 : d->n_geo, a = nerf ? 0 : d->n_app, cd = nerf ? 0 : d->color_depth;
    if (g < 0 || a < 0) return -1;
    if (!nerf && (g + a > 0) && (d->param_freq < 0 || d->param_freq > PAR_FREQ)) return -1;
    const bool force_flex = getenv("NERFTEX_FORCE_FLEX") != nullptr;         // A/B knobs for tests: a tuned family's model on the
    const bool force_generic = getenv("NERFTEX_FORCE_GENERIC") != nullptr;   // flex / generic kernels
    if (default_arch(d) && !(force_flex && !ipe)) {
        for (size_t i = 0; i < sizeof(kVariants) / sizeof(kVariants[0]) && !(force_generic && !nerf && !ipe); ++i)
            if (!kVariants[i].gen && kVariants[i].n_geo == g && kVariants[i].n_app == a && kVariants[i].cd == cd && kVariants[i].ipe == ipe) return (int)i;
        for (size_t i = 0; i < sizeof(kVariants) / sizeof(kVariants[0]); ++i)
            if (kVariants[i].gen && !kVariants[i].flex && !nerf && g <= kVariants[i].n_geo && a <= kVariants[i].n_app && kVariants[i].cd == cd && kVariants[i].ipe == ipe) return (int)i;
        return -1;
    }
    // any other architecture: the layer loop of the flex family
    if (ipe || g > GEN_NGEO || a > GEN_NAPP) return -1;
    if (d->depth < 1 || d->depth > FLEX_MAX_DEPTH || d->width < 2 || d->width > WIDTH || cd < 0 || cd > FLEX_MAX_COLOR) return -1;
    if (d->skip >= 0 && !(d->skip & NTX_SKIP_MASK) && d->skip >= 30) return -1;
    // a skip behind the LAST trunk layer widens the inputs of the alpha head and of the feature layer (model.py:107-114): not built
    if ((skip_mask_of(d) >> (d->depth - 1)) & 1u) return -1;
    if (d->kind == NTX_MODEL_PARAMNERF_EX && reinterpret_cast<const ntx_model_desc_ex *>(d)->param_depth < 0) return -1;
    if (const int pd = param_depth_of(d)) {
        if (pd > FLEX_MAX_PARAM_DEPTH || param_width_of(d) < 2 || param_width_of(d) > 2 * BRANCH_K) return -1;
        return kFlexParamVariant;
    }
    return kFlexVariant;
}

inline int unsupported(const ntx_model_desc *d) {
    if (!d) return ntx_set_error(NTX_E_INVALID, "model descriptor is NULL");
    return ntx_set_error(NTX_E_UNSUPPORTED,
                "unsupported model: kind=%d n_parameters=[%d,%d] n_pos=%d freqs=%d/%d/%d depth=%d width=%d "
                "skip=%d color_depth=%d pos_encoding=%d param_depth=%d param_width=%d (built: ParamNerf with n_parameters [g<=4, a<=8] -- tuned kernels for [1,6] [1,4] "
                "[2,3] at 8x256 / skips [4] / color_depth 1 --, Nerf, and ParamNerf [1,3] with IntegratedPositionalEncoding on 6-D positions; "
                "other architectures (FourierFeatures only): depth 1..24, width 2..256, color_depth 0..4, skips below depth-1, "
                "param_depth 0..4 with param_width 2..128; n_freq_bands <= 10 / 4 / 4)",
                d->kind, d->n_geo, d->n_app, d->n_pos, d->pos_freq, d->dir_freq, d->param_freq, d->depth,
                d->width, d->skip, d->color_depth, d->pos_encoding,
                d->kind == NTX_MODEL_PARAMNERF_EX ? reinterpret_cast<const ntx_model_desc_ex *>(d)->param_depth : 0, param_width_of(d));
}

// ---------------------------------------------------------------------------------------------
// reference-layout blob (Keras get_weights() order) -> layer views (model.py:104-125)
// ---------------------------------------------------------------------------------------------
struct BlobLayer { int in, out; size_t w, b; };      // offsets into the blob: kernel [in][out], then bias [out]
struct BlobView {
    std::vector<BlobLayer> trunk, colour;   // colour: the color_depth hidden colour layers
    std::vector<BlobLayer> pgeo, papp;      // param_depth > 0: the Dense layers of the geometry / appearance branch
    BlobLayer alpha, feature, c2, rgb;      // c2: the colour half layer
    int pos_map, dir_map;                   // widths of pos_map / dir_map as the trunk / the first colour layer see them
    size_t count;                           // floats of the whole blob
};
// get_weights() order of the functional model for ANY architecture (layer_table of nerf_tex_amd/model.py, checked against a
// restatement of Keras' rule in tests/test_oracle.py): every Dense layer in the order a depth-first traversal from outputs = [color,
// alpha] first meets it, with its graph depth (concat nodes take a level), then by decreasing depth, ties in traversal order -- so the
// alpha head comes LAST although it is created before the feature layer (model.py:111-123).
// Without branches: trunk, feature, colour layers, colour half, color, alpha.  With param_depth > 0 the geometry branch comes
// before the trunk and the appearance branch interleaves with the trunk layers of equal depth, ahead of them.
inline BlobView view_blob(const FlexArch &f, Dims m, int ipe = 0) {
    BlobView n{};
    const int pd = f.param_depth, pw = f.param_width, w = f.width, cd = f.color_depth;
    n.pos_map = pos_emb_m(m, ipe) + (m.g > 0 ? (pd > 0 ? pw : par_emb_m(m.g, m)) : 0);
    n.dir_map = dir_emb_m(m) + (m.a > 0 ? (pd > 0 ? pw : par_emb_m(m.a, m)) : 0);
    struct Slot { BlobLayer *l; int in, out, depth; };
    std::vector<Slot> seq;
    n.trunk.resize(f.depth); n.colour.resize(cd);
    n.pgeo.resize(f.has_geo ? pd : 0); n.papp.resize(f.has_app ? pd : 0);
    seq.push_back({&n.rgb, w / 2, 3, 0});
    seq.push_back({&n.c2, cd > 0 ? w : w + n.dir_map, w / 2, 1});
    for (int i = cd - 1; i >= 0; --i) seq.push_back({&n.colour[i], i == 0 ? w + n.dir_map : w, w, 1 + cd - i});
    int d = cd + 2;
    for (int i = (int)n.papp.size() - 1; i >= 0; --i) seq.push_back({&n.papp[i], i == 0 ? par_emb_m(m.a, m) : pw, pw, d + 2 + (pd - 1 - i)});
    d += 1;
    seq.push_back({&n.feature, w, w, d});                                    // (a skip behind the last trunk layer is refused)
    for (int i = f.depth - 1; i >= 0; --i) {
        d += 1 + (((f.skip_mask >> i) & 1u) ? 1 : 0);
        const int in = i == 0 ? n.pos_map : w + (((f.skip_mask >> (i - 1)) & 1u) ? n.pos_map : 0);
        seq.push_back({&n.trunk[i], in, w, d});
    }
    for (int i = (int)n.pgeo.size() - 1; i >= 0; --i) seq.push_back({&n.pgeo[i], i == 0 ? par_emb_m(m.g, m) : pw, pw, d + 2 + (pd - 1 - i)});
    seq.push_back({&n.alpha, w, 1, 0});
    std::stable_sort(seq.begin(), seq.end(), [](const Slot &x, const Slot &y) { return x.depth > y.depth; });
    for (const Slot &sl : seq) {
        *sl.l = BlobLayer{sl.in, sl.out, n.count, n.count + (size_t)sl.in * sl.out};
        n.count += (size_t)sl.in * sl.out + sl.out;
    }
    return n;
}
// ... of the model a descriptor of family v names
inline BlobView view_blob_of(int v, const ntx_model_desc *d) {
    return kVariants[v].flex ? view_blob(flex_arch_of(d), dims_of(d)) : view_blob(tuned_arch(kVariants[v].cd), dims_of(d), kVariants[v].ipe);
}
}  // namespace ntx
