// ntx_pack.cpp -- the weight packers: a model's blob in Keras' get_weights() order (ntx_arch.h: view_blob) -> the images the kernels stream
// (ntx_layout.h), and the five entries of the C ABI that need nothing else.  Host only: compiled into the library with the other units, and
// with a plain host compiler under the sanitizers by `make pack_check` (ntx_pack_check.cpp).
#include "ntx_pack.h"

#include <cstring>

using namespace ntx;

// one segment of the stream: for every k-step, NMT/4 records of [lane][4 consecutive M-tiles]
template <class RowFn>
static void emit_segment(float *&dst, const float *w, const BlobLayer &l, int nsteps, int nmt, int row_offset, RowFn rowfn) {
    for (int s = 0; s < nsteps; ++s)
        for (int q = 0; q < nmt / 4; ++q)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int row = rowfn(s, lane >> 5);
                    const int col = 32 * (4 * q + e) + (lane & 31);
                    float val = 0.0f;
                    if (row >= 0 && col < l.out) val = w[(size_t)(row_offset + row) * l.out + col];
                    *dst++ = val;
                }
}
static int hidrow(int s, int h) { return hidden_row(s, h); }

// a bias slot of the aux block, [half][128] in accumulator order, and the block's alpha / rgb heads: features the layer does not have
// (width < 256) are zero
static void put_bias(float *slot, const float *blob, const BlobLayer &l) {
    for (int h = 0; h < 2; ++h)
        for (int s = 0; s < HSTEPS; ++s) {
            const int r = hidden_row(s, h);
            slot[h * 128 + s] = r < l.out ? blob[l.b + r] : 0.0f;
        }
}
static void put_heads(float *aux, const float *blob, const BlobView &n) {
    for (int h = 0; h < 2; ++h)
        for (int s = 0; s < HSTEPS; ++s) {
            const int r = hidden_row(s, h);
            aux[aux_alpha_off() + h * 128 + s] = r < n.alpha.in ? blob[n.alpha.w + r] : 0.0f;
        }
    aux[aux_alpha_off() + 256] = blob[n.alpha.b];
    for (int c = 0; c < 3; ++c) {
        for (int h = 0; h < 2; ++h)
            for (int s = 0; s < 64; ++s) {
                const int r = hidden_row(s, h);
                aux[aux_rgb_off() + (c * 2 + h) * 64 + s] = r < n.rgb.in ? blob[n.rgb.w + r * 3 + c] : 0.0f;
            }
        aux[aux_rgb_off() + 384 + c] = blob[n.rgb.b + c];
    }
}

// ---- tuned and generic families: 8 x 256 / skips [4] / one colour layer or none ---------------------------------------------------
static void pack(const Variant &v, Dims m, const float *blob, float *out) {
    const Geometry g = make_geometry(v.n_geo, v.n_app, v.cd, v.ipe);
    const BlobView n = view_blob(tuned_arch(v.cd), m, v.ipe);
    const int pm = n.pos_map, dm = n.dir_map;
    float *dst = out;
    auto posrow = [&](int s, int h) { return pos_row_m(pos_row(v.n_geo, s, h, v.ipe, m.g), m, v.ipe); };
    auto dirrow = [&](int s, int h) { return dir_row_m(dir_row(v.n_app, s, h, m.a), m); };
    auto seg = [&](const BlobLayer &l, int nsteps, int nmt, int row_offset, auto rowfn) { emit_segment(dst, blob + l.w, l, nsteps, nmt, row_offset, rowfn); };

    seg(n.trunk[0], g.pos_steps, 8, 0, posrow);
    for (int i = 1; i < DEPTH; ++i) {
        if (i == SKIP + 1) {
            seg(n.trunk[i], g.pos_steps, 8, 0, posrow);
            seg(n.trunk[i], HSTEPS, 8, pm, hidrow);
        } else {
            seg(n.trunk[i], HSTEPS, 8, 0, hidrow);
        }
    }
    seg(n.feature, HSTEPS, 8, 0, hidrow);
    if (v.cd) {
        seg(n.colour[0], g.dir_steps, 8, 0, dirrow);
        seg(n.colour[0], HSTEPS, 8, dm, hidrow);
        seg(n.c2, HSTEPS, 4, 0, hidrow);
    } else {
        seg(n.c2, g.dir_steps, 4, 0, dirrow);
        seg(n.c2, HSTEPS, 4, dm, hidrow);
    }
    // zero pad up to a whole number of ring turns, then the wrap-around tail: the first RING records again
    for (int i = g.stream_records; i < g.padded_records; ++i) { memset(dst, 0, sizeof(float) * REC_FLOATS); dst += REC_FLOATS; }
    memcpy(dst, out, sizeof(float) * RING * REC_FLOATS);
    dst += RING * REC_FLOATS;

    // aux block
    float *aux = dst;
    memset(aux, 0, sizeof(float) * g.aux_floats);
    for (int i = 0; i < DEPTH; ++i) put_bias(aux + i * AUX_BIAS_STRIDE, blob, n.trunk[i]);
    put_bias(aux + 8 * AUX_BIAS_STRIDE, blob, n.feature);
    if (v.cd) put_bias(aux + 9 * AUX_BIAS_STRIDE, blob, n.colour[0]);
    put_bias(aux + 10 * AUX_BIAS_STRIDE, blob, n.c2);
    put_heads(aux, blob, n);
}

// ---- flex family (ntx_layout.h): any depth / width <= 256 / skips / color_depth ---------------------------------------------------
// emit_segment with the rows of a narrower layer (width < 256: hidden rows >= `rows` are zero) and zero records up to PADREC
template <class RowFn>
static void emit_segment_flex(float *&dst, const float *w, const BlobLayer &l, int nsteps, int nmt, int row_offset, int rows, RowFn rowfn) {
    emit_segment(dst, w, l, nsteps, nmt, row_offset, [&](int s, int h) { const int r = rowfn(s, h); return r < rows ? r : -1; });
    const int pad = flex_seg_records(nsteps, nmt) - nsteps * (nmt / 4);
    memset(dst, 0, sizeof(float) * REC_FLOATS * pad);
    dst += (size_t)REC_FLOATS * pad;
}

static size_t packed_floats_flex(const FlexArch &f) {
    return (size_t)(flex_stream_records(f) + RING) * REC_FLOATS + aux_total() + flex_floats();
}

static void pack_flex(const FlexArch &f, Dims m, const float *blob, float *out) {
    const BlobView n = view_blob(f, m);
    const bool pb = f.param_depth > 0;
    const int pe = pos_emb_m(m, 0), de = dir_emb_m(m);                       // FF(pos), FF(dir) as the model has them
    const int pm = n.pos_map, dm = n.dir_map;
    // without branches: the position / direction segments of the generic family (parameter features in them); with: FF(pos) /
    // FF(dir) alone, each followed by 64 k-steps over its branch's output
    const int ps = pb ? pos_steps(0) : pos_steps(GEN_NGEO), ds = pb ? dir_steps(0) : dir_steps(GEN_NAPP);
    float *dst = out;
    const Dims m0{0, 0, m.pf, m.df, m.qf};                                      // with branches the segments hold FF(pos) / FF(dir) alone
    auto posrow = [&](int s, int h) { return pb ? pos_row_m(pos_row(0, s, h), m0, 0) : pos_row_m(pos_row(GEN_NGEO, s, h, 0, m.g), m, 0); };
    auto dirrow = [&](int s, int h) { return pb ? dir_row_m(dir_row(0, s, h), m0) : dir_row_m(dir_row(GEN_NAPP, s, h, m.a), m); };
    auto seg = [&](const BlobLayer &l, int nsteps, int nmt, int row_offset, int rows, auto rowfn) { emit_segment_flex(dst, blob + l.w, l, nsteps, nmt, row_offset, rows, rowfn); };
    const int W = f.width, PW = f.param_width;
    auto branch = [&](const std::vector<BlobLayer> &ls, int n_slots, int n_act) {   // a branch's own layers, 4 tiles
        if (ls.empty()) return;
        seg(ls[0], parff_steps(n_slots), 4, 0, ls[0].in, [&](int s, int h) { const int r = parff_row(n_slots, s, h, n_act); return r < 0 ? r : par_row_m(r, n_act, m.qf); });
        for (size_t i = 1; i < ls.size(); ++i) seg(ls[i], BRANCH_K, 4, 0, PW, hidrow);
    };
    auto pos_input = [&](const BlobLayer &l) {                                  // concat[FF(pos) (+ parameter features) | G]
        seg(l, ps, 8, 0, pb ? pe : pm, posrow);
        if (pb && f.has_geo) seg(l, BRANCH_K, 8, pe, PW, hidrow);
    };
    auto dir_input = [&](const BlobLayer &l, int nmt) {                        // concat[FF(dir) (+ parameter features) | A]
        seg(l, ds, nmt, 0, pb ? de : dm, dirrow);
        if (pb && f.has_app) seg(l, BRANCH_K, nmt, de, PW, hidrow);
    };
    branch(n.pgeo, GEN_NGEO, m.g);
    pos_input(n.trunk[0]);
    for (int i = 1; i < f.depth; ++i) {
        const bool skip_in = (f.skip_mask >> (i - 1)) & 1u;
        if (skip_in) pos_input(n.trunk[i]);
        seg(n.trunk[i], HSTEPS, 8, skip_in ? pm : 0, W, hidrow);
    }
    seg(n.feature, HSTEPS, 8, 0, W, hidrow);
    branch(n.papp, GEN_NAPP, m.a);
    if (f.color_depth > 0) {
        dir_input(n.colour[0], 8);
        seg(n.colour[0], HSTEPS, 8, dm, W, hidrow);
        for (int i = 1; i < f.color_depth; ++i) seg(n.colour[i], HSTEPS, 8, 0, W, hidrow);
        seg(n.c2, HSTEPS, 4, 0, W, hidrow);
    } else {
        dir_input(n.c2, 4);
        seg(n.c2, HSTEPS, 4, dm, W, hidrow);
    }
    memcpy(dst, out, sizeof(float) * RING * REC_FLOATS);   // wrap-around tail
    dst += RING * REC_FLOATS;

    // aux block: the tuned layout (only its alpha / rgb heads are used), then [descriptor | bias slots]
    float *aux = dst;
    memset(aux, 0, sizeof(float) * (aux_total() + flex_floats()));
    put_heads(aux, blob, n);
    int32_t *desc = reinterpret_cast<int32_t *>(aux + aux_total());
    desc[0] = f.depth; desc[1] = (int32_t)f.skip_mask; desc[2] = f.color_depth;
    desc[3] = f.param_depth; desc[4] = f.has_geo; desc[5] = f.has_app;
    float *bias = aux + aux_total() + FLEX_DESC_FLOATS;
    int slot = 0;
    auto put = [&](int at, const BlobLayer &l) { put_bias(bias + at * AUX_BIAS_STRIDE, blob, l); };
    for (int i = 0; i < f.depth; ++i) put(slot++, n.trunk[i]);
    put(slot++, n.feature);
    for (int i = 0; i < f.color_depth; ++i) put(slot++, n.colour[i]);
    put(slot++, n.c2);
    // branch layers: geometry at n8 + 1 .., appearance at n8 + 1 + FLEX_MAX_PARAM_DEPTH .. (mlp_flex)
    for (size_t i = 0; i < n.pgeo.size(); ++i) put(slot + (int)i, n.pgeo[i]);
    for (size_t i = 0; i < n.papp.size(); ++i) put(slot + FLEX_MAX_PARAM_DEPTH + (int)i, n.papp[i]);
    static_assert(FLEX_MAX_DEPTH + 1 + FLEX_MAX_COLOR + 1 + 2 * FLEX_MAX_PARAM_DEPTH <= FLEX_MAX_LAYERS, "bias slots");
}

// ---- fp16x3 stream (ntx_layout.h: one record = the A operand of one (k16-step, M-tile), hi record then lo record) ----
// float32 -> IEEE half, round to nearest even, subnormals kept, overflow to inf (what v_cvt_f16_f32 does)
static uint16_t f16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u >= 0x47800000u) return sign | (u > 0x7f800000u ? 0x7e00 : 0x7c00);   // >= 65536: inf, or NaN
    if (u < 0x38800000u) {                                                       // < 2^-14: subnormal half or zero
        // adding 0.5f aligns the value so that float addition rounds it (RNE) to a multiple of 2^-24
        float t;
        memcpy(&t, &u, 4);
        t += 0.5f;
        uint32_t r;
        memcpy(&r, &t, 4);
        return sign | (uint16_t)(r - 0x3f000000u);
    }
    const uint32_t odd = (u >> 13) & 1u;
    u += 0xc8000fffu + odd;        // rebias the exponent by -112 and round the 13 dropped bits to nearest even
    return sign | (uint16_t)(u >> 13);                                           // 65520..65535.99 carries into inf
}
static float f16_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, em = h & 0x7fffu;
    uint32_t u;
    if (em >= 0x7c00u) u = sign | 0x7f800000u | ((em & 0x3ffu) << 13);
    else if (em >= 0x0400u) u = sign | ((em << 13) + 0x38000000u);
    else {                                                                       // subnormal: em * 2^-24
        const float t = (float)em * 5.9604644775390625e-08f;
        memcpy(&u, &t, 4);
        u |= sign;
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

template <class RowFn>
static void emit_segment16(uint16_t *&dst, const float *w, const BlobLayer &l, int nsteps16, int nmt, int row_offset, RowFn rowfn) {
    for (int u = 0; u < nsteps16; ++u)
        for (int mt = 0; mt < nmt; ++mt) {
            uint16_t *hi = dst, *lo = dst + 512;
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int row = rowfn(8 * u + e, lane >> 5);
                    const int col = 32 * mt + (lane & 31);
                    float val = 0.0f;
                    if (row >= 0 && col < l.out) val = w[(size_t)(row_offset + row) * l.out + col];
                    const uint16_t h = f16_rne(val);
                    hi[lane * 8 + e] = h;
                    lo[lane * 8 + e] = f16_rne(val - f16_f32(h));
                }
            dst += 1024;
        }
}

namespace ntx {
size_t packed16_bytes(const Variant &v, int with_dir) {
    return (size_t)stream16_padded(v.n_geo, v.n_app, v.cd, with_dir, v.ipe) * 1024;
}

// hidden segment first, encoder segment second within a pass (ntx_device_x3.h: Cfg16)
void pack16(const Variant &v, Dims m, const float *blob, uint16_t *out, int with_dir) {
    const BlobView n = view_blob(tuned_arch(v.cd), m, v.ipe);
    const int pm = n.pos_map, dm = n.dir_map;
    const int ps = steps16(pos_steps(v.n_geo, v.ipe)), ds = steps16(dir_steps(v.n_app)), hs = HSTEPS / 8;
    uint16_t *dst = out;
    auto posrow = [&](int s, int h) { return s < pos_steps(v.n_geo, v.ipe) ? pos_row_m(pos_row(v.n_geo, s, h, v.ipe, m.g), m, v.ipe) : -1; };
    auto dirrow = [&](int s, int h) { return s < dir_steps(v.n_app) ? dir_row_m(dir_row(v.n_app, s, h, m.a), m) : -1; };
    auto seg = [&](const BlobLayer &l, int nsteps16, int nmt, int row_offset, auto rowfn) { emit_segment16(dst, blob + l.w, l, nsteps16, nmt, row_offset, rowfn); };
    seg(n.trunk[0], ps, 8, 0, posrow);
    for (int i = 1; i < DEPTH; ++i) {
        if (i == SKIP + 1) {
            seg(n.trunk[i], hs, 8, pm, hidrow);
            seg(n.trunk[i], ps, 8, 0, posrow);
        } else {
            seg(n.trunk[i], hs, 8, 0, hidrow);
        }
    }
    seg(n.feature, hs, 8, 0, hidrow);
    if (v.cd) {
        seg(n.colour[0], hs, 8, dm, hidrow);   // render kernel: its direction rows are applied per ray by dir_block (float32)
        if (with_dir) seg(n.colour[0], ds, 8, 0, dirrow);
        seg(n.c2, hs, 4, 0, hidrow);
    } else {
        seg(n.c2, hs, 4, dm, hidrow);
        seg(n.c2, ds, 4, 0, dirrow);
    }
    const int rec = stream16_records(v.n_geo, v.n_app, v.cd, with_dir, v.ipe), pad = stream16_padded(v.n_geo, v.n_app, v.cd, with_dir, v.ipe);
    memset(dst, 0, (size_t)(pad - rec) * 1024);
}

size_t packed_floats_of(int v, const ntx_model_desc *d) {   // (the descriptor's architecture sizes the flex family's image)
    const Variant &k = kVariants[v];
    if (k.flex) return packed_floats_flex(flex_arch_of(d));
    const Geometry g = make_geometry(k.n_geo, k.n_app, k.cd, k.ipe);
    return (size_t)(g.padded_records + RING) * REC_FLOATS + g.aux_floats;
}
size_t aux_floats_of_variant(int v) {
    const Variant &k = kVariants[v];
    return k.flex ? (size_t)aux_total() + flex_floats() : (size_t)make_geometry(k.n_geo, k.n_app, k.cd, k.ipe).aux_floats;
}
int no_fp16x3(const Variant &v) {
    return v.flex ? ntx_set_error(NTX_E_UNSUPPORTED, "fp16x3 is built for the 8x256 / skips [4] / color_depth 1 families only; this model's architecture runs on "
                                                     "the float32 layer-loop kernels") : NTX_OK;
}
}  // namespace ntx

extern "C" {

size_t ntx_weight_count(const ntx_model_desc *desc) {
    const int v = find_variant(desc);
    if (v < 0) { unsupported(desc); return 0; }
    return view_blob_of(v, desc).count;
}

size_t ntx_packed_count(const ntx_model_desc *desc) {
    const int v = find_variant(desc);
    if (v < 0) { unsupported(desc); return 0; }
    return packed_floats_of(v, desc);
}

int ntx_pack_weights(const ntx_model_desc *desc, const float *weights_host, size_t n_floats, float *packed_out,
                     size_t n_packed) {
    const int v = find_variant(desc);
    if (v < 0) return unsupported(desc);
    if (!weights_host || !packed_out) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    const size_t want = view_blob_of(v, desc).count;
    if (n_floats != want) return ntx_set_error(NTX_E_INVALID, "weight blob has %zu floats, model needs %zu", n_floats, want);
    if (n_packed != packed_floats_of(v, desc))
        return ntx_set_error(NTX_E_INVALID, "packed buffer has %zu floats, needs %zu", n_packed, packed_floats_of(v, desc));
    if (kVariants[v].flex) pack_flex(flex_arch_of(desc), dims_of(desc), weights_host, packed_out);
    else pack(kVariants[v], dims_of(desc), weights_host, packed_out);
    return NTX_OK;
}

size_t ntx_packed_fp16x3_bytes(const ntx_model_desc *desc) {
    const int v = find_variant(desc);
    if (v < 0) { unsupported(desc); return 0; }
    if (no_fp16x3(kVariants[v])) return 0;
    return packed16_bytes(kVariants[v]);
}

int ntx_pack_weights_fp16x3(const ntx_model_desc *desc, const float *weights_host, size_t n_floats, uint16_t *packed_out,
                            size_t n_bytes) {
    const int v = find_variant(desc);
    if (v < 0) return unsupported(desc);
    if (int rc = no_fp16x3(kVariants[v])) return rc;
    if (!weights_host || !packed_out) return ntx_set_error(NTX_E_INVALID, "NULL buffer");
    const size_t want = view_blob_of(v, desc).count;
    if (n_floats != want) return ntx_set_error(NTX_E_INVALID, "weight blob has %zu floats, model needs %zu", n_floats, want);
    if (n_bytes != packed16_bytes(kVariants[v]))
        return ntx_set_error(NTX_E_INVALID, "packed buffer has %zu bytes, needs %zu", n_bytes, packed16_bytes(kVariants[v]));
    pack16(kVariants[v], dims_of(desc), weights_host, packed_out);
    return NTX_OK;
}

}  // extern "C"
