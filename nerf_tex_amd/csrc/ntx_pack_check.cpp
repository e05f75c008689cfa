// ntx_pack_check.cpp -- `make pack_check`: the weight packers of ntx_pack.cpp under AddressSanitizer and UBSan, on the CPU.  Every model the
// dispatch tells apart is packed with its blob and its images on the heap at EXACTLY the sizes the count functions return, so a read or a
// write one element outside any of them stops the program.  Cases: tools/pack_fingerprint.py's.  Exit status 0: every pack returned NTX_OK,
// every refused descriptor was refused, and neither sanitizer had anything to say.
#include "ntx_pack.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>

static char g_err[512];
extern "C" int ntx_set_error(int code, const char *fmt, ...) {   // the library's is nerftex.hip's
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

using namespace ntx;
constexpr int M = NTX_SKIP_MASK;
struct Case { const char *name; ntx_model_desc_ex d; bool refused; };
#define D(...) {{__VA_ARGS__}, 0, 0, {0}}
#define DX(pd, pw, ...) {{__VA_ARGS__}, pd, pw, {0}}
// the list of tools/pack_fingerprint.py (CASES), in its order: a case added here goes there too
static const Case kCases[] = {
    {"tuned [1,6]", D(0, 1, 6, 3, 10, 4, 4, 8, 256, 4, 1, 0)}, {"tuned [1,4]", D(0, 1, 4, 3, 10, 4, 4, 8, 256, 4, 1, 0)},
    {"tuned [2,3]", D(0, 2, 3, 3, 10, 4, 4, 8, 256, 4, 1, 0)}, {"Nerf", D(1, 0, 0, 3, 10, 4, 0, 8, 256, 4, 0, 0)},
    {"IPE [1,3]", D(0, 1, 3, 6, 10, 4, 4, 8, 256, 4, 1, 1)},
    {"generic [4,8]", D(0, 4, 8, 3, 10, 4, 4, 8, 256, 4, 1, 0)}, {"generic [0,0]", D(0, 0, 0, 3, 10, 4, 4, 8, 256, 4, 1, 0)},
    {"generic [3,1]", D(0, 3, 1, 3, 10, 4, 4, 8, 256, 4, 1, 0)},
    {"bands (3,0,-) Nerf", D(1, 0, 0, 3, 3, 0, 0, 8, 256, 4, 0, 0)}, {"bands (9,3,2) [1,6]", D(0, 1, 6, 3, 9, 3, 2, 8, 256, 4, 1, 0)},
    {"bands (0,0,0) [2,3]", D(0, 2, 3, 3, 0, 0, 0, 8, 256, 4, 1, 0)}, {"bands IPE pos_freq 4", D(0, 1, 3, 6, 4, 4, 4, 8, 256, 4, 1, 1)},
    {"flex 1x2 cd0", D(0, 1, 6, 3, 10, 4, 4, 1, 2, -1, 0, 0)}, {"flex 24x256 cd4", D(0, 4, 8, 3, 10, 4, 4, 24, 256, M | 0x7fffff, 4, 0)},
    {"flex 6x128 skips 0b01010", D(0, 1, 6, 3, 10, 4, 4, 6, 128, M | 0b01010, 1, 0)}, {"flex Nerf 4x64", D(1, 0, 0, 3, 10, 4, 0, 4, 64, 1, 0, 0)},
    {"flex skip index >= depth", D(0, 1, 4, 3, 10, 4, 4, 4, 128, 7, 1, 0)},
    {"branches pd1 pw2", DX(1, 2, 2, 1, 6, 3, 10, 4, 4, 8, 256, 4, 1, 0)}, {"branches pd4 pw128", DX(4, 128, 2, 4, 8, 3, 10, 4, 4, 24, 256, M | 0x7fffff, 4, 0)},
    {"branches geometry only [2,0]", DX(2, 64, 2, 2, 0, 3, 10, 4, 3, 3, 64, 0, 1, 0)}, {"branches appearance only [0,3]", DX(2, 100, 2, 0, 3, 3, 10, 4, 4, 3, 64, -1, 2, 0)},
    {"param_depth without parameters", DX(2, 128, 2, 0, 0, 3, 10, 4, 4, 4, 128, 2, 1, 0)},
    // tests/test_host.py: test_unsupported_desc_is_rejected_on_host
    {"refused", D(0, 5, 3, 3, 10, 4, 4, 8, 256, 4, 1, 0), true}, {"refused", D(0, 1, 9, 3, 10, 4, 4, 8, 256, 4, 1, 0), true},
    {"refused", D(0, 1, 6, 3, 11, 4, 4, 8, 256, 4, 1, 0), true}, {"refused", D(0, 1, 6, 3, 10, 5, 4, 8, 256, 4, 1, 0), true},
    {"refused", D(0, 1, 6, 3, 10, 4, 5, 8, 256, 4, 1, 0), true}, {"refused", D(0, 1, 6, 3, -1, 4, 4, 8, 256, 4, 1, 0), true},
    {"refused", D(0, 1, 3, 3, 10, 4, 4, 8, 256, 4, 1, 1), true}, {"refused", D(0, 1, 6, 6, 10, 4, 4, 8, 256, 4, 1, 1), true},
    {"refused", D(0, 1, 6, 3, 10, 4, 4, 25, 256, 4, 1, 0), true}, {"refused", D(0, 1, 6, 3, 10, 4, 4, 8, 257, 4, 1, 0), true},
    {"refused", D(0, 1, 6, 3, 10, 4, 4, 8, 256, 4, 5, 0), true}, {"refused", D(0, 1, 6, 3, 10, 4, 4, 8, 256, 7, 1, 0), true},
    {"refused", D(0, 1, 6, 3, 10, 4, 4, 6, 128, M | 0b100100, 1, 0), true}, {"refused", D(0, 1, 3, 6, 10, 4, 4, 6, 256, 4, 1, 1), true},
    {"refused", D(0, 1, 6, 3, 10, 4, 4, 0, 256, 4, 1, 0), true}, {"refused", D(0, 1, 6, 3, 10, 4, 4, 8, 1, 4, 1, 0), true},
};

static int fail(const char *name, const char *what) {
    fprintf(stderr, "pack_check: %s: %s (%s)\n", name, what, g_err);
    return 1;
}

// returns 0 when the case went as it should; want_variant >= 0: the family the dispatch must choose
static int run(const Case &c, int want_variant = -1) {
    const ntx_model_desc *d = &c.d.base;
    const int v = find_variant(d);
    const size_t n = ntx_weight_count(d), np = ntx_packed_count(d);
    if (c.refused) {
        if (v >= 0 || n || np || ntx_packed_fp16x3_bytes(d)) return fail(c.name, "a descriptor that must be refused was taken");
        printf("ok  refused: %.60s ...\n", g_err);
        return 0;
    }
    if (v < 0 || n == 0 || np == 0) return fail(c.name, "refused");
    if (want_variant >= 0 && v != want_variant) return fail(c.name, "the dispatch chose another family");
    if ((param_depth_of(d) > 0) != (v == kFlexParamVariant)) return fail(c.name, "branch path and param_depth disagree");
    std::unique_ptr<float[]> blob(new float[n]), out(new float[np]);
    for (size_t i = 0; i < n; ++i) blob[i] = (float)(i + 1);
    if (ntx_pack_weights(d, blob.get(), n, out.get(), np) != NTX_OK) return fail(c.name, "ntx_pack_weights");
    size_t bytes = 0, bytes_dir = 0;
    if (!kVariants[v].flex) {   // fp16x3 where built: the ABI's stream, and the one with C1's direction segment
        bytes = ntx_packed_fp16x3_bytes(d);
        if (bytes == 0 || bytes != packed16_bytes(kVariants[v])) return fail(c.name, "ntx_packed_fp16x3_bytes");
        std::unique_ptr<uint16_t[]> o16(new uint16_t[bytes / 2]);
        if (ntx_pack_weights_fp16x3(d, blob.get(), n, o16.get(), bytes) != NTX_OK) return fail(c.name, "ntx_pack_weights_fp16x3");
        bytes_dir = packed16_bytes(kVariants[v], 1);
        std::unique_ptr<uint16_t[]> o16d(new uint16_t[bytes_dir / 2]);
        pack16(kVariants[v], dims_of(d), blob.get(), o16d.get(), 1);
    } else if (ntx_packed_fp16x3_bytes(d) != 0) return fail(c.name, "fp16x3 on the flex family");
    printf("ok  %-34s family %d  %7zu weights -> %7zu floats, fp16x3 %7zu / %7zu bytes\n", c.name, v, n, np, bytes, bytes_dir);
    return 0;
}

int main() {
    int bad = 0;
    unsetenv("NERFTEX_FORCE_FLEX"); unsetenv("NERFTEX_FORCE_GENERIC");
    for (const Case &c : kCases) bad += run(c);
    const Case carpet{"tuned [1,6] under NERFTEX_FORCE_FLEX", kCases[0].d, false}, mip{"IPE under NERFTEX_FORCE_FLEX (stays tuned)", kCases[4].d, false},
        generic{"tuned [1,6] under NERFTEX_FORCE_GENERIC", kCases[0].d, false};
    setenv("NERFTEX_FORCE_FLEX", "1", 1);
    bad += run(carpet, kFlexVariant) + run(mip, 4);
    unsetenv("NERFTEX_FORCE_FLEX"); setenv("NERFTEX_FORCE_GENERIC", "1", 1);
    bad += run(generic, 5);
    printf("pack_check: %d of %zu cases failed\n", bad, sizeof(kCases) / sizeof(kCases[0]) + 3);
    return bad ? 1 : 0;
}
