// ntx_pack.h -- the host-only weight packers (ntx_pack.cpp) as the context (nerftex.hip) uses them: the sizes of a model's images and the
// fp16x3 emitter with its two streams.  The float32 images go through the ABI's ntx_pack_weights.  Plain C++.
#pragma once
#include "ntx_arch.h"
#include <cstdint>

namespace ntx {
size_t packed_floats_of(int v, const ntx_model_desc *d);   // v: the descriptor's family (find_variant)
size_t aux_floats_of_variant(int v);
int no_fp16x3(const Variant &v);                            // NTX_OK, or the error of a family without fp16x3 kernels
size_t packed16_bytes(const Variant &v, int with_dir = 0);
// with_dir: the stream of the kernels with per-sample directions, where C1 keeps its direction segment
void pack16(const Variant &v, Dims m, const float *blob, uint16_t *out, int with_dir = 0);
}  // namespace ntx
