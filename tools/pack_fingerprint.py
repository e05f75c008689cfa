"""The weight packers' bytes, as hashes: one JSON line per model descriptor with `ntx_weight_count`, `ntx_packed_count`, the sha256 of the
float32 image of a seeded random blob and of the blob i + 1, `ntx_packed_fp16x3_bytes` and the sha256 of that image where the family has
fp16x3 kernels -- or, for a descriptor the library refuses, the return values and the whole `ntx_last_error()` text.  The cases are the
descriptors of tests/test_host.py's pack tests plus the edges of the dispatch (nerf_tex_amd/csrc/ntx_arch.h: find_variant); `make -C
nerf_tex_amd/csrc pack_check` runs the same list under the sanitizers.  Runs on the CPU.  A change that only moves code prints what its parent prints:
    NERFTEX_LIB=<parent's libnerftex_hip.so> python tools/pack_fingerprint.py > parent.jsonl
    python tools/pack_fingerprint.py > new.jsonl && cmp parent.jsonl new.jsonl
With a GPU it adds one line per tuned ParamNerf family: the sha256 of `ntx_mlp_forward(..., NTX_FLAG_FP16X3)` on 64 seeded samples, the
one way through the ABI to the fp16x3 image that keeps the colour layer's direction segment.  Exits non-zero when a case raised."""

import ctypes as C
import hashlib
import json
import os
import sys
import traceback

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nerf_tex_amd import _lib                                 # noqa: E402

F, M = np.float32, _lib.SKIP_MASK
fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint16)
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
ALL23 = M | 0x7fffff                                          # skips = every trunk layer but the last of 24

# (name, the twelve fields of ntx_model_desc [, param_depth, param_width], environment).  nerf_tex_amd/csrc/ntx_pack_check.cpp has the same list as
# C initialisers (kCases): a case added here goes there too
CASES = [
    ("tuned [1,6]", (0, 1, 6, 3, 10, 4, 4, 8, 256, 4, 1, 0)), ("tuned [1,4]", (0, 1, 4, 3, 10, 4, 4, 8, 256, 4, 1, 0)),
    ("tuned [2,3]", (0, 2, 3, 3, 10, 4, 4, 8, 256, 4, 1, 0)), ("Nerf", (1, 0, 0, 3, 10, 4, 0, 8, 256, 4, 0, 0)),
    ("IPE [1,3]", (0, 1, 3, 6, 10, 4, 4, 8, 256, 4, 1, 1)),
    ("generic [4,8]", (0, 4, 8, 3, 10, 4, 4, 8, 256, 4, 1, 0)), ("generic [0,0]", (0, 0, 0, 3, 10, 4, 4, 8, 256, 4, 1, 0)),
    ("generic [3,1]", (0, 3, 1, 3, 10, 4, 4, 8, 256, 4, 1, 0)),
    ("bands (3,0,-) Nerf", (1, 0, 0, 3, 3, 0, 0, 8, 256, 4, 0, 0)), ("bands (9,3,2) [1,6]", (0, 1, 6, 3, 9, 3, 2, 8, 256, 4, 1, 0)),
    ("bands (0,0,0) [2,3]", (0, 2, 3, 3, 0, 0, 0, 8, 256, 4, 1, 0)), ("bands IPE pos_freq 4", (0, 1, 3, 6, 4, 4, 4, 8, 256, 4, 1, 1)),
    ("flex 1x2 cd0", (0, 1, 6, 3, 10, 4, 4, 1, 2, -1, 0, 0)), ("flex 24x256 cd4", (0, 4, 8, 3, 10, 4, 4, 24, 256, ALL23, 4, 0)),
    ("flex 6x128 skips 0b01010", (0, 1, 6, 3, 10, 4, 4, 6, 128, M | 0b01010, 1, 0)), ("flex Nerf 4x64", (1, 0, 0, 3, 10, 4, 0, 4, 64, 1, 0, 0)),
    ("flex skip index >= depth", (0, 1, 4, 3, 10, 4, 4, 4, 128, 7, 1, 0)),
    ("branches pd1 pw2", (2, 1, 6, 3, 10, 4, 4, 8, 256, 4, 1, 0, 1, 2)), ("branches pd4 pw128", (2, 4, 8, 3, 10, 4, 4, 24, 256, ALL23, 4, 0, 4, 128)),
    ("branches geometry only [2,0]", (2, 2, 0, 3, 10, 4, 3, 3, 64, 0, 1, 0, 2, 64)), ("branches appearance only [0,3]", (2, 0, 3, 3, 10, 4, 4, 3, 64, -1, 2, 0, 2, 100)),
    ("param_depth without parameters", (2, 0, 0, 3, 10, 4, 4, 4, 128, 2, 1, 0, 2, 128)),
    # the same 8 x 256 model on the other families' kernels; an IPE model stays where it is
    ("tuned [1,6] under NERFTEX_FORCE_FLEX", (0, 1, 6, 3, 10, 4, 4, 8, 256, 4, 1, 0), "NERFTEX_FORCE_FLEX"),
    ("tuned [1,6] under NERFTEX_FORCE_GENERIC", (0, 1, 6, 3, 10, 4, 4, 8, 256, 4, 1, 0), "NERFTEX_FORCE_GENERIC"),
    ("IPE [1,3] under NERFTEX_FORCE_FLEX", (0, 1, 3, 6, 10, 4, 4, 8, 256, 4, 1, 1), "NERFTEX_FORCE_FLEX"),
] + [("refused %d" % i, d) for i, d in enumerate([                   # tests/test_host.py: test_unsupported_desc_is_rejected_on_host
    (0, 5, 3, 3, 10, 4, 4, 8, 256, 4, 1, 0), (0, 1, 9, 3, 10, 4, 4, 8, 256, 4, 1, 0), (0, 1, 6, 3, 11, 4, 4, 8, 256, 4, 1, 0), (0, 1, 6, 3, 10, 5, 4, 8, 256, 4, 1, 0),
    (0, 1, 6, 3, 10, 4, 5, 8, 256, 4, 1, 0), (0, 1, 6, 3, -1, 4, 4, 8, 256, 4, 1, 0), (0, 1, 3, 3, 10, 4, 4, 8, 256, 4, 1, 1), (0, 1, 6, 6, 10, 4, 4, 8, 256, 4, 1, 1),
    (0, 1, 6, 3, 10, 4, 4, 25, 256, 4, 1, 0), (0, 1, 6, 3, 10, 4, 4, 8, 257, 4, 1, 0), (0, 1, 6, 3, 10, 4, 4, 8, 256, 4, 5, 0), (0, 1, 6, 3, 10, 4, 4, 8, 256, 7, 1, 0),
    (0, 1, 6, 3, 10, 4, 4, 6, 128, M | 0b100100, 1, 0), (0, 1, 3, 6, 10, 4, 4, 6, 256, 4, 1, 1), (0, 1, 6, 3, 10, 4, 4, 0, 256, 4, 1, 0), (0, 1, 6, 3, 10, 4, 4, 8, 1, 4, 1, 0)])]
GPU_FAMILIES = [c for c in CASES[:5] if c[1][0] == 0]               # tuned, with a colour layer


def last_error():
    return _lib.lib.ntx_last_error().decode("utf-8", "replace")


def host_case(desc):
    lib, d = _lib.lib, _lib.ModelDesc(*desc)
    n, npk = lib.ntx_weight_count(C.byref(d)), lib.ntx_packed_count(C.byref(d))
    out = {"desc": list(desc), "weight_count": n, "packed_count": npk}
    if n == 0:                                                 # refused: what every entry answers, and why
        dummy = np.zeros(4, F)
        out["pack_weights"] = lib.ntx_pack_weights(C.byref(d), dummy.ctypes.data_as(fp), 4, dummy.ctypes.data_as(fp), 4)
        out["packed_fp16x3_bytes"] = lib.ntx_packed_fp16x3_bytes(C.byref(d))
        out["error"] = last_error()
        return out
    image = np.empty(npk, F)
    blobs = {"random": np.random.default_rng(n).normal(size=n).astype(F), "iota": np.arange(1, n + 1, dtype=F)}
    for name, blob in blobs.items():
        _lib.check(lib.ntx_pack_weights(C.byref(d), blob.ctypes.data_as(fp), n, image.ctypes.data_as(fp), npk))
        out["f32_" + name] = sha(image)
    nb = out["packed_fp16x3_bytes"] = lib.ntx_packed_fp16x3_bytes(C.byref(d))
    if nb == 0:
        out["fp16x3_error"] = last_error()
    else:
        image16 = np.empty(nb // 2, np.uint16)
        _lib.check(lib.ntx_pack_weights_fp16x3(C.byref(d), blobs["random"].ctypes.data_as(fp), n, image16.ctypes.data_as(up), nb))
        out["fp16x3_random"] = sha(image16)
    return out


def gpu_case(desc):
    """color / sigma of the fp16x3 MLP kernel on 64 seeded samples: one tiny launch"""
    import torch
    lib, d, dev = _lib.lib, _lib.ModelDesc(*desc), torch.device("cuda", 0)
    n, m, rng = lib.ntx_weight_count(C.byref(d)), 64, np.random.default_rng(7)
    blob = (rng.normal(size=n) * 0.05).astype(F)
    ctx = C.c_void_p()
    _lib.check(lib.ntx_create(C.byref(d), blob.ctypes.data_as(fp), n, 0, C.byref(ctx)))
    try:
        pos, dirs, par = (torch.as_tensor(rng.uniform(-1, 1, size=(m, k)).astype(F), device=dev) for k in (d.n_pos, 3, d.n_geo + d.n_app + d.pos_encoding))   # an IPE model's rows carry the blur parameter too
        color, sigma = torch.empty((m, 3), device=dev), torch.empty((m, 1), device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ntx_mlp_forward(ctx, pos.data_ptr(), dirs.data_ptr(), par.data_ptr(), m, _lib.FLAG_FP16X3, color.data_ptr(), sigma.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
        if not torch.isfinite(color).all() or not color.any():
            raise ValueError("the colour is not finite, or all zero")
        return {"desc": list(desc), "color": sha(color.cpu().numpy()), "sigma": sha(sigma.cpu().numpy())}
    finally:
        lib.ntx_destroy(ctx)


def main():
    import torch
    for knob in ("NERFTEX_FORCE_FLEX", "NERFTEX_FORCE_GENERIC"):
        os.environ.pop(knob, None)
    runs = [("pack " + c[0], lambda c=c: host_case(c[1]), c[2] if len(c) > 2 else None) for c in CASES]
    if torch.cuda.is_available():
        runs += [("mlp fp16x3 " + c[0], lambda c=c: gpu_case(c[1]), None) for c in GPU_FAMILIES]
    for name, run, env in runs:
        if env:
            os.environ[env] = "1"                              # (find_variant asks the process environment at every call)
        try:
            print(json.dumps({"case": name, **run()}), flush=True)
        except Exception:                                      # (nothing more is started on a device that may just have faulted)
            print(json.dumps({"case": name, "error": traceback.format_exc(limit=3)}), flush=True)
            return 1
        finally:
            if env:
                del os.environ[env]
    return 0


if __name__ == "__main__":
    sys.exit(main())
