"""Opt-in bf16x6 training without a GPU: what the header and the binding declare, the refusals that come back before any device is asked for,
the class selection -- and the fairness check of the GPU bar: tests/bf16x6_common.py's numpy restatement of the documented arithmetic stays
within 2 float32 floors of the float64 product on the operand sets tests/test_gpu_gemm_bf16x6.py uses, and leaves them with any one of the six
products left out.  So a kernel that drops or mangles a term cannot pass the GPU file, and one that does what the header says can."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import bf16x6_common as x6

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "nerftex.h")) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------- declarations
def test_the_header_declares_the_entries_and_the_abi_stays_7():
    from nerf_tex_amd import _lib
    h = header()
    assert re.search(r"#define\s+NTX_ABI_VERSION\s+7\b", h) and _lib.ABI_VERSION == 7 and _lib.lib.ntx_abi_version() == 7
    assert re.search(r"typedef enum ntx_precision \{[^}]*NTX_PRECISION_F32 = 0,[^}]*NTX_PRECISION_FP16X3 = 1,[^}]*NTX_PRECISION_BF16X6 = 2[^}]*\} ntx_precision;", h)
    assert re.search(r"\bint ntx_trainer_set_precision\(ntx_trainer \*t, int precision\);", h)
    assert re.search(r"\bint ntx_trainer_precision\(const ntx_trainer \*t\);", h)
    proto = re.search(r"\bint ntx_gemm_bf16x6_ex\(([^;]*)\);", h)
    f32 = re.search(r"\bint ntx_gemm_f32_ex\(([^;]*)\);", h)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
    assert proto and f32 and "ntx_stream" not in proto.group(1)
    assert norm(proto.group(1)) == norm(f32.group(1))[:-1]               # ntx_gemm_f32_ex's list without the trailing stream
    assert norm(f32.group(1))[-1] == "ntx_stream stream"


def test_the_binding_carries_the_signatures():
    from nerf_tex_amd import _lib
    assert _lib.SYMBOLS["ntx_trainer_set_precision"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib.SYMBOLS["ntx_trainer_precision"] == (C.c_int, [C.c_void_p])
    res, args = _lib.SYMBOLS["ntx_gemm_bf16x6_ex"]
    assert res is C.c_int and args == _lib.SYMBOLS["ntx_gemm_f32_ex"][1][:-1]
    assert _lib.TRAIN_PRECISIONS == {"float32": 0, "bf16x6": 2} and _lib.PRECISION_BF16X6 == 2
    for name in ("ntx_trainer_set_precision", "ntx_trainer_precision", "ntx_gemm_bf16x6_ex"):
        assert getattr(_lib.lib, name).argtypes == _lib.SYMBOLS[name][1]


# ---------------------------------------------------------------------------------------------------------------- refusals without a device
def test_the_contraction_refuses_before_it_asks_for_a_device():
    """Bad dimensions, a leading dimension below its row, split ranges, column sums with k-contiguous A: NTX_E_INVALID with host pointers that
    are never read (no launch is reached)."""
    from nerf_tex_amd import _lib
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    M, N, K = 4, 3, 5
    good = dict(A=p, lda=M, ak=0, B=p, ldb=N, C=p, ldc=N, M=M, N=N, K=K, bias=None, relu=0, mask=None, ldmask=0, accumulate=0, n_split=1, k_chunk=0, split_stride=0, colsum=None)
    call = lambda **ch: _lib.lib.ntx_gemm_bf16x6_ex(*dict(good, **ch).values())
    cases = [dict(A=None), dict(B=None), dict(C=None), dict(M=0), dict(N=0), dict(K=0), dict(M=-1),
             dict(lda=M - 1), dict(ak=1, lda=K - 1), dict(ldb=N - 1), dict(ldc=N - 1), dict(mask=p, ldmask=N - 1),
             dict(n_split=0), dict(n_split=65536), dict(n_split=2, k_chunk=0, split_stride=M * N), dict(n_split=2, k_chunk=2, split_stride=M * N),
             dict(n_split=2, k_chunk=5, split_stride=M * N), dict(n_split=2, k_chunk=3, split_stride=M * N - 1),
             dict(ak=1, lda=K, colsum=p)]
    for ch in cases:
        assert call(**ch) == _lib.NTX_E_INVALID, ch
        assert _lib.lib.ntx_last_error()
    assert not buf.any()


def test_set_precision_refuses_null():
    from nerf_tex_amd import _lib
    for prec in (0, 1, 2, 3, -1):
        assert _lib.lib.ntx_trainer_set_precision(None, prec) == _lib.NTX_E_INVALID
    assert _lib.lib.ntx_trainer_precision(None) == -1


def test_class_selection():
    """`precision="bf16x6"` names the layer-by-layer class also for the chain's own 8 x 256 shape, and raises together with `fused=True`."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer, Trainer, trainer_class_for
    from tests.common import make_model
    chain_model = make_model((1, 6))[0]
    assert trainer_class_for(chain_model) is Trainer and trainer_class_for(chain_model, precision="float32") is Trainer
    assert trainer_class_for(chain_model, precision="bf16x6") is FlexTrainer
    with pytest.raises(_lib.NtxError) as e:
        trainer_class_for(chain_model, precision="bf16x6", fused=True)
    assert e.value.code == _lib.NTX_E_UNSUPPORTED
    assert trainer_class_for(chain_model, precision="float32", fused=True) is Trainer
    other = make_model((1, 6), arch=dict(depth=6))[0]
    assert trainer_class_for(other, precision="bf16x6") is FlexTrainer
    branches = make_model((1, 6), arch=dict(depth=5, skips=[2], param_depth=2))[0]
    assert trainer_class_for(branches, branches=True, precision="bf16x6") is BranchTrainer
    with pytest.raises(_lib.NtxError) as e:
        trainer_class_for(chain_model, precision="fp16x3")
    assert e.value.code == _lib.NTX_E_UNSUPPORTED
    with pytest.raises(ValueError):
        trainer_class_for(chain_model, precision="bf16")


# ---------------------------------------------------------------------------------------------------------------- the emulation
@pytest.fixture(scope="module")
def measured():
    """{(set, range): (floor, the emulation's error, {left-out product: error})}, computed once"""
    out = {}
    for name in x6.operand_sets():
        for z, (A, B) in enumerate(x6.ranges(name)):
            ref = A.astype(np.float64) @ B.astype(np.float64)
            out[name, z] = (x6.floor32(A, B), x6.rowwise(x6.emulate(A, B), ref), {p: x6.rowwise(x6.emulate(A, B, leave_out=p), ref) for p in x6.ORDER})
    return out


def test_the_split_is_exact_and_in_bf16():
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-30, 30, 4096)).astype(np.float32)
    terms = x6.split3(v)
    for t in terms:
        assert not (t.view(np.uint32) & 0xFFFF).any()                     # 16 low bits clear: a bf16
    total = terms[0].astype(np.float64) + terms[1].astype(np.float64) + terms[2].astype(np.float64)
    assert np.array_equal(total, v.astype(np.float64))                     # 3 x 8 mantissa bits hold a float32
    assert np.array_equal(x6.bf16_rne(np.asarray([1.00390625, 1.01171875], np.float32)), np.asarray([1.0, 1.015625], np.float32))      # ties go to even


def test_the_documented_arithmetic_meets_the_gpu_bar(measured):
    """On every operand set and range of the GPU file: within 2 float32 floors, and within the project's 2e-6 sqrt(K)."""
    for (name, z), (floor, err, _) in measured.items():
        K = x6.ranges(name)[z][0].shape[1]
        print(f"{name} range {z}: K {K} floor {floor:.3e} emulation {err:.3e} = {err / floor:.2f} floors")
        assert 1e-8 < floor < 2e-6
        assert err <= x6.FLOORS * floor and err <= 2e-6 * np.sqrt(K)


def test_any_product_left_out_misses_the_gpu_bar(measured):
    """Without a0b0 or a first-order product the error is thousands of floors; without a second-order one still beyond the bar."""
    for (name, z), (floor, _, left_out) in measured.items():
        for p, err in left_out.items():
            print(f"{name} range {z}: without a{p[0]}b{p[1]} {err / floor:.1f} floors")
            assert err > x6.FLOORS * floor, (name, z, p)
            if sum(p) < 2:
                assert err > 1000 * floor, (name, z, p)
