"""The opt-in fp8 (e4m3) path of the UNets' feed-forward linears without a GPU: its three entry points are declared, exported and bound; the
argument checks of mrag_gemm_fp8_k64 / mrag_layernorm_e4m3 return before any launch (so they can be called here with made-up addresses);
ops.fp8_linear_k64_supported says what the header says; layers.set_ff_precision marks exactly the FeedForward modules and validates its arguments."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mrag_layernorm_e4m3", "mrag_gemm_fp8_k64", "mrag_gemm_fp8_k64_launch_counts")
EPI_NONE, EPI_GELU_TANH, EPI_GELU_ERF, EPI_RESID, EPI_GATE_RESID, EPI_SILU, EPI_GEGLU = range(7)


def test_ff_fp8_symbols_declared_exported_and_bound():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.mrag_gemm_fp8_k64.argtypes == [ctypes.c_void_p, ctypes.POINTER(_lib.GemmFp8Args)]       # the existing argument block, unchanged
    assert len(L.mrag_layernorm_e4m3.argtypes) == 11 and L.mrag_layernorm_e4m3.argtypes[4] is ctypes.c_float
    assert _lib.ABI_VERSION == 11 and L.mrag_abi_version() == 11
    # the counters answer without a device: two slots of their own; mrag_fp8_launch_counts keeps its two
    buf = (ctypes.c_uint64 * 3)(1 << 63, 1 << 63, 1 << 63)
    assert L.mrag_gemm_fp8_k64_launch_counts(buf, 3) == 2 and max(buf[0], buf[1]) < (1 << 63) and buf[2] == 1 << 63
    one = (ctypes.c_uint64 * 2)(0, 1 << 63)
    assert L.mrag_gemm_fp8_k64_launch_counts(one, 1) == 2 and one[0] == buf[0] and one[1] == 1 << 63
    assert L.mrag_gemm_fp8_k64_launch_counts(None, 0) == 2
    assert L.mrag_fp8_launch_counts(None, 0) == 2


def _args(M=64, N=256, K=320, epilogue=EPI_NONE, **over):
    """a well-formed argument block over made-up (aligned, never dereferenced) device addresses"""
    from motionrag_amd import _lib
    a = _lib.GemmFp8Args()
    a.A8, a.W8, a.a_exp, a.w_exp, a.C = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    a.epilogue = epilogue
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _counts(L):
    k64, lin = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)()
    L.mrag_gemm_fp8_k64_launch_counts(k64, 2)
    L.mrag_fp8_launch_counts(lin, 2)
    return list(k64), list(lin)


def test_gemm_fp8_k64_argument_checks_return_before_any_launch():
    from motionrag_amd import _lib
    L = _lib.lib()
    call = lambda a: L.mrag_gemm_fp8_k64(None, ctypes.byref(a))
    before = _counts(L)
    assert L.mrag_gemm_fp8_k64(None, None) == _lib.MRAG_EINVAL
    assert call(_args(K=96, lda=96, ldw=96)) == _lib.MRAG_ENOTSUP                # K % 64
    assert call(_args(N=48, ldc=24, epilogue=EPI_GEGLU)) == _lib.MRAG_ENOTSUP    # GEGLU wants whole 32-row groups
    assert call(_args(N=24, ldc=24)) == _lib.MRAG_ENOTSUP                        # N % 16
    for epi in (EPI_GELU_TANH, EPI_GELU_ERF, EPI_GATE_RESID, EPI_SILU, 7):
        assert call(_args(epilogue=epi)) == _lib.MRAG_ENOTSUP, epi               # epilogues this entry point does not have
    for field in ("A8", "W8", "a_exp", "w_exp", "C"):
        assert call(_args(**{field: None})) == _lib.MRAG_EINVAL, field            # null pointer
    assert call(_args(A8=0x100008)) == _lib.MRAG_EINVAL                          # misaligned operand rows
    assert call(_args(W8=0x200004)) == _lib.MRAG_EINVAL
    assert call(_args(lda=328)) == _lib.MRAG_EINVAL
    assert call(_args(C=0x500008)) == _lib.MRAG_EINVAL
    assert call(_args(a_exp=0x300002)) == _lib.MRAG_EINVAL
    assert call(_args(bias=0x600004)) == _lib.MRAG_EINVAL
    assert call(_args(epilogue=EPI_RESID)) == _lib.MRAG_EINVAL                   # residual epilogue without a residual
    assert call(_args(epilogue=EPI_RESID, resid=0x600008, ldr=256)) == _lib.MRAG_EINVAL
    assert call(_args(epilogue=EPI_GEGLU, ldc=64)) == _lib.MRAG_EINVAL           # C is [M, N / 2]: ldc >= 128
    assert call(_args(M=0)) == _lib.MRAG_EINVAL
    ln = lambda x, x8, ex, M, K, ldx, ld8, gamma=None, beta=None: L.mrag_layernorm_e4m3(None, x, gamma, beta, 1e-5, x8, ex, M, K, ldx, ld8)
    assert ln(None, 0x200000, 0x300000, 4, 320, 320, 320) == _lib.MRAG_EINVAL
    assert ln(0x100000, None, 0x300000, 4, 320, 320, 320) == _lib.MRAG_EINVAL
    assert ln(0x100000, 0x200000, None, 4, 320, 320, 320) == _lib.MRAG_EINVAL
    assert ln(0x100000, 0x200000, 0x300000, 0, 320, 320, 320) == _lib.MRAG_EINVAL
    assert ln(0x100000, 0x200000, 0x300000, 4, 72, 72, 80) == _lib.MRAG_ENOTSUP   # K % 16
    assert ln(0x100000, 0x200000, 0x300000, 4, 320, 324, 320) == _lib.MRAG_ENOTSUP   # rows of x not 16-byte aligned
    assert ln(0x100000, 0x200008, 0x300000, 4, 320, 320, 320) == _lib.MRAG_ENOTSUP   # rows of x8
    assert ln(0x100000, 0x200000, 0x300000, 4, 320, 320, 320, gamma=0x700002) == _lib.MRAG_ENOTSUP
    assert ln(0x100000, 0x200000, 0x300000, 4, 4096, 4096, 4096) == _lib.MRAG_ENOTSUP   # wider than a row kept in registers
    assert _counts(L) == before                                                   # none of the refused calls counted as a launch


def test_fp8_k64_ops_refuse_cpu_tensors_and_state_their_shapes():
    from motionrag_amd import ops
    x = torch.zeros(4, 320, dtype=torch.bfloat16)
    with pytest.raises(ops.HipOnly):
        ops.layernorm_e4m3(x, None, None, 1e-5)
    with pytest.raises(ops.HipOnly):
        ops.linear_fp8_k64(x, torch.zeros(16, 320, dtype=torch.uint8), torch.zeros(16, dtype=torch.int32))
    # include/mrag_hip.h, mrag_gemm_fp8_k64: "MRAG_ENOTSUP unless K % 64 == 0 and N % 16 == 0 (MRAG_EPI_GEGLU: N % 32 == 0), and for every epilogue
    # but MRAG_EPI_NONE, MRAG_EPI_RESID and MRAG_EPI_GEGLU"
    hdr_says = lambda N, K, epi: epi in (EPI_NONE, EPI_RESID, EPI_GEGLU) and K % 64 == 0 and N % (32 if epi == EPI_GEGLU else 16) == 0
    cases = [(2560, 320, EPI_GEGLU), (320, 1280, EPI_RESID), (5120, 640, EPI_GEGLU), (10240, 1280, EPI_GEGLU), (640, 2560, EPI_RESID), (16, 64, EPI_NONE),
             (48, 64, EPI_GEGLU), (48, 64, EPI_NONE), (24, 128, EPI_NONE), (256, 96, EPI_NONE), (256, 32, EPI_RESID), (256, 128, EPI_GELU_TANH),
             (256, 128, EPI_GATE_RESID), (256, 128, EPI_GELU_ERF), (256, 128, EPI_SILU), (0, 128, EPI_NONE)]
    for N, K, epi in cases:
        assert ops.fp8_linear_k64_supported(N, K, epi) == (N > 0 and hdr_says(N, K, epi)), (N, K, epi)
    assert ops.fp8_linear_k64_supported(320, 1280)                                # the epilogue defaults to EPI_NONE
    assert not ops.fp8_linear_supported(2560, 320)                                # the entry point it extends keeps its refusal


def _small_blocks():
    from motionrag_amd import dynamicrafter, svd_unet
    dc = dynamicrafter.BasicTransformerBlock(64, 1, 64, context_dim=64)
    sv = svd_unet.TemporalBasicTransformerBlock(64, 64, 1, 64, 64)
    return dc, sv


def test_set_ff_precision_marks_the_feedforwards_and_validates():
    from torch import nn
    from motionrag_amd import dynamicrafter, layers, svd_unet
    dc, sv = _small_blocks()
    both = nn.ModuleList([dc, sv])
    ffs = [m for m in both.modules() if isinstance(m, (dynamicrafter.FeedForward, svd_unet.FeedForward))]
    assert len(ffs) == 3 and {id(m) for m in ffs} == {id(dc.ff), id(sv.ff_in), id(sv.ff)}
    marked = lambda: {id(m): getattr(m, layers.FF_SITES_ATTR) for m in both.modules() if hasattr(m, layers.FF_SITES_ATTR)}
    assert marked() == {}                                                         # a fresh model is bf16: nothing is marked
    for bad in ("fp16", "e4m3", "", None):
        with pytest.raises(ValueError):
            layers.set_ff_precision(both, bad)
    with pytest.raises(ValueError):
        layers.set_ff_precision(both, "fp8", sites=("ff1", "to_out"))
    with pytest.raises(ValueError):
        layers.set_ff_precision(both, "fp8", sites=())
    assert marked() == {}                                                         # a refused call changes nothing
    assert layers.set_ff_precision(both, "fp8") is both
    assert marked() == {id(m): ("ff1", "ff2") for m in ffs}                       # exactly the FeedForward modules
    layers.set_ff_precision(dc, "fp8", sites=("ff2",))
    assert getattr(dc.ff, layers.FF_SITES_ATTR) == ("ff2",) and getattr(sv.ff, layers.FF_SITES_ATTR) == ("ff1", "ff2")
    layers.set_ff_precision(both, "bf16")
    assert marked() == {id(m): () for m in ffs}
    other, _ = _small_blocks()
    layers.set_ff_precision(both, "fp8")
    assert not hasattr(other.ff, layers.FF_SITES_ATTR)                            # per module, not per class
    assert isinstance(layers.FF_FP8_MIN_ROWS, int) and layers.FF_FP8_MIN_ROWS > 0 and layers.FF2_FP8_MIN_ROWS > 0 and layers.FF2_FP8_MIN_WIDTH > 0
