"""The opt-in fp8 (e4m3) linear path without a GPU: its three entry points are declared, exported and bound; the argument checks of
mrag_gemm_fp8 / mrag_quant_rows_e4m3 return before any launch (so they can be called here with made-up addresses); the torch front end refuses
CPU tensors; cogvideox.set_linear_precision validates its arguments and a fresh model is bf16."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mrag_quant_rows_e4m3", "mrag_gemm_fp8", "mrag_fp8_launch_counts")
EPI_NONE, EPI_GELU_TANH, EPI_RESID, EPI_GATE_RESID, EPI_GEGLU = 0, 1, 3, 4, 6


def test_fp8_symbols_declared_exported_and_bound():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "gemm_fp8.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 11 and _lib.lib().mrag_abi_version() == 11
    # the ctypes struct follows the header's typedef field for field
    body = re.search(r"typedef struct mrag_gemm_fp8_args \{(.*?)\} mrag_gemm_fp8_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.GemmFp8Args._fields_]
    # the counters answer without a device: two slots; a short buffer gets only what it holds
    buf = (ctypes.c_uint64 * 2)(1 << 63, 1 << 63)
    assert _lib.lib().mrag_fp8_launch_counts(buf, 2) == 2 and max(buf) < (1 << 63)
    one = (ctypes.c_uint64 * 2)(0, 1 << 63)
    assert _lib.lib().mrag_fp8_launch_counts(one, 1) == 2 and one[0] == buf[0] and one[1] == 1 << 63
    assert _lib.lib().mrag_fp8_launch_counts(None, 0) == 2


def _args(M=64, N=256, K=256, epilogue=EPI_NONE, **over):
    """a well-formed argument block over made-up (aligned, never dereferenced) device addresses"""
    from motionrag_amd import _lib
    a = _lib.GemmFp8Args()
    a.A8, a.W8, a.a_exp, a.w_exp, a.C = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    a.epilogue = epilogue
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_gemm_fp8_argument_checks_return_before_any_launch():
    from motionrag_amd import _lib
    L = _lib.lib()
    call = lambda a: L.mrag_gemm_fp8(None, ctypes.byref(a))
    before = (ctypes.c_uint64 * 2)()
    L.mrag_fp8_launch_counts(before, 2)
    assert L.mrag_gemm_fp8(None, None) == _lib.MRAG_EINVAL
    for field in ("A8", "W8", "a_exp", "w_exp", "C"):
        assert call(_args(**{field: None})) == _lib.MRAG_EINVAL, field            # null pointer
    assert call(_args(A8=0x100008)) == _lib.MRAG_EINVAL                          # misaligned operand rows
    assert call(_args(lda=264)) == _lib.MRAG_EINVAL
    assert call(_args(C=0x500008)) == _lib.MRAG_EINVAL
    assert call(_args(epilogue=EPI_RESID)) == _lib.MRAG_EINVAL                   # residual epilogue without a residual
    assert call(_args(epilogue=EPI_GATE_RESID, resid=0x600000, ldr=256)) == _lib.MRAG_EINVAL   # ... without gates
    assert call(_args(K=192, lda=192, ldw=192)) == _lib.MRAG_ENOTSUP             # not whole 128-deep K-tiles
    assert call(_args(N=24, ldc=24)) == _lib.MRAG_ENOTSUP                        # N % 16
    assert call(_args(epilogue=EPI_GEGLU)) == _lib.MRAG_ENOTSUP                  # an epilogue the fp8 GEMM does not have
    assert call(_args(M=0)) == _lib.MRAG_EINVAL
    q = lambda x, x8, ex, M, K, ldx, ld8: L.mrag_quant_rows_e4m3(None, x, x8, ex, M, K, ldx, ld8)
    assert q(None, 0x200000, 0x300000, 4, 64, 64, 64) == _lib.MRAG_EINVAL
    assert q(0x100000, 0x200000, 0x300000, 4, 72, 72, 80) == _lib.MRAG_ENOTSUP   # K % 16
    assert q(0x100000, 0x200000, 0x300000, 4, 64, 68, 64) == _lib.MRAG_ENOTSUP   # rows of x not 16-byte aligned
    assert q(0x100000, 0x200008, 0x300000, 4, 64, 64, 64) == _lib.MRAG_ENOTSUP
    buf = (ctypes.c_uint64 * 2)()
    L.mrag_fp8_launch_counts(buf, 2)
    assert list(buf) == list(before)                                             # none of the refused calls counted as a launch


def test_fp8_ops_refuse_cpu_tensors_and_state_their_shapes():
    from motionrag_amd import ops
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(ops.HipOnly):
        ops.quant_rows_e4m3(x)
    with pytest.raises(ops.HipOnly):
        ops.linear_fp8(x, torch.zeros(16, 128, dtype=torch.uint8), torch.zeros(16, dtype=torch.int32))
    assert ops.fp8_linear_supported(9216, 3072) and ops.fp8_linear_supported(3072, 12288) and ops.fp8_linear_supported(16, 128)
    assert not ops.fp8_linear_supported(256, 192) and not ops.fp8_linear_supported(24, 128) and not ops.fp8_linear_supported(256, 64)


def test_set_linear_precision_validates_and_defaults_to_bf16():
    from motionrag_amd import cogvideox
    m = cogvideox.CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=2, in_channels=16, out_channels=8, time_embed_dim=64, text_embed_dim=64,
                                              max_text_seq_length=10, sample_frames=3, sample_height=8, sample_width=12)
    assert m.linear_precision == "bf16" and m.linear_fp8_sites == frozenset()
    with pytest.raises(ValueError):
        cogvideox.set_linear_precision(m, "fp16")
    with pytest.raises(ValueError):
        cogvideox.set_linear_precision(m, "fp8", sites=("qkv", "proj_out"))
    assert m.linear_precision == "bf16" and m.linear_fp8_sites == frozenset()      # a refused call changes nothing
    assert cogvideox.set_linear_precision(m, "fp8") is m
    assert m.linear_precision == "fp8" and m.linear_fp8_sites == frozenset(cogvideox.LINEAR_SITES)
    cogvideox.set_linear_precision(m, "fp8", sites=("ff1",))
    assert m.linear_fp8_sites == frozenset({"ff1"})
    cogvideox.set_linear_precision(m, "bf16")
    assert m.linear_precision == "bf16" and m.linear_fp8_sites == frozenset()
    other = cogvideox.CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=2, in_channels=16, out_channels=8, time_embed_dim=64,
                                                  text_embed_dim=64, max_text_seq_length=10, sample_frames=3, sample_height=8, sample_width=12)
    cogvideox.set_linear_precision(m, "fp8")
    assert other.linear_precision == "bf16"                                       # per model, not per class
