"""The opt-in MXFP6 (e2m3, block-scaled) linear path without a GPU: its entry points are declared, exported and bound; the size queries are exact
for the packed layout; the argument checks of mrag_gemm_mxfp6 / mrag_quant_rows_mxfp6 / mrag_dequant_rows_mxfp6 return before any launch (so they
can be called here with made-up addresses); the torch front end refuses CPU tensors; cogvideox.set_linear_precision takes "mxfp6"."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mrag_quant_rows_mxfp6", "mrag_dequant_rows_mxfp6", "mrag_gemm_mxfp6", "mrag_mxfp6_packed_bytes", "mrag_mxfp6_scale_bytes", "mrag_mxfp6_launch_counts")
EPI_NONE, EPI_GELU_TANH, EPI_GELU_ERF, EPI_RESID, EPI_GATE_RESID, EPI_GEGLU = 0, 1, 2, 3, 4, 6


def _counts(L):
    buf = (ctypes.c_uint64 * 3)()
    assert L.mrag_mxfp6_launch_counts(buf, 3) == 3
    return list(buf)


def test_mxfp6_symbols_declared_exported_and_bound():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "gemm_mxfp6.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 11 and _lib.lib().mrag_abi_version() == 11
    # the GEMM travels on the fp8 GEMM's argument block plus two flat pointers: no new struct
    restype, argtypes = _lib.PROTOTYPES["mrag_gemm_mxfp6"]
    assert restype is ctypes.c_int32 and argtypes == [ctypes.c_void_p, ctypes.POINTER(_lib.GemmFp8Args), ctypes.c_void_p, ctypes.c_void_p]
    # the counters answer without a device: three slots; a short buffer gets only what it holds
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 3)(1 << 63, 1 << 63, 1 << 63)
    assert L.mrag_mxfp6_launch_counts(buf, 3) == 3 and max(buf) < (1 << 63)
    one = (ctypes.c_uint64 * 3)(0, 1 << 63, 1 << 63)
    assert L.mrag_mxfp6_launch_counts(one, 1) == 3 and one[0] == buf[0] and one[1] == 1 << 63 and one[2] == 1 << 63
    assert L.mrag_mxfp6_launch_counts(None, 0) == 3


def test_mxfp6_size_queries_are_exact_and_monotone():
    """the packed layout is tiles of 32 rows x 64 k of 1536 bytes (64 lanes x 24 bytes: 32 elements of 6 bits each), rows padded to 32; one scale
    byte per row and block of 32"""
    from motionrag_amd import _lib
    L = _lib.lib()
    for M, K in ((1, 64), (1, 128), (32, 128), (33, 128), (37, 256), (300, 3072), (35552, 12288)):
        assert L.mrag_mxfp6_packed_bytes(M, K) == (M + 31) // 32 * (K // 64) * 1536, (M, K)
        assert L.mrag_mxfp6_packed_bytes(M, K) == (M + 31) // 32 * 32 * K * 6 // 8                # 6 bits per element of the padded rows
        assert L.mrag_mxfp6_scale_bytes(M, K) == M * (K // 32), (M, K)
    prev = (0, 0)
    for M in range(1, 100):                                                                       # monotone in M at fixed K, and in K at fixed M
        cur = (L.mrag_mxfp6_packed_bytes(M, 256), L.mrag_mxfp6_scale_bytes(M, 256))
        assert cur[0] >= prev[0] and cur[1] > prev[1]
        prev = cur
    prev = (0, 0)
    for K in range(64, 64 * 40, 64):
        cur = (L.mrag_mxfp6_packed_bytes(37, K), L.mrag_mxfp6_scale_bytes(37, K))
        assert cur[0] > prev[0] and cur[1] > prev[1]
        prev = cur
    for M, K in ((0, 128), (-1, 128), (4, 0), (4, 96), (4, 32)):                                  # no such operand
        assert L.mrag_mxfp6_packed_bytes(M, K) == 0 and L.mrag_mxfp6_scale_bytes(M, K) == 0, (M, K)


def _args(M=64, N=256, K=256, epilogue=EPI_NONE, **over):
    """a well-formed argument block over made-up (aligned, never dereferenced) device addresses"""
    from motionrag_amd import _lib
    a = _lib.GemmFp8Args()
    a.A8, a.W8, a.C = 0x100000, 0x200000, 0x500000
    a.M, a.N, a.K, a.ldc = M, N, K, N
    a.epilogue = epilogue
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_gemm_mxfp6_argument_checks_return_before_any_launch():
    from motionrag_amd import _lib
    L = _lib.lib()
    SA, SW = 0x300000, 0x400000
    call = lambda a, sa=SA, sw=SW: L.mrag_gemm_mxfp6(None, ctypes.byref(a), sa, sw)
    before = _counts(L)
    assert L.mrag_gemm_mxfp6(None, None, SA, SW) == _lib.MRAG_EINVAL
    for field in ("A8", "W8", "C"):
        assert call(_args(**{field: None})) == _lib.MRAG_EINVAL, field            # null pointer
    assert call(_args(), sa=None) == _lib.MRAG_EINVAL and call(_args(), sw=None) == _lib.MRAG_EINVAL
    assert call(_args(A8=0x100008)) == _lib.MRAG_EINVAL                          # misaligned packed operand
    assert call(_args(W8=0x200004)) == _lib.MRAG_EINVAL
    assert call(_args(), sa=0x300002) == _lib.MRAG_EINVAL                        # scale rows are read as aligned words
    assert call(_args(C=0x500008)) == _lib.MRAG_EINVAL
    assert call(_args(ldc=128)) == _lib.MRAG_EINVAL
    assert call(_args(bias=0x700004)) == _lib.MRAG_EINVAL
    assert call(_args(epilogue=EPI_RESID)) == _lib.MRAG_EINVAL                   # residual epilogue without a residual
    assert call(_args(epilogue=EPI_GATE_RESID, resid=0x600000, ldr=256)) == _lib.MRAG_EINVAL   # ... without gates
    assert call(_args(K=192)) == _lib.MRAG_ENOTSUP                               # not whole 128-deep K-tiles
    assert call(_args(K=64)) == _lib.MRAG_ENOTSUP
    assert call(_args(N=8, ldc=8)) == _lib.MRAG_ENOTSUP                          # N % 16
    assert call(_args(N=24, ldc=24)) == _lib.MRAG_ENOTSUP
    for epi in (EPI_GEGLU, EPI_GELU_ERF, 77):
        assert call(_args(epilogue=epi)) == _lib.MRAG_ENOTSUP, epi               # epilogues the MXFP6 GEMM does not have, an unknown one
    assert call(_args(M=0)) == _lib.MRAG_EINVAL
    q = lambda x, xq, sc, M, K, ldx: L.mrag_quant_rows_mxfp6(None, x, xq, sc, M, K, ldx)
    d = lambda xq, sc, y, M, K, ldy: L.mrag_dequant_rows_mxfp6(None, xq, sc, y, M, K, ldy)
    for f in (q, d):
        assert f(None, 0x200000, 0x300000, 4, 64, 64) == _lib.MRAG_EINVAL
        assert f(0x100000, None, 0x300000, 4, 64, 64) == _lib.MRAG_EINVAL
        assert f(0x100000, 0x200000, None, 4, 64, 64) == _lib.MRAG_EINVAL
        assert f(0x100000, 0x200000, 0x300000, 0, 64, 64) == _lib.MRAG_EINVAL
        assert f(0x100000, 0x200000, 0x300000, 4, 96, 96) == _lib.MRAG_ENOTSUP    # K % 64
        assert f(0x100000, 0x200000, 0x300000, 4, 64, 68) == _lib.MRAG_ENOTSUP    # bf16 rows not 16-byte aligned
        assert f(0x100000, 0x200000, 0x300000, 4, 128, 64) == _lib.MRAG_ENOTSUP   # row stride below K
    assert q(0x100000, 0x200008, 0x300000, 4, 64, 64) == _lib.MRAG_ENOTSUP        # misaligned packed operand
    assert d(0x100008, 0x200000, 0x300000, 4, 64, 64) == _lib.MRAG_ENOTSUP
    assert _counts(L) == before                                                   # none of the refused calls counted as a launch


def test_mxfp6_ops_refuse_cpu_tensors_and_state_their_shapes():
    from motionrag_amd import ops
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(ops.HipOnly):
        ops.quant_rows_mxfp6(x)
    with pytest.raises(ops.HipOnly):
        ops.dequant_rows_mxfp6(torch.zeros(1536 * 2, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ops.HipOnly):
        ops.linear_mxfp6(x, torch.zeros(1536 * 2, dtype=torch.uint8), torch.zeros(16, 4, dtype=torch.uint8))
    assert ops.mxfp6_linear_supported(9216, 3072) and ops.mxfp6_linear_supported(3072, 12288) and ops.mxfp6_linear_supported(16, 128)
    assert not ops.mxfp6_linear_supported(256, 192) and not ops.mxfp6_linear_supported(8, 128) and not ops.mxfp6_linear_supported(256, 64)
    assert ops.mxfp6_launch_counts().keys() == {"gemm", "quant", "dequant"}


def test_set_linear_precision_takes_mxfp6():
    from motionrag_amd import cogvideox
    m = cogvideox.CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=2, in_channels=16, out_channels=8, time_embed_dim=64, text_embed_dim=64,
                                              max_text_seq_length=10, sample_frames=3, sample_height=8, sample_width=12)
    assert m.linear_precision == "bf16" and m.linear_mxfp6_sites == frozenset() and m.linear_fp8_sites == frozenset()
    with pytest.raises(ValueError):
        cogvideox.set_linear_precision(m, "fp16")
    with pytest.raises(ValueError):
        cogvideox.set_linear_precision(m, "mxfp6", sites=("qkv", "proj_out"))
    assert m.linear_precision == "bf16" and m.linear_mxfp6_sites == frozenset()     # a refused call changes nothing
    assert cogvideox.set_linear_precision(m, "mxfp6") is m
    assert m.linear_precision == "mxfp6" and m.linear_mxfp6_sites == frozenset(cogvideox.LINEAR_SITES)
    assert m.linear_fp8_sites == frozenset()                                        # keeps its meaning: empty unless the precision is "fp8"
    cogvideox.set_linear_precision(m, "mxfp6", sites=("ff1",))
    assert m.linear_mxfp6_sites == frozenset({"ff1"})
    cogvideox.set_linear_precision(m, "fp8")
    assert m.linear_fp8_sites == frozenset(cogvideox.LINEAR_SITES) and m.linear_mxfp6_sites == frozenset()
    cogvideox.set_linear_precision(m, "mxfp6")
    cogvideox.set_linear_precision(m, "bf16")
    assert m.linear_precision == "bf16" and m.linear_mxfp6_sites == frozenset() and m.linear_fp8_sites == frozenset()
    other = cogvideox.CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=2, in_channels=16, out_channels=8, time_embed_dim=64,
                                                  text_embed_dim=64, max_text_seq_length=10, sample_frames=3, sample_height=8, sample_width=12)
    cogvideox.set_linear_precision(m, "mxfp6")
    assert other.linear_precision == "bf16" and other.linear_mxfp6_sites == frozenset()   # per model, not per class
