"""The opt-in fp8 (e4m3) joint attention of the CogVideoX DiT without a GPU: its two entry points are declared, exported and bound, the ABI version and the
dispatch table are what they were, mrag_attn_joint_fwd_fp8's argument checks return before any launch (so they are called here with made-up addresses),
mrag_attn_fwd_fp8 keeps its refusals, and the Python front end states its shapes and validates its switch."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mrag_attn_joint_fp8_workspace_bytes", "mrag_attn_joint_fwd_fp8")
# the dispatch table as it stands: the new entry point launches attn8_kernel's family and counts under ATTN_FP8, no id is added
DISPATCH_NAMES = [
    "GEMM_W4", "GEMM_W4_QKNORM_ROPE", "GEMM_W4_GEGLU", "GEMM_256x256", "GEMM_256x320", "GEMM_256x128", "GEMM_128x128", "GEMM_STREAMK_TAIL", "GEMM_N320K320", "GEMM_192x256",
    "CONV3_W4", "CONV3_256x256", "CONV3_256x320", "CONV3_256x128", "CONV3_128x128", "CONV3_192x256",
    "CONVT_W4", "CONVT_256x256", "CONVT_256x320", "CONVT_128x128", "CONVT_192x256", "CONVT_256x128",
    "ATTN16", "ATTN16_KSPLIT", "ATTN_FLASH", "ATTN_FLASH_KSPLIT", "ATTN_COMBINE", "ATTN_TINY", "ATTN_SMALL", "ATTN_FP8", "IP_ATTN_FOLDED",
    "LAYERNORM", "LAYERNORM_ROWS", "QKNORM_ROPE", "GN_STATS", "GN_FOLD", "GN_APPLY", "GN_APPLY_MOD", "LAYERNORM_STREAM", "GN_STATS_FOLD",
    "TOPK_SCAN", "TOPK_SCAN_FUSED_MERGE", "TOPK_MERGE", "TOPK_MFMA", "GEMM_W4_TAIL_RECT", "GEMM_W4_BATCHED_W", "GEMM_SKINNY_LNA", "TOPK_DENSE", "TOPK_DENSE_FINISH", "GEMM_SKINNY",
    "TOPK_RERANK"]


def ceil128(n):
    return (n + 127) // 128 * 128


def test_joint_fp8_symbols_abi_and_dispatch_table():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "attn_fp8.hip" in _lib.SOURCES
    L = _lib.lib()
    assert _lib.ABI_VERSION == 11 and L.mrag_abi_version() == 11
    assert L.mrag_attn_joint_fp8_workspace_bytes.restype is ctypes.c_int64
    n = L.mrag_dispatch_counts(None, 0)
    assert n == len(DISPATCH_NAMES)
    assert [L.mrag_dispatch_name(i).decode() for i in range(n)] == DISPATCH_NAMES
    # struct mrag_attn_args did not change: the ctypes struct still follows the header field for field
    body = re.search(r"typedef struct mrag_attn_args \{(.*?)\} mrag_attn_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.AttnArgs._fields_] and len(names) == 30


def test_joint_workspace_is_the_old_one_at_the_padded_key_count():
    from motionrag_amd import _lib
    L = _lib.lib()
    for B, H, Sq in ((1, 3, 300), (2, 48, 17776)):
        for Skv in (512, 513, 576, 639, 17776):
            got = L.mrag_attn_joint_fp8_workspace_bytes(B, H, Sq, Skv)
            assert got == L.mrag_attn_fp8_workspace_bytes(B, H, Sq, ceil128(Skv)) and got > 0, (B, H, Sq, Skv)
    assert L.mrag_attn_joint_fp8_workspace_bytes(2, 48, 17776, 17776) > L.mrag_attn_fp8_workspace_bytes(2, 48, 17776, 17776)
    for bad in ((0, 2, 300, 513), (1, 0, 300, 513), (1, 2, 0, 513), (1, 2, 300, 0), (1, 2, 300, -5), (-1, 2, 300, 513)):
        assert L.mrag_attn_joint_fp8_workspace_bytes(*bad) == 0, bad


def _args(B=1, H=2, Sq=300, Skv=513, **over):
    """a well-formed argument block over made-up (aligned, never dereferenced) device addresses: q / k / v as views of one fused [B, S, 3, H, 64] buffer"""
    from motionrag_amd import _lib
    a = _lib.AttnArgs()
    S = max(Sq, Skv)
    a.Q, a.K, a.V, a.O, a.workspace = 0x1000000, 0x1000000 + 2 * H * 64, 0x1000000 + 4 * H * 64, 0x4000000, 0x8000000
    a.q_sb = a.k_sb = a.v_sb = S * 3 * H * 64
    a.q_ss = a.k_ss = a.v_ss = 3 * H * 64
    a.q_sh = a.k_sh = a.v_sh = 64
    a.o_sb, a.o_ss = Sq * H * 64, H * 64
    a.B, a.H, a.Sq, a.Skv, a.kv_batch_div = B, H, Sq, Skv, 1
    a.scale, a.out_scale = 0.125, 1.0
    a.workspace_bytes = _lib.lib().mrag_attn_joint_fp8_workspace_bytes(B, H, Sq, Skv)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_joint_entry_point_refusals_return_before_any_launch():
    from motionrag_amd import _lib
    L = _lib.lib()
    joint = lambda a: L.mrag_attn_joint_fwd_fp8(None, ctypes.byref(a))
    n = L.mrag_dispatch_counts(None, 0)
    before = (ctypes.c_uint64 * n)()
    L.mrag_dispatch_counts(before, n)
    assert L.mrag_attn_joint_fwd_fp8(None, None) == _lib.MRAG_EINVAL
    assert joint(_args(mask=0x9000000)) == _lib.MRAG_ENOTSUP
    assert joint(_args(bias=0x9000000, bias_sh=300 * 513)) == _lib.MRAG_ENOTSUP
    assert joint(_args(kv_batch_div=2)) == _lib.MRAG_ENOTSUP
    assert joint(_args(Skv=511)) == _lib.MRAG_ENOTSUP
    for q_prescaled in (0, 1):                                                       # a pre-scaled Q is no refusal: the same argument errors either way
        assert joint(_args(workspace=None, q_prescaled=q_prescaled)) == _lib.MRAG_EINVAL
        ok_bytes = _args().workspace_bytes
        assert joint(_args(workspace_bytes=ok_bytes - 1, q_prescaled=q_prescaled)) == _lib.MRAG_EINVAL
    # the padded layout is what is checked: the old entry point's byte count for the same (unpadded) key count is too small
    assert joint(_args(workspace_bytes=L.mrag_attn_fp8_workspace_bytes(1, 2, 300, 513))) == _lib.MRAG_EINVAL
    for field in ("Q", "K", "V", "O"):
        assert joint(_args(**{field: None})) == _lib.MRAG_EINVAL, field
    assert joint(_args(K=0x1000008)) == _lib.MRAG_EINVAL                             # alignment rules of mrag_attn_fwd_fp8
    assert joint(_args(k_ss=388)) == _lib.MRAG_EINVAL
    assert joint(_args(Sq=0)) == _lib.MRAG_EINVAL
    # the old entry point keeps its contract, refusals included
    old = lambda a: L.mrag_attn_fwd_fp8(None, ctypes.byref(a))
    assert old(_args(Skv=576)) == _lib.MRAG_ENOTSUP
    assert old(_args(Skv=640, q_prescaled=1)) == _lib.MRAG_ENOTSUP
    assert old(_args(Skv=384)) == _lib.MRAG_ENOTSUP
    assert old(_args(Skv=640, mask=0x9000000)) == _lib.MRAG_ENOTSUP
    assert old(_args(Skv=640, workspace=None)) == _lib.MRAG_EINVAL
    after = (ctypes.c_uint64 * n)()
    L.mrag_dispatch_counts(after, n)
    assert list(after) == list(before)                                               # none of the refused calls counted as a launch


def test_joint_fp8_front_end_states_its_shapes_and_refuses_cpu_tensors():
    from motionrag_amd import ops
    assert ops.fp8_joint_attention_supported(17776, 17776)
    assert ops.fp8_joint_attention_supported(2222, 17776)
    assert ops.fp8_joint_attention_supported(300, 513)
    assert not ops.fp8_joint_attention_supported(300, 511)
    assert not ops.fp8_joint_attention_supported(17776, 17776, kv_batch_div=2)
    assert not ops.fp8_joint_attention_supported(17776, 17776, mask=torch.zeros(1, dtype=torch.bool))
    # the UNets' predicate is what it was
    assert not ops.fp8_attention_supported(17776, 17776) and not ops.fp8_attention_supported(640, 640, q_prescaled=True) and ops.fp8_attention_supported(640, 640)
    x = torch.zeros(1, 513, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(ops.HipOnly):
        ops.joint_attention_fp8(x, x, x)


def test_set_attention_precision_validates_and_defaults_to_bf16():
    from motionrag_amd import cogvideox
    make = lambda: cogvideox.CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=2, in_channels=16, out_channels=8, time_embed_dim=64, text_embed_dim=64,
                                                         max_text_seq_length=10, sample_frames=3, sample_height=8, sample_width=12)
    m, other = make(), make()
    assert m.attention_precision == "bf16"
    with pytest.raises(ValueError):
        cogvideox.set_attention_precision(m, "fp16")
    assert m.attention_precision == "bf16"                                           # a refused call changes nothing
    assert cogvideox.set_attention_precision(m, "fp8") is m
    assert m.attention_precision == "fp8" and other.attention_precision == "bf16"    # per model, not per class
    assert m.linear_precision == "bf16" and m.linear_fp8_sites == frozenset()        # independent of the linears' switch ...
    cogvideox.set_linear_precision(m, "fp8")
    cogvideox.set_attention_precision(m)
    assert m.attention_precision == "bf16" and m.linear_precision == "fp8"           # ... in both directions
