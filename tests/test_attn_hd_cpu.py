"""The MFMA attention for head dims 32 / 80 / 96 / 128 (mrag_attn_hd_fwd_bf16) without a GPU: the two entry points are declared, exported and bound, the ABI
version and the dispatch-name table are what they were, the entry point refuses each malformed argument block before any launch (made-up, never dereferenced
addresses and a null stream, as test_attn_args_cpu.py does) and a refused call does not count; clip_vision.set_attention_kernel; the routing rule of
layers.prenorm_block with the two attention ops stubbed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q0, O0, EXTRA = 0x1000000, 0x4000000, 0x9000000


def _args(B=1, H=2, Sq=300, Skv=513, D=80, **over):
    """a well-formed block: q / k / v as views of one fused [B, S, 3, H, D] buffer, o [B, Sq, H * D]"""
    from motionrag_amd import _lib
    a = _lib.AttnArgs()
    S = max(Sq, Skv, 1)
    a.Q, a.K, a.V, a.O = Q0, Q0 + 2 * H * D, Q0 + 4 * H * D, O0
    a.q_sb = a.k_sb = a.v_sb = S * 3 * H * D
    a.q_ss = a.k_ss = a.v_ss = 3 * H * D
    a.q_sh = a.k_sh = a.v_sh = D
    a.o_sb, a.o_ss = max(Sq, 1) * H * D, H * D
    a.B, a.H, a.Sq, a.Skv, a.kv_batch_div = B, H, Sq, Skv, 1
    a.scale, a.out_scale = D ** -0.5, 1.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _count(L):
    buf = (ctypes.c_uint64 * 1)()
    L.mrag_attn_hd_launch_counts(buf, 1)
    return int(buf[0])


def _dispatch_table(L):
    n = L.mrag_dispatch_counts(None, 0)
    buf = (ctypes.c_uint64 * n)()
    L.mrag_dispatch_counts(buf, n)
    return list(buf)


def test_symbols_declared_exported_and_bound():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name in ("mrag_attn_hd_fwd_bf16", "mrag_attn_hd_launch_counts"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "attn_hd.hip" in _lib.SOURCES
    assert L.mrag_attn_hd_fwd_bf16.argtypes == [ctypes.c_void_p, ctypes.POINTER(_lib.AttnArgs), ctypes.c_int32]          # mrag_attn_small_bf16's signature
    assert L.mrag_attn_hd_fwd_bf16.argtypes == L.mrag_attn_small_bf16.argtypes and L.mrag_attn_hd_fwd_bf16.restype == ctypes.c_int32
    assert L.mrag_attn_hd_launch_counts.argtypes == L.mrag_attn_varlen_launch_counts.argtypes


def test_abi_version_and_dispatch_names_unchanged():
    from motionrag_amd import _lib
    L = _lib.lib()
    assert L.mrag_abi_version() == 11 and _lib.ABI_VERSION == 11
    n = L.mrag_dispatch_counts(None, 0)
    names = [L.mrag_dispatch_name(i).decode() for i in range(n)]
    assert names[-1] == "TOPK_RERANK" and n == _lib.CONSTANTS["MRAG_K_COUNT"]
    assert all("ATTN_HD" not in s.upper() for s in names)                                   # enum mrag_kernel_id keeps its enumerators: the counter is its own function
    attn = [s for s in names if s.startswith("ATTN")]
    assert attn == ["ATTN16", "ATTN16_KSPLIT", "ATTN_FLASH", "ATTN_FLASH_KSPLIT", "ATTN_COMBINE", "ATTN_TINY", "ATTN_SMALL", "ATTN_FP8"]


def test_counter_answers_without_a_device():
    from motionrag_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 2)(1 << 63, 1 << 63)
    assert L.mrag_attn_hd_launch_counts(buf, 2) == 1 and buf[0] < (1 << 63) and buf[1] == 1 << 63           # one slot, at most n written
    assert L.mrag_attn_hd_launch_counts(None, 0) == 1
    keep = (ctypes.c_uint64 * 1)(1 << 63)
    assert L.mrag_attn_hd_launch_counts(keep, 0) == 1 and keep[0] == 1 << 63


def test_refusals_return_before_any_launch():
    from motionrag_amd import _lib
    EINVAL, ENOTSUP = _lib.MRAG_EINVAL, _lib.MRAG_ENOTSUP
    L = _lib.lib()
    table0, before = _dispatch_table(L), _count(L)

    def call(a, head_dim=80):
        return L.mrag_attn_hd_fwd_bf16(None, ctypes.byref(a), head_dim)
    assert L.mrag_attn_hd_fwd_bf16(None, None, 80) == EINVAL
    cases = ([(f"{f} null", {f: None}, EINVAL) for f in ("Q", "K", "V", "O")] +
             [(f"{f} = {bad}", {f: bad}, EINVAL) for f in ("B", "H", "Sq", "Skv") for bad in (0, -3)] +
             [("Q misaligned by 8", dict(Q=Q0 + 8), EINVAL), ("K misaligned by 8", dict(K=Q0 + 8), EINVAL), ("V misaligned by 8", dict(V=Q0 + 8), EINVAL),
              ("O misaligned by 8", dict(O=O0 + 8), EINVAL), ("q_ss % 8", dict(q_ss=484), EINVAL), ("k_sh % 8", dict(k_sh=84), EINVAL),
              ("v_sb % 8", dict(v_sb=513 * 480 + 4), EINVAL), ("o_ss % 8", dict(o_ss=2 * 80 + 4), EINVAL),
              ("mask", dict(mask=EXTRA), ENOTSUP), ("bias", dict(bias=EXTRA, bias_sh=300 * 513), ENOTSUP), ("resid", dict(resid=EXTRA), ENOTSUP),
              ("kv_batch_div = 2", dict(kv_batch_div=2), ENOTSUP), ("q_prescaled", dict(q_prescaled=1), ENOTSUP),
              ("mask + misaligned Q", dict(mask=EXTRA, Q=Q0 + 8), ENOTSUP)])                  # precedence: as mrag_attn_small_bf16, the refusals come first
    for what, over, code in cases:
        assert call(_args(**over)) == code, what
    for D in (64, 40, 0, -80, 256):                                                          # 64 belongs to mrag_attn_fwd_bf16; the others to nobody
        assert call(_args(D=64 if D <= 0 else D), D) == ENOTSUP, D
    assert call(_args(D=40, Q=Q0 + 8), 40) == ENOTSUP                                        # the head dim is decided before the alignment
    assert call(_args(B=1 << 20, H=1 << 10, Sq=129), 80) == ENOTSUP                          # 3 * 2^30 workgroups: more than one grid dimension holds
    assert _count(L) == before                                                               # refused calls do not count
    assert _dispatch_table(L) == table0


def test_ops_front_end_refuses_host_tensors():
    from motionrag_amd import ops
    q = torch.zeros(1, 8, 2, 80, dtype=torch.bfloat16)
    with pytest.raises(ops.HipOnly):
        ops.attention_hd(q, q, q)


def test_set_attention_kernel_marks_towers_and_returns_the_module():
    from motionrag_amd import clip_vision as C
    small = dict(hidden_size=160, intermediate_size=320, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14, projection_dim=32)
    m = C.CLIPVisionModelWithProjection(**small)
    assert m.attention_kernel == "fma"                                                       # off by default
    assert C.set_attention_kernel(m, "mfma") is m and m.attention_kernel == "mfma"
    assert C.set_attention_kernel(m, "fma") is m and m.attention_kernel == "fma"
    for bad in ("MFMA", "flash", "", None, True):
        with pytest.raises(ValueError):
            C.set_attention_kernel(m, bad)
    assert m.attention_kernel == "fma"                                                       # a refused name marks nothing
    emb = C.FrozenOpenCLIPImageEmbedderV2(width=160, layers=1, heads=2, mlp_ratio=2.0, image_size=28)
    assert emb.attention_kernel == "fma" and emb.model.visual.attention_kernel == "fma"
    assert C.set_attention_kernel(emb, "mfma") is emb
    assert emb.attention_kernel == "mfma" and emb.model.visual.attention_kernel == "mfma"
    v = C.OpenCLIPVisual(width=160, layers=1, heads=2, mlp_ratio=2.0, image_size=28)
    assert C.set_attention_kernel(v, "mfma") is v and v.attention_kernel == "mfma"
    assert C.CLIPVisionModelWithProjection(**small).attention_kernel == "fma"                # the mark is the instance's, not the class's
    holder = torch.nn.ModuleList([C.CLIPVisionModelWithProjection(**small), torch.nn.Linear(2, 2)])
    assert C.set_attention_kernel(holder, "mfma") is holder and holder[0].attention_kernel == "mfma" and not hasattr(holder[1], "attention_kernel")


@pytest.mark.parametrize("S,head_dim,kernel,want", [
    (257, 80, "fma", "small"), (257, 80, "mfma", "hd"),
    (409, 80, "fma", "small"), (410, 80, "fma", "hd"),                                       # 409 * 80 = 32 720 <= 32 768 < 410 * 80
    (577, 80, "fma", "hd"), (577, 80, "mfma", "hd"),
    (256, 128, "fma", "small"), (257, 128, "fma", "hd"), (1024, 32, "fma", "small"), (1025, 32, "fma", "hd"), (341, 96, "fma", "small"), (342, 96, "fma", "hd"),
    (257, 64, "fma", "flash"), (257, 64, "mfma", "flash")])                                 # head_dim 64 is the flash kernels' whatever the mark says
def test_prenorm_block_routing(monkeypatch, S, head_dim, kernel, want):
    from motionrag_amd import layers, ops
    heads, N = 2, 1
    D = heads * head_dim
    calls = []

    def stub(name):
        def f(q, k, v, **kw):
            assert q.shape == (N, S, heads, head_dim) and k.shape == q.shape and v.shape == q.shape
            calls.append((name, kw))
            return torch.zeros(N, S, D)
        return f
    monkeypatch.setattr(ops, "attention_hd", stub("hd"))
    monkeypatch.setattr(ops, "attention_small", stub("small"))
    monkeypatch.setattr(ops, "attention", stub("flash"))
    monkeypatch.setattr(ops, "layernorm", lambda x, *a, **kw: x)
    monkeypatch.setattr(ops, "linear", lambda a, w, *rest, **kw: torch.zeros(*a.shape[:-1], w.shape[0]))
    ln, lin = torch.nn.LayerNorm(D), torch.nn.Linear(D, D)
    out = layers.prenorm_block(torch.zeros(N, S, D), heads, ln, torch.zeros(3 * D, D), None, lin, ln, lin, lin, eps=1e-5, head_dim=head_dim, attn_kernel=kernel)
    assert out.shape == (N, S, D)
    assert [c[0] for c in calls] == [want]
    if want != "flash":
        assert calls[0][1] == {}                                                             # the two ops take the same call
    if head_dim != 64:
        calls.clear()
        with pytest.raises(NotImplementedError):                                             # the masked refusal is where it was
            layers.prenorm_block(torch.zeros(N, S, D), heads, ln, torch.zeros(3 * D, D), None, lin, ln, lin, lin, eps=1e-5, head_dim=head_dim,
                                 mask=torch.zeros(S, S, dtype=torch.bool), attn_kernel=kernel)
        assert calls == []


def test_prenorm_block_default_is_the_fma_kernel(monkeypatch):
    """without the new argument a call that attention_small takes goes where it went"""
    from motionrag_amd import layers, ops
    calls = []
    monkeypatch.setattr(ops, "attention_hd", lambda *a, **kw: calls.append("hd") or torch.zeros(1, 257, 160))
    monkeypatch.setattr(ops, "attention_small", lambda *a, **kw: calls.append("small") or torch.zeros(1, 257, 160))
    monkeypatch.setattr(ops, "layernorm", lambda x, *a, **kw: x)
    monkeypatch.setattr(ops, "linear", lambda a, w, *rest, **kw: torch.zeros(*a.shape[:-1], w.shape[0]))
    ln, lin = torch.nn.LayerNorm(160), torch.nn.Linear(160, 160)
    layers.prenorm_block(torch.zeros(1, 257, 160), 2, ln, torch.zeros(480, 160), None, lin, ln, lin, lin, eps=1e-5, head_dim=80)
    assert calls == ["small"]
