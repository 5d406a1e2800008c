"""Packed variable-length attention and the packed text embedder without a GPU: the two entry points are declared, exported and bound; the launch counter answers
without a device; mrag_attn_varlen_fwd_bf16 refuses each malformed argument block before any launch (made-up, never dereferenced addresses and a null stream, as
test_attn_args_cpu.py does for the fixed-length entry points) and a refused call does not count; the host packing function against a literal loop; which
attention masks the padded forward takes; how SentenceEmbedder(packed=True) cuts its passes."""
import ctypes
import os
import random
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q0, O0, CU0 = 0x1000000, 0x4000000, 0x8000000


def _args(H=2, B=5, T=300, max_seqlen=100, **over):
    """a well-formed block: q / k / v as views of one fused [T, 3 * H * 64] buffer, o [T, H * 64]"""
    from motionrag_amd import _lib
    a = _lib.AttnVarlenArgs()
    a.Q, a.K, a.V, a.O, a.cu_seqlens = Q0, Q0 + 2 * H * 64, Q0 + 4 * H * 64, O0, CU0
    a.q_ss = a.k_ss = a.v_ss = 3 * H * 64
    a.q_sh = a.k_sh = a.v_sh = 64
    a.o_ss = H * 64
    a.B, a.H, a.total_rows, a.max_seqlen, a.scale = B, H, T, max_seqlen, 0.125
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _count(L):
    buf = (ctypes.c_uint64 * 1)()
    L.mrag_attn_varlen_launch_counts(buf, 1)
    return int(buf[0])


def test_symbols_declared_exported_and_bound():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name in ("mrag_attn_varlen_fwd_bf16", "mrag_attn_varlen_launch_counts"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "attn_varlen.hip" in _lib.SOURCES and _lib.EXTRA_FLAGS["attn_varlen.hip"] == ["-fno-slp-vectorize"]
    assert L.mrag_attn_varlen_fwd_bf16.argtypes == [ctypes.c_void_p, ctypes.POINTER(_lib.AttnVarlenArgs)]
    # the ctypes struct is the header's, field for field
    body = re.search(r"typedef struct mrag_attn_varlen_args \{(.*?)\} mrag_attn_varlen_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl.strip()).split(",")]
    assert names == [f[0] for f in _lib.AttnVarlenArgs._fields_]
    assert "tools/build_rag_database.py:16-33" in hdr and "src/data/rag.py:13-15" in hdr        # the reference call sites beside the declaration


def test_counter_answers_without_a_device():
    from motionrag_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 2)(1 << 63, 1 << 63)
    assert L.mrag_attn_varlen_launch_counts(buf, 2) == 1 and buf[0] < (1 << 63) and buf[1] == 1 << 63     # one slot, at most n written
    assert L.mrag_attn_varlen_launch_counts(None, 0) == 1
    keep = (ctypes.c_uint64 * 1)(1 << 63)
    assert L.mrag_attn_varlen_launch_counts(keep, 0) == 1 and keep[0] == 1 << 63
    n = L.mrag_dispatch_counts(None, 0)
    assert all(b"VARLEN" not in L.mrag_dispatch_name(i).upper() for i in range(n))                          # enum mrag_kernel_id keeps its enumerators


def test_refusals_return_before_any_launch():
    from motionrag_amd import _lib
    EINVAL, ENOTSUP = _lib.MRAG_EINVAL, _lib.MRAG_ENOTSUP
    L = _lib.lib()
    n = L.mrag_dispatch_counts(None, 0)
    table0 = (ctypes.c_uint64 * n)()
    L.mrag_dispatch_counts(table0, n)
    before = _count(L)
    assert L.mrag_attn_varlen_fwd_bf16(None, None) == EINVAL
    cases = ([(f"{f} null", {f: None}, EINVAL) for f in ("Q", "K", "V", "O", "cu_seqlens")] +
             [(f"{f} = {bad}", {f: bad}, EINVAL) for f in ("B", "H", "max_seqlen") for bad in (0, -3)] +
             [("max_seqlen > total_rows", dict(max_seqlen=301), EINVAL),
              ("total_rows = 0", dict(T=0), EINVAL),
              ("Q misaligned by 8", dict(Q=Q0 + 8), EINVAL), ("K misaligned by 8", dict(K=Q0 + 8), EINVAL), ("V misaligned by 8", dict(V=Q0 + 8), EINVAL),
              ("O misaligned by 4", dict(O=O0 + 4), EINVAL), ("cu_seqlens misaligned by 2", dict(cu_seqlens=CU0 + 2), EINVAL),
              ("q_ss % 8", dict(q_ss=388), EINVAL), ("q_sh % 8", dict(q_sh=68), EINVAL), ("k_ss % 8", dict(k_ss=388), EINVAL), ("k_sh % 8", dict(k_sh=68), EINVAL),
              ("v_ss % 8", dict(v_ss=388), EINVAL), ("v_sh % 8", dict(v_sh=68), EINVAL), ("o_ss % 4", dict(o_ss=130), EINVAL),
              ("k_ss < 0", dict(k_ss=-8), ENOTSUP), ("v_ss < 0", dict(v_ss=-8), ENOTSUP),                   # the 32-bit K / V tile offsets of the LDS-DMA path
              ("k_ss too large", dict(k_ss=0x2000000), ENOTSUP), ("v_ss too large", dict(v_ss=0x2000000), ENOTSUP),
              ("grid z", dict(B=65536), ENOTSUP), ("grid y", dict(H=65536), ENOTSUP),
              # precedence: MRAG_EINVAL is decided first
              ("k_ss too large + misaligned Q", dict(k_ss=0x2000000, Q=Q0 + 8), EINVAL)])
    for what, over, code in cases:
        assert L.mrag_attn_varlen_fwd_bf16(None, ctypes.byref(_args(**over))) == code, what
    assert _count(L) == before                                                                              # refused calls do not count
    table1 = (ctypes.c_uint64 * n)()
    L.mrag_dispatch_counts(table1, n)
    assert list(table1) == list(table0)


def test_ops_front_end_refuses_host_tensors():
    from motionrag_amd import ops
    q = torch.zeros(8, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(ops.HipOnly):
        ops.attention_varlen(q, q, q, torch.tensor([0, 8], dtype=torch.int32), 8)


# ---------------------------------------------------------------------------------------------- host packing
@pytest.mark.parametrize("lengths,S", [([3, 1, 7, 2], None), ([3, 1, 7, 2], 9), ([5, 0, 2], None), ([1], None), ([4, 4, 4], 4)])
def test_pack_lengths_is_the_literal_loop(lengths, S):
    from motionrag_amd.text_embedder import pack_lengths
    cu, positions, index = pack_lengths(torch.tensor(lengths), S)
    width = max(lengths) if S is None else S
    want_cu, want_pos, want_idx = [0], [], []
    for i, n in enumerate(lengths):
        want_cu.append(want_cu[-1] + n)
        for j in range(n):
            want_pos.append(j)
            want_idx.append(i * width + j)
    assert cu.dtype == torch.int32 and cu.tolist() == want_cu
    assert positions.dtype == torch.int64 and positions.tolist() == want_pos
    assert index.dtype == torch.int64 and index.tolist() == want_idx
    assert all(t.device.type == "cpu" for t in (cu, positions, index))
    # gather out of a padded batch, scatter back: the valid cells and nothing else
    padded = torch.arange(len(lengths) * width).view(len(lengths), width) + 1000
    back = torch.zeros(len(lengths) * width, dtype=torch.long)
    back[index] = padded.reshape(-1)[index]
    valid = torch.arange(width)[None, :] < torch.tensor(lengths)[:, None]
    assert torch.equal(back.view(len(lengths), width), padded * valid)


def test_pack_lengths_refuses_nonsense():
    from motionrag_amd.text_embedder import pack_lengths
    with pytest.raises(ValueError):
        pack_lengths(torch.tensor([3, -1]))
    with pytest.raises(ValueError):
        pack_lengths(torch.tensor([3, 5]), 4)


def test_mask_validation_takes_right_padding_only():
    from motionrag_amd.text_embedder import mask_lengths
    ok = torch.tensor([[1, 1, 1, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]])
    assert mask_lengths(ok).tolist() == [3, 1, 5, 0]
    assert mask_lengths(ok.bool()).tolist() == [3, 1, 5, 0]
    for bad in ([[1, 0, 1, 0, 0]], [[0, 0, 1, 1, 1]], [[1, 1, 1, 1, 1], [0, 1, 1, 1, 1]], [[1, 1, 0, 0, 1]]):
        with pytest.raises(NotImplementedError, match="hole|left padding"):
            mask_lengths(torch.tensor(bad))


# ---------------------------------------------------------------------------------------------- pass cutting
def test_plan_passes_respects_the_budget_and_keeps_every_text():
    from motionrag_amd.text_embedder import plan_passes
    rng = random.Random(0)
    lengths = [rng.randint(1, 60) for _ in range(200)] + [500, 70, 300]
    order = sorted(range(len(lengths)), key=lambda i: lengths[i])
    passes = plan_passes(lengths, order, 256)
    assert sorted(i for p in passes for i in p) == list(range(len(lengths)))                                # every text exactly once
    assert [i for p in passes for i in p] == order                                                          # in the order given
    for p in passes:
        assert p and (sum(lengths[i] for i in p) <= 256 or len(p) == 1)                                     # the budget, or one over-long text alone
    assert [p for p in passes if sum(lengths[i] for i in p) > 256] == [[order[-2]], [order[-1]]]            # 300 and 500 tokens
    for a, b in zip(passes, passes[1:]):                                                                    # greedy: the next text did not fit
        assert sum(lengths[i] for i in a) + lengths[b[0]] > 256
    assert plan_passes([3, 4], [0, 1], 7) == [[0, 1]] and plan_passes([3, 4], [0, 1], 6) == [[0], [1]]
    assert plan_passes([], [], 8) == []
    with pytest.raises(ValueError):
        plan_passes([1], [0], 0)


def test_packed_encode_cuts_sorted_passes_without_a_device():
    """SentenceEmbedder(packed=True).encode on a stand-in model (CPU tensors, forward_packed returns one recognisable row per token): passes are sorted by length,
    within the budget, and every text's row lands at its place in the caller's order"""
    from types import SimpleNamespace
    from motionrag_amd.text_embedder import SentenceEmbedder

    class Stub:
        config = SimpleNamespace(hidden_size=4)

        def __init__(self):
            self.calls = []

        def parameters(self):
            return iter([torch.zeros(1)])

        def forward_packed(self, flat, cu, max_seqlen, positions):
            lens = (cu[1:] - cu[:-1]).tolist()
            assert flat.numel() == cu[-1].item() == positions.numel() and max_seqlen == max(lens) and lens == sorted(lens)
            assert positions.tolist() == [j for n in lens for j in range(n)]
            self.calls.append(lens)
            return torch.stack([flat.float(), positions.float(), flat.float() * 0, flat.float() * 0], dim=1)

    def tok(texts):
        return [[1000 + int(t.split()[0])] + [7] * (len(t.split()) - 1) for t in texts]
    rng = random.Random(1)
    texts = [f"{i} " + "w " * rng.randint(0, 30) for i in range(50)] + ["50 " + "w " * 99]
    stub = Stub()
    E = SentenceEmbedder(stub, tok, normalize=False, packed=True, max_tokens=64).encode(texts)
    assert E[:, 0].tolist() == [1000.0 + i for i in range(51)] and E[:, 1].abs().max().item() == 0          # each text's own first row
    assert all(sum(c) <= 64 or len(c) == 1 for c in stub.calls) and stub.calls[-1] == [100]
    assert sum(len(c) for c in stub.calls) == 51
    flat = [n for c in stub.calls for n in c]
    assert flat == sorted(flat)
