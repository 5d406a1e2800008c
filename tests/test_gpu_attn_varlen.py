"""Packed variable-length attention (mrag_attn_varlen_fwd_bf16, ops.attention_varlen) on the GPU: one launch over sequences on every side of the 16 / 32 / 64 /
128 boundaries -- both key-range paths (the clamped DMA below 64 keys, the slid-back last tile above), the longest sequence not last, a zero-length sequence, a
1-token sequence as the buffer's final row -- against the fp32 reference per sequence; no key of a neighbouring sequence is read; rows beyond cu_seqlens[-1]
stay untouched; agreement with the fixed-length entry; no host synchronisation (bit-equal runs, graph capture); the launch counter."""
import pytest
import torch

from test_gpu_kernels import bf, close, sdpa_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 3
LENGTHS = [17, 1, 64, 2, 129, 15, 63, 200, 16, 65, 31, 128, 33, 127, 32, 257, 0, 1]
T = sum(LENGTHS)


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


@pytest.fixture(scope="module")
def packed():
    """one fused [T, 3 * H * 64] buffer, its q / k / v views, cu_seqlens, and the per-sequence fp32 reference (computed once, never written to)"""
    gen = torch.Generator().manual_seed(11)
    qkv = bf(torch.randn(T, 3, H, 64, generator=gen)).to(DEV)
    cu = _cu(LENGTHS)
    want = torch.cat([sdpa_ref(*(qkv[s:e, i][None].cpu() for i in range(3)))[0] for s, e in zip(cu, cu[1:]) if e > s])
    return qkv, torch.tensor(cu, dtype=torch.int32, device=DEV), cu, want


def test_values_match_the_reference_per_sequence(hip, packed):
    from motionrag_amd import ops
    qkv, cu_d, cu, want = packed
    assert qkv.view(T, -1).stride() == (3 * H * 64, 1) and not qkv[:, 1].is_contiguous()        # views of one fused buffer
    got = ops.attention_varlen(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu_d, max(LENGTHS))
    assert got.shape == (T, H * 64) and got.dtype == torch.bfloat16
    close(got, want)
    for s, e in zip(cu, cu[1:]):                                                                 # and sequence by sequence, each on its own magnitude
        if e > s:
            close(got[s:e], want[s:e])


def test_no_key_of_a_neighbouring_sequence_is_read(hip, packed):
    """V of sequence i is the constant i + 1: a softmax-weighted mean of a constant is that constant, to one bf16 rounding; a single foreign key shows"""
    from motionrag_amd import ops
    qkv, cu_d, cu, _ = packed
    v = torch.empty(T, H, 64, dtype=torch.bfloat16, device=DEV)
    for i, (s, e) in enumerate(zip(cu, cu[1:])):
        v[s:e] = i + 1
    got = ops.attention_varlen(qkv[:, 0], qkv[:, 1], v, cu_d, max(LENGTHS)).float()
    assert torch.isfinite(got).all()
    for i, (s, e) in enumerate(zip(cu, cu[1:])):
        if e > s:
            err = (got[s:e] - (i + 1)).abs().max().item()
            assert err <= 2.0 ** -8 * (i + 1), (i, LENGTHS[i], err)


def test_rows_beyond_the_last_sequence_are_untouched(hip, packed):
    from motionrag_amd import ops
    qkv, cu_d, cu, want = packed
    assert cu[16] == cu[17] and cu[-1] == T                                                      # the zero-length sequence owns no row
    out = torch.full((T + 64, H * 64), -768.0, dtype=torch.bfloat16, device=DEV)
    res = ops.attention_varlen(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu_d, max(LENGTHS), out=out)
    assert res is out
    assert (out[T:] == -768.0).all()
    assert (out[:T] != -768.0).all()
    close(out[:T], want)


@pytest.mark.parametrize("B,S", [(5, 40), (3, 100)])
def test_agrees_with_the_fixed_length_entry(hip, B, S):
    """Equal lengths: the same data through ops.attention as [B, S, H, 64].  Both kernels run the tile functions of attn_flash_tile.h with 64-row workgroups at
    these lengths, but bit-equality is NOT guaranteed by the code (two kernels, two compilations of the shared body, which the compiler may schedule and
    contract differently): the assertion is the tolerance of the value tests, not equality."""
    from motionrag_amd import ops
    gen = torch.Generator().manual_seed(S)
    qkv = bf(torch.randn(B * S, 3, H, 64, generator=gen)).to(DEV)
    cu = torch.arange(0, B * S + 1, S, dtype=torch.int32, device=DEV)
    got = ops.attention_varlen(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu, S)
    q4 = qkv.view(B, S, 3, H, 64)
    fixed = ops.attention(q4[:, :, 0], q4[:, :, 1], q4[:, :, 2])
    close(got.view(B, S, H * 64), fixed)
    close(got.view(B, S, H * 64), sdpa_ref(q4[:, :, 0], q4[:, :, 1], q4[:, :, 2]))


def test_no_host_synchronisation_two_runs_bit_equal_and_graph_capture(hip, packed):
    from motionrag_amd import ops
    qkv, cu_d, _, _ = packed
    run = lambda out=None: ops.attention_varlen(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu_d, max(LENGTHS), out=out)
    eager = run()
    assert torch.equal(run(), eager)
    og = torch.zeros_like(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.HIPGraph() if hasattr(torch.cuda, "HIPGraph") else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                                # the captured region is that single kernel
        run(og)
    og.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(og, eager)


def test_one_call_is_one_counted_launch(hip, packed):
    from motionrag_amd import ops
    qkv, cu_d, _, _ = packed
    before = ops.attn_varlen_launch_counts()
    with ops.dispatched() as d:
        ops.attention_varlen(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu_d, max(LENGTHS))
    assert ops.attn_varlen_launch_counts() == before + 1
    assert d.counts == {}                                                                        # mrag_dispatch_counts: no attention counter (none at all) moved


def test_front_end_checks(hip, packed):
    from motionrag_amd import ops
    qkv, cu_d, _, _ = packed
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
    before = ops.attn_varlen_launch_counts()
    with pytest.raises(TypeError):
        ops.attention_varlen(q.float(), k, v, cu_d, 257)
    with pytest.raises(TypeError):
        ops.attention_varlen(q, k, v, cu_d.long(), 257)
    with pytest.raises(TypeError):
        ops.attention_varlen(q, k, v, cu_d, torch.tensor(257))
    with pytest.raises(ValueError):
        ops.attention_varlen(q[None], k[None], v[None], cu_d, 257)
    with pytest.raises(ValueError):
        ops.attention_varlen(q, k[:-1], v, cu_d, 257)
    with pytest.raises(ValueError):
        ops.attention_varlen(q, k, v, cu_d, T + 1)
    with pytest.raises(ValueError):
        ops.attention_varlen(q, k, v, cu_d, 257, out=torch.empty(T - 1, H * 64, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ops.HipOnly):
        ops.attention_varlen(q, k, v, cu_d.cpu(), 257)
    assert ops.attn_varlen_launch_counts() == before
