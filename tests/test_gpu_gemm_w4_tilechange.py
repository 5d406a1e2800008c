"""The persistent four-wave GEMM (csrc/gemm_w4.hip) at a tile change.  A workgroup's K-tile stream walks from one tile into its next; the next tile's first
fragments are read from LDS again behind the epilogue (not carried in registers across it), so a wrong stage, a missing wait or an epilogue that tramples
them shows up as wrong values in a workgroup's SECOND tile only.  One problem per epilogue in which sixteen workgroups run two tiles and the last row of
tiles is ragged -- M = 33 * 256 + 40 rows, N = 2048: 34 x 8 = 272 tiles on 256 CUs -- at K = 128 (the stream changes tile with the DMA ring exactly two
K-tiles deep) and K = 192 (an odd K-tile count: the stage parity at the tile change flips from tile to tile).  Every result must be BIT-equal to the same
call on another kernel family (the 8-wave tiles: same K order, same rounding points)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
M, N = 33 * 256 + 40, 2048
FOUR = 3 << 4            # the tuning word's developer knob: the four-wave kernel whatever the dispatch rule says about K


def bf(x):
    return x.to(torch.bfloat16)


def both(ops, call, kernel):
    """call() on the 8-wave family and on the persistent four-wave kernel (checked: it is what ran)"""
    outs = {}
    try:
        ops.TUNING["gemm"] = ops.GEMM_TUNE_NO_W4
        with ops.dispatched() as d8:
            outs["eight"] = call()
        ops.TUNING["gemm"] = FOUR
        with ops.dispatched() as d4:
            outs["four"] = call()
    finally:
        ops.TUNING["gemm"] = 0
    assert d4.counts == {kernel: 1}, d4.counts
    assert not any(k.startswith("GEMM_W4") for k in d8.counts), d8.counts
    return outs["four"], outs["eight"]


def same(four, eight, what):
    if not torch.equal(four, eight):
        bad = (four != eight).any(dim=-1).reshape(-1).nonzero().flatten()
        raise AssertionError(f"{what}: {bad.numel()} rows differ, first {bad[:4].tolist()}, last {bad[-4:].tolist()}; "
                             f"max |diff| {(four.float() - eight.float()).abs().max().item():.4g}")


@pytest.fixture(scope="module", params=[128, 192])
def problem(request, hip):
    K = request.param
    g = torch.Generator().manual_seed(K)
    x = bf(torch.randn(M, K, generator=g)).to(DEV)
    w = bf(torch.randn(N, K, generator=g) * K ** -0.5).to(DEV)
    b = bf(torch.randn(N, generator=g)).to(DEV)
    r = bf(torch.randn(M, N, generator=g)).to(DEV)
    return K, x, w, b, r, g


@pytest.mark.parametrize("epi", ["none", "gelu_tanh", "resid", "gate_resid"])
def test_second_tile_of_a_workgroup(problem, epi):
    from motionrag_amd import ops
    K, x, w, b, r, g = problem
    if epi == "none":
        kw = dict()
    elif epi == "gelu_tanh":
        kw = dict(epilogue=ops.EPI_GELU_TANH)
    elif epi == "resid":
        kw = dict(epilogue=ops.EPI_RESID, resid=r)
    else:
        # two samples of 4244 = 16 * 256 + 148 rows: the sample boundary and the text / video split (row 226 of a sample: inside the second wave tile of a
        # tile row) both fall inside a wave tile's 128 rows -- those wave tiles take the general path, the others the staged one
        gates = bf(torch.randn(2, 2, N, generator=torch.Generator().manual_seed(K + 1))).to(DEV)
        kw = dict(epilogue=ops.EPI_GATE_RESID, resid=r, gate0=gates[:, 0], gate1=gates[:, 1], rows_per_batch=M // 2, split=226, gate_stride=gates.stride(0))
    four, eight = both(ops, lambda: ops.linear(x, w, b, **kw), "GEMM_W4")
    same(four, eight, f"{epi}, K = {K}")
    # the reference side is not a copy of the same mistake: the plain product against fp32 (bf16 output: 2^-8 relative per value, fp32 sums of K <= 192 terms)
    if epi == "none":
        want = x.float() @ w.float().t() + b.float()
        assert ((four.float() - want).abs() <= 2.0 ** -7 * want.abs() + 2.0 ** -7).all()


@pytest.mark.parametrize("tanh", [False, True])
def test_second_tile_geglu(problem, tanh):
    from motionrag_amd import ops
    K, x, w, b, r, g = problem
    wi, bi = ops.geglu_interleave(w, b)
    four, eight = both(ops, lambda: ops.linear(x, wi, bi, epilogue=ops.EPI_GEGLU, geglu_tanh=tanh), "GEMM_W4_GEGLU")
    assert four.shape == (M, N // 2)
    same(four, eight, f"geglu tanh={tanh}, K = {K}")


def test_second_tile_per_sample_weights(problem):
    """two samples, each with its own weight matrix: the row-tile grid restarts at the second sample (17 row tiles each, the 17th ragged)"""
    from motionrag_amd import ops
    K, x, w, b, r, g = problem
    w2 = torch.stack([w, bf(torch.randn(N, K, generator=torch.Generator().manual_seed(K + 2)) * K ** -0.5).to(DEV)])
    four, eight = None, None
    try:
        ops.TUNING["gemm"] = FOUR
        with ops.dispatched() as d4:
            four = ops.linear_per_sample(x.view(2, M // 2, K), w2)
        ops.TUNING["gemm"] = ops.GEMM_TUNE_NO_W4                       # a launch per sample on the 8-wave family
        with ops.dispatched() as d8:
            eight = ops.linear_per_sample(x.view(2, M // 2, K), w2)
    finally:
        ops.TUNING["gemm"] = 0
    assert d4.counts == {"GEMM_W4_BATCHED_W": 1}, d4.counts
    assert not any(k.startswith("GEMM_W4") for k in d8.counts), d8.counts
    same(four, eight, f"per-sample weights, K = {K}")


@pytest.mark.parametrize("S", [M // 2, 5548])
def test_second_tile_qknorm_rope(problem, S):
    """the fused QKV projection, N = 3 * 512 (8 heads), two samples with the sample boundary and the text / video boundary inside wave tiles.  S = 4244: the
    rows of the other cases (34 x 6 = 204 tiles: one per workgroup); S = 5548: M = 43 * 256 + 88, 44 x 6 = 264 tiles -- eight workgroups run a second tile"""
    from motionrag_amd import ops
    K = problem[0]
    H, text = 8, 226
    g = torch.Generator().manual_seed(S + K)
    x = bf(torch.randn(2, S, K, generator=g)).to(DEV)
    w = bf(torch.randn(3 * H * 64, K, generator=g) * K ** -0.5).to(DEV)
    b = bf(torch.randn(3 * H * 64, generator=g)).to(DEV)
    qg, qb, kg, kb = (bf(torch.randn(64, generator=g)).to(DEV) for _ in range(4))
    ang = torch.rand(S - text, 64, generator=g) * 6.28
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
    four, eight = both(ops, lambda: ops.qkv_linear_qknorm_rope(x, w, b, H, qg, qb, kg, kb, cos, sin, text, q_premul=0.18), "GEMM_W4_QKNORM_ROPE")
    same(four, eight, f"qknorm + rope, S = {S}, K = {K}")
