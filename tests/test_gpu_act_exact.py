"""Every inlined copy of gelu_tanh_f / gelu_tanh_f2, gelu_erf_f, silu_f and geglu4 (csrc/common.h) on every finite bf16 input against fp64, site by site, and the
timestep embedding (inputs, references, the derived bound and the mutants in act_exact.py; that these checks can fail is proven on the host in
test_act_exact_cpu.py).  The bound is |got - want| <= (2^-8 + 2^-14) |want| + A(x) + 2^-126 for every finite input; nothing is excluded.

Delivery holds by construction, not by the kernel under test: the bf16 GEMMs get the patterns in A and a one-hot W (every other product is finite x 0), the
quantised GEMMs zero operands and the patterns in the bias, GroupNorm x = 0, gamma = 0 and the patterns in beta (or in the per-pixel shift), ff_fused x = 0,
W1 = 0, the (value, gate) pairs in b1 and a one-hot W2.  Every launch goes through ops.* with the dispatch / launch counter asserted (the pointwise kernels
silu_kernel, geglu_kernel and timestep_embedding_kernel have no counter: their entry points launch nothing else) into a sentinel-framed buffer that must survive.

Each check prints `EXACT <site> <fn> <worst error / bound>`; DESIGN.md section 3.10 keeps those figures."""
import functools

import pytest
import torch

import act_exact as E
import gemm_exact as X
from test_gpu_gemm_exact import Out, framed, tuned

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNARY = ("gelu_tanh", "gelu_erf", "silu")


def epi_of(fn):
    from motionrag_amd import ops
    return {"gelu_tanh": ops.EPI_GELU_TANH, "gelu_erf": ops.EPI_GELU_ERF, "silu": ops.EPI_SILU}[fn]


def check(site, fn, got, arg_bits, value=None, full=True):
    """got against the fp64 table at the arguments `arg_bits` (the patterns that were sent), every finite pattern among them"""
    if full:
        seen = torch.bincount(arg_bits.flatten(), minlength=65536) > 0
        assert seen[E.finite_bits().to(DEV)].all().item(), f"{site} {fn}: not every finite pattern reached an output"
    worst, refused, at = E.judge(got, arg_bits.expand(got.shape), fn, value)
    print(f"EXACT {site} {fn} {worst:.3f}")
    if refused:
        bits = arg_bits.expand(got.shape).flatten()[at].item()
        raise AssertionError(f"{site} {fn}: {refused} of {got.numel()} results outside the bound, worst {worst:.3g} bounds at argument {E.bits_to_bf16(torch.tensor([bits])).item()!r} "
                             f"(bits {bits:#06x}): got {got.flatten()[at].item()!r}")
    return worst


@functools.lru_cache(maxsize=None)
def unary_problem(shape):
    a_bits, w, P = E.onehot_unary(*shape)
    return framed(E.bits_to_bf16(a_bits)), framed(w), a_bits.to(DEV), P


@functools.lru_cache(maxsize=None)
def geglu_problem(shape, full=True):
    from motionrag_amd import ops
    a_bits, w, P, values = (E.onehot_geglu if full else onehot_geglu_partial)(*shape)
    wi, _ = ops.geglu_interleave(w, None)
    return framed(E.bits_to_bf16(a_bits)), framed(wi), a_bits.to(DEV), P, values.to(DEV)


def onehot_geglu_partial(M, N, K):
    """onehot_geglu for a shape too small to hold every pattern (a case that only asserts where the call lands): as many rows of patterns as there are"""
    rows = -(-E.NPAT // min(K - 2, N // 4))
    a, w, P, values = E.onehot_geglu(rows, N, K)
    return a[:M], w, P, values


def run_unary(site, shape, fn, counts, tuning=0, off=8):
    from motionrag_amd import ops
    M, N, K = shape
    a, w, a_bits, P = unary_problem(shape)
    out = Out(M, N, off)
    with tuned(tuning), ops.dispatched() as d:
        ops.linear(a, w, None, out=out.view, epilogue=epi_of(fn))
    assert d.counts == counts, (site, fn, d.counts)
    out.check(f"{site} {fn}")
    return check(site, fn, out.view, a_bits[:, torch.arange(N, device=DEV) % P])


def run_geglu(site, shape, fn, counts, tuning=0, off=8, full=True):
    from motionrag_amd import ops
    M, N, K = shape
    a, w, a_bits, P, values = geglu_problem(shape, full)
    out = Out(M, N // 2, off)
    with tuned(tuning), ops.dispatched() as d:
        ops.linear(a, w, None, out=out.view, epilogue=ops.EPI_GEGLU, geglu_tanh=fn == "gelu_tanh")
    assert d.counts == counts, (site, fn, d.counts)
    out.check(f"{site} geglu {fn}")
    return check(f"{site} geglu", fn, out.view, a_bits[:, torch.arange(N // 2, device=DEV) % P], values.view(1, -1), full)


# ---------------------------------------------------------------------------------------------- gemm_tile.h
@pytest.mark.parametrize("fn", UNARY)
def test_tile_128x128(hip, fn):
    """(1 020, 64, 64): 65 280 outputs, each finite pattern once.  The 128x128 tile has the direct epilogue only"""
    run_unary("gemm_tile 128x128 direct", E.TILE128, fn, {"GEMM_128x128": 1})


@pytest.mark.parametrize("fn", ["gelu_erf", "gelu_tanh"])
def test_tile_128x128_geglu(hip, fn):
    run_geglu("gemm_tile 128x128 direct", E.TILE128_GEGLU, fn, {"GEMM_128x128": 1})


@pytest.mark.parametrize("fn", UNARY)
def test_tile_256x256(hip, fn):
    """the LDS-staged epilogue (16-byte rows of C) and the direct one (MRAG_GEMM_TUNE_NO_STAGED)"""
    from motionrag_amd import ops
    run_unary("gemm_tile 256x256 staged", E.WAVE8, fn, {"GEMM_256x256": 1})
    run_unary("gemm_tile 256x256 direct", E.WAVE8, fn, {"GEMM_256x256": 1}, ops.GEMM_TUNE_NO_STAGED)


@pytest.mark.parametrize("fn", ["gelu_erf", "gelu_tanh"])
def test_tile_256x256_geglu(hip, fn):
    from motionrag_amd import ops
    run_geglu("gemm_tile 256x256 staged", E.WAVE8, fn, {"GEMM_256x256": 1})
    run_geglu("gemm_tile 256x256 direct", E.WAVE8, fn, {"GEMM_256x256": 1}, ops.GEMM_TUNE_GEGLU_NO_STAGED)


@pytest.mark.parametrize("fn", UNARY)
def test_tile_256x320(hip, fn):
    """(7 181, 1 600, 192) reaches the 320-wide tile as shipped: staged, and direct through a C whose rows are only 8-byte aligned.  The tile has no GEGLU form
    (TN = 5 is odd; the dispatch never sends GEGLU there)"""
    run_unary("gemm_tile 256x320 staged", E.WIDE320, fn, {"GEMM_256x320": 1})
    run_unary("gemm_tile 256x320 direct", E.WIDE320, fn, {"GEMM_256x320": 1}, off=4)


def test_stream_k_tail_gelu_tanh(hip):
    """section 3.9's shape: 256 whole tiles and a tail of 16 cut into runs of K-tiles; GELU tanh is the one activation the tail is planned for.  With a one-hot W
    all partial sums but one are zero, so the exchange cannot round"""
    from motionrag_amd import ops
    run_unary("gemm_tile stream-K tail", E.STREAMK, "gelu_tanh", {"GEMM_256x256": 1, "GEMM_STREAMK_TAIL": 1}, ops.GEMM_TUNE_STREAMK)


# ---------------------------------------------------------------------------------------------- the other bf16 GEMM kernels
def test_four_wave(hip):
    """gemm_w4: GELU tanh on the packed gelu_tanh_f2 path (from K = 1 536), GEGLU erf / tanh (from K = 320).  Not reachable, asserted where the calls land:
    GELU erf and SiLU do not exist on the four-wave kernel, and GELU tanh below K = 1 536 stays on the 8-wave tile"""
    run_unary("gemm_w4", E.W4_GELU, "gelu_tanh", {"GEMM_W4": 1})
    for fn in ("gelu_erf", "gelu_tanh"):
        run_geglu("gemm_w4", E.W4_K320, fn, {"GEMM_W4_GEGLU": 1})
    for fn in ("gelu_erf", "silu"):
        run_unary("gemm_w4 shape, on the 8-wave tile:", E.W4_GELU, fn, {"GEMM_256x256": 1})


def test_four_wave_short_k_gelu_tanh_lands_on_8_wave(hip):
    run_unary("gemm_w4 K = 320, on the 8-wave tile:", E.W4_K320, "gelu_tanh", {"GEMM_256x256": 1})


@pytest.mark.parametrize("fn", UNARY)
def test_skinny(hip, fn):
    run_unary("gemm_skinny", E.SKINNY, fn, {"GEMM_SKINNY": 1})


def test_skinny_ln_gelu_erf(hip):
    """gemm_skinny_kernel<.., LNA> (ops.linear_ln with GELU erf: CAMA's gelu(ff1(ln(latents)))): LayerNorm of x = 0 with gamma = 0 makes every A row the
    bf16 beta, an identity W brings 4 096 patterns per launch to the epilogue: 16 launches"""
    from motionrag_amd import ops
    M, K = 8, 4096
    bits = bias_patterns(16 * K).view(16, K)
    beta = E.bits_to_bf16(bits).to(DEV)
    x, gamma, w = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV), torch.zeros(K, dtype=torch.bfloat16, device=DEV), torch.eye(K, dtype=torch.bfloat16, device=DEV)
    outs = [Out(M, K) for _ in range(16)]
    for k in range(16):
        with ops.dispatched() as d:
            ops.linear_ln(x, gamma, beta[k], 1e-5, w, epilogue=ops.EPI_GELU_ERF, out=outs[k].view)
        assert d.counts == {"GEMM_SKINNY_LNA": 1}, d.counts
        outs[k].check("gemm_skinny LNA")
    check("gemm_skinny LNA", "gelu_erf", torch.stack([o.view for o in outs]), bits.to(DEV).view(16, 1, K))


def test_skinny_has_no_geglu(hip):
    """not reachable: GEGLU at the few-row shape runs the 128x128 tile (250 rows hold 48 000 of the patterns: the landing is what is asserted)"""
    run_geglu("gemm_skinny shape, on the 128x128 tile:", E.SKINNY, "gelu_erf", {"GEMM_128x128": 1}, full=False)


def test_k320_geglu_is_not_dispatched(hip):
    """gemm_k320_kernel instantiates GEGLU (its geglu4 site) but k320_applies takes EPI_NONE / EPI_RESID only: the UNets' K = 320 GEGLU projection runs the
    four-wave kernel, asserted here at N = 2 560 -- and judged there"""
    for fn in ("gelu_erf", "gelu_tanh"):
        run_geglu("gemm_k320 shape, on gemm_w4:", E.K320_GEGLU, fn, {"GEMM_W4_GEGLU": 1})


# ---------------------------------------------------------------------------------------------- the quantised GEMMs: zero operands, the patterns in the bias
def bias_patterns(n):
    bits = torch.zeros(n, dtype=torch.int64)
    bits[:E.NPAT] = E.finite_bits()
    return bits


def test_fp8_and_mxfp6_gelu_tanh(hip):
    """gemm_fp8 and gemm_mxfp6 have GELU tanh alone among the activations (ops.linear_fp8 / linear_mxfp6 refuse the others: asserted)"""
    from motionrag_amd import ops
    M, N, K = 8, E.QUANT_N, 128
    bits = bias_patterns(N)
    bias = E.bits_to_bf16(bits).to(DEV)
    x, w = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV), torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    for site, quant, entry, counter in (("gemm_fp8", ops.quant_rows_e4m3, ops.linear_fp8, ops.fp8_launch_counts),
                                        ("gemm_mxfp6", ops.quant_rows_mxfp6, ops.linear_mxfp6, ops.mxfp6_launch_counts)):
        wq, ws = quant(w)
        out = Out(M, N)
        before = counter()["gemm"]
        entry(x, wq, ws, bias, out=out.view, epilogue=ops.EPI_GELU_TANH)
        assert counter()["gemm"] == before + 1
        out.check(site)
        check(site, "gelu_tanh", out.view, bits.to(DEV).view(1, -1))
        for epi in (ops.EPI_GELU_ERF, ops.EPI_SILU, ops.EPI_GEGLU):
            with pytest.raises(ValueError):
                entry(x, wq, ws, bias, out=out.view, epilogue=epi)


def test_fp8_k64_geglu(hip):
    """gemm_fp8's K64 form: GEGLU (exact erf) in the lane, value 1 on the first half of the outputs and -3 on the second"""
    from motionrag_amd import ops
    M, K, inner = 8, 64, 2 * E.QUANT_N
    bits = torch.cat([bias_patterns(E.QUANT_N)] * 2)
    values = torch.tensor(E.GEGLU_VALUES, dtype=torch.float64).repeat_interleave(E.QUANT_N)
    b_full = torch.cat([X.bf(values), E.bits_to_bf16(bits)])
    wi, bi = ops.geglu_interleave(torch.zeros(2 * inner, K, dtype=torch.bfloat16, device=DEV), b_full.to(DEV))
    w8, w_exp = ops.quant_rows_e4m3(wi)
    out = Out(M, inner)
    before = ops.fp8_k64_launch_counts()["gemm"]
    ops.linear_fp8_k64(torch.zeros(M, K, dtype=torch.bfloat16, device=DEV), w8, w_exp, bi, epilogue=ops.EPI_GEGLU, out=out.view)
    assert ops.fp8_k64_launch_counts()["gemm"] == before + 1
    out.check("gemm_fp8 k64 geglu")
    check("gemm_fp8 k64 geglu", "gelu_erf", out.view, bits.to(DEV).view(1, -1), values.to(DEV).view(1, -1))


# ---------------------------------------------------------------------------------------------- the non-GEMM sites
def test_ff_fused(hip):
    """x = 0 and W1 = 0: the score tiles are zero and b1 carries the (value, gate) pairs; W2 is the identity on 320 hidden units, b2 none: 204 launches of one
    workgroup per value bring all 65 280 patterns to the output.  At value -3 the 213 gates from 2^126.4 up would make the hidden unit infinite, and an infinite
    hidden unit times W2's zeros is NaN in every channel of the row -- the arithmetic of any GEMM on an overflowed operand, out of scope like the non-finite
    inputs: those gates (all from 2^126 up) meet the value -1 instead, whose product is finite"""
    from motionrag_amd import ops
    C, inner, rows = 320, 320, 4
    fb = E.finite_bits()
    n = E.NPAT // inner
    assert n * inner == E.NPAT
    gates = E.bits_to_bf16(fb).view(n, inner)
    perm = ops.geglu_interleave(torch.arange(2 * inner).view(-1, 1), None)[0].flatten()
    x = torch.zeros(rows, C, dtype=torch.bfloat16, device=DEV)
    w1 = torch.zeros(2 * inner, C, dtype=torch.bfloat16, device=DEV)
    w2 = torch.eye(C, dtype=torch.bfloat16, device=DEV)
    for val in E.GEGLU_VALUES:
        values = torch.full((n, inner), val, dtype=torch.bfloat16)
        if val != 1.0:
            values[gates.float() >= 2.0 ** 126] = -1.0
        b1 = torch.cat([values, gates], dim=1)[:, perm].contiguous().to(DEV)
        buf = torch.full((n, rows + 1, C + 8), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
        before = ops.ff_fused_launches()
        for k in range(n):
            ops.ff_fused(x, None, None, 1e-5, w1, b1[k], w2, None, out=buf[k, :rows, :C])
        assert ops.ff_fused_launches() == before + n
        assert (buf[:, rows] == X.SENTINEL).all().item() and (buf[:, :, C:] == X.SENTINEL).all().item(), "ff_fused: written outside the result block"
        got = buf[:, :rows, :C].permute(1, 0, 2).reshape(rows, E.NPAT)
        assert (got.view(torch.int16) == got.view(torch.int16)[:1]).all().item(), "ff_fused: the rows of one launch differ"
        check(f"ff_fused value {val}", "gelu_erf", got, fb.to(DEV).view(1, -1), values.double().to(DEV).view(1, -1))


def test_silu_kernel(hip):
    """n = 65 280 + 3: the scalar tail (n % 8) gets patterns too (1.0, -3.0 and -0.0078125 once more)"""
    from motionrag_amd import ops
    bits = torch.cat([E.finite_bits(), torch.tensor([0x3f80, 0xc040, 0xbc00])])
    got = ops.silu(E.bits_to_bf16(bits).to(DEV))
    assert got.shape == (E.NPAT + 3,)
    check("silu_kernel", "silu", got, bits.to(DEV))


def test_geglu_kernel(hip):
    """mrag_geglu_bf16 (exact erf): row 0 has the value 1, row 1 the value -3, the gates sweep every pattern"""
    from motionrag_amd import ops
    fb = E.finite_bits()
    values = torch.tensor(E.GEGLU_VALUES, dtype=torch.float64).view(2, 1)
    x = torch.cat([X.bf(values).expand(2, E.NPAT), E.bits_to_bf16(fb).view(1, -1).expand(2, E.NPAT)], dim=1).contiguous().to(DEV)
    got = ops.geglu(x)
    assert got.shape == (2, E.NPAT)
    check("geglu_kernel", "gelu_erf", got, fb.to(DEV).view(1, -1), values.to(DEV))


def test_groupnorm_silu(hip):
    """gn_apply_kernel: x = 0, gamma = 0, beta = the patterns: scale 0 and shift beta exactly (direct or folded), so SiLU's argument is beta.  C = 2 048, G = 32,
    five pixels (one whole run of 1 024 vectors and a tail of 256): 32 launches"""
    from motionrag_amd import ops
    C, HW = 2048, 5
    bits = bias_patterns(32 * C).view(32, C)
    beta = E.bits_to_bf16(bits).to(DEV)
    x, gamma = torch.zeros(1, HW, C, dtype=torch.bfloat16, device=DEV), torch.zeros(C, dtype=torch.bfloat16, device=DEV)
    buf = torch.full((32, HW + 2, C), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
    for k in range(32):
        with ops.dispatched() as d:
            ops.groupnorm(x, gamma, beta[k], 32, 1e-5, silu=True, out=buf[k, 1:HW + 1].view(1, HW, C))
        assert d.counts == {"GN_STATS": 1, "GN_FOLD": 1, "GN_APPLY": 1}, d.counts
    assert (buf[:, 0] == X.SENTINEL).all().item() and (buf[:, HW + 1] == X.SENTINEL).all().item(), "groupnorm: written outside the result block"
    check("gn_apply", "silu", buf[:, 1:HW + 1], bits.to(DEV).view(32, 1, C))


def test_groupnorm_mod_silu(hip):
    """gn_apply_mod_kernel with silu: x = 0, gamma = 0, beta = 0, scale map 1, the patterns in the per-pixel shift map: all of them in one launch of 32 pixels"""
    from motionrag_amd import ops
    C, H, W = 2048, 4, 8
    bits = bias_patterns(H * W * C).view(H * W, C)
    mod = torch.cat([torch.ones(H * W, C, dtype=torch.bfloat16), E.bits_to_bf16(bits)], dim=1).view(1, 1, H, W, 2 * C).contiguous().to(DEV)
    x, gamma = torch.zeros(1, H * W, C, dtype=torch.bfloat16, device=DEV), torch.zeros(C, dtype=torch.bfloat16, device=DEV)
    buf = torch.full((H * W + 2, C), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
    with ops.dispatched() as d:
        ops.groupnorm(x, gamma, gamma, 32, 1e-5, silu=True, mod=mod, mod_geom=(1, H, W, 0, False), out=buf[1:H * W + 1].view(1, H * W, C))
    assert d.counts == {"GN_STATS": 1, "GN_FOLD": 1, "GN_APPLY_MOD": 1}, d.counts
    assert (buf[0] == X.SENTINEL).all().item() and (buf[H * W + 1] == X.SENTINEL).all().item(), "groupnorm (mod): written outside the result block"
    check("gn_apply_mod", "silu", buf[1:H * W + 1], bits.to(DEV))


# ---------------------------------------------------------------------------------------------- family P: the GEGLU rounding points
def check_p(site, fn, got, v, g, preround):
    """got against the site's own contract, and -- so that the check means something -- NOT inside the other contract's bound everywhere"""
    own, other = E.judge_p(got, v, g, fn, preround), E.judge_p(got, v, g, fn, not preround)
    print(f"EXACT {site} family-P {fn} {own[0]:.3f} (the other contract refuses {other[1]} of {got.numel()})")
    assert own[1] == 0, f"{site} {fn}: {own[1]} of {got.numel()} results leave the contract {'bf16(value) * act(bf16(gate))' if preround else 'one rounding'}: worst {own[0]:.3g} bounds"
    assert other[1] >= got.numel() // 10, (site, fn, other)


@pytest.mark.parametrize("site,shape,counts", [("gemm_tile 128x128", E.TILE128, {"GEMM_128x128": 1}), ("gemm_tile 256x256", E.WAVE8, {"GEMM_256x256": 1}),
                                               ("gemm_w4", E.W4_K320, {"GEMM_W4_GEGLU": 1})], ids=["128x128", "256x256", "w4"])
def test_geglu_rounding_points(hip, site, shape, counts):
    """geglu4: bf16(value) * act(bf16(gate)).  Two ones in every W row: the accumulators are hi + lo, at and beside half a bf16 step"""
    from motionrag_amd import ops
    M, N, K = shape
    a, w, v, g = E.family_p_gemm(M, N, K)
    wi, _ = ops.geglu_interleave(w, None)
    ad, wd = framed(a), framed(wi)
    for fn in ("gelu_erf", "gelu_tanh"):
        out = Out(M, N // 2)
        with ops.dispatched() as d:
            ops.linear(ad, wd, None, out=out.view, epilogue=ops.EPI_GEGLU, geglu_tanh=fn == "gelu_tanh")
        assert d.counts == counts, (site, fn, d.counts)
        out.check(f"{site} family P")
        check_p(site, fn, out.view, v.to(DEV), g.to(DEV), True)


def test_geglu_rounding_points_fp8_k64(hip):
    """bias + one product: x holds e4m3 numbers (exact behind the row quantiser's power-of-two scale), W is one-hot, the bias holds lo"""
    from motionrag_amd import ops
    M, K, inner = 300, 64, 32
    hv, lv, hg, lg = E.family_p_bias(M, inner)
    j = torch.arange(inner)
    w = torch.zeros(2 * inner, K)
    w[j, j] = w[inner + j, inner + j] = 1.0
    wi, bi = ops.geglu_interleave(X.bf(w).to(DEV), X.bf(torch.cat([lv, lg])).to(DEV))
    w8, w_exp = ops.quant_rows_e4m3(wi)
    out = Out(M, inner)
    before = ops.fp8_k64_launch_counts()["gemm"]
    ops.linear_fp8_k64(X.bf(torch.cat([hv, hg], dim=1)).to(DEV), w8, w_exp, bi, epilogue=ops.EPI_GEGLU, out=out.view)
    assert ops.fp8_k64_launch_counts()["gemm"] == before + 1
    out.check("gemm_fp8 k64 family P")
    check_p("gemm_fp8 k64", "gelu_erf", out.view, (hv + lv).double().to(DEV), (hg + lg).double().to(DEV), True)


def test_geglu_rounding_points_ff_fused(hip):
    """ff_fused promises the fp32 product (value + b1) * gelu(gate + b1) rounded ONCE.  LayerNorm with gamma = 0 turns every row into beta (hi, one per channel);
    W1 is one-hot (value of unit h from channel h, gate from channel 319 - h), b1 holds lo; W2 is the identity.  16 launches with inputs of their own"""
    from motionrag_amd import ops
    C, rows, n = 320, 4, 16
    h = torch.arange(C)
    w = torch.zeros(2 * C, C)
    w[h, h] = w[C + h, C - 1 - h] = 1.0
    w1, _ = ops.geglu_interleave(X.bf(w).to(DEV), None)
    perm = ops.geglu_interleave(torch.arange(2 * C).view(-1, 1), None)[0].flatten()
    x, gamma, w2 = torch.zeros(rows, C, dtype=torch.bfloat16, device=DEV), torch.zeros(C, dtype=torch.bfloat16, device=DEV), torch.eye(C, dtype=torch.bfloat16, device=DEV)
    got, vs, gs = [], [], []
    before = ops.ff_fused_launches()
    for k in range(n):
        hi, lo_v = E.family_p((C,), seed=100 + k)
        lo_g = E.half_step_lo(hi.flip(0), X.gen(200 + k))
        out = torch.full((rows, C), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
        ops.ff_fused(x, gamma, X.bf(hi).to(DEV), 1e-5, w1, X.bf(torch.cat([lo_v, lo_g]))[perm].to(DEV), w2, None, out=out)
        assert (out.view(torch.int16) == out.view(torch.int16)[:1]).all().item()
        got.append(out[0]); vs.append((hi + lo_v).double()); gs.append((hi.flip(0) + lo_g).double())
    assert ops.ff_fused_launches() == before + n
    check_p("ff_fused", "gelu_erf", torch.stack(got), torch.stack(vs).to(DEV), torch.stack(gs).to(DEV), False)


# ---------------------------------------------------------------------------------------------- timestep embedding
@pytest.mark.parametrize("dim", E.TS_DIMS)
def test_timestep_embedding(hip, dim):
    """cos | sin (t exp(-ln 1e4 j / half)) against fp64 at t in {0, 1e-4, 0.5, 1, 20, 481, 961.37, 999, 1000}: (2^-8 + 2^-14) |want| + |arg| (|z| + 2) 2^-22
    (act_exact.timestep_ref derives it)"""
    from motionrag_amd import ops
    t = torch.tensor(E.TS_T, dtype=torch.float32, device=DEV)
    got = ops.timestep_embedding(t, dim)
    want, bound = E.timestep_ref(t, dim)
    ratio = E.ratio_of(got, want, bound.clamp(min=1e-300))
    worst = ratio.max().item()
    print(f"EXACT timestep_embedding dim={dim} cos|sin {worst:.3f}")
    if worst > 1.0:
        b, c = divmod(int(ratio.flatten().argmax().item()), dim)
        raise AssertionError(f"timestep_embedding dim {dim}: {int((ratio > 1).sum())} results outside the bound, worst {worst:.3g} bounds at t = {E.TS_T[b]}, column {c}: "
                             f"got {got[b, c].item()!r}, want {want[b, c].item()!r}")
