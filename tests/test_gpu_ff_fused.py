"""The opt-in fused feed-forward kernel on the GPU: mrag_ff_fused_bf16 (ops.ff_fused) and layers.set_ff_fusion.

Reference: a float64 emulation on the host with the kernel's three rounding points -- the LayerNorm output, the hidden tensor value * gelu_erf(gate) and the
result are each rounded to bf16, everything between them is float64.  Error measure: e = max |got - emu| / (|emu| + mean |emu|).  The bound is not a
number: on the same inputs the three launches that the kernel replaces (ops.layernorm, ops.linear with EPI_GEGLU, ops.linear with EPI_RESID) are
measured against the same emulation, and the fused launch must stay within 1.5 x their error -- both round at the emulation's places and differ from
it by fp32 summation order (the three launches also round value and gate, and the projection in front of the residual, which the emulation and the fused
kernel do not).  T = ops.FF_FUSED_ROWS rows per workgroup; the grid is ceil(rows / T), neither persistent nor capped, so there is no cap to pass.

Measured on an MI355X (inner = 1280, LayerNorm affine and both biases, e of the fused launch / e of the three launches): 1 row 0 / 5.4e-3;
127, 128, 129 rows 3.2e-3 / 6.5e-3; 259 rows 5.1e-3 / 6.2e-3; without affine and biases 3.6e-3 / 5.4e-3."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 320
EPI_RESID, EPI_GEGLU = 3, 6


def bf(t):
    return t.to(torch.bfloat16)


def _T():
    from motionrag_amd import ops
    return ops.FF_FUSED_ROWS


@functools.lru_cache(maxsize=None)
def _problem(inner, affine):
    """bf16 inputs of one problem (host) and the float64 emulation of all 2 T + 3 rows, shared read-only by the cases that use them"""
    T = _T()
    g = torch.Generator().manual_seed(100 * inner + int(affine))
    rows = 2 * T + 3
    x = bf(torch.randn(rows, C, generator=g) + 2.0 * torch.randn(rows, 1, generator=g))            # N(0, 1) plus a per-row offset
    w1 = bf(torch.randn(2 * inner, C, generator=g) * C ** -0.5)                                    # [value rows | gate rows], the nn.Linear layout
    w2 = bf(torch.randn(C, inner, generator=g) * inner ** -0.5)
    if affine:
        gamma, beta = bf(1.0 + 0.2 * torch.randn(C, generator=g)), bf(0.2 * torch.randn(C, generator=g))
        b1, b2 = bf(0.2 * torch.randn(2 * inner, generator=g)), bf(0.2 * torch.randn(C, generator=g))
    else:
        gamma = beta = b1 = b2 = None
    eps = 1e-5
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=1, keepdim=True)
    ln = (xd - mean) / torch.sqrt(var + eps)
    if affine:
        ln = ln * gamma.double() + beta.double()
    ln = bf(ln).double()                                                                           # rounding point 1
    s = ln @ w1.double().T + (b1.double() if affine else 0.0)
    value, gate = s[:, :inner], s[:, inner:]
    hidden = bf(value * 0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))).double()            # rounding point 2
    emu = bf(hidden @ w2.double().T + (b2.double() if affine else 0.0) + xd)                       # rounding point 3
    return dict(x=x, w1=w1, w2=w2, gamma=gamma, beta=beta, b1=b1, b2=b2, eps=eps, emu=emu.double())


@functools.lru_cache(maxsize=None)
def _device_problem(inner, affine):
    from motionrag_amd import ops
    p = _problem(inner, affine)
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "emu" else v) for k, v in p.items()}
    d["w1i"], d["b1i"] = ops.geglu_interleave(d["w1"], d["b1"])
    return d


def _fused(d, rows, out=None):
    from motionrag_amd import ops
    return ops.ff_fused(d["x"][:rows], d["gamma"], d["beta"], d["eps"], d["w1i"], d["b1i"], d["w2"], d["b2"], out=out)


def _three_launches(d, rows):
    from motionrag_amd import ops
    x = d["x"][:rows]
    h = ops.linear(ops.layernorm(x, d["gamma"], d["beta"], d["eps"]), d["w1i"], d["b1i"], epilogue=EPI_GEGLU)
    return ops.linear(h, d["w2"], d["b2"], epilogue=EPI_RESID, resid=x)


def _e(got, emu):
    got, emu = got.detach().double().cpu(), emu.double().cpu()
    return float(((got - emu).abs() / (emu.abs() + emu.abs().mean())).max())


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("affine", [True, False], ids=["affine_biases", "plain"])
@pytest.mark.parametrize("inner", [64, 128, 1280])
def test_ff_fused_values(hip, inner, affine):
    """rows 1, T - 1, T, T + 1, 2 T + 3 (one row; a partial, a full and a just-over-full workgroup; more than two); inner 64 / 128 / 1280 (the only chunk
    pair, two, forty); with and without the LayerNorm affine and the two biases.  e_fused <= 1.5 e_three_launches against the float64 emulation."""
    from motionrag_amd import ops
    T = _T()
    d, emu = _device_problem(inner, affine), _problem(inner, affine)["emu"]
    for rows in (1, T - 1, T, T + 1, 2 * T + 3):
        before = ops.ff_fused_launches()
        got = _fused(d, rows)
        assert ops.ff_fused_launches() == before + 1
        assert got.shape == (rows, C) and got.dtype == torch.bfloat16
        e_fused, e_three = _e(got, emu[:rows]), _e(_three_launches(d, rows), emu[:rows])
        print(f"ff_fused rows={rows} inner={inner} affine={affine}: e_fused = {e_fused:.3e}, e_three_launches = {e_three:.3e}")
        assert math.isfinite(e_fused) and e_fused <= 1.5 * e_three, (rows, e_fused, e_three)


def test_ff_fused_keeps_leading_dimensions(hip):
    d = _device_problem(128, True)
    from motionrag_amd import ops
    x3 = d["x"][:2 * 60].view(2, 60, C)
    got = ops.ff_fused(x3, d["gamma"], d["beta"], d["eps"], d["w1i"], d["b1i"], d["w2"], d["b2"])
    assert got.shape == x3.shape and torch.equal(got.view(-1, C), _fused(d, 120))


# ---------------------------------------------------------------------------------------------------------------- 2. a row's bits
@pytest.mark.parametrize("inner", [64, 1280])
def test_ff_fused_row_bits_do_not_depend_on_the_row_count(hip, inner):
    T = _T()
    d = _device_problem(inner, True)
    big, again, small = _fused(d, 2 * T + 3), _fused(d, 2 * T + 3), _fused(d, 33)
    assert torch.equal(big, again)                                      # two identical calls
    assert torch.equal(big[:33], small)                                 # rows 0 .. 32 of the large call: the 33-row call, bit for bit


# ---------------------------------------------------------------------------------------------------------------- 3. nothing else is written
@pytest.mark.parametrize("rows", [1, 131])
def test_ff_fused_writes_its_rows_and_nothing_else(hip, rows):
    d = _device_problem(128, True)
    buf = torch.full((rows + 4, 328), -7.0, dtype=torch.bfloat16, device=DEV)     # ldo = 328: eight padding columns, four sentinel rows behind
    x_before = d["x"][:rows].clone()
    out = buf[:rows, :C]
    got = _fused(d, rows, out=out)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:rows, :C], _fused(d, rows))
    assert (buf[:rows, C:] == -7.0).all() and (buf[rows:] == -7.0).all()
    assert torch.equal(d["x"][:rows], x_before)


# ---------------------------------------------------------------------------------------------------------------- 4. through the models
def _d(t):
    return t.detach().double().cpu()


def _ln64(n, x):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), _d(n.weight), _d(n.bias), n.eps)


def _ff64(ff, x):
    pj, out = ff.net[0].proj, ff.net[2]
    value, gate = (x @ _d(pj.weight).T + _d(pj.bias)).chunk(2, dim=-1)
    return (value * 0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))) @ _d(out.weight).T + _d(out.bias)


def _mha64(q, k, v, heads):
    """[N, L, heads * 64] each: softmax(q k^T / 8) v per head"""
    split = lambda t: t.unflatten(-1, (heads, 64)).transpose(1, 2)
    p = torch.softmax(split(q) @ split(k).transpose(-1, -2) * 0.125, dim=-1)
    return (p @ split(v)).transpose(1, 2).flatten(-2)


def _self_attn64(attn, h, heads):
    """to_out(attention(to_q h, to_k h, to_v h)) of either package's attention module (no q/k/v bias)"""
    return _mha64(h @ _d(attn.to_q.weight).T, h @ _d(attn.to_k.weight).T, h @ _d(attn.to_v.weight).T, heads) @ _d(attn.to_out[0].weight).T + _d(attn.to_out[0].bias)


def _dc_block64(blk, x, heads):
    """dynamicrafter.BasicTransformerBlock.forward with context None, in float64 without any rounding between the launches"""
    x = x + _self_attn64(blk.attn1, _ln64(blk.norm1, x), heads)
    x = x + _self_attn64(blk.attn2, _ln64(blk.norm2, x), heads)
    return x + _ff64(blk.ff, _ln64(blk.norm3, x))


def _svd_block64(blk, x, ctx, heads):
    """svd_unet.TemporalBasicTransformerBlock.forward for one sample (b = 1): x [f, hw, C], attention over f per pixel, in float64"""
    x = x + _ff64(blk.ff_in, _ln64(blk.norm_in, x))
    x = x + _self_attn64(blk.attn1, _ln64(blk.norm1, x).transpose(0, 1), heads).transpose(0, 1)
    a = blk.attn2                                                       # one context token: softmax == 1, the branch is to_out(to_v(context))
    x = x + (ctx.reshape(1, -1) @ _d(a.to_v.weight).T) @ _d(a.to_out[0].weight).T + _d(a.to_out[0].bias)
    return x + _ff64(blk.ff, _ln64(blk.norm3, x))


def _block(kind, dim, seed):
    """a transformer block with torch's default initialisation (seeded) and perturbed LayerNorms, in bf16 on the device; returns (block, call, number of
    feed-forwards, float64 emulation of the call on the host)"""
    from motionrag_amd import dynamicrafter, svd_unet
    torch.manual_seed(seed)
    heads = dim // 64
    if kind == "dc":
        blk = dynamicrafter.BasicTransformerBlock(dim, heads, 64)
    else:
        blk = svd_unet.TemporalBasicTransformerBlock(dim, dim, heads, 64, 64)
    with torch.no_grad():
        for name, prm in blk.named_parameters():
            if "norm" in name:
                prm.add_(0.1 * torch.randn(prm.shape))
    blk = blk.to(DEV, torch.bfloat16)
    g = torch.Generator().manual_seed(seed + 1)
    if kind == "dc":
        x = bf(torch.randn(2, 160, dim, generator=g)).to(DEV)           # 320 rows
        return blk, (lambda: blk(x)), 1, (lambda: _dc_block64(blk, _d(x), heads))
    x = bf(torch.randn(4, 80, dim, generator=g)).to(DEV)                # (b f) = 4 frames of 80 pixels: 320 rows
    ctx = bf(torch.randn(1, 1, 64, generator=g)).to(DEV)
    return blk, (lambda: blk(x, (1, 4, 80), ctx)), 2, (lambda: _svd_block64(blk, _d(x), _d(ctx), heads))


@pytest.mark.parametrize("kind", ["dc", "svd"])
def test_ff_fusion_through_the_blocks(hip, monkeypatch, kind):
    """dynamicrafter.BasicTransformerBlock / svd_unet.TemporalBasicTransformerBlock at dim 320 (5 heads x 64), 320 rows.  Switch on: one fused launch per
    feed-forward, and against a float64 emulation of the whole block (bf16 weights and input, no rounding between the launches) the error measure of the
    values test stays within 1.5 x the switch-off block's.  (The temporal block runs two feed-forwards with an attention between them: one flipped last place
    behind the first moves the second's input, so the two paths' outputs are up to two last places apart, 1.6e-2 measured; the DynamiCrafter block's
    5.6e-3.)  The emulation is checked against the switch-off block first: e <= 0.05, a dozen bf16 roundings of 2^-9 each along the block.
    Switch off, or the row gate above the row count: no fused launch, bits of a block that was never marked."""
    from motionrag_amd import layers, ops
    shipped = layers.FF_FUSED_MIN_ROWS
    monkeypatch.setattr(layers, "FF_FUSED_MIN_ROWS", 0)
    blk, call, n_ff, emulate = _block(kind, 320, 5)
    never_marked = call().clone()
    emu = emulate()
    layers.set_ff_fusion(blk)
    before, before8 = ops.ff_fused_launches(), ops.fp8_k64_launch_counts()
    on = call().clone()
    assert ops.ff_fused_launches() - before == n_ff
    assert ops.fp8_k64_launch_counts() == before8
    e_on, e_off = _e(on, emu.reshape(on.shape)), _e(never_marked, emu.reshape(on.shape))
    print(f"ff fusion through the {kind} block: e_on = {e_on:.3e}, e_off = {e_off:.3e} against float64; e(on, off) = {_e(on, never_marked):.3e}")
    assert 0.0 < e_off <= 0.05, e_off
    assert e_on <= 1.5 * e_off, (e_on, e_off)
    # the row gate above the row count: the old path, bit for bit
    monkeypatch.setattr(layers, "FF_FUSED_MIN_ROWS", 321)
    before = ops.ff_fused_launches()
    assert torch.equal(call(), never_marked) and ops.ff_fused_launches() == before
    # switched off
    monkeypatch.setattr(layers, "FF_FUSED_MIN_ROWS", 0)
    layers.set_ff_fusion(blk, False)
    assert torch.equal(call(), never_marked) and ops.ff_fused_launches() == before
    assert shipped > 0


def test_ff_fusion_leaves_wider_blocks_alone(hip, monkeypatch):
    from motionrag_amd import layers, ops
    monkeypatch.setattr(layers, "FF_FUSED_MIN_ROWS", 0)
    blk, call, _, _ = _block("dc", 640, 6)
    never_marked = call().clone()
    layers.set_ff_fusion(blk)
    before = ops.ff_fused_launches()
    assert torch.equal(call(), never_marked) and ops.ff_fused_launches() == before


def test_ff_fusion_wins_over_fp8_at_320_channels(hip, monkeypatch):
    """a module marked for both: the fused bf16 launch at C = 320, no launch on the fp8 path; without the fusion mark the same module does launch there"""
    from motionrag_amd import layers, ops
    for name in ("FF_FUSED_MIN_ROWS", "FF_FP8_MIN_ROWS", "FF2_FP8_MIN_ROWS", "FF2_FP8_MIN_WIDTH"):
        monkeypatch.setattr(layers, name, 0)
    blk, call, n_ff, _ = _block("dc", 320, 7)
    layers.set_ff_precision(blk, "fp8")
    before8 = ops.fp8_k64_launch_counts()
    call()
    assert ops.fp8_k64_launch_counts()["gemm"] > before8["gemm"]         # (the fp8 marks alone do reach the fp8 kernels at these gates)
    layers.set_ff_fusion(blk)
    before, before8 = ops.ff_fused_launches(), ops.fp8_k64_launch_counts()
    call()
    assert ops.ff_fused_launches() - before == n_ff
    assert ops.fp8_k64_launch_counts() == before8


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_ff_fused_refuses_bad_arguments(hip):
    from motionrag_amd import ops
    d = _device_problem(128, True)
    x = d["x"][:40]
    args = lambda **kw: {**dict(x=x, ln_weight=d["gamma"], ln_bias=d["beta"], eps=d["eps"], w1_interleaved=d["w1i"], b1_interleaved=d["b1i"], w2=d["w2"],
                                b2=d["b2"]), **kw}
    before = ops.ff_fused_launches()
    with pytest.raises(ValueError):
        ops.ff_fused(**args(), out=x)                                   # out is x
    with pytest.raises(ValueError):
        ops.ff_fused(**args(), out=d["x"][8:48])                        # out overlaps x
    with pytest.raises(ValueError):
        ops.ff_fused(**args(w1_interleaved=d["w1i"][:128]))             # w1 is not [2 inner, 320]
    with pytest.raises(ValueError):
        ops.ff_fused(**args(w1_interleaved=d["w1i"].T.contiguous().T))  # not contiguous
    with pytest.raises(ValueError):
        ops.ff_fused(**args(x=x.float()))                               # fp32 input
    with pytest.raises(ValueError):
        ops.ff_fused(**args(w2=d["w2"].float()))
    with pytest.raises(ValueError):
        ops.ff_fused(**args(x=torch.zeros(4, 640, dtype=torch.bfloat16, device=DEV)))
    with pytest.raises(ValueError):
        ops.ff_fused(**args(), out=torch.empty(40, 328, dtype=torch.bfloat16, device=DEV))
    assert ops.ff_fused_launches() == before
