"""The opt-in fp8 (e4m3) 3x3 convolution on the GPU: mrag_conv_fp8 (ops.conv_implicit_fp8) and layers.set_conv_precision.

References, all computed on the host:
  * the emulation of the kernel's contract: x quantised per PIXEL and the [Cout, (ky, kx, cin)] weight per OUTPUT CHANNEL with the reference
    quantiser of tests/test_gpu_fp8_linear.py (pow2_fit_rows / quant_ref, imported), decoded, the scales undone (powers of two: exact in fp32),
    torch.nn.functional.conv2d in float64, plus bias, rounded to bf16, plus the residual, rounded again -- the kernel's rounding points.
    Bounds as for the fp8 GEMM (same rounding points): one bf16 rounding is at most 2^-8 relative per element and fp32 summation order is at the
    1e-6 level, so NONE <= 4e-3 relative Frobenius error; RESID rounds twice: <= 8e-3.
  * the un-quantised float64 convolution of the bf16 inputs, self-calibrated: E = the emulation's error against it, G = the kernel's,
    G <= 1.1 E + 4e-3.  E is printed, not asserted (measured: 0.0370 at Cin = Cout = 320, kernel 0.0370).
  * model level: the bf16 model is the reference; E_model = the error of the same model with layers.conv3x3 replaced by the host emulation for the
    gated convolutions, G_model = the fp8 model's; G_model <= 1.5 E_model + 0.02 (the bound of test_dit_fp8_linears_against_oracle).

mrag_conv_fp8 runs its one tile shape at every size (the tile-count threshold is layers.conv3x3's: CONV_FP8_MIN_TILES), so the shapes below are the
issue's, unchanged."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_fp8_linear import bf, dequant, quant_ref, rel_fro

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPI_NONE, EPI_RESID = 0, 3
BOUND = {EPI_NONE: 4e-3, EPI_RESID: 8e-3}


# ---------------------------------------------------------------------------------------------------------------- the host emulation
def tap_major(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, ky, kx] -> [Cout, (ky, kx, cin)]: the layout layers.conv3x3 builds"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def emulate_acc(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x [N, H, W, Cin] bf16, w [Cout, Cin, 3, 3] bf16 (host) -> the float64 convolution of the quantise-dequantised operands, [N, H, W, Cout]"""
    N, H, W, C = x.shape
    cout = w.shape[0]
    xq = dequant(*quant_ref(x.reshape(-1, C))).view(N, H, W, C)                       # one exponent per pixel
    wq = dequant(*quant_ref(tap_major(w))).view(cout, 3, 3, C).permute(0, 3, 1, 2)    # one exponent per output channel
    return F.conv2d(xq.permute(0, 3, 1, 2).double(), wq.double(), padding=1).permute(0, 2, 3, 1)


def emulate(x, w, bias=None, resid=None) -> torch.Tensor:
    y = emulate_acc(x, w)
    if bias is not None:
        y = y + bias.double()
    if resid is None:
        return y.float()
    return bf(y.float()).float() + resid.float()                                      # (the caller compares against the bf16 rounding of this sum)


def exact_conv(x, w) -> torch.Tensor:
    return F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def _problem(N, H, W, Cin, Cout):
    """inputs of one problem and its references, computed once and shared (read-only) by the cases that use it.  Pixel p is scaled by
    2^((p mod 13) - 6), so neighbouring taps carry different exponents; weights are log-normal per output channel; one all-zero pixel and one
    all-zero output channel (exponent 0)."""
    g = torch.Generator().manual_seed(N * 1000003 + H * 1009 + W * 101 + Cin + Cout)
    M = N * H * W
    x = torch.randn(M, Cin, generator=g)
    x = torch.ldexp(x, ((torch.arange(M) % 13) - 6)[:, None])
    x[M // 3] = 0
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5 * torch.exp(torch.randn(Cout, 1, 1, 1, generator=g))
    w[Cout // 2] = 0
    x, w = bf(x).view(N, H, W, Cin), bf(w)
    bias = bf(torch.randn(Cout, generator=g))
    resid = bf(torch.randn(N, H, W, Cout, generator=g) * 4)
    acc = emulate_acc(x, w)
    return dict(x=x, w=w, bias=bias, resid=resid, acc=acc, exact=exact_conv(x, w))


def _weights(w):
    from motionrag_amd import ops
    return ops.quant_rows_e4m3(tap_major(w).to(DEV))


def _run(p, epi, bias=True, alias=False):
    from motionrag_amd import ops
    w8, w_exp = _weights(p["w"])
    resid = p["resid"].to(DEV) if epi == EPI_RESID else None
    before, before_q = ops.conv_fp8_launch_counts(), ops.fp8_launch_counts()
    got = ops.conv_implicit_fp8(p["x"].to(DEV), w8, w_exp, p["bias"].to(DEV) if bias else None, resid, out=resid if alias else None)
    after, after_q = ops.conv_fp8_launch_counts(), ops.fp8_launch_counts()
    assert after["conv"] == before["conv"] + 1 and after_q["quant"] == before_q["quant"] + 1 and after_q["gemm"] == before_q["gemm"]
    assert got.dtype == torch.bfloat16 and got.shape == p["resid"].shape
    if alias:
        assert got.data_ptr() == resid.data_ptr()
    return got


def _want(p, epi, bias=True):
    y = p["acc"] + (p["bias"].double() if bias else 0.0)
    return y.float() if epi == EPI_NONE else bf(y.float()).float() + p["resid"].float()


# ---------------------------------------------------------------------------------------------------------------- 1. kernel against the emulation
SHAPES = [(2, 16, 24, 64, 256),        # one K-step per tap; every output row at a border of some tap
          (1, 40, 52, 320, 320),       # five steps per tap (45 steps: a dead last half-tile), M = 2 080: a ragged last M-tile
          (3, 24, 24, 128, 260),       # Cout % 256 != 0 with Cout % 8 == 4: a ragged N-tile on 8-byte rows; tiles that span two samples
          (2, 72, 128, 320, 320)]      # the production row length at two samples


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_RESID], ids=["none", "resid"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_fp8_matches_emulation(hip, shape, epi):
    from motionrag_amd import ops
    assert ops.conv_fp8_supported(*shape)
    p = _problem(*shape)
    got = _run(p, epi)
    assert torch.isfinite(got.float()).all()
    want = _want(p, epi)
    err = rel_fro(got, want)
    # the same comparison per pixel scale class: the Frobenius norm above is carried by the largest pixels, this one weighs every class alike
    N, H, W, _, Cout = shape
    cls = (torch.arange(N * H * W) % 13)
    g2, w2 = got.float().cpu().view(-1, Cout), want.view(-1, Cout)
    worst = max(rel_fro(g2[cls == c], w2[cls == c]) for c in range(13))
    print(f"fp8 conv {shape} {'resid' if epi else 'none'}: rel fro vs emulation {err:.3e}, worst pixel class {worst:.3e} (bound {BOUND[epi]:.0e})")
    assert err <= BOUND[epi], err
    assert worst <= BOUND[epi], worst
    if epi == EPI_NONE:
        zero_ch = got[..., Cout // 2].float().cpu()
        assert torch.equal(zero_ch, p["bias"][Cout // 2].float().expand_as(zero_ch))           # the all-zero output channel: bias alone


def test_conv_fp8_tap_placement(hip):
    """impulses (one interior, one in a corner of the second sample) against a weight that is distinct per tap: the nine outputs sit at the nine
    mirrored positions with the right tap's value, exactly (1 .. 9 times a power of two are e4m3 and bf16 numbers)"""
    from motionrag_amd import ops
    N, H, W, Cin, Cout = 2, 9, 11, 64, 12
    x = torch.zeros(N, H, W, Cin)
    x[0, 4, 5, 7] = 1.0
    x[1, 0, 10, 63] = 2.0
    w = torch.zeros(Cout, Cin, 3, 3)
    taps = torch.arange(1.0, 10.0).view(3, 3)
    for co in range(Cout):
        w[co, 7] = taps * 2 ** (co % 3)
        w[co, 63] = taps.flip(0) * 2 ** (co % 2)
    x, w = bf(x), bf(w)
    want = exact_conv(x, w).float()
    assert (want != 0).sum() == Cout * (9 + 4)                                                   # the corner impulse keeps four taps
    w8, w_exp = _weights(w)
    got = ops.conv_implicit_fp8(x.to(DEV), w8, w_exp, None).float().cpu()
    assert torch.equal(got, want), (got - want).abs().max()
    assert got[0, 3, 4, 0] == 9.0 and got[0, 5, 6, 0] == 1.0 and got[0, 4, 4, 1] == 2 * 6.0      # y[ho, wo] = W[ky = y0 - ho + 1, kx = x0 - wo + 1]


def test_conv_fp8_in_place_residual(hip):
    shape = SHAPES[2]
    p = _problem(*shape)
    plain = _run(p, EPI_RESID)
    aliased = _run(p, EPI_RESID, alias=True)
    assert torch.equal(plain, aliased)


def test_conv_fp8_is_deterministic_and_captures(hip):
    """two runs are bit-equal; the quantiser + kernel pair captures into a graph (nothing read back, no allocation once warm) and replays to the
    eager result"""
    from motionrag_amd import ops
    p = _problem(*SHAPES[1])
    w8, w_exp = _weights(p["w"])
    x, bias, resid = p["x"].to(DEV), p["bias"].to(DEV), p["resid"].to(DEV)
    eager = ops.conv_implicit_fp8(x, w8, w_exp, bias, resid).clone()                             # warm: the workspace exists
    assert torch.equal(ops.conv_implicit_fp8(x, w8, w_exp, bias, resid), eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.conv_implicit_fp8(x, w8, w_exp, bias, resid)                                         # the capture stream's own workspace
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.HIPGraph() if hasattr(torch.cuda, "HIPGraph") else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = ops.conv_implicit_fp8(x, w8, w_exp, bias, resid)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---------------------------------------------------------------------------------------------------------------- 2. against un-quantised fp32
def test_conv_fp8_against_fp32_self_calibrated(hip):
    shape = SHAPES[1]
    p = _problem(*shape)
    E = rel_fro(p["acc"], p["exact"])
    G = rel_fro(_run(p, EPI_NONE, bias=False), p["exact"])
    print(f"fp8 conv {shape} vs float64: emulation E = {E:.4f}, kernel G = {G:.4f}")
    assert G <= 1.1 * E + 4e-3, (G, E)


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_conv_fp8_gate_matches_the_c_entry_point(hip):
    """admitted shapes launch (so this side of the table needs the GPU), refused ones return MRAG_ENOTSUP and count nothing"""
    from motionrag_amd import _lib, ops
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    # (shape, admitted): written out, not derived from ops.conv_fp8_supported
    table = [((1, 4, 4, 64, 16, 1, 0), True), ((2, 5, 3, 128, 12, 1, 0), True), ((1, 4, 4, 64, 16, 2, 0), False), ((1, 4, 4, 64, 16, 1, 1), False),
             ((1, 4, 4, 96, 16, 1, 0), False), ((1, 4, 4, 64, 14, 1, 0), False), ((1, 4, 4, 64, 8, 1, 0), False), ((1, 4, 4, 64, 4, 1, 0), False)]
    for (N, H, W, Cin, Cout, stride, up), admitted in table:
        a = _lib.ConvFp8Args()
        a.x8 = a.W8 = a.x_exp = a.w_exp = a.y = buf.data_ptr()                                  # zero bytes, zero exponents: a harmless launch
        a.N, a.H, a.Wd, a.Cin, a.Cout, a.stride, a.upsample = N, H, W, Cin, Cout, stride, up
        before = ops.conv_fp8_launch_counts()["conv"]
        rc = hip.mrag_conv_fp8(None, ctypes.byref(a))
        torch.cuda.synchronize()
        ok = ops.conv_fp8_supported(N, H, W, Cin, Cout, stride, bool(up))
        assert ok == admitted, (N, H, W, Cin, Cout, stride, up)
        assert rc == (_lib.MRAG_OK if ok else _lib.MRAG_ENOTSUP), (N, H, W, Cin, Cout, stride, up)
        assert ops.conv_fp8_launch_counts()["conv"] == before + (1 if ok else 0)
    with pytest.raises(ValueError):
        ops.conv_implicit_fp8(torch.zeros(1, 4, 4, 96, dtype=torch.bfloat16, device=DEV), buf[:16 * 864].view(16, 864), torch.zeros(16, dtype=torch.int32, device=DEV), None)


# ---------------------------------------------------------------------------------------------------------------- 4. one tile with the fp8 GEMM
@pytest.mark.parametrize("epi", [EPI_NONE, EPI_RESID], ids=["none", "resid"])
@pytest.mark.parametrize("n,cin,cout", [(300, 64, 320),     # 9 steps: the dead last half-tile, two row tiles, two column tiles, ragged both ways
                                        (257, 128, 48)],    # 18 steps: both halves live, and the GEMM's two-step tile
                         ids=["300x64x320", "257x128x48"])
def test_conv_fp8_on_1x1_images_is_the_fp8_gemm(hip, n, cin, cout, epi):
    """mrag_conv_fp8 and mrag_gemm_fp8_k64 run one tile (csrc/gemm_fp8_tile.h): on 1x1 images the convolution is the GEMM, bit for bit.  With H = W = 1
    eight taps gather zero bytes, so the accumulator receives exact zeros around the centre tap's Cin / 64 k-steps: the MFMA steps, in the order, of the GEMM
    on A8 = x8, a_exp = x_exp and W8 = the centre-tap column slice w8[:, 4 Cin : 5 Cin] (row stride 9 Cin, 16-byte aligned) with the same w_exp.  Bias and
    residual have the same rounding points in both epilogues."""
    from motionrag_amd import _lib, ops
    from test_gpu_ff_fp8 import _c_gemm
    g = torch.Generator().manual_seed(n + cin + cout)
    x = bf(torch.randn(n, cin, generator=g) * torch.exp2(torch.randint(-6, 7, (n, 1), generator=g).float())).to(DEV)
    w = bf(torch.randn(cout, 9 * cin, generator=g) * cin ** -0.5).to(DEV)
    bias = bf(torch.randn(cout, generator=g)).to(DEV)
    resid = bf(torch.randn(n, cout, generator=g) * 4).to(DEV) if epi == EPI_RESID else None
    x8, x_exp = ops.quant_rows_e4m3(x)
    w8, w_exp = ops.quant_rows_e4m3(w)
    conv = torch.empty(n, cout, dtype=torch.bfloat16, device=DEV)
    a = _lib.ConvFp8Args()
    a.x8, a.W8, a.x_exp, a.w_exp, a.bias, a.y = x8.data_ptr(), w8.data_ptr(), x_exp.data_ptr(), w_exp.data_ptr(), bias.data_ptr(), conv.data_ptr()
    a.N, a.H, a.Wd, a.Cin, a.Cout, a.stride, a.epilogue = n, 1, 1, cin, cout, 1, epi
    if resid is not None:
        a.resid = resid.data_ptr()
    _lib.check(hip.mrag_conv_fp8(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a)), "mrag_conv_fp8")
    gemm = _c_gemm(hip.mrag_gemm_fp8_k64, x8, x_exp, w8[:, 4 * cin:5 * cin], w_exp, bias, epi, resid)
    assert torch.equal(conv, gemm), (conv.float() - gemm.float()).abs().max()
    product = gemm.float() - bias.float() - (resid.float() if resid is not None else 0.0)
    assert torch.isfinite(gemm.float()).all() and product.abs().mean() > 0.05, product.abs().mean()   # the centre tap's product is in the result


# ---------------------------------------------------------------------------------------------------------------- 5. models
def _emulating_conv3x3(real, log):
    """layers.conv3x3 with the host emulation in place of the gated convolutions (the others run as they are)"""
    from motionrag_amd import ops

    def conv3x3(x, conv, *, stride=1, upsample=False, resid=None):
        N, H, W, C = x.shape
        if not ops.conv_fp8_supported(N, H, W, C, conv.weight.shape[0], stride, upsample):
            return real(x, conv, stride=stride, upsample=upsample, resid=resid)
        log.append(conv)
        y = emulate(x.cpu(), conv.weight.detach().cpu(), conv.bias.detach().cpu() if conv.bias is not None else None, resid.cpu() if resid is not None else None)
        return bf(y).to(x.device)
    return conv3x3


def _dc_unet(golden_dir):
    """the reduced UNetModel of tests/test_gpu_unet.py with its G10 weights: model_channels = 64, so every ResBlock convolution has Cin % 64 == 0"""
    from motionrag_amd import dynamicrafter as dc
    from test_oracle_golden import dc_unet_fixture
    g, sd, spec, x, ctx = dc_unet_fixture(golden_dir)
    unet = dc.UNetModel(in_channels=8, out_channels=4, model_channels=64, attention_resolutions=(1, 2), num_res_blocks=1, channel_mult=(1, 2),
                        num_head_channels=64, transformer_depth=1, context_dim=64, use_linear=True, temporal_conv=True, temporal_attention=True,
                        temporal_self_att_only=True, use_relative_position=False, temporal_length=4, addition_attention=True,
                        image_cross_attention=True, action_cross_attention=True, default_fs=10, fs_condition=True)
    unet.load_state_dict(sd, strict=True)
    unet = unet.to(DEV, torch.bfloat16)
    args = (x.to(DEV), torch.from_numpy(g["timesteps"]).to(DEV))
    kw = dict(context={k: v.to(DEV) for k, v in ctx.items()}, fs=torch.from_numpy(g["fs"]).to(DEV))
    return unet, args, kw


def test_dc_unet_switch_off_changes_nothing(hip, golden_dir):
    """a model that never saw the setter, and one switched on and back off: the same bits, no fp8 launch"""
    from motionrag_amd import ops
    unet, args, kw = _dc_unet(golden_dir)
    never = unet(*args, **kw).clone()
    counts = getattr(ops, "conv_fp8_launch_counts", lambda: {"conv": 0})
    before = counts()
    again = unet(*args, **kw)
    assert torch.equal(again, never) and counts() == before
    from motionrag_amd import layers
    setter = getattr(layers, "set_conv_precision", None)
    if setter is not None:
        setter(unet, "fp8")
        setter(unet, "bf16")
        before = counts()
        assert torch.equal(unet(*args, **kw), never) and counts() == before


def _conv_names(unet, convs):
    names = {id(m): n for n, m in unet.named_modules()}
    return sorted(names[id(c)] for c in convs)


def test_dc_unet_fp8_convolutions_against_emulation(hip, golden_dir, monkeypatch):
    """the reduced model's problems are a few tiles each, so the test lifts layers.CONV_FP8_MIN_TILES (the production threshold of 192 tiles, below which
    a marked convolution stays bf16) to reach the kernel"""
    from motionrag_amd import dynamicrafter as dc, layers, ops
    monkeypatch.setattr(layers, "CONV_FP8_MIN_TILES", 0)
    unet, args, kw = _dc_unet(golden_dir)
    want = unet(*args, **kw).clone()                                                             # the bf16 model

    emu_log = []
    monkeypatch.setattr(dc, "conv3x3", _emulating_conv3x3(layers.conv3x3, emu_log))
    emu = unet(*args, **kw).clone()
    monkeypatch.setattr(dc, "conv3x3", layers.conv3x3)

    assert layers.set_conv_precision(unet, "fp8") is unet
    unet(*args, **kw)                                                                            # the first fp8 forward also quantises the weights (once)
    calls = []

    def logging_conv3x3(x, conv, **k):
        before = ops.conv_fp8_launch_counts()["conv"]
        y = layers.conv3x3(x, conv, **k)
        calls.append((conv, ops.conv_fp8_launch_counts()["conv"] - before))                      # what RAN, from the launch counter
        return y
    monkeypatch.setattr(dc, "conv3x3", logging_conv3x3)
    before, before_q = ops.conv_fp8_launch_counts(), ops.fp8_launch_counts()
    got = unet(*args, **kw)
    after, after_q = ops.conv_fp8_launch_counts(), ops.fp8_launch_counts()
    monkeypatch.setattr(dc, "conv3x3", layers.conv3x3)
    # the expected convolutions by name: the ResBlocks' in_layers / out_layers / 3x3 skip connections and nothing else -- not conv_in (from 8 channels),
    # not conv_out (to 4 channels: `out.2`), not the stride-2 Downsample, not the Upsample
    ran = _conv_names(unet, [c for c, n in calls if n])
    stayed = _conv_names(unet, [c for c, n in calls if not n])
    assert all(n == 1 for c, n in calls if n)
    assert stayed == sorted(["input_blocks.0.0", "out.2"] + [n for n, m in unet.named_modules() if isinstance(m, (dc.Downsample, dc.Upsample)) for n in
                                                             [n + (".op" if isinstance(m, dc.Downsample) else ".conv")]]), stayed
    assert len(ran) == 16 and all(".in_layers.2" in n or ".out_layers.3" in n or ".skip_connection" in n for n in ran), ran
    assert _conv_names(unet, emu_log) == ran                                                     # the emulated forward replaced the same convolutions
    assert after["conv"] - before["conv"] == 16 and after_q["quant"] - before_q["quant"] == 16   # activations only: the weights are cached
    assert torch.isfinite(got.float()).all()
    E_model, G_model = rel_fro(emu, want), rel_fro(got, want)
    print(f"fp8 convolutions, reduced DynamiCrafter UNet ({len(ran)} of {len(calls)} conv3x3 calls): E_model = {E_model:.4f}, kernel path = {G_model:.4f}, "
          f"bound = {1.5 * E_model + 0.02:.4f}")
    assert E_model > 1e-3                                   # the emulation did quantise something
    assert G_model <= 1.5 * E_model + 0.02, (G_model, E_model)
    assert not torch.equal(got, want)


@pytest.mark.parametrize("cin,cout", [(8, 320), (320, 4), (128, 8)], ids=["unet_conv_in", "unet_conv_out", "vae_enc_conv_out"])
def test_first_and_last_convolutions_stay_bf16(hip, monkeypatch, cin, cout):
    """the convolutions from or to 3, 4 or 8 channels (the UNets' conv_in 8 -> 320 and conv_out 320 -> 4, the VAE encoders' conv_out -> 8), marked fp8 and with
    the tile threshold lifted: the fp8 launch counter does not move and the result is the unmarked module's, bit for bit"""
    from motionrag_amd import layers, ops
    monkeypatch.setattr(layers, "CONV_FP8_MIN_TILES", 0)
    g = torch.Generator().manual_seed(cin + cout)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.05)
    conv = conv.to(DEV, torch.bfloat16)
    x = bf(torch.randn(2, 12, 16, cin, generator=g)).to(DEV)
    plain = layers.conv3x3(x, conv).clone()
    layers.set_conv_precision(conv, "fp8")
    before = ops.conv_fp8_launch_counts()
    marked = layers.conv3x3(x, conv)
    assert ops.conv_fp8_launch_counts() == before
    assert torch.equal(marked, plain)


def test_small_problems_stay_bf16_below_the_tile_threshold(hip, monkeypatch):
    """layers.CONV_FP8_MIN_TILES: a marked, admitted convolution of fewer than 192 output tiles of 256x256 stays on the bf16 kernel (which has a 128x128 tile
    for it); at the threshold it takes the fp8 kernel"""
    from motionrag_amd import layers, ops
    assert layers.CONV_FP8_MIN_TILES == 192
    conv = layers.set_conv_precision(torch.nn.Conv2d(64, 64, 3, padding=1).to(DEV, torch.bfloat16), "fp8")
    for n_frames, runs_fp8 in ((2, False), (8, True)):                  # 2 x 96 x 128 rows = 96 tiles; 8 x 96 x 64 = 192 tiles
        x = bf(torch.randn(n_frames, 96, 128 if n_frames == 2 else 64, 64, generator=torch.Generator().manual_seed(1))).to(DEV)
        assert ops.conv_fp8_supported(*x.shape, 64)
        before = ops.conv_fp8_launch_counts()["conv"]
        layers.conv3x3(x, conv)
        assert ops.conv_fp8_launch_counts()["conv"] - before == (1 if runs_fp8 else 0)


def _block_case(hip, monkeypatch, module, block, run):
    """one block: bf16, emulated and fp8 forwards; both of its 3x3 convolutions take the fp8 kernel"""
    from motionrag_amd import layers, ops
    monkeypatch.setattr(layers, "CONV_FP8_MIN_TILES", 0)            # a block of the reduced size is a few tiles
    want = run(block).clone()
    log = []
    monkeypatch.setattr(module, "conv3x3", _emulating_conv3x3(layers.conv3x3, log))
    emu = run(block).clone()
    monkeypatch.setattr(module, "conv3x3", layers.conv3x3)
    layers.set_conv_precision(block, "fp8")
    before = ops.conv_fp8_launch_counts()
    got = run(block)
    assert ops.conv_fp8_launch_counts()["conv"] - before["conv"] == len(log) == 2
    E, G = rel_fro(emu, want), rel_fro(got, want)
    print(f"{type(block).__name__}: E = {E:.4f}, kernel path = {G:.4f}; kernel vs emulation {rel_fro(got, emu):.4f}")
    assert E > 1e-3 and G <= 1.5 * E + 0.02, (G, E)


def _randomise(block, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in block.named_parameters():
            if prm.dim() > 1:
                prm.copy_(torch.randn(prm.shape, generator=g) * (prm[0].numel() ** -0.5))
            else:
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.1 + (1.0 if "norm" in name and name.endswith("weight") else 0.0))
    return block.to(DEV, torch.bfloat16)


def test_svd_resnet_block_takes_the_fp8_path(hip, monkeypatch):
    from motionrag_amd import svd_unet
    block = _randomise(svd_unet.ResnetBlock2D(64, 128, 128, 1e-5), 5)
    g = torch.Generator().manual_seed(6)
    x = bf(torch.randn(3, 12, 10, 64, generator=g)).to(DEV)
    temb = bf(F.silu(torch.randn(3, 128, generator=g))).to(DEV)
    _block_case(hip, monkeypatch, svd_unet, block, lambda b: b(x, temb))


def test_dc_vae_resnet_block_takes_the_fp8_path(hip, monkeypatch):
    from motionrag_amd import dynamicrafter_vae
    block = _randomise(dynamicrafter_vae.ResnetBlock(in_channels=128, out_channels=64), 7)
    x = bf(torch.randn(2, 9, 14, 128, generator=torch.Generator().manual_seed(8))).to(DEV)
    _block_case(hip, monkeypatch, dynamicrafter_vae, block, lambda b: b(x))
