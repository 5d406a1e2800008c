"""The opt-in fp8 (e4m3) path of the UNets' feed-forward linears on the GPU: mrag_layernorm_e4m3, mrag_gemm_fp8_k64 (ops.layernorm_e4m3 /
ops.linear_fp8_k64) and layers.set_ff_precision.

References, all computed on the host in the style of tests/test_gpu_fp8_linear.py (its quant_ref / dequant / rel_fro are used as they are):
  * LayerNorm -> e4m3 is specified as the composition of two kernels the project has: ops.quant_rows_e4m3(ops.layernorm(x)), compared with torch.equal.
  * mrag_gemm_fp8_k64 with EPI_NONE / EPI_RESID is specified by the kernel it extends: mrag_gemm_fp8 on the same operands (K % 128 == 0) or on
    the operands zero-padded to the next multiple of 128, compared with torch.equal (adding the products of zero bytes changes no fp32 sum).
  * EPI_GEGLU: the fp32 product of the decoded operands times 2^-(ea + ew), plus bias, de-interleaved, both halves rounded to bf16,
    v * gelu_erf(g), rounded to bf16.  The emulation shares all three rounding points, so what remains are rounding flips from the fp32 summation
    order and the device's erf (|error| <= 1e-7): <= 4e-3 relative Frobenius error, one whole bf16 rounding (2^-8) on every element -- the bound of
    EPI_GELU_TANH in tests/test_gpu_fp8_linear.py; EPI_RESID rounds twice: 8e-3 as there.
  * un-quantised fp32 GEGLU(A . W^T + bias) on the bf16 inputs, self-calibrated: E = the emulation's error against it, G = the kernel's;
    G <= 1.1 E + 4e-3.
  * model level: the E_model scheme of test_dit_fp8_linears_against_oracle with the fp32 DynamiCrafter oracle (see the test's docstring)."""
import ctypes
import functools
import re

import pytest
import torch
import torch.nn.functional as F

from test_gpu_fp8_linear import bf, decode, dequant, quant_ref, rel_fro

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPI_NONE, EPI_RESID, EPI_GEGLU = 0, 3, 6
EPI_NAMES = {EPI_NONE: "none", EPI_RESID: "resid", EPI_GEGLU: "geglu"}
BOUND = {EPI_NONE: 4e-3, EPI_RESID: 8e-3, EPI_GEGLU: 4e-3}


# ---------------------------------------------------------------------------------------------------------------- 1. LayerNorm -> e4m3, exact
def _ln_input(M, K, seed, zero_beta):
    """rows with scales spread over 2^+-12; row 1 is constant (2.0: its mean is exact, so the normalised row is exactly zero)"""
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-12, 13, (M, 1), generator=g).float()))
    if M >= 2:
        x[1] = 2.0
    gamma = bf(1.0 + 0.5 * torch.randn(K, generator=g))
    beta = torch.zeros(K, dtype=torch.bfloat16) if zero_beta else bf(0.3 * torch.randn(K, generator=g))
    return x, gamma, beta


# (1030, 320), (1025, 640), (1026, 1280): from 1024 rows on these widths run the several-rows-per-wave LayerNorm, whose statistics round differently
# K = 2304: wider than a row the kernel keeps in registers -- refused, the wrapper runs the two launches
LN_SHAPES = [(1, 320), (37, 320), (300, 640), (67, 1280), (1030, 320), (1025, 640), (1026, 1280), (300, 64), (300, 2048), (37, 2304)]


@pytest.mark.parametrize("zero_beta", [False, True], ids=["beta", "zero_beta"])
@pytest.mark.parametrize("M,K", LN_SHAPES)
def test_layernorm_e4m3_is_the_two_kernels_bit_for_bit(hip, M, K, zero_beta):
    from motionrag_amd import ops
    x, gamma, beta = _ln_input(M, K, 7 * M + K, zero_beta)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    want8, want_e = ops.quant_rows_e4m3(ops.layernorm(xd, gd, bd, 1e-5))
    before, before_q = ops.fp8_k64_launch_counts(), ops.fp8_launch_counts()
    x8, ex = ops.layernorm_e4m3(xd, gd, bd, 1e-5)
    after, after_q = ops.fp8_k64_launch_counts(), ops.fp8_launch_counts()
    fused = K <= 2048
    assert after["ln"] - before["ln"] == (1 if fused else 0) and after["gemm"] == before["gemm"]          # which path ran
    assert after_q["quant"] - before_q["quant"] == (0 if fused else 1) and after_q["gemm"] == before_q["gemm"]
    assert x8.dtype == torch.uint8 and tuple(x8.shape) == (M, K) and ex.dtype == torch.int32 and tuple(ex.shape) == (M,)
    assert torch.equal(ex, want_e)
    assert torch.equal(x8, want8)
    assert decode(x8).abs().max() <= 448.0
    if M >= 2:
        if zero_beta:                                                   # the constant row: all zero, exponent 0
            assert ex[1].item() == 0 and (x8[1] == 0).all()
        else:                                                           # ... or beta itself
            q_ref, e_ref = quant_ref(beta[None])
            assert ex[1].item() == e_ref[0].item() and torch.equal(decode(x8[1:2]), q_ref)
    # against the host: the exponents are the reference quantiser's of the device's LayerNorm rows
    assert torch.equal(ex.cpu(), quant_ref(ops.layernorm(xd, gd, bd, 1e-5).cpu())[1])


def test_layernorm_e4m3_without_gamma_and_beta(hip):
    from motionrag_amd import ops
    x, _, _ = _ln_input(45, 320, 3, False)
    xd = x.to(DEV)
    want8, want_e = ops.quant_rows_e4m3(ops.layernorm(xd, None, None, 1e-6))
    x8, ex = ops.layernorm_e4m3(xd, None, None, 1e-6)
    assert torch.equal(x8, want8) and torch.equal(ex, want_e)


# ---------------------------------------------------------------------------------------------------------------- 2. GEMM against the kernel it extends
@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    """bf16 inputs of one problem (host), shared read-only by the cases that use it"""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    x = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = bf(torch.randn(N, generator=g))
    resid = bf(torch.randn(M, N, generator=g))
    return x, w, bias, resid


def _c_gemm(entry, a8, ea, w8, ew, bias, epi, resid=None, out=None):
    """one of the two C entry points on already quantised operands"""
    from motionrag_amd import _lib
    M, K = a8.shape
    N = w8.shape[0]
    if out is None:
        out = torch.empty(M, N // 2 if epi == EPI_GEGLU else N, dtype=torch.bfloat16, device=DEV)
    a = _lib.GemmFp8Args()
    a.A8, a.W8, a.a_exp, a.w_exp, a.C = a8.data_ptr(), w8.data_ptr(), ea.data_ptr(), ew.data_ptr(), out.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, a8.stride(0), w8.stride(0), out.stride(0)
    a.epilogue = epi
    if resid is not None:
        a.resid, a.ldr = resid.data_ptr(), resid.stride(0)
    _lib.check(entry(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a)), "fp8 gemm")
    return out


def _padded(t8, K128):
    """a separate allocation with the K bytes of every row followed by zero bytes (e4m3 zero)"""
    p = torch.zeros(t8.shape[0], K128, dtype=torch.uint8, device=DEV)
    p[:, :t8.shape[1]] = t8
    return p


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_RESID], ids=lambda e: EPI_NAMES[e])
@pytest.mark.parametrize("M,N,K", [(300, 320, 256), (8, 32, 128), (300, 320, 64), (300, 320, 192), (300, 320, 320)])
def test_gemm_fp8_k64_equals_the_kernel_it_extends(hip, M, N, K, epi):
    """K % 128 == 0: the same operands; K % 128 == 64: mrag_gemm_fp8 on operands zero-padded to whole K-tiles.  The unpadded A8 and W8 are allocations
    of exactly M K and N K bytes: a read behind the last row's K bytes would leave the buffer."""
    from motionrag_amd import ops
    x, w, bias, resid = _operands(M, N, K)
    a8, ea = ops.quant_rows_e4m3(x.to(DEV))
    w8, ew = ops.quant_rows_e4m3(w.to(DEV))
    assert a8.numel() == M * K and w8.numel() == N * K and a8.is_contiguous() and w8.is_contiguous()
    bd, rd = bias.to(DEV), (resid.to(DEV) if epi == EPI_RESID else None)
    before, before_lin = ops.fp8_k64_launch_counts(), ops.fp8_launch_counts()
    got = _c_gemm(hip.mrag_gemm_fp8_k64, a8, ea, w8, ew, bd, epi, rd)
    after, after_lin = ops.fp8_k64_launch_counts(), ops.fp8_launch_counts()
    assert after["gemm"] == before["gemm"] + 1 and after["ln"] == before["ln"] and after_lin == before_lin   # its own counter, not mrag_gemm_fp8's
    K128 = (K + 127) // 128 * 128
    if K128 != K:
        a8r, w8r = _padded(a8, K128), _padded(w8, K128)
        assert a8r.data_ptr() != a8.data_ptr() and w8r.data_ptr() != w8.data_ptr()
    else:
        a8r, w8r = a8, w8
    want = _c_gemm(hip.mrag_gemm_fp8, a8r, ea, w8r, ew, bd, epi, rd)
    assert torch.isfinite(got.float()).all() and got.float().abs().max() > 0.1
    assert torch.equal(got, want)
    # and through the torch front end, from bf16 rows: the same bits again
    via_ops = ops.linear_fp8_k64(x.to(DEV), w8, ew, bd, epilogue=epi, resid=rd)
    assert torch.equal(via_ops, want)


# ---------------------------------------------------------------------------------------------------------------- 3. GEGLU against the emulation
@functools.lru_cache(maxsize=None)
def _geglu_problem(M, N, K):
    """W [N, K] in the module's order ([value rows | gate rows], `chunk(2)`); the emulation and the un-quantised fp32 result"""
    x, w, bias, _ = _operands(M, N, K)
    qa, ea = quant_ref(x)
    qw, ew = quant_ref(w)
    acc = torch.ldexp(qa @ qw.T, -(ea[:, None] + ew[None, :])) + bias.float()
    v, g = acc.chunk(2, dim=1)
    emu = bf(bf(v).float() * F.gelu(bf(g).float())).float()
    ve, ge = (x.float() @ w.float().T + bias.float()).chunk(2, dim=1)
    return dict(x=x, w=w, bias=bias, emu=emu, exact=ve * F.gelu(ge))


def _run_geglu(p, M, N):
    from motionrag_amd import ops
    wi, bi = ops.geglu_interleave(p["w"].to(DEV), p["bias"].to(DEV))
    w8, ew = ops.quant_rows_e4m3(wi)
    before = ops.fp8_k64_launch_counts()
    got = ops.linear_fp8_k64(p["x"].to(DEV), w8, ew, bi, epilogue=EPI_GEGLU)
    assert ops.fp8_k64_launch_counts()["gemm"] == before["gemm"] + 1
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N // 2)
    return got


# (300, 320, 320): the second n-tile holds two 32-row groups; (513, 2560, 320): the level-0 width, three m-tiles with a ragged last one
GEGLU_SHAPES = [(300, 64, 64), (300, 320, 320), (513, 2560, 320), (64, 5120, 640)]


@pytest.mark.parametrize("M,N,K", GEGLU_SHAPES)
def test_gemm_fp8_k64_geglu_matches_emulation(hip, M, N, K):
    p = _geglu_problem(M, N, K)
    got = _run_geglu(p, M, N)
    assert torch.isfinite(got.float()).all()
    err = rel_fro(got, p["emu"])
    print(f"fp8 k64 gemm {M}x{N}x{K} geglu: rel fro vs emulation {err:.3e} (bound {BOUND[EPI_GEGLU]:.0e})")
    assert err <= BOUND[EPI_GEGLU], err


@pytest.mark.parametrize("M,N,K", [(513, 2560, 320), (64, 5120, 640)])
def test_gemm_fp8_k64_geglu_against_fp32_self_calibrated(hip, M, N, K):
    p = _geglu_problem(M, N, K)
    E = rel_fro(p["emu"], p["exact"])
    G = rel_fro(_run_geglu(p, M, N), p["exact"])
    print(f"fp8 k64 gemm {M}x{N}x{K} geglu vs fp32: emulation E = {E:.4f}, kernel G = {G:.4f}")
    assert 0.02 < E < 0.09                                              # the quantisation error of two operands through v * gelu(g)
    assert G <= 1.1 * E + 4e-3, (G, E)


def test_gemm_fp8_k64_geglu_column_map(hip):
    """one-hot rows of A (row m selects k = m % 64) and power-of-two weights, distinct per (output column, k) between value and gate: C[m, j] must be
    v * gelu(g) of W's rows j and inner + j at that k.  A value / gate mix-up or a misplaced 16-column group lands on another pair."""
    from motionrag_amd import ops
    M, K, inner = 300, 64, 192                                          # N = 384: two n-tiles, the second with four groups
    j, k = torch.arange(inner)[:, None], torch.arange(K)[None, :]
    wv = torch.exp2(((j + k) % 7 - 3).float())                          # 2^-3 .. 2^3: exact in e4m3 under every row's scale
    wg = torch.exp2(((3 * j + 5 * k) % 5 - 2).float()) * torch.where((j + k) % 2 == 0, 1.0, -1.0)
    w = bf(torch.cat([wv, wg]))
    x = torch.zeros(M, K)
    x[torch.arange(M), torch.arange(M) % K] = 1.0
    wi, _ = ops.geglu_interleave(w.to(DEV), None)
    w8, ew = ops.quant_rows_e4m3(wi)
    got = ops.linear_fp8_k64(bf(x).to(DEV), w8, ew, None, epilogue=EPI_GEGLU).float().cpu()
    sel = torch.arange(M) % K
    want = wv.T[sel] * F.gelu(wg.T[sel])                                # [M, inner]: exact up to the device's erf and the final bf16 rounding
    assert tuple(got.shape) == (M, inner)
    assert ((got - want).abs() <= 2.0 ** -7 * want.abs()).all()
    swapped = wg.T[sel] * F.gelu(wv.T[sel])
    assert ((swapped - want).abs() > 2.0 ** -5 * want.abs()).float().mean() > 0.5    # the check does tell the two halves apart


@pytest.mark.parametrize("M,N,K", [(300, 320, 1280), (513, 320, 320)])
def test_gemm_fp8_k64_resid_matches_emulation(hip, M, N, K):
    from motionrag_amd import ops
    x, w, bias, resid = _operands(M, N, K)
    qa, ea = quant_ref(x)
    qw, ew = quant_ref(w)
    want = bf(torch.ldexp(qa @ qw.T, -(ea[:, None] + ew[None, :])) + bias.float()).float() + resid.float()
    w8, w_exp = ops.quant_rows_e4m3(w.to(DEV))
    got = ops.linear_fp8_k64(x.to(DEV), w8, w_exp, bias.to(DEV), epilogue=EPI_RESID, resid=resid.to(DEV))
    err = rel_fro(got, want)
    print(f"fp8 k64 gemm {M}x{N}x{K} resid: rel fro vs emulation {err:.3e} (bound {BOUND[EPI_RESID]:.0e})")
    assert err <= BOUND[EPI_RESID], err


# ---------------------------------------------------------------------------------------------------------------- 4. in-place residual
def test_gemm_fp8_k64_residual_in_place(hip):
    from motionrag_amd import ops
    M, N, K = 300, 320, 1280
    x, w, bias, resid = _operands(M, N, K)
    w8, w_exp = ops.quant_rows_e4m3(w.to(DEV))
    xd, bd = x.to(DEV), bias.to(DEV)
    separate = ops.linear_fp8_k64(xd, w8, w_exp, bd, epilogue=EPI_RESID, resid=resid.to(DEV))
    r = resid.to(DEV)
    same = ops.linear_fp8_k64(xd, w8, w_exp, bd, epilogue=EPI_RESID, resid=r, out=r)
    assert same.data_ptr() == r.data_ptr()
    assert torch.equal(same, separate) and not torch.equal(separate.cpu(), resid)


def test_linear_fp8_k64_refuses_what_the_kernel_does_not_take(hip):
    from motionrag_amd import ops
    w8, w_exp = ops.quant_rows_e4m3(torch.zeros(48, 96, dtype=torch.bfloat16, device=DEV))
    x = torch.zeros(8, 96, dtype=torch.bfloat16, device=DEV)
    before = ops.fp8_k64_launch_counts()
    with pytest.raises(ValueError):
        ops.linear_fp8_k64(x, w8, w_exp)                                # K = 96
    w8, w_exp = ops.quant_rows_e4m3(torch.zeros(48, 64, dtype=torch.bfloat16, device=DEV))
    x = torch.zeros(8, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.linear_fp8_k64(x, w8, w_exp, epilogue=EPI_GEGLU)            # N = 48: not whole 32-row groups
    with pytest.raises(ValueError):
        ops.linear_fp8_k64(x, w8, w_exp, epilogue=1)                    # EPI_GELU_TANH
    with pytest.raises(ValueError):
        ops.linear_fp8_k64(x, w8, w_exp, epilogue=EPI_RESID)            # no residual
    assert ops.fp8_k64_launch_counts() == before


# ---------------------------------------------------------------------------------------------------------------- 5. determinism and capture
def _open_gates(monkeypatch):
    """reduced models are a few hundred rows of 64 .. 512 channels: lift the production gates (layers.FF_FP8_MIN_ROWS and the two FF2 gates) to reach the kernels"""
    from motionrag_amd import layers
    for name in ("FF_FP8_MIN_ROWS", "FF2_FP8_MIN_ROWS", "FF2_FP8_MIN_WIDTH"):
        monkeypatch.setattr(layers, name, 0)


def _randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in module.named_parameters():
            if prm.dim() > 1:
                prm.copy_(torch.randn(prm.shape, generator=g) * (prm[0].numel() ** -0.5))
            else:
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.1 + (1.0 if "norm" in name and name.endswith("weight") else 0.0))
    return module.to(DEV, torch.bfloat16)


def test_feed_forward_fp8_is_deterministic_and_captures(hip, monkeypatch):
    """FF1 + FF2 of one feed-forward at M = 512, C = 320: no host synchronisation, nothing read back"""
    from motionrag_amd import dynamicrafter as dc, layers, ops
    _open_gates(monkeypatch)
    C = 320
    holder = torch.nn.ModuleDict({"norm": torch.nn.LayerNorm(C), "ff": dc.FeedForward(C)})
    holder = _randomise(holder, 11)
    layers.set_ff_precision(holder, "fp8")
    x = bf(torch.randn(512, C, generator=torch.Generator().manual_seed(12))).to(DEV)
    before = ops.fp8_k64_launch_counts()
    first = layers.feed_forward(holder["ff"], holder["norm"], x).clone()     # warm: weights quantised, workspaces grown
    after = ops.fp8_k64_launch_counts()
    assert after["gemm"] - before["gemm"] == 2 and after["ln"] - before["ln"] == 1
    second = layers.feed_forward(holder["ff"], holder["norm"], x).clone()
    assert torch.equal(first, second)
    graph = torch.cuda.HIPGraph() if hasattr(torch.cuda, "HIPGraph") else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = layers.feed_forward(holder["ff"], holder["norm"], x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)


# ---------------------------------------------------------------------------------------------------------------- 6. DynamiCrafter
FF_WEIGHT = re.compile(r"\.ff\.net\.(0\.proj|2)\.weight$")


def _counts():
    from motionrag_amd import ops
    return ops.fp8_k64_launch_counts(), ops.fp8_launch_counts()


def test_dc_unet_ff_fp8_against_oracle(hip, golden_dir, monkeypatch):
    """The reduced DynamiCrafter UNet of tests/test_gpu_conv_fp8.py (`_dc_unet`: tests/golden/dc_unet.npz, widths 64 / 128 / 512, 15 FeedForwards).
    E_model: the fp32 oracle (bf16-rounded weights and inputs) against the same oracle with F.linear of the 30 feed-forward weights patched to quantise the
    bf16-rounded input rows and the weight rows with the reference quantiser -- 0.0602 computed on the CPU (ff1 alone 0.049, ff2 alone 0.035), window
    0.03 .. 0.09.  The fp8 model must be within 1.5 E_model + 0.03 of the un-patched oracle: 0.03 is the bf16 path's own bound for this UNet
    (tests/test_gpu_unet.py: rel_l2 = 3e-2), the factor 1.5 as in test_dit_fp8_linears_against_oracle.  Measured on an MI355X: kernel path 0.0634 (bound 0.1202),
    the bf16 model 0.0138."""
    from motionrag_amd import dynamicrafter as dc, layers, ops
    from oracle import dynamicrafter_ref
    from test_gpu_conv_fp8 import _dc_unet
    from test_oracle_golden import dc_unet_fixture
    shipped = layers.FF_FP8_MIN_ROWS
    unet, args, kw = _dc_unet(golden_dir)
    n_ff = sum(isinstance(m, dc.FeedForward) for m in unet.modules())
    assert n_ff == 15
    never_switched = unet(*args, **kw).clone()

    # marked, at the shipped row threshold: the reduced model's few hundred rows stay on the bf16 kernels
    layers.set_ff_precision(unet, "fp8")
    before = _counts()
    assert torch.equal(unet(*args, **kw), never_switched) and _counts() == before
    # switched on and back: the same bits, no fp8 launch
    _open_gates(monkeypatch)
    layers.set_ff_precision(unet, "bf16")
    before = _counts()
    assert torch.equal(unet(*args, **kw), never_switched) and _counts() == before

    layers.set_ff_precision(unet, "fp8")
    unet(*args, **kw)                                                   # the first fp8 forward also quantises the weights (once)
    before, before_q = _counts()
    got = unet(*args, **kw).clone()
    after, after_q = _counts()
    assert after["gemm"] - before["gemm"] == 2 * n_ff and after["ln"] - before["ln"] == n_ff
    assert after_q["quant"] - before_q["quant"] == n_ff and after_q["gemm"] == before_q["gemm"]      # the row quantiser in front of every FF2
    assert torch.isfinite(got.float()).all() and not torch.equal(got, never_switched)

    layers.set_ff_precision(unet, "fp8", sites=("ff1",))
    before, before_q = _counts()
    unet(*args, **kw)
    after, after_q = _counts()
    assert after["gemm"] - before["gemm"] == n_ff and after["ln"] - before["ln"] == n_ff and after_q == before_q
    layers.set_ff_precision(unet, "fp8", sites=("ff2",))
    before, before_q = _counts()
    unet(*args, **kw)
    after, after_q = _counts()
    assert after["gemm"] - before["gemm"] == n_ff and after["ln"] == before["ln"] and after_q["quant"] - before_q["quant"] == n_ff

    # the fp32 oracle, and the same oracle with the feed-forward weights on reference-quantised operands
    g, sd, spec, x, ctx = dc_unet_fixture(golden_dir)
    sdr = {k: bf(v).float() for k, v in sd.items()}
    xr, ctxr = bf(x).float(), {k: bf(v).float() for k, v in ctx.items()}
    t, fs = torch.from_numpy(g["timesteps"]), torch.from_numpy(g["fs"])
    want = dynamicrafter_ref.unet_forward(sdr, spec, xr, t, ctxr, fs)
    patched_ids = {id(v) for k, v in sdr.items() if FF_WEIGHT.search(k)}
    assert len(patched_ids) == 2 * n_ff
    plain_linear = F.linear
    hits = []

    def quantised_linear(inp_, weight, bias=None):
        if id(weight) not in patched_ids:
            return plain_linear(inp_, weight, bias)
        hits.append(id(weight))
        x2 = bf(inp_.reshape(-1, inp_.shape[-1]))                       # the kernel's activations are bf16
        return plain_linear(dequant(*quant_ref(x2)).reshape(inp_.shape), dequant(*quant_ref(weight)), bias)

    monkeypatch.setattr(torch.nn.functional, "linear", quantised_linear)
    emu = dynamicrafter_ref.unet_forward(sdr, spec, xr, t, ctxr, fs)
    monkeypatch.setattr(torch.nn.functional, "linear", plain_linear)
    assert len(hits) == 2 * n_ff
    E_model, G_model, B_model = rel_fro(emu, want), rel_fro(got, want), rel_fro(never_switched, want)
    print(f"fp8 feed-forwards, reduced DynamiCrafter UNet ({n_ff} FeedForwards): E_model = {E_model:.4f}, kernel path = {G_model:.4f}, "
          f"bound = {1.5 * E_model + 0.03:.4f}; the bf16 model: {B_model:.4f}")
    assert 0.03 < E_model < 0.09                                        # (0.0602 computed on the CPU)
    assert G_model <= 1.5 * E_model + 0.03, (G_model, E_model)
    assert shipped > 0 and layers.FF_FP8_MIN_ROWS == 0


def test_ff_fp8_gates_keep_the_measured_losses_on_bf16(hip, monkeypatch):
    """the shipped gates: a marked feed-forward of fewer than FF_FP8_MIN_ROWS rows launches nothing on fp8; from that many rows on FF1 does, and
    FF2 only from FF2_FP8_MIN_ROWS rows and FF2_FP8_MIN_WIDTH channels on (in narrower blocks the quantiser pass costs what the kernel saves, or more)"""
    from motionrag_amd import dynamicrafter as dc, layers, ops
    assert (layers.FF_FP8_MIN_ROWS, layers.FF2_FP8_MIN_ROWS, layers.FF2_FP8_MIN_WIDTH) == (4608, 18432, 1280)
    monkeypatch.setattr(layers, "FF_FP8_MIN_ROWS", 128)                 # the rule at test-sized row counts and widths
    monkeypatch.setattr(layers, "FF2_FP8_MIN_ROWS", 256)
    monkeypatch.setattr(layers, "FF2_FP8_MIN_WIDTH", 640)
    for C, rows, want in ((320, 127, (0, 0)), (320, 256, (1, 1)), (640, 255, (1, 1)), (640, 256, (2, 1))):
        holder = _randomise(torch.nn.ModuleDict({"norm": torch.nn.LayerNorm(C), "ff": dc.FeedForward(C)}), C)
        x = bf(torch.randn(rows, C, generator=torch.Generator().manual_seed(rows))).to(DEV)
        plain = layers.feed_forward(holder["ff"], holder["norm"], x).clone()
        layers.set_ff_precision(holder, "fp8")
        before = ops.fp8_k64_launch_counts()
        marked = layers.feed_forward(holder["ff"], holder["norm"], x)
        after = ops.fp8_k64_launch_counts()
        assert (after["gemm"] - before["gemm"], after["ln"] - before["ln"]) == want, (C, rows)
        assert torch.equal(marked, plain) == (want == (0, 0))


# ---------------------------------------------------------------------------------------------------------------- 7. SVD
def _emulating_feed_forward(log):
    """layers.feed_forward with both GEMMs emulated on the host from the device's LayerNorm rows (the rounding points of the kernels)"""
    from motionrag_amd import ops

    def lin(a, w):
        (qa, ea), (qw, ew) = quant_ref(a), quant_ref(w)
        return torch.ldexp(qa @ qw.T, -(ea[:, None] + ew[None, :]))

    def feed_forward(ff, norm, x):
        log.append(ff)
        pj, out = ff.net[0].proj, ff.net[2]
        ln = ops.layernorm(x, norm.weight, norm.bias, norm.eps).cpu()
        rows = ln.reshape(-1, ln.shape[-1])
        v, g = (lin(rows, pj.weight.detach().cpu()) + pj.bias.detach().cpu().float()).chunk(2, dim=1)
        h = bf(bf(v).float() * F.gelu(bf(g).float()))
        y = bf(lin(h, out.weight.detach().cpu()) + out.bias.detach().cpu().float()).float() + x.cpu().reshape(rows.shape).float()
        return bf(y).reshape(x.shape).to(x.device)
    return feed_forward


def test_svd_transformer_block_takes_the_fp8_path(hip, monkeypatch):
    """one spatial block of the SVD UNet at its level-0 width C = 320 (FF1 2560 x 320: the half K-tile; FF2 320 x 1280), random weights: counters, and
    bf16 / emulated / fp8 forwards composed through the block as test_svd_resnet_block_takes_the_fp8_path composes the convolutions: E = emulation vs
    bf16, G = kernel path vs bf16, G <= 1.5 E + 0.02; the kernel path against the emulation itself stays within the two GEMMs' bounds, 4e-3 + 8e-3
    (measured: E = 0.0281, G = 0.0281, kernel against emulation 0.0009)."""
    from motionrag_amd import layers, svd_unet
    _open_gates(monkeypatch)
    C = 320
    block = _randomise(svd_unet.BasicTransformerBlock(C, 5, 64, 1024), 21)
    g = torch.Generator().manual_seed(22)
    x = bf(torch.randn(2, 150, C, generator=g)).to(DEV)
    ehs = bf(torch.randn(2, 1, 1024, generator=g)).to(DEV)
    run = lambda: block(x, ehs)
    want = run().clone()
    log = []
    monkeypatch.setattr(svd_unet, "feed_forward", _emulating_feed_forward(log))
    emu = run().clone()
    monkeypatch.setattr(svd_unet, "feed_forward", layers.feed_forward)
    layers.set_ff_precision(block, "fp8")
    run()                                                               # the first fp8 forward also quantises the weights (once)
    before, before_q = _counts()
    got = run()
    after, after_q = _counts()
    assert len(log) == 1
    assert after["gemm"] - before["gemm"] == 2 and after["ln"] - before["ln"] == 1 and after_q["quant"] - before_q["quant"] == 1
    E, G, D = rel_fro(emu, want), rel_fro(got, want), rel_fro(got, emu)
    print(f"svd BasicTransformerBlock C = {C}: E = {E:.4f}, kernel path = {G:.4f}; kernel vs emulation {D:.4f}")
    assert E > 1e-3 and G <= 1.5 * E + 0.02, (G, E)
    assert D <= 4e-3 + 8e-3, D
