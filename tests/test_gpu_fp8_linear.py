"""The opt-in fp8 (e4m3) linear path on the GPU: mrag_quant_rows_e4m3, mrag_gemm_fp8 (ops.quant_rows_e4m3 / ops.linear_fp8) and
cogvideox.set_linear_precision.

References, all computed on the host:
  * the reference quantiser: per row e = pow2_fit(amax) (the largest e with amax * 2^e <= 448, clamped to +-60, 0 for a zero row), then
    (x.float() * 2^e).to(torch.float8_e4m3fn) -- the emulation style of tests/test_gpu_fp8.py.  The kernel must reproduce it EXACTLY: both sides are
    round-to-nearest-even of exact fp32 products.
  * the emulation of the GEMM: the fp32 product of the decoded operands times 2^-(ea + ew), plus bias, then the epilogue with the bf16 GEMM's
    rounding points.  Bounds: one bf16 rounding is at most 2^-8 = 3.9e-3 relative per element and fp32 summation order is at the 1e-6 level, so
    NONE / GELU_TANH <= 4e-3 relative Frobenius error; RESID / GATE_RESID round twice, each time relative to a quantity no larger in norm than the
    output for these inputs (independent gaussian residual, gate and product): <= 8e-3.
  * un-quantised fp32 A . W^T on the bf16 inputs, self-calibrated: E = the emulation's error against it (0.037-0.038 for gaussian, outlier-channel
    and log-normal inputs at K = 256 .. 12288), G = the kernel's; G <= 1.1 E + 4e-3.  A kernel that drops or misplaces a scale lands orders of
    magnitude away.
  * model level: the fp32 oracle with F.linear of the blocks' six large weights patched to quantise the bf16-rounded input and the weight rows with
    the reference quantiser gives E_model (0.0145 for 2 layers); the fp8 model must be within 1.5 E_model + 0.02 of the un-patched fp32 oracle:
    0.02 is the bf16 path's own bound (test_gpu_models.close), the factor 1.5 covers quantisation decisions that flip because the kernel's
    activations are bf16 where the oracle's are fp32 -- an independent second draw of the same error, sqrt 2."""
import ctypes
import functools
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPI_NONE, EPI_GELU_TANH, EPI_RESID, EPI_GATE_RESID = 0, 1, 3, 4
EPI_NAMES = {EPI_NONE: "none", EPI_GELU_TANH: "gelu_tanh", EPI_RESID: "resid", EPI_GATE_RESID: "gate_resid"}
BOUND = {EPI_NONE: 4e-3, EPI_GELU_TANH: 4e-3, EPI_RESID: 8e-3, EPI_GATE_RESID: 8e-3}


def bf(x):
    return x.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- reference quantiser
def pow2_fit_rows(amax: torch.Tensor) -> torch.Tensor:
    """per row: the largest e with amax * 2^e <= 448 (exact in float64), clamped to +-60, 0 where amax == 0"""
    a = amax.double()
    safe = torch.where(a > 0, a, torch.ones_like(a))
    e = torch.floor(torch.log2(448.0 / safe))
    e = torch.where(torch.ldexp(safe, e.to(torch.int32)) > 448.0, e - 1, e)
    e = torch.where(torch.ldexp(safe, (e + 1).to(torch.int32)) <= 448.0, e + 1, e)
    e = e.clamp(-60, 60)
    return torch.where(a > 0, e, torch.zeros_like(e)).to(torch.int32)


def quant_ref(x: torch.Tensor):
    """(decoded e4m3 values as fp32 [M, K], exp [M] int32) of a bf16 / fp32 matrix"""
    xf = x.float()
    e = pow2_fit_rows(xf.abs().amax(dim=1))
    q = torch.ldexp(xf, e[:, None]).to(torch.float8_e4m3fn).float()
    return q, e


def dequant(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    return torch.ldexp(q, -e[:, None])


def decode(x8: torch.Tensor) -> torch.Tensor:
    return x8.cpu().contiguous().view(torch.float8_e4m3fn).float()


def rel_fro(got, want):
    g, w = got.float().cpu(), want.float().cpu()
    return ((g - w).norm() / w.norm()).item()


# ---------------------------------------------------------------------------------------------------------------- 1. the quantiser, exact
def _quant_input(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-12, 13, (M, 1), generator=g).float())
    x = bf(x)
    if M >= 4:
        x[1] = 0                                                      # an all-zero row
        for r, top in ((2, 56.0), (3, 56.25)):                         # a row whose maximum is exactly 448 * 2^-3, and one a bf16 step above it
            x[r] = bf(torch.randn(K, generator=g).clamp(-3, 3) * 8)    # (|.| <= 24 < 56)
            x[r, (7 * r) % K] = -top if r == 2 else top
    return x


@pytest.mark.parametrize("M,K,strided", [(1, 128, False), (37, 256, False), (37, 256, True), (300, 3072, False), (67, 12288, False)])
def test_quant_rows_is_exact(hip, M, K, strided):
    from motionrag_amd import ops
    x = _quant_input(M, K, seed=M + K)
    if strided:                                                       # a column slice of a wider buffer: ldx > K
        wide = torch.zeros(M, K + 64, dtype=torch.bfloat16, device=DEV)
        wide[:, :K] = x.to(DEV)
        wide[:, K:] = 3e4                                             # must not be seen
        xd = wide[:, :K]
    else:
        xd = x.to(DEV)
    before = ops.fp8_launch_counts()
    x8, ex = ops.quant_rows_e4m3(xd)
    after = ops.fp8_launch_counts()
    assert after["quant"] == before["quant"] + 1 and after["gemm"] == before["gemm"]
    assert x8.dtype == torch.uint8 and tuple(x8.shape) == (M, K) and ex.dtype == torch.int32 and tuple(ex.shape) == (M,)
    q_ref, e_ref = quant_ref(x)
    assert torch.equal(ex.cpu(), e_ref)
    if M >= 4:
        assert e_ref[1] == 0 and e_ref[2] == 3 and e_ref[3] == 2      # 56 * 2^3 = 448 fits exactly; 56.25 does not
    assert torch.equal(decode(x8), q_ref)
    assert decode(x8).abs().max() <= 448.0


# ---------------------------------------------------------------------------------------------------------------- 2. GEMM against the emulation
def _batches(M):
    return next(b for b in (2, 3, 1) if M % b == 0)


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, spread=False):
    """inputs of one problem and everything the references need, computed once and shared (read-only) by the cases that use it"""
    g = torch.Generator().manual_seed(1000 * M + N + K + (7 if spread else 0))
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    if spread:                                                         # row scales over 2^+-12 on A, 2^+-8 on W, one zero row
        sa = torch.randint(-12, 13, (M, 1), generator=g)
        sw = torch.randint(-8, 9, (N, 1), generator=g)
        x, w = torch.ldexp(x, sa), torch.ldexp(w, sw)
        x[M // 2] = 0
        norm = torch.exp2(-(sa.float() + sw.float().T))                # undoes the row / column scales (powers of two: relative errors unchanged)
    else:
        norm = None
    x, w = bf(x), bf(w)
    B = _batches(M)
    rpb = M // B
    split = min(226, max(rpb // 3, 1)) if rpb > 1 else 0
    bias = bf(torch.randn(N, generator=g))
    resid = bf(torch.randn(M, N, generator=g))
    mod = bf(torch.randn(B, 3 * N, generator=g))                       # gates are column slices of a wider modulation row: gate_stride = 3 N
    if spread:                                                         # keep bias / residual on the scale of each output element
        out_scale = torch.exp2(sa.float() + sw.float().T)
        bias = bf(torch.zeros(N))
        resid = bf(resid.float() * out_scale)
    qa, ea = quant_ref(x)
    qw, ew = quant_ref(w)
    acc = torch.ldexp(qa @ qw.T, -(ea[:, None] + ew[None, :]))         # fp32 product of the decoded operands times 2^-(ea + ew)
    exact = x.float() @ w.float().T                                    # un-quantised fp32 A . W^T on the bf16 inputs
    return dict(x=x, w=w, bias=bias, resid=resid, mod=mod, B=B, rpb=rpb, split=split, acc=acc, exact=exact, norm=norm)


def _gate_rows(p, M, N):
    """[M, N] fp32: the gate every row multiplies by (rows with position < split inside their sample take gate0, the others gate1)"""
    pos = torch.arange(M) % p["rpb"]
    b = torch.arange(M) // p["rpb"]
    g0, g1 = p["mod"][:, :N].float(), p["mod"][:, N:2 * N].float()
    return torch.where((pos < p["split"])[:, None], g0[b], g1[b])


def _emulate(p, epi, M, N, bias=True):
    y = p["acc"] + (p["bias"].float() if bias else 0.0)
    if epi == EPI_GELU_TANH:
        return F.gelu(y, approximate="tanh")
    if epi == EPI_RESID:
        return bf(y).float() + p["resid"].float()
    if epi == EPI_GATE_RESID:
        return bf(y * _gate_rows(p, M, N)).float() + p["resid"].float()
    return y


def _run(p, epi, M, N, bias=True, alias=False):
    from motionrag_amd import ops
    w8, w_exp = ops.quant_rows_e4m3(p["w"].to(DEV))
    kw = {}
    out = None
    if epi in (EPI_RESID, EPI_GATE_RESID):
        kw["resid"] = p["resid"].to(DEV)
        if alias:
            out = kw["resid"]
    if epi == EPI_GATE_RESID:
        mod = p["mod"].to(DEV)
        kw.update(gate0=mod[:, :N], gate1=mod[:, N:2 * N], rows_per_batch=p["rpb"], split=p["split"], gate_stride=mod.stride(0))
    before = ops.fp8_launch_counts()
    got = ops.linear_fp8(p["x"].to(DEV), w8, w_exp, p["bias"].to(DEV) if bias else None, out=out, epilogue=epi, **kw)
    after = ops.fp8_launch_counts()
    assert after["gemm"] == before["gemm"] + 1 and after["quant"] == before["quant"] + 1      # the activation quantiser + the GEMM
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N)
    if alias:
        assert got.data_ptr() == kw["resid"].data_ptr()
    return got


SHAPES = [(1, 128, 128), (33, 256, 128), (255, 384, 256), (257, 128, 384), (700, 640, 3072), (130, 256, 12288)]


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_GELU_TANH, EPI_RESID, EPI_GATE_RESID], ids=lambda e: EPI_NAMES[e])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_fp8_matches_emulation(hip, M, N, K, epi):
    p = _problem(M, N, K)
    got = _run(p, epi, M, N)
    assert torch.isfinite(got.float()).all()
    err = rel_fro(got, _emulate(p, epi, M, N))
    print(f"fp8 gemm {M}x{N}x{K} {EPI_NAMES[epi]}: rel fro vs emulation {err:.3e} (bound {BOUND[epi]:.0e})")
    assert err <= BOUND[epi], err


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_GELU_TANH, EPI_RESID, EPI_GATE_RESID], ids=lambda e: EPI_NAMES[e])
def test_gemm_fp8_spread_row_scales(hip, epi):
    """row exponents over 2^+-12 (A) and 2^+-8 (W) and a zero row: the E8M0 scale operands carry every row's own power"""
    M, N, K = 700, 640, 3072
    p = _problem(M, N, K, True)
    got = _run(p, epi, M, N, bias=False)
    want = _emulate(p, epi, M, N, bias=False)
    assert torch.isfinite(got.float()).all()
    err = rel_fro(got, want)
    # the same comparison with every element brought to unit scale: the Frobenius norm above is carried by the largest rows, this one weighs all rows alike
    # (multiplying by powers of two changes no relative error, so the bound is the same)
    err_n = rel_fro(got.float().cpu() * p["norm"], want * p["norm"])
    print(f"fp8 gemm spread scales {EPI_NAMES[epi]}: rel fro {err:.3e}, scale-normalised {err_n:.3e} (bound {BOUND[epi]:.0e})")
    assert err <= BOUND[epi] and err_n <= BOUND[epi], (err, err_n)
    if epi == EPI_NONE:
        assert (got[M // 2].float() == 0).all()                         # the zero row: exponent 0, zero product


def test_gemm_fp8_gate_resid_in_place_boundaries(hip):
    """M = 300 = 2 samples of 150 rows, 10 text rows each: the gate boundary (row 10) and the sample boundary (row 150) fall inside 32-row groups
    (rows 0-31 and 128-159); out aliases resid, as the DiT updates its residual stream"""
    M, N, K = 300, 256, 256
    p = dict(_problem(M, N, K))
    p.update(B=2, rpb=150, split=10)
    got = _run(p, EPI_GATE_RESID, M, N, alias=True)
    want = _emulate(p, EPI_GATE_RESID, M, N)
    assert rel_fro(got, want) <= BOUND[EPI_GATE_RESID]
    for rows in (slice(0, 10), slice(10, 32), slice(128, 150), slice(150, 160), slice(160, 300)):      # every gate segment on its own
        assert rel_fro(got[rows], want[rows]) <= BOUND[EPI_GATE_RESID], rows


# ---------------------------------------------------------------------------------------------------------------- 3. against un-quantised fp32
@pytest.mark.parametrize("M,N,K", [(700, 640, 3072), (130, 256, 12288)])
def test_gemm_fp8_against_fp32_self_calibrated(hip, M, N, K):
    p = _problem(M, N, K)
    E = rel_fro(p["acc"], p["exact"])
    G = rel_fro(_run(p, EPI_NONE, M, N, bias=False), p["exact"])
    print(f"fp8 gemm {M}x{N}x{K} vs fp32: emulation E = {E:.4f}, kernel G = {G:.4f}")
    assert 0.02 < E < 0.06                                              # the quantisation error itself is where it was measured (0.037-0.038)
    assert G <= 1.1 * E + 4e-3, (G, E)


# ---------------------------------------------------------------------------------------------------------------- 4. one production-width shape
def test_gemm_fp8_production_width(hip):
    """(5000, 3072, 3072) with the gated residual epilogue: 240 tiles of 256x256 with a ragged last row tile, 24 K-tiles"""
    M, N, K = 5000, 3072, 3072
    p = _problem(M, N, K)
    got = _run(p, EPI_GATE_RESID, M, N)
    err = rel_fro(got, _emulate(p, EPI_GATE_RESID, M, N))
    print(f"fp8 gemm {M}x{N}x{K} gate_resid: rel fro vs emulation {err:.3e}")
    assert err <= BOUND[EPI_GATE_RESID], err


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_linear_fp8_refuses_unsupported_shapes(hip):
    from motionrag_amd import _lib, ops
    x = torch.zeros(8, 192, dtype=torch.bfloat16, device=DEV)
    w8, w_exp = ops.quant_rows_e4m3(torch.zeros(32, 192, dtype=torch.bfloat16, device=DEV))      # K % 16 == 0: the quantiser takes it
    before = ops.fp8_launch_counts()
    with pytest.raises(ValueError):
        ops.linear_fp8(x, w8, w_exp)                                    # K = 192: not whole 128-deep K-tiles
    with pytest.raises(ValueError):
        ops.quant_rows_e4m3(torch.zeros(8, 72, dtype=torch.bfloat16, device=DEV))
    assert ops.fp8_launch_counts() == before
    hdr_says = lambda N, K: K % 128 == 0 and N % 16 == 0                # include/mrag_hip.h: mrag_gemm_fp8
    for N, K in ((9216, 3072), (3072, 12288), (16, 128), (24, 128), (256, 192), (256, 64), (640, 3072)):
        assert ops.fp8_linear_supported(N, K) == hdr_says(N, K), (N, K)
    # the C entry point says the same for a well-formed call
    a = _lib.GemmFp8Args()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    a.A8 = a.W8 = a.a_exp = a.w_exp = a.C = buf.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = 8, 32, 192, 192, 192, 32
    assert hip.mrag_gemm_fp8(None, ctypes.byref(a)) == _lib.MRAG_ENOTSUP


# ---------------------------------------------------------------------------------------------------------------- 6. model level
BLOCK_WEIGHT = re.compile(r"transformer_blocks\.\d+\.(attn1\.to_[qkv]|attn1\.to_out\.0|ff\.net\.0\.proj|ff\.net\.2)\.weight$")


def _small_dit(seed=31, layers=2):
    """the two-layer reduced DiT of tests/test_gpu_models.py: heads = 2 (D = 128, FF 512), std 0.08, motion adapters installed"""
    from motionrag_amd.cogvideox import CogVideoXTransformer3DModel
    from oracle import cogvideox_ref
    cfg = cogvideox_ref.DiTConfig(num_layers=layers, heads=2, in_channels=16, out_channels=8, time_embed_dim=64, text_embed_dim=64,
                                  max_text_len=10, ip_dim=64, frames=3, height=8, width=12)
    sd = cogvideox_ref.random_dit_sd(cfg, seed=seed, std=0.08)
    model = CogVideoXTransformer3DModel(num_layers=layers, num_attention_heads=2, in_channels=16, out_channels=8, time_embed_dim=64,
                                        text_embed_dim=64, max_text_seq_length=10, sample_frames=3, sample_height=8, sample_width=12)
    model.install_motion_adapters(64)
    model.load_state_dict(sd, strict=True)
    return cfg, sd, model.to(DEV, torch.bfloat16)


def _dit_inputs(seed=32):
    from oracle import cogvideox_ref
    g = torch.Generator().manual_seed(seed)
    lat, img = (bf(torch.randn(1, 3, 8, 8, 12, generator=g)) for _ in range(2))
    text = bf(torch.randn(2, 10, 64, generator=g))
    ip = bf(torch.randn(2, 25, 64, generator=g))
    t = torch.tensor([481.0, 481.0])
    cos, sin = cogvideox_ref.rope_3d(64, 3, 4, 6)
    return lat, img, text, ip, t, cos, sin


def _forward(model, inp):
    lat, img, text, ip, t, cos, sin = inp
    return model(lat.to(DEV), text.to(DEV), t.to(DEV), image_rotary_emb=((cos.to(DEV), sin.to(DEV)), ip.to(DEV)), image_latents=img.to(DEV), batch=2)


def test_dit_fp8_linears_against_oracle(hip, monkeypatch):
    from motionrag_amd import cogvideox, ops
    from oracle import cogvideox_ref
    layers = 2
    cfg, sd, model = _small_dit(layers=layers)
    inp = _dit_inputs()
    lat, img, text, ip, t, cos, sin = inp
    never_switched = _forward(model, inp).clone()

    cogvideox.set_linear_precision(model, "fp8")
    _forward(model, inp)                                                # the first fp8 forward also quantises the weights (once)
    before = ops.fp8_launch_counts()
    got = _forward(model, inp)
    after = ops.fp8_launch_counts()
    assert after["gemm"] - before["gemm"] == 4 * layers and after["quant"] - before["quant"] == 4 * layers
    assert torch.isfinite(got.float()).all()

    # the fp32 oracle, and the same oracle with the six large weights of every block on reference-quantised operands
    sdr = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    x = torch.cat([torch.cat([lat] * 2), torch.cat([img] * 2)], dim=2).float()
    want = cogvideox_ref.dit_forward(sdr, cfg, x, text.float(), t, (cos, sin), ip.float())
    patched_ids = {id(v) for k, v in sdr.items() if BLOCK_WEIGHT.search(k)}
    assert len(patched_ids) == 6 * layers
    plain_linear = F.linear
    hits = []

    def quantised_linear(inp_, weight, bias=None):
        if id(weight) not in patched_ids:
            return plain_linear(inp_, weight, bias)
        hits.append(id(weight))
        x2 = bf(inp_.reshape(-1, inp_.shape[-1]))                       # the kernel's activations are bf16
        xq = dequant(*quant_ref(x2)).reshape(inp_.shape)
        wq = dequant(*quant_ref(weight))
        return plain_linear(xq, wq, bias)

    monkeypatch.setattr(torch.nn.functional, "linear", quantised_linear)
    emu = cogvideox_ref.dit_forward(sdr, cfg, x, text.float(), t, (cos, sin), ip.float())
    monkeypatch.undo()
    assert len(hits) == 6 * layers
    E_model = rel_fro(emu, want)
    G_model = rel_fro(got, want)
    print(f"fp8 DiT ({layers} layers): E_model = {E_model:.4f}, kernel path = {G_model:.4f}, bound = {1.5 * E_model + 0.02:.4f}")
    assert 0.005 < E_model < 0.03                                       # (0.0145 measured for 2 layers)
    assert G_model <= 1.5 * E_model + 0.02, (G_model, E_model)

    # a subset of the sites: only those launch
    cogvideox.set_linear_precision(model, "fp8", sites=("ff1", "ff2"))
    before = ops.fp8_launch_counts()
    _forward(model, inp)
    after = ops.fp8_launch_counts()
    assert after["gemm"] - before["gemm"] == 2 * layers and after["quant"] - before["quant"] == 2 * layers

    # switching back: the bf16 model, bit for bit, and no fp8 launch
    cogvideox.set_linear_precision(model, "bf16")
    before = ops.fp8_launch_counts()
    back = _forward(model, inp)
    assert ops.fp8_launch_counts() == before
    assert torch.equal(back, never_switched)
    assert not torch.equal(got, never_switched)


# ---------------------------------------------------------------------------------------------------------------- 7. graph capture
def test_dit_fp8_forward_as_hip_graph(hip):
    """no host synchronisation and nothing read back on the fp8 path: the one-layer model's forward captures (a straight-line graph) and the replay
    equals the eager result bit for bit"""
    from motionrag_amd import cogvideox
    cfg, sd, model = _small_dit(layers=1)
    cogvideox.set_linear_precision(model, "fp8")
    lat, img, text, ip, t, cos, sin = _dit_inputs()
    args = (lat.to(DEV), text.to(DEV), t.to(DEV))
    kw = dict(image_rotary_emb=((cos.to(DEV), sin.to(DEV)), ip.to(DEV)), image_latents=img.to(DEV), batch=2)
    eager = model(*args, **kw).clone()                                  # warm: weights quantised, fused-weight caches and workspaces built
    graph = torch.cuda.HIPGraph() if hasattr(torch.cuda, "HIPGraph") else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model(*args, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
