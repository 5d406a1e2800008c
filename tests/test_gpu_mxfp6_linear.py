"""The opt-in MXFP6 (OCP e2m3, one E8M0 scale per block of 32 along K) linear path on the GPU: mrag_quant_rows_mxfp6, mrag_dequant_rows_mxfp6,
mrag_gemm_mxfp6 (ops.quant_rows_mxfp6 / ops.dequant_rows_mxfp6 / ops.linear_mxfp6) and cogvideox.set_linear_precision(model, "mxfp6").

References, all computed on the host:
  * the reference quantiser (include/mrag_hip.h states the format): per (row, block of 32) s = the smallest integer with amax * 2^-s <= 7.5, clamped
    to +-60, 0 for a zero block; the element is the nearest of the 32 non-negative e2m3 values to |x| * 2^-s (searchsorted, in float64: exact), a tie
    going to the even code.  torch has no fp6 dtype.  The kernel must reproduce it EXACTLY (dequantised values and scale bytes).
  * exact GEMM: operands drawn from the grid times per-(row, block) powers of two quantise without loss, and their magnitudes are bounded so that
    every partial sum is an exact fp32 number -- K = 256, |a|, |w| <= 7.5 * 2^2: a product is a multiple of 2^-6 below 900 = 56.25 * 16, a sum of 256
    of them stays below 256 * 56.25 * 16 * 64 = 14.7e6 < 2^24 units of 2^-6.  The kernel must return the bits of bf16(float64 product), in any
    summation order.  Three mutants of the reference (one block's scale dropped, the two 32-k halves of every 64-deep step swapped on one side, k
    blocks permuted on one side) must not.
  * the emulation of the GEMM: the fp32 product of the decoded operands, plus bias, then the epilogue with the bf16 GEMM's rounding points.  Bounds as
    derived in tests/test_gpu_fp8_linear.py: one bf16 rounding is at most 2^-8 = 3.9e-3 relative per element and fp32 summation order is at the 1e-6
    level, so NONE / GELU_TANH <= 4e-3 relative Frobenius error; RESID / GATE_RESID round twice: <= 8e-3.
  * un-quantised fp32 A . W^T on the bf16 inputs, self-calibrated: E = the emulation's error against it, G = the kernel's; G <= 1.1 E + 4e-3.
  * model level: the fp32 oracle with F.linear of the blocks' six large weights patched to the reference quantiser gives E_model; the MXFP6 model must
    be within 1.5 E_model + 0.02 of the un-patched fp32 oracle (0.02: the bf16 path's own bound; 1.5: an independent second draw of the same error)."""
import functools
import re
import threading

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPI_NONE, EPI_GELU_TANH, EPI_RESID, EPI_GATE_RESID = 0, 1, 3, 4
EPI_NAMES = {EPI_NONE: "none", EPI_GELU_TANH: "gelu_tanh", EPI_RESID: "resid", EPI_GATE_RESID: "gate_resid"}
BOUND = {EPI_NONE: 4e-3, EPI_GELU_TANH: 4e-3, EPI_RESID: 8e-3, EPI_GATE_RESID: 8e-3}
# the 32 non-negative e2m3 values in code order: 0 .. 0.875 (subnormal), 1 .. 1.875, 2 .. 3.75, 4 .. 7.5
GRID = torch.tensor([m / 8 for m in range(8)] + [(1 + m / 8) * 2 ** e for e in range(3) for m in range(8)], dtype=torch.float64)


def bf(x):
    return x.to(torch.bfloat16)


def rel_fro(got, want):
    g, w = got.float().cpu(), want.float().cpu()
    return ((g - w).norm() / w.norm()).item()


def bits(x):
    return bf(x).cpu().contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------- reference quantiser
def mx_quant_ref(x: torch.Tensor):
    """(the quantised operand decoded, element * 2^s, as fp32 [M, K] -- exact; scale bytes [M, K / 32] uint8) of a matrix of bf16 values"""
    M, K = x.shape
    b = x.double().reshape(M, K // 32, 32)
    amax = b.abs().amax(dim=2)
    mant, ex = torch.frexp(amax)                                       # amax = mant * 2^ex with mant in [0.5, 1); 7.5 = 0.9375 * 2^3
    s = torch.where(mant <= 0.9375, ex - 3, ex - 2).clamp(-60, 60)
    s = torch.where(amax > 0, s, torch.zeros_like(s))
    v = b * torch.exp2(-s.double())[..., None]                         # exact: a power of two
    a = v.abs().clamp(max=7.5).contiguous()
    hi = torch.searchsorted(GRID, a).clamp(max=31)                     # the first grid value >= a
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - GRID[lo], GRID[hi] - a
    code = torch.where((dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0)), hi, lo)   # nearest; a tie to the even code
    q = torch.where(v < 0, -GRID[code], GRID[code])
    q = torch.where(code == 0, torch.zeros_like(q), q)                # a result of zero is +0
    deq = q * torch.exp2(s.double())[..., None]
    return deq.reshape(M, K).float(), (127 + s).to(torch.uint8)


def test_reference_quantiser_on_the_format_s_own_examples():
    """the host reference itself (no device): ties to the even code, the 7.5 boundary, zero blocks"""
    x = torch.zeros(2, 64)
    x[0, :8] = torch.tensor([6.0, 1.0625, -1.0625, 0.0625, 0.1875, 2.125, 2.375, 4.75])
    x[1, :3] = torch.tensor([7.5 * 8, 3.0, -0.5])                      # s = 3: 3.0 -> 0.375, -0.5 -> -0.0625: a tie, to code 0
    x[1, 32:35] = torch.tensor([7.53125 * 8, 8.0, -2.0])               # a bf16 step above: s = 4
    deq, sc = mx_quant_ref(bf(x))
    assert sc.tolist() == [[127, 127], [130, 131]]
    assert deq[0, :8].tolist() == [6.0, 1.0, -1.0, 0.0, 0.25, 2.0, 2.5, 5.0]
    assert deq[1, :3].tolist() == [60.0, 3.0, 0.0] and deq[1, 32:35].tolist() == [60.0, 8.0, -2.0]   # 60.25 / 16 = 3.766 -> 3.75 (the grid's step is 0.25 there)
    assert (deq[0, 8:] == 0).all() and not torch.signbit(deq).logical_and(deq == 0).any()


# ---------------------------------------------------------------------------------------------------------------- 1. the quantiser, exact
TIES = (6.0, 1.0625, -1.0625, 0.0625, -0.0625, 0.1875, 2.125, -2.375, 4.25, 4.75, -7.0, 0.5625, 3.625)   # under s = 0 (6.0 holds the block's scale)


def _quant_input(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    nb = K // 32
    x = torch.randn(M, K, generator=g).reshape(M, nb, 32) * torch.exp2(torch.randint(-12, 13, (M, nb, 1), generator=g).float())   # scales 2^-12 .. 2^12 inside a row
    x = bf(x).float()
    # row 0: block 0 exact ties (times 2^5), block 1 all zero, block 2 a maximum of exactly 7.5 * 2^3, block 3 one bf16 step above it
    x[0, 0] = 0
    x[0, 0, :len(TIES)] = torch.tensor(TIES) * 32
    x[0, 1] = 0
    for blk, top in ((2, 60.0), (3, 60.25)):
        x[0, blk] = bf(torch.randn(32, generator=g).clamp(-3, 3) * 8).float()     # (|.| <= 24 < 60)
        x[0, blk, (7 * blk) % 32] = -top if blk == 2 else top
    if M >= 4:
        x[1] = 0                                                      # an all-zero row
        x[2, nb - 1] = 0                                              # a zero block at the end of a row
        x[3, nb - 1, 31] = 0.0625 * 2.0 ** -7                         # the last element of a row: a tie under its block's scale
        x[3, nb - 1, 0] = 6.0 * 2.0 ** -7
        x[3, nb - 1, 1:31] = 0
    return bf(x.reshape(M, K))


@pytest.mark.parametrize("M,K,strided", [(1, 128, False), (37, 256, False), (37, 256, True), (300, 3072, False), (67, 12288, False)])
def test_quant_rows_mxfp6_is_exact(hip, M, K, strided):
    from motionrag_amd import ops
    x = _quant_input(M, K, seed=M + K)
    if strided:                                                       # a column slice of a wider buffer: ldx > K
        wide = torch.zeros(M, K + 64, dtype=torch.bfloat16, device=DEV)
        wide[:, :K] = x.to(DEV)
        wide[:, K:] = 3e4                                             # must not be seen
        xd = wide[:, :K]
    else:
        xd = x.to(DEV)
    before = ops.mxfp6_launch_counts()
    xq, sc = ops.quant_rows_mxfp6(xd)
    mid = ops.mxfp6_launch_counts()
    assert mid == dict(before, quant=before["quant"] + 1)
    got = ops.dequant_rows_mxfp6(xq, sc)
    assert ops.mxfp6_launch_counts() == dict(mid, dequant=mid["dequant"] + 1)
    assert xq.dtype == torch.uint8 and xq.numel() == (M + 31) // 32 * (K // 64) * 1536
    assert sc.dtype == torch.uint8 and tuple(sc.shape) == (M, K // 32) and got.dtype == torch.bfloat16 and tuple(got.shape) == (M, K)
    deq_ref, sc_ref = mx_quant_ref(x)
    assert torch.equal(sc.cpu(), sc_ref)
    assert sc_ref[0, :4].tolist() == [127 + 5, 127, 127 + 3, 127 + 4]   # 6 * 2^5; the zero block; 60 = 7.5 * 2^3 fits exactly; 60.25 does not
    assert torch.equal(bits(got), bits(deq_ref))
    assert torch.equal(got[0, :len(TIES)].float().cpu(), torch.tensor([6.0, 1.0, -1.0, 0.0, 0.0, 0.25, 2.0, -2.5, 4.0, 5.0, -7.0, 0.5, 3.5]) * 32)
    if M >= 4:
        assert sc_ref.min() < 127 - 8 and sc_ref.max() > 127 + 8      # the row's blocks do span many octaves
        assert (got[1] == 0).all() and (sc_ref[1] == 127).all()


# ---------------------------------------------------------------------------------------------------------------- 2. GEMM, bit for bit
def _exact_operand(R, K, seed):
    """[R, K] fp64: grid values with random signs times a power of two in {1, 2, 4} of each (row, block); every block holds a magnitude of 4 or more, so
    its scale byte is 127 + its exponent; -> (values, exponents [R, K / 32])"""
    g = torch.Generator().manual_seed(seed)
    nb = K // 32
    code = torch.randint(0, 32, (R, nb, 32), generator=g)
    pos = torch.randint(0, 32, (R, nb, 1), generator=g)
    code.scatter_(2, pos, torch.randint(24, 32, (R, nb, 1), generator=g))
    sign = torch.randint(0, 2, (R, nb, 32), generator=g) * 2 - 1
    e = torch.randint(0, 3, (R, nb), generator=g)
    return (GRID[code] * sign * torch.exp2(e.double())[..., None]).reshape(R, K), e


@functools.lru_cache(maxsize=None)
def _exact_problem(M, N, K=256):
    a, ea = _exact_operand(M, K, 11 * M + N)
    w, ew = _exact_operand(N, K, 13 * N + M + 5)
    return a, ea, w, ew, bits(a @ w.T)                                 # bf16(float64 product)


def test_exact_reference_mutants_leave_the_expected_bits():
    """host only: each named mistake changes the expected output, so the exact comparison below would catch it"""
    M, N, K = 257, 272, 256
    a, ea, w, ew, want = _exact_problem(M, N)
    assert (a.abs().max() <= 30) and (w.abs().max() <= 30) and (a.abs() @ w.abs().T).max() * 64 < 2 ** 24      # every partial sum is exact in fp32
    blocks = a.reshape(M, K // 32, 32)
    dropped = blocks.clone()
    r = int((ea[:, 3] > 0).nonzero()[0])
    dropped[r, 3] /= 2.0 ** int(ea[r, 3])                             # one block's scale dropped
    halves = blocks.reshape(M, K // 64, 2, 32).flip(2)                # the lane halves (k 0 .. 31 | 32 .. 63 of a 64-deep step) swapped on one side
    permuted = blocks[:, torch.tensor([1, 2, 3, 4, 5, 6, 7, 0])]      # k blocks permuted on one side
    for name, mut in (("scale dropped", dropped), ("halves swapped", halves), ("blocks permuted", permuted)):
        assert not torch.equal(bits(mut.reshape(M, K) @ w.T), want), name
    assert not torch.equal(bits((a @ w.T).T.contiguous()[:M, :M]), want[:M, :M])                                # a transposed store


@pytest.mark.parametrize("N", [16, 272])
@pytest.mark.parametrize("M", [1, 255, 257, 513])
def test_gemm_mxfp6_is_exact_on_grid_operands(hip, M, N):
    from motionrag_amd import ops
    K = 256
    a, ea, w, ew, want = _exact_problem(M, N)
    ad, wd = bf(a).to(DEV), bf(w).to(DEV)
    aq, a_sc = ops.quant_rows_mxfp6(ad)
    wq, w_sc = ops.quant_rows_mxfp6(wd)
    # quantisation is lossless for these operands, and each block's scale byte is its own exponent
    assert torch.equal(ops.dequant_rows_mxfp6(aq, a_sc), ad) and torch.equal(ops.dequant_rows_mxfp6(wq, w_sc), wd)
    assert torch.equal(a_sc.cpu().int(), 127 + ea.int()) and torch.equal(w_sc.cpu().int(), 127 + ew.int())
    before = ops.mxfp6_launch_counts()
    got = ops.linear_mxfp6(ad, wq, w_sc)
    after = ops.mxfp6_launch_counts()
    assert after["gemm"] == before["gemm"] + 1 and after["quant"] == before["quant"] + 1
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N)
    bad = (bits(got) != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {M * N} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()}, want {(a @ w.T)[tuple(bad[0])].item()}"


# ---------------------------------------------------------------------------------------------------------------- 3. GEMM against the emulation
def _batches(M):
    return next(b for b in (2, 3, 1) if M % b == 0)


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, kind="gaussian"):
    """inputs of one problem and everything the references need, computed once and shared (read-only) by the cases that use it"""
    g = torch.Generator().manual_seed(1000 * M + N + K + len(kind))
    x = torch.randn(M, K, generator=g)
    if kind == "outlier":                                              # 1 % of the channels 30 times larger
        x[:, torch.randperm(K, generator=g)[:max(K // 100, 1)]] *= 30.0
    elif kind == "heavy":                                              # Student-t, 3 degrees of freedom
        x = x / (torch.randn(M, K, 3, generator=g).pow(2).mean(dim=2).sqrt())
    w = torch.randn(N, K, generator=g) * K ** -0.5
    x, w = bf(x), bf(w)
    B = _batches(M)
    rpb = M // B
    split = min(226, max(rpb // 3, 1)) if rpb > 1 else 0
    bias = bf(torch.randn(N, generator=g))
    resid = bf(torch.randn(M, N, generator=g))
    mod = bf(torch.randn(B, 3 * N, generator=g))                       # gates are column slices of a wider modulation row: gate_stride = 3 N
    qa, _ = mx_quant_ref(x)
    qw, _ = mx_quant_ref(w)
    acc = qa @ qw.T                                                    # fp32 product of the decoded operands
    exact = x.float() @ w.float().T                                    # un-quantised fp32 A . W^T on the bf16 inputs
    return dict(x=x, w=w, bias=bias, resid=resid, mod=mod, B=B, rpb=rpb, split=split, acc=acc, exact=exact)


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
    wq, w_sc = ops.quant_rows_mxfp6(p["w"].to(DEV))
    kw = {}
    out = None
    if epi in (EPI_RESID, EPI_GATE_RESID):
        kw["resid"] = p["resid"].to(DEV)
        if alias:
            out = kw["resid"]
    if epi == EPI_GATE_RESID:
        mod = p["mod"].to(DEV)
        kw.update(gate0=mod[:, :N], gate1=mod[:, N:2 * N], rows_per_batch=p["rpb"], split=p["split"], gate_stride=mod.stride(0))
    before = ops.mxfp6_launch_counts()
    got = ops.linear_mxfp6(p["x"].to(DEV), wq, w_sc, p["bias"].to(DEV) if bias else None, out=out, epilogue=epi, **kw)
    after = ops.mxfp6_launch_counts()
    assert after["gemm"] == before["gemm"] + 1 and after["quant"] == before["quant"] + 1      # the activation quantiser + the GEMM
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N)
    if alias:
        assert got.data_ptr() == kw["resid"].data_ptr()
    return got


SHAPES = [(300, 272, 384), (513, 16, 128), (64, 3072, 3072), (520, 1024, 12288)]


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_GELU_TANH, EPI_RESID, EPI_GATE_RESID], ids=lambda e: EPI_NAMES[e])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_mxfp6_matches_emulation(hip, M, N, K, epi):
    p = _problem(M, N, K)
    got = _run(p, epi, M, N)
    assert torch.isfinite(got.float()).all()
    err = rel_fro(got, _emulate(p, epi, M, N))
    print(f"mxfp6 gemm {M}x{N}x{K} {EPI_NAMES[epi]}: rel fro vs emulation {err:.3e} (bound {BOUND[epi]:.0e})")
    assert err <= BOUND[epi], err


def test_gemm_mxfp6_gate_resid_in_place_boundaries(hip):
    """M = 300 = 2 samples of 150 rows, 10 text rows each: the gate boundary (row 10) and the sample boundary (row 150) fall inside 32-row groups
    (rows 0-31 and 128-159); out aliases resid, as the DiT updates its residual stream; the gates are column slices of a wider modulation row"""
    M, N, K = 300, 272, 384
    p = dict(_problem(M, N, K))
    p.update(B=2, rpb=150, split=10)
    got = _run(p, EPI_GATE_RESID, M, N, alias=True)
    want = _emulate(p, EPI_GATE_RESID, M, N)
    assert rel_fro(got, want) <= BOUND[EPI_GATE_RESID]
    for rows in (slice(0, 10), slice(10, 32), slice(128, 150), slice(150, 160), slice(160, 300)):      # every gate segment on its own
        assert rel_fro(got[rows], want[rows]) <= BOUND[EPI_GATE_RESID], rows


def test_gemm_mxfp6_resid_in_place(hip):
    M, N, K = 513, 16, 128
    p = _problem(M, N, K)
    got = _run(p, EPI_RESID, M, N, alias=True)
    assert rel_fro(got, _emulate(p, EPI_RESID, M, N)) <= BOUND[EPI_RESID]


@pytest.mark.parametrize("M,N,K,kind", [(64, 3072, 3072, "gaussian"), (520, 1024, 12288, "gaussian"), (300, 272, 384, "gaussian"), (300, 272, 384, "outlier"),
                                        (300, 272, 384, "heavy")])
def test_gemm_mxfp6_against_fp32_self_calibrated(hip, M, N, K, kind):
    p = _problem(M, N, K, kind)
    E = rel_fro(p["acc"], p["exact"])
    G = rel_fro(_run(p, EPI_NONE, M, N, bias=False), p["exact"])
    print(f"mxfp6 gemm {M}x{N}x{K} {kind} vs fp32: emulation E = {E:.4f}, kernel G = {G:.4f}")
    assert 0.02 < E < 0.08                                              # the quantisation error itself is in e2m3's class (0.040 / 0.052 / 0.045 emulated)
    assert G <= 1.1 * E + 4e-3, (G, E)


def test_linear_mxfp6_refuses_unsupported_shapes(hip):
    from motionrag_amd import ops
    x = torch.zeros(8, 192, dtype=torch.bfloat16, device=DEV)
    wq, w_sc = ops.quant_rows_mxfp6(torch.zeros(32, 192, dtype=torch.bfloat16, device=DEV))      # K % 64 == 0: the quantiser takes it
    before = ops.mxfp6_launch_counts()
    with pytest.raises(ValueError):
        ops.linear_mxfp6(x, wq, w_sc)                                   # K = 192: not whole 128-deep K-tiles
    with pytest.raises(ValueError):
        ops.quant_rows_mxfp6(torch.zeros(8, 96, dtype=torch.bfloat16, device=DEV))
    x = torch.zeros(8, 128, dtype=torch.bfloat16, device=DEV)
    wq, w_sc = ops.quant_rows_mxfp6(torch.zeros(8, 128, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError):
        ops.linear_mxfp6(x, wq, w_sc)                                   # N = 8
    wq, w_sc = ops.quant_rows_mxfp6(torch.zeros(16, 128, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError):
        ops.linear_mxfp6(x, wq, w_sc, epilogue=6)                       # GEGLU does not exist on this GEMM
    assert ops.mxfp6_launch_counts() == dict(before, quant=before["quant"] + 2)


def test_linear_mxfp6_as_hip_graph(hip):
    """two launches, nothing read back: one captured-graph replay equals the eager result bit for bit"""
    from motionrag_amd import ops
    M, N, K = 300, 272, 384
    p = _problem(M, N, K)
    x, bias = p["x"].to(DEV), p["bias"].to(DEV)
    wq, w_sc = ops.quant_rows_mxfp6(p["w"].to(DEV))
    eager = ops.linear_mxfp6(x, wq, w_sc, bias, epilogue=EPI_GELU_TANH).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.HIPGraph() if hasattr(torch.cuda, "HIPGraph") else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.linear_mxfp6(x, wq, w_sc, bias, epilogue=EPI_GELU_TANH)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---------------------------------------------------------------------------------------------------------------- 4. model level
BLOCK_WEIGHT = re.compile(r"transformer_blocks\.\d+\.(attn1\.to_[qkv]|attn1\.to_out\.0|ff\.net\.0\.proj|ff\.net\.2)\.weight$")


def _small_dit(seed=31, layers=2):
    """the two-layer reduced DiT of tests/test_gpu_fp8_linear.py: heads = 2 (D = 128, FF 512), std 0.08, motion adapters installed"""
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


def _forward(model, inp, **kw):
    lat, img, text, ip, t, cos, sin = inp
    return model(lat.to(DEV), text.to(DEV), t.to(DEV), image_rotary_emb=((cos.to(DEV), sin.to(DEV)), ip.to(DEV)), image_latents=img.to(DEV), batch=2, **kw)


@functools.lru_cache(maxsize=None)
def _model_references(model_seed, input_seed, layers):
    """(the fp32 oracle's output, E_model): E_model is the error of the same oracle with F.linear of the six large weights of every block patched to
    quantise the bf16-rounded input and the weight with the reference quantiser"""
    from oracle import cogvideox_ref
    cfg = cogvideox_ref.DiTConfig(num_layers=layers, heads=2, in_channels=16, out_channels=8, time_embed_dim=64, text_embed_dim=64,
                                  max_text_len=10, ip_dim=64, frames=3, height=8, width=12)
    sd = cogvideox_ref.random_dit_sd(cfg, seed=model_seed, std=0.08)
    lat, img, text, ip, t, cos, sin = _dit_inputs(input_seed)
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
        xq = mx_quant_ref(x2)[0].reshape(inp_.shape)
        return plain_linear(xq, mx_quant_ref(weight)[0], bias)

    torch.nn.functional.linear = quantised_linear
    try:
        emu = cogvideox_ref.dit_forward(sdr, cfg, x, text.float(), t, (cos, sin), ip.float())
    finally:
        torch.nn.functional.linear = plain_linear
    assert len(hits) == 6 * layers
    return want, rel_fro(emu, want)


def test_dit_mxfp6_linears_against_oracle(hip):
    from motionrag_amd import cogvideox, ops
    layers = 2
    cfg, sd, model = _small_dit(layers=layers)
    inp = _dit_inputs()
    lat, img, text, ip, t, cos, sin = inp
    never_switched = _forward(model, inp).clone()
    cogvideox.set_linear_precision(model, "fp8")
    fp8_first = _forward(model, inp).clone()                            # the fp8 path before the model ever ran MXFP6

    assert cogvideox.set_linear_precision(model, "mxfp6") is model
    _forward(model, inp)                                                # the first forward also quantises the weights (once)
    before, before8 = ops.mxfp6_launch_counts(), ops.fp8_launch_counts()
    got = _forward(model, inp)
    after = ops.mxfp6_launch_counts()
    assert after["gemm"] - before["gemm"] == 4 * layers and after["quant"] - before["quant"] == 4 * layers and after["dequant"] == before["dequant"]
    assert ops.fp8_launch_counts() == before8                           # nothing of the fp8 path ran
    assert torch.isfinite(got.float()).all()

    want, E_model = _model_references(31, 32, layers)
    G_model = rel_fro(got, want)
    print(f"mxfp6 DiT ({layers} layers): E_model = {E_model:.4f}, kernel path = {G_model:.4f}, bound = {1.5 * E_model + 0.02:.4f}")
    assert 1e-3 < E_model < 0.06                                        # the patch took effect, and the error is in the class of the fp8 path's (0.0145)
    assert G_model <= 1.5 * E_model + 0.02, (G_model, E_model)

    # a subset of the sites: only those launch
    cogvideox.set_linear_precision(model, "mxfp6", sites=("ff1", "ff2"))
    before = ops.mxfp6_launch_counts()
    _forward(model, inp)
    after = ops.mxfp6_launch_counts()
    assert after["gemm"] - before["gemm"] == 2 * layers and after["quant"] - before["quant"] == 2 * layers

    # the fp8 path after the switch: what it was, bit for bit, and no MXFP6 launch
    cogvideox.set_linear_precision(model, "fp8")
    before, before8 = ops.mxfp6_launch_counts(), ops.fp8_launch_counts()
    fp8_again = _forward(model, inp)
    after8 = ops.fp8_launch_counts()
    assert ops.mxfp6_launch_counts() == before
    assert after8["gemm"] - before8["gemm"] == 4 * layers and after8["quant"] - before8["quant"] == 4 * layers
    assert torch.equal(fp8_again, fp8_first)

    # switching back: the bf16 model, bit for bit, and no low-precision launch
    cogvideox.set_linear_precision(model, "bf16")
    before, before8 = ops.mxfp6_launch_counts(), ops.fp8_launch_counts()
    back = _forward(model, inp)
    assert ops.mxfp6_launch_counts() == before and ops.fp8_launch_counts() == before8
    assert torch.equal(back, never_switched)
    assert not torch.equal(got, never_switched) and not torch.equal(got, fp8_first)


def test_dit_mxfp6_weight_update_rebuilds_the_quantised_weight(hip):
    """the quantised weights live in the model's derived-weight cache: an in-place update of a weight is seen by the next forward"""
    from motionrag_amd import cogvideox
    cfg, sd, model = _small_dit(layers=1)
    inp = _dit_inputs()
    cogvideox.set_linear_precision(model, "mxfp6")
    first = _forward(model, inp).clone()
    with torch.no_grad():
        model.transformer_blocks[0].ff.net[2].weight.mul_(0.5)
    assert not torch.equal(_forward(model, inp), first)


def test_dit_mxfp6_sequence_parallel_keeps_qkv_in_bf16(hip):
    """the harness of tests/test_gpu_models.py::test_sequence_parallel_dit_equals_unsharded (two threads with their own streams as two ranks): under
    sequence sharding the QKV projection stays on the bf16 GEMM, so a rank launches three MXFP6 GEMMs per layer, not four.  Each rank is held to the
    model-level bound against the oracle (E_model quantises all four sites: the sharded path quantises three of them)"""
    from motionrag_amd import cogvideox, ops
    from motionrag_amd.dist import SequenceParallel
    layers = 2
    cfg, sd, model = _small_dit(seed=41, layers=layers)
    inp = _dit_inputs(42)
    cogvideox.set_linear_precision(model, "mxfp6")
    _forward(model, inp)                                                # unsharded; builds the fused-weight caches
    want, E_model = _model_references(41, 42, layers)
    torch.cuda.synchronize()
    world = 2
    slots, bar, outs, errs = [None] * world, threading.Barrier(world), [None] * world, []

    def gather_for(rank):
        def ag(x):
            torch.cuda.current_stream().synchronize()
            slots[rank] = x.contiguous()
            bar.wait()
            out = torch.cat(list(slots), dim=0)
            torch.cuda.current_stream().synchronize()
            bar.wait()
            return out
        return ag

    def run(rank):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                outs[rank] = _forward(model, inp, sp=SequenceParallel(rank, world, all_gather=gather_for(rank)))
                torch.cuda.current_stream().synchronize()
        except Exception as e:                                          # surface thread failures in the test
            errs.append(e)
            bar.abort()

    before = ops.mxfp6_launch_counts()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [x.start() for x in th]
    [x.join(timeout=120) for x in th]
    assert not errs, errs
    after = ops.mxfp6_launch_counts()
    assert after["gemm"] - before["gemm"] == world * layers * 3 and after["quant"] - before["quant"] == world * layers * 3
    for r in range(world):
        assert outs[r] is not None and outs[r].shape == want.shape and torch.isfinite(outs[r].float()).all()
        G = rel_fro(outs[r], want)
        print(f"rank {r}: kernel path = {G:.4f}, bound = {1.5 * E_model + 0.02:.4f}")
        assert G <= 1.5 * E_model + 0.02, (r, G, E_model)
