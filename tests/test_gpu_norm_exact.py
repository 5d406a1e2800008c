"""LayerNorm and GroupNorm statistics element by element: every kernel and template instantiation behind ops.layernorm / linear_ln / layernorm_e4m3 /
qknorm_rope_ / qkv_linear_qknorm_rope / groupnorm / groupnorm_partial + groupnorm_apply_stats, on inputs whose statistics are known exactly (norm_exact.py;
that the checks can fail is proven on the host in test_norm_exact_cpu.py).

Family A (one spike per row / (sample, group); integer sums; gamma +- powers of two) is judged at |got - want| <= (2^-8 + 2^-14) |want| against the fp64
normalisation, every element counted.  Family B (mean 8 and 32 standard deviations from zero, random gamma / beta / emb) at 2^-8 |want| + c |gamma x^| +
2^-16 |gamma mean rstd| with c = 2^-11 for the two-pass LayerNorms and 2^-9 for the one-pass GroupNorm; at 128 standard deviations GroupNorm is held to
norm_exact.C_GN_128, four times what was measured.  Every launch goes through ops.* inside ops.dispatched() and the launch counters are
asserted, so a case cannot land on another kernel.

Each check prints `NORM-EXACT <case> <worst error as a fraction of its bound>` (pytest -s shows it)."""
import ctypes

import pytest
import torch

import norm_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dv(t):
    """a host fp32 tensor of bf16 values -> bf16 on the device"""
    return None if t is None else X.bf(t).to(DEV)


def d64(t):
    return None if t is None else t.to(DEV)


def report(what, w):
    print(f"NORM-EXACT {what} {w:.3g}")
    return X.check(w, what)


# ---------------------------------------------------------------------------------------------- LayerNorm
def ln_launch(x, gamma, beta, counts, what, *, eps=X.EPS, rms=False, mod=None, rpb=0, split=0, strided=False, batched=None):
    """one ops.layernorm launch on host inputs -> the result [rows, D] on the device.  mod [B, 4, D]; strided: column slices of wider buffers in and out, whose
    other columns must stay zero; batched = (B, L, pad): x as [B, L, D] into a [B, L + pad, D] buffer behind `pad` rows that must stay zero"""
    from motionrag_amd import ops
    rows, D = x.shape
    xd, kw = dv(x), {}
    if mod is not None:
        md = dv(mod)
        kw = dict(shift0=md[:, 0], scale0=md[:, 1], shift1=md[:, 2], scale1=md[:, 3], rows_per_batch=rpb, split=split, mod_stride=md.stride(0))
    if rms:
        kw["rms"] = True
    if strided:
        wide_in, wide_out = torch.zeros(rows, D + 64, dtype=torch.bfloat16, device=DEV), torch.zeros(rows, D + 128, dtype=torch.bfloat16, device=DEV)
        wide_in[:, 8:8 + D] = xd
        xd, kw["out"] = wide_in[:, 8:8 + D], wide_out[:, 64:64 + D]
    if batched is not None:
        B, L, pad = batched
        buf = torch.zeros(B, L + pad, D, dtype=torch.bfloat16, device=DEV)
        xd, kw["out_batched"] = xd.view(B, L, D), buf[:, pad:]
    with ops.dispatched() as d:
        got = ops.layernorm(xd, dv(gamma), dv(beta), eps, **kw)
    assert d.counts == counts, (what, d.counts)
    if strided:
        assert wide_out[:, :64].abs().max().item() == 0 and wide_out[:, 64 + D:].abs().max().item() == 0, f"{what}: a column outside the result was written"
    if batched is not None:
        assert buf[:, :pad].abs().max().item() == 0, f"{what}: a row outside the result was written"
    return got.reshape(rows, D)


def ln_both_families(rows, D, counts, what, *, rms=False, adaln=None, **kw):
    """families A and B, affine and None / None.  adaln = (B, rows_per_batch, split)"""
    x, g = X.ln_family_a(rows, D), X.gamma_pattern(D)
    mod_a = mod_b = rows_a = rows_b = None
    if adaln is not None:
        B, rpb, split = adaln
        mod_a = X.adaln_pow2(B, D)
        mod_b = X.bf(0.3 * torch.randn(B, 4, D, generator=torch.Generator().manual_seed(D))).float()
        rows_a, rows_b = (tuple(d64(t) for t in X.adaln_rows(rows, rpb, split, m)) for m in (mod_a, mod_b))
        kw.update(rpb=rpb, split=split)
    for gamma in (g, None):
        want, lin, _ = X.ln_ref64(d64(x), d64(gamma), None, rms=rms, mod=rows_a)
        if adaln is not None:
            assert (want.abs() / lin).min().item() >= 2.0 ** -6
        got = ln_launch(x, gamma, None, counts, what, rms=rms, mod=mod_a, **kw)
        report(f"A {what}{'' if gamma is not None else ' no-affine'}", X.worst_a(got, want))
    xb, gb, bb = X.ln_family_b(rows, D)
    for gamma, beta in ((gb, bb), (None, None)):
        want, lin, off = X.ln_ref64(d64(xb), d64(gamma), d64(beta), rms=rms, mod=rows_b)
        got = ln_launch(xb, gamma, beta, counts, what, rms=rms, mod=mod_b, **kw)
        report(f"B {what}{'' if gamma is not None else ' no-affine'}", X.worst_b(got, want, lin, off, X.C_LN))


@pytest.mark.parametrize("D", [D for Ds in X.LN_DIMS.values() for D in Ds])
def test_layernorm_kernel(hip, D):
    """layernorm_kernel<2 / 4 / 6 / 8 / 16> at both ends of each instantiation's range (8 and 64: idle lanes; x032 / x056 / x080 / x104: one vector into the
    last register set; the upper ends: every lane busy).  rows = max(D / 8, 9): every 8-vector of the row is probed, the last workgroup is ragged.  The upper
    end of each range again through column slices of wider buffers"""
    maxc = next(m for m, Ds in X.LN_DIMS.items() if D in Ds)
    ln_both_families(X.ln_rows(D), D, {"LAYERNORM": 1}, f"layernorm<{maxc}> D={D}")
    if D == X.LN_DIMS[maxc][-1]:
        ln_both_families(X.ln_rows(D), D, {"LAYERNORM": 1}, f"layernorm<{maxc}> D={D} strided", strided=True)


@pytest.mark.parametrize("D", [512, 4096])
def test_rmsnorm(hip, D):
    """the RMS form: no mean, variance = mean(x^2); want is the fp64 RMSNorm"""
    ln_both_families(X.ln_rows(D), D, {"LAYERNORM": 1}, f"rmsnorm D={D}", rms=True)


def test_adaln_modulation(hip):
    """131 rows in samples of 65 with the text / video split at 37: sample and segment boundaries inside a 4-row workgroup"""
    ln_both_families(131, 1024, {"LAYERNORM": 1}, "adaln D=1024", adaln=(3, 65, 37))


@pytest.mark.parametrize("D", X.LN_ROWS_DIMS)
def test_layernorm_rows_kernel(hip, D):
    """layernorm_rows_kernel<8, 5> / <16, 5> / <32, 5> / <16, 8>: 8 / 4 / 2 / 4 rows per wave, 1 029 rows (a ragged last wave whose spare lanes re-read the last
    row); D = 1 024 again through the output row remap of a concat buffer, D = 640 through column slices"""
    rows = X.LN_ROWS_ROWS
    ln_both_families(rows, D, {"LAYERNORM_ROWS": 1}, f"layernorm_rows D={D}")
    if D == 1024:
        ln_both_families(rows, D, {"LAYERNORM_ROWS": 1}, f"layernorm_rows D={D} out_batched", batched=(3, rows // 3, 5))
    if D == 640:
        ln_both_families(rows, D, {"LAYERNORM_ROWS": 1}, f"layernorm_rows D={D} strided", strided=True)


def test_layernorm_stream_kernel(hip):
    """layernorm_stream_kernel<6>: 8 197 rows over 2 048 persistent waves -- five waves take a fifth row -- unmodulated, modulated with samples of 4 100 rows split
    at 37 (a wave's rows are 2 048 apart: it crosses a boundary at every step), and through column slices"""
    rows, D = X.LN_STREAM
    ln_both_families(rows, D, {"LAYERNORM_STREAM": 1}, "layernorm_stream")
    ln_both_families(rows, D, {"LAYERNORM_STREAM": 1}, "layernorm_stream adaln", adaln=(2, 4100, 37))
    x, g = X.ln_family_a(rows, D), X.gamma_pattern(D)
    got = ln_launch(x, g, None, {"LAYERNORM_STREAM": 1}, "layernorm_stream strided", strided=True)
    report("A layernorm_stream strided", X.worst_a(got, X.ln_ref64(d64(x), d64(g))[0]))


# ---------------------------------------------------------------------------------------------- fused forms of the same arithmetic
@pytest.mark.parametrize("M", [16, 250])
def test_linear_ln(hip, M):
    """LayerNorm in the few-row GEMM's A load: the bits of linear(layernorm(x)) on both families, and with an identity weight (N = K: every product but one is
    an exact zero) the family A bound itself"""
    from motionrag_amd import ops
    K = 1024
    g = X.gamma_pattern(K)
    xa = X.ln_family_a(M, K)
    xb, gb, bb = X.ln_family_b(M, K)
    eye = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    w = X.bf(torch.randn(1024, K, generator=torch.Generator().manual_seed(M)) * K ** -0.5).to(DEV)
    for name, x, gamma, beta in (("A", xa, g, None), ("A no-affine", xa, None, None), ("B", xb, gb, bb)):
        for wt in (eye, w):
            with ops.dispatched() as d:
                got = ops.linear_ln(dv(x), dv(gamma), dv(beta), X.EPS, wt)
            assert d.counts == {"GEMM_SKINNY_LNA": 1}, d.counts
            assert torch.equal(got, ops.linear(ops.layernorm(dv(x), dv(gamma), dv(beta), X.EPS), wt)), (name, tuple(wt.shape))
        if name != "B":
            got = ops.linear_ln(dv(x), dv(gamma), None, X.EPS, eye)
            report(f"A linear_ln M={M}{name[1:]}", X.worst_a(got, X.ln_ref64(d64(x), d64(gamma))[0]))


@pytest.mark.parametrize("rows,D", [(40, 320), (1029, 320), (1029, 640), (1029, 1280), (1029, 1024), (128, 1024), (9, 64), (256, 2048), (131, 1040)])
def test_layernorm_e4m3(hip, rows, D):
    """one pass over x must give the bits of quant_rows_e4m3(layernorm(x)): layernorm_kernel<2, Q8> (D <= 1 024), <4, Q8> (1 040 and 2 048) and the four
    narrow-row instantiations from 1 024 rows up, on both families"""
    from motionrag_amd import ops
    g = X.gamma_pattern(D)
    xb, gb, bb = X.ln_family_b(rows, D)
    for name, x, gamma, beta in (("A", X.ln_family_a(rows, D), g, None), ("A no-affine", X.ln_family_a(rows, D), None, None), ("B", xb, gb, bb)):
        before = ops.fp8_k64_launch_counts()["ln"]
        with ops.dispatched() as d:
            x8, ex = ops.layernorm_e4m3(dv(x), dv(gamma), dv(beta), X.EPS)
        assert d.counts == {} and ops.fp8_k64_launch_counts()["ln"] == before + 1, (name, d.counts)           # the one-pass kernel itself, not the two launches
        x8, ex = x8.clone(), ex.clone()
        with ops.dispatched() as d:
            ln = ops.layernorm(dv(x), dv(gamma), dv(beta), X.EPS)
        assert d.counts == ({"LAYERNORM_ROWS": 1} if rows >= 1024 and D in X.LN_ROWS_DIMS else {"LAYERNORM": 1}), d.counts
        w8, wex = ops.quant_rows_e4m3(ln)
        assert torch.equal(x8, w8) and torch.equal(ex, wex), (name, rows, D)


def head_rows(B, S, H, family):
    """[B, S, 3, H, 64] fp32: every 64-wide head row of Q, K and V is a unit of its own"""
    rows = B * S * 3 * H
    if family == "A":
        return X.ln_family_a(rows, 64, amp=16).view(B, S, 3, H, 64)
    return X.ln_family_b(rows, 64)[0].view(B, S, 3, H, 64)


def qk_params(family):
    """q_gamma, q_beta, k_gamma, k_beta [64] fp32"""
    if family == "A":
        return X.gamma_pattern(64), None, X.gamma_pattern(64).roll(3), None
    g = torch.Generator().manual_seed(64)
    return tuple(X.bf(torch.randn(64, generator=g)).float() for _ in range(4))


def check_heads(got, x, family, what):
    """got [B, S, 3, H, 64] on the device against the fp64 LayerNorm of every Q and K head row; V as it was"""
    B, S, _, H, _ = x.shape
    qg, qb, kg, kb = qk_params(family)
    for which, (gm, bt) in enumerate(((qg, qb), (kg, kb))):
        want, lin, off = X.ln_ref64(d64(x[:, :, which].reshape(-1, 64)), d64(gm), d64(bt), eps=1e-6)
        g2 = got[:, :, which].reshape(-1, 64)
        report(f"{family} {what} {'QK'[which]}", X.worst_a(g2, want) if family == "A" else X.worst_b(g2, want, lin, off, X.C_LN))
    assert torch.equal(got[:, :, 2], dv(x[:, :, 2])), f"{what}: V changed"


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("H", [3, 8, 12])
def test_qknorm_rope(hip, H, family):
    """qknorm_rope_kernel without RoPE and Q pre-multiplication: eight heads per wave (H = 3: five idle head slots; 12: a ragged second head group), A = 16"""
    from motionrag_amd import ops
    B, S = 2, 37
    x = head_rows(B, S, H, family)
    with ops.dispatched() as d:
        got = ops.qknorm_rope_(dv(x).view(B, S, 3 * H * 64).clone(), H, *(dv(t) for t in qk_params(family)), None, None, 0, eps=1e-6, q_premul=1.0)
    assert d.counts == {"QKNORM_ROPE": 1}, d.counts
    check_heads(got.view(B, S, 3, H, 64), x, family, f"qknorm_rope H={H}")


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("H,K,S", [(8, 128, 4100), (8, 320, 4100), (12, 320, 2900)])
def test_qkv_linear_qknorm_rope(hip, H, K, S, family):
    """the same head rows through the fused QKV projection's epilogue.  The projection is exact by construction: row r of x is one-hot at column r mod K and
    column k of W holds the wanted Q | K | V row k, so every accumulator is one bf16 value plus zeros; cos = 1, sin = 0.  K = 320: the four-wave persistent
    kernel and, with GEMM_TUNE_NO_W4, the eight-wave tile -- both within the bound and bit-equal; K = 128 is below the four-wave kernel's 320: the eight-wave
    tile alone"""
    from motionrag_amd import ops
    B = 2
    rows = head_rows(1, K, H, family)[0]                                           # [K, 3, H, 64]: the K wanted rows
    w = dv(rows.reshape(K, 3 * H * 64).t().contiguous())                           # [3 H 64, K]
    r = torch.arange(B * S)
    xd = torch.zeros(B * S, K, dtype=torch.bfloat16, device=DEV)
    xd[r, r % K] = 1.0
    cos, sin = torch.ones(S, 64, device=DEV), torch.zeros(S, 64, device=DEV)
    params = tuple(dv(t) for t in qk_params(family))
    outs = {}
    for name, tuning, counts in (("eight", ops.GEMM_TUNE_NO_W4, {"GEMM_256x256": 1}), ("four", 0, {"GEMM_W4_QKNORM_ROPE": 1} if K >= 320 else {"GEMM_256x256": 1})):
        ops.TUNING["gemm"] = tuning
        try:
            with ops.dispatched() as d:
                outs[name] = ops.qkv_linear_qknorm_rope(xd.view(B, S, K), w, None, H, *params, cos, sin, 0, eps=1e-6, q_premul=1.0)
        finally:
            ops.TUNING["gemm"] = 0
        assert d.counts == counts, (name, d.counts)
        want_rows = rows[r % K].view(B, S, 3, H, 64)
        check_heads(outs[name].view(B, S, 3, H, 64), want_rows, family, f"qkv_linear {name} H={H} K={K} {'+'.join(counts)}")
    assert torch.equal(outs["four"], outs["eight"])


@pytest.mark.parametrize("family", ["A", "B"])
def test_qkv_linear_three_heads(hip, family):
    """H = 3 (192 columns per third) fits neither fused epilogue -- the four-wave kernel wants whole 128-column wave tiles inside a third, the eight-wave epilogue
    its 256 x 256 tile, and 576 columns go to other tiles -- so the entry point runs the plain GEMM and qknorm_rope_kernel: the same head rows, the same bound"""
    from motionrag_amd import ops
    B, S, H, K = 2, 150, 3, 128
    rows = head_rows(1, K, H, family)[0]
    w = dv(rows.reshape(K, 3 * H * 64).t().contiguous())
    r = torch.arange(B * S)
    xd = torch.zeros(B * S, K, dtype=torch.bfloat16, device=DEV)
    xd[r, r % K] = 1.0
    cos, sin = torch.ones(S, 64, device=DEV), torch.zeros(S, 64, device=DEV)
    with ops.dispatched() as d:
        got = ops.qkv_linear_qknorm_rope(xd.view(B, S, K), w, None, H, *(dv(t) for t in qk_params(family)), cos, sin, 0, eps=1e-6, q_premul=1.0)
    assert d.counts == {"GEMM_128x128": 1, "QKNORM_ROPE": 1}, d.counts
    check_heads(got.view(B, S, 3, H, 64), rows[r % K].view(B, S, 3, H, 64), family, "qkv_linear two kernels H=3 K=128")


# ---------------------------------------------------------------------------------------------- GroupNorm
GN_COUNTS = {"GN_STATS": 1, "GN_FOLD": 1, "GN_APPLY": 1}
_GN_A, _GN_B = {}, {}


def gn_case_a(shape, chunks, silu, emb, affine=True):
    """family A inputs on the host and their fp64 result on the device (computed once per case, never written to)"""
    key = (shape, chunks, silu, emb, affine)
    if key not in _GN_A:
        N, HW, C, G = shape
        g = X.gamma_pattern(C) if affine else None
        x, _ = X.gn_family_a(N, HW, C, G, chunks=chunks, silu=silu, gamma=g)
        e = X.gn_emb_a(N, C) if emb else None
        _GN_A[key] = (x, g, e, X.gn_ref64(d64(x), G, d64(g), None, emb=d64(e), silu=silu)[0])
    return _GN_A[key]


def gn_case_b(shape, silu, emb, ratio=None):
    key = (shape, silu, emb, ratio)
    if key not in _GN_B:
        N, HW, C, G = shape
        x, g, b, e = X.gn_family_b(N, HW, C, G, emb=emb, ratio=ratio)
        _GN_B[key] = (x, g, b, e) + X.gn_ref64(d64(x), G, d64(g), d64(b), emb=d64(e), silu=silu)
    return _GN_B[key]


@pytest.mark.parametrize("emb", [False, True], ids=["", "emb"])
@pytest.mark.parametrize("silu", [False, True], ids=["", "silu"])
@pytest.mark.parametrize("shape", X.GN_SHAPES, ids=lambda s: "x".join(str(i) for i in s[:3]))
def test_groupnorm(hip, shape, silu, emb):
    """(4, 600, 320): 18 chunks of 34 pixels and a last one of 22, C / 8 = 40 (16 idle threads, a channel-vector step that does not divide 256), 128 probes;
    (2, 2 304, 64): two channels per group, 32 rows per pass, 72 chunks; (1, 40, 2 560): one chunk, two channel segments, group 25 across channel 2 048;
    (5, 1 000, 64): 31 chunks of 33 pixels and a last one of ten"""
    from motionrag_amd import ops
    N, HW, C, G = shape
    chunks = X.gn_chunks(N, HW)
    assert ops._gn_chunks(N, HW) == chunks
    what = f"groupnorm {N}x{HW}x{C}{' silu' if silu else ''}{' emb' if emb else ''}"
    for affine in (True, False):
        x, g, e, want = gn_case_a(shape, chunks, silu, emb, affine)
        with ops.dispatched() as d:
            got = ops.groupnorm(dv(x), dv(g), None, G, X.EPS, silu=silu, emb=dv(e))
        assert d.counts == GN_COUNTS, d.counts
        report(f"A {what}{'' if affine else ' no-affine'}", X.worst_a(got, want))
    x, g, b, e, want, lin, off = gn_case_b(shape, silu, emb)
    with ops.dispatched() as d:
        got = ops.groupnorm(dv(x), dv(g), dv(b), G, X.EPS, silu=silu, emb=dv(e))
    assert d.counts == GN_COUNTS, d.counts
    report(f"B {what}", X.worst_b(got, want, lin, off, X.C_GN))


@pytest.mark.parametrize("chunks", [64, 1])
def test_groupnorm_c_abi_chunks(hip, chunks):
    """mrag_groupnorm_bf16 with the chunk count set here: 64 chunks over 100 pixels are 50 of two pixels and 14 empty ones, whose partials must be zeros although the
    workspace held 0x7f bytes (3.4e38 as fp32) before the call; one chunk sums all 100 pixels in one workgroup"""
    from motionrag_amd import _lib, ops
    N, HW, C, G = X.GN_RAW
    L = _lib.lib()
    need = L.mrag_groupnorm_workspace_bytes(N, C, chunks)
    for family in ("A", "B"):
        if family == "A":
            x, g, _, want = gn_case_a(X.GN_RAW, chunks, True, False)
            b = None
        else:
            x, g, b, _, want, lin, off = gn_case_b(X.GN_RAW, True, False)
        ws = torch.full((need,), 0x7f, dtype=torch.uint8, device=DEV)
        ws[:16384] = 0                                                              # the arrival counters in front are zero between calls
        xd, gd, bd = dv(x), dv(g), dv(b)
        out = torch.empty_like(xd)
        a = _lib.GroupNormArgs()
        a.x, a.y, a.gamma, a.beta, a.workspace = xd.data_ptr(), out.data_ptr(), gd.data_ptr(), bd.data_ptr() if bd is not None else None, ws.data_ptr()
        a.N, a.HW, a.C, a.G, a.chunks, a.silu, a.eps = N, HW, C, G, chunks, 1, X.EPS
        with ops.dispatched() as d:
            rc = L.mrag_groupnorm_bf16(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a))
        assert rc == _lib.MRAG_OK and d.counts == GN_COUNTS, (rc, d.counts)
        report(f"{family} groupnorm C-ABI chunks={chunks}", X.worst_a(out, want) if family == "A" else X.worst_b(out, want, lin, off, X.C_GN))


@pytest.mark.parametrize("shape", X.GN_SHAPES[:2], ids=lambda s: "x".join(str(i) for i in s[:3]))
def test_groupnorm_fold_by_last_arriver(hip, shape):
    """gn_stats_kernel<true>: the sample's last statistics workgroup folds the partials itself, per channel over the chunks in index order where the fold
    kernel sums k-slices.  Family A's sums are exact in any order: the two forms must agree bit for bit there; on family B both meet the bound"""
    from motionrag_amd import ops
    N, HW, C, G = shape
    chunks = X.gn_chunks(N, HW)
    for emb in (False, True):
        x, g, e, want = gn_case_a(shape, chunks, True, emb)
        with ops.dispatched() as d:
            got = ops.groupnorm(dv(x), dv(g), None, G, X.EPS, silu=True, emb=dv(e), fold=True)
        assert d.counts == {"GN_STATS_FOLD": 1, "GN_APPLY": 1}, d.counts
        report(f"A groupnorm fold {N}x{HW}x{C}{' emb' if emb else ''}", X.worst_a(got, want))
        assert torch.equal(got, ops.groupnorm(dv(x), dv(g), None, G, X.EPS, silu=True, emb=dv(e)))
        x, g, b, e, want, lin, off = gn_case_b(shape, True, emb)
        with ops.dispatched() as d:
            got = ops.groupnorm(dv(x), dv(g), dv(b), G, X.EPS, silu=True, emb=dv(e), fold=True)
        assert d.counts == {"GN_STATS_FOLD": 1, "GN_APPLY": 1}, d.counts
        report(f"B groupnorm fold {N}x{HW}x{C}{' emb' if emb else ''}", X.worst_b(got, want, lin, off, X.C_GN))


@pytest.mark.parametrize("family", ["A", "B"])
def test_groupnorm_sharded(hip, family):
    """three shards of 256 / 200 / 144 pixels (8 / 6 / 4 chunks of their own) with hw_total = 600: the statistics of the whole extent, probes in every shard,
    judged against the fp64 norm of the whole extent"""
    from motionrag_amd import ops
    N, sizes, C, G = X.GN_SPLIT
    HW = sum(sizes)
    if family == "A":
        g, b = X.gamma_pattern(C), None
        x, _ = X.gn_family_a(N, HW, C, G, pixels=X.split_probe_pixels(sizes, C, N), silu=True, gamma=g)
    else:
        x, g, b, _ = X.gn_family_b(N, HW, C, G)
    want, lin, off = X.gn_ref64(d64(x), G, d64(g), d64(b), silu=True)
    shards = [s.contiguous() for s in torch.split(dv(x), list(sizes), dim=1)]
    with ops.dispatched() as d:
        partials = torch.stack([ops.groupnorm_partial(s, G) for s in shards])
    assert d.counts == {"GN_STATS": 3, "GN_FOLD": 3}, d.counts
    with ops.dispatched() as d:
        got = torch.cat([ops.groupnorm_apply_stats(s, partials, HW, dv(g), dv(b), G, X.EPS, silu=True) for s in shards], dim=1)
    assert d.counts == {"GN_FOLD": 3, "GN_APPLY": 3}, d.counts
    report(f"{family} groupnorm sharded", X.worst_a(got, want) if family == "A" else X.worst_b(got, want, lin, off, X.C_GN))
    if family == "A":                                                               # the partials are the shards' exact integer sums
        xs = torch.split(x.double().view(N, HW, G, C // G), list(sizes), dim=1)
        ref = torch.stack([torch.stack([s.sum((1, 3)), (s * s).sum((1, 3))], dim=-1) for s in xs])
        assert torch.equal(partials.double().cpu(), ref)


@pytest.mark.parametrize("case", X.GN_MOD, ids=lambda c: "x".join(str(i) for i in c[1]) + f"-C{c[2]}")
def test_groupnorm_mod_form(hip, case):
    """gn_apply_mod_kernel: the latent-resolution maps through the frame / pixel map (frame 0 from latent frame 0, the rest resampled; shift 1: 2 x 2 pixels per
    latent pixel), written into a view whose sample stride is larger than HW C.  Family A: the scale is +- a power of two per latent pixel, the shift 0"""
    from motionrag_amd import ops
    N, (T, H, W), C, shift, split, Tz = case
    HW, G = T * H * W, 32
    for family in ("A", "B"):
        mod = X.mod_maps(N, Tz, H >> shift, W >> shift, C, family=family)
        full = tuple(d64(t) for t in X.mod_full(mod, T, H, W, shift, split))
        if family == "A":
            g, b = X.gamma_pattern(C), None
            x, _ = X.gn_family_a(N, HW, C, G)
        else:
            x, g, b, _ = X.gn_family_b(N, HW, C, G)
        silu = family == "B"
        want, lin, off = X.gn_ref64(d64(x), G, d64(g), d64(b), silu=silu, mod=full)
        buf = torch.zeros(N, HW + 7, C, dtype=torch.bfloat16, device=DEV)
        with ops.dispatched() as d:
            got = ops.groupnorm(dv(x), dv(g), dv(b), G, X.EPS, silu=silu, out=buf[:, 7:], mod=dv(mod), mod_geom=(T, H, W, shift, split))
        assert d.counts == {"GN_STATS": 1, "GN_FOLD": 1, "GN_APPLY_MOD": 1}, d.counts
        assert buf[:, :7].abs().max().item() == 0
        report(f"{family} groupnorm mod {T}x{H}x{W} C={C}", X.worst_a(got, want) if family == "A" else X.worst_b(got, want, lin, off, X.C_GN))


def test_groupnorm_one_pass_variance_at_128_sigma(hip):
    """mean 128 standard deviations from zero (mu = +-32, sigma = 1/4: the coarsest spread bf16 resolves there): E[x^2] - mean^2 cancels 14 of fp32's 24 bits.
    The relative error of rstd is read from the kernels' own sums (groupnorm_partial's fp32 (sum, sum of squares) through the folds' formula) against fp64;
    the outputs are held to 2^-8 |want| + C_GN_128 |gamma x^| + 2^-16 |gamma mean rstd| with C_GN_128 four times the measured figure"""
    from motionrag_amd import ops
    worst_rho = 0.0
    for shape in X.GN_SHAPES:
        N, HW, C, G = shape
        for emb in (False, True):
            x, g, b, e, want, lin, off = gn_case_b(shape, False, emb, ratio=128)
            got = ops.groupnorm(dv(x), dv(g), dv(b), G, X.EPS, emb=dv(e))
            need = ((got.double() - want).abs() - X.ULP * want.abs() - X.C_MEAN * off).clamp_min(0) / lin.clamp_min(1e-300)
            print(f"NORM-EXACT groupnorm mu/sigma=128 {N}x{HW}x{C}{' emb' if emb else ''}: smallest c that holds {need.max().item():.3g}")
            report(f"B128 groupnorm {N}x{HW}x{C}{' emb' if emb else ''}", X.worst_b(got, want, lin, off, X.C_GN_128))
        part = ops.groupnorm_partial(dv(x), G).cpu()
        rho = (X.rstd_fp32(part[..., 0], part[..., 1], HW * (C // G)).double() / X.rstd_ref64(x, G) - 1).abs().max().item()
        print(f"NORM-EXACT groupnorm mu/sigma=128 {N}x{HW}x{C}: relative rstd error {rho:.3g} ({rho * 256:.2f} x 2^-8)")
        worst_rho = max(worst_rho, rho)
    assert worst_rho <= 2.0 ** -8, "the one-pass variance loses a full bf16 step of rstd"
