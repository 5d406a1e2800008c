"""GPU parity tests: every kernel of libmrag_hip.so, called through the C ABI (motionrag_amd.ops -> ctypes), against the
CPU oracle / a plain torch fp32 reference on the same seeded inputs.

Tolerances (stated per the task): bf16 outputs carry 8 significant bits, accumulation is fp32 ->
  |got - want| <= 2e-2 * |want| + 2e-2 * scale     (scale = typical magnitude of the output)
retrieval rows and distances are BIT-EXACT against oracle/topk_oracle.c (same fp32 fmaf chain)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bf(x):
    return x.to(torch.bfloat16)


def close(got, want, scale=None, rtol=2e-2, atol_frac=2e-2):
    got = got.float().cpu()
    want = want.float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    s = want.abs().mean().item() if scale is None else scale
    err = (got - want).abs()
    tol = rtol * want.abs() + atol_frac * s
    bad = (err > tol)
    assert not bad.any(), f"{bad.sum().item()} / {bad.numel()} outside tolerance; max err {err.max().item():.4g}, scale {s:.4g}"


# ---------------------------------------------------------------------------------------------- GEMM
GEMM_SHAPES = [(300, 256, 128), (17, 64, 64), (1000, 520, 192), (4096, 3072, 256), (2, 1024, 512), (257, 132, 64)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_plain_and_bias(hip, M, N, K):
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N)
    x, w, b = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g) * 0.1), bf(torch.randn(N, generator=g))
    want = x.float() @ w.float().t()
    got = ops.linear(x.to(DEV), w.to(DEV))
    close(got, want, scale=want.abs().mean().item())
    got = ops.linear(x.to(DEV), w.to(DEV), b.to(DEV))
    close(got, want + b.float(), scale=want.abs().mean().item())


@pytest.mark.parametrize("epi", ["gelu_tanh", "gelu_erf", "silu", "resid", "gate_resid"])
@pytest.mark.parametrize("M,N,K", [(500, 384, 128), (4100, 3072, 64)])
def test_gemm_epilogues(hip, epi, M, N, K):
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(11)
    x, w, b = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g) * 0.1), bf(torch.randn(N, generator=g))
    acc = x.float() @ w.float().t() + b.float()
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    if epi == "gelu_tanh":
        got, want = ops.linear(xd, wd, bd, epilogue=ops.EPI_GELU_TANH), torch.nn.functional.gelu(acc, approximate="tanh")
    elif epi == "gelu_erf":
        got, want = ops.linear(xd, wd, bd, epilogue=ops.EPI_GELU_ERF), torch.nn.functional.gelu(acc)
    elif epi == "silu":
        got, want = ops.linear(xd, wd, bd, epilogue=ops.EPI_SILU), torch.nn.functional.silu(acc)
    elif epi == "resid":
        r = bf(torch.randn(M, N, generator=g))
        got, want = ops.linear(xd, wd, bd, epilogue=ops.EPI_RESID, resid=r.to(DEV)), r.float() + acc
    else:
        B, rpb, split = 2, M // 2, 37
        M2 = B * rpb
        r = bf(torch.randn(M2, N, generator=g))
        gates = bf(torch.randn(B, 2, N, generator=g))                       # [:, 0] text gate, [:, 1] video gate
        gd = gates.to(DEV)
        rd = r.to(DEV)
        got = ops.linear(xd[:M2], wd, bd, out=rd, epilogue=ops.EPI_GATE_RESID, resid=rd, gate0=gd[:, 0], gate1=gd[:, 1],
                         rows_per_batch=rpb, split=split, gate_stride=gd.stride(0))        # in place, like the DiT
        pos = torch.arange(M2) % rpb
        gsel = torch.where((pos < split)[:, None], gates[torch.arange(M2) // rpb, 0].float(), gates[torch.arange(M2) // rpb, 1].float())
        want = r.float() + gsel * acc[:M2]
    close(got, want, scale=acc.abs().mean().item())


@pytest.mark.parametrize("M,N,K", [(256 * 14, 256 * 16, 320), (256 * 21 + 77, 1280, 1024), (17 * 1024 + 130, 640, 1984), (256 * 300, 256, 64 * 3)])
def test_gemm_persistent_four_wave_kernel(hip, M, N, K):
    """the persistent four-wave 256x256 kernel (gemm_w4_kernel: one workgroup per CU walking its tiles, the K-tile stream running across tile boundaries,
    accumulators pinned in AGPRs, LDS-staged fast epilogue / predicated general epilogue) gives the SAME BITS as the 8-wave tile it replaces for every
    epilogue it carries -- same K order per output, same rounding points -- and both equal the fp32 reference: whole tiles, a ragged last row of tiles
    (rows of a wave tile cut anywhere), one tile per workgroup only, fewer tiles than CUs' second round, a sample boundary and the text / video split
    inside a wave's rows (general epilogue path), K of 3 K-tiles"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = bf(torch.randn(M, K, generator=g)).to(DEV), bf(torch.randn(N, K, generator=g) * K ** -0.5).to(DEV), bf(torch.randn(N, generator=g)).to(DEV)
    r = bf(torch.randn(M, N, generator=g)).to(DEV)
    rpb = 4000 + 37                                                  # sample boundaries fall inside wave tiles
    nb = -(-M // rpb)
    g0, g1 = (bf(torch.randn(nb, N, generator=g)).to(DEV) for _ in range(2))
    acc = x.float() @ w.float().t() + b.float()
    rows = torch.arange(M, device=DEV)
    gate = torch.where(((rows % rpb) < 226)[:, None], g0[rows // rpb].float(), g1[rows // rpb].float())
    cases = {"none": (dict(), acc), "gelu": (dict(epilogue=ops.EPI_GELU_TANH), torch.nn.functional.gelu(acc, approximate="tanh")),
             "resid": (dict(epilogue=ops.EPI_RESID, resid=r), r.float() + acc.to(torch.bfloat16).float()),
             "resid scaled": (dict(epilogue=ops.EPI_RESID, resid=r, acc_scale=0.375), r.float() + (0.375 * acc).to(torch.bfloat16).float()),
             "gate": (dict(epilogue=ops.EPI_GATE_RESID, resid=r, gate0=g0, gate1=g1, rows_per_batch=rpb, split=226, gate_stride=N), r.float() + (gate * acc).to(torch.bfloat16).float())}
    for name, (kw, want) in cases.items():
        try:
            ops.TUNING["gemm"] = ops.GEMM_TUNE_NO_W4
            eight = ops.linear(x, w, b, **kw)
            ops.TUNING["gemm"] = 3 << 4                              # the four-wave kernel whatever the dispatch rule says about this shape
            four = ops.linear(x, w, b, **kw)
            inplace = r.clone()
            if "resid" in kw:                                        # in place over the residual, as the DiT calls it
                ops.linear(x, w, b, out=inplace, **{**kw, "resid": inplace})
        finally:
            ops.TUNING["gemm"] = 0
        assert torch.equal(four, eight), f"{name}: {(four.float() - eight.float()).abs().max().item()}"
        assert "resid" not in kw or torch.equal(inplace, four), name
        close(four, want, scale=want.abs().mean().item())
    # GEGLU (value * gelu(gate) of interleaved weight rows -> [M, N / 2]), erf and tanh gates
    wi, bi = ops.geglu_interleave(w, b)
    for tanh in (False, True):
        outs = {}
        for name, t in (("eight", ops.GEMM_TUNE_NO_W4), ("four", 3 << 4)):
            ops.TUNING["gemm"] = t
            try:
                outs[name] = ops.linear(x, wi, bi, epilogue=ops.EPI_GEGLU, geglu_tanh=tanh)
            finally:
                ops.TUNING["gemm"] = 0
        assert torch.equal(outs["four"], outs["eight"]), f"geglu tanh={tanh}"
        a16 = acc.to(torch.bfloat16).float()
        want = a16[:, :N // 2] * torch.nn.functional.gelu(a16[:, N // 2:], approximate="tanh" if tanh else "none")
        close(outs["four"], want, scale=want.abs().mean().item())
    # two launches in flight on two streams (each wants every CU's whole LDS: the workgroups of the second fill CUs as the first one's leave): same bits
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o1, o2 = torch.empty(M, N, device=DEV, dtype=torch.bfloat16), torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ops.TUNING["gemm"] = 3 << 4
    try:
        for _ in range(3):
            with torch.cuda.stream(s1):
                ops.linear(x, w, b, out=o1, epilogue=ops.EPI_GELU_TANH)
            with torch.cuda.stream(s2):
                ops.linear(x, w, b, out=o2, epilogue=ops.EPI_RESID, resid=r)
    finally:
        ops.TUNING["gemm"] = 0
    torch.cuda.synchronize()
    ops.TUNING["gemm"] = ops.GEMM_TUNE_NO_W4
    try:
        assert torch.equal(o1, ops.linear(x, w, b, epilogue=ops.EPI_GELU_TANH)) and torch.equal(o2, ops.linear(x, w, b, epilogue=ops.EPI_RESID, resid=r))
    finally:
        ops.TUNING["gemm"] = 0
    # a strided output / residual (a column block of a wider tensor) and an unaligned one (general epilogue: 8-byte stores)
    wide = torch.zeros(M, N + 136, device=DEV, dtype=torch.bfloat16)
    ops.TUNING["gemm"] = ops.GEMM_TUNE_NO_W4
    try:
        plain = ops.linear(x, w, b)
    finally:
        ops.TUNING["gemm"] = 0
    for off in (128, 4):
        try:
            ops.TUNING["gemm"] = 3 << 4
            ops.linear(x, w, b, out=wide[:, off:off + N])
        finally:
            ops.TUNING["gemm"] = 0
        assert torch.equal(wide[:, off:off + N], plain), off
        assert int((wide[:, :off] != 0).sum().item()) == 0 and int((wide[:, off + N:] != 0).sum().item()) == 0
        wide.zero_()


@pytest.mark.parametrize("B,S,H,text,first,n", [(2, 3000 + 11, 4, 226, 0, 3), (2, 256 * 24 + 5, 8, 17, 1, 2), (3, 2048, 6, 0, 0, 3)])
def test_qkv_gemm_four_wave_kernel_matches_eight_wave(hip, B, S, H, text, first, n):
    """the fused QKV projection (per-head qk LayerNorm + RoPE + Q pre-multiplication in the GEMM epilogue) on the persistent four-wave kernel: the same bits
    as on the 8-wave tile (the row math is one shared function; the four-wave row layout holds two heads per wave tile), for Q|K|V and the K|V form of a
    sequence-sharded rank, with sample boundaries and the text / video boundary inside wave tiles and a ragged last row of tiles"""
    from motionrag_amd import ops
    D, K = H * 64, 640
    g = torch.Generator().manual_seed(B * S + H)
    x = bf(torch.randn(B, S, K, generator=g)).to(DEV)
    w = bf(torch.randn(n * D, K, generator=g) * K ** -0.5).to(DEV)
    b = bf(torch.randn(n * D, generator=g)).to(DEV)
    qg, qb, kg, kb = (bf(torch.randn(64, generator=g)).to(DEV) for _ in range(4))
    ang = torch.rand(S - text, 64, generator=g) * 6.28
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
    outs = {}
    for name, t in (("eight", ops.GEMM_TUNE_NO_W4), ("four", 0)):
        ops.TUNING["gemm"] = t
        try:
            outs[name] = ops.qkv_linear_qknorm_rope(x, w, b, H, qg, qb, kg, kb, cos, sin, text, q_premul=0.18, first=first)
        finally:
            ops.TUNING["gemm"] = 0
    assert torch.equal(outs["four"], outs["eight"]), (outs["four"].float() - outs["eight"].float()).abs().max().item()
    ops.TUNING["no_qkv_fuse"] = True                                  # the unfused pair of kernels: same arithmetic up to the order of the bf16 roundings
    try:
        two = ops.qkv_linear_qknorm_rope(x, w, b, H, qg, qb, kg, kb, cos, sin, text, q_premul=0.18, first=first) if (first == 0 and n == 3) else None
    finally:
        ops.TUNING["no_qkv_fuse"] = False
    if two is not None:
        close(outs["four"], two.float(), scale=two.float().abs().mean().item())


@pytest.mark.parametrize("M,N,K", [(4352, 4096, 1024), (5000, 3840, 3072), (8300, 3072, 2048)])
def test_gemm_stream_k_tail(hip, M, N, K):
    """stream-K for the partial last round of 256x256 tiles (272 tiles = 1 round + 16: 64 units of a quarter tile; 300 tiles = 1 + 44: 176 uneven
    units; 396 = 1 + 140: 256 units of ~half a tile, the DiT's regime): every epilogue the DiT runs equals the fp32 reference and the plain launch
    (fp32 summation order is the only difference: a bf16 ulp on a few elements), results are bit-identical run to run whichever contributor
    finishes a tile, the tickets are left at zero, and the C-ABI falls back to the plain launch without (enough) workspace.  Stream-K is an OPT-IN
    developer path (MRAG_GEMM_TUNE_STREAMK): built for VERDICT r2 item 2b, measured slower than the partial last round it replaces"""
    import ctypes
    from motionrag_amd import ops, _lib
    L = _lib.lib()
    need = L.mrag_gemm_workspace_bytes(M, N, K)
    assert need > 0 and L.mrag_gemm_workspace_bytes(256 * 16, 256 * 16, K) == 0          # a grid of whole rounds has no tail
    g = torch.Generator().manual_seed(M + N)
    x, w, b = bf(torch.randn(M, K, generator=g)).to(DEV), bf(torch.randn(N, K, generator=g) * K ** -0.5).to(DEV), bf(torch.randn(N, generator=g)).to(DEV)
    r = bf(torch.randn(M, N, generator=g)).to(DEV)
    rpb = M // 2
    g0, g1 = (bf(torch.randn(2, N, generator=g)).to(DEV) for _ in range(2))
    acc = x.float() @ w.float().t() + b.float()
    pos = torch.arange(M, device=DEV) % rpb
    gate = torch.where((pos < 37)[:, None], g0[torch.arange(M, device=DEV) // rpb].float(), g1[torch.arange(M, device=DEV) // rpb].float()) if M % 2 == 0 else None
    # (keyword arguments, reference, magnitude of the bf16-rounded product in front of the residual add: ITS ulp bounds a rounding flip)
    cases = {"none": (dict(), acc, acc.abs()), "gelu": (dict(epilogue=ops.EPI_GELU_TANH), torch.nn.functional.gelu(acc, approximate="tanh"), acc.abs()),
             "resid": (dict(epilogue=ops.EPI_RESID, resid=r), r.float() + acc.to(torch.bfloat16).float(), acc.abs())}
    if gate is not None:
        cases["gate"] = (dict(epilogue=ops.EPI_GATE_RESID, resid=r, gate0=g0, gate1=g1, rows_per_batch=rpb, split=37, gate_stride=N),
                         r.float() + (gate * acc).to(torch.bfloat16).float(), (gate * acc).abs())
    for name, (kw, want, mag) in cases.items():
        plain = ops.linear(x, w, b, **kw)
        ops.TUNING["gemm"] = ops.GEMM_TUNE_STREAMK          # opt-in developer path (measured slower than the partial last round: DESIGN.md section 7)
        try:
            got = ops.linear(x, w, b, **kw)
            close(got, want, scale=want.abs().mean().item())
            for _ in range(4):
                assert torch.equal(ops.linear(x, w, b, **kw), got), f"{name}: stream-K result differs run to run"
        finally:
            ops.TUNING["gemm"] = 0
        d = (got.float() - plain.float()).abs()
        assert (d > 0).float().mean().item() < 2e-2 and (d <= (plain.float().abs() + mag) * 2.0 ** -7 + 1e-3 * want.abs().mean().item()).all(), name
        assert not torch.equal(got, plain) or name != "none"          # the tail really ran as stream-K (some element rounds differently)
    ws = ops._attn_workspace(x.device, need, "gemm")
    assert int(ws[:1024].to(torch.int32).abs().sum().item()) == 0      # tickets back at zero
    # raw C-ABI: no / short workspace -> the plain launch; a misaligned one is refused
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    plain = ops.linear(x, w, b)
    ops.TUNING["gemm"] = ops.GEMM_TUNE_STREAMK
    try:
        sk = ops.linear(x, w, b)
    finally:
        ops.TUNING["gemm"] = 0
    buf = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    for ptr, nbytes, expect in ((None, 0, plain), (buf.data_ptr(), need - 1, plain), (buf.data_ptr(), need, sk), (buf.data_ptr() + 8, need, None)):
        a = _lib.GemmArgs()
        a.A, a.W, a.bias, a.C = x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr()
        a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
        a.workspace, a.workspace_bytes, a.tuning = ptr, nbytes, ops.GEMM_TUNE_STREAMK
        rc = L.mrag_gemm_bf16(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a))
        if expect is None:
            assert rc == _lib.MRAG_EINVAL
        else:
            assert rc == _lib.MRAG_OK and torch.equal(out, expect)
    a.workspace, a.workspace_bytes, a.tuning = buf.data_ptr(), need, 0                       # workspace without the opt-in bit: the plain launch
    assert L.mrag_gemm_bf16(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a)) == _lib.MRAG_OK and torch.equal(out, plain)


def test_qkv_gemm_stream_k_tail_matches_plain(hip):
    """the fused QKV + qk-norm + RoPE epilogue behind a stream-K tail (the DiT's QKV GEMM: 5 004 tiles = 19 rounds + 140)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(5)
    B, S, H, K, text_len = 2, 3900, 12, 1024, 226                     # M = 7 800 (31 m-tiles) x N = 2 304 (9 n-tiles) = 279 tiles = 1 round + 23
    D = H * 64
    x = bf(torch.randn(B, S, K, generator=g)).to(DEV)
    w = bf(torch.randn(3 * D, K, generator=g) * K ** -0.5).to(DEV)
    b = bf(torch.randn(3 * D, generator=g) * 0.1).to(DEV)
    qg, qb, kg, kb = (bf(1.0 + 0.2 * torch.randn(64, generator=g)).to(DEV) if i % 2 == 0 else bf(0.1 * torch.randn(64, generator=g)).to(DEV) for i in range(4))
    ang = torch.rand(S - text_len, 64, generator=g) * 6.28
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
    from motionrag_amd import _lib
    assert _lib.lib().mrag_gemm_workspace_bytes(B * S, 3 * D, K) > 0
    plain = ops.qkv_linear_qknorm_rope(x, w, b, H, qg, qb, kg, kb, cos, sin, text_len, eps=1e-6, q_premul=0.18)
    ops.TUNING["gemm"] = ops.GEMM_TUNE_STREAMK
    try:
        got = ops.qkv_linear_qknorm_rope(x, w, b, H, qg, qb, kg, kb, cos, sin, text_len, eps=1e-6, q_premul=0.18)
        assert torch.equal(got, ops.qkv_linear_qknorm_rope(x, w, b, H, qg, qb, kg, kb, cos, sin, text_len, eps=1e-6, q_premul=0.18))
    finally:
        ops.TUNING["gemm"] = 0
    # a rounding flip of the bf16 projection moves a normalised, rotated feature by up to ~ulp(proj) * rstd * gamma: bound it loosely, count it tightly
    d = (got.float() - plain.float()).abs()
    assert (d > 0).float().mean().item() < 2e-2 and d.max().item() < 0.12 and not torch.equal(got, plain)


def test_gemm_rejects_bad_arguments(hip):
    from motionrag_amd import ops, _lib
    import ctypes
    x, w = torch.zeros(8, 72, dtype=torch.bfloat16, device=DEV), torch.zeros(16, 72, dtype=torch.bfloat16, device=DEV)
    a = _lib.GemmArgs()
    a.A, a.W, a.C = x.data_ptr(), w.data_ptr(), torch.empty(8, 16, dtype=torch.bfloat16, device=DEV).data_ptr()
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = 8, 16, 72, 72, 72, 16
    assert hip.mrag_gemm_bf16(None, ctypes.byref(a)) == -2          # the C ABI refuses K % 64 != 0 (MRAG_ENOTSUP) ...
    g = torch.Generator().manual_seed(0)
    xr, wr = bf(torch.randn(8, 72, generator=g)), bf(torch.randn(16, 72, generator=g))
    close(ops.linear(xr.to(DEV), wr.to(DEV)), xr.float() @ wr.float().t(), scale=5.0)   # ... the host wrapper zero-pads the reduction dim
    a.K, a.M = 64, 0
    assert hip.mrag_gemm_bf16(None, ctypes.byref(a)) == -1          # MRAG_EINVAL
    with pytest.raises(ops.HipOnly):
        ops.linear(torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(16, 64, dtype=torch.bfloat16))


# ---------------------------------------------------------------------------------------------- attention
def sdpa_ref(q, k, v, mask=None, kv_div=1):
    """fp32 reference on [B, S, H, 64] tensors (bf16-rounded inputs)"""
    q, k, v = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    if kv_div > 1:
        k, v = k.repeat_interleave(kv_div, dim=0), v.repeat_interleave(kv_div, dim=0)
    s = q @ k.transpose(-1, -2) / 8.0
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    o = torch.softmax(s, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[2], -1)


ATTN_SHAPES = [(2, 3, 300, 300), (1, 2, 1000, 777), (2, 2, 64, 64), (1, 1, 257, 130), (3, 12, 25, 1593), (1, 4, 33, 1), (2, 1, 600, 64)]


@pytest.mark.parametrize("B,H,Sq,Skv", ATTN_SHAPES)
def test_attention_matches_reference(hip, B, H, Sq, Skv):
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(B * 100 + Sq)
    q, k, v = (bf(torch.randn(B if i == 0 else B, Sq if i == 0 else Skv, H, 64, generator=g)) for i in range(3))
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    close(got, sdpa_ref(q, k, v), scale=0.3)


def test_attention_fused_qkv_views_and_residual(hip):
    """strided views of a fused QKV buffer + the motion-injection update out = resid + scale * attn (kv batch repeat)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(5)
    B, S, H = 4, 333, 3
    qkv = bf(torch.randn(B, S, 3, H, 64, generator=g))
    d = qkv.to(DEV)
    got = ops.attention(d[:, :, 0], d[:, :, 1], d[:, :, 2])
    close(got, sdpa_ref(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]), scale=0.3)
    kv = bf(torch.randn(2, 25, 2, H, 64, generator=g))                   # B' = 2 motion-token sets, r = 2
    resid = bf(torch.randn(B, S, H * 64, generator=g))
    kd, rd = kv.to(DEV), resid.to(DEV)
    out = ops.attention(d[:, :, 0], kd[:, :, 0], kd[:, :, 1], out=rd, resid=rd, kv_batch_div=2, out_scale=0.75)   # in place
    want = resid.float() + 0.75 * sdpa_ref(qkv[:, :, 0], kv[:, :, 0], kv[:, :, 1], kv_div=2)
    close(out, want, scale=1.0)


def test_attention_block_causal_mask(hip):
    from motionrag_amd import ops
    from oracle import cama_ref
    g = torch.Generator().manual_seed(6)
    B, H, n, l = 2, 4, 10, 25
    q, k, v = (bf(torch.randn(B, n * l, H, 64, generator=g)) for _ in range(3))
    mask = cama_ref.block_causal_mask(n, l)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), mask=mask.to(DEV))
    close(got, sdpa_ref(q, k, v, mask=mask), scale=0.3)


def test_attention_deferred_rescale_branch(hip):
    """cdna guide rule 26: force the running max to jump far past the deferred-rescale threshold at a late tile (and
    again later), and make the first tile strongly negative, so every branch of the online softmax is exercised."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(7)
    B, H, Sq, Skv = 1, 2, 96, 640
    q, k, v = (torch.randn(B, S, H, 64, generator=g) for S in (Sq, Skv, Skv))
    k[:, :64] -= 3.0 * q[:, :1].mean(dim=1, keepdim=True)                 # first tile: low scores
    k[:, 200] = 6.0 * q[:, 5] / q[:, 5].norm(dim=-1, keepdim=True)        # row 5's max jumps at key 200 (tile 3)
    k[:, 450] = 9.0 * q[:, 40] / q[:, 40].norm(dim=-1, keepdim=True)      # row 40 jumps at key 450 (tile 7)
    k[:, 451] = 12.0 * q[:, 5] / q[:, 5].norm(dim=-1, keepdim=True)       # row 5 jumps again
    q, k, v = bf(q), bf(k), bf(v)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    close(got, sdpa_ref(q, k, v), scale=0.3)


def test_attention16_lazy_max_recentre_and_legacy_agreement(hip):
    """attn16.hip (long unmasked sequences on 16x16x32 MFMAs) keeps a LAZY running max: after a row's first tile no row maximum is formed
    and only a tile whose partial row sums exceed 2^24 re-centres.  cdna guide rule 26: force that branch -- a score 40 log2 units above the
    stale max (finite blow-up), one 150 units above (exp2 overflows to inf), one in the slid-back ragged last key tile of the ragged last
    query tile, low scores in the first tile -- against the fp32 reference, and check the 32x32x16 kernel agrees on the same inputs"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(17)
    B, H, Sq, Skv = 1, 2, 300, 1000
    q, k, v = (torch.randn(B, S, H, 64, generator=g) for S in (Sq, Skv, Skv))
    k[:, :64] -= 3.0 * q[:, :1].mean(dim=1, keepdim=True)
    unit = lambda r: q[:, r] / q[:, r].norm(dim=-1, keepdim=True)
    k[:, 300] = 20.0 * unit(7)          # ~ +29 log2 units over row 7's typical maximum: 2^29 > 2^24 -> re-centre
    k[:, 700] = 104.0 * unit(200)       # ~ +150: exp2 overflows -> inf -> re-centre
    k[:, 701] = 21.5 * unit(7)          # row 7 again, two units above its new maximum: P > 1 after a re-centre, no second one needed
    k[:, 990] = 45.0 * unit(290)        # ragged q-tile row, key inside the slid-back last key tile
    q, k, v = bf(q), bf(k), bf(v)
    want = sdpa_ref(q, k, v)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    # Q carries scale * log2 e in bf16 (one extra rounding, 2^-9 relative, documented in attn_flash.hip / DESIGN.md section 4): with keys of
    # norm 20-100 in the set that is up to 0.1 log2 units on a score.  So: the standard tolerance against the fp32 reference evaluated on
    # that rounded Q and against the plain one, both with an absolute term of 0.036-0.045: a CPU emulation of the kernel's roundings (bf16 Q',
    # bf16 P) lands at max |err| 0.0345 on these inputs (rows whose softmax mixes two or three huge keys), exactly what the kernels return
    q_r = bf(q * (0.125 * 1.4426950408889634)) / (0.125 * 1.4426950408889634)
    close(got, sdpa_ref(q_r, k, v), scale=0.3, rtol=3e-2, atol_frac=0.12)
    close(got, want, scale=0.3, rtol=3e-2, atol_frac=0.15)
    ops.TUNING["attn"] = ops.ATTN_TUNE_LEGACY
    try:
        old = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    finally:
        ops.TUNING["attn"] = 0
    close(old, sdpa_ref(q_r, k, v), scale=0.3, rtol=3e-2, atol_frac=0.12)
    close(got, old.float().cpu(), scale=0.3, rtol=2e-2, atol_frac=4e-2)           # the two kernel families agree to a bf16 ulp or two


def test_attention16_optimistic_sweep_ranges(hip):
    """attn16's fast sweep forms P = exp2(S) with NO running maximum and checks each row sum once per sweep against [2^-100, 2^100]; a workgroup
    with a row outside repeats the pass in the checked form.  Softmax is invariant under a per-row offset of the logits, so three copies of one
    problem with the logits shifted by a per-query constant must give the same output as the unshifted fp32 reference:
      +-40 nats (+-58 log2 units: inside the fast sweep's range -- the scale-invariance claim itself),
      +90 nats (exp2 overflows: inf row sums) and -90 nats (every P underflows: zero row sums) -- the checked re-run,
    the shift riding on a dedicated feature (q[63] = c, k[63] = 8: c per logit after the 1/8 scale), exact in bf16.  Also a launch in which only
    ONE row of one workgroup is out of range, and the key-split tail (Sq % 192 != 0 with a workspace) in both regimes."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(31)
    B, H, Sq, Skv = 1, 2, 500, 1344
    q, k, v = (torch.randn(B, S, H, 64, generator=g) for S in (Sq, Skv, Skv))
    q[..., 63] = 0.0
    k[..., 63] = 8.0
    q, k, v = bf(q), bf(k), bf(v)
    want = sdpa_ref(q, k, v)                                  # q[63] = 0: the shift feature does not enter the reference
    base = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV))
    close(base, want, scale=0.3)
    for shift in (40.0, -40.0, 90.0, -90.0):
        qs = q.clone()
        qs[..., 63] = shift                                   # every logit of every row moves by `shift` nats (bf16-exact: 40, 90 and 8 are representable)
        got = ops.attention(qs.to(DEV), k.to(DEV), v.to(DEV))
        # Q' = bf16(Q * scale * log2 e) rounds the shift feature too: the rounding is common to all keys of a row, so it cancels in the softmax
        close(got, want, scale=0.3)
        close(got, base.float().cpu(), scale=0.3, rtol=2e-2, atol_frac=3e-2)
    qs = q.clone()
    qs[:, 137, 1, 63] = 95.0                                  # one row of one (b, h): its workgroup takes the checked re-run, the others stay fast
    qs[:, 499, 0, 63] = -95.0                                 # a row of the ragged last query tile (the key-split units when a workspace is given)
    got = ops.attention(qs.to(DEV), k.to(DEV), v.to(DEV))
    close(got, want, scale=0.3)
    # AT the boundary of the range check.  A row's sum is l = sum_j exp(s_j + c) ~ 1344 e^0.5 e^c = 2^(11.1 + 1.4427 c): it crosses 2^100 at c = +61.6 nats
    # and 2^-100 at c = -77.0 nats.  Shifts on either side of both crossings (bf16-exact values) make SOME rows of a workgroup fail the check and others
    # pass it -- rows differ in their sums by a few bits -- so fast and checked workgroups mix inside one launch; just inside the lower bound the smallest
    # P terms of a row flush below 2^-126 (a relative loss of about 2^-12, far below the bf16 output rounding).  +-69 / +-70 nats (2^+-100 as a LOGIT,
    # the advisor's figure) ride along.
    for shift in (60.0, 61.0, 61.5, 62.0, 63.0, 69.0, 70.0, -69.0, -70.0, -76.0, -76.5, -77.0, -77.5, -78.0):
        qs = q.clone()
        qs[..., 63] = shift
        got = ops.attention(qs.to(DEV), k.to(DEV), v.to(DEV))
        close(got, want, scale=0.3)
        close(got, base.float().cpu(), scale=0.3, rtol=2e-2, atol_frac=3e-2)
    # a per-row ramp across the upper crossing: row r shifted by 59 + r / 64 nats (59 .. 66.8), every workgroup holds rows on both sides
    qs = q.clone()
    qs[..., 63] = bf(59.0 + torch.arange(Sq).float() / 64.0)[None, :, None]
    close(ops.attention(qs.to(DEV), k.to(DEV), v.to(DEV)), want, scale=0.3)


def test_attention_large_sequence_properties(hip):
    """BASELINE-size sequence (S = 17 776, the CogVideoX joint length), checked through size-independent properties:
    (1) with V = ones the output is exactly 1 (softmax rows sum to one); (2) permuting the keys/values does not change
    the output; (3) a random subset of query rows equals the fp32 reference."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(8)
    B, H, S = 1, 2, 17776
    q, k, v = (bf(torch.randn(B, S, H, 64, generator=g)) for _ in range(3))
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ones = ops.attention(qd, kd, torch.ones_like(vd))
    assert (ones.float() - 1.0).abs().max().item() < 1e-2
    out = ops.attention(qd, kd, vd)
    perm = torch.randperm(S, generator=g).to(DEV)
    out_p = ops.attention(qd, kd[:, perm].contiguous(), vd[:, perm].contiguous())
    assert (out.float() - out_p.float()).abs().max().item() < 2e-2
    rows = torch.randint(0, S, (64,), generator=g)
    want = sdpa_ref(q[:, rows], k, v)
    close(out[:, rows.to(DEV)], want, scale=0.05, rtol=3e-2, atol_frac=5e-2)


def test_attention_key_split_tail(hip):
    """long launches hand the ragged last query tile (Sq % 192 rows per head in attn16.hip, Sq % 256 in attn_flash.hip) to short key-chunk
    workgroups + a merge kernel (attn_bf16.hip: mrag_plan_kv_split, attn_combine_kernel): the tail rows and a sample of the others equal the fp32 reference, with a fused residual,
    and agree with the unsplit kernel to a bf16 ulp or two -- for both kernel families"""
    from motionrag_amd import ops, _lib
    g = torch.Generator().manual_seed(9)
    B, H, Sq, Skv = 1, 16, 64 * 256 + 112, 4200
    TAIL = Sq % 192                                                                    # 176 rows (attn16: 192-row workgroups); Sq % 256 = 112 (legacy)
    assert _lib.lib().mrag_attn_workspace_bytes(B, H, Sq, Skv) > 0 and _lib.lib().mrag_attn_workspace_bytes(B, H, 21 * 768, Skv) == 0
    q = bf(torch.randn(B, Sq, H, 64, generator=g))
    k, v = (bf(torch.randn(B, Skv, H, 64, generator=g)) for _ in range(2))
    k[:, 3000] = bf(9.0 * q[:, Sq - 5] / q[:, Sq - 5].norm(dim=-1, keepdim=True))     # one tail row's max lives in a late chunk
    resid = bf(torch.randn(B, Sq, H * 64, generator=g))
    rows = torch.cat([torch.arange(Sq - 176, Sq), torch.randint(0, Sq - 176, (80,), generator=g)])
    want = sdpa_ref(q[:, rows], k, v)
    qd, kd, vd, rd = q.to(DEV), k.to(DEV), v.to(DEV), resid.to(DEV)
    outs = {}
    for family, tail in ((ops.ATTN_TUNE_LEGACY, 112), (0, TAIL)):          # the shipped family last: `outs` feeds the C-ABI checks below
        for splits in ("", "0"):                       # "0": no workspace handed over -> the unsplit launch
            ops.TUNING["attn_no_split"], ops.TUNING["attn"] = splits == "0", family
            try:
                outs[splits] = ops.attention(qd, kd, vd)
                fused = ops.attention(qd, kd, vd, resid=rd, out_scale=0.5)
            finally:
                ops.TUNING["attn_no_split"], ops.TUNING["attn"] = False, 0
            close(outs[splits][:, rows.to(DEV)], want, scale=0.05, rtol=3e-2, atol_frac=5e-2)
            close(fused[:, rows.to(DEV)], resid[:, rows].float() + 0.5 * want, scale=1.0)
        assert torch.equal(outs[""][:, :Sq - tail], outs["0"][:, :Sq - tail])              # full tiles: same code path, bit-identical
        assert not torch.equal(outs[""][:, Sq - tail:], outs["0"][:, Sq - tail:])          # the tail really took the key-split path
        close(outs[""][:, Sq - tail:], outs["0"][:, Sq - tail:].float().cpu(), scale=0.05, rtol=2e-2, atol_frac=4e-2)
    # key-split partials of MIXED kinds in one merge: the tail rows' shift feature (q[63] = c) meets k[63] = 8 only on the first 576 keys -- exactly the
    # first key chunk of this shape's plan (66 key tiles over 8 chunks = 9 tiles) -- so that chunk's logits move by c nats and the other chunks' do not.
    # c = +110: the first chunk overflows the fast sweep and re-runs in the checked form (m ~ +158 in log2 units), the others stay fast (m = 0), and the
    # merge must weigh them e^110 apart; c = -110: every P of the first chunk underflows (checked re-run, m ~ -158) and the chunk must vanish from the
    # merge.  fp32 reference on the same bf16 inputs.
    for c in (110.0, -110.0):
        q2, k2 = q.clone(), k.clone()
        q2[..., 63] = 0.0
        k2[..., 63] = 0.0
        k2[:, :576, :, 63] = 8.0
        q2[:, Sq - TAIL:, :, 63] = c
        tail_rows = torch.arange(Sq - TAIL, Sq)
        want2 = sdpa_ref(q2[:, tail_rows], k2, v)
        with ops.dispatched() as d:
            got2 = ops.attention(q2.to(DEV), k2.to(DEV), vd)
        assert d.counts.get("ATTN16_KSPLIT", 0) == 1 and d.counts.get("ATTN_COMBINE", 0) == 1, d.counts
        close(got2[:, tail_rows.to(DEV)], want2, scale=0.05, rtol=3e-2, atol_frac=5e-2)
    # C ABI: the workspace is optional (none / too small -> the unsplit launch, same result as without the split) and must be 16-byte aligned
    import ctypes
    need = _lib.lib().mrag_attn_workspace_bytes(B, H, Sq, Skv)
    ws = torch.empty(need + 64, dtype=torch.uint8, device=DEV)
    for ws_ptr, ws_bytes, expect in ((None, 0, "0"), (ws.data_ptr(), need - 1, "0"), (ws.data_ptr(), need, ""), (ws.data_ptr() + 8, need, None)):
        out = torch.empty(B, Sq, H * 64, dtype=torch.bfloat16, device=DEV)
        a = _lib.AttnArgs()
        a.Q, a.K, a.V, a.O = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr()
        a.q_sb, a.q_ss, a.q_sh = qd.stride(0), qd.stride(1), qd.stride(2)
        a.k_sb, a.k_ss, a.k_sh = kd.stride(0), kd.stride(1), kd.stride(2)
        a.v_sb, a.v_ss, a.v_sh = vd.stride(0), vd.stride(1), vd.stride(2)
        a.o_sb, a.o_ss = out.stride(0), out.stride(1)
        a.B, a.H, a.Sq, a.Skv, a.kv_batch_div, a.scale, a.out_scale = B, H, Sq, Skv, 1, 0.125, 1.0
        a.workspace, a.workspace_bytes = ws_ptr, ws_bytes
        rc = _lib.lib().mrag_attn_fwd_bf16(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a))
        if expect is None:
            assert rc == _lib.MRAG_EINVAL
        else:
            assert rc == _lib.MRAG_OK and torch.equal(out, outs[expect])


def test_attention_baseline_shape_split_tail_properties(hip):
    """the BASELINE launch itself (B = 2, H = 48, S = 17 776 = 92 x 192 + 112: 8 832 full query tiles + 96 ragged ones run as 768 key-chunk workgroups + merge):
    softmax rows sum to one everywhere (V = ones -> exactly 1), and the ragged tiles' rows of a few heads equal the fp32 reference"""
    from motionrag_amd import ops, _lib
    g = torch.Generator().manual_seed(10)
    B, H, S = 2, 48, 17776
    assert _lib.lib().mrag_attn_workspace_bytes(B, H, S, S) > 0
    q, k, v = (bf(torch.randn(B, S, H, 64, generator=g)) for _ in range(3))
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ones = ops.attention(qd, kd, torch.ones_like(vd))
    assert (ones.float() - 1.0).abs().max().item() < 1e-2
    out = ops.attention(qd, kd, vd)
    rows = torch.cat([torch.arange(S - 112, S), torch.randint(0, S - 112, (16,), generator=g)])
    for h in (0, 23, 47):
        want = sdpa_ref(q[:, rows, h:h + 1], k[:, :, h:h + 1], v[:, :, h:h + 1])
        close(out[:, rows.to(DEV), h * 64:(h + 1) * 64], want, scale=0.05, rtol=3e-2, atol_frac=5e-2)


def test_attention_routes(hip):
    """which kernel family every branch of mrag_attn_fwd_bf16's dispatch takes, at the smallest shapes on each side of it (one call per row, the exact launch
    counts), with the values against the fp32 reference; the rows at 32 / 33 and 128 / 129 queries also cross the wave counts of the 32x32x16 launcher, which
    the counters do not show.  mrag_attn_small_bf16 and mrag_ip_attn_folded_bf16 close the table.  (The key-split routes need long sequences:
    test_attention_key_split_tail.)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(11)
    B, H = 1, 2
    routes = [  # Sq, Skv, extra, tuning, expected counts
        (16, 16, None, 0, {"ATTN_TINY": 1}),
        (16, 16, "resid", 0, {"ATTN_FLASH": 1}),
        (16, 16, None, ops.ATTN_TUNE_NO_TINY, {"ATTN_FLASH": 1}),
        (32, 65, None, 0, {"ATTN_FLASH": 1}),
        (33, 65, None, 0, {"ATTN_FLASH": 1}),
        (128, 65, None, 0, {"ATTN_FLASH": 1}),
        (129, 64, None, 0, {"ATTN_FLASH": 1}),
        (129, 65, None, 0, {"ATTN_FLASH": 1}),                 # the attn16 launcher refuses fewer than 256 keys: the call falls through
        (129, 256, None, 0, {"ATTN16": 1}),
        (129, 256, "mask", 0, {"ATTN_FLASH": 1}),
        (129, 256, "bias", 0, {"ATTN_FLASH": 1}),
        (129, 256, None, ops.ATTN_TUNE_LEGACY, {"ATTN_FLASH": 1}),
    ]
    for Sq, Skv, extra, tuning, counts in routes:
        q = bf(torch.randn(B, Sq, H, 64, generator=g))
        k, v = (bf(torch.randn(B, Skv, H, 64, generator=g)) for _ in range(2))
        kw, want = {}, None
        if extra == "resid":
            resid = bf(torch.randn(B, Sq, H * 64, generator=g))
            kw["resid"] = resid.to(DEV)
            want = resid.float() + sdpa_ref(q, k, v)
        elif extra == "mask":
            mask = torch.rand(Sq, Skv, generator=g) < 0.5
            mask[:, 0] = False                                  # the first key open in every row
            kw["mask"] = mask.to(DEV)
            want = sdpa_ref(q, k, v, mask=mask)
        elif extra == "bias":
            bias = torch.randn(H, Sq, Skv, generator=g)
            kw["bias"] = bias.to(DEV)
            qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
            want = (torch.softmax(qf @ kf.transpose(-1, -2) / 8.0 + bias, dim=-1) @ vf).permute(0, 2, 1, 3).reshape(B, Sq, -1)
        else:
            want = sdpa_ref(q, k, v)
        ops.TUNING["attn"] = tuning
        try:
            with ops.dispatched() as d:
                got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), **kw)
        finally:
            ops.TUNING["attn"] = 0
        assert d.counts == counts, (Sq, Skv, extra, tuning, d.counts)
        close(got, want, scale=1.0 if extra == "resid" else 0.3)
    # head dim 32, 17 x 17
    q, k, v = (bf(torch.randn(B, 17, H, 32, generator=g)) for _ in range(3))
    with ops.dispatched() as d:
        got = ops.attention_small(q.to(DEV), k.to(DEV), v.to(DEV))
    assert d.counts == {"ATTN_SMALL": 1}, d.counts
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    close(got, (torch.softmax(qf @ kf.transpose(-1, -2) * 32 ** -0.5, dim=-1) @ vf).permute(0, 2, 1, 3).reshape(B, 17, -1), scale=0.3)
    # the folded motion-adapter branch at its smallest legal shape
    S, keys = 64, 25
    sc = bf(torch.randn(B, S, H, 32, generator=g) * 3)
    vi = bf(torch.randn(B, keys, H * 64, generator=g))
    hid = bf(torch.randn(B, S, H * 64, generator=g))
    with ops.dispatched() as d:
        got = ops.ip_attn_folded_(sc.view(B, S, H * 32).to(DEV), vi.to(DEV), hid.to(DEV).clone(), H, keys, key_stride=32)
    assert d.counts == {"IP_ATTN_FOLDED": 1}, d.counts
    p = torch.softmax(sc.float()[..., :keys] * 0.125, dim=-1)
    close(got, hid.float() + torch.einsum("bshk,bkhd->bshd", p, vi.float().view(B, keys, H, 64)).reshape(B, S, H * 64), scale=1.0)


# ---------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("rows,D", [(37, 1024), (300, 3072), (9, 64), (5, 320), (4, 4104), (1027, 320), (2050, 640), (1029, 1280), (1571, 1024)])
def test_layernorm(hip, rows, D):
    """(the last four: the narrow-row kernel -- 8 / 4 / 2 / 4 rows per wave at C = 320 / 640 / 1 280 / 1 024 from 1 024 rows up -- with ragged last workgroups)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(rows)
    x, w, b = bf(torch.randn(rows, D, generator=g) * 2 + 0.5), bf(1 + 0.1 * torch.randn(D, generator=g)), bf(0.1 * torch.randn(D, generator=g))
    want = torch.nn.functional.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-5)
    with ops.dispatched() as d:
        got = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5)
    assert d.counts == ({"LAYERNORM_ROWS": 1} if rows >= 1024 and D in (320, 640, 1280, 1024) else {"LAYERNORM": 1}), d.counts
    close(got, want, scale=1.0)
    close(ops.layernorm(x.to(DEV), None, None, 1e-6), torch.nn.functional.layer_norm(x.float(), (D,), None, None, 1e-6), scale=1.0)
    # a strided input / output view (a column slice of a wider buffer) takes the same kernels
    wide_in, wide_out = torch.zeros(rows, D + 64, dtype=torch.bfloat16, device=DEV), torch.zeros(rows, D + 128, dtype=torch.bfloat16, device=DEV)
    wide_in[:, :D] = x.to(DEV)
    ops.layernorm(wide_in[:, :D], w.to(DEV), b.to(DEV), 1e-5, out=wide_out[:, 64:64 + D])
    assert torch.equal(wide_out[:, 64:64 + D], got) and wide_out[:, :64].abs().max().item() == 0 and wide_out[:, 64 + D:].abs().max().item() == 0


def test_layernorm_adaln_modulation_and_batched_output(hip):
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(3)
    B, S, D, split = 2, 50, 256, 7
    x = bf(torch.randn(B, S, D, generator=g))
    w, b = bf(1 + 0.1 * torch.randn(D, generator=g)), bf(0.1 * torch.randn(D, generator=g))
    mod = bf(0.3 * torch.randn(B, 4, D, generator=g))                      # enc_shift, enc_scale, shift, scale
    md = mod.to(DEV)
    got = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, shift0=md[:, 0], scale0=md[:, 1], shift1=md[:, 2], scale1=md[:, 3],
                        rows_per_batch=S, split=split, mod_stride=md.stride(0))
    ln = torch.nn.functional.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-5)
    want = ln.clone()
    want[:, :split] = ln[:, :split] * (1 + mod[:, 1].float()[:, None]) + mod[:, 0].float()[:, None]
    want[:, split:] = ln[:, split:] * (1 + mod[:, 3].float()[:, None]) + mod[:, 2].float()[:, None]
    close(got, want, scale=1.0)
    buf = torch.zeros(B, S + 9, D, dtype=torch.bfloat16, device=DEV)       # write into a slice of a concat buffer
    ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, out_batched=buf[:, 9:])
    close(buf[:, 9:], ln, scale=1.0)
    assert buf[:, :9].abs().max().item() == 0
    # the narrow-row kernel with the same remap: CAMA's media rows (N clips x 1 568 tokens x 1 024) land in front of the latent rows of the K / V concat buffer
    N, T, Dm = 3, 523, 1024
    xm = bf(torch.randn(N, T, Dm, generator=g) * 1.5 - 0.2)
    wm, bm = bf(1 + 0.1 * torch.randn(Dm, generator=g)), bf(0.1 * torch.randn(Dm, generator=g))
    cat = torch.zeros(N, T + 25, Dm, dtype=torch.bfloat16, device=DEV)
    with ops.dispatched() as d:
        ops.layernorm(xm.to(DEV), wm.to(DEV), bm.to(DEV), 1e-5, out_batched=cat[:, :T])
    assert d.counts == {"LAYERNORM_ROWS": 1}, d.counts
    close(cat[:, :T], torch.nn.functional.layer_norm(xm.float(), (Dm,), wm.float(), bm.float(), 1e-5), scale=1.0)
    assert cat[:, T:].abs().max().item() == 0
    assert torch.equal(cat[:, :T].reshape(N * T, Dm), ops.layernorm(xm.to(DEV).view(N * T, Dm), wm.to(DEV), bm.to(DEV), 1e-5))


def test_qknorm_rope(hip):
    from motionrag_amd import ops
    from oracle import cogvideox_ref, cama_ref
    g = torch.Generator().manual_seed(4)
    B, H, text_len, (t, h, w) = 2, 3, 5, (2, 3, 4)
    S = text_len + t * h * w
    qkv = bf(torch.randn(B, S, 3, H, 64, generator=g))
    qg, qb, kg, kb = (bf(1 + 0.2 * torch.randn(64, generator=g)) for _ in range(4))
    cos, sin = cogvideox_ref.rope_3d(64, t, h, w)
    got = ops.qknorm_rope_(qkv.reshape(B, S, 3 * H * 64).to(DEV).clone(), H, qg.to(DEV), qb.to(DEV), kg.to(DEV), kb.to(DEV), cos.to(DEV), sin.to(DEV),
                           text_len, eps=1e-6, q_premul=0.37).view(B, S, 3, H, 64)
    for which, (gm, bt, mul) in enumerate(((qg, qb, 0.37), (kg, kb, 1.0))):
        x = cama_ref.layer_norm(qkv[:, :, which].float(), gm.float(), bt.float(), 1e-6).permute(0, 2, 1, 3)     # [B, H, S, 64]
        x = x.clone()
        x[:, :, text_len:] = cogvideox_ref.apply_rotary_emb(x[:, :, text_len:], cos, sin)
        close(got[:, :, which], (x * mul).permute(0, 2, 1, 3), scale=1.0 * mul)
    assert torch.equal(got[:, :, 2].cpu(), qkv[:, :, 2])                    # V untouched


# ---------------------------------------------------------------------------------------------- pointwise
def test_pointwise_kernels(hip):
    from motionrag_amd import ops
    from oracle import cogvideox_ref
    g = torch.Generator().manual_seed(9)
    t = torch.tensor([999.0, 19.0, 500.0])
    close(ops.timestep_embedding(t.to(DEV), 256), cogvideox_ref.timestep_embedding(t, 256), scale=0.7)
    x = bf(torch.randn(1003, generator=g) * 3)
    close(ops.silu(x.to(DEV)), torch.nn.functional.silu(x.float()), scale=1.0)
    a, b = bf(torch.randn(77, 40, generator=g)), bf(torch.randn(77, 40, generator=g))
    close(ops.add(a.to(DEV), b.to(DEV)), a.float() + b.float(), scale=1.0)
    xx, tab = bf(torch.randn(3, 25, 64, generator=g)), bf(torch.randn(25, 64, generator=g))
    close(ops.add_rows(xx.to(DEV), tab.to(DEV)), xx.float() + tab.float()[None], scale=1.0)


def test_patchify_unpatchify_exact(hip):
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(10)
    Bl, F, C, H, W = 1, 3, 4, 6, 10
    lat, img = bf(torch.randn(Bl, F, C, H, W, generator=g)), bf(torch.randn(Bl, F, C, H, W, generator=g))
    rows = ops.patchify(lat.to(DEV), img.to(DEV), 2).cpu()
    x = torch.cat([lat, img], dim=2).repeat(2, 1, 1, 1, 1).float()          # cat([latents]*2) ; cat on channels
    want = torch.nn.functional.unfold(x.reshape(2 * F, 2 * C, H, W), kernel_size=2, stride=2)      # [BF, C*4, L]
    want = want.transpose(1, 2).reshape(-1, 2 * C * 4)
    assert torch.equal(rows.float(), want)
    back = ops.unpatchify(rows.to(DEV).contiguous(), 2, F, 2 * C, H, W).cpu()
    assert torch.equal(back.float(), x)


def test_cfg_ddim_step(hip):
    from motionrag_amd import ops
    from oracle import cogvideox_ref
    g = torch.Generator().manual_seed(12)
    lat = bf(torch.randn(1, 3, 4, 6, 8, generator=g))
    v = bf(torch.randn(2, 3, 4, 6, 8, generator=g))
    ac = cogvideox_ref.ddim_alphas_cumprod()
    for t in (999, 499, 19):
        co = cogvideox_ref.ddim_coeffs(ac, t, 50)
        got = ops.cfg_ddim_step_(v.to(DEV), lat.to(DEV).clone(), 6.0, *co)
        close(got, cogvideox_ref.cfg_ddim_step(v, lat, 6.0, co), scale=1.0)


# ---------------------------------------------------------------------------------------------- retrieval
def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("N,Q,D,k", [(1000, 5, 64, 12), (300, 33, 768, 12), (5000, 16, 128, 64), (70, 3, 32, 12)])
def test_topk_bit_exact(hip, metric, N, Q, D, k):
    from motionrag_amd import ops
    from oracle import topk_ref
    rng = np.random.default_rng(N + Q)
    db, q = _unit(rng, N, D), _unit(rng, Q, D)
    group = (np.arange(N) // 2).astype(np.int32)
    excl = group[rng.integers(0, N, Q)].astype(np.int32)
    # the 16-chain scan kernel (`order="chain16"`: every batch size) and, where it applies (>= 16 queries, k <= 16), the fan-out kernel -- which is also what
    # "auto" then picks, at every table size
    fan = Q >= 16 and k <= 16
    for order, mode in (("chain16", "f32chain"), ("auto", "f32mfma" if fan else "f32chain")) + ((("mfma", "f32mfma"),) if fan else ()):
        want_r, want_d = topk_ref.topk(db, q, k, metric, group, excl, mode=mode)
        with ops.dispatched() as d:
            rows, dist = ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), k, metric=metric,
                                  group=torch.from_numpy(group).to(DEV), exclude=torch.from_numpy(excl).to(DEV), order=order)
        assert ("TOPK_DENSE" in d.counts) == (mode == "f32mfma") and "TOPK_MFMA" not in d.counts, (order, d.counts)   # (tables of one resident round: the fan-out form's ONE-launch shape)
        np.testing.assert_array_equal(rows.cpu().numpy(), want_r)
        np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32))      # same fmaf chain -> same bits
        rows2, _ = ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), k, metric=metric, order=order)
        np.testing.assert_array_equal(rows2.cpu().numpy(), topk_ref.topk(db, q, k, metric, mode=mode)[0])
    if not (Q >= 16 and k <= 16):
        with pytest.raises(Exception):
            ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), k, metric=metric, order="mfma")     # MRAG_ENOTSUP: the fan-out form takes >= 16 queries, k <= 16


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("Q", [1, 3, 5, 40])
def test_topk_filter_order_bit_exact(hip, metric, Q):
    """lancedb's post-filter (`where(..., prefilter=False)`: the k nearest first, then the filter) and the pre-filter against the C oracle in the
    matching mode, bit for bit, on a database with 6 clips per video where the two orders give different lists; Q = 1 / 3 run the fused
    single-launch form, 5 the query-tile scan + merge kernel, 40 the fan-out kernel ("auto" takes it from 16 queries up: oracle mode f32mfma) and, pinned
    with order="chain16", the scan kernel's 16-query tiles"""
    from motionrag_amd import ops
    from oracle import topk_ref
    from test_oracle_golden import multi_clip_db
    rng = np.random.default_rng(100 + Q)
    db, group = multi_clip_db(rng, n_videos=200, clips=6, dim=128)
    own = rng.integers(0, 200, Q).astype(np.int32)
    q = (db[own * 6 + 1] + 0.01 * rng.standard_normal((Q, 128))).astype(np.float32)
    if Q >= 5:
        own[-1] = 777                        # an id no row carries: nothing is excluded in either order
    dbd, qd, gd, ed = (torch.from_numpy(a).to(DEV) for a in (db, q, group, own))
    lists = {}
    for post in (False, True):
        for order, mode in (("auto", "f32mfma" if Q >= 16 else "f32chain"), ("chain16", "f32chain")):
            want_r, want_d = topk_ref.topk(db, q, 12, metric, group, own, mode=mode, postfilter=post)
            with ops.dispatched() as d:
                rows, dist = ops.topk(dbd, qd, 12, metric=metric, group=gd, exclude=ed, postfilter=post, order=order)
            assert ("TOPK_DENSE" in d.counts) == (mode == "f32mfma") and "TOPK_MFMA" not in d.counts, (order, d.counts)
            np.testing.assert_array_equal(rows.cpu().numpy(), want_r)
            np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32))
        lists[post] = rows.cpu().numpy()
    assert (lists[False] >= 0).all()
    short = (lists[True] >= 0).sum(axis=1)
    assert short[0] == 6 and (short <= 12).all()                                          # 6 of the 12 nearest were the query's own video
    if Q >= 5:
        assert short[-1] == 12 and np.array_equal(lists[True][-1], lists[False][-1])
    # a prepared plan (the interactive path) in post-filter order gives the same list
    if Q <= 4:
        plan = ops.TopkPlan(dbd, Q, 12, metric=metric, group=gd, postfilter=True)
        plan.queries.copy_(qd); plan.exclude.copy_(ed)
        r, _ = plan.run()
        np.testing.assert_array_equal(r.cpu().numpy(), lists[True])


def test_topk_ties_and_short_results(hip):
    from motionrag_amd import ops
    db = np.zeros((40, 32), dtype=np.float32)
    db[3, 0] = 1.0
    q = np.zeros((2, 32), dtype=np.float32)
    rows, dist = ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), 4)
    assert rows.cpu().tolist() == [[0, 1, 2, 4]] * 2 and dist.cpu().tolist() == [[0.0] * 4] * 2
    group = torch.zeros(40, dtype=torch.int32); group[38:] = 1
    rows, dist = ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), 4, group=group.to(DEV),
                          exclude=torch.tensor([0, 5], dtype=torch.int32, device=DEV))
    assert rows.cpu().tolist() == [[38, 39, -1, -1], [0, 1, 2, 4]]
    assert torch.isinf(dist[0, 2:]).all()
    rows, dist = ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), 4, group=group.to(DEV),
                          exclude=torch.tensor([0, 5], dtype=torch.int32, device=DEV), postfilter=True)
    assert rows.cpu().tolist() == [[-1, -1, -1, -1], [0, 1, 2, 4]] and torch.isinf(dist[0]).all()      # the 4 nearest all carry the excluded id


def test_topk_baseline_size(hip):
    """BASELINE config #1 size: 10 000 x 768 database, 256 queries, k = 12 -- equal to the oracle, sorted, filtered."""
    from motionrag_amd import ops
    from oracle import topk_ref
    rng = np.random.default_rng(0)
    db, q = _unit(rng, 10000, 768), _unit(rng, 256, 768)
    group = np.arange(10000, dtype=np.int32)
    excl = rng.integers(0, 10000, 256).astype(np.int32)
    q[:64] = db[excl[:64]] + 0.01 * q[:64]                                   # queries whose own row must be filtered out
    dbd, qd, gd, ed = (torch.from_numpy(a).to(DEV) for a in (db, q, group, excl))
    # "auto" = the fan-out kernel (ONE pass over the table, oracle mode f32mfma); order="chain16" = the scan kernel, 16 passes of 16 queries (mode f32chain)
    for order, mode in (("auto", "f32mfma"), ("chain16", "f32chain"), ("mfma", "f32mfma"), ("mfma_stream", "f32mfma"), ("mfma_nowait", "f32mfma")):
        with ops.dispatched() as d:
            rows, dist = ops.topk(dbd, qd, 12, metric="l2", group=gd, exclude=ed, order=order)
        # the fan-out form: ONE launch at this size ("mfma_stream" forces its three-launch shape, "mfma_nowait" the one launch without the grid wait: the same defined result)
        want = {"TOPK_SCAN": 1, "TOPK_MERGE": 1} if mode == "f32chain" else {"TOPK_MFMA": 1, "TOPK_MERGE": 1} if order == "mfma_stream" else {"TOPK_DENSE": 1}
        assert d.counts == want, (order, d.counts)
        rows, dist = rows.cpu().numpy(), dist.cpu().numpy()
        want_r, want_d = topk_ref.topk(db, q, 12, "l2", group, excl, mode=mode)
        np.testing.assert_array_equal(rows, want_r)
        np.testing.assert_array_equal(dist, want_d.astype(np.float32))
        assert np.all(np.diff(dist, axis=1) >= 0) and not np.any(rows == excl[:, None])


def _fanout_shape(N, Q):
    """which launch shape the fan-out form's plan takes (plan_dense in topk.hip; the kernels are topk_dense.hip's and topk_mfma.hip's): 'one' launch (the dense grid is resident at once), 'two' (dense scores, then the
    finishing launch) or 'stream' (pre-pass, streaming kernel with in-kernel lists, merge)"""
    blocks, qtiles = -(-N // 128), -(-Q // 32)
    if blocks > 512 or Q * blocks * 128 > (16 << 20):
        return "stream"
    for tiles, per_cu in ((4, 1), (2, 2), (2, 2), (1, 3)):
        qb = 32 * tiles
        if qb > 32 * qtiles and qb > 32:
            continue
        if blocks * -(-Q // qb) <= 256 * per_cu:
            return "one"
    return "two"


_FANOUT_COUNTS = {"one": {"TOPK_DENSE": 1}, "two": {"TOPK_DENSE": 1, "TOPK_DENSE_FINISH": 1}, "stream": {"TOPK_MFMA": 1, "TOPK_MERGE": 1}}


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("N,Q,D,k", [(3000, 130, 768, 12), (70001, 40, 768, 12), (66000, 256, 256, 16), (5000, 20, 100, 1), (9000, 300, 64, 7), (130, 16, 32, 12),
                                     (20000, 256, 64, 12), (40000, 100, 96, 16), (39000, 64, 64, 12)])
def test_topk_fanout_bit_exact(hip, metric, N, Q, D, k):
    """the fan-out kernel (fp32 MFMA, `order="mfma"`) against mode 2 of the C oracle, rows AND distances bit for bit, in every configuration of its plan:
    a small table with many queries (the waves split the queries: 32 rows x 4 x 32 TN queries per workgroup), a large table (4 x 32 rows per workgroup,
    32 TN queries per wave, TN = 1 / 2 / 8), more than one query block (Q = 300), a feature count that is no multiple of the 32-feature slab (D = 100: the
    tail chunks stream from a zero row), k = 1 / 7 / 16, a table smaller than a row block; with the self-exclusion filter in both orders"""
    from motionrag_amd import ops
    from oracle import topk_ref
    rng = np.random.default_rng(N + Q)
    db, q = _unit(rng, N, D), _unit(rng, Q, D)
    db[N // 2] = db[N // 3]                                                       # an exact tie: (distance, row) order decides
    group = (np.arange(N) // 2).astype(np.int32)
    excl = group[rng.integers(0, N, Q)].astype(np.int32)
    q[: Q // 4] = db[(2 * excl[: Q // 4])] + 0.01 * q[: Q // 4]                   # queries next to a row of the excluded video
    dbd, qd, gd, ed = (torch.from_numpy(a).to(DEV) for a in (db, q, group, excl))
    shape = _fanout_shape(N, Q)                                                   # (3000, 130) .. (130, 16): one launch; (20000, 256), (40000, 100): two; 66 000 / 70 001 rows: streaming
    assert shape == {3000: "one", 70001: "stream", 66000: "stream", 5000: "one", 9000: "one", 130: "one", 20000: "two", 40000: "two", 39000: "one"}[N]   # (39000, 64): 64 queries on FOUR waves per workgroup
    one_launch = shape == "one"
    for post in (False, True):
        want_r, want_d = topk_ref.topk(db, q, k, metric, group, excl, mode="f32mfma", postfilter=post)
        # "mfma": the shape the plan picks (one launch / dense scores + finishing launch / streaming); "mfma_stream": pre-pass + streaming kernel + merge launch;
        # "mfma_nowait": ONE launch whose workgroups do not wait for each other (the last arriver finishes every query: the bounded wait's fall-back) -- the same
        # defined result from all of them
        for order in ("mfma", "mfma_stream") + (("mfma_nowait",) if one_launch else ()):
            with ops.dispatched() as d:
                rows, dist = ops.topk(dbd, qd, k, metric=metric, group=gd, exclude=ed, postfilter=post, order=order)
            assert d.counts == _FANOUT_COUNTS["stream" if order == "mfma_stream" else shape], (order, d.counts)
            np.testing.assert_array_equal(rows.cpu().numpy(), want_r, err_msg=order)
            np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32), err_msg=order)
    want_r, want_d = topk_ref.topk(db, q, k, metric, mode="f32mfma")
    with ops.dispatched() as d:
        rows, dist = ops.topk(dbd, qd, k, metric=metric, order="auto")            # automatic: the fan-out form wherever it applies
    assert d.counts == _FANOUT_COUNTS[shape], d.counts
    np.testing.assert_array_equal(rows.cpu().numpy(), want_r)
    np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32))


@pytest.mark.parametrize("M", [16384, 40000, 36864 + 37])
def test_gemm_n320_k320_weight_in_registers(hip, M):
    """K = 320, N = 320 / 960 / 2 560 from 16 384 rows up (the UNets' level-0 linears): gemm_k320_kernel -- a 320-column weight slice as MFMA operands in registers, 64-row activation
    tiles streamed, rows leaving whole through an LDS staging tile.  Against torch fp32, bit-equal to the 256x256 / 256x320 tiles (same K order and rounding
    points), with bias, with the residual epilogue and its acc_scale, a ragged last tile, and strided input / output / residual views (column slices)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(M)
    x, w, b, r = bf(torch.randn(M, 320, generator=g)), bf(torch.randn(320, 320, generator=g) * 0.05), bf(torch.randn(320, generator=g)), bf(torch.randn(M, 320, generator=g))
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    ref = x.float() @ w.float().t()
    cases = {"plain": dict(), "bias": dict(bias=bd), "resid": dict(bias=bd, epilogue=ops.EPI_RESID, resid=rd), "resid_scaled": dict(epilogue=ops.EPI_RESID, resid=rd, acc_scale=0.25)}
    outs = {}
    for name, kw in cases.items():
        bias = kw.pop("bias", None)
        with ops.dispatched() as d:
            outs[name] = ops.linear(xd, wd, bias, **kw)
        assert d.counts == {"GEMM_N320K320": 1}, (name, d.counts)
        ops.TUNING["gemm"] = ops.GEMM_TUNE_NO_WIDE
        try:
            with ops.dispatched() as d:
                other = ops.linear(xd, wd, bias, **kw)
        finally:
            ops.TUNING["gemm"] = 0
        assert "GEMM_N320K320" not in d.counts and torch.equal(other, outs[name]), (name, d.counts)
    close(outs["plain"], ref, scale=1.0)
    close(outs["bias"], ref + b.float(), scale=1.0)
    close(outs["resid"], r.float() + (ref + b.float()).to(torch.bfloat16).float(), scale=1.0)
    close(outs["resid_scaled"], r.float() + (0.25 * ref).to(torch.bfloat16).float(), scale=1.0)
    # column slices of wider buffers: lda / ldc / ldr > 320
    xw, ow, rw = torch.zeros(M, 384, dtype=torch.bfloat16, device=DEV), torch.zeros(M, 640, dtype=torch.bfloat16, device=DEV), torch.zeros(M, 328, dtype=torch.bfloat16, device=DEV)
    xw[:, 64:] = xd; rw[:, 8:] = rd
    with ops.dispatched() as d:
        ops.linear(xw[:, 64:], wd, bd, out=ow[:, 320:], epilogue=ops.EPI_RESID, resid=rw[:, 8:])
    assert d.counts == {"GEMM_N320K320": 1}, d.counts
    assert torch.equal(ow[:, 320:], outs["resid"]) and ow[:, :320].abs().max().item() == 0
    # N = 960 (the fused QKV projection: three 320-column slices); the N = 2 560 GEGLU projection on the persistent kernel against the 8-wave tile
    w3, b3 = bf(torch.randn(960, 320, generator=g) * 0.05), bf(torch.randn(960, generator=g))
    wg, bg = bf(torch.randn(2560, 320, generator=g) * 0.05), bf(torch.randn(2560, generator=g) * 0.2)
    wgi, bgi = ops.geglu_interleave(wg.to(DEV), bg.to(DEV))
    for name, fn in (("qkv", lambda: ops.linear(xd, w3.to(DEV), b3.to(DEV))), ("geglu", lambda: ops.linear(xd, wgi, bgi, epilogue=ops.EPI_GEGLU))):
        with ops.dispatched() as d:
            got = fn()
        assert d.counts == ({"GEMM_N320K320": 1} if name == "qkv" else {"GEMM_W4_GEGLU": 1}), (name, d.counts)    # (GEGLU stays on the persistent four-wave kernel: measured faster)
        ops.TUNING["gemm"] = ops.GEMM_TUNE_NO_WIDE
        try:
            with ops.dispatched() as d:
                other = fn()
        finally:
            ops.TUNING["gemm"] = 0
        assert "GEMM_N320K320" not in d.counts and torch.equal(other, got), (name, d.counts)
        if name == "qkv":
            close(got, x.float() @ w3.float().t() + b3.float(), scale=1.0)
        else:
            y = (x.float() @ wg.float().t() + bg.float()).to(torch.bfloat16).float()
            close(got, y[:, :1280] * torch.nn.functional.gelu(y[:, 1280:]), scale=1.0)


@pytest.mark.parametrize("M,inner,K", [(300, 128, 64), (3000, 1280, 320), (40000, 256, 128), (30001, 272, 192)])
def test_gemm_geglu_epilogue(hip, M, inner, K):
    """C = v * gelu_erf(g) with [v | g] = x W^T + b (lvdm attention.py:448-455 / diffusers GEGLU), both tile configurations"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(M + inner)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(2 * inner, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    b = (torch.randn(2 * inner, generator=g) * 0.2).to(torch.bfloat16)
    y = (x.float() @ w.float().T + b.float()).to(torch.bfloat16).float()
    want = y[:, :inner] * torch.nn.functional.gelu(y[:, inner:])
    wi, bi = ops.geglu_interleave(w.to(DEV), b.to(DEV))
    got = ops.linear(x.to(DEV), wi, bi, epilogue=ops.EPI_GEGLU)
    assert got.shape == (M, inner)
    close(got, want, scale=want.abs().mean().item())
    close(ops.linear(x.to(DEV), wi, None, epilogue=ops.EPI_GEGLU), (lambda z: z[:, :inner] * torch.nn.functional.gelu(z[:, inner:]))((x.float() @ w.float().T).to(torch.bfloat16).float()),
          scale=want.abs().mean().item())


@pytest.mark.parametrize("B,H,Sq,Skv,kvdiv", [(37, 5, 16, 16, 1), (100, 3, 14, 14, 1), (9, 2, 1, 16, 1), (12, 4, 16, 5, 3), (1000, 5, 16, 16, 1)])
def test_attention_tiny_sequences(hip, B, H, Sq, Skv, kvdiv):
    """the per-wave kernel for <= 16 x 16 attention (attn_tiny.hip; UNet temporal attention): contiguous layout, the strided (b hw) t c view the temporal
    transformers hand over, kv batch repeat, out_scale, pre-scaled Q -- and agreement with the 64-key-tile kernel on the same inputs"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(B + Sq)
    q = bf(torch.randn(B, Sq, H, 64, generator=g))
    k, v = (bf(torch.randn(B // kvdiv, Skv, H, 64, generator=g)) for _ in range(2))
    want = sdpa_ref(q, k, v, kv_div=kvdiv)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), kv_batch_div=kvdiv)
    close(got, want, scale=0.3)
    close(ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), kv_batch_div=kvdiv, out_scale=0.5), 0.5 * want, scale=0.15)
    ops.TUNING["attn"] = ops.ATTN_TUNE_NO_TINY
    try:
        old = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), kv_batch_div=kvdiv)
    finally:
        ops.TUNING["attn"] = 0
    close(got, old.float().cpu(), scale=0.3, rtol=2e-2, atol_frac=4e-2)     # two bf16 results of the same math: a bf16 ulp or two apart
    if Sq == Skv and kvdiv == 1:            # temporal layout: fused qkv rows ordered (t, hw), attention over t for every hw
        t, hw = Sq, B
        qkv = bf(torch.randn(t, hw, 3, H, 64, generator=g)).to(DEV)
        out = torch.empty(t, hw, H * 64, dtype=torch.bfloat16, device=DEV)
        ops.attention(qkv[:, :, 0].permute(1, 0, 2, 3), qkv[:, :, 1].permute(1, 0, 2, 3), qkv[:, :, 2].permute(1, 0, 2, 3), out=out.permute(1, 0, 2))
        c = qkv.cpu()
        close(out.permute(1, 0, 2), sdpa_ref(c[:, :, 0].permute(1, 0, 2, 3), c[:, :, 1].permute(1, 0, 2, 3), c[:, :, 2].permute(1, 0, 2, 3)), scale=0.3)


@pytest.mark.parametrize("B,S,H,keys,r", [(2, 100, 3, 25, 1), (4, 77, 16, 25, 2), (2, 513, 20, 7, 2)])
def test_ip_attn_folded_kernel(hip, B, S, H, keys, r):
    """hidden += scale * softmax(scores / 8) . V over the valid keys of every (row, head) -- the finishing kernel of the folded motion-adapter
    branch -- and the whole folded branch against the literal to_q_ip -> SDPA order (attn_processor.py:250-273)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(S + H)
    sc = bf(torch.randn(B, S, H, 32, generator=g) * 3)
    v = bf(torch.randn(B // r, keys, H * 64, generator=g))
    hid = bf(torch.randn(B, S, H * 64, generator=g))
    p = torch.softmax(sc.float()[..., :keys] * 0.125, dim=-1)                                     # [B, S, H, keys]
    vv = v.float().view(B // r, keys, H, 64).repeat_interleave(r, dim=0)
    want = hid.float() + 0.75 * torch.einsum("bshk,bkhd->bshd", p, vv).reshape(B, S, H * 64)
    got = ops.ip_attn_folded_(sc.view(B, S, H * 32).to(DEV), v.to(DEV), hid.to(DEV).clone(), H, keys, kv_batch_div=r, out_scale=0.75)
    close(got, want, scale=1.0)


@pytest.mark.parametrize("B,S,H,K,text_len", [(2, 8200, 4, 256, 10), (1, 16500, 4, 192, 0), (2, 100, 2, 128, 7)])
def test_qkv_gemm_fused_qknorm_rope_epilogue(hip, B, S, H, K, text_len):
    """the QKV GEMM whose epilogue applies per-head qk LayerNorm + RoPE + Q pre-scale (attn_processor.py:209-231) equals the plain GEMM
    followed by the norm / RoPE kernel: same arithmetic on the same bf16-rounded projection, so results agree except for a handful of
    round-to-nearest ties decided differently by the two compilations' fp32 contraction (measured: 25 of 12.6 M elements, one bf16 ulp);
    the last shape takes the MRAG_ENOTSUP fallback (small problem -> 128x128 tiles without the LDS-staged epilogue)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(S + H)
    D = H * 64
    x = bf(torch.randn(B, S, K, generator=g)).to(DEV)
    w = bf(torch.randn(3 * D, K, generator=g) * K ** -0.5).to(DEV)
    b = bf(torch.randn(3 * D, generator=g) * 0.1).to(DEV)
    qg, qb, kg, kb = (bf(1.0 + 0.2 * torch.randn(64, generator=g)).to(DEV) if i % 2 == 0 else bf(0.1 * torch.randn(64, generator=g)).to(DEV) for i in range(4))
    ang = torch.rand(S - text_len, 64, generator=g) * 6.28
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
    got = ops.qkv_linear_qknorm_rope(x, w, b, H, qg, qb, kg, kb, cos, sin, text_len, eps=1e-6, q_premul=0.18)
    want = ops.qknorm_rope_(ops.linear(x, w, b), H, qg, qb, kg, kb, cos, sin, text_len, eps=1e-6, q_premul=0.18)
    diff = (got.float() - want.float()).abs()
    assert (diff > 0).float().mean().item() < 1e-4 and (diff <= want.float().abs() * 2.0 ** -7 + 1e-6).all()
    got2 = ops.qkv_linear_qknorm_rope(x, w, None, H, None, None, None, None, None, None, 0)          # no norm, no RoPE: a plain GEMM
    assert torch.equal(got2, ops.linear(x, w))


def test_qkv_gemm_fused_epilogue_matches_oracle(hip):
    """the fused QKV projection + qk LayerNorm + 3-D RoPE epilogue (the form the DiT runs: 256x256 tiles, LDS-staged epilogue) against the
    ORACLE (fp32 projection -> bf16 rounding -> cama_ref.layer_norm -> cogvideox_ref.apply_rotary_emb, attn_processor.py:209-231), not
    against the two-kernel HIP path"""
    from motionrag_amd import ops
    from oracle import cogvideox_ref, cama_ref
    g = torch.Generator().manual_seed(77)
    B, H, K, text_len, (t, h, w) = 2, 4, 256, 226, (8, 30, 45)          # S = 226 + 10 800 rows per sample -> M = 22 052 (fused path)
    S, D = text_len + t * h * w, H * 64
    x = bf(torch.randn(B, S, K, generator=g))
    wq = bf(torch.randn(3 * D, K, generator=g) * K ** -0.5)
    bq = bf(torch.randn(3 * D, generator=g) * 0.1)
    qg, kg = (bf(1.0 + 0.2 * torch.randn(64, generator=g)) for _ in range(2))
    qb, kb = (bf(0.1 * torch.randn(64, generator=g)) for _ in range(2))
    cos, sin = cogvideox_ref.rope_3d(64, t, h, w)
    ops.TUNING["no_qkv_fuse"] = False
    got = ops.qkv_linear_qknorm_rope(x.to(DEV), wq.to(DEV), bq.to(DEV), H, qg.to(DEV), qb.to(DEV), kg.to(DEV), kb.to(DEV), cos.to(DEV), sin.to(DEV),
                                     text_len, eps=1e-6, q_premul=0.18).view(B, S, 3, H, 64)
    rows = torch.cat([torch.arange(0, 300), torch.randint(300, S, (400,), generator=g), torch.arange(S - 40, S)])      # text rows, the text/video seam, a sample, the tail
    proj = (x[:, rows].float() @ wq.float().T + bq.float()).to(torch.bfloat16).float().view(B, len(rows), 3, H, 64)
    pos = rows - text_len
    for which, (gm, bt, mul) in enumerate(((qg, qb, 0.18), (kg, kb, 1.0))):
        y = cama_ref.layer_norm(proj[:, :, which], gm.float(), bt.float(), 1e-6).permute(0, 2, 1, 3).clone()           # [B, H, rows, 64]
        vid = pos >= 0
        y[:, :, vid] = cogvideox_ref.apply_rotary_emb(y[:, :, vid], cos[pos[vid]], sin[pos[vid]])
        close(got[:, rows.to(DEV), which], (y * mul).permute(0, 2, 1, 3), scale=1.0 * mul)
    close(got[:, rows.to(DEV), 2], proj[:, :, 2], scale=1.0)


def test_topk_baseline_size_ranks_equal_float64_oracle(hip):
    """BASELINE config #1 (10 000 x 768, 256 queries, k = 12, self-filter): the rows the GPU returns are the rows the float64 oracle ranks
    (canonical math, independent of the kernel's fp32 evaluation order), wherever neighbouring float64 distances are further apart than the
    fp32 rounding of the 16-chain 768-term sum (SURVEY G13's min-gap guard: 1e-6 absolute on distances <= 2, four times the largest
    error the C oracle's fp32 mode shows here; asserted to cover > 98 % of the ranks), and the distances agree to that bound"""
    from motionrag_amd import ops
    from oracle import topk_ref
    rng = np.random.default_rng(1)
    db, q = _unit(rng, 10000, 768), _unit(rng, 256, 768)
    group = np.arange(10000, dtype=np.int32)
    excl = rng.integers(0, 10000, 256).astype(np.int32)
    q[:64] = db[excl[:64]] + 0.01 * q[:64]
    for metric, order in (("l2", "auto"), ("dot", "auto"), ("l2", "mfma"), ("dot", "mfma")):          # both summation orders rank like the float64 oracle
        rows, dist = ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), 12, metric=metric,
                              group=torch.from_numpy(group).to(DEV), exclude=torch.from_numpy(excl).to(DEV), order=order)
        rows, dist = rows.cpu().numpy(), dist.cpu().numpy()
        want_r, want_d = topk_ref.topk(db, q, 13, metric, group, excl, mode="f64")          # one more: the gap below rank 12 matters too
        gap = np.diff(want_d, axis=1)                                                             # [Q, 12] float64 gaps between neighbours
        tol = 1e-6 * np.maximum(np.abs(want_d[:, :12]), 1.0)                                      # fp32 sum rounding bound (see docstring)
        safe = np.ones((256, 12), bool)
        safe &= gap > 2 * tol                                                                     # rank j vs j + 1
        safe[:, 1:] &= gap[:, :-1] > 2 * tol[:, 1:]                                               # rank j vs j - 1
        assert safe.mean() > 0.98
        assert np.array_equal(rows[safe], want_r[:, :12][safe])
        np.testing.assert_allclose(dist, want_d[:, :12], rtol=0, atol=2e-6)
        assert not np.any(rows == excl[:, None])


def test_topk_prepared_plan_single_launch(hip):
    """ops.TopkPlan: the prepared single-query search (one C-ABI call, scan + merge in ONE launch through the arrival-counter hand-off) returns
    the same rows / distances as the two-kernel path and the oracle, call after call (the counters are left zero), with and without the
    self-exclusion filter, directly and through a HIP-graph replay"""
    from motionrag_amd import ops
    from oracle import topk_ref
    rng = np.random.default_rng(5)
    db, qs = _unit(rng, 10000, 768), _unit(rng, 6, 768)
    group = (np.arange(10000) // 3).astype(np.int32)
    dbd, gd = torch.from_numpy(db).to(DEV), torch.from_numpy(group).to(DEV)
    plan = ops.TopkPlan(dbd, 1, 12, group=gd, graph=True)
    for i in range(6):
        plan.queries.copy_(torch.from_numpy(qs[i:i + 1]))
        excl = int(group[rng.integers(0, 10000)]) if i % 2 else -1
        plan.exclude.fill_(excl)
        rows, dist = plan.run() if i < 4 else plan.replay()
        want_r, want_d = topk_ref.topk(db, qs[i:i + 1], 12, "l2", group, np.array([excl], np.int32), mode="f32chain")
        np.testing.assert_array_equal(rows.cpu().numpy(), want_r)
        np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32))
    plan4 = ops.TopkPlan(dbd, 4, 12, metric="dot")
    plan4.queries.copy_(torch.from_numpy(qs[:4]))
    rows, dist = plan4.run()
    want_r, want_d = topk_ref.topk(db, qs[:4], 12, "dot", mode="f32chain")
    np.testing.assert_array_equal(rows.cpu().numpy(), want_r)
    np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32))


@pytest.mark.parametrize("M,N,K", [(250, 768, 1024), (251, 4096, 1024), (25, 1024, 4096), (16, 2304, 768), (256, 1000, 320), (1, 260, 256), (33, 4100, 2048)])
def test_gemm_few_rows_k_split(hip, M, N, K):
    """M <= 256 (CAMA's Perceiver latents / encoder tokens, the retrieval query's embedder): gemm_skinny_kernel -- 32 x 64 output tiles, the workgroup's eight waves
    split K and meet once in LDS in a fixed order.  Against torch fp32 for every epilogue it carries, ragged M / N (N % 64 != 0, rows past the last tile), strided
    input / output / residual views, run-to-run bit-equality, and the developer knob back to the 128 x 128 tile (equal within the fp32 summation order)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV, torch.bfloat16)
    b = torch.randn(N, generator=g).to(DEV, torch.bfloat16)
    r = torch.randn(M, N, generator=g).to(DEV, torch.bfloat16)
    lin = x.float() @ w.float().T
    cases = {"none": ({}, lin + b.float()), "nobias": (None, lin), "gelu_erf": (dict(epilogue=ops.EPI_GELU_ERF), torch.nn.functional.gelu(lin + b.float())),
             "gelu_tanh": (dict(epilogue=ops.EPI_GELU_TANH), torch.nn.functional.gelu(lin + b.float(), approximate="tanh")),
             "silu": (dict(epilogue=ops.EPI_SILU), torch.nn.functional.silu(lin + b.float())),
             "resid": (dict(epilogue=ops.EPI_RESID, resid=r), (lin + b.float()).to(torch.bfloat16).float() + r.float()),
             "resid_scaled": (dict(epilogue=ops.EPI_RESID, resid=r, acc_scale=0.25), (0.25 * (lin + b.float())).to(torch.bfloat16).float() + r.float())}
    for name, (kw, want) in cases.items():
        with ops.dispatched() as d:
            got = ops.linear(x, w, None, **{}) if kw is None else ops.linear(x, w, b, **kw)
        assert d.counts == {"GEMM_SKINNY": 1}, (name, d.counts)
        rel = ((got.float() - want).norm() / want.norm()).item()
        assert rel < 4e-3, (name, rel)
        again = ops.linear(x, w, None) if kw is None else ops.linear(x, w, b, **kw)
        assert torch.equal(got, again), name                                          # fixed summation order: bit-reproducible
        ops.TUNING["gemm"] = 1 << 17                                                   # MRAG_GEMM_TUNE_NO_SKINNY
        try:
            with ops.dispatched() as d:
                tiled = ops.linear(x, w, None) if kw is None else ops.linear(x, w, b, **kw)
        finally:
            ops.TUNING["gemm"] = 0
        assert "GEMM_SKINNY" not in d.counts and ((tiled.float() - got.float()).norm() / want.norm()).item() < 4e-3, (name, d.counts)
    # strided views: A a column slice of a wider buffer, C / resid column slices of wider buffers
    xa = torch.zeros(M, K + 64, device=DEV, dtype=torch.bfloat16); xa[:, 64:] = x
    cw = torch.zeros(M, N + 128, device=DEV, dtype=torch.bfloat16)
    rw = torch.zeros(M, N + 64, device=DEV, dtype=torch.bfloat16); rw[:, 64:] = r
    with ops.dispatched() as d:
        ops.linear(xa[:, 64:], w, b, epilogue=ops.EPI_RESID, resid=rw[:, 64:], out=cw[:, 64:64 + N])
    assert d.counts == {"GEMM_SKINNY": 1}, d.counts
    assert torch.equal(cw[:, 64:64 + N], ops.linear(x, w, b, epilogue=ops.EPI_RESID, resid=r)) and cw[:, :64].abs().max().item() == 0 and cw[:, 64 + N:].abs().max().item() == 0
