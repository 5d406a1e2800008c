"""mrag_gemm_bf16, mrag_conv_bf16 and the fp8 GEMM / convolution bit for bit: every kernel family behind ops.linear / linear_per_sample /
qkv_linear_qknorm_rope / linear_fp8 / linear_fp8_k64 / conv_implicit / conv_implicit_fp8, on inputs whose correct output is known exactly (gemm_exact.py; that
the checks can fail is proven on the host in test_gemm_exact_cpu.py).

Families A (no rounding anywhere), R (the two rounding points of the residual epilogues, with ties), T (one-hot taps) and Q (quarter-turn RoPE) are judged
with torch.equal against the exact reference: an fp64 product on the device (exact on integers; checked against int64 on the host) followed by bf16
round-to-nearest-even written out.  No tolerance anywhere.  The activation epilogues are judged on the table v -> bits that the result implies (all elements
of one integer accumulator v carry the same bits; the table lies within the existing close() rule of fp64 f(v) and rises strictly over v >= 1): with the bias
drawn from [2, 8] between 56 and 68 % of the elements sit at v >= 1 (60 to 65 % at |value| >= 1 and gate >= 1 for GEGLU), where an accumulator off by one product shows.

Every launch goes through ops.* inside ops.dispatched() (or the fp8 launch counters) and the counters are asserted, so a case cannot land on another kernel.
A and W are column blocks of wider buffers whose padding is NaN, C is a column block of a wider, taller buffer filled with a sentinel that must survive;
conv_implicit wants contiguous tensors and gets NaN guard frames in front and behind.

Shapes come from the dispatch code.  Where the shape first planned for a kernel does not reach it, the shape was moved and the reason stands at the case."""
import pytest
import torch

import gemm_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def dv(t):
    return None if t is None else X.bf(t).to(DEV)


def framed(t, pad=8):
    """host fp32 [R, C] of bf16 values -> a bf16 [R, C] view on the device of a [R, C + pad] buffer whose padding is NaN"""
    wide = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=torch.bfloat16, device=DEV)
    wide[:, :t.shape[1]] = t.to(DEV)
    return wide[:, :t.shape[1]]


class Out:
    """a [M, N] block at column `off` of a [M + 2, N + 16] sentinel buffer"""

    def __init__(self, M, N, off=8):
        self.wide = torch.full((M + 2, N + 16), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
        self.M, self.N, self.off = M, N, off
        self.view = self.wide[:M, off:off + N]

    def check(self, what):
        w = self.wide.clone()
        w[:self.M, self.off:self.off + self.N] = X.SENTINEL
        assert (w == X.SENTINEL).all().item(), f"{what}: written outside the result block"


def same(got, want, what):
    g = got.double()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not torch.equal(g, want):
        bad = (g != want) | torch.isnan(g)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result; first at {idx}: got {g[tuple(idx)].item()}, "
                             f"want {want[tuple(idx)].item()}")


class tuned:
    def __init__(self, tuning=0, **flags):
        self.tuning, self.flags = tuning, flags

    def __enter__(self):
        from motionrag_amd import ops
        ops.TUNING["gemm"] = self.tuning
        for k in self.flags:
            ops.TUNING[k] = self.flags[k]

    def __exit__(self, *exc):
        from motionrag_amd import ops
        ops.TUNING["gemm"] = 0
        for k in self.flags:
            ops.TUNING[k] = False
        return False


class Problem:
    """one (family, M, N, K): operands framed on the device, the exact accumulator computed once"""

    def __init__(self, family, M, N, K, **kw):
        self.M, self.N, self.K, self.family = M, N, K, family
        p = (X.family_r if family == "R" else X.family_a)(M, N, K, **kw)
        self.x, self.w, self.resid = framed(p["x"]), framed(p["w"]), framed(p["resid"])
        self.bias = dv(p["bias"])
        self.acc = X.acc_exact(self.x, self.w)
        self.rpb, self.split = X.gate_plan(M)
        self.gt = dv(X.gates(2, N))

    def want(self, epi):
        if epi == "nobias":
            return X.epilogue_ref(self.acc, None)
        if epi == "bias":
            return X.epilogue_ref(self.acc, self.bias)
        if epi in ("resid", "resid1"):
            return X.epilogue_ref(self.acc, self.bias, X.EPI_RESID, self.resid, 0.5 if epi == "resid" else 1.0)
        return X.epilogue_ref(self.acc, self.bias, X.EPI_GATE_RESID, self.resid, gate=X.gate_rows(self.gt.double(), self.M, self.rpb, self.split))

    def launch(self, epi, counts, tuning=0, off=8):
        from motionrag_amd import ops
        out = Out(self.M, self.N, off)
        kw = {}
        if epi in ("resid", "resid1"):
            kw = dict(epilogue=ops.EPI_RESID, resid=self.resid, acc_scale=0.5 if epi == "resid" else 1.0)
        elif epi == "gate":
            kw = dict(epilogue=ops.EPI_GATE_RESID, resid=self.resid, gate0=self.gt[:, 0], gate1=self.gt[:, 1], rows_per_batch=self.rpb, split=self.split,
                      gate_stride=self.gt.stride(0))
        what = f"{self.family} {self.M}x{self.N}x{self.K} {epi} {'+'.join(counts)}"
        with tuned(tuning), ops.dispatched() as d:
            ops.linear(self.x, self.w, None if epi == "nobias" else self.bias, out=out.view, **kw)
        assert d.counts == counts, (what, d.counts)
        out.check(what)
        return out.view, what

    def check(self, epis, counts, tuning=0, off=8):
        for epi in epis:
            got, what = self.launch(epi, counts, tuning, off)
            same(got, self.want(epi), what)


ALL4 = ("nobias", "bias", "resid", "gate")


# ---------------------------------------------------------------------------------------------- 1, 2: the 128x128 tile, the host's K padding
@pytest.mark.parametrize("shape", X.TILE128, ids=lambda s: "x".join(map(str, s)))
def test_tile_128x128(hip, shape):
    """17 rows (one ragged tile), 257 x 132 (a second row tile of one row, 4 columns into a second column tile), 300 x 260 and 1000 x 520; the sample boundary
    (row ceil(M / 2)) and the split fall inside a wave tile"""
    Problem("A", *shape).check(ALL4, {"GEMM_128x128": 1})


@pytest.mark.parametrize("shape", X.R_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rounding_points_128x128(hip, shape):
    Problem("R", *shape).check(ALL4, {"GEMM_128x128": 1})


def test_host_k_padding(hip):
    """K = 72: ops.linear pads both operands to 128 with zeros"""
    from motionrag_amd import ops
    p = X.family_a(50, 64, 72)
    with ops.dispatched() as d:
        got = ops.linear(dv(p["x"]), dv(p["w"]), dv(p["bias"]))
    assert d.counts == {"GEMM_128x128": 1}, d.counts
    same(got, X.epilogue_ref(X.acc_exact(p["x"], p["w"]), p["bias"]).to(DEV), "K = 72")


# ---------------------------------------------------------------------------------------------- 3, 4: the 8-wave tiles
def test_tile_256x256(hip):
    """200 tiles, K = 192 (below the four-wave kernel's 320), and K = 1024 with the four-wave kernel switched off; family R at K = 1024"""
    from motionrag_amd import ops
    Problem("A", *X.WAVE8[0]).check(ALL4, {"GEMM_256x256": 1})
    Problem("A", *X.WAVE8[1]).check(ALL4, {"GEMM_256x256": 1}, ops.GEMM_TUNE_NO_W4)
    Problem("R", *X.WAVE8[1]).check(("bias", "resid", "gate"), {"GEMM_256x256": 1}, ops.GEMM_TUNE_NO_W4)


def test_tile_256x320(hip):
    """(16384, 640, 384) goes to the four-wave kernel (N % 128 == 0, K >= 320: it replaced the 320-wide tile there), so it reaches the 320-wide tile only with
    that kernel switched off; (7181, 1600, 192) reaches it as shipped (N = 1600 is no multiple of 128, K is below 320)"""
    from motionrag_amd import ops
    Problem("A", *X.WIDE320[0]).check(("bias", "resid"), {"GEMM_256x320": 1}, ops.GEMM_TUNE_NO_W4)
    Problem("A", *X.WIDE320[1]).check(ALL4, {"GEMM_256x320": 1})


# ---------------------------------------------------------------------------------------------- 5: the persistent four-wave kernel
@pytest.mark.parametrize("shape", X.W4, ids=lambda s: "x".join(map(str, s)))
def test_four_wave(hip, shape):
    """200 tiles at K = 320 and 1984 (31 K-tiles: odd), and 542 = 2 x 256 + 30 tiles: workgroups change tile twice, the last round is ragged.  C is a strided,
    16-byte aligned block (the LDS-staged epilogue)"""
    Problem("A", *shape).check(ALL4, {"GEMM_W4": 1})
    if shape[2] == 1984:
        Problem("R", *shape).check(("bias", "resid", "gate"), {"GEMM_W4": 1})


def test_four_wave_general_epilogue(hip):
    """C at column offset 4 (8-byte aligned rows): the dispatch keeps such a C away from the four-wave kernel (16-byte rows are one of its conditions), so the
    kernel's direct-store path is reached through the developer knob that forces it (tuning bits 4..7 = 3); as shipped the shape runs the 8-wave tile"""
    p = Problem("A", *X.W4[0])
    p.check(ALL4, {"GEMM_W4": 1}, tuning=3 << 4, off=4)
    p.check(("bias", "gate"), {"GEMM_256x256": 1}, off=4)


def test_four_wave_per_sample_weights(hip):
    """two samples of 300 rows (two row tiles each, the second ragged: the row-tile grid restarts at every sample), each with its own weight"""
    from motionrag_amd import ops
    B, S, N, K = 2, 300, 256, 320
    ps = [X.family_a(S, N, K, seed=b) for b in range(B)]
    x, w = dv(torch.stack([p["x"] for p in ps])), dv(torch.stack([p["w"] for p in ps]))
    buf = torch.full((B * S + 2, N), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
    with ops.dispatched() as d:
        ops.linear_per_sample(x, w, out=buf[:B * S].view(B, S, N))
    assert d.counts == {"GEMM_W4_BATCHED_W": 1}, d.counts
    assert (buf[B * S:] == X.SENTINEL).all().item()
    for b in range(B):
        same(buf[b * S:(b + 1) * S], X.epilogue_ref(X.acc_exact(x[b], w[b]), None), f"per-sample weights, sample {b}")


# ---------------------------------------------------------------------------------------------- 6: stream-K
@pytest.mark.parametrize("family", ["A", "R"])
def test_stream_k_tail(hip, family):
    """272 tiles: 256 whole ones and a tail of 16 cut into 64 runs of K-tiles whose fp32 partial sums meet in the workspace.  On integers the order cannot show:
    the result is the exact one, and bit-equal to the plain launch"""
    from motionrag_amd import ops
    p = Problem(family, *X.STREAMK)
    for epi in ("bias", "resid", "gate"):
        sk, what = p.launch(epi, {"GEMM_256x256": 1, "GEMM_STREAMK_TAIL": 1}, ops.GEMM_TUNE_STREAMK)
        plain, _ = p.launch(epi, {"GEMM_256x320": 1})                  # as shipped: 221 tiles of 256x320 are one round, 272 of 256x256 two
        same(sk, p.want(epi), what)
        assert torch.equal(sk, plain), what


# ---------------------------------------------------------------------------------------------- 7: K = 320, the weight in registers
@pytest.mark.parametrize("shape", X.K320, ids=lambda s: "x".join(map(str, s)))
def test_n320_k320(hip, shape):
    Problem("A", *shape).check(("nobias", "bias", "resid"), {"GEMM_N320K320": 1})


# ---------------------------------------------------------------------------------------------- 8: the few-row kernel
@pytest.mark.parametrize("shape", X.SKINNY, ids=lambda s: "x".join(map(str, s)))
def test_skinny(hip, shape):
    """eight waves split K; (33, 4100, 2048) runs sixteen waves x 32 columns as shipped and eight x 64 under GEMM_TUNE_SKINNY_8.  The header lets the few-row
    kernel and the tiles differ in the last bit; on integers they may not: both are the exact result"""
    from motionrag_amd import ops, _lib
    p = Problem("A", *shape)
    epis = ("nobias", "bias", "resid", "resid1")
    p.check(epis, {"GEMM_SKINNY": 1})
    if shape[2] >= 2048:
        p.check(epis, {"GEMM_SKINNY": 1}, _lib.CONSTANTS["MRAG_GEMM_TUNE_SKINNY_8"])
    p.check(epis, {"GEMM_128x128": 1}, ops.GEMM_TUNE_NO_SKINNY)


def test_skinny_rounding_points(hip):
    p = Problem("R", 250, 768, 1024)
    p.check(("bias", "resid", "resid1"), {"GEMM_SKINNY": 1})


# ---------------------------------------------------------------------------------------------- 9: activation epilogues
def table_check(bits_of, vals_of, key, size, present_min, what):
    """key [n] int64 table index per element -> (table of values [size] with NaN where no element has the key, present mask); asserts one bit pattern per key"""
    lo = torch.full((size,), 2 ** 20, dtype=torch.int32, device=DEV).scatter_reduce(0, key, bits_of, "amin")
    hi = torch.full((size,), -2 ** 20, dtype=torch.int32, device=DEV).scatter_reduce(0, key, bits_of, "amax")
    present = hi >= lo
    assert present.sum().item() >= present_min, what
    assert (lo == hi)[present].all().item(), f"{what}: elements with the same accumulator carry different bits"
    tab = torch.full((size,), NAN, dtype=torch.float64, device=DEV)
    tab[key] = vals_of
    return tab, present


def check_activation(got, v, epi, what, pair=None):
    """got [M, N'] bf16; v [M, N'] fp64 integers (GEGLU: the gate, `pair` the value half)"""
    f = X.ACT[epi]
    bits = got.contiguous().view(torch.int16).to(torch.int32).flatten()
    g = got.double().flatten()
    lo_v = int(v.min().item())
    nv = int(v.max().item()) - lo_v + 1
    want = f(v) if pair is None else pair * f(v)
    tol_abs = 2e-2 * want.abs().mean().item()                                        # close(): 2 % of the element + 2 % of the mean magnitude of the whole result
    if pair is None:
        key = (v - lo_v).long().flatten()
        tab, present = table_check(bits, g, key, nv, 20, what)
        vs = torch.arange(nv, device=DEV, dtype=torch.float64) + lo_v
        ft = f(vs)
        assert ((tab - ft).abs() <= 2e-2 * ft.abs() + tol_abs)[present].all().item(), f"{what}: the table leaves close() of fp64 f(v)"
        inc = tab[present & (vs >= 1)]
        assert inc.numel() >= 10 and (inc[1:] > inc[:-1]).all().item(), f"{what}: the table does not rise strictly over v >= 1"
        share = X.act_sensitive_share(v)
    else:
        lo_p = int(pair.min().item())
        np_ = int(pair.max().item()) - lo_p + 1
        key = ((pair - lo_p) * nv + (v - lo_v)).long().flatten()
        tab, present = table_check(bits, g, key, np_ * nv, 100, what)
        ps, vs = torch.arange(np_, device=DEV, dtype=torch.float64).view(-1, 1) + lo_p, torch.arange(nv, device=DEV, dtype=torch.float64).view(1, -1) + lo_v
        ft = (ps * f(vs)).flatten()
        assert ((tab - ft).abs() <= 2e-2 * ft.abs() + tol_abs)[present].all().item(), f"{what}: the table leaves close() of fp64 value * f(gate)"
        t2, pr = tab.view(np_, nv), present.view(np_, nv)
        sgn = torch.sign(ps)                                                         # value > 0: rises with the gate; value < 0: falls
        ok_g = ((t2[:, 1:] - t2[:, :-1]) * sgn > 0) | ~(pr[:, 1:] & pr[:, :-1]) | (vs[:, :-1] < 1) | (ps == 0)
        ok_p = (t2[1:] > t2[:-1]) | ~(pr[1:] & pr[:-1]) | (vs < 1)                     # gate >= 1: rises with the value
        assert ok_g.all().item() and ok_p.all().item(), f"{what}: the table is not strictly monotonic over gate >= 1"
        share = ((pair.abs() >= 1) & (v >= 1)).double().mean().item()
    assert share >= 0.5, (what, share)
    print(f"GEMM-EXACT {what}: {int(present.sum())} table entries, {share:.3f} of the elements where the table is strictly monotonic")


ACT_KERNELS = [  # shape, tuning, the unary epilogues' counter (None: that kernel has no unary epilogue at this K), the GEGLU counter
    ("128x128", (300, 288, 192), 0, "GEMM_128x128", "GEMM_128x128"),
    ("8-wave", (6144 + 77, 2048, 192), 0, "GEMM_256x256", "GEMM_256x256"),
    ("four-wave", (6144 + 77, 2048, 1536), 0, "GEMM_W4", "GEMM_W4_GEGLU"),
    ("skinny", (250, 768, 1024), 0, "GEMM_SKINNY", None),
]


@pytest.mark.parametrize("kernel,shape,tuning,unary,geglu", ACT_KERNELS, ids=[k[0] for k in ACT_KERNELS])
def test_activation_epilogues(hip, kernel, shape, tuning, unary, geglu):
    """GELU tanh / erf, SiLU and GEGLU erf / tanh on family A with the bias drawn from [2, 8].  The four-wave kernel has GELU tanh (from K = 1536) and GEGLU
    only: GELU erf and SiLU are asserted to run the 8-wave tile at that shape; the few-row kernel has no GEGLU"""
    from motionrag_amd import ops
    M, N, K = shape
    p = Problem("A", M, N, K, bias_lo=2)
    v = p.acc + p.bias.double()
    for name, epi in (("gelu_tanh", ops.EPI_GELU_TANH), ("gelu_erf", ops.EPI_GELU_ERF), ("silu", ops.EPI_SILU)):
        counts = {unary: 1} if not (kernel == "four-wave" and epi != ops.EPI_GELU_TANH) else {"GEMM_256x256": 1}
        out = Out(M, N)
        with tuned(tuning), ops.dispatched() as d:
            ops.linear(p.x, p.w, p.bias, out=out.view, epilogue=epi)
        assert d.counts == counts, (kernel, name, d.counts)
        out.check(f"{kernel} {name}")
        check_activation(out.view, v, epi, f"{kernel} {name}")
    if geglu is None:
        return
    # [value | gate] in 16-row groups: output column j of group j // 16 multiplies accumulator columns 32 (j // 16) + j % 16 and + 16
    j = torch.arange(N // 2, device=DEV)
    cv, cg = 32 * (j // 16) + j % 16, 32 * (j // 16) + 16 + j % 16
    for name, tanh, epi in (("geglu_erf", False, X.EPI_GELU_ERF), ("geglu_tanh", True, X.EPI_GELU_TANH)):
        out = Out(M, N // 2)
        with tuned(tuning), ops.dispatched() as d:
            ops.linear(p.x, p.w, p.bias, out=out.view, epilogue=ops.EPI_GEGLU, geglu_tanh=tanh)
        assert d.counts == {geglu: 1}, (kernel, name, d.counts)
        out.check(f"{kernel} {name}")
        check_activation(out.view, v[:, cg], epi, f"{kernel} {name}", pair=v[:, cv])


# ---------------------------------------------------------------------------------------------- 10: the fused QKV projection
def qkv_run(H, first, n, counts, tuning=0, **flags):
    from motionrag_amd import ops
    B, S, text, K = (X.QKV[k] for k in ("B", "S", "text", "K"))
    D = H * 64
    p = X.family_a(B * S, 3 * D, K)
    x, w, bias = dv(p["x"]), framed(p["w"][first * D:(first + n) * D]), dv(p["bias"][first * D:(first + n) * D])
    cos, sin = (t.to(DEV) for t in X.rope_tables(S - text))
    buf = torch.full((B * S + 2, n * D), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
    with tuned(tuning, **flags), ops.dispatched() as d:
        ops.qkv_linear_qknorm_rope(x.view(B, S, K), w, bias, H, None, None, None, None, cos, sin, text, q_premul=0.5, first=first, out=buf[:B * S].view(B, S, n * D))
    what = f"qkv H={H} first={first} {'+'.join(counts)}"
    assert d.counts == counts, (what, d.counts)
    assert (buf[B * S:] == X.SENTINEL).all().item(), what
    proj = X.epilogue_ref(X.acc_exact(x, w), bias)
    want = X.qkv_want(proj, B, S, H, text, 0.5, first)
    got = buf[:B * S].double()
    for name, rows in (("text rows", slice(0, text)), ("first video row", slice(text, text + 1)), ("last row of sample 0", slice(S - 1, S)),
                       ("first row of sample 1", slice(S, S + 1)), ("first video row of sample 1", slice(S + text, S + text + 1))):
        same(got[rows], want[rows], f"{what}: {name}")
    same(got, want, what)
    return buf[:B * S]


def test_fused_qkv(hip):
    """B = 2, S = 3011, text 226, K = 640.  At H = 4 the problem is 24 x 3 = 72 tiles, below the 192 at which the fused epilogues start, and the entry point runs
    the plain GEMM and qknorm_rope_kernel (asserted); the fused kernels are reached at H = 16: 288 tiles for Q | K | V, 192 for K | V.  Four-wave, eight-wave and
    the two kernels all give the exact result"""
    from motionrag_amd import ops
    qkv_run(4, 0, 3, {"GEMM_128x128": 1, "QKNORM_ROPE": 1})
    four = qkv_run(X.QKV_FUSED_H, 0, 3, {"GEMM_W4_QKNORM_ROPE": 1})
    eight = qkv_run(X.QKV_FUSED_H, 0, 3, {"GEMM_256x256": 1}, ops.GEMM_TUNE_NO_W4)
    two = qkv_run(X.QKV_FUSED_H, 0, 3, {"GEMM_256x320": 1, "QKNORM_ROPE": 1}, no_qkv_fuse=True)     # (240 tiles of 256x320: one round against two)
    assert torch.equal(four, eight) and torch.equal(four, two)
    qkv_run(X.QKV_FUSED_H, 1, 2, {"GEMM_W4_QKNORM_ROPE": 1})
    qkv_run(X.QKV_FUSED_H, 1, 2, {"GEMM_256x256": 1}, ops.GEMM_TUNE_NO_W4)


# ---------------------------------------------------------------------------------------------- 11: fp8
def test_fp8_linears(hip):
    """A in {-2 .. 2}, W in {-1, 0, 1}: exact in e4m3 behind the row quantiser's power-of-two scale, so the fp8 kernels give the bits of the same reference as
    the bf16 kernel"""
    from motionrag_amd import ops
    for entry, K, counter in (("linear_fp8", 256, ops.fp8_launch_counts), ("linear_fp8_k64", 320, ops.fp8_k64_launch_counts)):
        M, N = 300, 256
        p = X.family_a(M, N, K, a_max=2)
        x, w, bias, resid = framed(p["x"]), framed(p["w"]), dv(p["bias"]), framed(p["resid"])
        w8, w_exp = ops.quant_rows_e4m3(w)
        acc = X.acc_exact(x, w)
        rpb, split = X.gate_plan(M)
        gt = dv(X.gates(2, N))
        cases = [("bias", {}, X.epilogue_ref(acc, bias)), ("resid", dict(epilogue=ops.EPI_RESID, resid=resid), X.epilogue_ref(acc, bias, X.EPI_RESID, resid))]
        if entry == "linear_fp8":
            cases.append(("gate", dict(epilogue=ops.EPI_GATE_RESID, resid=resid, gate0=gt[:, 0], gate1=gt[:, 1], rows_per_batch=rpb, split=split, gate_stride=gt.stride(0)),
                          X.epilogue_ref(acc, bias, X.EPI_GATE_RESID, resid, gate=X.gate_rows(gt.double(), M, rpb, split))))
        for name, kw, want in cases:
            out = Out(M, N)
            before = counter()["gemm"]
            getattr(ops, entry)(x, w8, w_exp, bias, out=out.view, **kw)
            assert counter()["gemm"] == before + 1
            out.check(f"{entry} {name}")
            same(out.view, want, f"{entry} {name}")
            ref16 = Out(M, N)
            ops.linear(x, w, bias, out=ref16.view, **kw)
            assert torch.equal(out.view, ref16.view), f"{entry} {name}: differs from the bf16 kernel"


# ---------------------------------------------------------------------------------------------- 12: convolutions
def guarded(t):
    """host fp32 [F, ...] -> contiguous bf16 on the device between two NaN guard frames"""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), NAN, dtype=torch.bfloat16, device=DEV)
    buf[1:-1] = t.to(DEV)
    return buf[1:-1]


def conv_check(cv, counter, resid=False):
    """families A (bias; with `resid` also the residual at acc_scale 0.5) and T on one convolution, on the kernel `counter`"""
    from motionrag_amd import ops
    mode = ops.CONV_T3 if cv.mode == "t3" else ops.CONV_3X3
    what = f"{cv.mode} {cv.x_shape()}->{cv.Cout} {cv.kwargs()} {counter}"
    p = cv.family_a()
    x, w, bias, res = guarded(p["x"].view(cv.x_shape())), dv(p["w"]), dv(p["bias"]), dv(p["resid"])
    acc = X.acc_exact(cv.rows(x.double().view(cv.F, cv.H, cv.W, cv.Cin)), w)
    for name, kw, want in [("A", {}, X.epilogue_ref(acc, bias))] + ([("A resid", dict(resid=res, acc_scale=0.5), X.epilogue_ref(acc, bias, X.EPI_RESID, res, 0.5))] if resid else []):
        with ops.dispatched() as d:
            got = ops.conv_implicit(x, w, bias, mode, **cv.kwargs(), **kw)
        assert d.counts == {counter: 1}, (what, d.counts)
        same(got.view(cv.M, cv.Cout), want, f"{what} {name}")
    xt = guarded(cv.act_t().expand(cv.F, cv.H, cv.W, cv.Cin).reshape(cv.x_shape()))
    with ops.dispatched() as d:
        got = ops.conv_implicit(xt, dv(cv.weight_t()), None, mode, **cv.kwargs())
    assert d.counts == {counter: 1}, (what, d.counts)
    same(got.view(cv.M, cv.Cout), cv.want_t().double().to(DEV), f"{what} T")


@pytest.mark.parametrize("name", list(X.CONV_SMALL))
def test_conv3_128x128(hip, name):
    """(2, 7, 10, 64 -> 96) and its stride-2 / upsample / asym_pad (7 x 9: odd) / causal forms (two samples of 3 frames behind 2 context frames each: the second
    sample's context must not come from the first's frames nor the first's from the second's)"""
    conv_check(X.CONV_SMALL[name], "CONV3_128x128", resid=True)


@pytest.mark.parametrize("counter,cv,resid", X.CONV_BIG, ids=[f"{c[0]}-{i}" for i, c in enumerate(X.CONV_BIG)])
def test_conv_tiles(hip, counter, cv, resid):
    """every convolution id the dispatch reaches (CONV3_W4, CONVT_W4 and CONVT_256x128 are never dispatched: mrag_conv_bf16 has no branch to them); the (3,1,1)
    cases are two clips of four frames: t = -1 and t = T read zero, not the neighbouring clip"""
    conv_check(cv, counter, resid)


def test_conv_fp8(hip):
    from motionrag_amd import ops
    cv = X.CONV_SMALL["3x3"]
    p = cv.family_a()
    p["x"] = p["x"] * torch.randint(1, 3, p["x"].shape, generator=X.gen(8)).float()
    x, w, bias, res = guarded(p["x"]), dv(p["w"]), dv(p["bias"]), dv(p["resid"])
    w8, w_exp = ops.quant_rows_e4m3(w)
    acc = X.acc_exact(cv.rows(x.double()), w)
    for name, r, want in (("bias", None, X.epilogue_ref(acc, bias)), ("resid", res.view(cv.Fo, cv.Ho, cv.Wo, cv.Cout), X.epilogue_ref(acc, bias, X.EPI_RESID, res))):
        before = ops.conv_fp8_launch_counts()["conv"]
        got = ops.conv_implicit_fp8(x, w8, w_exp, bias, r)
        assert ops.conv_fp8_launch_counts()["conv"] == before + 1
        same(got.view(cv.M, cv.Cout), want, f"conv_implicit_fp8 {name}")
        assert torch.equal(got, ops.conv_implicit(x, w, bias, ops.CONV_3X3, resid=r)), f"conv_implicit_fp8 {name}: differs from the bf16 kernel"
