"""Host-only proof that the exact GEMM / convolution tests (test_gpu_gemm_exact.py) can fail: no kernel is involved.  The family conditions of gemm_exact.py are
asserted from the reference alone for every shape the GPU file uses; fp32 host models of a tiled GEMM (32-deep K steps, tiles, the epilogue with its two
roundings), of the implicit convolution and of the rotary epilogue equal the exact reference bit for bit; the same models with one named mistake ("mutants")
must each differ from it on the family named.

MUTANT TABLE -- each mutant, the family that must refuse it (asserted below), and what the old `close()` (2 % of the element + 2 % of the mean
magnitude, test_gpu_kernels) makes of the same mutant on the N(0, 1) data of the existing tests at M x N = 300 x 260, K = 64 / 1024 / 3072 (`old_close_verdicts()`
below recomputes the verdicts; "share" = the share of elements at which the mistake, made there, leaves the tolerance):

  mutant                                       family   old close() on N(0, 1) data, K = 64 / 1024 / 3072
  drop_product (one product of one element)    A        seen at 60 % / 26 % / 10 % of the elements: PASSES at 40 % / 74 % / 90 % of the places it can happen
  drop_last_kstep (32-deep, one tile)          A        caught / caught / caught (97 % / 86 % / 76 % of the tile's elements outside)
  ktile_twice (64-deep, at a tile change)      A        caught / caught / caught
  read_past_k (garbage 3 x 3 for one row)      A        caught / caught / caught (a product of 9; garbage of magnitude 1 is drop_product's case)
  bias_next_col (wave tile's last column)      A        caught / caught / PASSES on the probed columns at 3072 (share 84 % / 52 % / 28 % per element)
  gate_other_segment (rows split - 1, split)   A        caught / caught / caught
  sample_off_by_one (a sample's first row)     A        caught / caught / caught
  scale_resid (acc_scale on the residual)      A        caught / caught / caught
  resid_before_round                           R        PASSES / PASSES / PASSES (one bf16 step at most)
  half_up (ties away from zero)                R        PASSES / PASSES / PASSES
  border_wraps                                 T        caught (3x3, K = 576)
  upsample_off_by_one                          T        caught (K = 576)
  asym_origin                                  T        caught (K = 576)
  tap_crosses_clip                             T        caught ((3,1,1), K = 192)
  causal_next_sample                           T        caught (3x3x3, K = 1728)
  pair_partner                                 Q        caught (random angles)
  pos_from_sample_start                        Q        caught (random angles)

So the old tolerance sees every gross mistake -- a whole K-step, a wrong gate, a shifted tap, a wrong rotary partner: those existing tests do their work -- and
misses the two kinds this file is for: a SINGLE product lost, doubled or foreign (the more so the longer K), and the ORDER and MODE of the bf16 roundings,
which it cannot see at any K.  Families A and R refuse all of them with torch.equal.  The tap and rotary families add no detection power over random data;
they turn "outside tolerance somewhere" into the exact pixel, tap and pair that went wrong, and make the border / clip / sample cases certain instead of likely."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_exact as X

EPIS = (X.EPI_NONE, X.EPI_RESID, X.EPI_GATE_RESID)
ALL_SHAPES = X.TILE128 + [(50, 64, 72)] + X.WAVE8 + X.WIDE320 + X.W4 + [X.STREAMK] + X.K320 + X.SKINNY + X.OTHER + [(X.QKV["B"] * X.QKV["S"], 3 * X.QKV["H"] * 64, X.QKV["K"])]


def ref(p, epi, acc_scale=1.0, gt=None, rpb=0, split=0, **mut):
    M = p["x"].shape[0]
    gate = X.gate_rows(gt, M, rpb, split) if epi == X.EPI_GATE_RESID else None
    return X.epilogue_ref(X.acc_exact(p["x"], p["w"]), p["bias"], epi, p["resid"], acc_scale, gate, **mut)


def model_args(M, N, epi):
    rpb, split = X.gate_plan(M)
    return dict(acc_scale=0.5, gt=X.gates(2, N), rpb=rpb, split=split) if epi != X.EPI_NONE else {}


# ---------------------------------------------------------------------------------------------- the reference itself
def test_bf16_rne_is_round_to_nearest_even():
    g = X.gen(1)
    v = torch.cat([torch.randn(4096, generator=g) * 300, torch.randint(-70000, 70000, (4096,), generator=g).float(), torch.tensor([0.0, 257.0, 259.0, -257.0, 513.0 + 1.0, 127.5, 255.5])])
    assert torch.equal(X.bf16_rne(v.double()).float(), v.to(torch.bfloat16).float())          # v is an fp32 number: one rounding either way
    assert X.bf16_rne(torch.tensor([257.0, 259.0, -257.0, 255.5])).tolist() == [256.0, 260.0, -256.0, 256.0]
    assert X.bf16_rne(torch.tensor([257.0, -257.0]), half_up=True).tolist() == [258.0, -258.0]
    assert X.is_tie(torch.tensor([257.0, 258.0, 514.0, 516.0, 127.5, 128.5])).tolist() == [True, False, True, False, False, True]
    # twice rounded is not once rounded: 256.5 + 2^-20 is above the tie; through float32 first it would come down to 256
    assert X.bf16_rne(torch.tensor([257.0 + 2.0 ** -30], dtype=torch.float64)).item() == 258.0


def test_fp64_product_equals_int64():
    M, N, K = X.TILE128[0]
    for p in (X.family_a(M, N, K), X.family_r(M, N, 512)):
        want = p["x"].numpy().astype(np.int64) @ p["w"].numpy().astype(np.int64).T
        assert np.array_equal(X.acc_exact(p["x"], p["w"]).numpy(), want.astype(np.float64))
        assert np.array_equal((p["x"] @ p["w"].t()).numpy().astype(np.int64), want)                 # fp32 is exact on these too


# ---------------------------------------------------------------------------------------------- family conditions
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_family_a_never_rounds(shape):
    """operands are bf16 numbers and at most 0.1 % of the elements reach 256 at any rounding point, whichever epilogue (fp32 product: exact on integers)"""
    M, N, K = shape
    p = X.family_a(M, N, K)
    assert all(X.bf16_exact(t) for t in p.values())
    assert p["x"].abs().max() == 1 and ((p["x"] != 0).float().mean() - X.density(K)).abs() < 0.02
    acc = p["x"] @ p["w"].t()
    assert acc.abs().max() < 2 ** 23
    rpb, split = X.gate_plan(M)
    gate = X.gate_rows(X.gates(2, N), M, rpb, split)
    for epi in EPIS:
        share = X.overflow_share(X.rounding_points(acc, p["bias"], epi, p["resid"], 0.5, gate))
        assert share <= 1e-3, (shape, epi, share)


def test_family_a_fp8_operands():
    p = X.family_a(300, 256, 256, a_max=2)
    assert p["x"].abs().max() == 2 and X.overflow_share(X.rounding_points(p["x"] @ p["w"].t(), p["bias"], X.EPI_RESID, p["resid"])) <= 1e-3


@pytest.mark.parametrize("shape", X.R_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_family_r_rounds(shape):
    """>= 10 % of the elements tell "round, then add the residual" from "add, then round once"; >= 1 % are exact ties at one of the two rounding points"""
    M, N, K = shape
    p = X.family_r(M, N, K)
    assert all(X.bf16_exact(t) for t in p.values()) and (p["x"].abs() @ p["w"].abs().t()).max() < 2 ** 24
    rpb, split = X.gate_plan(M)
    gt = X.gates(2, N)
    for epi, kw in ((X.EPI_RESID, dict(acc_scale=0.5)), (X.EPI_GATE_RESID, dict(gt=gt, rpb=rpb, split=split))):
        want = ref(p, epi, **kw)
        assert (want != ref(p, epi, resid_first=True, **kw)).double().mean() >= 0.10, (shape, epi)
        pts = X.rounding_points(X.acc_exact(p["x"], p["w"]), p["bias"], epi, p["resid"], kw.get("acc_scale", 1.0), X.gate_rows(gt, M, rpb, split))
        assert (X.is_tie(pts[0]) | X.is_tie(pts[1])).double().mean() >= 0.01, (shape, epi)
        assert (want != ref(p, epi, half_up=True, **kw)).double().mean() >= 0.005
    assert (X.acc_exact(p["x"], p["w"]) + p["bias"]).abs().gt(256).double().mean() >= 0.10


# ---------------------------------------------------------------------------------------------- the models equal the reference
@pytest.mark.parametrize("shape", X.TILE128 + [(300, 260, 3072)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("epi", EPIS)
def test_gemm_model_is_exact_on_family_a(shape, epi):
    M, N, K = shape
    p = X.family_a(M, N, K)
    kw = model_args(M, N, epi)
    assert torch.equal(X.gemm_model(p, epi, **kw).double(), ref(p, epi, **kw))
    assert torch.equal(X.gemm_model(p, epi, BM=256, BN=320, **kw), X.gemm_model(p, epi, **kw))     # whatever the tile


@pytest.mark.parametrize("shape", X.R_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("epi", EPIS)
def test_gemm_model_is_exact_on_family_r(shape, epi):
    M, N, K = shape
    p = X.family_r(M, N, K)
    kw = model_args(M, N, epi)
    assert torch.equal(X.gemm_model(p, epi, **kw).double(), ref(p, epi, **kw))


# ---------------------------------------------------------------------------------------------- GEMM mutants
@pytest.mark.parametrize("mutant", X.MUTANTS_A)
def test_family_a_refuses(mutant):
    for M, N, K in ((300, 260, 192), (300, 260, 3072)):
        p = X.family_a(M, N, K)
        epi = X.MUTANT_EPI.get(mutant, X.EPI_NONE)
        kw = model_args(M, N, epi)
        got, want = X.gemm_model(p, epi, mutant=mutant, **kw).double(), ref(p, epi, **kw)
        assert not torch.equal(got, want), (mutant, K)
        assert torch.isfinite(got).all()


@pytest.mark.parametrize("mutant", X.MUTANTS_R)
def test_family_r_refuses(mutant):
    for M, N, K in X.R_SHAPES:
        p = X.family_r(M, N, K)
        for epi in (X.EPI_RESID, X.EPI_GATE_RESID):
            kw = model_args(M, N, epi)
            assert not torch.equal(X.gemm_model(p, epi, mutant=mutant, **kw).double(), ref(p, epi, **kw)), (mutant, K, epi)


# ---------------------------------------------------------------------------------------------- convolutions
CONVS = {
    "3x3": X.Conv("3x3", 2, 7, 10, 64, 96),
    "stride2": X.Conv("3x3", 2, 7, 9, 64, 96, stride=2),
    "upsample": X.Conv("3x3", 2, 5, 6, 64, 96, upsample=True),
    "asym_pad": X.Conv("3x3", 2, 7, 9, 64, 96, stride=2, asym_pad=True),
    "causal": X.Conv("3x3", 10, 5, 6, 64, 96, t_frames=3),
    "t3": X.Conv("t3", 8, 1, 12, 64, 96, frames=4),
}


def torch_conv(cv, p):
    """the same convolution by torch's routines in fp64 (checks the index arithmetic of Conv.coords; the GPU reference does not use it)"""
    x, w = p["x"].double(), p["w"].double()
    if cv.mode == "t3":
        xx = F.pad(x.view(cv.F // cv.frames, cv.frames, cv.W, cv.Cin), (0, 0, 0, 0, 1, 1))
        wt = w.view(cv.Cout, 3, cv.Cin)
        return sum(torch.einsum("bthc,oc->btho", xx[:, k:k + cv.frames], wt[:, k]) for k in range(3)).reshape(cv.M, cv.Cout)
    if cv.t_frames:
        vol = x.view(-1, cv.t_frames + 2, cv.H, cv.W, cv.Cin).permute(0, 4, 1, 2, 3)
        return F.conv3d(vol, w.view(cv.Cout, 3, 3, 3, cv.Cin).permute(0, 4, 1, 2, 3), padding=(0, 1, 1)).permute(0, 2, 3, 4, 1).reshape(cv.M, cv.Cout)
    img = x.permute(0, 3, 1, 2)
    if cv.upsample:
        img = F.interpolate(img, scale_factor=2, mode="nearest")
    img = F.pad(img, (0, 1, 0, 1)) if cv.asym_pad else F.pad(img, (1, 1, 1, 1))
    return F.conv2d(img, w.view(cv.Cout, 3, 3, cv.Cin).permute(0, 3, 1, 2), stride=cv.stride).permute(0, 2, 3, 1).reshape(cv.M, cv.Cout)


@pytest.mark.parametrize("name", list(CONVS))
def test_conv_model_and_reference(name):
    cv = CONVS[name]
    p = cv.family_a()
    acc = X.acc_exact(cv.rows(p["x"]), p["w"])
    assert torch.equal(acc, torch_conv(cv, p))                                                    # the index arithmetic is that convolution
    assert X.overflow_share(X.rounding_points(acc, p["bias"], X.EPI_RESID, p["resid"], 0.5)) <= 1e-3
    for epi in (X.EPI_NONE, X.EPI_RESID):
        assert torch.equal(X.conv_model(cv, p, epi, 0.5).double(), X.epilogue_ref(acc, p["bias"], epi, p["resid"], 0.5))
    pt = dict(x=cv.act_t().expand(cv.F, cv.H, cv.W, cv.Cin), w=cv.weight_t(), bias=None)
    assert X.bf16_exact(pt["x"]) and pt["x"].abs().max() <= 125 and (pt["w"].sum(1) == 1).all()
    pt["bias"] = torch.zeros(cv.Cout)
    want = cv.want_t()
    assert torch.equal(X.conv_model(cv, pt), want) and torch.equal(torch_conv(cv, pt).float(), want)
    assert cv.Cout >= cv.taps or cv.t_frames                                                       # every tap has a channel (27 taps: channels 0 .. 95 cover them)
    assert (want == 0).float().mean() < 0.5


@pytest.mark.parametrize("cv", list(X.CONV_SMALL.values()) + [c[1] for c in X.CONV_BIG], ids=lambda cv: f"{cv.mode}-{cv.M}x{cv.Cout}x{cv.K}")
def test_family_a_never_rounds_in_the_gpu_convolutions(cv):
    """the condition of family A on every convolution of the GPU file (fp32 product of the gathered rows: exact on integers), and family T's operands"""
    p = cv.family_a()
    acc = cv.rows(p["x"]) @ p["w"].t()
    for epi in (X.EPI_NONE, X.EPI_RESID):
        assert X.overflow_share(X.rounding_points(acc, p["bias"], epi, p["resid"], 0.5)) <= 1e-3
    assert (cv.weight_t().sum(1) == 1).all() and cv.want_t().abs().max() <= 125


@pytest.mark.parametrize("mutant", list(X.MUTANTS_T))
def test_family_t_refuses(mutant):
    cv = {"border_wraps": CONVS["3x3"], "upsample_off_by_one": CONVS["upsample"], "asym_origin": CONVS["asym_pad"], "tap_crosses_clip": CONVS["t3"],
          "causal_next_sample": CONVS["causal"]}[mutant]
    pt = dict(x=cv.act_t().expand(cv.F, cv.H, cv.W, cv.Cin), w=cv.weight_t(), bias=torch.zeros(cv.Cout))
    got = X.conv_model(cv, pt, mutant=mutant)
    assert not torch.equal(got, cv.want_t()) and torch.equal(got, cv.want_t(mutant))


# ---------------------------------------------------------------------------------------------- quarter-turn RoPE
def qkv_case(B=2, S=40, text=7, H=2, K=64):
    p = X.family_a(B * S, 3 * H * 64, K)
    proj = X.epilogue_ref(X.acc_exact(p["x"], p["w"]), p["bias"])
    cos, sin = X.rope_tables(S - text)
    return proj, (B, S, H, text), cos, sin


def test_family_q_model_is_the_signed_permutation():
    proj, (B, S, H, text), cos, sin = qkv_case()
    assert set(cos.unique().tolist()) | set(sin.unique().tolist()) == {-1.0, 0.0, 1.0} and ((cos != 0) != (sin != 0)).all()
    assert len({tuple(r) for r in (cos[:8, ::2] * 2 + sin[:8, ::2]).tolist()}) == 4                 # the turn varies with the position ... and the pair:
    assert (cos[0, ::2] != cos[0, 0]).any()
    for first, n in ((0, 3), (1, 2)):
        pr = proj[:, first * H * 64:(first + n) * H * 64]
        want = X.qkv_want(pr, B, S, H, text, 0.5, first)
        assert torch.equal(X.qkv_model(pr, B, S, H, text, cos, sin, 0.5, first), want)
        assert X.overflow_share([want]) == 0
        w3, p3 = want.view(B, S, n, H * 64), pr.view(B, S, n, H * 64)
        assert torch.equal(w3[:, :text, -1], p3[:, :text, -1]) and torch.equal(w3[:, :, -1], p3[:, :, -1])          # V untouched
        if first == 0:
            assert torch.equal(w3[:, :text, 0], p3[:, :text, 0] * 0.5)                                    # text rows: halved, not turned
            assert torch.equal(w3[:, text, 0, 0:2], p3[:, text, 0, 0:2] * 0.5) and torch.equal(w3[:, text, 0, 2], p3[:, text, 0, 3] * 0.5)      # first video row: pair 0 kept, pair 1 turned three quarters: (a, b) -> (b, -a)
        assert not torch.equal(w3[:, text + 1, 0], p3[:, text + 1, 0] * (0.5 if first == 0 else 1.0))


@pytest.mark.parametrize("mutant", X.MUTANTS_Q)
def test_family_q_refuses(mutant):
    proj, (B, S, H, text), cos, sin = qkv_case()
    assert not torch.equal(X.qkv_model(proj, B, S, H, text, cos, sin, 0.5, mutant=mutant), X.qkv_want(proj, B, S, H, text, 0.5))


# ---------------------------------------------------------------------------------------------- activations
@pytest.mark.parametrize("epi", list(X.ACT))
def test_activation_share(epi):
    """at least half of the elements sit where the table is strictly increasing (v >= 1), with the bias drawn from [2, 8]; fp64 f is strictly increasing there
    by more than a bf16 step, so the assertion on the kernel's table is one it can meet"""
    for M, N, K in ((300, 288, 192), (6221, 2048, 192), (6221, 2048, 1536), (250, 768, 1024)):       # the shapes of test_activation_epilogues
        p = X.family_a(M, N, K, bias_lo=2)
        v = X.acc_exact(p["x"], p["w"]) + p["bias"]
        assert X.act_sensitive_share(v) >= 0.5, (epi, K, X.act_sensitive_share(v))
        tab = X.bf16_rne(X.ACT[epi](torch.arange(1.0, 200.0, dtype=torch.float64)))
        assert (tab[1:] > tab[:-1]).all()


# ---------------------------------------------------------------------------------------------- what the old tolerance makes of the mutants
def old_close_verdicts():
    """{mutant: {K: passes close() on N(0, 1) data}} -- the docstring's table (python -c "import test_gemm_exact_cpu as t; print(t.old_close_verdicts())")"""
    out = {}
    for mutant in X.MUTANTS_A + X.MUTANTS_R:
        out[mutant] = {}
        for K in (64, 1024, 3072):
            M, N = 300, 260
            p = X.family_n(M, N, K)
            epi = X.MUTANT_EPI.get(mutant, X.EPI_NONE)
            kw = model_args(M, N, epi)
            if "gt" in kw:
                kw["gt"] = X.bf(torch.randn(2, 2, N, generator=X.gen(K))).float()
            acc = p["x"].double() @ p["w"].double().t()
            gate = X.gate_rows(kw["gt"], M, kw["rpb"], kw["split"]) if epi == X.EPI_GATE_RESID else None
            want = X.epilogue_ref(acc, p["bias"], epi, p["resid"], kw.get("acc_scale", 1.0), gate)
            out[mutant][K] = X.passes_close(X.gemm_model(p, epi, mutant=mutant, **kw), want)
    for mutant in X.MUTANTS_T:
        cv = {"border_wraps": CONVS["3x3"], "upsample_off_by_one": CONVS["upsample"], "asym_origin": CONVS["asym_pad"], "tap_crosses_clip": CONVS["t3"],
              "causal_next_sample": CONVS["causal"]}[mutant]
        g = X.gen(cv.K)
        p = dict(x=X.bf(torch.randn(cv.F, cv.H, cv.W, cv.Cin, generator=g)).float(), w=X.bf(torch.randn(cv.Cout, cv.K, generator=g)).float(), bias=torch.zeros(cv.Cout))
        want = X.bf16_rne(X.acc_exact(cv.rows(p["x"]), p["w"]))
        out[mutant] = {cv.K: X.passes_close(X.conv_model(cv, p, mutant=mutant), want)}
    proj, (B, S, H, text), _, _ = qkv_case()
    g = X.gen(3)
    proj = X.bf(torch.randn(proj.shape, generator=g)).double()
    ang = torch.rand(S - text, 64, generator=g) * 6.28
    want = X.qkv_model(proj, B, S, H, text, torch.cos(ang), torch.sin(ang), 0.5)
    for mutant in X.MUTANTS_Q:
        out[mutant] = {64: X.passes_close(X.qkv_model(proj, B, S, H, text, torch.cos(ang), torch.sin(ang), 0.5, mutant=mutant), want)}
    return out
