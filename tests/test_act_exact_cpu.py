"""Proves on the host that test_gpu_act_exact.py can fail and that its bounds hold for a correct implementation (inputs, references, bounds, models and mutants in
act_exact.py, whose docstring carries the table of what the old close() makes of each mutant).

The fp32 host models of gelu_tanh_f, gelu_erf_f, silu_f and of the timestep embedding stay inside the derived bounds on every finite bf16 input (worst 0.97 / 0.96 /
0.98 / 0.96 of the bound); every mutant is refused on at least one input, the numbers are printed (`pytest -s`) and held to a floor; one mutant -- an A & S coefficient
off by 1e-9 -- is recorded as NOT refusable."""
import pytest
import torch

import act_exact as E
import gemm_exact as X

FB = E.finite_bits()
XS = E.bits_to_bf16(FB).float()


def test_patterns():
    assert FB.numel() == E.NPAT == 2 * 255 * 128
    x = E.bits_to_bf16(FB)
    assert torch.isfinite(x.float()).all() and torch.equal(E.bf16_to_bits(x), FB)
    assert not torch.isfinite(E.bits_to_bf16(torch.tensor([0x7f80, 0xff80, 0x7fc0])).float()).any()
    for fn in E.FNS:
        want, a = E.table(fn)
        assert int(torch.isnan(want).sum()) == 256 and not torch.isnan(want[FB]).any() and (a[FB] >= 0).all()


@pytest.mark.parametrize("fn", E.FNS)
def test_host_model_inside_the_bound(fn):
    """torch float32, no FMA: the issue's figures are 0.972 (tanh), 0.960 (erf), 0.981 (SiLU) of the bound; evaluated in fp64 the same formulas give the same
    worst case, so the figure is bf16's own rounding, not the chain"""
    worst, refused, at = E.judge(X.bf(E.MODEL[fn](XS)), FB, fn)
    worst64, refused64, _ = E.judge(X.bf(E.MODEL[fn](XS.double())), FB, fn)
    print(f"EXACT host-model {fn} {worst:.3f} at x = {XS[at].item()!r}; the formula in fp64 {worst64:.3f}")
    assert refused == 0 and refused64 == 0 and 0.9 < worst < 0.99


FLOORS = {"tanh_as_erf": 100, "erf_as_tanh": 300, "textbook_tanh": 16000, "quick_gelu_as_erf": 1000, "quick_gelu_as_tanh": 1000, "hard_swish": 2000,
          "erf_missing_half": 30000, "tanh_missing_half": 40000, "silu_missing_log2e": 2000}


@pytest.mark.parametrize("name", list(E.MUTANTS))
def test_mutant_is_refused(name):
    """measured: tanh judged as erf 174 inputs, erf judged as tanh 338 (all with 1.1 <= |x| <= 5.2), textbook tanh 16 117 (NaN from x = 4.5 up), quick-GELU 1 577 /
    1 887, hard-swish 2 885, missing 1/2 32 461 / 48 414, SiLU on exp2(-x) 2 653.  The first three PASS the old close() on N(0, 1)"""
    f, ref = E.MUTANTS[name]
    worst, refused, at = E.judge(X.bf(f(XS)), FB, ref)
    xn = E.normal_samples()
    passes = X.passes_close(X.bf(f(xn)), E.REF[ref](xn.double()))
    print(f"EXACT mutant {name}: refused at {refused} of {E.NPAT} inputs, worst {worst:.3g} bounds at x = {XS[at].item()!r}; old close() on N(0, 1): {'PASSES' if passes else 'caught'}")
    assert refused >= FLOORS[name]
    assert passes == E.CLOSE_PASSES[name]


def test_coefficient_off_by_1e9_is_not_refusable():
    """the bound is not bit-exactness: 1e-9 on any coefficient of 0.5 P(t) is below A & S 7.1.26's own 0.75e-7 and stays inside, in fp32 (where most of it
    disappears in the constant's rounding) and with the formula evaluated in fp64 (where it is a real change)"""
    base = E.judge(X.bf(E.model_gelu_erf(XS)), FB, "gelu_erf")[0]
    for which in range(5):
        for delta in (1e-9, -1e-9):
            for x in (XS, XS.double()):
                worst, refused, _ = E.judge(X.bf(E.model_gelu_erf(x, delta=delta, which=which)), FB, "gelu_erf")
                assert refused == 0 and worst <= base + 1e-3, (which, delta, x.dtype, worst)
    # where the bound does start to see a coefficient: 1e-4 still passes (0.9998 of the bound), 3e-4 is refused at 8 to 16 inputs, 1e-3 at 580 to 800
    for which in range(5):
        assert E.judge(X.bf(E.model_gelu_erf(XS, delta=1e-4, which=which)), FB, "gelu_erf")[1] == 0
        assert E.judge(X.bf(E.model_gelu_erf(XS, delta=3e-4, which=which)), FB, "gelu_erf")[1] >= 5
        assert E.judge(X.bf(E.model_gelu_erf(XS, delta=1e-3, which=which)), FB, "gelu_erf")[1] >= 500


def test_geglu_sweep_and_mutants():
    """the gate sweeps every finite pattern at value 1 and -3.  -3 x gelu(gate) passes bf16's largest number for the 213 gates from 1.13e38 up: there the right
    result is -inf (ratio_of).  Measured: the other gate function is refused at 174 / 338 pairs (value 1) and 177 / 347 (value -3), swapped halves at > 64 000"""
    for val in E.GEGLU_VALUES:
        v = torch.full_like(XS, val)
        for fn, other in (("gelu_erf", "gelu_tanh"), ("gelu_tanh", "gelu_erf")):
            worst, refused, _ = E.judge(X.bf(E.model_geglu(v, XS, fn)), FB, fn, value=v.double())
            assert refused == 0 and worst < 0.99, (val, fn, worst)
            n_gate = E.judge(X.bf(E.model_geglu(v, XS, other)), FB, fn, value=v.double())[1]
            n_swap = E.judge(X.bf(E.model_geglu(XS, v, fn)), FB, fn, value=v.double())[1]
            print(f"EXACT mutant geglu value {val} {fn}: the other gate refused at {n_gate}, halves swapped at {n_swap} of {E.NPAT}")
            assert n_gate >= 100 and n_swap >= 60000
    got = X.bf(E.model_geglu(torch.full_like(XS, -3.0), XS, "gelu_erf")).double()
    assert int(torch.isinf(got).sum()) == 213
    # an infinity where the reference is nowhere near overflow is refused
    assert E.ratio_of(torch.tensor([float("inf")]), torch.tensor([1.0], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64)).item() == float("inf")
    assert E.ratio_of(torch.tensor([float("inf")]), torch.tensor([-3.3e38], dtype=torch.float64), torch.tensor([2e36], dtype=torch.float64)).item() == float("inf")
    # on N(0, 1) pairs the old close() passes the other gate function and the missing pre-rounding, and catches the swapped halves
    vn, gn = (torch.randn(1 << 20, generator=X.gen(s)) for s in (5, 6))
    for fn, other in (("gelu_erf", "gelu_tanh"), ("gelu_tanh", "gelu_erf")):
        w = E.geglu_want(vn, gn, fn, True)[0]
        assert X.passes_close(X.bf(E.model_geglu(vn, gn, other)), w) and X.passes_close(X.bf(E.model_geglu(vn, gn, fn, preround=False)), w)
        assert not X.passes_close(X.bf(E.model_geglu(gn, vn, fn)), w)


@pytest.mark.parametrize("fn", ["gelu_erf", "gelu_tanh"])
def test_family_p_tells_the_contracts_apart(fn):
    """from the references alone: geglu4's contract and ff_fused's differ in the output bits on >= 10 % of family P (measured 63 %), >= 1 % of the accumulators are
    exact ties (55 % of the elements have one); each model passes its own contract and is refused by the other's (measured 14 590 / 17 266 of 32 640 elements)"""
    a, w, v, g = E.family_p_gemm(*E.TILE128)
    assert torch.equal((a @ w.t()).double(), torch.cat([v, g], dim=1))          # two ones per row deliver hi + lo exactly
    assert not X.bf16_exact(v) and not X.bf16_exact(g)
    pre, once = X.bf16_rne(E.geglu_want(v, g, fn, True)[0]), X.bf16_rne(E.geglu_want(v, g, fn, False)[0])
    differ = (pre != once).double().mean().item()
    ties = (X.is_tie(v) | X.is_tie(g)).double().mean().item()
    assert differ >= 0.10 and ties >= 0.01 and X.is_tie(v).double().mean().item() >= 0.01, (differ, ties)
    for preround in (True, False):
        got = X.bf(E.model_geglu(v.float(), g.float(), fn, preround))
        own, other = E.judge_p(got, v, g, fn, preround), E.judge_p(got, v, g, fn, not preround)
        print(f"EXACT mutant family-P {fn} preround={preround}: own contract {own[0]:.3f}, the other contract refuses {other[1]} of {v.numel()} (bits differ on {differ:.3f})")
        assert own[1] == 0 and other[1] >= 1000
    # the bias + one product forms deliver hi + lo exactly too
    for frac in (8, 128):
        hv, lv, hg, lg = E.family_p_bias(300, 32, frac=frac)
        assert X.bf16_exact(hv) and X.bf16_exact(lv) and torch.equal((hv + lv).double(), hv.double() + lv.double()) and not X.bf16_exact(hv + lv)
        assert X.is_tie((hg + lg).double()).double().mean().item() >= 0.01


def test_one_hot_delivery():
    """the accumulator of every output is the pattern itself: an fp32 product on the host of the operands the GPU file sends (every other product is finite x 0),
    every finite pattern present; the GPU shapes' builders assert their own coverage"""
    a_bits, w, P = E.onehot_unary(*E.TILE128)
    a = E.bits_to_bf16(a_bits).float()
    got, sent = E.bf16_to_bits(X.bf(a @ w.t())), a_bits[:, torch.arange(E.TILE128[1]) % P]
    assert torch.equal(got[sent != 0x8000], sent[sent != 0x8000]) and got[sent == 0x8000].item() == 0     # -0 + 0 = +0: the one pattern that arrives as its twin
    assert torch.equal(torch.sort(a_bits.flatten()).values, FB)
    M, N, K = E.TILE128_GEGLU
    a_bits, w, P, values = E.onehot_geglu(M, N, K)
    acc = E.bits_to_bf16(a_bits).float() @ w.t()
    j = torch.arange(N // 2)
    assert torch.equal(acc[:, :N // 2].double(), values.view(1, -1).expand(M, -1)) and torch.equal(acc[:, N // 2:], E.bits_to_bf16(a_bits[:, j % P]).float())
    for val in E.GEGLU_VALUES:                                                   # every pattern meets both values
        assert torch.equal(torch.unique(a_bits[:, j % P][:, values == val]), FB)
    for shape in (E.WAVE8, E.WIDE320, E.STREAMK, E.W4_GELU, E.SKINNY):
        E.onehot_unary(*shape)
    for shape in (E.WAVE8, E.W4_K320, E.K320_GEGLU):
        E.onehot_geglu(*shape)


@pytest.mark.parametrize("dim", E.TS_DIMS)
def test_timestep_embedding_model(dim):
    """the fp32 host model stays inside the derived bound (worst 0.96) at the issue's nine timesteps; swapped halves and a frequency divided by half - 1 are refused"""
    t = torch.tensor(E.TS_T, dtype=torch.float32)
    want, bound = E.timestep_ref(t, dim)
    ratio = lambda got: E.ratio_of(got, want, bound.clamp(min=1e-300))
    r = ratio(E.timestep_model(t, dim))
    print(f"EXACT host-model timestep_embedding dim {dim} {r.max().item():.3f}")
    assert r.max().item() <= 1.0
    for m in ("sin_cos", "half_minus_one"):
        n = int((ratio(E.timestep_model(t, dim, m)) > 1).sum())
        print(f"EXACT mutant timestep {m} dim {dim}: refused at {n} of {want.numel()}")
        assert n >= dim
