"""The activation functions of csrc/common.h (gelu_tanh_f / gelu_tanh_f2, gelu_erf_f, silu_f, geglu4) and the timestep embedding on EVERY finite bf16 input,
against fp64 (helper, not collected; used by test_act_exact_cpu.py and test_gpu_act_exact.py).  Nothing here touches a kernel: the inputs, the fp64 references,
the derived bounds, fp32 host models of the device functions and the same models with one named mistake ("mutants").

Inputs.  bf16 has 65 280 finite bit patterns (2 signs x 255 exponents x 128 fractions); a 256 x 256 tile has more outputs than that, so every site is swept over
all of them.  A table indexed by the bit pattern holds the fp64 reference and the input-dependent part of the bound, computed once per device and shared.

References (fp64, none of them the kernel's formula):
    erf GELU   x * 0.5 erfc(-x / sqrt 2)          tanh GELU   x * sigmoid(2 u), u = sqrt(2 / pi) (x + 0.044715 x^3)          SiLU   x * sigmoid(x)

Bound, derived, for every finite input, no exclusions:
    |got - want| <= (2^-8 + 2^-14) |want| + A(x) + 2^-126
  2^-8    bf16 round-to-nearest of the result (8 significant bits: half a step is at most 2^-8 of the value).
  2^-14   the fp32 chain: about 15 operations of 2^-24 each, v_exp_f32 / v_rcp_f32 at 1 ulp, and the rounding of the exponential's argument z (|z| <= 128 where
          the result still matters: a relative 2^-24 |z| <= 2^-17 of e^z) -- 2^-14 is eight times that sum.
  A(x)    erf: 1e-7 |x| -- Abramowitz & Stegun 7.1.26 documents |error| <= 0.75e-7 on Q; the kernel returns max(x, 0) - |x| Q, so the error enters times |x|;
          rounded up to 1e-7 for the fp32 Horner chain whose terms cancel (the polynomial's alternating coefficients).
          tanh, SiLU: (|x| + 1) 2^-125 -- raw v_exp_f32 / v_rcp_f32 flush results below 2^-126 to zero, and 1 + e = e once e > 2^24: the sigmoid of a very
          negative argument is 0 instead of a number below 2^-126, which times |x| is the term.
          GEGLU: A times |bf16(value)|.
  2^-126  a subnormal bf16 input that the matrix pipe flushes, and a subnormal result that the conversion flushes.

GEGLU contracts (family P).  geglu4 promises bf16( bf16(value) * act(bf16(gate)) ) (the reference's two nn.Linear outputs are bf16); ff_fused.hip promises the fp32
product (value + b1) * gelu(gate + b1) rounded once.  Family P builds accumulators that are NOT bf16 numbers: hi + lo with hi a bf16 number and lo at and beside
half a step of hi (exact ties a third of them, either sign), exact in fp32.  The two contracts then differ in the output bits on a large share of the elements
(test_act_exact_cpu.py asserts >= 10 %, and >= 1 % exact ties), so each site can be held to its own.

What the old close() (2 % of the element + 2 % of the mean magnitude) makes of each mutant on 2^20 N(0, 1) samples, beside the number of the 65 280 inputs
(GEGLU: of the 65 280 (value, gate) pairs of a value; family P: of the 32 640 elements of the (1 020, 64, 64) problem) at which the bound refuses it -- asserted in test_act_exact_cpu.py:

    mutant                                             old close() on N(0, 1)      refused by the bound at
    tanh model judged as erf GELU                      PASSES                      174 inputs (1.1 <= |x| <= 5.2)
    erf model judged as tanh GELU                      PASSES                      338 inputs (the same range)
    textbook 0.5 x (1 + (e^2u - 1) / (e^2u + 1))       PASSES                      16 117 inputs (NaN from x = 4.5 up)
    quick-GELU x sigmoid(1.702 x)                      caught                      1 577 (as erf) / 1 887 (as tanh)
    hard-swish for SiLU                                caught                      2 885
    missing 1/2: max(x, 0) - 2 |x| Q; 2 x sigmoid(2u)  caught                      32 461 / 48 414
    SiLU on exp2(-x) (log2 e missing)                  caught                      2 653
    GEGLU halves swapped                               caught                      64 223 .. 65 107 of 65 280 pairs
    GEGLU with the other gate function                 PASSES                      174 / 338 pairs at value 1, 177 / 347 at value -3
    GEGLU without the pre-rounding (family P)          PASSES                      14 514 (erf) / 17 264 (tanh) of 32 640 elements
    A & S coefficient off by 1e-9                      PASSES                      NONE: below the approximation's own 0.75e-7, inside the bound by design
    timestep: sin | cos; frequency over half - 1       caught                      all but 0 .. 15; 56 .. 67 % of the elements

The last but one row is there so that nobody mistakes the bound for bit-exactness: it pins the function, the gate, the halves and the rounding points, not the
last bit.  (A coefficient error shows from about 3e-4: 1e-4 reaches 0.9998 of the bound, 3e-4 is refused at 8 to 16 inputs, 1e-3 at 580 to 800.)"""
import math

import torch

import gemm_exact as X

REL = 2.0 ** -8 + 2.0 ** -14
FLOOR = 2.0 ** -126
NPAT = 65280
FNS = ("gelu_tanh", "gelu_erf", "silu")
GEGLU_VALUES = (1.0, -3.0)           # output = act(gate) itself; a product that rounds


# ---------------------------------------------------------------------------------------------- bit patterns
def finite_bits():
    """the 65 280 finite bf16 bit patterns, ascending, int64"""
    b = torch.arange(65536, dtype=torch.int64)
    return b[(b & 0x7f80) != 0x7f80]


def bits_to_bf16(bits):
    """integers in [0, 65536) -> the bf16 tensor with those bits"""
    b = bits.to(torch.int64)
    return torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(torch.bfloat16)


def bf16_to_bits(t):
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xffff


# ---------------------------------------------------------------------------------------------- fp64 references and the bound
def ref_gelu_erf(x):
    return x * (0.5 * torch.special.erfc(-x / math.sqrt(2.0)))


def ref_gelu_tanh(x):
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


def ref_silu(x):
    return x * torch.sigmoid(x)


REF = {"gelu_tanh": ref_gelu_tanh, "gelu_erf": ref_gelu_erf, "silu": ref_silu}
A_TERM = {"gelu_erf": lambda x: 1e-7 * x.abs(), "gelu_tanh": lambda x: (x.abs() + 1.0) * 2.0 ** -125, "silu": lambda x: (x.abs() + 1.0) * 2.0 ** -125}
_TABLES = {}


def table(fn, device="cpu"):
    """-> (want [65536], A [65536]) fp64 indexed by the bf16 bit pattern of the argument; NaN at the 256 non-finite patterns.  Computed once per device"""
    key = (fn, str(device))
    if key not in _TABLES:
        x = bits_to_bf16(torch.arange(65536)).double()
        fin = torch.isfinite(x)
        xs = torch.where(fin, x, torch.zeros_like(x))
        nan = torch.full_like(x, float("nan"))
        _TABLES[key] = (torch.where(fin, REF[fn](xs), nan).to(device), torch.where(fin, A_TERM[fn](xs), nan).to(device))
    return _TABLES[key]


def bound_of(want, a):
    return REL * want.abs() + a + FLOOR


OVERFLOW = (2.0 - 2.0 ** -8) * 2.0 ** 127      # from here on bf16 round-to-nearest gives infinity (the largest bf16 number plus half a step)


def ratio_of(got, want, bound):
    """error / bound per element.  A NaN result counts as infinite.  An infinite result is right (0) where the reference, give or take the bound, reaches the
    magnitude at which bf16 rounding overflows -- GEGLU's -3 x gelu(gate) beyond 1.13e38 -- and infinite anywhere else"""
    g = got.double()
    err = (g - want).abs()
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err) / bound
    inf_ok = torch.isinf(g) & (torch.sign(g) == torch.sign(want)) & (want.abs() + bound >= OVERFLOW)
    return torch.where(inf_ok, torch.zeros_like(r), r)


def judge(got, arg_bits, fn, value=None):
    """got: the results (any float dtype, bf16 numbers); arg_bits: int64 of got's shape, the bit pattern of the activation's argument; value: None or the
    bf16 value half (fp64, broadcastable).  -> (worst error / bound, number of refused elements, flat index of the worst)"""
    want, a = table(fn, got.device)
    w, aa = want[arg_bits], a[arg_bits]
    if value is not None:
        w, aa = w * value, aa * value.abs()
    assert not torch.isnan(w).any().item(), "a non-finite argument reached the judge"
    ratio = ratio_of(got, w, bound_of(w, aa))
    worst = ratio.max().item()
    return worst, int((ratio > 1.0).sum().item()), int(ratio.flatten().argmax().item())


# ---------------------------------------------------------------------------------------------- host models of the device functions (torch, no FMA)
C1, C2 = 0.7978845608028654, 0.0356774081363001
AS_P, AS_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def model_gelu_tanh(x):
    """gelu_tanh_f / gelu_tanh_f2: x * rcp(1 + exp2(-2 log2(e) x (c1 + c2 x^2)))"""
    t = (x * x) * C2 + C1
    e = torch.exp2(-2.8853900817779268 * (t * x))
    return x * (1.0 / (1.0 + e))


def model_gelu_erf(x, q_scale=1.0, delta=0.0, which=0):
    """gelu_erf_f: max(x, 0) - |x| Q(|x|), Q by A & S 7.1.26 with the 1/2 folded into the coefficients.  q_scale = 2: the mutant without the 1/2;
    delta: added to coefficient `which` of 0.5 P"""
    ax = x.abs()
    t = 1.0 / (ax * (AS_P * 0.7071067811865476) + 1.0)
    c = [0.5 * a for a in AS_A]
    c[which] += delta
    pl = t * c[4] + c[3]
    pl = pl * t + c[2]
    pl = pl * t + c[1]
    pl = pl * t + c[0]
    e = torch.exp2((ax * -0.7213475204444817) * ax)
    q = ((pl * t) * e) * ax
    return torch.clamp(x, min=0.0) - q_scale * q


def model_silu(x):
    return x * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * x)))


MODEL = {"gelu_tanh": model_gelu_tanh, "gelu_erf": model_gelu_erf, "silu": model_silu}


def model_geglu(v, g, fn, preround=True):
    """geglu4 (preround) / ff_fused's geglu_pair (not): fp32 accumulators -> the fp32 product in front of the final rounding"""
    if preround:
        v, g = X.bf(v).float(), X.bf(g).float()
    return v * MODEL[fn](g)


def textbook_tanh(x):
    e = torch.exp(2.0 * (math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))
    return 0.5 * x * (1.0 + (e - 1.0) / (e + 1.0))


# name -> (fp32 function of x, the reference it is judged against)
MUTANTS = {
    "tanh_as_erf": (model_gelu_tanh, "gelu_erf"),
    "erf_as_tanh": (model_gelu_erf, "gelu_tanh"),
    "textbook_tanh": (textbook_tanh, "gelu_tanh"),
    "quick_gelu_as_erf": (lambda x: x * torch.sigmoid(1.702 * x), "gelu_erf"),
    "quick_gelu_as_tanh": (lambda x: x * torch.sigmoid(1.702 * x), "gelu_tanh"),
    "hard_swish": (lambda x: x * torch.clamp(x + 3.0, 0.0, 6.0) / 6.0, "silu"),
    "erf_missing_half": (lambda x: model_gelu_erf(x, q_scale=2.0), "gelu_erf"),
    "tanh_missing_half": (lambda x: 2.0 * model_gelu_tanh(x), "gelu_tanh"),
    "silu_missing_log2e": (lambda x: x * (1.0 / (1.0 + torch.exp2(-x))), "silu"),
}
CLOSE_PASSES = {"tanh_as_erf": True, "erf_as_tanh": True, "textbook_tanh": True, "quick_gelu_as_erf": False, "quick_gelu_as_tanh": False, "hard_swish": False,
                "erf_missing_half": False, "tanh_missing_half": False, "silu_missing_log2e": False}


def normal_samples(n=1 << 20, seed=3):
    return X.bf(torch.randn(n, generator=X.gen(seed, n))).float()


# ---------------------------------------------------------------------------------------------- one-hot delivery through a GEMM
def onehot_unary(M, N, K):
    """-> (a_bits [M, K] int64, w [N, K] fp32 one-hot, P).  Column c < P = min(K, N) of row m holds pattern (m P + c) mod 65 280, the rest +0; W row n picks
    column n mod P: every other product is finite x 0, so the accumulator of output (m, n) is the pattern a_bits[m, n mod P] exactly.  All patterns occur
    when M P >= 65 280 (asserted)"""
    P = min(K, N)
    assert M * P >= NPAT, (M, N, K)
    fb = finite_bits()
    a = torch.zeros(M, K, dtype=torch.int64)
    a[:, :P] = fb[(torch.arange(M).view(-1, 1) * P + torch.arange(P).view(1, -1)) % NPAT]
    w = torch.zeros(N, K)
    n = torch.arange(N)
    w[n, n % P] = 1.0
    return a, w, P


def onehot_geglu(M, N, K):
    """-> (a_bits [M, K], w [N, K] in chunk(2) order [value rows | gate rows], P, values [N / 2]).  Columns c < P = min(K - 2, N / 4) hold the gate patterns,
    column K - 2 holds 1.0 and K - 1 holds -3.0; output j has the gate of column j mod P and the value of column K - 2 + (j div P) mod 2, so every gate
    column meets both values (N / 2 >= 2 P).  The rows go through ops.geglu_interleave"""
    inner = N // 2
    P = min(K - 2, inner // 2)
    assert M * P >= NPAT and inner >= 2 * P, (M, N, K)
    fb = finite_bits()
    a = torch.zeros(M, K, dtype=torch.int64)
    a[:, :P] = fb[(torch.arange(M).view(-1, 1) * P + torch.arange(P).view(1, -1)) % NPAT]
    a[:, K - 2], a[:, K - 1] = 0x3f80, 0xc040
    j = torch.arange(inner)
    which = (j // P) % 2
    w = torch.zeros(N, K)
    w[j, K - 2 + which] = 1.0
    w[inner + j, j % P] = 1.0
    return a, w, P, torch.tensor(GEGLU_VALUES, dtype=torch.float64)[which]


# ---------------------------------------------------------------------------------------------- family P: accumulators that are not bf16 numbers
_F = (1.0, 1.0 + 2.0 ** -7, 1.0 - 2.0 ** -8)      # lo / (half a step of hi): an exact tie, just above, just below -- each a bf16 number


def half_step_lo(hi, g):
    """lo = s f 2^(e - 8) for hi = +-m 2^e (1 <= m < 2), s = +-1 and f drawn from _F: at and beside half a bf16 step of hi"""
    e = torch.floor(torch.log2(hi.abs()))
    s = (torch.randint(0, 2, hi.shape, generator=g) * 2 - 1).float()
    return s * torch.tensor(_F)[torch.randint(0, 3, hi.shape, generator=g)] * torch.exp2(e - 8.0)


def family_p(shape, seed=0):
    """-> (hi, lo) fp32 of `shape`: hi = +-(1 + k / 128) 2^e (k < 128, e in -2 .. 2: a bf16 number), lo = half_step_lo(hi): a bf16 number too, and hi + lo is
    exact in fp32 (17 significant bits) but not a bf16 number"""
    g = X.gen(seed, 77, *shape)
    k = torch.randint(0, 128, shape, generator=g).float()
    e = torch.randint(-2, 3, shape, generator=g).float()
    sh = (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    hi = sh * (1.0 + k / 128.0) * torch.exp2(e)
    lo = half_step_lo(hi, g)
    assert X.bf16_exact(hi) and X.bf16_exact(lo) and torch.equal((hi + lo).double(), hi.double() + lo.double())
    return hi, lo


def family_p_gemm(M, N, K, seed=0):
    """family P through a bf16 GEMM with the GEGLU epilogue: two ones in every W row.  A's columns are four quarters of q = K / 4 -- value hi | value lo |
    gate hi | gate lo; output j (of N / 2) adds columns j mod q of the first two for its value and of the last two for its gate.
    -> (a [M, K] fp32, w [N, K] in chunk(2) order, v [M, N / 2] fp64, g [M, N / 2] fp64: the accumulators)"""
    q, inner = K // 4, N // 2
    vh, vl = family_p((M, q), seed)
    gh, gl = family_p((M, q), seed + 1)
    a = torch.cat([vh, vl, gh, gl], dim=1)
    j = torch.arange(inner)
    w = torch.zeros(N, K)
    w[j, j % q] = w[j, q + j % q] = 1.0
    w[inner + j, 2 * q + j % q] = w[inner + j, 3 * q + j % q] = 1.0
    return a, w, (vh + vl).double()[:, j % q], (gh + gl).double()[:, j % q]


def family_p_bias(M, inner, seed=0, frac=8):
    """family P as bias + one product (the e4m3 GEMM, frac = 8: hi = +-(1 + k / 8) 2^e is an e4m3 number at any power-of-two row scale; ff_fused, frac = 128):
    the exponent e is one per column, so that lo -- which rides in the bias, one per column -- sits at half a bf16 step of every hi of its column.
    -> (hi_v [M, inner], lo_v [inner], hi_g [M, inner], lo_g [inner]) fp32"""
    g = X.gen(seed, 78, M, inner)
    out = []
    for _ in range(2):
        k = torch.randint(0, frac, (M, inner), generator=g).float()
        e = torch.randint(-2, 3, (1, inner), generator=g).float()
        sh = (torch.randint(0, 2, (M, inner), generator=g) * 2 - 1).float()
        hi = sh * (1.0 + k / frac) * torch.exp2(e)
        out += [hi, half_step_lo(torch.exp2(e[0]), g)]
    return out


def geglu_want(v, g, fn, preround):
    """fp64 accumulators -> (want, A) of one contract: preround = geglu4's bf16(value) * act(bf16(gate)), else the product of the accumulators themselves.  The
    rounded gate is a bf16 number and goes through the table; the unrounded one through the reference itself"""
    v, g = v.double(), g.double()
    if preround:
        v, g = X.bf16_rne(v), X.bf16_rne(g)
    return v * REF[fn](g), A_TERM[fn](g) * v.abs()


def judge_p(got, v, g, fn, preround):
    """-> (worst error / bound, refused) of got against one GEGLU contract on family P accumulators"""
    w, a = geglu_want(v, g, fn, preround)
    ratio = ratio_of(got, w, bound_of(w, a))
    return ratio.max().item(), int((ratio > 1.0).sum().item())


# ---------------------------------------------------------------------------------------------- timestep embedding
TS_T = (0.0, 1e-4, 0.5, 1.0, 20.0, 481.0, 961.37, 999.0, 1000.0)
TS_DIMS = (64, 256, 320, 1280)
LN1E4 = 9.210340371976184


def timestep_ref(t32, dim):
    """t32 fp32 [B] -> (want [B, dim], bound [B, dim]) fp64: cos | sin of arg = t f_j, f_j = exp(z_j), z_j = -ln(1e4) j / half.
    Bound (2^-8 + 2^-14) |want| + |arg| (|z| + 2) 2^-22: the kernel forms z in fp32 -- the constant, its product with j and the division round, 3 x 2^-24 |z|
    -- then expf (<= 2 ulp) and the product with t (1 ulp): a relative (3 |z| + 3) 2^-24 on arg, which moves cos and sin by at most that times |arg|;
    (|z| + 2) 2^-22 = (4 |z| + 8) 2^-24 leaves the rest to cosf / sinf themselves"""
    half = dim // 2
    z = -LN1E4 * torch.arange(half, dtype=torch.float64, device=t32.device) / half
    arg = t32.double().view(-1, 1) * torch.exp(z).view(1, -1)
    want = torch.cat([torch.cos(arg), torch.sin(arg)], dim=1)
    slack = arg.abs() * (z.abs().view(1, -1) + 2.0) * 2.0 ** -22
    return want, REL * want.abs() + torch.cat([slack, slack], dim=1)


def timestep_model(t32, dim, mutant=None):
    """timestep_embedding_kernel in fp32.  Mutants: "sin_cos" (the halves swapped), "half_minus_one" (the frequency divided by half - 1)"""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float32)
    den = float(half - 1 if mutant == "half_minus_one" else half)
    f = torch.exp((torch.tensor(-LN1E4, dtype=torch.float32) * j) / den)
    arg = t32.view(-1, 1) * f.view(1, -1)
    parts = [torch.cos(arg), torch.sin(arg)]
    return X.bf(torch.cat(parts[::-1] if mutant == "sin_cos" else parts, dim=1))


# ---------------------------------------------------------------------------------------------- the shapes of the GPU file (M, N, K); the builders assert that every pattern occurs
TILE128, TILE128_GEGLU = (1020, 64, 64), (1056, 256, 64)        # 1 020 x 64 = 65 280 outputs: each pattern once; GEGLU: 62 gate columns x 1 056 rows
WAVE8 = X.WAVE8[0]                                              # 200 tiles at K = 192: the 8-wave 256x256 tile, staged and direct
WIDE320 = X.WIDE320[1]                                          # (7 181, 1 600, 192): the 256x320 tile as shipped
STREAMK = X.STREAMK
W4_K320, W4_GELU = X.W4[0], (6144 + 77, 2048, 1536)             # the four-wave kernel: GEGLU from K = 320, GELU tanh from K = 1 536
SKINNY = X.SKINNY[0]
K320_GEGLU = (16384 + 37, 2560, 320)                            # where gemm_k320_kernel's GEGLU form would run were it dispatched
QUANT_N = 65536                                                 # the quantised GEMMs: all patterns (and 256 zeros) in one bias
