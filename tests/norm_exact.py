"""Inputs for LayerNorm / GroupNorm whose statistics are known exactly, so that ONE 16-byte vector, pixel row, chunk or channel left out of (or counted twice
in) a statistics reduction shows (helper, not collected; used by test_norm_exact_cpu.py and test_gpu_norm_exact.py).  Nothing here touches a kernel: builders,
fp64 references, the bounds, fp32 host models of the kernels' statistics forms and of kernels with a named mistake ("mutants").

A "unit" is what one set of statistics covers: a LayerNorm row (M = D elements) or a GroupNorm (sample, group) (M = HW * C / G elements).

Family A -- one spike per unit.  The background is seeded +-1; one element of the unit is +-A or +-2A with A the power of two nearest sqrt(3 M).  Every value
is a bf16 number and every sum and sum of squares is an integer below 2^24 (multiples of 1/64 below 2^18 with an `emb`), so fp32 accumulation is exact in any
order: whatever differs from the fp64 normalisation of the same input beyond the fp32 chain behind the sums (division, rsqrt, products: a few 2^-24) and the bf16
rounding of the result is a mistake.  The spike carries 3/4 (A) or 12/13 (2A) of the variance: a spike left out of the statistics moves every background output of
the unit by sqrt(1 + A^2 / M): a factor 1.6 to 2.6 (A) or 2.6 to 5 (2 A); one counted twice or a wrong M by more than 20 %.  Neighbouring units differ in the spike's sign and in A against 2A (by the
parity of the row, of n + g), so another unit's statistics show.  gamma = sign(c) 2^((c mod 5) - 2) with sign(c) = -1 where c mod 3 == 1 differs for every
channel of an 8-vector and for channels 8 apart, beta = 0: a misrouted channel shows and the result stays one product away from the normalised value.
Bound: |got - want| <= (2^-8 + 2^-14) |want| -- bf16's round-to-nearest bound plus 2^-14 for the fp32 chain and the SiLU's exponential; the background
stays away from zero (`min_background` is asserted), so the bound needs no absolute term.  With SiLU the spike takes the sign of its channel's gamma:
silu of a large negative value is e^-|x| |x|, which has no usable relative bound.

Family B -- offset data.  x = bf16(N(mu, 1)) with |mu| = 8 or 32 per unit, random gamma and beta (and an `emb` of a few sigma for GroupNorm); the reference
is the fp64 normalisation of the rounded inputs.  Bound: 2^-8 |want| + c |gamma x^| with x^ the normalised value (times the modulation's factor where there
is one).  Two-pass LayerNorms: c = 2^-11 = 8 192 * 2^-24, a sequential fp32 sum of the widest row.  GroupNorm (one pass, E[x^2] - mean^2): c = 2^-9; an
fp32 emulation of the kernels' summation order gave a relative rstd error of at most 1e-4 at mu / sigma = 32, a margin of 20 for another order.  At
mu / sigma = 128 (mu = 32, sigma = 1/4) the one-pass form loses log2(128^2) = 14 of fp32's 24 bits; the measured figure is recorded in DESIGN.md.
A third term, 2^-16 |gamma mean rstd|, is what fp32 itself asks for and the first two lack: the mean is an fp32 number, off by its own rounding and by that of the
sum behind it, and where x is within a few 2^-20 |mean| of the mean (x^ ~ 0: some element of every few rows) that error is all of x - mean, which neither
|want| nor |gamma x^| scales with -- the fp32 models below miss the two-term bound by a factor 3.6 on such elements.  2^-16 = 256 * 2^-24: no chain of fp32
additions behind a sum is longer than 256 at the tested shapes (LayerNorm: 128 per lane and 6 shuffles; GroupNorm: at most 40 pixels, 32 row groups, 72 chunks
and 80 channels), so the sum, and with it the mean, is within 256 roundings whatever the order.  At mu / sigma = 32 that is 5e-4 of a normalised unit."""
import math

import torch

ULP = 2.0 ** -8
REL_A = 2.0 ** -8 + 2.0 ** -14
C_LN = 2.0 ** -11
C_GN = 2.0 ** -9
C_MEAN = 2.0 ** -16
RSTD_128_MEASURED = 2.11e-3       # GroupNorm at mu / sigma = 128 on the MI355X: worst relative error of rstd over the four shapes, 0.54 x 2^-8
C_GN_128 = 4 * RSTD_128_MEASURED  # = 2.2 x 2^-8
EPS = 1e-5
MIN_BACKGROUND = 0.04            # floor of the normalised background of family A: 0.044 at D = 8 and 0.066 at 64 (the spike moves the mean by half a unit), 0.15 and more from D = 320 up


def bf(x):
    return x.to(torch.bfloat16)


def bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).to(t.dtype), t)


def spike_amp(M):
    """the power of two nearest sqrt(3 M) (nearest in the exponent)"""
    return 2.0 ** round(math.log2(math.sqrt(3.0 * M)))


def gamma_pattern(C):
    c = torch.arange(C)
    return torch.where(c % 3 == 1, -1.0, 1.0) * 2.0 ** ((c % 5) - 2).float()


def _gen(*key):
    s = 12345
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _pm1(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


# ---------------------------------------------------------------------------------------------- LayerNorm inputs
def ln_spike_cols(rows, D):
    """row r probes 8-vector r mod (D / 8) at its element (3 r) mod 8"""
    r = torch.arange(rows)
    return (r % (D // 8)) * 8 + (3 * r) % 8


def ln_family_a(rows, D, seed=0, amp=None):
    """-> x [rows, D] fp32 (bf16-exact).  Row r: sign (-1)^r, amplitude A (even r) or 2 A (odd r)"""
    A = float(amp or spike_amp(D))
    assert (2 * A) ** 2 + D < 2 ** 24
    x = _pm1((rows, D), _gen(rows, D, seed))
    r = torch.arange(rows)
    x[r, ln_spike_cols(rows, D)] = A * (1 + r % 2).float() * (1 - 2 * (r % 2)).float()
    assert bf16_exact(x)
    return x


def ln_family_b(rows, D, seed=0, ratio=None):
    """-> x [rows, D] fp32 = bf16(N(mu_r, sigma)), gamma, beta [D] fp32 (bf16 values).  |mu| / sigma = 8, 32 by the row's parity, the sign by r // 2; `ratio` = 128:
    mu = +-32, sigma = 1/4 in every row"""
    g = _gen(rows, D, seed, 77)
    r = torch.arange(rows)
    if ratio is None:
        mu, sigma = torch.where(r % 2 == 0, 8.0, 32.0) * (1 - 2 * ((r // 2) % 2)).float(), 1.0
    else:
        mu, sigma = 32.0 * (1 - 2 * (r % 2)).float(), 32.0 / ratio
    x = bf(torch.randn(rows, D, generator=g) * sigma + mu[:, None]).float()
    return x, bf(torch.randn(D, generator=g)).float(), bf(torch.randn(D, generator=g)).float()


def adaln_rows(rows, rows_per_batch, split, mod):
    """mod [B, 4, D] = (shift0, scale0, shift1, scale1) per sample -> (shift, scale) [rows, D] as the kernels pick them: position < split takes pair 0"""
    r = torch.arange(rows)
    b, pos = r // rows_per_batch, r % rows_per_batch
    first = (pos < split)[:, None]
    return torch.where(first, mod[b, 0], mod[b, 2]), torch.where(first, mod[b, 1], mod[b, 3])


def adaln_pow2(B, D, seed=0):
    """[B, 4, D] fp32: shifts +-8 / +-64, 1 + scale = 1/2 or 2 -- powers of two, different per sample, pair and channel"""
    g = _gen(B, D, seed, 5)
    sh = (1 - 2 * torch.randint(0, 2, (B, 2, D), generator=g)).float() * torch.where(torch.randint(0, 2, (B, 2, D), generator=g) == 0, 8.0, 64.0)
    sc = torch.where(torch.randint(0, 2, (B, 2, D), generator=g) == 0, -0.5, 1.0)
    return torch.stack([sh[:, 0], sc[:, 0], sh[:, 1], sc[:, 1]], dim=1)


# ---------------------------------------------------------------------------------------------- GroupNorm inputs
def gn_chunks(N, HW):
    """statistics chunks per sample as ops.groupnorm sets them (the GPU tests assert that the two agree)"""
    return max(1, min(1024, HW // 32, max(64, -(-2048 // N))))


def gn_rpps(C):
    """pixel rows per pass of gn_stats_kernel in each 2 048-channel segment"""
    return [256 // (min(2048, C - off) // 8) for off in range(0, C, 2048)]


def gn_probe_pixels(HW, C, chunks):
    """the pixels a spike must sit on, most wanted first: the sample's last pixel; chunk 0's first and last row-group; the first and the last pixel of the
    4-way unrolled loop's remainder in the first and in the last chunk; then the first and the last pixel of every chunk, from both ends inwards"""
    ppc = -(-HW // chunks)
    nonempty = -(-HW // ppc)
    px = [HW - 1]
    for rpp in gn_rpps(C):
        px += [0, min(rpp, ppc, HW) - 1]
        for k in (0, nonempty - 1):
            rem = [k * ppc + o for o in range(min(ppc, HW - k * ppc)) if _in_remainder(o, min(ppc, HW - k * ppc), rpp)]
            px += rem[:1] + rem[-1:]
    order = []
    for i in range((nonempty + 1) // 2):
        order += [i, nonempty - 1 - i]
    for k in order:
        px += [k * ppc, min(HW, (k + 1) * ppc) - 1]
    return list(dict.fromkeys(px))


def _in_remainder(o, L, rpp):
    """pixel o of a chunk of L pixels is summed by the one-at-a-time loop behind the 4-way unrolled one: thread row-group o % rpp owns n = ceil((L - rsub) / rpp)
    pixels and unrolls the first 4 (n // 4) of them"""
    rsub, i = o % rpp, o // rpp
    n = -(-(L - rsub) // rpp)
    return i >= 4 * (n // 4)


def gn_family_a(N, HW, C, G, chunks=None, seed=0, silu=False, gamma=None, pixels=None):
    """-> x [N, HW, C] fp32 (bf16-exact) and the spike pixel of every unit [N, G].  Unit (n, g): parity (n + g) % 2 picks sign and A / 2 A; its spike sits on
    `pixels` (default gn_probe_pixels) dealt to the units in a scattered order, pseudo-random pixels once they run out, in channel g cpg + (unit mod cpg).
    silu: the spike takes the sign of its channel's gamma"""
    cpg = C // G
    A = spike_amp(HW * cpg)
    assert (2 * A) ** 2 + HW * cpg < 2 ** 24
    g_ = _gen(N, HW, C, seed)
    x = _pm1((N, HW, C), g_)
    must = list(pixels if pixels is not None else gn_probe_pixels(HW, C, chunks or gn_chunks(N, HW)))
    units = N * G
    step = next(s for s in range(max(1, int(0.618 * units)), 2 * units + 2) if math.gcd(s, units) == 1)
    where = torch.empty(N, G, dtype=torch.long)
    for i in range(units):
        u = (i * step + 1) % units
        n, g = divmod(u, G)
        px = must[i] if i < len(must) else int(torch.randint(0, HW, (1,), generator=g_))
        c = g * cpg + u % cpg
        par = (n + g) % 2
        sign = (1.0 if gamma is None or gamma[c] > 0 else -1.0) if silu else 1.0 - 2.0 * par
        x[n, px, c] = sign * A * (1 + par)
        where[n, g] = px
    assert bf16_exact(x)
    return x, where


def gn_emb_a(N, C, seed=0):
    """[N, C] fp32 from {+-1/8, +-1/4}: the sums stay multiples of 1/64 and the background stays at least 1/2 from the group mean"""
    g = _gen(N, C, seed, 9)
    return (1 - 2 * torch.randint(0, 2, (N, C), generator=g)).float() * torch.where(torch.randint(0, 2, (N, C), generator=g) == 0, 0.125, 0.25)


def gn_family_b(N, HW, C, G, seed=0, ratio=None, emb=False):
    """-> x [N, HW, C] fp32 = bf16(N(mu, sigma)) with mu per (n, group) (|mu| / sigma = 8, 32 by the parity of n + g, sign by g // 2; `ratio` = 128: mu = +-32,
    sigma = 1/4), gamma, beta [C], emb [N, C] of up to 3 sigma or None"""
    g_ = _gen(N, HW, C, seed, 78)
    cpg = C // G
    n, g = torch.arange(N)[:, None], torch.arange(G)[None]
    if ratio is None:
        mu, sigma = torch.where((n + g) % 2 == 0, 8.0, 32.0) * (1 - 2 * ((g // 2) % 2)).float(), 1.0
    else:
        mu, sigma = 32.0 * (1 - 2 * ((n + g) % 2)).float(), 32.0 / ratio
    x = bf(torch.randn(N, HW, C, generator=g_) * sigma + mu.repeat_interleave(cpg, dim=1)[:, None, :]).float()
    gamma, beta = bf(torch.randn(C, generator=g_)).float(), bf(torch.randn(C, generator=g_)).float()
    e = bf((torch.rand(N, C, generator=g_) * 6 - 3) * sigma).float() if emb else None
    return x, gamma, beta, e


def mod_maps(N, Tz, hz, wz, C, seed=0, family="A"):
    """[N, Tz, hz, wz, 2 C] fp32: family A -- scale +- a power of two, constant over the channels of a latent pixel and different per pixel, shift 0;
    family B -- random scale and shift"""
    g = _gen(N, Tz, hz, wz, C, seed)
    if family == "A":
        sc = (1 - 2 * torch.randint(0, 2, (N, Tz, hz, wz, 1), generator=g)).float() * 2.0 ** (torch.randint(0, 4, (N, Tz, hz, wz, 1), generator=g) - 1).float()
        return torch.cat([sc.expand(N, Tz, hz, wz, C), torch.zeros(N, Tz, hz, wz, C)], dim=-1).contiguous()
    return bf(torch.randn(N, Tz, hz, wz, 2 * C, generator=g)).float()


def mod_full(mod, T, H, W, shift, split):
    """the latent-resolution maps through the nearest-neighbour frame / pixel map of CogVideoXSpatialNorm3D -> scale, shift [N, T H W, C]: odd T > 1 (`split`)
    takes frame 0 from latent frame 0 and resamples the rest separately, otherwise floor(t Tz / T)"""
    N, Tz, hz, wz, C2 = mod.shape
    t = torch.arange(T)
    tz = torch.where(t == 0, 0, 1 + ((t - 1) * (Tz - 1)) // max(T - 1, 1)) if split else (t * Tz) // T
    full = mod[:, tz][:, :, torch.arange(H) >> shift][:, :, :, torch.arange(W) >> shift].reshape(N, T * H * W, C2)
    return full[..., :C2 // 2], full[..., C2 // 2:]


# ---------------------------------------------------------------------------------------------- fp64 references
def ln_ref64(x, gamma=None, beta=None, eps=EPS, rms=False, mod=None):
    """-> want, |gamma x^|, |gamma mean rstd| (what the two statistics terms of the family B bound scale with), fp64 [rows, D].  mod = (shift, scale) [rows, D]"""
    x = x.double()
    mean = torch.zeros_like(x[:, :1]) if rms else x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    lin, off = (x - mean) * rstd, (mean * rstd).expand_as(x)
    if gamma is not None:
        lin, off = lin * gamma.double(), off * gamma.double()
    out = lin + beta.double() if beta is not None else lin
    if mod is not None:
        lin, off = lin * (1 + mod[1].double()), off * (1 + mod[1].double())
        out = out * (1 + mod[1].double()) + mod[0].double()
    return out, lin.abs(), off.abs()


def gn_ref64(x, G, gamma=None, beta=None, eps=EPS, emb=None, silu=False, mod=None):
    """x [N, HW, C] -> want, |gamma x^|, |gamma mean rstd| fp64.  emb [N, C] is added before the statistics; mod = (scale, shift) [N, HW, C] at full resolution"""
    N, HW, C = x.shape
    x = x.double() + (emb.double()[:, None] if emb is not None else 0.0)
    xg = x.view(N, HW, G, C // G)
    mean = xg.mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(((xg - mean) ** 2).mean((1, 3), keepdim=True) + eps)
    lin, off = ((xg - mean) * rstd).view(N, HW, C), (mean * rstd).expand_as(xg).reshape(N, HW, C)
    if gamma is not None:
        lin, off = lin * gamma.double(), off * gamma.double()
    out = lin + beta.double() if beta is not None else lin
    if mod is not None:
        lin, off = lin * mod[0].double(), off * mod[0].double()
        out = out * mod[0].double() + mod[1].double()
    return (torch.nn.functional.silu(out) if silu else out), lin.abs(), off.abs()


# ---------------------------------------------------------------------------------------------- comparator
def worst(got, want, rel=REL_A, extra=None, mask=None):
    """max over every element (of `mask`) of |got - want| / (rel |want| [+ extra]); a zero bound must be met exactly"""
    dev = got.device if got.is_cuda else want.device
    got, want = got.detach().to(dev).double(), want.detach().to(dev).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    err = (got - want).abs()
    tol = rel * want.abs()
    if extra is not None:
        tol = tol + extra.to(dev).double()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    if mask is not None:
        ratio = ratio[mask.to(dev)]
    return ratio.max().item()


def worst_a(got, want):
    return worst(got, want, REL_A)


def worst_b(got, want, lin, off, c):
    return worst(got, want, ULP, extra=c * lin + C_MEAN * off)


def check(w, what):
    assert w <= 1.0, f"{what}: worst error {w:.4g} times its bound"
    return w


def min_background(want):
    """the smallest |want| of a family A case: the relative bound needs it away from zero"""
    return want.abs().min().item()


def rstd_fp32(gs, gq, cnt, eps=EPS):
    """the folds' fp32 formula on (sum, sum of squares): mean = s / cnt, var = max(q / cnt - mean^2, 0), rstd = rsqrt(var + eps)"""
    gs, gq = gs.float(), gq.float()
    mean = gs / float(cnt)
    return torch.rsqrt((gq / float(cnt) - mean * mean).clamp_min(0.0) + eps)


def rstd_ref64(x, G, eps=EPS):
    """fp64 rstd per (sample, group) of x [N, HW, C]"""
    N, HW, C = x.shape
    xg = x.double().view(N, HW, G, C // G)
    return 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + eps)


# ---------------------------------------------------------------------------------------------- fp32 host models and mutants
LN_MUTANTS = ("drop_vec", "next_row", "gamma_next_vec")


def ln_model(x, gamma=None, beta=None, eps=EPS, rms=False, mod=None, mutant=None, arg=0):
    """layernorm_kernel's two-pass statistics in fp32 (any summation order: family A's sums are exact) -> bf16.
       drop_vec        8-vector `arg` left out of both passes of every row (the count stays D)
       next_row        row r normalised with the statistics of row r + 1
       gamma_next_vec  gamma / beta of the channel vector behind the right one"""
    assert mutant is None or mutant in LN_MUTANTS
    x = x.float()
    D = x.shape[1]
    keep = torch.ones(D)
    if mutant == "drop_vec":
        keep[8 * arg:8 * arg + 8] = 0
    mean = torch.zeros_like(x[:, :1]) if rms else (x * keep).sum(-1, keepdim=True) / D
    rstd = torch.rsqrt((((x - mean) ** 2) * keep).sum(-1, keepdim=True) / D + eps)
    if mutant == "next_row":
        mean, rstd = mean.roll(-1, 0), rstd.roll(-1, 0)
    if mutant == "gamma_next_vec":
        gamma, beta = (None if t is None else t.roll(-8) for t in (gamma, beta))
    o = (x - mean) * rstd
    if gamma is not None:
        o = o * gamma.float()
    if beta is not None:
        o = o + beta.float()
    if mod is not None:
        o = o * (1 + mod[1].float()) + mod[0].float()
    return bf(o)


GN_MUTANTS = ("drop_last_pixel", "drop_chunk_last", "drop_remainder", "chunk_twice", "stale_empty", "cnt_no_cpg", "cnt_short", "segment_drop", "group_next", "sample_next",
              "gamma_next_vec")
SPLIT_MUTANTS = ("hw_one_shard", "shard_missing")


def gn_group_sums(x, G, chunks, emb=None, mutant=None):
    """gn_stats_kernel + the fold in fp32: per-(n, chunk, channel) partial sum and sum of squares, folded over the chunks, the analytic `emb` terms, then over the
    group's channels -> (sum, sum of squares) [N, G]"""
    x = x.float()
    N, HW, C = x.shape
    cpg = C // G
    ppc = -(-HW // chunks)
    o = torch.arange(chunks * ppc) % ppc
    k = torch.arange(chunks * ppc) // ppc
    L = (HW - k * ppc).clamp(0, ppc)                                      # pixels of this pixel's chunk
    keep = (torch.arange(chunks * ppc) < HW)[:, None].expand(chunks * ppc, C).clone()
    if mutant == "drop_chunk_last":
        keep &= (o != L - 1)[:, None]
    if mutant == "drop_last_pixel":
        keep[HW - 1] = False
    if mutant == "drop_remainder":
        for seg, rpp in enumerate(gn_rpps(C)):
            rsub, i = o % rpp, o // rpp
            n = -(-(L - rsub) // rpp)
            keep[:, seg * 2048:(seg + 1) * 2048] &= (i < 4 * (n // 4))[:, None]
    xp = torch.nn.functional.pad(x, (0, 0, 0, chunks * ppc - HW)) * keep.float()
    xp = xp.view(N, chunks, ppc, C)
    S, Q = xp.sum(2), (xp * xp).sum(2)
    if mutant == "stale_empty":                                          # an empty chunk's partial is never written: what an earlier call left there (here: chunk 0's)
        empty = torch.arange(chunks) * ppc >= HW
        S, Q = torch.where(empty[None, :, None], S[:, :1], S), torch.where(empty[None, :, None], Q[:, :1], Q)
    if mutant == "chunk_twice":
        k2 = min(1, chunks - 1)
        S[:, k2], Q[:, k2] = 2 * S[:, k2], 2 * Q[:, k2]
    cs, cq = S.sum(1), Q.sum(1)
    if emb is not None:
        e = emb.float()
        cq = cq + 2.0 * e * cs + float(HW) * e * e
        cs = cs + float(HW) * e
    if mutant == "segment_drop":                                         # a group that straddles channel 2 048 loses its channels behind it
        c = torch.arange(C)
        g = c // cpg
        lost = (c >= 2048) & (g * cpg < 2048)
        cs, cq = cs * (~lost).float(), cq * (~lost).float()
    return cs.view(N, G, cpg).sum(-1), cq.view(N, G, cpg).sum(-1)


def _gn_apply(x, gs, gq, cnt, G, gamma, beta, eps, emb, silu, mod, mutant):
    N, HW, C = x.shape
    cpg = C // G
    mean = gs / cnt
    rstd = torch.rsqrt((gq / cnt - mean * mean).clamp_min(0.0) + eps)
    if mutant == "group_next":
        mean, rstd = mean.roll(-1, 1), rstd.roll(-1, 1)
    if mutant == "sample_next":
        mean, rstd = mean.roll(-1, 0), rstd.roll(-1, 0)
    ga = gamma.float() if gamma is not None else torch.ones(C)
    be = beta.float() if beta is not None else torch.zeros(C)
    if mutant == "gamma_next_vec":
        ga, be = ga.roll(-8), be.roll(-8)
    e = emb.float() if emb is not None else torch.zeros(N, C)
    a = ga * rstd.repeat_interleave(cpg, 1)
    b = be + (e - mean.repeat_interleave(cpg, 1)) * a
    o = x.float() * a[:, None] + b[:, None]
    if mod is not None:
        o = o * mod[0].float() + mod[1].float()
    return bf(torch.nn.functional.silu(o) if silu else o)


def gn_model(x, G, chunks, gamma=None, beta=None, eps=EPS, emb=None, silu=False, mod=None, mutant=None):
    """mrag_groupnorm_bf16 in fp32: one-pass variance E[x^2] - mean^2 from chunk partials -> bf16, or None where the shape gives the mistake nothing to act on.
       drop_last_pixel   the sample's last pixel left out (the ragged last chunk's clamp off by one)
       drop_chunk_last   the last pixel of every chunk left out (px1 off by one)
       drop_remainder    the pixels behind the 4-way unrolled loop left out
       chunk_twice       one chunk's partial counted twice
       stale_empty       empty chunks hold another call's partial
       cnt_no_cpg        cnt = HW                       cnt_short   cnt = (HW - one chunk's pixels) cpg
       segment_drop      the channels behind 2 048 left out of the group that straddles it
       group_next / sample_next   the statistics of group g + 1 / sample n + 1
       gamma_next_vec    gamma / beta of the channel vector behind the right one in the apply pass"""
    assert mutant is None or mutant in GN_MUTANTS
    N, HW, C = x.shape
    cpg = C // G
    ppc = -(-HW // chunks)
    if (mutant == "cnt_short" and chunks == 1) or (mutant == "stale_empty" and (chunks - 1) * ppc < HW) or \
            (mutant == "segment_drop" and not any(g * cpg < 2048 < (g + 1) * cpg for g in range(G))) or (mutant == "sample_next" and N == 1):
        return None                                                      # the shape has no such chunk, group or sample: the mistake cannot show
    gs, gq = gn_group_sums(x, G, chunks, emb, mutant)
    cnt = float(HW) * cpg
    if mutant == "cnt_no_cpg":
        cnt = float(HW)
    if mutant == "cnt_short":
        cnt = float(HW - -(-HW // chunks)) * cpg
    return _gn_apply(x, gs, gq, cnt, G, gamma, beta, eps, emb, silu, mod, mutant)


def gn_split_model(shards, G, gamma=None, beta=None, eps=EPS, silu=False, mutant=None):
    """groupnorm_partial per shard + groupnorm_apply_stats with the partials of all shards -> the shards' results, concatenated along the pixels.
       hw_one_shard   hw_total is the shard's own pixel count      shard_missing   the last shard's partial left out of the fold"""
    assert mutant is None or mutant in SPLIT_MUTANTS
    parts = [gn_group_sums(s, G, gn_chunks(s.shape[0], s.shape[1])) for s in shards]
    used = parts[:-1] if mutant == "shard_missing" else parts
    gs, gq = sum(p[0] for p in used), sum(p[1] for p in used)
    cpg = shards[0].shape[2] // G
    total = sum(s.shape[1] for s in shards)
    outs = [_gn_apply(s, gs, gq, float(s.shape[1] if mutant == "hw_one_shard" else total) * cpg, G, gamma, beta, eps, None, silu, None, None) for s in shards]
    return torch.cat(outs, dim=1)


def split_probe_pixels(sizes, C, N):
    """probe pixels of a sharded extent: every shard's own list (its own chunking), shifted to the extent and interleaved, so every shard holds probes"""
    lists, start = [], 0
    for hw in sizes:
        lists.append([start + p for p in gn_probe_pixels(hw, C, gn_chunks(N, hw))])
        start += hw
    out = []
    for i in range(max(len(l) for l in lists)):
        out += [l[i] for l in lists if i < len(l)]
    return list(dict.fromkeys(out))


# ---------------------------------------------------------------------------------------------- the shapes both test files use
def ln_rows(D):
    return max(D // 8, 9)


LN_DIMS = {2: (8, 64, 1024), 4: (1032, 2048), 6: (2056, 3072), 8: (3080, 4096), 16: (4104, 8192)}          # layernorm_kernel<MAXC>: D
LN_ROWS_DIMS, LN_ROWS_ROWS = (320, 640, 1280, 1024), 1029                                                    # layernorm_rows_kernel
LN_STREAM = (8192 + 5, 3072)                                                                                 # layernorm_stream_kernel
# (N, HW, C, G)
GN_SHAPES = [(4, 600, 320, 32), (2, 2304, 64, 32), (1, 40, 2560, 32), (5, 1000, 64, 32)]
GN_RAW = (3, 100, 256, 32)                    # through the C ABI with 64 chunks (14 of them empty) and with 1
GN_SPLIT = (2, (256, 200, 144), 320, 32)      # N, the shards' pixels, C, G
GN_MOD = [(2, (3, 8, 12), 64, 0, True, 2), (2, (5, 16, 8), 128, 1, True, 3)]     # N, (T, H, W), C, shift, split, Tz
