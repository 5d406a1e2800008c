"""Inputs for unmasked attention whose exact result is known, so that ONE key counted twice, dropped or let in from padding shows (helper, not collected;
used by test_attn_exact_cpu.py and test_gpu_attention_exact.py).  Nothing here touches a kernel: builders, closed-form / fp64 expected values, the comparator,
the guarded buffers a launch reads and writes, and the fp64 "mutant" references with which the host-side tests prove that the comparator can fail.

Family A -- every key counted exactly once.  All keys of a (batch, head) are +1 in every feature, all queries are q0 in every feature: every score of a row is
the same number s = D * q0 * scale, the softmax is exactly uniform whatever roundings Q' and P take (they are common to all keys of a row), and with the 0 / 1
indicator V of `v_pattern` the result is O[., d] = n_d / L in closed form (n_d keys carry feature d, L keys in all).  P is one value for every key, fp32 sums of
at most 2^16 copies of an 8-bit value are exact, so the only rounding is the bf16 output: |got - n_d / L| <= 2^-8 (n_d / L).  That is bf16's round-to-nearest
bound itself, not twice it: bf16 keeps 8 significant bits, so values in [2^e, 2^(e+1)) are 2^(e-7) apart and a perfect kernel is off by up to half of that, 2^(e-8) --
which is 2^-8 / (1 + 2^-8) = 0.9961 of the bound at the worst value, 2^e (1 + 2^-8).  The fp32 steps before it (out_scale / l, the product: 2^-24 each) add
2^-15 of the bound, so a perfect kernel always meets it, by a margin of 0.4 % rather than a factor 2; a single key moves a feature by 4 bounds or more
(`sensitivity_a`).  With a fused residual the kernels form fl(fl(o * fl(out_scale / l)) + resid) in fp32 before that rounding: three roundings of 2^-24,
which matter only where the two terms cancel (resid = -1/2 against feature D - 1's 1/2), so the bound on the sum gains 2^-22 |out_scale n_d / L|.

Family B -- every row, head and batch routed, K paired with its own V.  K is uniform +-1, Q[b, r, h] = 6 K[b_kv, pi(r), h]: with scale 8 / D the target key
scores 48 nats and every other key is far below (the leak 1 - p_target is asserted below 2^-12 on the fp64 reference), V[b_kv, j, h] is a bf16-exact code of
(b_kv, h, j).  Expected value: the fp64 softmax on the same bf16 inputs; bound 2^-8 |want| + 2^-11, one bf16 ulp plus twice the asserted leak."""
import math

import torch

LOG2E = 1.4426950408889634
GUARD = 64                      # guard rows before and after each (batch, sequence) of K / V: K = 0 (scores 0 against -20 / -90 nats), V = V_GUARD
V_GUARD = 1000.0                # bf16-exact
SENTINEL = -768.0               # bf16-exact; what the output buffer holds outside the result
ULP = 2.0 ** -8
LEAK = 2.0 ** -12
Q0_LEVELS = (0.0, -2.5, -11.25)  # s = 8 q0 = 0, -20, -90 nats at scale 8 / D; all bf16-exact
C_B = 6.0
MAX_KEYS_A = 1900               # the longest key set of family A
# what one miscounted key must move its features by, relative (sensitivity_a).  The issue behind these tests asks for 4 x 2^-8 and names 1 900 keys as within
# it; at 1 900 keys (n = 62) the move is 1838 / (62 * 1901) = 3.992 x 2^-8 -- 4 holds up to 1 889 keys.  What the floor protects needs more than 2: the kernel's
# own bound plus the mutant's
MIN_MOVE_A = 3.99 * ULP


def bf(x):
    return x.to(torch.bfloat16)


def bf16_exact(t):
    """every value of the fp32 / fp64 tensor is a bf16 number"""
    return torch.equal(t.to(torch.bfloat16).to(t.dtype), t)


# ---------------------------------------------------------------------------------------------- family A
def moduli(D):
    return D // 2 - 1, D // 2 + 1


def v_pattern(L, D=64):
    """[L, D] of 0 / 1: feature d < m1 where j % m1 == d; m1 <= d < D - 1 where j % m2 == d - m1; feature D - 1 everywhere ((m1, m2) = (31, 33) at D = 64).  Two
    moduli so that a 64-key stage used twice while another is skipped cannot cancel: a shift by 64 moves both residues."""
    m1, m2 = moduli(D)
    j, d = torch.arange(L)[:, None], torch.arange(D)[None]
    return (((d < m1) & (j % m1 == d)) | ((d >= m1) & (d < D - 1) & (j % m2 == d - m1)) | (d == D - 1)).float()


def counts(L, D=64):
    """n_d in closed form (no pattern is materialised): keys j < L with j % m == r number ceil((L - r) / m)"""
    m1, m2 = moduli(D)
    n = [max(0, -(-(L - d) // m1)) for d in range(m1)] + [max(0, -(-(L - r) // m2)) for r in range(D - 1 - m1)] + [L]
    return torch.tensor(n, dtype=torch.float64)


def family_a(B, H, Sq, Skv, q0, D=64, kv_div=1):
    q = torch.full((B, Sq, H, D), float(q0))
    k = torch.ones(B // kv_div, Skv, H, D)
    v = v_pattern(Skv, D)[None, :, None, :].expand(B // kv_div, Skv, H, D).contiguous()
    assert bf16_exact(q) and bf16_exact(k) and bf16_exact(v)
    return bf(q), bf(k), bf(v)


def expected_a(B, H, Sq, Skv, D=64):
    """[B, Sq, H * D] fp64: n_d / L for every row, head and batch"""
    return (counts(Skv, D) / Skv).repeat(H).expand(B, Sq, H * D).clone()


def sensitivity_a(L, D=64):
    """the smallest relative move of a feature when one of its keys is counted twice, (n + 1) / (L + 1) against n / L (a dropped key moves it further); one
    key has nothing to be told from, so L >= 2"""
    n = counts(L, D)[:D - 1]
    n = n[n > 0]
    return ((L - n) / (n * (L + 1))).min().item()


def check_shape_a(L, D=64):
    assert L <= MAX_KEYS_A, L
    assert L < 2 or sensitivity_a(L, D) >= MIN_MOVE_A, (L, D, sensitivity_a(L, D))


# ---------------------------------------------------------------------------------------------- family B
def must_keys(Skv, boundaries=()):
    """the keys a launch with fewer rows than keys must still aim rows at: both ends of the first, the second and the slid-back last 64-key tile, and both
    sides of every key-split chunk boundary"""
    ks = {0, 63, 64, Skv - 65, Skv - 64, Skv - 1}
    for b in boundaries:
        ks |= {b - 1, b}
    return sorted(j for j in ks if 0 <= j < Skv)


def pi_map(B, H, Sq, Skv, boundaries=()):
    """[B, H, Sq] target key of every row: affine in the row with a step coprime to Skv and an offset per (b, h) -- onto the keys where Sq >= Skv.  Otherwise
    the first and the last rows of every (b, h) (rows of the first, full, and of the last, ragged, query tile) are aimed at `must_keys`, rotated by (b, h)"""
    step = max(1, int(0.618 * Skv))
    while math.gcd(step, Skv) != 1:
        step += 1
    r = torch.arange(Sq)
    bh = torch.arange(B)[:, None] * H + torch.arange(H)[None]
    pi = (step * r[None, None] + 17 * bh[..., None] + 1) % Skv
    if Sq >= Skv:
        assert all(len(set(pi[b, h].tolist())) == Skv for b in range(B) for h in range(H))
        return pi
    must = torch.tensor(must_keys(Skv, boundaries))
    n = min(len(must), Sq // 2)
    for i in range(n):
        tgt = must[(i + bh) % len(must)]
        pi[:, :, i] = tgt
        pi[:, :, Sq - 1 - i] = tgt
    if n * B * H >= len(must):            # enough rows across the launch: every such key is hit from the first rows and from the last rows
        want = set(must.tolist())
        assert set(pi[:, :, :n].flatten().tolist()) >= want and set(pi[:, :, Sq - n:].flatten().tolist()) >= want
    return pi


def v_code(Bkv, Skv, H, D=64):
    """[Bkv, Skv, H, D] fp32, bf16-exact, no two rows alike: bits of j in features 0-11, of h in 12-15 (and 20-23 from 16 heads up), of b_kv in 16-19; the
    other features from {-1, -1/2, 0, 1/2, 1} as a function of (j, d, h)"""
    assert Skv <= 4096 and H <= 256 and Bkv <= 16 and D >= 32
    b, j, h, d = torch.arange(Bkv)[:, None, None, None], torch.arange(Skv)[None, :, None, None], torch.arange(H)[None, None, :, None], torch.arange(D)[None, None, None]
    v = ((3 * j + 5 * d + 7 * h) % 5 - 2).float() / 2
    v = torch.where(d < 12, ((j >> d.clamp(max=11)) & 1).float(), v)
    v = torch.where((d >= 12) & (d < 16), ((h >> (d - 12).clamp(0, 3)) & 1).float(), v)
    v = torch.where((d >= 16) & (d < 20), ((b >> (d - 16).clamp(0, 3)) & 1).float(), v)
    v = torch.where((d >= 20) & (d < 24), ((h >> (d - 16).clamp(4, 7)) & 1).float(), v)
    return v.contiguous()


def family_b(B, H, Sq, Skv, D=64, kv_div=1, seed=0, boundaries=(), pi=None):
    """-> q, k, v (bf16) and pi [B, H, Sq].  `pi`: a map of the caller's (the packed sequences build theirs per sequence)"""
    g = torch.Generator().manual_seed(1000 * Skv + Sq + seed)
    Bkv = B // kv_div
    k = (torch.randint(0, 2, (Bkv, Skv, H, D), generator=g) * 2 - 1).float()
    v = v_code(Bkv, Skv, H, D)
    if pi is None:
        pi = pi_map(B, H, Sq, Skv, boundaries)
    kq = k.repeat_interleave(kv_div, dim=0).permute(0, 2, 1, 3)                       # [B, H, Skv, D]
    q = (C_B * torch.gather(kq, 2, pi[..., None].expand(B, H, Sq, D))).permute(0, 2, 1, 3).contiguous()
    assert bf16_exact(q) and bf16_exact(k) and bf16_exact(v)
    return bf(q), bf(k), bf(v), pi


def ref64(q, k, v, scale, kv_div=1, pi=None):
    """fp64 softmax(scale q k^T) v on [B, S, H, D] tensors (on their device, one batch at a time) -> [B, Sq, H * D] and, with `pi`, the worst off-target
    weight 1 - p[pi(r)] of the launch"""
    B, Sq, H, D = q.shape
    out = torch.empty(B, Sq, H * D, dtype=torch.float64, device=q.device)
    leak = 0.0
    for b in range(B):
        qb, kb, vb = (t[i].double().permute(1, 0, 2) for t, i in ((q, b), (k, b // kv_div), (v, b // kv_div)))
        p = torch.softmax(qb @ kb.transpose(-1, -2) * scale, dim=-1)
        out[b] = (p @ vb).permute(1, 0, 2).reshape(Sq, H * D)
        if pi is not None:
            tgt = pi[b].to(q.device)[..., None]
            leak = max(leak, (p.sum(dim=-1) - torch.gather(p, 2, tgt)[..., 0]).max().item())
    return out, leak


# ---------------------------------------------------------------------------------------------- packed variable-length sequences
def packed_a(lengths, H, q0):
    """family A over packed sequences -> q, k, v [T, H, 64] and the closed form [T, H * 64]: n_d and L are per sequence, j is the key's index inside its own"""
    T = sum(lengths)
    q, k = torch.full((T, H, 64), float(q0)), torch.ones(T, H, 64)
    v = torch.cat([v_pattern(L)[:, None, :].expand(L, H, 64) for L in lengths if L > 0])
    want = torch.cat([(counts(L) / L).repeat(H).expand(L, H * 64) for L in lengths if L > 0])
    assert bf16_exact(q) and bf16_exact(v)
    return bf(q), bf(k), bf(v.contiguous()), want.clone()


def packed_b(lengths, H, seed=0):
    """family B over packed sequences: pi stays inside the row's own sequence (and is onto it); V codes (sequence, h, j) -> q, k, v [T, H, 64], the fp64
    expected value [T, H * 64] and the worst leak"""
    qs, ks, vs, wants, leak = [], [], [], [], 0.0
    code = v_code(len(lengths), max(lengths), H)
    for i, L in enumerate(lengths):
        if L == 0:
            continue
        q, k, _, pi = family_b(1, H, L, L, seed=seed + i)
        v = bf(code[i:i + 1, :L])
        want, lk = ref64(q, k, v, 0.125, pi=pi)
        leak = max(leak, lk)
        qs.append(q[0]); ks.append(k[0]); vs.append(v[0]); wants.append(want[0])
    return torch.cat(qs), torch.cat(ks), torch.cat(vs), torch.cat(wants), leak


def packed_qkv(q, k, v, dev):
    """q / k / v [T, H, 64] as views of one fused [GUARD + T + GUARD, 3, H, 64] buffer: zero K and V_GUARD V before the first and after the last sequence
    (between sequences the neighbours are the guards: their keys carry other counts and codes)"""
    T, H, D = q.shape
    buf = torch.zeros(T + 2 * GUARD, 3, H, D, dtype=torch.bfloat16, device=dev)
    buf[:, 2] = V_GUARD
    for i, t in enumerate((q, k, v)):
        buf[GUARD:GUARD + T, i] = t
    return tuple(buf[GUARD:GUARD + T, i] for i in range(3))


# ---------------------------------------------------------------------------------------------- comparator
def worst(got, want, rel=ULP, abs_=0.0, extra=None):
    """max over EVERY element of |got - want| / (rel |want| + abs_ [+ extra]); an element with a zero bound must be met exactly"""
    dev = got.device if got.is_cuda else want.device          # where the larger operand already is
    got, want = got.detach().to(dev).double(), want.detach().to(dev).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    err = (got - want).abs()
    tol = rel * want.abs() + abs_
    if extra is not None:
        tol = tol + extra.to(dev).double()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return ratio.max().item()


def passes(got, want, **kw):
    return worst(got, want, **kw) <= 1.0


def check(got, want, what="", **kw):
    w = worst(got, want, **kw)
    assert w <= 1.0, f"{what}: worst error {w:.4g} times its bound"
    return w


TOL_A = dict(rel=ULP, abs_=0.0)
TOL_B = dict(rel=ULP, abs_=2.0 ** -11)


def resid_values(B, Sq, HD, seed=3):
    """multiples of 1/4 in [-2, 2]: resid + out_scale * (0 or 1) stays a bf16 number"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 9, (B, Sq, HD), generator=g).float() / 4)


# ---------------------------------------------------------------------------------------------- mutants (fp64 references of a kernel that miscounts)
KEY_MUTANTS = ("drop_last", "dup_m64", "pad_zero", "stage_twice")


def mutate_keys(k, v, kind):
    """(k, v) as a kernel with the named mistake would see them; None where the key set is too short for it
       drop_last    key Skv - 1 dropped
       dup_m64      key Skv - 64 counted twice (the first key of the slid-back last tile)
       pad_zero     one zero-K / zero-V padding key appended
       stage_twice  64-key stage 1 consumed twice and stage 2 skipped (a ring off-by-one)"""
    Skv = k.shape[1]
    if kind == "drop_last":
        return (k[:, :-1], v[:, :-1]) if Skv > 1 else None
    if kind == "dup_m64":
        j = max(Skv - 64, 0)
        return torch.cat([k, k[:, j:j + 1]], 1), torch.cat([v, v[:, j:j + 1]], 1)
    if kind == "pad_zero":
        return torch.cat([k, torch.zeros_like(k[:, :1])], 1), torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    if kind == "stage_twice":
        if Skv < 192:
            return None
        k2, v2 = k.clone(), v.clone()
        k2[:, 128:192], v2[:, 128:192] = k[:, 64:128], v[:, 64:128]
        return k2, v2
    raise ValueError(kind)


ROUTE_MUTANTS = ("next_key", "next_head", "own_batch")


def mutate_routing(v, kind, kv_div=1):
    """V as a kernel would pair it with the scores if it took the row's value from key pi(r) + 1, from head h + 1, or (-> a per-QUERY-batch V, to be used with
    kv_div 1) from K / V batch b % Bkv where the launch says b // kv_div"""
    if kind == "next_key":
        return torch.roll(v, -1, dims=1)
    if kind == "next_head":
        return torch.roll(v, -1, dims=2)
    if kind == "own_batch":
        Bkv = v.shape[0]
        return v[torch.arange(Bkv * kv_div) % Bkv]
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------- guarded buffers
def guarded_kv(k, v, dev):
    """K and V [Bkv, Skv, H, D] as views of [Bkv, GUARD + Skv + GUARD, H, D] buffers: guard K rows zero, guard V rows V_GUARD"""
    Bkv, Skv, H, D = k.shape
    kb = torch.zeros(Bkv, Skv + 2 * GUARD, H, D, dtype=torch.bfloat16, device=dev)
    vb = torch.full((Bkv, Skv + 2 * GUARD, H, D), V_GUARD, dtype=torch.bfloat16, device=dev)
    kb[:, GUARD:GUARD + Skv] = k
    vb[:, GUARD:GUARD + Skv] = v
    return kb[:, GUARD:GUARD + Skv], vb[:, GUARD:GUARD + Skv]


def fused_qkv(q, k, v, dev):
    """q / k / v as strided views of one [B, GUARD + S + GUARD, 3, H, D] buffer (Sq == Skv, one K / V set per batch)"""
    B, S, H, D = q.shape
    assert k.shape == q.shape and v.shape == q.shape
    buf = torch.zeros(B, S + 2 * GUARD, 3, H, D, dtype=torch.bfloat16, device=dev)
    buf[:, :, 2] = V_GUARD
    for i, t in enumerate((q, k, v)):
        buf[:, GUARD:GUARD + S, i] = t
    return tuple(buf[:, GUARD:GUARD + S, i] for i in range(3))


def temporal_qkv(q, k, v, dev):
    """the (t, hw) row order the UNets' temporal transformers hand over: q a permuted view of [Sq, B, H, D], k / v of one [GUARD + Skv + GUARD, Bkv, 2, H, D]"""
    Bkv, Skv, H, D = k.shape
    qb = q.to(dev).permute(1, 0, 2, 3).contiguous()
    kv = torch.zeros(Skv + 2 * GUARD, Bkv, 2, H, D, dtype=torch.bfloat16, device=dev)
    kv[:, :, 1] = V_GUARD
    kv[GUARD:GUARD + Skv, :, 0] = k.to(dev).permute(1, 0, 2, 3)
    kv[GUARD:GUARD + Skv, :, 1] = v.to(dev).permute(1, 0, 2, 3)
    return qb.permute(1, 0, 2, 3), kv[GUARD:GUARD + Skv, :, 0].permute(1, 0, 2, 3), kv[GUARD:GUARD + Skv, :, 1].permute(1, 0, 2, 3)


ROW_PAD, COL_PAD = 8, 32


class OutBuffer:
    """the result [B, Sq, HD] as a view of a larger SENTINEL-filled buffer (8 rows and 32 columns on every side; `temporal`: rows ordered (t, hw)); `fill`: what
    the view holds before the launch (a residual added in place)"""

    def __init__(self, B, Sq, HD, dev, fill=None, temporal=False):
        shape = (Sq + 2 * ROW_PAD, B, HD + 2 * COL_PAD) if temporal else (B, Sq + 2 * ROW_PAD, HD + 2 * COL_PAD)
        self.buf = torch.full(shape, SENTINEL, dtype=torch.bfloat16, device=dev)
        inner = self.buf[ROW_PAD:ROW_PAD + Sq, :, COL_PAD:COL_PAD + HD] if temporal else self.buf[:, ROW_PAD:ROW_PAD + Sq, COL_PAD:COL_PAD + HD]
        self.temporal = temporal
        self.view = inner.permute(1, 0, 2) if temporal else inner
        if fill is not None:
            self.view.copy_(fill)

    def guards_intact(self):
        """rows and columns outside the result still hold the sentinel"""
        rest = self.buf.clone()
        (rest[ROW_PAD:-ROW_PAD, :, COL_PAD:-COL_PAD] if self.temporal else rest[:, ROW_PAD:-ROW_PAD, COL_PAD:-COL_PAD]).fill_(SENTINEL)
        return bool((rest == SENTINEL).all())
