"""Inputs for the two softmax kernels that work on a MATERIALISED score matrix -- ip_attn_folded_kernel (ops.ip_attn_folded_) and softmax_rows_kernel
(ops.softmax_rows) -- whose exact result is known, so that ONE key or column counted twice, dropped, misrouted or let in from padding shows (helper, not
collected; used by test_softmax_exact_cpu.py and test_gpu_softmax_exact.py).  Nothing here touches a kernel: builders, closed-form / fp64 expected values, the
bounds, the guarded buffers a launch reads and writes, fp32 emulations of the kernels' rounding points and the fp64 "mutant" references with which the host-side
tests prove that every check can fail.  bf / bf16_exact / SENTINEL / the comparator are attn_exact.py's.

ip_attn_folded: hidden[b, r, h, :] += out_scale * softmax(scale * scores[b, r, h, :keys]) . V[b // kv_div, :, h, :]

  Family A -- every key counted once.  All valid scores of a launch are one level c (0, +48, -20, -90 nats at scale 1/8): sv - m is exactly 0 and every P
  exactly 1 whatever the level (the levels show a missing max subtraction, as overflow or l = 0).  V is the 0 / 1 pattern of `ip_v_pattern`, the residual
  r a multiple of 1/4 with |r| <= 1/4: the result is r + out_scale n_d / keys in closed form, and (derivation in attn_exact.py's header: one bf16 rounding of
  the sum, three fp32 roundings in front of it that matter where the two terms cancel) |got - want| <= 2^-8 |want| + 2^-22 |out_scale n_d / keys|.
  Blind by design: to the score of a padding slot at the +48-nat level (a slot at score 0 is then e^-48 down: the other three levels are for it), and on
  feature 63, which every key carries, to a doubled or dropped key (it is there for a padding slot: keys / (keys + 1)).

  Family B -- every row, head and batch routed.  Row r of head h aims at key pi(b, h, r), which scores T; every other valid key scores T - 384, 48 nats
  lower.  V holds integer codes in [1, 63] (ip_v_code: why not 0), the residual integers in [-32, 31], out_scale is 1 (or 0.5 with even codes): the leak is <= 31 e^-48 < 2^-64, l
  rounds to 1 in fp32, the accumulator is the target's V row up to 2^-60, r + V an integer below 256 -- the result is judged with torch.equal.  Blind by design:
  to a doubled first key or a padding slot at score 0 (both 24 nats or more below the target unless they ARE the target: a doubled target changes nothing
  either), and at out_scale 1 to out_scale applied to the residual.  Family A counts, family B routes.

  Family G -- the generic softmax: scores randn * 24 in bf16 (+-9 nats), V and residual randn, against the fp64 softmax of the same bf16 inputs under
  2^-8 |want| + 2^-8 out_scale sum_k p_k |v_kd| + 2^-20 (|r| + out_scale sum_k p_k |v_kd|): the bf16 rounding of the output; the bf16 rounding of each P
  (<= 2^-8 relative each) against a row sum l taken from the UNROUNDED exponentials, so those errors do not cancel; the fp32 steps and the hardware exp2.
  A derived worst case without margin.

softmax_rows: y[r, :] = softmax(scale * x[r, :]), scale = 512^-0.5 (as an fp32 number: the kernel's argument)

  Family C -- every column counted once.  Row r has the 24 columns (24 r + i) mod cols at level T, the others at T - 1088 (bf16-exact, 48 nats lower), and
  there are ceil(cols / 24) rows: every column is a high one in some row.  Expected: the fp64 softmax (1/24 on the high columns), bound
  2^-8 (1 + 2^-10) want + 2^-40: the bf16 rounding; the fp32 row sum's at most ceil(cols / 256) + 8 roundings, the reciprocal and the product (2^-10 of a bf16
  ulp is 2^-18: 64 fp32 roundings); 2^-40 for exponentials the hardware flushes.  A column missed or doubled in the sum is 1/24 against 1/25 (1/23): 4 %.
  Family P -- the max finds every column: one column j* at T = 1024, the rest T - 1088; expected 1 at j* (same bound: the same arithmetic, one high column).
  A softmax does not care which pivot is subtracted as long as nothing overflows, and fp32 holds e^48 = 2^69: at this gap a max that missed j* gives the RIGHT
  result, so families C and P at 48 nats are blind to every max mutant.  The rows `far=True` adds are the same peaks over T - 3072 (136 nats, 2^196): there
  a pivot that missed j* makes exp2 overflow, the row sum is inf and the row is 0 / NaN.  The max mutants below carry fp32's exponent range for that reason.
  Family G -- randn * 6 / scale in bf16 against the fp64 softmax under (2^-8 + 2^-16) want + 2^-40; derivation at TOL_SM_G.  The family that notices a
  scale applied twice or not at all (C and P are blind to it: 48 or 1088 nats down, a low column is under 2^-40 either way)."""
import math

import torch

from attn_exact import SENTINEL, ULP, bf, bf16_exact, check, passes, worst  # noqa: F401  (re-exported for the two test files)

LOG2E = 1.4426950408889634
NAN = float("nan")
D = 64
GUARD_ROWS = 64                 # sentinel rows in front of and behind `hidden`


def f32(x):
    """one fp32 rounding (round to nearest even) of an fp64 tensor, back in fp64"""
    return x.float().double()


def rbf(x):
    """one bf16 rounding of an fp64 tensor whose values are fp32 numbers, back in fp64"""
    return x.float().to(torch.bfloat16).double()


def rejects(got, want, **tol):
    """the comparator refuses `got`: a non-finite value or an element outside its bound"""
    return not bool(torch.isfinite(got).all()) or worst(got, want, **tol) > 1.0


# ============================================================================================== ip_attn_folded
# case: (H, keys, key_stride, B, S, kv_div)
IP_CASES = {
    1: (6, 25, 32, 2, 100, 1),      # ragged second head group (4 + 2 heads); a 36-row tail after one full 64-row group
    2: (3, 25, 26, 4, 77, 2),       # shifts 0, 2, 4; 16-row groups that straddle the two q batches of a K/V batch (154 rows); the clamp at the end of each
    3: (9, 25, 25, 2, 65, 1),       # every shift 0..7; shift 7 puts key 24 in slot 31
    4: (5, 25, 30, 2, 33, 1),       # shifts 0, 6, 4, 2, 0
    5: (4, 32, 32, 1, 17, 1),       # no masked slot
    6: (1, 1, 32, 1, 1, 1),         # p = 1: hidden + out_scale V
    7: (20, 7, 10, 6, 15, 3),
    8: (48, 25, 26, 4, 2711, 1),    # the second trip of the grid-stride loop (ip_grid_x)
    9: (3, 9, 10, 4, 40, 2),        # through the C ABI with hidden_ld = H * 64 + 64
}
IP_G_CASES = (1, 2, 3)
IP_LEVELS = (0.0, 384.0, -160.0, -720.0)     # 0, +48, -20, -90 nats at scale 1/8
IP_SCALE = 0.125
IP_T, IP_GAP = 192.0, 384.0
IP_LEAK = 31.0 * math.exp(-48.0)
IP_OUT_SCALE_A, IP_OUT_SCALE_G = 0.5, 0.75
IP_MODULI = (5, 7, 9)
IP_MIN_MOVE = 4.0                # bounds one miscounted key must move its features by


def ip_admits(H, keys, ks):
    """the entry point's check on the key stride (mrag_ip_attn_folded_bf16): every block's keys fit the 32 slots of the aligned chunks that cover it"""
    return 0 < keys <= ks <= 32 and all(((ks * h) & 7) + keys <= 32 for h in range(min(H, 8)))


def ip_min_width(H, ks, entry="c"):
    """the narrowest score buffer an entry point admits, a multiple of 8: the C ABI asks for the aligned chunk that holds the last block's start plus 32
    columns, ops.ip_attn_folded_ for (H - 1) ks + 32 (more where ks is no multiple of 8)"""
    w = (((H - 1) * ks) & ~7) + 32 if entry == "c" else (H - 1) * ks + 32
    return -(-w // 8) * 8


def ip_grid_x(H, B, S, kv_div, wg_per_cu):
    """workgroups in x and 64-row groups per K/V batch, as the launcher computes them"""
    groups = (kv_div * S + 63) // 64
    per = (256 * wg_per_cu) // (((H + 3) // 4) * (B // kv_div))
    return min(groups, max(per, 1)), groups


def ip_scores_buffer(valid, ks, W):
    """[B, S, W] bf16: key k of head h at column ks h + k, NaN in every other column (slots keys..31 of a block, the gaps between packed blocks, everything
    behind the last block)"""
    B, S, H, keys = valid.shape
    assert W % 8 == 0 and W >= (H - 1) * ks + keys and bf16_exact(valid)
    buf = torch.full((B, S, W), NAN, dtype=torch.bfloat16)
    for h in range(H):
        buf[:, :, ks * h:ks * h + keys] = valid[:, :, h].to(torch.bfloat16)
    return buf


def ip_v_buffer(v, dev):
    """V [Bkv, keys, H, 64] as the [Bkv, keys, H * 64] column block of a NaN-filled [Bkv, keys + 1, H * 64 + 16] buffer: both strides non-trivial multiples of 8"""
    Bkv, keys, H, _ = v.shape
    assert bf16_exact(v)
    buf = torch.full((Bkv, keys + 1, H * D + 16), NAN, dtype=torch.bfloat16, device=dev)
    view = buf[:, :keys, 8:8 + H * D]
    view.copy_(v.reshape(Bkv, keys, H * D))
    assert view.stride(0) != keys * view.stride(1) and view.stride(1) != H * D and view.stride(0) % 8 == 0 and view.stride(1) % 8 == 0
    return view


class Hidden:
    """`hidden` [B, S, H * 64] holding the residual, a slice of a SENTINEL-filled buffer: 64 rows in front and behind, `col_pad` columns behind every row"""

    def __init__(self, resid, dev, col_pad=0):
        B, S, HD = resid.shape
        assert bf16_exact(resid)
        self.buf = torch.full((B * S + 2 * GUARD_ROWS, HD + col_pad), SENTINEL, dtype=torch.bfloat16, device=dev)
        self.rows = self.buf[GUARD_ROWS:GUARD_ROWS + B * S]
        self.inner = self.rows[:, :HD]
        self.inner.copy_(resid.reshape(B * S, HD))
        self.view = self.rows.view(B, S, HD) if col_pad == 0 else None       # contiguous: what ops.ip_attn_folded_ takes
        self.shape, self.ld = (B, S, HD), HD + col_pad

    def result(self):
        return self.inner.reshape(self.shape)

    def guards_intact(self):
        rest = self.buf.clone()
        rest[GUARD_ROWS:-GUARD_ROWS, :self.shape[2]] = SENTINEL
        return bool((rest == SENTINEL).all())


def ip_ref64(sc, v, resid, scale, out_scale, kv_div=1):
    """fp64: resid + out_scale softmax(scale sc) . V -> (want [B, S, H * 64], sum_k p_k |v_kd| [B, S, H * 64], p [B, S, H, keys]); sc [B, S, H, keys] holds the
    valid scores only, v is [Bkv, keys, H, 64].  On the tensors' device"""
    B, S, H, keys = sc.shape
    p = torch.softmax(sc.double() * scale, dim=-1)
    vv = v.double()
    if kv_div != 1:
        vv = vv.repeat_interleave(kv_div, dim=0)
    att = torch.einsum("bshk,bkhd->bshd", p, vv).reshape(B, S, H * D)
    mag = torch.einsum("bshk,bkhd->bshd", p, vv.abs()).reshape(B, S, H * D)
    return resid.double() + out_scale * att, mag, p


def ip_emulate32(sc, v, resid, scale, out_scale, kv_div=1):
    """the kernel's rounding points in fp32 with an exact exp2: sv = fl(s qscale), e = fl(exp2(fl(sv - m))), l = fp32 sum of the UNROUNDED e (eight keys per
    lane in order, then the two lane-group adds), P = bf16(e), the fp32 accumulator of P . V, inv = fl(out_scale / l), bf16(fl(r + fl(acc inv)))"""
    B, S, H, keys = sc.shape
    qscale = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).double()
    sv = f32(sc.double() * qscale)
    e = f32(torch.exp2(f32(sv - sv.amax(dim=-1, keepdim=True))))
    e32 = torch.zeros(B, S, H, 32, dtype=torch.float64)
    e32[..., :keys] = e
    lane = torch.zeros(B, S, H, 4, dtype=torch.float64)
    for i in range(8):
        lane = f32(lane + e32.view(B, S, H, 4, 8)[..., i])
    l = f32(f32(lane[..., 0] + lane[..., 1]) + f32(lane[..., 2] + lane[..., 3]))
    acc = f32(torch.einsum("bshk,bkhd->bshd", rbf(e), v.double().repeat_interleave(kv_div, dim=0)))
    inv = f32(torch.tensor(out_scale, dtype=torch.float32).double() / l)
    return rbf(f32(resid.double().view(B, S, H, D) + f32(acc * inv[..., None]))).reshape(B, S, H * D)


# ---------------------------------------------------------------------------------------------- family A
def ip_v_pattern(Bkv, H, keys):
    """[Bkv, keys, H, 64] of 0 / 1: with j' = key + h + 3 b_kv, feature d < 5 where j' % 5 == d, 5 <= d < 12 where j' % 7 == d - 5, 12 <= d < 21 where
    j' % 9 == d - 12, feature 63 on every key, the others on none: every key carries four features, another set per head and per K/V batch"""
    b, j, h, d = (torch.arange(n).view(s) for n, s in ((Bkv, (-1, 1, 1, 1)), (keys, (1, -1, 1, 1)), (H, (1, 1, -1, 1)), (D, (1, 1, 1, -1))))
    jj = j + h + 3 * b
    v, off = d == D - 1, 0
    for m in IP_MODULI:
        v = v | ((d >= off) & (d < off + m) & (jj % m == d - off))
        off += m
    return v.expand(Bkv, keys, H, D).float().contiguous()


def ip_resid_a(B, S, HD, seed=5):
    g = torch.Generator().manual_seed(seed + S)
    return torch.randint(-1, 2, (B, S, HD), generator=g).float() / 4


def ip_family_a(H, keys, B, S, kv_div, level):
    """-> valid scores [B, S, H, keys], V [Bkv, keys, H, 64], residual [B, S, H * 64] (fp32 holding bf16 numbers)"""
    sc = torch.full((B, S, H, keys), float(level))
    v = ip_v_pattern(B // kv_div, H, keys)
    r = ip_resid_a(B, S, H * D)
    assert bf16_exact(sc) and bf16_exact(v) and bf16_exact(r) and r.abs().max().item() <= 0.25
    return sc, v, r


def ip_expected_a(v, resid, kv_div, out_scale=IP_OUT_SCALE_A):
    """(r + out_scale n_d / keys, the 2^-22 term of the bound), fp64 on resid's device"""
    Bkv, keys, H, _ = v.shape
    att = out_scale * (v.double().sum(dim=1) / keys).reshape(Bkv, 1, H * D).to(resid.device)        # n_d / keys per (b_kv, h)
    if kv_div != 1:
        att = att.repeat_interleave(kv_div, dim=0)
    return resid.double() + att, (2.0 ** -22 * att.abs()).expand(resid.shape)


def ip_sensitivity_a(Bkv, H, keys, out_scale=IP_OUT_SCALE_A):
    """the least number of BOUNDS (at the largest |want| the residual allows, 1/4 + out_scale n / keys) by which a feature moves when one of the keys that
    carry it is counted twice ((n + 1) / (keys + 1) against n / keys; a dropped key moves it further), or when one key k takes V[k + 1] (the zero padding row
    for the last key): every feature carried by one of the two and not by the other moves by out_scale / keys.  Features every key carries have nothing to
    tell a key by (feature 63; all of them at keys = 1): exempt"""
    v = ip_v_pattern(Bkv, H, keys).double()
    n = v.sum(dim=1, keepdim=True).expand_as(v)
    bound = ULP * (0.25 + out_scale * n / keys) + 2.0 ** -22 * out_scale * n / keys
    dup = out_scale * (keys - n) / (keys * (keys + 1)) / bound
    nxt = torch.cat([v[:, 1:], torch.zeros_like(v[:, :1])], dim=1)
    swap = (out_scale / keys) / bound
    worst_dup = dup[(v > 0) & (n < keys)]
    worst_swap = swap[v != nxt]
    return min(worst_dup.min().item() if worst_dup.numel() else math.inf, worst_swap.min().item() if worst_swap.numel() else math.inf)


# ---------------------------------------------------------------------------------------------- family B
def ip_pi(H, keys, B, S, kv_div):
    """[B, S, H] target key: affine in the row g = (b % kv_div) S + r of the K/V batch with a step coprime to `keys`, offset by 16 steps per head and by 7 per
    K/V batch: the first 16 rows of heads h and h + 1 aim at 32 consecutive multiples of the step, i.e. at every key, and so do the last 16 (ip_check_pi)"""
    step = max(1, int(0.618 * keys))
    while math.gcd(step, keys) != 1:
        step += 1
    b, r, h = torch.arange(B).view(-1, 1, 1), torch.arange(S).view(1, -1, 1), torch.arange(H).view(1, 1, -1)
    return (step * ((b % kv_div) * S + r + 16 * h) + 7 * (b // kv_div)) % keys


def ip_check_pi(pi, keys, kv_div, tail_from=None):
    """every key is aimed at from the first 16 and from the last 16 rows of every K/V batch (over its heads), by every head somewhere in the K/V batch where that
    has as many rows as keys, and (tail_from) from the rows past `tail_from` of every batch"""
    B, S, H = pi.shape
    every = set(range(keys))
    per_kv = pi.reshape(B // kv_div, kv_div * S, H)
    for rows in per_kv:
        assert set(rows[:16].flatten().tolist()) == every and set(rows[-16:].flatten().tolist()) == every
        if kv_div * S >= keys:
            assert all(set(rows[:, h].tolist()) == every for h in range(H))
    if tail_from is not None:
        assert all(set(pi[b, tail_from:].flatten().tolist()) == every for b in range(B))


def ip_v_code(Bkv, H, keys, even=False):
    """[Bkv, keys, H, 64] integers in [1, 63] (even ones only: `even`), a fixed pseudo-random code of (b_kv, h, key, d); what makes it a code is checked by
    ip_check_code.  No zeros: where the target's V is 0 the fp32 accumulator holds the other keys' leak, 1e-18, instead of rounding it away against V, and
    with a zero residual a correct kernel returns that rather than 0"""
    g = torch.Generator().manual_seed(64 * keys + H + 1000 * Bkv)
    v = torch.randint(1, 32 if even else 64, (Bkv, keys, H, D), generator=g) * (2 if even else 1)
    return v.float()


def ip_check_code(v):
    """the 64-vectors of any two (b_kv, h, key) differ in at least 32 features, and no two feature columns agree on all of them"""
    rows = v.reshape(-1, D).long()
    onehot = torch.zeros(rows.shape[0], D * 64)
    onehot.scatter_(1, rows + 64 * torch.arange(D), 1.0)
    agree = onehot @ onehot.T
    agree.fill_diagonal_(0)
    assert agree.max().item() <= D - 32, agree.max().item()
    assert torch.unique(rows.T, dim=0).shape[0] == D or rows.shape[0] == 1


def ip_family_b(H, keys, B, S, kv_div, out_scale=1.0):
    """-> valid scores, V, residual, pi and the expected value r + out_scale V[b // kv_div, pi, h] (an integer below 256: exact in bf16)"""
    pi = ip_pi(H, keys, B, S, kv_div)
    sc = torch.where(torch.arange(keys).view(1, 1, 1, -1) == pi[..., None], IP_T, IP_T - IP_GAP)
    v = ip_v_code(B // kv_div, H, keys, even=out_scale != 1.0)
    g = torch.Generator().manual_seed(S + 31 * H)
    r = torch.randint(-32, 32, (B, S, H * D), generator=g).float()
    vq = v.repeat_interleave(kv_div, dim=0).permute(0, 2, 1, 3)                                         # [B, H, keys, 64]
    tgt = torch.gather(vq, 2, pi.permute(0, 2, 1)[..., None].expand(B, H, S, D))                        # [B, H, S, 64]
    want = r.double() + out_scale * tgt.permute(0, 2, 1, 3).reshape(B, S, H * D).double()
    assert bf16_exact(sc) and bf16_exact(v) and bf16_exact(r) and bf16_exact(want) and want.abs().max().item() < 256
    return sc, v, r, pi, want


def ip_leak(p, pi):
    """the worst off-target weight of an fp64 softmax p [B, S, H, keys]"""
    return (1.0 - torch.gather(p, 3, pi.to(p.device)[..., None])).max().item()


# ---------------------------------------------------------------------------------------------- family G
def ip_family_g(H, keys, B, S, kv_div):
    g = torch.Generator().manual_seed(7 * S + H)
    sc = bf(torch.randn(B, S, H, keys, generator=g) * 24).float()
    v = bf(torch.randn(B // kv_div, keys, H, D, generator=g)).float()
    r = bf(torch.randn(B, S, H * D, generator=g)).float()
    return sc, v, r


def ip_tol_g(resid, mag, out_scale=IP_OUT_SCALE_G):
    """the two terms of family G's bound beside 2^-8 |want| (module docstring)"""
    return ULP * out_scale * mag + 2.0 ** -20 * (resid.double().abs() + out_scale * mag)


# ---------------------------------------------------------------------------------------------- mutants
IP_MUTANTS = ("drop_last", "dup_first", "next_key", "next_head", "own_batch", "pad_zero", "feat_swap", "no_resid", "scale_resid")
# family -> the mutants it is blind to by design (module docstring); own_batch needs kv_div > 1, next_head two heads, drop_last / next_key two keys
IP_BLIND = {"A": (), "B": ("dup_first", "pad_zero"), "B1": ("dup_first", "pad_zero", "scale_resid"), "G": ()}


def ip_mutant(kind, sc, v, resid, scale, out_scale, kv_div=1):
    """fp64 restatement of the kernel with one fault -> [B, S, H * 64], or None where the shape has no room for it
       drop_last    key keys - 1 dropped                       dup_first    key 0 counted twice
       next_key     key k paired with V[k + 1] (the zeroed LDS row for the last key)
       next_head    V of head h + 1                            own_batch    V of batch b (mod the K/V batches) instead of b // kv_div
       pad_zero     one padding slot let in at score 0 (its V^T column is zero)
       feat_swap    features 4..7 swapped with 32..35          no_resid / scale_resid   residual left out / multiplied by out_scale too"""
    B, S, H, keys = sc.shape
    Bkv = v.shape[0]
    if kind == "drop_last":
        return ip_ref64(sc[..., :-1], v[:, :-1], resid, scale, out_scale, kv_div)[0] if keys > 1 else None
    if kind == "dup_first":
        return ip_ref64(torch.cat([sc, sc[..., :1]], -1), torch.cat([v, v[:, :1]], 1), resid, scale, out_scale, kv_div)[0]
    if kind == "next_key":
        return ip_ref64(sc, torch.cat([v[:, 1:], torch.zeros_like(v[:, :1])], 1), resid, scale, out_scale, kv_div)[0]
    if kind == "next_head":
        return ip_ref64(sc, torch.roll(v, -1, dims=2), resid, scale, out_scale, kv_div)[0] if H > 1 else None
    if kind == "own_batch":
        return ip_ref64(sc, v[torch.arange(B) % Bkv], resid, scale, out_scale, 1)[0] if kv_div > 1 and Bkv > 1 else None
    if kind == "pad_zero":
        return ip_ref64(torch.cat([sc, torch.zeros_like(sc[..., :1])], -1), torch.cat([v, torch.zeros_like(v[:, :1])], 1), resid, scale, out_scale, kv_div)[0]
    if kind == "feat_swap":
        perm = torch.arange(D)
        perm[4:8], perm[32:36] = torch.arange(32, 36), torch.arange(4, 8)
        return ip_ref64(sc, v[..., perm], resid, scale, out_scale, kv_div)[0]
    if kind == "no_resid":
        return ip_ref64(sc, v, torch.zeros_like(resid), scale, out_scale, kv_div)[0]
    if kind == "scale_resid":
        return ip_ref64(sc, v, resid.double() * out_scale, scale, out_scale, kv_div)[0]
    raise ValueError(kind)


# ============================================================================================== softmax_rows
SM_SCALE = torch.tensor(512 ** -0.5, dtype=torch.float32).item()       # the product's scale as the fp32 number the kernel is handed
SM_COLS = (1, 5, 8, 96, 100, 2048, 2052, 2056, 9216)
SM_LEVELS = (0.0, 1024.0, -2048.0)
SM_HIGH = 24
SM_GAP, SM_GAP_FAR = 1088.0, 3072.0        # 48 and 136 nats at SM_SCALE; T - gap is a bf16 number for every level used (asserted by the builders)
SM_T_P = 1024.0
SM_G_ROWS = 8
TOL_SM_C = dict(rel=ULP * (1 + 2.0 ** -10), abs_=2.0 ** -40)
# Family G's bound, (2^-8 + 2^-16) want + 2^-40.  The kernel forms e_j = exp2(t_j), t_j = fl(x_j k - mk) (one fma rounding) with k = fl(scale log2 e) and the
# pivot mk = fl(fl(max scale) log2 e).  Whatever error mk carries multiplies EVERY e_j of the row by one factor and leaves e_j / sum e alone.  What does not
# cancel, as relative errors of e_j (p_j's error is e_j's minus the p-weighted mean of the row's): k's rounding, |x_j scale| 2^-24 <= 2^-18 at |x scale| <= 64,
# so 2^-17 between two columns; the fma's rounding of t_j -- an element with p_j < 2^-24 is within the 2^-40 term whatever happens to it, the others have
# |t_j| < 64 and round by at most 2^-19 log2-units = 0.69 x 2^-19, twice (its own and the mean's); the fp32 row sum's ceil(cols / 256) + 8 <= 44 roundings,
# 2^-18.5; exp2, the reciprocal and the product, a few 2^-24.  In all 2^-17 (1 + 0.35 + 0.36 + 0.1) < 2^-16, in front of ONE bf16 rounding (2^-8).
TOL_SM_G = dict(rel=ULP + 2.0 ** -16, abs_=2.0 ** -40)


def sm_family_c(cols, T):
    """[ceil(cols / 24), cols]: row r holds T in the 24 columns (24 r + i) mod cols (every column where cols <= 24), T - 1088 elsewhere"""
    rows = -(-cols // SM_HIGH)
    x = torch.full((rows, cols), T - SM_GAP)
    idx = (SM_HIGH * torch.arange(rows)[:, None] + torch.arange(SM_HIGH)[None]) % cols
    x.scatter_(1, idx, T)
    assert bf16_exact(x) and bool((x == T).any(dim=0).all())                     # every column is a high one in some row
    return x


def sm_peaks(cols):
    """the columns family P puts its peak at, one row each: both ends of the first thread's first vector, of wave 0's / the workgroup's first sweep (63 * 8,
    64 * 8 - 1, 64 * 8, 2047, 2048, 2055), the last nine columns, and every position of the scalar tail"""
    js = {0, 7, 8, 63 * 8, 64 * 8 - 1, 64 * 8, 2047, 2048, 2055} | set(range(cols - 9, cols)) | set(range(cols - cols % 8, cols))
    return sorted(j for j in js if 0 <= j < cols)


def sm_family_p(cols, far=False):
    """-> x [len(peaks), cols] (T = 1024 at the row's peak, T - 1088 -- `far`: T - 3072 -- elsewhere) and the peaks"""
    js = sm_peaks(cols)
    x = torch.full((len(js), cols), SM_T_P - (SM_GAP_FAR if far else SM_GAP))
    x[torch.arange(len(js)), torch.tensor(js)] = SM_T_P
    assert bf16_exact(x)
    return x, js


def sm_family_g(cols):
    g = torch.Generator().manual_seed(cols)
    x = bf(torch.randn(SM_G_ROWS, cols, generator=g) * (6.0 / SM_SCALE)).float()
    assert (x.abs() * SM_SCALE).max().item() <= 64.0                              # what TOL_SM_G's derivation assumes
    return x


def sm_ref64(x, scale=SM_SCALE):
    return torch.softmax(x.double() * scale, dim=-1)


def sm_lds(cols):
    """the two row strides of the tests: the tightest the entry point admits (a multiple of 8: `cols` itself where it is one) and that plus 8"""
    tight = -(-cols // 8) * 8
    return tight, tight + 8


class Rows:
    """x [rows, cols] and the result buffer as slices of [1 + rows + 1, ld] buffers: one guard row in front and behind, ld - cols padding columns.  Out of
    place x's guards and padding are NaN and y is all SENTINEL; in place (y is x) they are SENTINEL.  Whatever is not the result must keep the sentinel"""

    def __init__(self, x, ld, inplace, dev):
        rows, cols = x.shape
        assert bf16_exact(x) and ld % 8 == 0 and ld >= cols
        self.xbuf = torch.full((rows + 2, ld), SENTINEL if inplace else NAN, dtype=torch.bfloat16, device=dev)
        self.x = self.xbuf[1:1 + rows, :cols]
        self.x.copy_(x)
        self.ybuf = self.xbuf if inplace else torch.full((rows + 2, ld), SENTINEL, dtype=torch.bfloat16, device=dev)
        self.y = self.ybuf[1:1 + rows, :cols]
        self.cols = cols

    def guards_intact(self):
        rest = self.ybuf.clone()
        rest[1:-1, :self.cols] = SENTINEL
        return bool((rest == SENTINEL).all())


def sm_emulate32(x, scale=SM_SCALE):
    """softmax_rows_kernel's rounding points in fp32 with an exact exp2, sums in the kernel's order: thread tid takes the 8-column vectors tid, tid + 256, ...
    and tail column 8 (cols // 8) + tid, a butterfly over the 64 lanes of a wave, ((w0 + w1) + w2) + w3, fl(1 / sum), bf16(fl(e inv))"""
    rows, cols = x.shape
    s32, l2e = torch.tensor(scale, dtype=torch.float32), torch.tensor(LOG2E, dtype=torch.float32)
    k = (s32 * l2e).double()
    mk = f32(f32(x.double().amax(dim=1, keepdim=True) * s32.double()) * l2e.double())
    e = f32(torch.exp2(f32(x.double() * k - mk)))                                # fma: one rounding of the exact x k - mk (fp64 holds it exactly)
    c8 = cols // 8
    sweeps = -(-c8 // 256)
    body = torch.zeros(rows, sweeps * 256 * 8, dtype=torch.float64)
    body[:, :c8 * 8] = e[:, :c8 * 8]
    body = body.view(rows, sweeps, 256, 8)
    acc = torch.zeros(rows, 256, dtype=torch.float64)
    for s in range(sweeps):
        for i in range(8):
            acc = f32(acc + body[:, s, :, i])
    tail = cols - c8 * 8
    acc[:, :tail] = f32(acc[:, :tail] + e[:, c8 * 8:])
    acc = acc.view(rows, 4, 64)
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = f32(acc + acc[:, :, lanes ^ o])
    w = acc[:, :, 0]
    inv = f32(1.0 / f32(f32(f32(w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]))
    return rbf(f32(e * inv[:, None]))


SM_MUTANTS = ("tail_unsummed", "dup_col0", "max_body_only", "max_first_wave", "no_scale", "tail_unwritten")
# family -> the mutants it is blind to by design (module docstring).  "Pfar" sees a max mutant where a peak lies outside the columns the mutant looks at,
# G sees a column miscounted in the sum only through that column's weight (not asserted), C and the P families no missing scale
SM_BLIND = {"C": ("max_body_only", "max_first_wave", "no_scale"), "P": ("max_body_only", "max_first_wave", "no_scale", "tail_unsummed"),
            "Pfar": ("no_scale", "tail_unsummed"), "G": ("tail_unsummed", "dup_col0", "max_body_only", "max_first_wave")}


def sm_mutant(kind, x, prev, scale=SM_SCALE):
    """fp64 restatement of softmax_rows with one fault -> [rows, cols], or None where the row length has no room for it.  `prev`: what the result buffer held
    before the launch (the sentinel, or x itself in place).  exp2 carries fp32's exponent range (2^128 and above is inf), which is how a wrong pivot shows
       tail_unsummed   the cols % 8 tail columns left out of the sum          dup_col0         column 0 counted twice
       max_body_only   max over the first cols // 8 * 8 columns only          max_first_wave   max over the columns of wave 0 only
       no_scale        scale not applied                                      tail_unwritten   the last tail column not written"""
    rows, cols = x.shape
    body = cols // 8 * 8
    if kind == "no_scale" and cols == 1:
        return None                                                               # one column is 1 at any scale
    xs = x.double() * (1.0 if kind == "no_scale" else scale)
    seen = torch.ones(cols, dtype=torch.bool)
    if kind == "max_body_only":
        if body == cols or body == 0:
            return None
        seen[body:] = False
    if kind == "max_first_wave":
        seen = (torch.arange(cols) // 8) % 256 < 64
        seen[body:] = True                                                        # the tail's threads 0..6 are wave 0's
        if bool(seen.all()):
            return None
    t = (xs - xs[:, seen].amax(dim=1, keepdim=True)) * LOG2E
    e = torch.where(t >= 128.0, torch.full_like(t, math.inf), torch.exp2(t.clamp(max=127.0)))
    total = e.sum(dim=1, keepdim=True)
    if kind == "tail_unsummed":
        if body == cols:
            return None
        total = e[:, :body].sum(dim=1, keepdim=True)
    if kind == "dup_col0":
        total = total + e[:, :1]
    out = e * (1.0 / total)
    if kind == "tail_unwritten":
        if body == cols:
            return None
        out[:, -1] = prev.double()[:, -1]
    return out
