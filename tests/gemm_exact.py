"""Inputs for the GEMM and convolution kernels whose correct output is known bit for bit (helper, not collected; used by test_gemm_exact_cpu.py and
test_gpu_gemm_exact.py).  Nothing here touches a kernel: builders, exact references, fp32 host models of a tiled GEMM / implicit convolution / rotary epilogue
and the same models with one named mistake ("mutants").

With small-integer operands every product and every partial sum is an exact fp32 integer, so the result does not depend on summation order, tile shape, K-split
or stream-K exchange: every kernel must return the bits of the exact reference (torch.equal, no tolerance).

Family A -- no rounding anywhere.  A and W in {-1, 0, +1} (dense for K <= 1024, density 1/4 each above), bias integers in [-8, 8], residual integers in
[-64, 64], gates in {+1, -1, +2, -2} distinct per (sample, segment), acc_scale 1 or 0.5.  Every value at every rounding point is an integer (or a half) below
256 in magnitude, a bf16 number: one lost, doubled or foreign non-zero product changes the output bits.  `overflow_share` measures the condition (at most
0.1 % of the elements reach 256 at a rounding point); the reference rounds explicitly all the same, so the few that do are still exact.
Family R -- rounding points.  Dense +-{1, 2, 3} at K in [512, 2048]: |acc + bias| mostly exceeds 256, partial sums stay below 2^24.  The reference applies
the rounding points of gemm_tile.h (epilogue_direct) in exact arithmetic with round-to-nearest-even written out (`bf16_rne`):
    NONE bf16(acc + bias);  RESID bf16(resid + bf16(acc_scale (acc + bias)));  GATE_RESID bf16(resid + bf16(gate (acc + bias))).
Family T -- tap identification (convolutions).  One-hot weight: output channel co selects tap co % taps of input channel (co // taps) % Cin; activations
((31 n + 7 y + 3 x + c) mod 251) - 125.  The expected output is the named neighbour's value by index arithmetic, 0 outside the image / clip.
Family Q -- quarter-turn RoPE on family A: cos / sin in {0, +-1}, q_premul 0.5, no norm: the expected output is a signed permutation of the exact projection."""
import math

import torch

EPI_NONE, EPI_GELU_TANH, EPI_GELU_ERF, EPI_RESID, EPI_GATE_RESID, EPI_SILU, EPI_GEGLU = 0, 1, 2, 3, 4, 5, 6
SENTINEL = 24576.0          # a bf16 number no case produces: what frames every output block
GATE_VALUES = (1.0, -1.0, 2.0, -2.0)


def bf(x):
    return x.to(torch.bfloat16)


def bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).to(t.dtype), t)


def gen(*key):
    s = 54321
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


_DROP = 45                      # fp64 carries 52 fraction bits, bf16 7


def bf16_rne(v, half_up=False):
    """fp64 -> the nearest bf16 value (8 significant bits), ties to even, as fp64, in integer arithmetic on the bit pattern (sign and magnitude: adding to the
    magnitude bits carries into the exponent as it should): add half a step less one, plus the bit that will be the last, and clear the 45 bits below.  No
    float32 step in between and no floating-point operation, so the host and the device agree.  half_up: the mutant that rounds ties away from zero"""
    bits = v.double().contiguous().view(torch.int64)
    add = (1 << (_DROP - 1)) if half_up else (1 << (_DROP - 1)) - 1 + ((bits >> _DROP) & 1)
    return ((bits + add) & ~((1 << _DROP) - 1)).view(torch.float64)


def is_tie(v):
    """v (fp64) lies exactly half-way between two bf16 numbers"""
    return (v.double().contiguous().view(torch.int64) & ((1 << _DROP) - 1)) == (1 << (_DROP - 1))


# ---------------------------------------------------------------------------------------------- operands
def density(K):
    return 1.0 if K <= 1024 else 0.25


def tri(shape, g, dens):
    """entries in {-1, 0, +1}, non-zero with probability `dens`"""
    s = (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    return s if dens >= 1.0 else s * (torch.rand(shape, generator=g) < dens).float()


def family_a(M, N, K, seed=0, dens=None, bias_lo=-8, a_max=1):
    """-> dict x [M, K], w [N, K], bias [N], resid [M, N] (fp32 tensors of bf16 values).  a_max = 2: A entries in {-2 .. 2} (the fp8 cases).  bias_lo: the
    activation cases draw the bias from [bias_lo, 8]"""
    g = gen(M, N, K, seed)
    d = density(K) if dens is None else dens
    x = tri((M, K), g, d)
    if a_max > 1:
        x = x * torch.randint(1, a_max + 1, (M, K), generator=g).float()
    return dict(x=x, w=tri((N, K), g, d), bias=torch.randint(bias_lo, 9, (N,), generator=g).float(), resid=torch.randint(-64, 65, (M, N), generator=g).float())


def family_r(M, N, K, seed=0):
    """dense +-{1, 2, 3}: |acc| ~ 4.7 sqrt(K).  The bias is family A's times 64, which carries |acc + bias| past 256 (where bf16 steps by 2 and more) on half
    of the elements at any K; the residual is family A's: odd, below the step of the value it meets, so the order of rounding and adding shows"""
    g = gen(M, N, K, seed, 7)
    def mag(shape):
        return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * torch.randint(1, 4, shape, generator=g).float()
    return dict(x=mag((M, K)), w=mag((N, K)), bias=torch.randint(-8, 9, (N,), generator=g).float() * 64, resid=torch.randint(-64, 65, (M, N), generator=g).float())


def family_n(M, N, K, seed=0):
    """the N(0, 1) data of the existing tests (test_gpu_kernels): what the old close() tolerance is measured on"""
    g = gen(M, N, K, seed, 11)
    return dict(x=bf(torch.randn(M, K, generator=g)).float(), w=bf(torch.randn(N, K, generator=g)).float(), bias=bf(torch.randn(N, generator=g)).float(),
                resid=bf(torch.randn(M, N, generator=g)).float())


def gates(B, N):
    """[B, 2, N]: gate0 = [:, 0] (rows in front of `split`), gate1 = [:, 1]; a value of its own per (sample, segment) for B <= 2"""
    v = torch.tensor([GATE_VALUES[(2 * b + s) % 4] for b in range(B) for s in range(2)]).view(B, 2, 1)
    return v.expand(B, 2, N).contiguous()


def gate_rows(gt, M, rpb, split, sample_shift=None, seg_flip=()):
    """[M, N]: the gate of every row.  sample_shift / seg_flip: the mutants' hooks (rows whose sample index is one too small; rows that take the other segment)"""
    m = torch.arange(M, device=gt.device)
    b, pos = m // rpb, m % rpb
    seg = (pos >= split).long()
    if sample_shift is not None:
        b = torch.where(sample_shift.to(gt.device), (b - 1).clamp(min=0), b)
    for r in seg_flip:
        seg[r] = 1 - seg[r]
    return gt[b, seg]


# ---------------------------------------------------------------------------------------------- the exact reference
def acc_exact(x, w):
    """fp64 product of integer operands: exact (every partial sum is an integer far below 2^53).  Runs on the tensors' device"""
    return x.double() @ w.double().t()


def epilogue_ref(acc, bias, epi=EPI_NONE, resid=None, acc_scale=1.0, gate=None, *, resid_first=False, half_up=False, scale_resid=False):
    """acc [M, N] fp64 exact -> the bf16 result as fp64, rounding points of gemm_tile.h.  resid_first / half_up / scale_resid: the mutants"""
    rnd = lambda t: bf16_rne(t, half_up)
    v = acc.double() + (bias.double() if bias is not None else 0.0)
    if epi == EPI_NONE:
        return rnd(v)
    v = v * (gate.double() if epi == EPI_GATE_RESID else acc_scale)
    r = resid.double() * (acc_scale if scale_resid else 1.0)
    return rnd(v + r) if resid_first else rnd(rnd(v) + r)


def rounding_points(acc, bias, epi, resid=None, acc_scale=1.0, gate=None):
    """the values that get rounded (fp64): family A wants them below 256"""
    v = acc.double() + (bias.double() if bias is not None else 0.0)
    if epi == EPI_NONE:
        return [v]
    v = v * (gate.double() if epi == EPI_GATE_RESID else acc_scale)
    return [v, bf16_rne(v) + resid.double()]


def overflow_share(points):
    return max((p.abs() >= 256).double().mean().item() for p in points)


ACT = {
    EPI_GELU_TANH: lambda v: 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3))),
    EPI_GELU_ERF: lambda v: 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0))),
    EPI_SILU: lambda v: v * torch.sigmoid(v),
}


def close_tol(want, rtol=2e-2, atol_frac=2e-2):
    """the tolerance of the existing close() (test_gpu_kernels): 2 % of the element + 2 % of the mean magnitude"""
    return rtol * want.abs() + atol_frac * want.abs().mean()


def passes_close(got, want):
    return bool(((got.double() - want.double()).abs() <= close_tol(want.double())).all())


def act_sensitive_share(v):
    """share of the elements with v >= 1.  The activation cases assert that all elements of one v carry the same bits and that the table v -> bits is strictly
    increasing over v >= 1: an element there whose accumulator is off by one product carries the bits of v +- 1, which differ from its fellows'.  (Below 1 the
    table flattens -- gelu(-1) = -0.16, gelu(-4) = -1e-4, then about 0 -- and neighbours may share bits: those elements are not counted.)"""
    return (v >= 1).double().mean().item()


# ---------------------------------------------------------------------------------------------- fp32 host model of a tiled GEMM
def gemm_model(p, epi=EPI_NONE, *, BM=128, BN=128, WT=64, acc_scale=1.0, gt=None, rpb=0, split=0, pad=8, mutant=None):
    """C = epilogue(x w^T + bias) the way a tiled kernel works, in fp32: operands in row-padded buffers (NaN behind column K), tiles of BM x BN walked in order,
    K in 32-deep steps into an fp32 accumulator, the epilogue per tile with its two bf16 roundings.  `mutant` names one mistake (MUTANTS).  -> fp32 [M, N]"""
    x, w, bias = p["x"], p["w"], p["bias"]
    M, K = x.shape
    N = w.shape[0]
    fill = 3.0 if mutant == "read_past_k" else float("nan")      # the mutant's padding holds finite garbage: a NaN would show anywhere
    xp, wp = torch.full((M, K + pad), fill), torch.full((N, K + pad), fill)
    xp[:, :K], wp[:, :K] = x, w
    out = torch.zeros(M, N)
    tiles = [(m0, n0) for m0 in range(0, M, BM) for n0 in range(0, N, BN)]
    hit = len(tiles) // 2                                        # the tile a one-tile mistake lands in
    rne = lambda t: t.to(torch.bfloat16).float()
    if mutant == "half_up":
        rne = lambda t: bf16_rne(t, half_up=True).float()
    for ti, (m0, n0) in enumerate(tiles):
        m1, n1 = min(m0 + BM, M), min(n0 + BN, N)
        acc = torch.zeros(m1 - m0, n1 - n0)
        steps = list(range(0, K, 32))
        if mutant == "drop_last_kstep" and ti == hit:
            steps = steps[:-1]
        for k0 in steps:
            acc += xp[m0:m1, k0:k0 + 32] @ wp[n0:n1, k0:k0 + 32].t()
        if mutant == "ktile_twice" and ti == hit and ti > 0:     # the first 64-deep K-tile of a tile taken once more at the tile change
            acc += xp[m0:m1, :64] @ wp[n0:n1, :64].t()
        if mutant == "drop_product" and ti == hit:
            nz = (xp[m0, :K] * wp[n0, :K]).nonzero()[0, 0]
            acc[0, 0] -= xp[m0, nz] * wp[n0, nz]
        if mutant == "read_past_k" and ti == hit:                # one element of row m0 from behind K, against the weights' padding
            acc[0, :] += xp[m0, K] * wp[n0:n1, K]
        b = bias[n0:n1].clone()
        if mutant == "bias_next_col":                            # the last column of every wave tile takes its neighbour's bias
            for c in range(WT - 1, n1 - n0, WT):
                if n0 + c + 1 < N:
                    b[c] = bias[n0 + c + 1]
        v = acc + b
        if epi in (EPI_RESID, EPI_GATE_RESID):
            r = p["resid"][m0:m1, n0:n1]
            if epi == EPI_GATE_RESID:
                rows = torch.arange(M)
                shift = (rows % rpb == 0) if mutant == "sample_off_by_one" else None
                flip = [s for b_ in range((M + rpb - 1) // rpb) for s in (b_ * rpb + split - 1, b_ * rpb + split) if s < M] if mutant == "gate_other_segment" else ()
                v = v * gate_rows(gt, M, rpb, split, shift, flip)[m0:m1, n0:n1]
            else:
                v = v * acc_scale
                if mutant == "scale_resid":
                    r = r * acc_scale
            v = rne(v + r) if mutant == "resid_before_round" else rne(rne(v) + r)
        else:
            v = rne(v)
        out[m0:m1, n0:n1] = v
    return out


MUTANTS_A = ("drop_product", "drop_last_kstep", "ktile_twice", "read_past_k", "bias_next_col", "gate_other_segment", "sample_off_by_one", "scale_resid")
MUTANTS_R = ("resid_before_round", "half_up")
MUTANT_EPI = {"gate_other_segment": EPI_GATE_RESID, "sample_off_by_one": EPI_GATE_RESID, "scale_resid": EPI_RESID, "resid_before_round": EPI_RESID,
              "half_up": EPI_RESID}


# ---------------------------------------------------------------------------------------------- convolutions
class Conv:
    """one convolution problem in channels-last layout.  mode "3x3": x [F, H, W, Cin]; stride 1 / 2, upsample (nearest 2x in front), asym_pad (padding
    behind only, stride 2), t_frames = T > 0: causal 3x3x3 over samples of T + 2 input frames.  mode "t3": x [(b t), HW, Cin] as [B T, 1, HW, Cin]"""

    def __init__(self, mode, F, H, W, Cin, Cout, *, stride=1, upsample=False, asym_pad=False, t_frames=0, frames=0):
        self.mode, self.F, self.H, self.W, self.Cin, self.Cout = mode, F, H, W, Cin, Cout
        self.stride, self.upsample, self.asym_pad, self.t_frames, self.frames = stride, upsample, asym_pad, t_frames, frames
        if mode == "3x3":
            self.Hi, self.Wi = (2 * H, 2 * W) if upsample else (H, W)
            self.front = 0 if asym_pad else 1
            self.Ho, self.Wo = (self.Hi + self.front - 2) // stride + 1, (self.Wi + self.front - 2) // stride + 1
            self.taps = 27 if t_frames else 9
            self.Fo = F // (t_frames + 2) * t_frames if t_frames else F
        else:
            self.Ho, self.Wo, self.taps, self.Fo = 1, W, 3, F
        self.M, self.K = self.Fo * self.Ho * self.Wo, self.taps * Cin

    def coords(self, mutant=None):
        """-> (f, y, x, valid), each [M, taps] int64: the input pixel under tap t of output row m, by index arithmetic; invalid = reads zero"""
        m = torch.arange(self.M).view(-1, 1)
        t = torch.arange(self.taps).view(1, -1)
        fo, yo, xo = m // (self.Ho * self.Wo), (m // self.Wo) % self.Ho, m % self.Wo
        if self.mode == "t3":
            b, tt = fo // self.frames, fo % self.frames + t - 1
            valid = (tt >= 0) & (tt < self.frames)
            if mutant == "tap_crosses_clip":                      # the neighbouring frame of the buffer, whichever clip it belongs to
                valid = (fo + t - 1 >= 0) & (fo + t - 1 < self.F)
            return b * self.frames + tt, torch.zeros_like(tt), xo + 0 * t, valid
        kt, ky, kx = (t // 9, (t // 3) % 3, t % 3) if self.t_frames else (0 * t, t // 3, t % 3)
        front = 1 if mutant == "asym_origin" else self.front
        y, x = yo * self.stride + ky - front, xo * self.stride + kx - front
        valid = (y >= 0) & (y < self.Hi) & (x >= 0) & (x < self.Wi)
        if mutant == "border_wraps":                              # a column outside the image is the neighbouring row's pixel, not zero
            valid = (y >= 0) & (y < self.Hi) & (y * self.Wi + x >= 0) & (y * self.Wi + x < self.Hi * self.Wi)
            y, x = (y * self.Wi + x) // self.Wi, (y * self.Wi + x) % self.Wi
        if self.upsample:
            y, x = (((y + 1) // 2, (x + 1) // 2) if mutant == "upsample_off_by_one" else (y // 2, x // 2))
            valid = valid & (y < self.H) & (x < self.W)
        if self.t_frames:
            s, tf = fo // self.t_frames, fo % self.t_frames
            f = s * (self.t_frames + 2) + tf + kt
            if mutant == "causal_next_sample":                    # the two context frames taken from the sample behind
                f = torch.where(tf + kt < 2, ((s + 1) * (self.t_frames + 2) + tf + kt) % self.F, f)
        else:
            f = fo + 0 * t
        return f, y, x, valid

    def rows(self, x, mutant=None):
        """the gathered operand [M, taps * Cin] (what an im2col would hold), zero where a tap falls outside"""
        f, y, xx, valid = self.coords(mutant)
        flat = x.reshape(-1, self.Cin)
        idx = ((f * self.H + y) * self.W + xx).clamp(0, flat.shape[0] - 1).to(x.device)
        return (flat[idx] * valid.unsqueeze(-1).to(x.device, x.dtype)).reshape(self.M, self.K)

    def act_t(self, f=None, y=None, x=None, c=None):
        """family T's activation at the given coordinates (default: the whole input tensor [F, H, W, Cin])"""
        if f is None:
            f, y, x, c = (torch.arange(n).view(s) for n, s in ((self.F, (-1, 1, 1, 1)), (self.H, (1, -1, 1, 1)), (self.W, (1, 1, -1, 1)), (self.Cin, (1, 1, 1, -1))))
        return ((31 * f + 7 * y + 3 * x + c) % 251 - 125).float()

    def weight_t(self):
        """[Cout, taps * Cin] one-hot in (tap, cin) order"""
        co = torch.arange(self.Cout)
        w = torch.zeros(self.Cout, self.K)
        w[co, (co % self.taps) * self.Cin + (co // self.taps) % self.Cin] = 1.0
        return w

    def want_t(self, mutant=None):
        """[M, Cout]: the named neighbour's value from the formula, no product anywhere"""
        f, y, x, valid = self.coords(mutant)
        co = torch.arange(self.Cout)
        tap, c = co % self.taps, (co // self.taps) % self.Cin
        return self.act_t(f[:, tap], y[:, tap], x[:, tap], c.view(1, -1)) * valid[:, tap].float()

    def family_a(self, seed=0):
        g = gen(self.F, self.H, self.W, self.Cin, self.Cout, self.taps, seed)
        d = density(self.K)
        return dict(x=tri((self.F, self.H, self.W, self.Cin), g, d), w=tri((self.Cout, self.K), g, d), bias=torch.randint(-8, 9, (self.Cout,), generator=g).float(),
                    resid=torch.randint(-64, 65, (self.M, self.Cout), generator=g).float())

    def kwargs(self):
        """the keyword arguments of ops.conv_implicit"""
        if self.mode == "t3":
            return dict(frames=self.frames)
        return dict(stride=self.stride, upsample=self.upsample, asym_pad=self.asym_pad, t_frames=self.t_frames)

    def x_shape(self):
        return (self.F, self.W, self.Cin) if self.mode == "t3" else (self.F, self.H, self.W, self.Cin)


def conv_model(cv, p, epi=EPI_NONE, acc_scale=1.0, mutant=None, BM=128, BN=128):
    """the implicit convolution as the tiled GEMM of its gathered rows (gemm_model: 32-deep K steps inside each tap's channels)"""
    return gemm_model(dict(p, x=cv.rows(p["x"], mutant)), epi, acc_scale=acc_scale, BM=BM, BN=BN)


MUTANTS_T = {"border_wraps": dict(), "upsample_off_by_one": dict(upsample=True), "asym_origin": dict(stride=2, asym_pad=True), "tap_crosses_clip": "t3",
             "causal_next_sample": dict(t_frames=3)}


# ---------------------------------------------------------------------------------------------- quarter-turn RoPE
def rope_tables(rows):
    """cos / sin [rows, 64] fp32 with entries in {0, +-1}: position r turns pair i by ((r + 3 i) mod 4) quarter turns; both features of a pair share the angle"""
    r, i = torch.arange(rows).view(-1, 1), (torch.arange(64) // 2).view(1, -1)
    q = (r + 3 * i) % 4
    return torch.tensor([1.0, 0.0, -1.0, 0.0])[q], torch.tensor([0.0, 1.0, 0.0, -1.0])[q]


def qkv_want(proj, B, S, H, text_len, q_premul, first=0):
    """the reference of family Q, no product with a table entry anywhere: proj [B S, n H 64] (the exact bf16 projection, fp64) -> Q and K thirds of the rows at
    position >= text_len turned by ((pos - text_len) + 3 i) mod 4 quarter turns -- (a, b) -> (a, b), (-b, a), (-a, -b), (b, -a) -- Q halved, V and text rows kept"""
    D = H * 64
    n = proj.shape[1] // D
    v = proj.double().view(B, S, n, H, 32, 2)
    pos = torch.arange(S, device=proj.device).view(1, S, 1, 1, 1)
    q = ((pos - text_len) + 3 * torch.arange(32, device=proj.device).view(1, 1, 1, 1, 32)) % 4
    a, b = v[..., 0], v[..., 1]
    oa = torch.where(q == 0, a, torch.where(q == 1, -b, torch.where(q == 2, -a, b)))
    ob = torch.where(q == 0, b, torch.where(q == 1, a, torch.where(q == 2, -b, -a)))
    vid = pos >= text_len
    out = torch.stack([torch.where(vid, oa, a), torch.where(vid, ob, b)], dim=-1).clone()
    for j in range(n):
        if first + j == 0:
            out[:, :, j] *= q_premul
        if first + j == 2:
            out[:, :, j] = v[:, :, j]
    return bf16_rne(out.reshape(B * S, n * D))


def qkv_model(proj, B, S, H, text_len, cos, sin, q_premul, first=0, *, mutant=None):
    """the fused epilogue's arithmetic on the tables (gemm_common.h, qk_row_math): oa = a cos[2i] - b sin[2i], ob = b cos[2i + 1] + a sin[2i + 1] on rows at
    position >= text_len, table row = position - text_len; Q times q_premul.  Mutants: "pair_partner" (the partner comes from the next pair),
    "pos_from_sample_start" (the table row is the position inside the sample)"""
    D = H * 64
    n = proj.shape[1] // D
    v = proj.double().view(B, S, n, H, 32, 2).clone()
    pos = torch.arange(S, device=proj.device)
    row = (pos - text_len).clamp(min=0)
    if mutant == "pos_from_sample_start":
        row = pos.clamp(max=cos.shape[0] - 1)
    c, s = (t.double().to(proj.device)[row].view(1, S, 1, 1, 32, 2) for t in (cos, sin))
    a, b = v[..., 0], v[..., 1]
    if mutant == "pair_partner":
        b = torch.roll(v[..., 1], -1, dims=-1)
    oa, ob = a * c[..., 0] - b * s[..., 0], v[..., 1] * c[..., 1] + a * s[..., 1]
    if mutant == "pair_partner":
        ob = v[..., 1] * c[..., 1] + torch.roll(a, -1, dims=-1) * s[..., 1]
    vid = (pos >= text_len).view(1, S, 1, 1, 1)
    rot = torch.stack([torch.where(vid, oa, v[..., 0]), torch.where(vid, ob, v[..., 1])], dim=-1)
    for j in range(n):
        third = first + j
        if third < 2:
            v[:, :, j] = rot[:, :, j] * (q_premul if third == 0 else 1.0)
    return bf16_rne(v.reshape(B * S, n * D))


MUTANTS_Q = ("pair_partner", "pos_from_sample_start")

# ---------------------------------------------------------------------------------------------- the shapes of the GPU file (M, N, K), asserted on the CPU too
TILE128 = [(17, 64, 64), (257, 132, 64), (300, 260, 192), (1000, 520, 320)]
WAVE8 = [(6144 + 77, 2048, 192), (6144 + 77, 2048, 1024)]
WIDE320 = [(16384, 640, 384), (7168 + 13, 1600, 192)]
W4 = [(6144 + 77, 2048, 320), (6144 + 77, 2048, 1984), (271 * 256 - 100, 512, 320)]
STREAMK = (4352, 4096, 1024)
K320 = [(16384 + 37, 320, 320), (16384 + 37, 960, 320)]
SKINNY = [(250, 768, 1024), (16, 2304, 768), (1, 260, 256), (33, 4100, 2048)]
QKV = dict(B=2, S=3011, text=226, H=4, K=640)
R_SHAPES = [(300, 260, 512), (257, 132, 2048)]


QKV_FUSED_H = 16      # heads at which the QKV problem reaches the 192 tiles of the fused epilogues (H = 4 of the same rows is 72 tiles)
OTHER = [(300, 256, 320), (300, 256, 256), (QKV["B"] * QKV["S"], 3 * QKV_FUSED_H * 64, QKV["K"])]      # per-sample weights / fp8 k64, fp8, the fused QKV

# the convolutions of the GPU file: every form on the 128x128 tile, then every tile the dispatch reaches (counter, problem, with the residual case)
CONV_SMALL = {
    "3x3": Conv("3x3", 2, 7, 10, 64, 96),
    "stride2": Conv("3x3", 2, 7, 9, 64, 96, stride=2),
    "upsample": Conv("3x3", 2, 7, 10, 64, 96, upsample=True),
    "asym_pad": Conv("3x3", 2, 7, 9, 64, 96, stride=2, asym_pad=True),
    "causal": Conv("3x3", 10, 7, 10, 64, 96, t_frames=3),
}


CONV_BIG = [
    ("CONV3_256x256", Conv("3x3", 2, 160, 157, 64, 256), True),
    ("CONV3_256x256", Conv("3x3", 2, 320, 313, 64, 256, stride=2), False),
    ("CONV3_256x256", Conv("3x3", 2, 80, 79, 64, 256, upsample=True), False),
    ("CONV3_256x256", Conv("3x3", 2, 319, 313, 64, 256, stride=2, asym_pad=True), False),
    ("CONV3_256x256", Conv("3x3", 10, 92, 92, 64, 256, t_frames=3), False),
    ("CONV3_256x320", Conv("3x3", 1, 128, 129, 64, 640), True),
    ("CONV3_256x128", Conv("3x3", 2, 160, 157, 64, 128), True),
    ("CONV3_192x256", Conv("3x3", 6, 96, 114, 64, 256), True),       # 257 tiles of 256 rows (two rounds) against 342 of 192; the planned (6, 96, 112) is 252 tiles: one round, the 256x256 tile
    ("CONVT_128x128", Conv("t3", 8, 1, 12, 64, 96, frames=4), True),
    ("CONVT_256x256", Conv("t3", 8, 1, 6300, 64, 256, frames=4), True),
    ("CONVT_256x320", Conv("t3", 8, 1, 2050, 64, 640, frames=4), False),
    ("CONVT_192x256", Conv("t3", 8, 1, 8208, 64, 256, frames=4), False),
]



def gate_plan(M):
    """two samples, the split a third into the sample: (rows_per_batch, split).  Both boundaries fall inside a wave tile for every shape above"""
    rpb = (M + 1) // 2
    return rpb, rpb // 3 + 1
