"""Masked / biased attention by value: the HAS_MASK instantiation of attn_fwd_kernel (attn_flash.hip) behind `ops.attention(mask=..., bias=...)`.

Every expected value is an fp64 softmax on the bf16-rounded q / k / v with the mask as -inf and the bias added as given (so a finite -1e9, finfo.min and
-inf agree); nothing is compared with the kernel itself.  Tolerance: `close` of test_gpu_kernels.py (2e-2 |want| + 2e-2 scale; scale 0.3 for unit-variance
V, 1.0 where a residual is added), every element counted.  Scores stay where the existing attention tests run: q, k ~ N(0, 1) with scale 1/8 for the
mask-only launches, the T5 form (q, k ~ 0.4 N(0, 1), scale 1, bias ~ 2 N(0, 1)) wherever a bias is given.  Every mask / bias leaves each query row at
least one open key (asserted on the host before the launch): the result of a row with no open key is unspecified (include/mrag_hip.h).

Which random draw.  Where two or three keys carry a row's weight (the 90 % masks, 25 keys, the T5 form's score spread of 2.4) the kernel's two DOCUMENTED
roundings -- Q pre-multiplied by scale * log2 e in bf16, P in bf16 -- use up 0.6 to 1.5 times that tolerance on their own in the worst of ~10^5 elements:
two keys of weight p1, p2 give |error| = p1 p2 |eps1 - eps2| |v1 - v2| with eps up to 2^-8 and unit-variance values up to 6 apart, against 6e-3 at
want = 0.  A draw on which they exceed it would fail a perfect kernel.  `draw` therefore takes the first seed of a fixed sequence on which `format_model` --
those roundings applied on the host, fp64 otherwise; never the kernel's output -- stays within ROOM of the tolerance, and every comparison keeps the
tolerance itself.

Launch paths (mrag_attn_fwd_bf16): Sq <= 32 one wave, 33..128 two waves, > 128 eight waves, and Sq > 128 with Skv <= 64 the one-tile instantiation.
Key tiles are 64 wide; a ragged last tile of a >= 64-key sequence is slid back to [Skv - 64, Skv), shorter key sets clamp rows."""
import os

import numpy as np
import pytest
import torch

from test_gpu_kernels import bf, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMIN = torch.finfo(torch.float32).min
LOG2E = 1.4426950408889634
KTHR = 5.0                                      # attn_flash.hip's deferred-rescale threshold, log2 units
# share of the tolerance the documented roundings may use up on an accepted draw.  The rest is for what format_model does not carry: fp32 where it has fp64
# (now and then a P rounds the other way), and on rows re-centred from the first-tile floor the 2^-10 log2 units to which S + 16384 keeps S in fp32 --
# a quarter of such a row's P values round the other way, which moves single elements by up to half the tolerance but the worst element by about 0.1
ROOM = 0.85


def ref64(q, k, v, scale, mask=None, bias=None, kv_div=1):
    """fp64 softmax(scale q k^T + bias [mask -> -inf]) v on [B, S, H, 64] tensors -> [B, Sq, H * 64]; mask [Sq, Skv] bool, bias [H, Sq, Skv]"""
    q, k, v = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    if kv_div > 1:
        k, v = k.repeat_interleave(kv_div, dim=0), v.repeat_interleave(kv_div, dim=0)
    s = q @ k.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias.double()[None]
    if mask is not None:
        s = s.masked_fill(mask[None, None], float("-inf"))
    o = torch.softmax(s, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[2], -1)


def format_model(q, k, v, scale, mask=None, bias=None):
    """The result as the kernel's number formats alone leave it (module docstring): Q times scale * log2 e rounded to bf16; P = exp2(S - m) rounded to bf16, with
    the running max m where attn_flash.hip keeps it -- a bf16 value set on the first 64-key tile (floor -2^14) and moved by a later tile only when a row of
    the 32-row wave exceeds it by more than 2^5; the row sum over the rounded P; bf16 output.  fp64 everywhere else.  Not an expected value: `draw` alone uses it."""
    B, Sq, H, _ = q.shape
    Skv = k.shape[1]
    s = torch.einsum("bqhd,bkhd->bhqk", bf(q.float() * (scale * LOG2E)).double(), k.double())
    if bias is not None:
        s = s + bias.double()[None] * LOG2E
    if mask is not None:
        s = s.masked_fill(mask[None, None], float("-inf"))
    vd = v.double().permute(0, 2, 1, 3)
    o = torch.zeros(B, H, Sq, 64, dtype=torch.float64)
    l = torch.zeros(B, H, Sq, dtype=torch.float64)
    m = torch.zeros(B, H, Sq, dtype=torch.float64)
    for t0 in range(0, Skv, 64):
        st = s[..., t0:t0 + 64]
        tm = st.amax(dim=-1) - m
        if t0 == 0:
            move = bf(tm.clamp_min(-16384.0)).double()
        else:
            wave = torch.nn.functional.pad(tm > KTHR, (0, -Sq % 32)).view(B, H, -1, 32).any(dim=-1, keepdim=True)
            wave = wave.expand(-1, -1, -1, 32).reshape(B, H, -1)[..., :Sq]
            move = torch.where(wave, bf(m + tm.clamp_min(0.0)).double() - m, torch.zeros_like(m))
        if t0 > 0:
            f = torch.exp2(-move)
            o, l = o * f[..., None], l * f
        m = m + move
        p = bf(torch.exp2(st - m[..., None])).double()
        o, l = o + p @ vd[:, :, t0:t0 + 64], l + p.sum(dim=-1)
    return bf((o / l[..., None]).permute(0, 2, 1, 3).reshape(B, Sq, H * 64)).double()


def draw(seed, build):
    """build(generator) -> (q, k, v, scale, mask, bias).  The first of the seeds seed, seed + 1, ... whose case leaves every row an open key and on which the
    documented roundings alone stay within ROOM of the tolerance; returns the case and its fp64 expected value."""
    for s in range(seed, seed + 32):
        q, k, v, scale, mask, bias = build(torch.Generator().manual_seed(s))
        Sq, Skv = q.shape[1], k.shape[1]
        open_ = torch.ones(1, Sq, Skv, dtype=torch.bool) if mask is None else ~mask[None]
        if bias is not None:
            open_ = open_ & (bias > -1e8)       # blocked entries here are -inf, finfo.min or -1e9; the random part is ~ 2 N(0, 1)
        assert open_.any(dim=-1).all(), "a query row without an open key"        # no row is excluded from the comparison
        want = ref64(q, k, v, scale, mask, bias)
        used = ((format_model(q, k, v, scale, mask, bias) - want).abs() / (2e-2 * want.abs() + 2e-2 * 0.3)).max().item()
        if used <= ROOM:
            return q, k, v, scale, mask, bias, want
    raise AssertionError("no draw in 32 on which the bf16 roundings of Q and P leave the tolerance room")


def qkv_unit(g, B, H, Sq, Skv):                 # scale 1/8
    return tuple(bf(torch.randn(B, S, H, 64, generator=g)) for S in (Sq, Skv, Skv))


def qkv_t5(g, B, H, Sq, Skv):                   # scale 1, with a bias ~ 2 N(0, 1)
    q, k = (bf(0.4 * torch.randn(B, S, H, 64, generator=g)) for S in (Sq, Skv))
    return q, k, bf(torch.randn(B, Skv, H, 64, generator=g))


def random_mask(g, Sq, Skv, density):
    """True = blocked at the given density; one key per row (a random one) is always left open"""
    m = torch.rand(Sq, Skv, generator=g) < density
    m[torch.arange(Sq), torch.randint(0, Skv, (Sq,), generator=g)] = False
    return m


def run(q, k, v, **kw):
    from motionrag_amd import ops
    kw = {n: (t.to(DEV) if torch.is_tensor(t) else t) for n, t in kw.items()}
    return ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), **kw)


# ---------------------------------------------------------------------------------------------- A. every launch path
# (B, H, Sq, Skv): Skv < 64 (clamped rows), Skv % 64 == 0, the slid-back last tile, Sq not a multiple of 32; B * H = 6 (bias head stride, bias shared by the
# batch) and B * H = 8 (the other block -> (q-tile, b, h) mapping)
PATH_SHAPES = [(2, 3, 7, 130), (2, 4, 32, 64), (2, 3, 20, 40),              # one wave
               (2, 3, 77, 77), (2, 4, 128, 200), (2, 3, 40, 1),            # two waves (77 x 77: OpenCLIP's text tower)
               (2, 3, 130, 257), (2, 4, 300, 192),                         # eight waves
               (2, 3, 200, 25), (2, 4, 129, 64)]                           # the one-tile launch
MODES = ["mask30", "mask90", "bias", "bias_mask", "bias_inf_cols", "bias_fmin_cols"]
# one key: nothing can be blocked, so that shape runs the bias-only launch alone
PATH_CASES = [(*shape, mode) for shape in PATH_SHAPES for mode in MODES if shape[3] > 1 or mode == "bias"]


@pytest.mark.parametrize("B,H,Sq,Skv,mode", PATH_CASES)
def test_masked_attention_every_launch_path(hip, B, H, Sq, Skv, mode):
    def build(g):
        if mode.startswith("mask"):
            return (*qkv_unit(g, B, H, Sq, Skv), 0.125, random_mask(g, Sq, Skv, 0.3 if mode == "mask30" else 0.9), None)
        q, k, v = qkv_t5(g, B, H, Sq, Skv)
        bias = 2.0 * torch.randn(H, Sq, Skv, generator=g)
        mask = random_mask(g, Sq, Skv, 0.3) if mode == "bias_mask" else None
        if mode.endswith("_cols"):              # key padding: whole columns blocked for every row and head
            cols = torch.rand(Skv, generator=g) < 0.3
            cols[Skv // 2] = False
            cols[Skv - 1] = True                # the last key of the ragged tile among them
            bias[:, :, cols] = float("-inf") if mode == "bias_inf_cols" else bias[:, :, cols] + FMIN
        return q, k, v, 1.0, mask, bias
    q, k, v, scale, mask, bias, want = draw(1000 * Sq + Skv + 100 * MODES.index(mode), build)
    close(run(q, k, v, scale=scale, mask=mask, bias=bias), want, scale=0.3)


# ---------------------------------------------------------------------------------------------- B. structured rows
SKV_B = 200                                     # tiles [0, 64), [64, 128), [128, 192) and the slid-back [136, 200), of which [136, 192) counts as seen
N_PAT = 9


def pattern_mask(Sq, Skv=SKV_B):
    """blocked keys of row r follow pattern r % 9, so every 32-row wave holds all of them (the rescale decision is __any over the wave)"""
    m = torch.zeros(Sq, Skv, dtype=torch.bool)
    for r in range(Sq):
        p = r % N_PAT
        if p == 1: m[r, :64] = True                                    # first key tile blocked
        elif p == 2: m[r, :128] = True                                 # first two
        elif p == 3: m[r, :70] = True                                  # first tile and a little of the second
        elif p == 4: m[r] = True; m[r, 199] = False                    # only the last key (new in the slid-back tile)
        elif p == 5: m[r] = True; m[r, 150] = False                    # only a key the slid-back tile has seen already: counted exactly once
        elif p == 6: m[r] = True; m[r, 0] = False                      # only key 0
        elif p == 7: m[r, 64:128] = True                               # a blocked tile in the middle
        elif p == 8: m[r, 64:] = True                                  # everything after the first tile
    return m


FORMS = ["mask", "bias_inf", "bias_fmin", "bias_1e9"]


def structured_case(g, B, H, Sq, form):
    pat = pattern_mask(Sq)
    if form == "mask":
        return (*qkv_unit(g, B, H, Sq, SKV_B), 0.125, pat, None)
    q, k, v = qkv_t5(g, B, H, Sq, SKV_B)
    bias = 2.0 * torch.randn(H, Sq, SKV_B, generator=g)
    if form == "bias_inf":
        bias = bias.masked_fill(pat[None], float("-inf"))
    elif form == "bias_fmin":                   # the way t5.py folds attention_mask: finfo.min added to the finite bias
        bias = bias + pat[None].float() * FMIN
    else:
        bias = bias + pat[None].float() * -1e9
    return q, k, v, 1.0, None, bias


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Sq", [20, 96, 160])   # one, two and eight waves
def test_masked_attention_rows_blocked_in_leading_tiles(hip, Sq, form):
    q, k, v, scale, mask, bias, want = draw(100 * Sq + 1000 * FORMS.index(form), lambda g: structured_case(g, 2, 3, Sq, form))
    close(run(q, k, v, scale=scale, mask=mask, bias=bias), want, scale=0.3)


# ---------------------------------------------------------------------------------------------- C. a max jump beside unseeded rows
JUMPS = ((0, 100), (36, 170))                   # (p0 row, key planted against it)


@pytest.mark.parametrize("form", ["mask", "bias_fmin"])
def test_masked_attention_max_jump_beside_unseeded_rows(hip, form):
    """The structured rows at 96 x 200, with two p0 rows (nothing blocked) whose max jumps far past the deferred-rescale threshold: row 0 at key 100 (tile 1:
    rows p1, p2, p3 of its wave have had no open key before that tile, p2 has none in it either) and row 36 at key 170 (tile 2: p2 rows of its wave get
    their first open key in the very tile of the jump).  The wave-wide rescale must move the jumping row and leave the unseeded ones sound."""
    def build(g):
        q, k, v, scale, mask, bias = structured_case(g, 2, 3, 96, form)
        q, k = q.float(), k.float()
        for row, key in JUMPS:
            k[:, key] = (16.0 / scale) * q[:, row] / (q[:, row].norm(dim=-1, keepdim=True) ** 2)    # score ~ 16 (23 in log2 units) against `row`
            if bias is not None:
                bias[:, row, key] = 0.0
        return bf(q), bf(k), v, scale, mask, bias
    q, k, v, scale, mask, bias, want = draw(7700 + FORMS.index(form), build)
    # the planted score exceeds everything the row saw in earlier tiles by more than the threshold (with a margin for the deferred max), per batch and head
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    if bias is not None:
        s = s + bias.double()[None]
    for row, key in JUMPS:
        assert row % N_PAT == 0 and (bias is None or (bias[:, row] > -1e8).all())       # a p0 row: nothing blocked
        before = s[:, :, row, :(key // 64) * 64].max(dim=-1).values
        assert ((s[:, :, row, key] - before) * LOG2E).min().item() > KTHR + 1.0
    close(run(q, k, v, scale=scale, mask=mask, bias=bias), want, scale=0.3)


# ---------------------------------------------------------------------------------------------- D. mask with the fused features
def test_masked_attention_with_fused_features(hip):
    """a mask (random, with every third row blocked on keys [0, 70)) on strided views of a fused QKV buffer; with resid in place, out_scale 0.75 and
    kv_batch_div 2; a bias with q_prescaled (Q carries scale * log2 e, `scale` is ignored)"""
    from motionrag_amd import ops
    B, S, H = 4, 150, 3

    def build(g):
        mask = random_mask(g, S, S, 0.3)
        mask[1::3, :70] = True
        mask[1::3, 70] = False
        qkv = bf(torch.randn(B, S, 3, H, 64, generator=g))
        return qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 0.125, mask, None
    q, k, v, _, mask, _, want = draw(1100, build)
    assert q.stride(1) == 3 * H * 64            # views of one [B, S, 3, H, 64] buffer, as the model code passes them
    qd, kd, vd, md = q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV)
    close(ops.attention(qd, kd, vd, mask=md), want, scale=0.3)
    g = torch.Generator().manual_seed(12)
    kv = bf(torch.randn(2, S, 2, H, 64, generator=g))                    # two K/V sets for four query batches
    resid = bf(torch.randn(B, S, H * 64, generator=g))
    kvd, rd = kv.to(DEV), resid.to(DEV)
    out = ops.attention(qd, kvd[:, :, 0], kvd[:, :, 1], out=rd, resid=rd, mask=md, kv_batch_div=2, out_scale=0.75)   # in place
    assert out.data_ptr() == rd.data_ptr()
    close(out, resid.double() + 0.75 * ref64(q, kv[:, :, 0], kv[:, :, 1], 0.125, mask, kv_div=2), scale=1.0)
    # q_prescaled: the kernel takes Q as it is (log2 units, the bf16 values of q * log2 e); the expected value divides exactly those values by log2 e
    q, k, v, _, _, bias, _ = draw(1300, lambda g: structured_case(g, 2, H, 96, "bias_fmin"))
    q_pre = bf(q.float() * LOG2E)
    got = run(q_pre, k, v, scale=123.0, q_prescaled=True, bias=bias)
    close(got, ref64(q_pre, k, v, 1.0 / LOG2E, None, bias), scale=0.3)


# ---------------------------------------------------------------------------------------------- E. model level
def test_t5_left_padded_attention_mask_vs_oracle(hip, golden_dir):
    """t5.T5EncoderModel folds attention_mask into the bias as finfo.min: left padding blocks whole leading key tiles (sample 0: 100 leading zeros; sample 1:
    64 leading and 30 trailing).  Reduced config and weights of tests/golden/t5.npz, against the fp32 oracle with the same mask, at that file's bound."""
    from motionrag_amd import t5
    from oracle import t5_ref as R
    G = np.load(os.path.join(golden_dir, "t5.npz"))
    d, h, dk, dff, layers, vocab = (int(v) for v in G["cfg"])
    sd = {k[3:]: torch.from_numpy(G[k].view(np.int16).copy()).view(torch.bfloat16).float() for k in G.files if k.startswith("sd.")}
    m = t5.T5EncoderModel(vocab_size=vocab, d_model=d, d_kv=dk, d_ff=dff, num_layers=layers, num_heads=h)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV, torch.bfloat16)
    ids = torch.from_numpy(G["ids"])
    B, S = ids.shape
    assert (B, S) == (2, 226)
    am = torch.ones(B, S, dtype=torch.int64)
    am[0, :100] = 0
    am[1, :64] = 0
    am[1, S - 30:] = 0
    want = R.t5_encoder(sd, dict(d_model=d, num_heads=h, d_kv=dk, num_layers=layers, eps=1e-6), ids, am)
    got = m(ids.to(DEV), attention_mask=am.to(DEV))[0].float().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert ((got - want).norm() / want.norm()).item() <= 2e-2
