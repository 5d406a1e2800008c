"""The MFMA attention for head dims 32 / 80 / 96 / 128 at any length (mrag_attn_hd_fwd_bf16, ops.attention_hd) through the C ABI: values against fp64 attention of
the same bf16 inputs, inputs whose exact result is known (attn_exact.py), agreement with mrag_attn_small_bf16 wherever both run, untouched neighbours, bit-equal
runs, graph capture, the launch counter, and the CLIP vision tower on it -- opted in at 257 tokens, by the routing rule alone at 577."""
import os

import numpy as np
import pytest
import torch

import attn_exact as X
from oracle import clip_vision_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (32, 80, 96, 128)
SHAPES = ((1, 1), (31, 31), (32, 32), (33, 33), (64, 65), (257, 257), (300, 70), (70, 300))
LONG = ((577, 577), (900, 900))                     # D = 80, B = 1, H = 2: what mrag_attn_small_bf16 refuses
BOUND = 6e-3                                        # relative L2, the bound test_gpu_clip_vision.py::test_attention_small holds the fp32-FMA kernel to
KT = 64                                             # keys per tile of the kernel


def rel(got, want):
    g, w = got.double().cpu(), want.double().cpu()
    assert g.shape == w.shape and torch.isfinite(g).all()
    return ((g - w).norm() / w.norm()).item()


def small_takes(Skv, D):
    return Skv * D <= 32768


_CASES = {}


def case(D, Sq, Skv):
    """(q, k, v) as strided views of one fused [B, S, 3, H, D] buffer on the device and the fp64 result; built once per shape, never written again"""
    key = (D, Sq, Skv)
    if key not in _CASES:
        B, H = (1, 2) if (Sq, Skv) in LONG else (2, 3)
        S = max(Sq, Skv)
        g = torch.Generator().manual_seed(1000 * D + 7 * Sq + Skv)
        qkv = (torch.randn(B, S, 3, H, D, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
        q, k, v = qkv[:, :Sq, 0], qkv[:, :Skv, 1], qkv[:, :Skv, 2]
        want, _ = X.ref64(q, k, v, D ** -0.5)
        _CASES[key] = (q, k, v, want)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("Sq,Skv", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_values_against_fp64(hip, D, Sq, Skv):
    from motionrag_amd import ops
    q, k, v, want = case(D, Sq, Skv)
    got = ops.attention_hd(q, k, v)
    assert got.shape == want.shape and got.dtype == torch.bfloat16
    r = rel(got, want)
    print(f"attention_hd D={D} Sq={Sq} Skv={Skv}: relative L2 {r:.3e}")
    assert r <= BOUND


@pytest.mark.parametrize("Sq,Skv", LONG)
def test_values_beyond_the_fma_kernels_length(hip, Sq, Skv):
    from motionrag_amd import ops
    from motionrag_amd._lib import HipError
    q, k, v, want = case(80, Sq, Skv)
    with pytest.raises(HipError):                   # the refusal that stays: K and V of a head do not fit the LDS of the fp32-FMA kernel
        ops.attention_small(q, k, v)
    r = rel(ops.attention_hd(q, k, v), want)
    print(f"attention_hd D=80 Sq={Sq} Skv={Skv}: relative L2 {r:.3e}")
    assert r <= BOUND


# ---------------------------------------------------------------------------------------------- 2. exact inputs
class Planted:
    """q / k / v [B, S, H, D] as views of one fused [B, GUARD + S + GUARD, 3, H + 1, D] buffer that is -1 wherever the launch has no business: the guard rows
    in front of and behind every sequence (what a ragged key tile would pick up) and a whole head behind the last one (what a row read past column D would)"""

    def __init__(self, q, k, v):
        B, Sq, H, D = q.shape
        S = max(Sq, k.shape[1])
        self.buf = torch.full((B, S + 2 * X.GUARD, 3, H + 1, D), -1.0, dtype=torch.bfloat16, device=DEV)
        for i, t in enumerate((q, k, v)):
            self.buf[:, X.GUARD:X.GUARD + t.shape[1], i, :H] = t.to(DEV)
        self.views = tuple(self.buf[:, X.GUARD:X.GUARD + t.shape[1], i, :H] for i, t in enumerate((q, k, v)))
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(self.buf, self.before)


@pytest.mark.parametrize("q0", X.Q0_LEVELS[:2])
@pytest.mark.parametrize("Skv", (KT, KT + 1, 257))
@pytest.mark.parametrize("D", (80, 96))
def test_every_key_counted_once(hip, D, Skv, q0):
    """family A: equal scores (zero at q0 = 0), 0 / 1 indicator V: every output is the count n_d / Skv, to the bf16 rounding of the output alone.  A key dropped,
    counted twice or let in from the -1 planted around the inputs moves a feature by four bounds or more."""
    from motionrag_amd import ops
    B, H, Sq = 2, 3, 70                              # two workgroups per (batch, head), the second ragged (6 rows)
    X.check_shape_a(Skv, D)
    q, k, v = X.family_a(B, H, Sq, Skv, q0, D=D)
    pl = Planted(q, k, v)
    out = X.OutBuffer(B, Sq, H * D, DEV)
    res = ops.attention_hd(*pl.views, scale=8.0 / D, out=out.view)
    assert res is out.view
    w = X.check(out.view, X.expected_a(B, H, Sq, Skv, D), f"D={D} Skv={Skv} q0={q0}", **X.TOL_A)
    print(f"family A D={D} Skv={Skv} q0={q0}: worst {w:.3f} of the bf16 rounding bound")
    assert out.guards_intact() and pl.unchanged()


@pytest.mark.parametrize("Sq,Skv", ((257, 257), (70, 300), (300, 70)))
@pytest.mark.parametrize("D", (80, 96))
def test_every_row_meets_its_own_key(hip, D, Sq, Skv):
    """family B: row r of (b, h) is aimed at key pi(r), whose V row is a code of (b, h, key): a row, head or batch routed elsewhere, or K paired with another
    key's V, shows in the code bits"""
    from motionrag_amd import ops
    B, H = 2, 3
    q, k, v, pi = X.family_b(B, H, Sq, Skv, D=D)
    pl = Planted(q, k, v)
    want, leak = X.ref64(*pl.views, 8.0 / D, pi=pi)
    assert leak <= X.LEAK
    got = ops.attention_hd(*pl.views, scale=8.0 / D)
    X.check(got, want, f"D={D} Sq={Sq} Skv={Skv}", **X.TOL_B)
    assert pl.unchanged()


# ---------------------------------------------------------------------------------------------- 3. agreement with the fp32-FMA kernel
BOTH = [(D, Sq, Skv) for D in DIMS for Sq, Skv in SHAPES if small_takes(Skv, D)]      # all but 257 and 300 keys at D = 128
assert len(BOTH) == len(DIMS) * len(SHAPES) - 2


@pytest.mark.parametrize("D,Sq,Skv", BOTH)
def test_agrees_with_attention_small(hip, D, Sq, Skv):
    from motionrag_amd import ops
    q, k, v, _ = case(D, Sq, Skv)
    assert rel(ops.attention_hd(q, k, v), ops.attention_small(q, k, v)) <= 2 * BOUND      # each within BOUND of fp64: the sum of the two bounds


# ---------------------------------------------------------------------------------------------- 4. neighbours untouched
@pytest.mark.parametrize("D,Sq,Skv", [(80, 257, 257), (32, 33, 33), (96, 70, 300), (128, 65, 64), (80, 1, 1)])
def test_neighbours_untouched(hip, D, Sq, Skv):
    """`out` a view with 8 guard rows and 32 guard columns of a sentinel on every side; the inputs views of a fused [B, S, 3, H, D] buffer whose last V row of the
    last head is the last thing in front of sentinel bytes: nothing outside [B, Sq, H * D] changes, and the result is the one of the plain buffers"""
    from motionrag_amd import ops
    q, k, v, want = case(D, Sq, Skv)
    B, _, H, _ = q.shape
    S = max(Sq, Skv)
    n = B * S * 3 * H * D
    flat = torch.full((n + 4096,), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
    fused = flat[:n].view(B, S, 3, H, D)
    fused[:, :Sq, 0], fused[:, :Skv, 1], fused[:, :Skv, 2] = q, k, v
    before = flat.clone()
    out = X.OutBuffer(B, Sq, H * D, DEV)
    ops.attention_hd(fused[:, :Sq, 0], fused[:, :Skv, 1], fused[:, :Skv, 2], out=out.view)
    assert out.guards_intact() and torch.equal(flat, before)
    assert torch.equal(out.view, ops.attention_hd(q, k, v)) and rel(out.view, want) <= BOUND


# ---------------------------------------------------------------------------------------------- 5. determinism, capture, the counter
def test_two_runs_bit_equal_and_graph_capture(hip):
    from motionrag_amd import ops
    q, k, v, _ = case(80, 257, 257)
    eager = ops.attention_hd(q, k, v)
    assert torch.equal(ops.attention_hd(q, k, v), eager)
    og = torch.zeros_like(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.HIPGraph() if hasattr(torch.cuda, "HIPGraph") else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                                # the captured region is that single kernel
        ops.attention_hd(q, k, v, out=og)
    og.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(og, eager)


def test_one_call_is_one_counted_launch_and_a_refusal_is_none(hip):
    from motionrag_amd import ops
    from motionrag_amd._lib import HipError
    q, k, v, _ = case(96, 33, 33)
    before = ops.attn_hd_launch_counts()
    with ops.dispatched() as d:
        ops.attention_hd(q, k, v)
    assert ops.attn_hd_launch_counts() == before + 1 and d.counts == {}                          # a counter of its own: the dispatch table does not move
    ops.attention_hd(q, k, v)
    assert ops.attn_hd_launch_counts() == before + 2
    bad = torch.zeros(1, 8, 3, 2, 40, dtype=torch.bfloat16, device=DEV)
    for qkv in (bad, torch.zeros(1, 8, 3, 2, 64, dtype=torch.bfloat16, device=DEV)):            # head dims 40 and 64: refused
        with pytest.raises(HipError):
            ops.attention_hd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    assert ops.attn_hd_launch_counts() == before + 2


# ---------------------------------------------------------------------------------------------- 6. the CLIP vision tower
def _golden_tower(golden_dir):
    from motionrag_amd import clip_vision as C
    G = np.load(os.path.join(golden_dir, "clip_vision.npz"))
    d, heads, layers, ff, img, patch, proj = (int(v) for v in G["cfg"])
    m = C.CLIPVisionModelWithProjection(hidden_size=d, intermediate_size=ff, num_hidden_layers=layers, num_attention_heads=heads, image_size=img, patch_size=patch, projection_dim=proj)
    m.load_state_dict({k[3:]: torch.from_numpy(G[k].view(np.int16).copy()).view(torch.bfloat16).float() for k in G.files if k.startswith("sd.")}, strict=True)
    return m.to(DEV, torch.bfloat16), G, layers


def test_tower_on_the_mfma_kernel_equals_transformers_golden(hip, golden_dir):
    from motionrag_amd import clip_vision as C
    from motionrag_amd import ops
    m, G, layers = _golden_tower(golden_dir)
    assert m.head_dim != 64
    pix = torch.from_numpy(G["pixel_values"]).to(DEV)
    n0 = ops.attn_hd_launch_counts()
    with ops.dispatched() as d:
        off = m(pix)
    assert ops.attn_hd_launch_counts() == n0 and d.counts.get("ATTN_SMALL") == layers            # the switch is off by default: nothing moves
    assert C.set_attention_kernel(m, "mfma") is m
    with ops.dispatched() as d:
        out = m(pix)
    assert ops.attn_hd_launch_counts() == n0 + layers and "ATTN_SMALL" not in d.counts           # one launch per layer
    assert rel(out.last_hidden_state, torch.from_numpy(G["last_hidden_state"])) <= 2e-2          # vs the REAL transformers class
    assert rel(out.image_embeds, torch.from_numpy(G["image_embeds"])) <= 2e-2
    print(f"golden tower: mfma vs fma relative L2 {rel(out.last_hidden_state, off.last_hidden_state):.3e}")
    C.set_attention_kernel(m, "fma")
    m(pix)
    assert ops.attn_hd_launch_counts() == n0 + layers


def test_openclip_tower_opts_in_through_the_embedder(hip):
    from motionrag_amd import clip_vision as C
    from motionrag_amd import ops
    emb = C.FrozenOpenCLIPImageEmbedderV2(width=160, layers=2, heads=2, mlp_ratio=2.0).to(DEV, torch.bfloat16)
    x = (torch.rand(1, 3, 320, 512) * 2 - 1).to(DEV, torch.bfloat16)
    n0 = ops.attn_hd_launch_counts()
    off = emb(x)
    assert ops.attn_hd_launch_counts() == n0
    on = C.set_attention_kernel(emb, "mfma")(x)
    assert ops.attn_hd_launch_counts() == n0 + 2 and on.shape == off.shape == (1, 257, 160)
    assert rel(on, off) <= 1e-2


def test_tower_at_336_px_runs_without_a_switch(hip):
    """577 tokens of 2 heads of 80: 577 * 80 > 32 768, the fp32-FMA kernel refuses and the block routes to the MFMA kernel by the rule alone"""
    from motionrag_amd import clip_vision as C
    from motionrag_amd import ops
    torch.manual_seed(23)
    m = C.CLIPVisionModelWithProjection(hidden_size=160, intermediate_size=320, num_hidden_layers=1, num_attention_heads=2, image_size=336, patch_size=14, projection_dim=64)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p)) if "class_embedding" not in n else p.normal_(0.0, 0.02)
            elif "position_embedding" in n:
                p.normal_(0.0, 0.02)
            p.copy_(p.to(torch.bfloat16).float())
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    pix = torch.randn(2, 3, 336, 336)
    want_last, want_emb = R.clip_vision(sd, 2, pix.to(torch.bfloat16).float())
    assert m.attention_kernel == "fma"
    n0 = ops.attn_hd_launch_counts()
    out = m.to(DEV, torch.bfloat16)(pix.to(DEV, torch.bfloat16))
    assert ops.attn_hd_launch_counts() == n0 + 1
    assert out.last_hidden_state.shape == (2, 577, 160) and out.image_embeds.shape == (2, 64)
    assert rel(out.last_hidden_state, want_last) <= 2e-2 and rel(out.image_embeds, want_emb) <= 2e-2
