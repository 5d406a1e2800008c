"""The opt-in fp8 (e4m3) joint attention of the CogVideoX DiT (mrag_attn_joint_fwd_fp8, ops.joint_attention_fp8, cogvideox.set_attention_precision): key counts that
are no multiple of the 128-key stage -- the last stage is zero-padded by the quantiser and masked in the kernel -- and a Q that already carries scale * log2 e.

References and tolerances are those of tests/test_gpu_fp8.py (helpers restated here; the emulation takes the multiplier c as an argument, c = 1 for a
pre-scaled Q, and zero-pads P to whole 64-key tiles for `lazy_ok`):
    against fp32 attention   relative Frobenius error <= 8 %, and > 99 % of the elements within 10 % of |want| + 0.25 x the mean magnitude
    against the fp32 emulation of the same quantisation   <= 1.2 % over the rows the emulation models (`lazy_ok`, which may exclude at most 1 % of the rows)
At model level the bound is the one of tests/test_gpu_fp8_linear.py: G_model <= 1.5 E_model + 0.02, E_model being the error of the fp32 oracle run on the
emulated attention."""
import functools
import math
import re
import threading

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG2E = 1.4426950408889634
C_PRE = 0.125 * LOG2E                      # what the QKV GEMM's epilogue multiplies Q by (q_premul)


def bf(x):
    return x.to(torch.bfloat16)


def e4m3(x):
    """round-to-nearest-even onto OCP e4m3fn (max 448, subnormals down to 2^-9)"""
    return x.to(torch.float8_e4m3fn).float()


def pow2_fit(amax):
    if not amax > 0:
        return 0
    e = math.floor(math.log2(448.0 / amax))
    if amax * 2.0 ** e > 448.0:
        e -= 1
    if amax * 2.0 ** (e + 1) <= 448.0:
        e += 1
    return e


def sdpa_fp32(q, k, v, scale=0.125):
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.float()).reshape(q.shape[0], q.shape[1], -1)


def sdpa_fp8_emulated(q, k, v, c=C_PRE):
    """what the kernel computes, in fp32 arithmetic: per-(b, h) power-of-two scales, e4m3 operands (Q times c: scale * log2 e, or 1 when Q carries it already),
    exact softmax with P' = 4 P quantised (numerator AND row sum), centred on the maximum of the row's first 64 keys.  q [B, Sq, H, 64], k / v [B, Skv, H, 64]"""
    B, Sq, H, _ = q.shape
    Skv = k.shape[1]
    out = torch.empty(B, Sq, H, 64)
    lazy_ok = torch.ones(B, Sq, H, dtype=torch.bool)
    for b in range(B):
        for h in range(H):
            qq, kk, vv = q[b, :, h].float(), k[b, :, h].float(), v[b, :, h].float()
            y, ek, ev = pow2_fit(qq.abs().max().item() * c), pow2_fit(kk.abs().max().item()), pow2_fit(vv.abs().max().item())
            q8, k8, v8 = e4m3(qq * (c * 2.0 ** y)), e4m3(kk * 2.0 ** ek), e4m3(vv * 2.0 ** ev)
            s = (q8 @ k8.T) * 2.0 ** -(y + ek)                       # log2-domain scores
            p = torch.exp2(s - s[:, :64].amax(-1, keepdim=True) + 2.0)
            # rows whose 64-key tile sum of P' reaches e4m3's largest value re-centre in the kernel: excluded by the caller, with a margin.  The kernel's tiles
            # are whole: the padding keys of the last one hold P' = 0
            pp = F.pad(p, (0, -Skv % 64))
            lazy_ok[b, :, h] = pp.view(Sq, -1, 64).sum(-1).amax(-1) <= 400.0
            p8 = e4m3(p.clamp(max=448.0))
            out[b, :, h] = (p8 @ v8) / p8.sum(-1, keepdim=True) * 2.0 ** -ev
    return out.reshape(B, Sq, H * 64), lazy_ok


def rel_l2(got, want):
    g, w = got.float().cpu(), want.float().cpu()
    return ((g - w).norm() / w.norm()).item()


# (B, H, Sq, Skv, pre-scaled Q)
CASES = [(1, 3, 300, 513, False),      # one real key in the tail stage, its second sub-tile all padding; tail in LDS stage slot 0
         (1, 2, 512, 576, True),       # exactly one whole sub-tile real
         (2, 2, 257, 639, True),       # 127 real tail keys; one query row in the second query tile
         (1, 2, 256, 700, True),       # tail in stage slot 1
         (1, 2, 256, 850, False),      # tail in stage slot 2
         (1, 2, 256, 1000, True),      # tail in stage slot 3
         (1, 2, 256, 1100, True)]      # the four-stage unrolled loop runs twice before the tail


@functools.lru_cache(maxsize=None)
def _case(B, H, Sq, Skv, pre):
    """inputs (host, bf16, strided views of one fused buffer) and both references of one case: computed once, shared, never modified"""
    g = torch.Generator().manual_seed(100 * B + H + Skv)
    x = torch.randn(B, max(Sq, Skv), 3, H, 64, generator=g) * torch.tensor([1.5, 0.7, 2.0]).view(1, 1, 3, 1, 1)
    if pre:
        x[:, :, 0] *= C_PRE                                           # before the bf16 rounding, as the GEMM epilogue does
    qkv = bf(x)
    q, k, v = qkv[:, :Sq, 0], qkv[:, :Skv, 1], qkv[:, :Skv, 2]
    want = sdpa_fp32(q, k, v, scale=math.log(2.0) if pre else 0.125)   # a pre-scaled Q's scores are in the log2 domain
    emu, ok = sdpa_fp8_emulated(q, k, v, c=1.0 if pre else C_PRE)
    return qkv, want, emu, ok


def _run(qkv_dev, Sq, Skv, pre, **kw):
    from motionrag_amd import ops
    return ops.joint_attention_fp8(qkv_dev[:, :Sq, 0], qkv_dev[:, :Skv, 1], qkv_dev[:, :Skv, 2], q_prescaled=pre, **kw)


def _check_both(got, want, emu, ok, tag):
    B, Sq, HD = want.shape
    assert got.shape == want.shape and torch.isfinite(got.float()).all(), tag
    g = got.float().cpu()
    err = rel_l2(g, want)
    d = (g - want).abs()
    near = (d <= 0.10 * want.abs() + 0.25 * want.abs().mean()).float().mean().item()
    share = ok.float().mean().item()
    sel = ok.unsqueeze(-1).expand(B, Sq, HD // 64, 64).reshape(B, Sq, HD)
    e2 = ((g - emu)[sel].norm() / emu[sel].norm()).item()
    print(f"{tag}: vs fp32 {err:.4f} (<= 0.08), within the element bound {near:.4f} (> 0.99), lazy_ok share {share:.4f} (> 0.99), vs emulation {e2:.4f} (<= 0.012)")
    assert err <= 0.08, f"{tag}: relative Frobenius error {err:.4f} > 0.08"
    assert near > 0.99, f"{tag}: {near:.4f} of the elements within 10 % + 0.25 mean"
    assert share > 0.99, f"{tag}: lazy_ok keeps {share:.4f} of the rows"
    assert e2 <= 0.012, f"{tag}: kernel vs the fp32 emulation of the same quantisation: {e2:.4f}"


# ------------------------------------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("B,H,Sq,Skv,pre", CASES)
def test_joint_fp8_attention_matches_both_references(hip, B, H, Sq, Skv, pre):
    qkv, want, emu, ok = _case(B, H, Sq, Skv, pre)
    dq = qkv.to(DEV)
    got = _run(dq, Sq, Skv, pre)
    _check_both(got, want, emu, ok, f"Skv={Skv} pre={pre}")
    if Skv == 639:                                                    # fused residual + out_scale, same contract as the bf16 entry point
        resid = bf(torch.randn(B, Sq, H * 64, generator=torch.Generator().manual_seed(7)))
        fused = _run(dq, Sq, Skv, pre, resid=resid.to(DEV), out_scale=0.5)
        assert rel_l2(fused, resid.float() + 0.5 * want) <= 0.04


# ------------------------------------------------------------------------------------------------------------------------ 2. stale workspace
def test_joint_fp8_padding_owes_nothing_to_the_workspace(hip):
    """the workspace is a shared grow-only buffer: whatever it held (0x7F is NaN in e4m3fn), the padding keys are written on every call"""
    from motionrag_amd import _lib, ops
    B, H, Sq, Skv, pre = CASES[0]
    qkv, want, emu, ok = _case(B, H, Sq, Skv, pre)
    dq = qkv.to(DEV)
    need = _lib.lib().mrag_attn_joint_fp8_workspace_bytes(B, H, Sq, Skv)
    outs = []
    for fill in (0x7F, 0x00):
        ws = ops._attn_workspace(torch.device(DEV, torch.cuda.current_device()), need, "fp8")
        assert ws.numel() >= need
        ws.fill_(fill)
        outs.append(_run(dq, Sq, Skv, pre).clone())
    _check_both(outs[0], want, emu, ok, "workspace full of 0x7F")
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------------ 3. the old contract
def test_joint_fp8_keeps_the_old_entry_point(hip):
    from motionrag_amd import ops
    B, H, Sq, Skv = 1, 2, 384, 640
    g = torch.Generator().manual_seed(100 * B + H + Skv)
    qkv = bf(torch.randn(B, Skv, 3, H, 64, generator=g) * torch.tensor([1.5, 0.7, 2.0]).view(1, 1, 3, 1, 1)).to(DEV)
    q, k, v = qkv[:, :Sq, 0], qkv[:, :, 1], qkv[:, :, 2]
    with ops.dispatched() as d:
        new = ops.joint_attention_fp8(q, k, v)
    assert d.counts == {"ATTN_FP8": 1}, d.counts                       # one launch of the family; ATTN16 / ATTN_FLASH did not move
    old = ops.attention(q, k, v, fp8=True)
    assert torch.equal(new, old)                                      # whole stages, Q not pre-scaled: the very kernels of mrag_attn_fwd_fp8
    x = torch.zeros(1, 576, 2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.attention(x, x, x, fp8=True)                              # the UNets' entry point still refuses Skv % 128 != 0
    with ops.dispatched() as d:
        ops.joint_attention_fp8(x, x, x, q_prescaled=True)            # ... which the joint one takes
    assert d.counts == {"ATTN_FP8": 1}, d.counts
    short = torch.zeros(1, 511, 2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.joint_attention_fp8(short, short, short)


# ------------------------------------------------------------------------------------------------------------------------ 4. determinism, capture
def test_joint_fp8_is_deterministic_and_captures(hip):
    """no host synchronisation, nothing read back: a straight-line graph (one memset, three kernels) whose replay equals the eager result bit for bit"""
    B, H, Sq, Skv, pre = CASES[2]
    qkv, _, _, _ = _case(B, H, Sq, Skv, pre)
    dq = qkv.to(DEV)
    eager = _run(dq, Sq, Skv, pre).clone()                            # warm: the workspace is grown
    assert torch.equal(_run(dq, Sq, Skv, pre), eager)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.HIPGraph() if hasattr(torch.cuda, "HIPGraph") else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(dq, Sq, Skv, pre, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------------------------------ 5. model level
BLOCK_WEIGHT = re.compile(r"transformer_blocks\.\d+\.(attn1\.to_[qkv]|attn1\.to_out\.0|ff\.net\.0\.proj|ff\.net\.2)\.weight$")
LAYERS = 2
LONG = dict(frames=5, height=16, width=28)        # 5 x 8 x 14 patches + 10 text rows = 570 joint rows: 570 % 128 = 58
E_ATTN_BRACKET = (0.0003, 0.003)                  # E_model of the unmodified oracle on the emulated attention: 0.0010 measured on the host (E_lin: 0.0150)
SHORT = dict(frames=3, height=8, width=12)        # the 82-row model of the other model tests: below the fp8 kernel's 512 keys


def _oracle_dit(geom, seed=31):
    from oracle import cogvideox_ref
    cfg = cogvideox_ref.DiTConfig(num_layers=LAYERS, heads=2, in_channels=16, out_channels=8, time_embed_dim=64, text_embed_dim=64,
                                  max_text_len=10, ip_dim=64, **geom)
    return cfg, cogvideox_ref.random_dit_sd(cfg, seed=seed, std=0.08)


def _small_dit(geom, seed=31):
    """the two-layer reduced DiT of tests/test_gpu_fp8_linear.py (heads = 2, D = 128, FF 512, std 0.08, motion adapters installed) at a given latent geometry"""
    from motionrag_amd.cogvideox import CogVideoXTransformer3DModel
    cfg, sd = _oracle_dit(geom, seed)
    model = CogVideoXTransformer3DModel(num_layers=LAYERS, num_attention_heads=2, in_channels=16, out_channels=8, time_embed_dim=64,
                                        text_embed_dim=64, max_text_seq_length=10, sample_frames=geom["frames"], sample_height=geom["height"],
                                        sample_width=geom["width"])
    model.install_motion_adapters(64)
    model.load_state_dict(sd, strict=True)
    return cfg, sd, model.to(DEV, torch.bfloat16)


def _dit_inputs(geom, seed=32):
    from oracle import cogvideox_ref
    f, h, w = geom["frames"], geom["height"], geom["width"]
    g = torch.Generator().manual_seed(seed)
    lat, img = (bf(torch.randn(1, f, 8, h, w, generator=g)) for _ in range(2))
    text = bf(torch.randn(2, 10, 64, generator=g))
    ip = bf(torch.randn(2, 25, 64, generator=g))
    t = torch.tensor([481.0, 481.0])
    cos, sin = cogvideox_ref.rope_3d(64, f, h // 2, w // 2)
    return lat, img, text, ip, t, cos, sin


def _forward(model, inp, **kw):
    lat, img, text, ip, t, cos, sin = inp
    return model(lat.to(DEV), text.to(DEV), t.to(DEV), image_rotary_emb=((cos.to(DEV), sin.to(DEV)), ip.to(DEV)), image_latents=img.to(DEV), batch=2, **kw)


def _quant_rows(x):
    """tests/test_gpu_fp8_linear.py's reference of mrag_quant_rows_e4m3, dequantised: per-row power-of-two scale, e4m3 round-to-nearest"""
    amax = x.float().abs().amax(-1, keepdim=True)
    e = torch.floor(torch.log2(448.0 / amax.clamp_min(1e-30)))
    e = torch.where(amax * torch.exp2(e) > 448.0, e - 1, e)
    e = torch.where(amax * torch.exp2(e + 1) <= 448.0, e + 1, e)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    return e4m3(x.float() * torch.exp2(e)) * torch.exp2(-e)


@functools.lru_cache(maxsize=None)
def _long_model_references():
    """the fp32 oracle on the 570-row model, the same oracle with its joint attention on the fp8 emulation (E_attn), and with its six large weights per
    block on reference-quantised operands (E_lin, as tests/test_gpu_fp8_linear.py does): computed once, shared by the two model-level tests"""
    from oracle import cogvideox_ref
    cfg, sd = _oracle_dit(LONG)
    lat, img, text, ip, t, cos, sin = _dit_inputs(LONG)
    sdr = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    x = torch.cat([torch.cat([lat] * 2), torch.cat([img] * 2)], dim=2).float()
    run = lambda: cogvideox_ref.dit_forward(sdr, cfg, x, text.float(), t, (cos, sin), ip.float())
    want = run()
    mp = pytest.MonkeyPatch()
    try:
        plain_sdpa, hits = cogvideox_ref._sdpa, []

        def emulated_sdpa(q, k, v):                                   # [b, heads, S, 64]
            if k.shape[-2] <= 32:
                return plain_sdpa(q, k, v)                            # the 25-key motion branch stays plain
            hits.append(k.shape[-2])
            o, _ = sdpa_fp8_emulated(bf(q.transpose(1, 2) * C_PRE), bf(k.transpose(1, 2)), bf(v.transpose(1, 2)), c=1.0)   # the kernel's operands are bf16
            return o.view(q.shape[0], q.shape[2], q.shape[1], 64).transpose(1, 2)

        mp.setattr(cogvideox_ref, "_sdpa", emulated_sdpa)
        emu_attn = run()
        mp.undo()
        assert hits == [570] * LAYERS, hits                           # once per layer
        patched = {id(v) for k, v in sdr.items() if BLOCK_WEIGHT.search(k)}
        plain_linear, lhits = F.linear, []

        def quantised_linear(inp_, weight, bias=None):
            if id(weight) not in patched:
                return plain_linear(inp_, weight, bias)
            lhits.append(id(weight))
            return plain_linear(_quant_rows(bf(inp_)), _quant_rows(weight), bias)

        mp.setattr(torch.nn.functional, "linear", quantised_linear)
        emu_lin = run()
        mp.undo()
        assert len(lhits) == 6 * LAYERS
    finally:
        mp.undo()
    return want, rel_l2(emu_attn, want), rel_l2(emu_lin, want)


def test_dit_fp8_attention_against_oracle(hip):
    from motionrag_amd import cogvideox, ops
    want, E_attn, E_lin = _long_model_references()
    cfg, sd, model = _small_dit(LONG)
    inp = _dit_inputs(LONG)
    never_switched = _forward(model, inp).clone()

    cogvideox.set_attention_precision(model, "fp8")
    with ops.dispatched() as d:
        got = _forward(model, inp).clone()
    assert d.counts.get("ATTN_FP8", 0) == LAYERS, d.counts
    assert torch.isfinite(got.float()).all()
    G_attn = rel_l2(got, want)
    print(f"fp8-attention DiT ({LAYERS} layers, 570 rows): E_model = {E_attn:.4f}, kernel path = {G_attn:.4f}, bound = {1.5 * E_attn + 0.02:.4f}")
    assert E_ATTN_BRACKET[0] < E_attn < E_ATTN_BRACKET[1], E_attn
    assert G_attn <= 1.5 * E_attn + 0.02, (G_attn, E_attn)
    assert not torch.equal(got, never_switched)

    # both switches on: finite, and within the sum of the two bounds
    cogvideox.set_linear_precision(model, "fp8")
    with ops.dispatched() as d:
        both = _forward(model, inp).clone()
    assert d.counts.get("ATTN_FP8", 0) == LAYERS, d.counts
    G_both = rel_l2(both, want)
    print(f"fp8 attention + fp8 linears: E_lin = {E_lin:.4f}, kernel path = {G_both:.4f}, bound = {(1.5 * E_attn + 0.02) + (1.5 * E_lin + 0.02):.4f}")
    assert torch.isfinite(both.float()).all()
    assert G_both <= (1.5 * E_attn + 0.02) + (1.5 * E_lin + 0.02), (G_both, E_attn, E_lin)
    cogvideox.set_linear_precision(model, "bf16")

    # switching back: the never-switched model bit for bit, and no fp8 attention launch
    cogvideox.set_attention_precision(model, "bf16")
    with ops.dispatched() as d:
        back = _forward(model, inp)
    assert "ATTN_FP8" not in d.counts, d.counts
    assert torch.equal(back, never_switched)


def test_dit_fp8_attention_leaves_short_sequences_on_bf16(hip):
    """82 joint rows: below the kernel's 512 keys, so 'fp8' launches no fp8 attention and changes nothing"""
    from motionrag_amd import cogvideox, ops
    cfg, sd, model = _small_dit(SHORT)
    inp = _dit_inputs(SHORT)
    ref = _forward(model, inp).clone()
    cogvideox.set_attention_precision(model, "fp8")
    with ops.dispatched() as d:
        got = _forward(model, inp)
    assert "ATTN_FP8" not in d.counts, d.counts
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------------------------------ 6. sharded
def test_dit_fp8_attention_sequence_parallel(hip):
    """the harness of tests/test_gpu_models.py::test_sequence_parallel_dit_equals_unsharded (two threads with their own streams as two ranks) on the 570-row
    model: 285 query rows per rank against the 570 gathered keys, read through strides.  The per-head Q scales come from the rank's own rows, so the ranks
    need not equal the unsharded fp8 run: each is held to the model-level bound against the oracle."""
    from motionrag_amd import cogvideox, ops
    from motionrag_amd.dist import SequenceParallel
    want, E_attn, _ = _long_model_references()
    cfg, sd, model = _small_dit(LONG)
    inp = _dit_inputs(LONG)
    _forward(model, inp)                                              # builds the fused-weight caches
    cogvideox.set_attention_precision(model, "fp8")
    torch.cuda.synchronize()
    world = 2
    slots, bar, outs, errs = [None] * world, threading.Barrier(world), [None] * world, []

    def gather_for(rank):
        def ag(x):
            torch.cuda.current_stream().synchronize()
            slots[rank] = x.contiguous()
            bar.wait()
            out = torch.cat(list(slots), dim=0)
            torch.cuda.current_stream().synchronize()
            bar.wait()
            return out
        return ag

    def run(rank):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                outs[rank] = _forward(model, inp, sp=SequenceParallel(rank, world, all_gather=gather_for(rank)))
                torch.cuda.current_stream().synchronize()
        except Exception as e:                                        # surface thread failures in the test
            errs.append(e)
            bar.abort()

    before = ops.dispatch_counts()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [x.start() for x in th]
    [x.join(timeout=120) for x in th]
    assert not errs, errs
    assert ops.dispatch_counts()["ATTN_FP8"] - before["ATTN_FP8"] == world * LAYERS
    for r in range(world):
        assert outs[r] is not None and outs[r].shape == want.shape and torch.isfinite(outs[r].float()).all()
        G = rel_l2(outs[r], want)
        print(f"rank {r}: kernel path = {G:.4f}, bound = {1.5 * E_attn + 0.02:.4f}")
        assert G <= 1.5 * E_attn + 0.02, (r, G, E_attn)
