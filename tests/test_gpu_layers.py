"""The derived-weight caches on the DiT's hot path (layers.WeightCache behind attn_processor / cogvideox): built once, served while nothing changed, and never
stale -- after every kind of update the cached path equals, bit for bit, a freshly constructed module that loaded the same final weights and tokens."""
import pytest
import torch
from torch import nn

from test_gpu_models import _small_dit

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, H, CROSS, TEXT, VIDEO, B = 128, 2, 64, 8, 56, 2


def _toy(state=None):
    """Attention (2 heads of 64, qk-norm) + its motion adapter processor on the GPU: seeded weights, or those of `state`"""
    from motionrag_amd.attn_processor import APAdapterCogVideoXAttnProcessor2_0, Attention
    attn = Attention(D, heads=H, dim_head=64, bias=True, out_bias=True, qk_norm="layer_norm", eps=1e-6)
    proc = APAdapterCogVideoXAttnProcessor2_0(D, CROSS)
    attn.set_processor(proc)
    if state is None:
        g = torch.Generator().manual_seed(61)
        for p in attn.parameters():
            nn.init.normal_(p, std=0.15, generator=g)
        for n in ("norm_q", "norm_k"):
            getattr(attn, n).weight.data.add_(1.0)
    else:
        attn.load_state_dict(state)
    return attn.to(DEV, torch.bfloat16), proc


def test_joint_attention_caches_build_once_and_never_serve_stale(hip):
    from motionrag_amd import ops
    from motionrag_amd.attn_processor import joint_attention_core
    from motionrag_amd.cogvideox import get_3d_rotary_pos_embed
    attn, proc = _toy()
    g = torch.Generator().manual_seed(62)
    x = torch.randn(B, TEXT + VIDEO, D, generator=g).to(DEV, torch.bfloat16)
    ip = torch.randn(1, 4, CROSS, generator=g).to(DEV, torch.bfloat16)
    rope = tuple(t.to(DEV) for t in get_3d_rotary_pos_embed(64, 2, 4, 7))
    assert rope[0].shape == (VIDEO, 64)

    def run(attn, proc, ip, rope):
        with ops.dispatched() as d:
            o = joint_attention_core(attn, proc, x, TEXT, rope, ip, 1.0)
        return o, sum(d.counts.values())

    def fresh():
        """a new Attention + processor loaded with the current weights, on copies of the current tokens and tables: nothing cached"""
        a, p = _toy({k: v.float().cpu() for k, v in attn.state_dict().items()})
        return run(a, p, ip.clone(), tuple(t.clone() for t in rope))[0]

    (o1, n1), (o2, n2), (o3, n3) = (run(attn, proc, ip, rope) for _ in range(3))
    assert n2 == n3 < n1, f"launches per call {n1}, {n2}, {n3}: the folded motion keys are built once per clip"
    assert torch.equal(o1, o2) and torch.equal(o1, o3) and torch.equal(o1, fresh())

    ip.mul_(1.5)                                                              # same tokens object, new content
    o4, n4 = run(attn, proc, ip, rope)
    assert n4 == n1 and not torch.equal(o4, o1) and torch.equal(o4, fresh())

    attn.to_q.weight = nn.Parameter(torch.randn(D, D, generator=g).mul_(0.15).to(DEV, torch.bfloat16))   # a new weight object
    o5, n5 = run(attn, proc, ip, rope)
    assert n5 == n2 and not torch.equal(o5, o4) and torch.equal(o5, fresh())


def test_dit_modulation_weights_follow_every_block(hip):
    """an in-place update of ANY block's modulation linear reaches the step's one concatenated modulation GEMM (not only block 0's and norm_out's)"""
    from oracle import cogvideox_ref
    cfg, sd, model = _small_dit(seed=63)
    g = torch.Generator().manual_seed(64)
    lat, img = (torch.randn(1, 3, 8, 8, 12, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    text = torch.randn(2, 10, 64, generator=g).to(DEV, torch.bfloat16)
    ip = torch.randn(2, 25, 64, generator=g).to(DEV, torch.bfloat16)
    t = torch.tensor([481.0, 481.0], device=DEV)
    cos, sin = (x.to(DEV) for x in cogvideox_ref.rope_3d(64, 3, 4, 6))
    step = lambda m: m(lat, text, t, image_rotary_emb=((cos, sin), ip), image_latents=img, batch=2)
    before = step(model)
    with torch.no_grad():
        model.transformer_blocks[1].norm1.linear.weight.mul_(2)
    after = step(model)
    _, _, other = _small_dit(seed=63)
    other.load_state_dict(model.state_dict())
    assert not torch.equal(after, before) and torch.equal(after, step(other))
