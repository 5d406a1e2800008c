"""`layers.WeightCache` on plain CPU tensors (no library load): when a derived weight is served, when it is rebuilt, and when its entry goes;
plus the import graph -- the encoders do not pull in a UNet file, the SVD UNet does not pull in the DynamiCrafter one, `layers` pulls in no model file --
the one FeedForward / GEGLU class the UNets share, and the SVD UNet's and VAE's checkpoint layout (tests/golden/svd_keys.json)."""
import gc
import json
import os
import subprocess
import sys

import torch
from torch import nn

from motionrag_amd.layers import WeightCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Builder:
    """build() that counts its calls and returns a fresh copy of what it reads"""

    def __init__(self, *tensors):
        self.tensors, self.calls = tensors, 0

    def __call__(self):
        self.calls += 1
        return torch.cat([t.detach().reshape(-1) for t in self.tensors if t is not None]).clone()


def test_unchanged_refs_hit():
    c, lin = WeightCache(), nn.Linear(4, 3)
    b = _Builder(lin.weight)
    first = c.get("k", lin.weight, b)
    assert c.get("k", lin.weight, b) is first and b.calls == 1


def test_in_place_updates_rebuild():
    c, lin = WeightCache(), nn.Linear(4, 3)
    b = _Builder(lin.weight)
    c.get("k", lin.weight, b)
    with torch.no_grad():
        lin.weight.mul_(2.0)
    got = c.get("k", lin.weight, b)
    assert b.calls == 2 and torch.equal(got, lin.weight.detach().reshape(-1))
    with torch.no_grad():
        lin.weight.copy_(torch.ones(3, 4))
    c.get("k", lin.weight, b)
    assert b.calls == 3
    lin.load_state_dict({"weight": torch.full((3, 4), 5.0), "bias": torch.zeros(3)})
    got = c.get("k", lin.weight, b)
    assert b.calls == 4 and torch.equal(got, torch.full((12,), 5.0))
    assert c.get("k", lin.weight, b) is got and b.calls == 4 and len(c.d) == 1


def test_new_parameter_under_the_same_key_rebuilds_even_at_an_equal_tag():
    c, lin = WeightCache(), nn.Linear(4, 3)
    lin.weight = old = nn.Parameter(torch.ones(3, 4))
    c.get("k", lin.weight, _Builder(old))
    lin.weight = new = nn.Parameter(old.data)                # another object over the SAME storage: address, dtype and version all equal
    assert new is not old and (new.data_ptr(), new.dtype, new._version) == (old.data_ptr(), old.dtype, old._version)
    b = _Builder(new)
    c.get("k", lin.weight, b)
    assert b.calls == 1
    lin.weight = nn.Parameter(torch.zeros(3, 4))             # and the ordinary case: fresh storage
    b = _Builder(lin.weight)
    assert torch.equal(c.get("k", lin.weight, b), torch.zeros(12)) and b.calls == 1


def test_dtype_change_rebuilds():
    c, lin = WeightCache(), nn.Linear(4, 3)
    b = _Builder(lin.weight)
    c.get("k", lin.weight, b)
    w = lin.weight
    lin.to(torch.float64)                                    # same Parameter object, new dtype
    assert lin.weight is w and w.dtype == torch.float64
    assert c.get("k", lin.weight, b).dtype == torch.float64 and b.calls == 2


def test_none_among_the_refs_is_ignored():
    c, lin = WeightCache(), nn.Linear(4, 3, bias=False)
    b = _Builder(lin.weight, lin.bias)
    first = c.get("k", (lin.weight, lin.bias), b)
    assert c.get("k", (lin.weight, None), b) is first and c.get("k", lin.weight, b) is first and b.calls == 1


def test_any_member_of_a_tuple_rebuilds():
    c = WeightCache()
    lins = [nn.Linear(4, 3) for _ in range(3)]
    refs = lambda: tuple(m.weight for m in lins) + tuple(m.bias for m in lins)
    b = _Builder(*refs())
    c.get("k", refs(), b)
    for n, t in enumerate(refs(), start=2):
        with torch.no_grad():
            t.add_(1.0)
        c.get("k", refs(), b)
        assert b.calls == n
        c.get("k", refs(), b)
        assert b.calls == n
    lins[1].bias = nn.Parameter(torch.zeros(3))
    b2 = _Builder(*refs())
    c.get("k", refs(), b2)
    assert b2.calls == 1


def test_entry_goes_with_its_module():
    c = WeightCache()
    keep, gone = nn.Linear(4, 3), nn.Linear(4, 3)
    c.get(("w", "keep"), keep.weight, _Builder(keep.weight))
    c.get(("w", "gone"), (gone.weight, gone.bias), _Builder(gone.weight, gone.bias))
    assert len(c.d) == 2
    del gone
    gc.collect()
    assert list(c.d) == [("w", "keep")]


def test_rebuilt_entry_survives_the_tensor_it_replaced():
    c = WeightCache()
    old, new = nn.Parameter(torch.ones(3)), nn.Parameter(torch.zeros(3))
    c.get("k", old, _Builder(old))
    stale = c.d["k"]                                         # keeps the replaced entry's weak references (and their callbacks) alive
    b = _Builder(new)
    first = c.get("k", new, b)
    del old
    gc.collect()
    assert stale[1][0]() is None
    assert c.get("k", new, b) is first and b.calls == 1


def test_clear():
    c, lin = WeightCache(), nn.Linear(4, 3)
    b = _Builder(lin.weight)
    c.get("a", lin.weight, b)
    c.get("b", lin.bias, b)
    c.clear()
    assert not c.d
    c.get("a", lin.weight, b)
    assert b.calls == 3


MODEL_FILES = ("dynamicrafter", "dynamicrafter_vae", "svd", "svd_unet", "svd_vae", "cogvideox", "cogvideox_vae", "attn_processor", "cama", "t5", "clip_vision",
               "encoders", "text_embedder", "openclip_text", "rag", "dynamicrafter_pipeline")


def test_encoders_do_not_import_a_unet_file():
    for imports, absent in ((("t5", "clip_vision", "encoders", "text_embedder", "openclip_text"), ("dynamicrafter",)),
                            (("svd_unet",), ("dynamicrafter",)),
                            (("layers",), MODEL_FILES)):
        code = (f"import sys, {', '.join('motionrag_amd.' + m for m in imports)}; "
                f"bad = [m for m in {absent!r} if 'motionrag_amd.' + m in sys.modules]; print(bad); sys.exit(1 if bad else 0)")
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr or f"importing {imports} imported {r.stdout}"


def test_one_feed_forward_class():
    from motionrag_amd import dynamicrafter, layers, svd_unet
    assert dynamicrafter.FeedForward is svd_unet.FeedForward is layers.FeedForward
    assert dynamicrafter.GEGLU is svd_unet.GEGLU is layers.GEGLU
    assert dynamicrafter.TembBank is layers.TembBank and dynamicrafter.temb_proj is layers.temb_proj
    ff = layers.FeedForward(8, dim_out=16, mult=2)
    assert {k: tuple(v.shape) for k, v in ff.state_dict().items()} == {"net.0.proj.weight": (32, 8), "net.0.proj.bias": (32,), "net.2.weight": (16, 16), "net.2.bias": (16,)}
    holder = nn.Module()
    holder.ff, holder.other = ff, nn.Linear(8, 8)
    layers.set_ff_precision(holder, "fp8", sites=("ff2",))
    layers.set_ff_fusion(holder, True)
    assert getattr(ff, layers.FF_SITES_ATTR) == ("ff2",) and getattr(ff, layers.FF_FUSION_ATTR) is True
    assert not hasattr(holder.other, layers.FF_SITES_ATTR) and not hasattr(holder.other, layers.FF_FUSION_ATTR)
    layers.set_ff_precision(holder, "bf16")
    layers.set_ff_fusion(holder, False)
    assert getattr(ff, layers.FF_SITES_ATTR) == () and getattr(ff, layers.FF_FUSION_ATTR) is False


def svd_layouts():
    """sorted (key, shape) lists of the reduced SVD UNet (tests/test_oracle_golden.svd_tiny, plain and with the motion adapters installed) and of the reduced
    and the default temporal-decoder VAE (tests/test_gpu_svd_vae.py)"""
    from motionrag_amd import svd, svd_unet, svd_vae
    cfg = dict(in_channels=8, out_channels=4, block_out_channels=(64, 128), addition_time_embed_dim=64, projection_class_embeddings_input_dim=192,
               layers_per_block=1, cross_attention_dim=64, num_attention_heads=(1, 2))
    unet = svd_unet.UNetSpatioTemporalConditionModel(**cfg)
    mods = {"unet": svd_unet.UNetSpatioTemporalConditionModel(**cfg), "unet_motion": unet,
            "vae_64_128": svd_vae.AutoencoderKLTemporalDecoder(block_out_channels=(64, 128), layers_per_block=1), "vae_default": svd_vae.AutoencoderKLTemporalDecoder()}
    names = [n for n in unet.attn_processors if "temporal_transformer_blocks" not in n and n.endswith("attn2.processor")]
    svd.set_attention_processors(unet, names, 64, {n: dict(unet.named_modules())[n[: -len(".processor")]].to_q.in_features for n in names})
    return {name: [[k, list(v.shape)] for k, v in sorted(m.state_dict().items())] for name, m in mods.items()}


def test_svd_checkpoint_layout():
    with open(os.path.join(ROOT, "tests", "golden", "svd_keys.json")) as f:
        want = json.load(f)
    got = svd_layouts()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
