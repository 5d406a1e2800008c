"""What the model files share: the derived-weight cache, the bf16 view of a parameter, the empty state-dict namespace, the 3x3 / (3,1,1)
convolutions as GEMMs, the pre-LayerNorm transformer block, and ONE body for every block the UNets and VAEs have in common -- `groupnorm_rows`, the spatial and
temporal residual blocks (`resnet2d`, `resnet_t3`), the GEGLU `FeedForward` with its opt-in paths, the UNets' attention core (`self_attention`, `kv_proj`,
`linear_resid`), the VAEs' single-head attention, and the timestep plumbing (`TembBank`, `temb_proj`, `temb_bank`, `silu_mlp`).  The model classes keep their
constructors (hence their state-dict keys) and hand their sub-modules to these functions.  Host plumbing only: every launch goes through `ops`; this file imports
no model file."""
from __future__ import annotations

import itertools
import weakref
from typing import Optional

import torch
from torch import nn

from . import ops


class WeightCache:
    """weights re-laid-out once per weight tensor: conv kernels as [Cout, (ky, kx, cin)] GEMM operands, fused Q|K|V projections, GEGLU row
    interleaves, folded motion keys.  An entry is valid only for the SAME tensor objects (weak references: `id()` and the storage address of
    a collected tensor can be reused), at the same storage address, dtype and in-place version (`load_state_dict` copies in place).  It
    holds its tensors weakly and is dropped when any of them is collected, so the derived copy does not outlive the module it came from."""

    def __init__(self):
        self.d = {}

    def get(self, key, refs, build):
        """`refs`: the tensor -- or a tuple of ALL tensors (None entries allowed) -- that `build` reads: replacing or updating any one of
        them in place invalidates the entry, which `build()` then replaces under `key`"""
        refs = tuple(r for r in (refs if isinstance(refs, (tuple, list)) else (refs,)) if r is not None)
        tag = tuple((r.data_ptr(), r.dtype, r._version) for r in refs)
        ent = self.d.get(key)
        if ent is None or ent[0] != tag or any(w() is not r for w, r in zip(ent[1], refs)):
            token, cache = object(), weakref.ref(self)

            def drop(_):
                # a collected tensor drops ITS entry only: one rebuilt since for live tensors under the same key carries another token
                c = cache()
                if c is not None and key in c.d and c.d[key][3] is token:
                    del c.d[key]
            ent = (tag, tuple(weakref.ref(r, drop) for r in refs), build(), token)
            self.d[key] = ent
        return ent[2]

    def clear(self):
        self.d.clear()


CACHE = WeightCache()          # the model files' cache (keys carry the owner's id()); the attention processors keep one per instance


def bf16(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.detach()
    return t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)


class Holder(nn.Module):
    """empty module: a namespace that gives its children the checkpoint's state-dict keys"""


def cat0(ts):
    return torch.cat([t.detach() for t in ts], dim=0).contiguous()


def lin_w(m) -> torch.Tensor:
    """nn.Linear or 1x1 Conv1d / Conv2d weight as [out, in]"""
    w = m.weight
    return w if w.dim() == 2 else CACHE.get(("w2", id(m)), w, lambda: w.detach().reshape(w.shape[0], w.shape[1]).contiguous())


def wb(m):
    """(weight [out, in], bias) of an nn.Linear or a 1x1 convolution, as bf16"""
    return bf16(lin_w(m)), bf16(m.bias)


def linear_resid(x: torch.Tensor, lin, resid: Optional[torch.Tensor] = None, acc_scale: float = 1.0) -> torch.Tensor:
    """`lin(x)`, or with `resid`: resid + acc_scale * lin(x) in the GEMM's epilogue.  `lin`: an nn.Linear or a (weight [out, in], bias) pair."""
    w, b = lin if isinstance(lin, tuple) else (lin.weight, lin.bias)
    if resid is None:
        return ops.linear(x, w, b)
    return ops.linear(x, w, b, epilogue=ops.EPI_RESID, resid=resid, acc_scale=acc_scale)


def host_scalar(fn, p: torch.Tensor) -> float:
    """`fn` (torch.tanh, torch.sigmoid) of a learnable scalar gate as a host float, read back ONCE per weight version: a `.item()` per
    call is a host sync per layer and cannot be captured in a HIP graph"""
    return CACHE.get(("scalar", fn, id(p)), p, lambda: float(fn(p.detach().float()).item()))


CONV_PRECISION_ATTR = "_mrag_conv_precision"
# a marked convolution takes the fp8 kernel from this many 256x256 output tiles on (the `t256 >= 192` of gemm_conv.hip: below it the bf16 path runs
# 128x128 tiles that fill the device, the fp8 kernel's one tile shape does not); tests of reduced models set it to 0
CONV_FP8_MIN_TILES = 192


def set_conv_precision(module: nn.Module, precision: str = "bf16") -> nn.Module:
    """precision of the 3x3 convolutions under `module` that run through `conv3x3` (the UNets' ResBlocks, the VAE decoders' ResnetBlocks):
    "bf16" (default, the reference precision) or "fp8" -- the e4m3 implicit GEMM (mrag_conv_fp8: per-pixel activation exponents, per-output-channel
    weight exponents, fp32 accumulation) wherever `ops.conv_fp8_supported` admits the call and it makes at least CONV_FP8_MIN_TILES
    output tiles of 256x256; stride-2, upsampling and temporal convolutions and those from or to 3, 4 or 8 channels stay bf16 through that gate.  Marks every nn.Conv2d with a 3x3 kernel; returns the module."""
    if precision not in ("bf16", "fp8"):
        raise ValueError(f"conv precision must be 'bf16' or 'fp8', got {precision!r}")
    for m in module.modules():
        if isinstance(m, nn.Conv2d) and tuple(m.kernel_size) == (3, 3):
            setattr(m, CONV_PRECISION_ATTR, precision)
    return module


def conv3x3(x: torch.Tensor, conv: nn.Conv2d, *, stride: int = 1, upsample: bool = False, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N, H, W, Cin] -> [N, Ho, Wo, Cout]: implicit GEMM over gathered rows; `resid` (same shape as the output) fused in the epilogue."""
    N, H, W, C = x.shape
    cout = conv.weight.shape[0]
    kp = ops._kpad(9 * C)

    def build():
        w = conv.weight.detach().permute(0, 2, 3, 1).reshape(cout, 9 * C)          # [Cout, Cin, ky, kx] -> [Cout, (ky, kx, cin)]
        if kp != 9 * C:
            w = torch.cat([w, torch.zeros(cout, kp - 9 * C, dtype=w.dtype, device=w.device)], dim=1)
        return w.contiguous()

    wk = CACHE.get(("c3", id(conv)), conv.weight, build)
    if (getattr(conv, CONV_PRECISION_ATTR, "bf16") == "fp8" and ops.conv_fp8_supported(N, H, W, C, cout, stride, upsample)
            and ((N * H * W + 255) // 256) * ((cout + 255) // 256) >= CONV_FP8_MIN_TILES):
        # opt-in e4m3 path (set_conv_precision): the weight quantised once per output channel, the activation per pixel in front of the launch
        w8, w_exp = CACHE.get(("c3f8", id(conv)), conv.weight, lambda: ops.quant_rows_e4m3(bf16(wk)))
        return ops.conv_implicit_fp8(x.contiguous(), w8, w_exp, conv.bias, resid=resid.contiguous() if resid is not None else None)
    if C % 64 == 0:                                                                 # implicit GEMM: the GEMM's DMA gathers the taps itself
        return ops.conv_implicit(x.contiguous(), wk, conv.bias, ops.CONV_3X3, stride=stride, upsample=upsample,
                                 resid=resid.contiguous() if resid is not None else None)
    rows = ops.im2col3x3(x, stride=stride, upsample=upsample)
    Hi, Wi = (2 * H, 2 * W) if upsample else (H, W)
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    return linear_resid(rows, (wk, conv.bias), None if resid is None else resid.reshape(-1, cout)).view(N, Ho, Wo, cout)


FF_SITES_ATTR = "_mrag_ff_fp8_sites"
FF_SITES = ("ff1", "ff2")
# The gates of a marked feed-forward, set from the measured table of tools/ff_fp8_measure.py: a site / shape that did not beat its bf16 launch there,
# or is smaller than anything measured, stays bf16.  Tests of reduced models set all three to 0.
# Both sites: calls of fewer rows stay bf16.  4 608 rows (DynamiCrafter-1024's middle block, C = 1280) is the smallest problem measured; FF1 wins there (1.33x).
FF_FP8_MIN_ROWS = 4608
# The output projection ("ff2") also needs this many rows -- 18 432 x 1280 wins (1.25x), 4 608 x 1280 (90 tiles of the kernel's one 256x256 shape) loses (0.97x) --
# and this many channels: the row quantiser in front of it (3 bytes per element of the 4 C wide GEGLU output) costs what the kernel saves at C = 640 (1.01x per
# GEMM, -0.25 ms on the SVD step: a tie) and more at C = 320, where the 256-wide tile also computes 512 columns for 320 (0.72x / 0.68x).
FF2_FP8_MIN_ROWS = 18432
FF2_FP8_MIN_WIDTH = 1280


def set_ff_precision(module: nn.Module, precision: str = "bf16", sites=FF_SITES) -> nn.Module:
    """precision of the feed-forward linears of the UNets' transformer blocks under `module` (every `FeedForward`):
    "bf16" (default, the reference precision) or "fp8" -- the e4m3 GEMM mrag_gemm_fp8_k64 (per-row activation exponents, per-output-channel weight
    exponents, fp32 accumulation) at the `sites` named: "ff1" the GEGLU projection, fed by a LayerNorm that writes e4m3 (ops.layernorm_e4m3), "ff2" the
    output projection with its residual, fed by a row quantiser.  Calls of fewer than FF_FP8_MIN_ROWS rows stay bf16, and so does "ff2" below
    FF2_FP8_MIN_ROWS rows or FF2_FP8_MIN_WIDTH channels: the shapes measured to lose, or smaller than any measured.  Returns the module."""
    if precision not in ("bf16", "fp8"):
        raise ValueError(f"feed-forward precision must be 'bf16' or 'fp8', got {precision!r}")
    sites = tuple(sites)
    if not sites or any(s not in FF_SITES for s in sites):
        raise ValueError(f"feed-forward sites are a non-empty subset of {FF_SITES}, got {sites!r}")
    for m in module.modules():
        if isinstance(m, FeedForward):
            setattr(m, FF_SITES_ATTR, tuple(s for s in FF_SITES if s in sites) if precision == "fp8" else ())
    return module


FF_FUSION_ATTR = "_mrag_ff_fused"
# A marked feed-forward takes the fused launch from this many rows on: the smallest row count at which it did not lose to the three launches in the table
# of tools/ff_fused_measure.py -- 258 048 (SVD's level 0) 1.09x, 294 912 (DynamiCrafter-1024's) 1.11x; 18 432 rows 0.94x, 4 608 rows 0.58x (a
# workgroup's 128 rows take ~95 us whatever the row count: below a few rounds of 256 workgroups the three launches win).  Tests of reduced models set it to 0.
FF_FUSED_MIN_ROWS = 258048


def set_ff_fusion(module: nn.Module, on: bool = True) -> nn.Module:
    """marks every `FeedForward` under `module`: a marked one runs LayerNorm, GEGLU projection, output projection and
    residual as ONE launch (ops.ff_fused, mrag_ff_fused_bf16: the normalised rows and the hidden tensor stay on chip) where `ops.ff_fused_supported` admits
    it -- 320 channels, the UNets' level 0 -- and the call has at least FF_FUSED_MIN_ROWS rows; everywhere else it runs as before.  bf16 with the rounding
    points of the three launches.  A module also marked by `set_ff_precision` takes the fused bf16 launch where it applies (C = 320, where FF2-fp8 is off
    by rule anyway) and its fp8 sites elsewhere.  `on=False` unmarks.  Returns the module."""
    if not isinstance(on, bool):
        raise ValueError(f"set_ff_fusion: on must be a bool, got {on!r}")
    for m in module.modules():
        if isinstance(m, FeedForward):
            setattr(m, FF_FUSION_ATTR, on)
    return module


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):
    """the UNets' gated feed-forward (lvdm attention.py:458-475 with glu=True; diffusers' FeedForward with activation_fn "geglu"): state-dict keys
    `net.0.proj.{weight,bias}`, `net.2.{weight,bias}`"""

    def __init__(self, dim, dim_out=None, mult=4, glu=True, dropout=0.0):
        super().__init__()
        if not glu:
            raise NotImplementedError("the UNets use gated feed-forwards")
        inner = int(dim * mult)
        self.net = nn.Sequential(GEGLU(dim, inner), nn.Dropout(dropout), nn.Linear(inner, dim if dim_out is None else dim_out))

    def forward(self, x, resid=None):
        return _geglu_ff(self, x, resid)


def _geglu_ff(ff: FeedForward, x: torch.Tensor, resid: Optional[torch.Tensor], norm: Optional[nn.LayerNorm] = None, ff1: bool = False, ff2: bool = False) -> torch.Tensor:
    """[resid +] out(GEGLU([norm](x))): value * gelu(gate) in the first GEMM's epilogue, the residual in the second's.  `ff1` / `ff2`: that GEMM on the e4m3
    kernel (FF1 fed by a LayerNorm that writes e4m3, FF2 by a row quantiser).  The bf16 form normalises before it looks the weights up, the fp8 forms after:
    the order their first call has always launched in."""
    pj, out = ff.net[0].proj, ff.net[2]
    ln = lambda f: x if norm is None else f(x, norm.weight, norm.bias, norm.eps)
    a = None if ff1 or ff2 else ln(ops.layernorm)
    w, b = CACHE.get(("geglu", id(pj)), (pj.weight, pj.bias), lambda: ops.geglu_interleave(pj.weight, pj.bias))
    if ff1:
        # the weights quantised once per output channel (FF1: the interleaved rows), the activation by the LayerNorm itself
        w8, w_exp = CACHE.get(("geglu8", id(pj)), (pj.weight, pj.bias), lambda: ops.quant_rows_e4m3(bf16(w)))
        h = ops.linear_fp8_k64(ln(ops.layernorm_e4m3), w8, w_exp, b, epilogue=ops.EPI_GEGLU).view(*x.shape[:-1], out.weight.shape[1])
    else:
        h = ops.linear(ln(ops.layernorm) if a is None else a, w, b, epilogue=ops.EPI_GEGLU)
    if ff2:
        w8, w_exp = CACHE.get(("ff2w8", id(out)), out.weight, lambda: ops.quant_rows_e4m3(bf16(out.weight)))
        return ops.linear_fp8_k64(h, w8, w_exp, out.bias, epilogue=ops.EPI_RESID, resid=resid)
    return linear_resid(h, out, resid)


def feed_forward(ff: FeedForward, norm: nn.LayerNorm, x: torch.Tensor) -> torch.Tensor:
    """x + ff(norm(x)) of a pre-norm transformer block.  Unmarked (the default): the LayerNorm launch and the two bf16 GEMMs; marked by `set_ff_fusion`: one
    fused launch at 320 channels; marked by `set_ff_precision`: the sites that are on run on the e4m3 GEMM.  Marked for both: the fused bf16 launch where it
    applies, the fp8 sites elsewhere."""
    pj, out = ff.net[0].proj, ff.net[2]
    sites = getattr(ff, FF_SITES_ATTR, ())
    C, inner = pj.weight.shape[1], out.weight.shape[1]
    rows = x.numel() // C
    if (getattr(ff, FF_FUSION_ATTR, False) and ops.ff_fused_supported(C, inner) and out.weight.shape[0] == C and rows >= FF_FUSED_MIN_ROWS
            and rows > 0 and pj.weight.shape[0] == 2 * inner):
        w, b = CACHE.get(("geglu", id(pj)), (pj.weight, pj.bias), lambda: ops.geglu_interleave(pj.weight, pj.bias))
        w2 = out.weight if out.weight.is_contiguous() else CACHE.get(("ff2c", id(out)), out.weight, lambda: out.weight.detach().contiguous())
        return ops.ff_fused(x, norm.weight, norm.bias, norm.eps, w, b, w2, out.bias)
    if sites and (rows < FF_FP8_MIN_ROWS or out.weight.shape[0] != C):
        sites = ()
    ff1 = "ff1" in sites and ops.fp8_linear_k64_supported(2 * inner, C, ops.EPI_GEGLU)
    ff2 = "ff2" in sites and rows >= FF2_FP8_MIN_ROWS and C >= FF2_FP8_MIN_WIDTH and ops.fp8_linear_k64_supported(C, inner, ops.EPI_RESID)
    return _geglu_ff(ff, x, x, norm, ff1, ff2)


def conv_t3(x: torch.Tensor, conv: nn.Conv3d, B: int, T: int, *, resid: Optional[torch.Tensor] = None, acc_scale: float = 1.0) -> torch.Tensor:
    """nn.Conv3d((3,1,1), padding (1,0,0)) on x [(b t), HW, C]; with `resid`: resid + acc_scale * conv(x)"""
    C = x.shape[-1]
    cout = conv.weight.shape[0]
    wk = CACHE.get(("t3", id(conv)), conv.weight, lambda: conv.weight.detach()[:, :, :, 0, 0].permute(0, 2, 1).reshape(cout, 3 * C).contiguous())
    if C % 64 == 0:
        return ops.conv_implicit(x.contiguous(), wk, conv.bias, ops.CONV_T3, frames=T, resid=resid.contiguous() if resid is not None else None, acc_scale=acc_scale)
    rows = ops.unfold_t3(x, B, T)
    return linear_resid(rows, (wk, conv.bias), None if resid is None else resid.reshape(-1, cout), acc_scale).view(x.shape[0], x.shape[1], cout)


def _conv_small_cin(z: torch.Tensor, conv: nn.Conv2d, tag: str) -> torch.Tensor:
    """3x3 convolution from 3 (RGB) or 4 (latent) channels: the row gather moves 16-byte (8-channel) granules, so the input and the kernel get zero channels"""
    N, H, W, cz = z.shape
    cp = (cz + 7) // 8 * 8
    if cp != cz:
        z = torch.nn.functional.pad(z, (0, cp - cz))
    kp = ops._kpad(9 * cp)

    def build():
        w = torch.nn.functional.pad(bf16(conv.weight), (0, 0, 0, 0, 0, cp - cz)).permute(0, 2, 3, 1).reshape(conv.weight.shape[0], 9 * cp)
        return torch.nn.functional.pad(w, (0, kp - 9 * cp)).contiguous()
    wk = CACHE.get((tag, id(conv), cp), conv.weight, build)
    return ops.linear(ops.im2col3x3(z.contiguous()), wk, bf16(conv.bias)).view(N, H, W, -1)


def groupnorm_rows(x: torch.Tensor, gn: nn.GroupNorm, *, silu: bool = False, frames_per_sample: int = 1, emb: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm [of x + emb] [+ SiLU] of channels-last x [N, H, W, C] or [N, HW, C], returned in x's shape.  Statistics per image, or per clip over (t, h, w)
    with `frames_per_sample` = t consecutive frames (the temporal blocks' 5-D GroupNorm: a row-count change)."""
    f = frames_per_sample
    return ops.groupnorm(x.view(x.shape[0] // f, -1, x.shape[-1]), bf16(gn.weight), bf16(gn.bias), gn.num_groups, gn.eps, silu=silu, emb=emb).view(x.shape)


class TembBank:
    """SiLU(emb) [N, E] together with EVERY residual block's projection of it.  Each ResBlock applies its own `Linear(emb_channels, C_out)` to the
    same SiLU(emb) (openaimodel3d.py:222; diffusers `time_emb_proj`): 25-44 GEMMs of 28-32 rows per step, each a 20 us launch on 3-10 workgroups.
    They do not depend on the activations, so the bank runs them as ONE GEMM against the row-concatenated weights at the start of the step and
    hands out column slices `[N, C_out]` (row stride = the concatenated width).  Same kernel (128 x 128 tiles), same K order per output
    element as the separate launches: identical bits."""

    def __init__(self, silu_emb: torch.Tensor, owner: nn.Module, linears):
        self.silu = silu_emb
        refs = tuple(t for lin in linears for t in (lin.weight, lin.bias))
        w, b, offs = CACHE.get(("tembbank", id(owner)), refs, lambda: (
            torch.cat([lin.weight.detach() for lin in linears], dim=0).contiguous(),
            torch.cat([(lin.bias.detach() if lin.bias is not None else torch.zeros(lin.out_features, dtype=lin.weight.dtype, device=lin.weight.device))
                       for lin in linears], dim=0).contiguous(),
            {id(lin): (o, lin.out_features) for lin, o in zip(linears, itertools.accumulate([0] + [lin.out_features for lin in linears[:-1]]))}))
        self._all = ops.linear(silu_emb, w, b) if linears else None
        self._offs = offs

    def proj(self, lin: nn.Linear) -> torch.Tensor:
        ent = self._offs.get(id(lin))
        if ent is None or ent[0] % 8:                      # a block outside the bank (or an unaligned slice): its own launch
            return ops.linear(self.silu, lin.weight, lin.bias)
        return self._all[:, ent[0]:ent[0] + ent[1]]


def temb_bank(model: nn.Module, silu_emb: torch.Tensor, pick) -> TembBank:
    """the step's TembBank over every time-embedding projection of `model`: `pick(module)` returns a residual block's nn.Linear, None for any other module
    (listed once per model)"""
    if getattr(model, "_temb_linears", None) is None:
        model._temb_linears = [lin for lin in map(pick, model.modules()) if lin is not None]
    return TembBank(silu_emb, model, model._temb_linears)


def temb_proj(silu_emb, lin: nn.Linear) -> torch.Tensor:
    """`lin(SiLU(emb))`: a slice of the step's TembBank, or the plain projection when a block is driven with a bare tensor (unit tests)"""
    return silu_emb.proj(lin) if isinstance(silu_emb, TembBank) else ops.linear(silu_emb, lin.weight, lin.bias)


def silu_mlp(lin1: nn.Linear, lin2: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """lin2(SiLU(lin1(x))): the timestep / frame-rate / added-condition embedding MLPs"""
    return ops.linear(ops.linear(x, lin1.weight, lin1.bias, epilogue=ops.EPI_SILU), lin2.weight, lin2.bias)


def resnet2d(x: torch.Tensor, norm1, conv1, norm2, conv2, shortcut=None, *, temb=None, temb_lin: Optional[nn.Linear] = None, conv=None) -> torch.Tensor:
    """the spatial residual block of both UNets and both VAEs on x [N, H, W, C]: GroupNorm + SiLU, 3x3 convolution, GroupNorm + SiLU [of h + temb_lin(temb)],
    3x3 convolution with the shortcut as its residual.  `shortcut`: None or nn.Identity, a 1x1 convolution (a GEMM) or a 3x3 one.  `temb`: the step's TembBank or
    a bare SiLU(emb) [N, E]; its projection is taken between the first convolution and the second norm, where a block driven with a bare tensor launches it.
    `conv`: the 3x3 convolution; a model file passes its own module-level `conv3x3`, the name tests and measuring tools replace to log or emulate its convolutions."""
    conv = conv or conv3x3
    h = conv(groupnorm_rows(x, norm1, silu=True), conv1)
    h = groupnorm_rows(h, norm2, silu=True, emb=None if temb_lin is None else temb_proj(temb, temb_lin))
    if shortcut is not None and not isinstance(shortcut, nn.Identity):
        x = ops.linear(x, *wb(shortcut)) if tuple(shortcut.kernel_size) == (1, 1) else conv(x, shortcut)
    return conv(h, conv2, resid=x)


def resnet_t3(x: torch.Tensor, norm1, conv1, norm2, conv2, b: int, frames: int, *, temb=None, temb_lin: Optional[nn.Linear] = None, acc_scale: float = 1.0) -> torch.Tensor:
    """the temporal residual block of the SVD UNet and VAE on x [(b f), HW, C]: x + acc_scale * branch(x) with GroupNorm statistics over (f, h, w) per sample and
    (3, 1, 1) convolutions; `temb_lin(temb)` [(b f), C] is added per frame in front of the second norm"""
    h = conv_t3(groupnorm_rows(x, norm1, silu=True, frames_per_sample=frames), conv1, b, frames)
    if temb_lin is not None:
        h = ops.add_bcast(h, temb_proj(temb, temb_lin), x.shape[1])
    h = groupnorm_rows(h, norm2, silu=True, frames_per_sample=frames)
    return conv_t3(h, conv2, b, frames, resid=x, acc_scale=acc_scale)


def self_attention(owner: nn.Module, x: torch.Tensor, heads: int, *, temporal: Optional[tuple] = None, fp8: bool = False) -> torch.Tensor:
    """head_dim-64 self-attention of x [Nb, L, C] through ONE GEMM against the owner's fused `to_q | to_k | to_v`; the result [Nb, L, heads * 64] goes to the
    owner's output projection.  `temporal=(b, t, hw)`: the rows are ordered (b, t, hw) and attention runs over t for every (b, hw), on permuted views of the
    projection (no copy).  `fp8`: long spatial sequences (ops.fp8_attention_supported) on the e4m3 MFMA path."""
    Nb, L, _ = x.shape
    w = CACHE.get(("qkv", id(owner)), (owner.to_q.weight, owner.to_k.weight, owner.to_v.weight), lambda: cat0([owner.to_q.weight, owner.to_k.weight, owner.to_v.weight]))
    qkv = ops.linear(x, w)
    if temporal is None:
        q5 = qkv.view(Nb, L, 3, heads, 64)
        return ops.attention(q5[:, :, 0], q5[:, :, 1], q5[:, :, 2], fp8=fp8 and ops.fp8_attention_supported(L, L))
    b, t, hw = temporal
    out = torch.empty(Nb, L, heads * 64, dtype=torch.bfloat16, device=x.device)
    q6, o4 = qkv.view(b, t, hw, 3, heads, 64), out.view(b, t, hw, heads * 64)
    for i in range(b):                                                      # batch = hw (stride one row), sequence = t
        ops.attention(q6[i, :, :, 0].permute(1, 0, 2, 3), q6[i, :, :, 1].permute(1, 0, 2, 3), q6[i, :, :, 2].permute(1, 0, 2, 3), out=o4[i].permute(1, 0, 2))
    return out


def kv_proj(owner: nn.Module, key: str, to_k: nn.Linear, to_v: nn.Linear, ctx: torch.Tensor, heads: int):
    """keys and values [B, L, heads, 64] of a cross-attention context through ONE GEMM against the fused `to_k | to_v` (cached under (key, id(owner)))"""
    w = CACHE.get((key, id(owner)), (to_k.weight, to_v.weight), lambda: cat0([to_k.weight, to_v.weight]))
    kv = ops.linear(ctx.contiguous(), w)
    return kv[..., : heads * 64].unflatten(-1, (heads, 64)), kv[..., heads * 64:].unflatten(-1, (heads, 64))


def attention_1head(x: torch.Tensor, norm: nn.GroupNorm, q, k, v, out) -> torch.Tensor:
    """the VAEs' attention block on x [N, H, W, C]: GroupNorm, ONE head over all pixels of a frame with head_dim = C (512), output projection with the residual.
    `q`, `k`, `v`, `out`: (weight [C, C], bias) pairs.  Per frame: S = q k^T as a GEMM, a row softmax, V^T [C, S] = Wv h^T by a GEMM with swapped operands (no
    transpose pass), O = P V as a GEMM whose bias is the value bias (rows of P sum to 1).  One [S, S] score buffer: 170 MB at 72 x 128."""
    N, H, W, C = x.shape
    S = H * W
    h = groupnorm_rows(x, norm).view(N, S, C)
    qs, ks = ops.linear(h, *q), ops.linear(h, *k)
    a = torch.empty(N, S, C, dtype=torch.bfloat16, device=x.device)
    scores = torch.empty(S, S, dtype=torch.bfloat16, device=x.device)
    for n in range(N):
        ops.linear(qs[n], ks[n], out=scores)
        ops.softmax_rows(scores, scale=float(C) ** -0.5, out=scores)
        ops.linear(scores, ops.linear(v[0], h[n]), v[1], out=a[n])
    return linear_resid(a, out, x.view(N, S, C)).view(N, H, W, C)


def prenorm_block(x: torch.Tensor, heads: int, ln1: nn.LayerNorm, qkv_w: torch.Tensor, qkv_b: Optional[torch.Tensor], out_proj: nn.Linear, ln2: nn.LayerNorm,
                  fc1: nn.Linear, fc2: nn.Linear, *, eps: float, head_dim: int = 64, mask: Optional[torch.Tensor] = None, ls1=None, ls2=None, attn_kernel: str = "fma") -> torch.Tensor:
    """pre-LayerNorm transformer block (VideoMAE, DINOv2, CLIP / open_clip towers): x + [ls1 *] out_proj(attn(ln1(x))), then x + [ls2 *] fc2(gelu(fc1(ln2(x))));
    every residual rides in a GEMM epilogue.  `qkv_w` / `qkv_b`: the fused [3D, D] projection (bf16); `mask`: the head_dim-64 kernel's byte mask;
    `ls1` / `ls2`: LayerScale modules (`lambda1` [D]), applied through the AdaLN-gate epilogue with a constant gate.  `attn_kernel` (head dims other than 64,
    clip_vision.set_attention_kernel): "fma" = ops.attention_small wherever it takes the shape, "mfma" = ops.attention_hd everywhere."""
    N, S, D = x.shape

    def resid_linear(a, lin, ls, x):
        if ls is None:
            return ops.linear(a, bf16(lin.weight), bf16(lin.bias), epilogue=ops.EPI_RESID, resid=x)
        g = bf16(ls.lambda1)
        return ops.linear(a, bf16(lin.weight), bf16(lin.bias), epilogue=ops.EPI_GATE_RESID, resid=x, gate0=g, gate1=g, rows_per_batch=N * S, split=0, gate_stride=0)
    h = ops.layernorm(x, bf16(ln1.weight), bf16(ln1.bias), eps)
    qkv = ops.linear(h, qkv_w, qkv_b).view(N, S, 3, heads, head_dim)
    if head_dim == 64:
        a = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask=mask)
    elif mask is None:
        # what attention_small refuses (K and V of a head beyond its LDS) runs on the MFMA kernel; what it takes stays on it unless the tower opted in
        hd = attn_kernel == "mfma" or S * head_dim > ops.ATTN_SMALL_MAX_KEY_ELEMS
        a = (ops.attention_hd if hd else ops.attention_small)(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    else:
        raise NotImplementedError("masked attention at head_dim 64 only")
    x = resid_linear(a, out_proj, ls1, x)
    h = ops.layernorm(x, bf16(ln2.weight), bf16(ln2.bias), eps)
    h = ops.linear(h, bf16(fc1.weight), bf16(fc1.bias), epilogue=ops.EPI_GELU_ERF)
    return resid_linear(h, fc2, ls2, x)
