"""Single-process GPU tests of the frame-parallel (tier 2) UNet's kernels: the GroupNorm split at its statistics (mrag_groupnorm_partial_bf16 +
mrag_groupnorm_apply_stats_bf16), the outer-axis swap copy (mrag_swap_outer_bf16), and that a model with sharding off -- never set, set to None, or a
FrameParallel of world 1 -- runs today's launches and writes today's bits.

Bounds.  One shard (W = 1): the pair is the unsplit kernel's arithmetic with an identity fold in the middle -> the same BITS.  Several shards: the
reference is a float64 GroupNorm of the same bf16 input on the host; E = the unsplit kernel's own maximum error against it, measured here on the same
input, and the sharded result must stay within 2 E (a reordered fp32 sum of the same terms has no reason to be worse; the factor 2 allows one extra bf16
rounding flip at the output).  Both errors are printed (DESIGN.md section 6 quotes them)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 4 * 64, 64), (2, 16 * 576, 320), (1, 7 * 9, 1280)]            # level-like, the level-0 width over 16 frames of 576 pixels, an odd pixel count


@functools.lru_cache(maxsize=None)
def _input(N, HW, C, offset):
    """(x, gamma, beta) bf16 on the host, seeded; `offset`: a common offset of 30 standard deviations (sum-of-squares statistics lose digits there)"""
    g = torch.Generator().manual_seed(N * 1000003 + HW * 101 + C + (7 if offset else 0))
    x = torch.randn(N, HW, C, generator=g) * (1.0 + torch.rand(1, 1, C, generator=g)) + (30.0 if offset else 0.0)
    return x.to(torch.bfloat16), (1.0 + 0.3 * torch.randn(C, generator=g)).to(torch.bfloat16), (0.3 * torch.randn(C, generator=g)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _reference(N, HW, C, offset, silu):
    """float64 GroupNorm(32, eps 1e-5) [+ SiLU] of the bf16 input, on the host (computed once per input, shared, never modified)"""
    x, ga, be = _input(N, HW, C, offset)
    xd = x.double().view(N, HW, 32, C // 32)
    mean = xd.mean(dim=(1, 3), keepdim=True)
    var = xd.var(dim=(1, 3), unbiased=False, keepdim=True)
    y = ((xd - mean) / torch.sqrt(var + 1e-5)).view(N, HW, C) * ga.double() + be.double()
    return y * torch.sigmoid(y) if silu else y


def _max_err(got, want):
    return (got.double().cpu() - want).abs().max().item()


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("N,HW,C", SHAPES)
def test_one_shard_writes_the_bits_of_the_unsplit_groupnorm(hip, N, HW, C, silu):
    from motionrag_amd import ops
    x, ga, be = (t.to(DEV) for t in _input(N, HW, C, False))
    want = ops.groupnorm(x, ga, be, 32, 1e-5, silu=silu)
    with ops.dispatched() as d:
        part = ops.groupnorm_partial(x, 32)
        got = ops.groupnorm_apply_stats(x, part.unsqueeze(0).contiguous(), HW, ga, be, 32, 1e-5, silu=silu)
    assert part.shape == (N, 32, 2) and part.dtype == torch.float32
    assert torch.equal(got, want)
    assert d.counts == {"GN_STATS": 1, "GN_FOLD": 2, "GN_APPLY": 1}, d.counts
    # the partial is the shard's (sum, sum of squares): against float64 sums of the same input, fp32 accumulation of HW * C / 32 terms
    xd = x.double().cpu().view(N, HW, 32, C // 32)
    ref = torch.stack([xd.sum(dim=(1, 3)), (xd * xd).sum(dim=(1, 3))], dim=-1)
    assert torch.allclose(part.double().cpu(), ref, rtol=1e-4, atol=1e-4 * float(xd.abs().sum(dim=(1, 3)).max()))


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("N,HW,C,offset", [s + (False,) for s in SHAPES] + [(2, 16 * 576, 320, True)])
def test_shards_stay_within_twice_the_unsplit_kernels_error(hip, N, HW, C, offset, W):
    from motionrag_amd import ops
    x, ga, be = (t.to(DEV) for t in _input(N, HW, C, offset))
    shards = [s.contiguous() for s in torch.tensor_split(x, W, dim=1)]                    # contiguous shards along HW (unequal when W does not divide HW)
    partials = torch.stack([ops.groupnorm_partial(s, 32) for s in shards])                # [W, N, 32, 2]: what the all-gather returns
    for silu in (False, True):
        want = _reference(N, HW, C, offset, silu)
        e_unsplit = _max_err(ops.groupnorm(x, ga, be, 32, 1e-5, silu=silu), want)
        got = torch.cat([ops.groupnorm_apply_stats(s, partials, HW, ga, be, 32, 1e-5, silu=silu) for s in shards], dim=1)
        e_shards = _max_err(got, want)
        print(f"groupnorm N={N} HW={HW} C={C} offset={int(offset)} silu={int(silu)} W={W}: max |err| against float64: unsplit {e_unsplit:.4e}, "
              f"sharded {e_shards:.4e} (bound {2 * e_unsplit:.4e})")
        assert torch.isfinite(got.float()).all() and e_shards <= 2 * e_unsplit


def test_split_groupnorm_refuses_emb_mod_and_fold(hip):
    from motionrag_amd import _lib, ops
    L = _lib.lib()
    x, ga, be = (t.to(DEV) for t in _input(2, 256, 64, False))
    y = torch.empty_like(x)
    part = torch.zeros(1, 2, 32, 2, dtype=torch.float32, device=DEV)
    other = torch.zeros(2, 64, dtype=torch.bfloat16, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = ops.dispatch_counts()
    for field in ("emb", "mod", "fold"):
        a = ops._gn_split_args(x, 32)
        a.y, a.gamma, a.beta, a.eps = y.data_ptr(), ga.data_ptr(), be.data_ptr(), 1e-5
        if field == "fold":
            a.fold = 1
        else:
            setattr(a, field, other.data_ptr())
            a.emb_stride = 64
        assert L.mrag_groupnorm_partial_bf16(st, ctypes.byref(a), ctypes.c_void_p(part.data_ptr())) == _lib.MRAG_ENOTSUP, field
        assert L.mrag_groupnorm_apply_stats_bf16(st, ctypes.byref(a), ctypes.c_void_p(part.data_ptr()), 1, 256) == _lib.MRAG_ENOTSUP, field
    assert ops.dispatch_counts() == before                                                 # no launch is counted


@pytest.mark.parametrize("A,B,R", [(4, 2, 8), (8, 4, 32 * 64), (3, 8, 1152 * 320), (3, 5, 8 * 1031)])
def test_swap_outer_is_a_permute_copy(hip, A, B, R):
    """(3, 8, 1152 * 320): a pixel slab of level 0 at 8 ranks; R = 8 * 1031: 1031 vectors per row = one whole run of 1024 and a 7-vector tail behind it"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(A * 100 + B)
    x = torch.randn(A, B, R, generator=g).to(torch.bfloat16).to(DEV)
    got = ops.swap_outer(x)
    assert got.shape == (B, A, R) and got.is_contiguous()
    assert torch.equal(got, x.permute(1, 0, 2).contiguous())
    assert torch.equal(ops.swap_outer(got), x)


def test_sharding_off_or_world1_changes_nothing(hip, golden_dir):
    """never set, set to None, and a FrameParallel of one rank: the same bits and the same launch counts"""
    from motionrag_amd import dynamicrafter as dc, ops
    from motionrag_amd.dist import FrameParallel
    from test_gpu_conv_fp8 import _dc_unet
    unet, args, kw = _dc_unet(golden_dir)
    never = unet(*args, **kw).clone()                                                       # (also warms every cache the forwards below share)
    with ops.dispatched() as d0:
        again = unet(*args, **kw)
    assert torch.equal(again, never)
    for fp in (None, FrameParallel(0, 1)):
        dc.set_frame_parallel(unet, fp)
        with ops.dispatched() as d:
            got = unet(*args, **kw)
        assert torch.equal(got, never) and d.counts == d0.counts, (fp, d.counts, d0.counts)
