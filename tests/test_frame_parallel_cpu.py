"""CPU suite of the frame-parallel (tier 2) DynamiCrafter UNet: the C ABI of the split GroupNorm and the swap copy is bound as declared, `FrameParallel`'s
geometry, and its three exchanges over a four-rank gloo group on CPU tensors."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mrag_groupnorm_split_workspace_bytes", "mrag_groupnorm_partial_bf16", "mrag_groupnorm_apply_stats_bf16", "mrag_swap_outer_bf16")


def test_new_prototypes_are_bound_with_matching_argument_counts():
    from motionrag_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/mrag_hip.h"
        n_args = len([a for a in m.group(2).split(",") if a.strip()])
        assert name in _lib.SYMBOLS and hasattr(L, name)
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, (name, n_args, fn.argtypes)
        assert fn.restype is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int32), name
    # the split form's workspace holds what the unsplit form's does (chunk partials + per-(n, c) scale / shift behind the 16 KiB in front)
    assert L.mrag_groupnorm_split_workspace_bytes(2, 320, 1024) >= 16384 + (2 * 1024 * 320 * 2 + 2 * 320 * 2) * 4
    assert _lib.ABI_VERSION == 11                                             # additive: the ABI number stays


def test_frame_ranges_and_refusals():
    from motionrag_amd.dist import FrameParallel
    for world in (1, 2, 4, 8):
        got = [i for r in range(world) for i in FrameParallel(r, world).frames(16)]
        assert got == list(range(16))
        assert len({len(FrameParallel(r, world).frames(16)) for r in range(world)}) == 1
    with pytest.raises(ValueError):
        FrameParallel(0, 4).frames(14)                                         # SVD's 14 frames: the padding design, not this one
    with pytest.raises(ValueError):
        FrameParallel(0, 4).check(14, [64])
    with pytest.raises(ValueError):
        FrameParallel(0, 32).check(32, [9216, 2304, 576, 144])                 # 144 pixels at the lowest level do not split over 32 ranks
    with pytest.raises(ValueError):
        FrameParallel(0, 32).to_pixels(torch.zeros(1, 1, 144, 8))
    FrameParallel(3, 8).check(16, [9216, 2304, 576, 144])                      # DynamiCrafter-1024 over one node
    with pytest.raises(ValueError):
        FrameParallel(4, 4)


def test_world1_is_the_identity():
    from motionrag_amd.dist import FrameParallel
    fp = FrameParallel(0, 1)
    x = torch.randn(2, 4, 6, 8)
    p = torch.randn(2, 32, 2)
    assert fp.to_pixels(x) is x and fp.to_frames(x) is x and fp.gather_stats(p) is p and fp.gather_frames(x) is x


def _worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    from motionrag_amd.dist import FrameParallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        fp = FrameParallel(rank, world)
        ok = {}
        for tl in (1, 2):
            b, t, hw, c = 2, tl * world, 8, 8
            full = torch.arange(b * t * hw * c, dtype=torch.float32).view(b, t, hw, c)          # every element names its (b, frame, pixel, channel)
            fr = fp.frames(t)
            mine = full[:, fr.start:fr.stop].contiguous()
            px = fp.to_pixels(mine)
            hwl = hw // world
            ok[f"pixels{tl}"] = tuple(px.shape) == (b, t, hwl, c) and torch.equal(px, full[:, :, rank * hwl:(rank + 1) * hwl])
            # rank-major receive order == frame order: the frame index read off the elements of each received frame
            ok[f"order{tl}"] = ((px // (hw * c)) % t)[1, :, 0, 0].tolist() == [float(f) for f in range(t)]
            ok[f"round{tl}"] = torch.equal(fp.to_frames(px), mine)
            ok[f"frames{tl}"] = torch.equal(fp.gather_frames(mine), full)
        part = torch.full((2, 32, 2), float(rank)) + torch.arange(2 * 32 * 2, dtype=torch.float32).view(2, 32, 2) / 1024
        g = fp.gather_stats(part)
        ok["stats"] = tuple(g.shape) == (world, 2, 32, 2) and g.dtype == torch.float32 and \
            all(torch.equal(g[r], part - float(rank) + float(r)) for r in range(world))
        ret[rank] = ok
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_transposes_and_gathers_world4_gloo():
    """four ranks: to_pixels hands every rank ALL frames of its pixel slab in frame order (t_loc = 1 and 2), to_frames restores the frame shard exactly,
    gather_frames rebuilds the clip, and gather_stats returns the ranks' partials in rank order on every rank"""
    world, port = 4, 39500 + os.getpid() % 2000
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    want = {f"{k}{tl}": True for k in ("pixels", "order", "round", "frames") for tl in (1, 2)}
    want["stats"] = True
    for r in range(world):
        assert ret[r] == want, (r, ret[r])
