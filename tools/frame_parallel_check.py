"""Worker of tests/test_gpu_frame_parallel_ranks.py: the frame-parallel (tier 2) DynamiCrafter UNet with W ranks on ONE GPU.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node=W tools/frame_parallel_check.py

Every rank opens cuda:0 and the ranks talk through gloo (dist.FrameParallel stages GPU tensors through the host on a gloo group), so the Python path is the
multi-GPU one except for the transport.  Each rank builds the reduced UNet of tests/golden/dc_unet.npz, runs the forward unsharded and sharded (twice), and
checks: shape, finiteness, the same bits on every rank and from run to run, the golden bound of tests/test_gpu_unet.py (rel_l2 3e-2), and that sharding moves
the result by no more than the bf16 model's own distance from the fp32 golden output.  Rank 0 prints ONE JSON line (with the sha1 of its sharded and unsharded output bytes, to compare two trees); the first failure ends the process with a
non-zero status before anything else is launched.  Says nothing about multi-GPU step time (unmeasured on hardware)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN_BOUND = 3e-2


def build_unet(dev):
    from motionrag_amd import dynamicrafter as dc
    from oracle.seeded import seeded_sd
    g = np.load(os.path.join(ROOT, "tests", "golden", "dc_unet.npz"))
    shapes = [s[:n].tolist() for s, n in zip(g["shapes"], g["ndims"])]
    sd = seeded_sd([str(k) for k in g["keys"]], shapes, int(g["seed"]), float(g["std"]))
    gi = torch.Generator().manual_seed(int(g["input_seed"]))
    x = torch.randn(2, 8, 4, 8, 8, generator=gi)
    ctx = {"image": torch.randn(2, 12, 64, generator=gi), "prompt": torch.randn(2, 7, 64, generator=gi), "action": torch.randn(2, 25, 64, generator=gi)}
    unet = dc.UNetModel(in_channels=8, out_channels=4, model_channels=64, attention_resolutions=(1, 2), num_res_blocks=1, channel_mult=(1, 2),
                        num_head_channels=64, transformer_depth=1, context_dim=64, use_linear=True, temporal_conv=True, temporal_attention=True,
                        temporal_self_att_only=True, use_relative_position=False, temporal_length=4, addition_attention=True,
                        image_cross_attention=True, action_cross_attention=True, default_fs=10, fs_condition=True)
    unet.load_state_dict(sd, strict=True)
    unet = unet.to(dev, torch.bfloat16)
    args = (x.to(dev), torch.from_numpy(g["timesteps"]).to(dev))
    kw = dict(context={k: v.to(dev) for k, v in ctx.items()}, fs=torch.from_numpy(g["fs"]).to(dev))
    return unet, args, kw, torch.from_numpy(g["y"])


def rel_fro(got, want):
    g, w = got.float().cpu(), want.float().cpu()
    return ((g - w).norm() / w.norm()).item()


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from motionrag_amd import dynamicrafter as dc, ops
        from motionrag_amd.dist import FrameParallel
        torch.cuda.set_device(0)
        unet, args, kw, golden = build_unet("cuda:0")

        def fail(why):
            print(f"rank {rank}: {why}", file=sys.stderr, flush=True)
            sys.exit(1)

        plain = unet(*args, **kw).clone()
        dc.set_frame_parallel(unet, FrameParallel(rank, world))
        with ops.dispatched() as d:
            first = unet(*args, **kw).clone()
        second = unet(*args, **kw)
        torch.cuda.synchronize()
        if tuple(first.shape) != (2, 4, 4, 8, 8):
            fail(f"output shape {tuple(first.shape)}")
        if not torch.isfinite(first.float()).all():
            fail("non-finite output")
        if not torch.equal(first, second):
            fail("two sharded forwards in a row differ")
        e_golden, e_plain, e_shard = rel_fro(first, golden), rel_fro(plain, golden), rel_fro(first, plain)
        if not e_golden <= GOLDEN_BOUND:
            fail(f"sharded against the golden output: {e_golden:.4e} > {GOLDEN_BOUND}")
        if not e_shard <= e_plain:
            fail(f"sharded against unsharded {e_shard:.4e} > unsharded against golden {e_plain:.4e}")
        mine = first.cpu().contiguous().view(torch.uint8)                 # bytes: a type every gloo build carries
        everyone = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(everyone, mine)
        same = all(torch.equal(e, mine) for e in everyone)
        if not same:
            fail("the ranks' outputs differ in bits")
        if rank == 0:
            sha1 = lambda t: hashlib.sha1(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
            print(json.dumps({"world": world, "sha1_sharded": sha1(first), "sha1_unsharded": sha1(plain), "shape": list(first.shape), "finite": True, "same_bits_on_all_ranks": same, "repeatable": True,
                              "rel_fro_sharded_vs_golden": e_golden, "rel_fro_unsharded_vs_golden": e_plain, "rel_fro_sharded_vs_unsharded": e_shard,
                              "golden_bound": GOLDEN_BOUND, "launches": {k: v for k, v in d.counts.items() if k.startswith("GN_")}}), flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
