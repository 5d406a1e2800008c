"""developer tool: the two kernels the frame-parallel (tier 2) DynamiCrafter UNet adds, on ONE GPU, arms interleaved in one process, medians over rounds.

  * the GroupNorm pair (ops.groupnorm_partial + ops.groupnorm_apply_stats, W = 8 gathered partials) against mrag_groupnorm_bf16 (ops.groupnorm) at the
    temporal level-0 shard shape of DynamiCrafter-1024 over 8 ranks: N = 2, HW = 16 * 9216 / 8, C = 320 (SiLU on, as in TemporalConvBlock)
  * the swap copy (ops.swap_outer) against torch's permute copy at [4, 8, 1152 * 320] (a rank's to_pixels send buffer: b * t_loc = 4, 8 peers)

    python tools/frame_parallel_measure.py [--rounds 9] [--iters 200] [--out profiles/frame_parallel.txt]

Kernel time on one GPU only: the collectives between the pair's halves and the multi-GPU step time are NOT measured here (unmeasured on hardware)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import microbench as mb  # noqa: E402
from motionrag_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- GroupNorm: unsplit (3 launches) against partial + apply_stats (2 + 2 launches)
    N, HW, C, W = 2, 16 * 9216 // 8, 320, 8
    x = torch.randn(N, HW, C, generator=g).to(torch.bfloat16).to(dev)
    ga, be = (torch.randn(C, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    y = torch.empty_like(x)
    part = torch.empty(N, 32, 2, dtype=torch.float32, device=dev)
    partials = ops.groupnorm_partial(x, 32).unsqueeze(0).repeat(W, 1, 1, 1).contiguous()
    arms = {"groupnorm (unsplit)": lambda: ops.groupnorm(x, ga, be, 32, 1e-5, silu=True, out=y),
            "partial + apply_stats": lambda: (ops.groupnorm_partial(x, 32, out=part), ops.groupnorm_apply_stats(x, partials, W * HW, ga, be, 32, 1e-5, silu=True, out=y)),
            "partial only": lambda: ops.groupnorm_partial(x, 32, out=part),
            "apply_stats only": lambda: ops.groupnorm_apply_stats(x, partials, W * HW, ga, be, 32, 1e-5, silu=True, out=y)}
    t = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            t[k].append(mb.timeit(fn, iters=a.iters, warm=10) * 1e6)
    nbytes = x.numel() * 2
    say(f"GroupNorm(32)+SiLU, N={N} HW={HW} C={C} bf16 ({nbytes / 1e6:.1f} MB; 2 reads + 1 write per call), W={W} partials; {a.rounds} interleaved rounds x {a.iters} calls")
    for k in arms:
        med = statistics.median(t[k])
        say(f"  {k:24s} median {med:8.2f} us   min {min(t[k]):8.2f}   max {max(t[k]):8.2f}")
    say(f"  pair / unsplit = {statistics.median(t['partial + apply_stats']) / statistics.median(t['groupnorm (unsplit)']):.3f}")

    # ---- swap copy against torch's permute copy
    A, B, R = 4, 8, 1152 * 320
    s = torch.randn(A, B, R, generator=g).to(torch.bfloat16).to(dev)
    d = torch.empty(B, A, R, dtype=torch.bfloat16, device=dev)
    assert torch.equal(ops.swap_outer(s), s.permute(1, 0, 2).contiguous())
    arms = {"ops.swap_outer": lambda: ops.swap_outer(s, out=d), "torch permute copy": lambda: d.copy_(s.permute(1, 0, 2))}
    t = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            t[k].append(mb.timeit(fn, iters=a.iters, warm=10) * 1e6)
    nbytes = s.numel() * 2
    say(f"outer-axis swap [{A}, {B}, {R}] bf16 ({nbytes / 1e6:.1f} MB read + as much written); {a.rounds} interleaved rounds x {a.iters} calls")
    for k in arms:
        med = statistics.median(t[k])
        say(f"  {k:24s} median {med:8.2f} us   min {min(t[k]):8.2f}   max {max(t[k]):8.2f}   {2 * nbytes / med / 1e6:6.2f} TB/s (read + write)")
    say(f"  swap / torch = {statistics.median(t['ops.swap_outer']) / statistics.median(t['torch permute copy']):.3f}")
    say("multi-GPU step time of the frame-parallel UNet: unmeasured on hardware (one GPU per run here)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
