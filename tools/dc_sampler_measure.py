"""The guidance-rescale DDIM update (ops.ddim_v_step_rescaled_: statistics + fold-and-update, two launches) beside the plain update it stands in for
(ops.ddim_v_step_: one launch), at DynamiCrafter-1024's latent [1, 4, 16, 72, 128] (589 824 elements per sample; v bf16 [2, ...], x and noise fp32).

One process, arms interleaved round by round, HIP events around a burst of `--calls` back-to-back calls of one arm (a call is microseconds of device work:
one call between two events would time the events), medians over `--reps` rounds of the per-call time.  No target is attached: both are microseconds beside
the UNet step they follow.

    python tools/dc_sampler_measure.py [--reps R] [--calls K] [--out FILE]      # prints one JSON object"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import ops
from motionrag_amd.dynamicrafter import DDIMSampler

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback and no CPU figure"
dev = "cuda"
torch.cuda.set_device(0)
shape = (1, 4, 16, 72, 128)
gen = torch.Generator(device=dev).manual_seed(7)
v = (torch.randn(2, *shape[1:], generator=gen, device=dev) * 1.5).to(torch.bfloat16)
x_plain, x_resc = (torch.randn(shape, generator=gen, device=dev) for _ in range(2))
noise = torch.randn(shape, generator=gen, device=dev)
smp = DDIMSampler()
smp.make_schedule(50, 1.0, "uniform_trailing")
coef = smp.step_coeffs(25)[1:]
arms = {"plain": lambda: ops.ddim_v_step_(v, x_plain, noise, 7.5, *coef),
        "rescaled": lambda: ops.ddim_v_step_rescaled_(v, x_resc, noise, 7.5, 0.7, *coef)}


def burst(fn):
    """device microseconds per call over `--calls` back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.calls


for fn in arms.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
t = {k: [] for k in arms}
for _ in range(args.reps):
    for k, fn in arms.items():
        t[k].append(burst(fn))
elems = x_plain.numel()
result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "reps": args.reps, "calls_per_burst": args.calls,
          "bytes_plain": elems * (2 * 2 + 3 * 4), "bytes_rescaled": elems * (2 * 2 + 2 * 2 + 3 * 4)}
for k, vals in t.items():
    result[k] = {"median_us": round(statistics.median(vals), 2), "min_us": round(min(vals), 2), "max_us": round(max(vals), 2)}
result["rescaled_minus_plain_us"] = round(result["rescaled"]["median_us"] - result["plain"]["median_us"], 2)
text = json.dumps(result, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
