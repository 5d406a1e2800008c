"""The opt-in fused feed-forward kernel of the UNets' 320-channel blocks against the three launches it replaces.

(a) per feed-forward -- x [rows, 320], inner = 1280, gaussian operands, LayerNorm affine and both biases:
      arm A  the three launches of layers.feed_forward today: ops.layernorm, ops.linear (EPI_GEGLU), ops.linear (EPI_RESID)
      arm B  ops.ff_fused (mrag_ff_fused_bf16)
    at 294 912 rows (DynamiCrafter-1024 level 0, spatial and temporal), 258 048 (SVD level 0) and 18 432 / 4 608 rows, which place layers.FF_FUSED_MIN_ROWS.
    TFLOP/s = 2 rows (2 inner C + C inner) over the time.
(b) whole steps -- the DynamiCrafter-1024 CFG UNet step and the SVD CFG step (workloads.py) with layers.set_ff_fusion off and on; the relative
    Frobenius distance of the switch-on output from the switch-off output beside the times.

One process, the arms interleaved round by round, HIP events around each call group, medians and minima after warm-up.  Every comparison is against
the launches the site runs today, never against the fused code itself.

    python tools/ff_fused_measure.py [--reps R] [--step-reps R] [--no-ffs] [--no-steps] [--out FILE]      # prints one JSON object"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import layers, ops, workloads

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--step-reps", type=int, default=5)
ap.add_argument("--no-ffs", action="store_true")
ap.add_argument("--no-steps", action="store_true")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback and no CPU figure"
dev = "cuda"
torch.cuda.set_device(0)
gen = torch.Generator(device=dev).manual_seed(7)
rnd = lambda *shape, std=1.0: (torch.randn(*shape, generator=gen, device=dev) * std).to(torch.bfloat16)


def timed(fn, inner):
    """device milliseconds per call of fn (HIP events around `inner` back-to-back calls)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def interleaved(arms, reps, warm=2, inner=2):
    for fn in arms.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn, inner))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for k, v in t.items()}


def rel(a, b):
    a, b = a.float(), b.float()
    return round(((a - b).norm() / b.norm()).item(), 5)


C, INNER = 320, 1280
result = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "FF_FUSED_MIN_ROWS_shipped": layers.FF_FUSED_MIN_ROWS, "feed_forwards": {}}
SHAPES = (("dc_level0", 2 * 16 * 72 * 128), ("svd_level0", 28 * 72 * 128), ("rows_18432", 18432), ("rows_4608", 4608))
for name, M in (() if args.no_ffs else SHAPES):
    x, gamma, beta = rnd(M, C), rnd(C, std=0.1) + 1.0, rnd(C, std=0.1)
    w1, b1 = ops.geglu_interleave(rnd(2 * INNER, C, std=C ** -0.5), rnd(2 * INNER, std=0.02))
    w2, b2 = rnd(C, INNER, std=INNER ** -0.5), rnd(C, std=0.02)
    xn, h = torch.empty_like(x), torch.empty(M, INNER, dtype=torch.bfloat16, device=dev)
    o, o_fused = torch.empty_like(x), torch.empty_like(x)

    def three_launches():
        ops.layernorm(x, gamma, beta, 1e-5, out=xn)
        ops.linear(xn, w1, b1, epilogue=ops.EPI_GEGLU, out=h)
        return ops.linear(h, w2, b2, epilogue=ops.EPI_RESID, resid=x, out=o)
    arms = {"three_launches": three_launches,
            "ln": lambda: ops.layernorm(x, gamma, beta, 1e-5, out=xn),
            "ff1": lambda: ops.linear(xn, w1, b1, epilogue=ops.EPI_GEGLU, out=h),
            "ff2": lambda: ops.linear(h, w2, b2, epilogue=ops.EPI_RESID, resid=x, out=o),
            "fused": lambda: ops.ff_fused(x, gamma, beta, 1e-5, w1, b1, w2, b2, out=o_fused)}
    with ops.dispatched() as d:
        three_launches()
    before = ops.ff_fused_launches()
    r = interleaved(arms, args.reps)
    assert ops.ff_fused_launches() > before
    flop = 2.0 * M * (2 * INNER * C + C * INNER)
    r["three_launches_tflops"] = round(flop / r["three_launches"]["median_ms"] * 1e-9, 1)
    r["fused_tflops"] = round(flop / r["fused"]["median_ms"] * 1e-9, 1)
    r["speedup_fused_vs_three_launches"] = round(r["three_launches"]["median_ms"] / r["fused"]["median_ms"], 3)
    r["rel_fro_vs_three_launches"] = rel(o_fused, o)
    r["shape"] = {"rows": M, "C": C, "inner": INNER, "gflop": round(flop * 1e-9, 1), "kernels_today": d.counts}
    result["feed_forwards"][name] = r
    print(f"# {name}: {json.dumps(r)}", file=sys.stderr, flush=True)
    del x, xn, h, o, o_fused, arms
    torch.cuda.empty_cache()


def measure_step(name, model, run):
    """`run()` with the switch off and on: set outside the timed window, round by round"""
    t, outs, launches = {"off": [], "on": []}, {}, {}
    with torch.no_grad():
        for rep in range(2 + args.step_reps):                                   # two warm rounds
            for arm in ("off", "on"):
                layers.set_ff_fusion(model, arm == "on")
                before = ops.ff_fused_launches()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = run()
                e1.record()
                e1.synchronize()
                launches[arm] = ops.ff_fused_launches() - before
                if rep == 1:
                    outs[arm] = out.clone()
                if rep >= 2:
                    t[arm].append(e0.elapsed_time(e1))
    layers.set_ff_fusion(model, False)
    r = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for k, v in t.items()}
    assert launches["off"] == 0
    r["on"]["fused_launches_per_call"] = launches["on"]
    r["on"]["rel_fro_vs_off"] = rel(outs["on"], outs["off"])
    r["on"]["saved_ms"] = round(r["off"]["median_ms"] - r["on"]["median_ms"], 3)
    r["on"]["speedup_vs_off"] = round(r["off"]["median_ms"] / r["on"]["median_ms"], 4)
    result.setdefault("steps", {})[name] = r
    print(f"# {name}: {json.dumps(r)}", file=sys.stderr, flush=True)


if not args.no_steps:
    result["step_reps"] = args.step_reps
    unet = workloads.dynamicrafter1024_unet(dev)
    x, ts, ctx, fs = workloads.dynamicrafter1024_inputs(dev)
    measure_step("dc1024_cfg_step", unet, lambda: unet(x, ts, context=ctx, fs=fs))
    del unet, x, ts, ctx, fs
    torch.cuda.empty_cache()

    net, _ = workloads.svd_unet(dev)
    step, lat, reset = workloads.svd_step(net, dev)

    def svd_run():
        reset()
        return step()
    measure_step("svd_cfg_step", net, svd_run)

text = json.dumps(result, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
