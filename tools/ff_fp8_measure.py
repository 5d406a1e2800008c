"""The opt-in fp8 (e4m3) feed-forward linears of the UNets against the bf16 launches they would replace.

(a) per GEMM -- the FeedForward of DynamiCrafter-1024's three transformer levels at the 32 frames of the CFG pair (rows 2 x 16 x 72 x 128 = 294 912,
    73 728 and 18 432; C = 320 / 640 / 1280), of its middle block (4 608 rows, C = 1280) and of SVD's level 0 (28 x 72 x 128 = 258 048 rows, C = 320), gaussian operands:
      FF1 (GEGLU projection, N = 8 C, K = C):  the bf16 launch (ops.linear, EPI_GEGLU), the fp8 kernel alone (mrag_gemm_fp8_k64 on rows quantised
          beforehand), the LayerNorm in front as it runs today (ops.layernorm) and as ops.layernorm_e4m3, and the two sites whole: LayerNorm + GEMM.
      FF2 (output projection + residual, N = C, K = 4 C):  the bf16 launch (EPI_RESID), the fp8 kernel alone, the row quantiser in front of it, and
          the two as ops.linear_fp8_k64 issues them.
    TFLOP/s = 2 M N K over the time.
(b) whole steps -- the DynamiCrafter-1024 CFG UNet step and the SVD CFG step (workloads.py) with layers.set_ff_precision off, each site alone, both,
    and both beside layers.set_conv_precision; the relative Frobenius distance of each output from the switch-off output beside the times.
    --open-gates sets layers.FF_FP8_MIN_ROWS, FF2_FP8_MIN_ROWS and FF2_FP8_MIN_WIDTH to 0 for the steps (every marked site on fp8); default: the shipped gates.

One process, the arms interleaved round by round, HIP events around each call group, medians and minima after warm-up.  Every comparison is against
the bf16 launches the site runs today, never against the fp8 code itself.

    python tools/ff_fp8_measure.py [--reps R] [--step-reps R] [--no-gemms] [--no-steps] [--open-gates] [--out FILE]      # prints one JSON object"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import layers, ops, workloads

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--step-reps", type=int, default=5)
ap.add_argument("--no-gemms", action="store_true")
ap.add_argument("--no-steps", action="store_true")
ap.add_argument("--open-gates", action="store_true")
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


def gates():
    return {k: getattr(layers, k) for k in ("FF_FP8_MIN_ROWS", "FF2_FP8_MIN_ROWS", "FF2_FP8_MIN_WIDTH")}


def rel(a, b):
    a, b = a.float(), b.float()
    return round(((a - b).norm() / b.norm()).item(), 5)


def ratios(r, flop, bf16, kernel, path):
    med = lambda k: r[k]["median_ms"]
    r["bf16_tflops"] = round(flop / med(bf16) * 1e-9, 1)
    r["fp8_kernel_tflops"] = round(flop / med(kernel) * 1e-9, 1)
    r["speedup_kernel_vs_bf16"] = round(med(bf16) / med(kernel), 3)
    r["speedup_total_vs_bf16"] = round(path[0] / path[1], 3)


result = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "gates_shipped": gates(), "gemms": {}}
LEVELS = (("dc_level0", 2 * 16 * 72 * 128, 320), ("dc_level1", 2 * 16 * 72 * 128 // 4, 640), ("dc_level2", 2 * 16 * 72 * 128 // 16, 1280),
          ("dc_middle", 2 * 16 * 72 * 128 // 64, 1280),
          ("svd_level0", 28 * 72 * 128, 320))
for name, M, C in (() if args.no_gemms else LEVELS):
    inner = 4 * C
    x, gamma, beta = rnd(M, C), rnd(C, std=0.1) + 1.0, rnd(C, std=0.1)
    w1, b1 = ops.geglu_interleave(rnd(2 * inner, C, std=C ** -0.5), rnd(2 * inner, std=0.02))
    w2, b2 = rnd(C, inner, std=inner ** -0.5), rnd(C, std=0.02)
    w1_8, w1_e = ops.quant_rows_e4m3(w1)
    w2_8, w2_e = ops.quant_rows_e4m3(w2)
    xn = torch.empty_like(x)
    h, h_fp8 = torch.empty(M, inner, dtype=torch.bfloat16, device=dev), torch.empty(M, inner, dtype=torch.bfloat16, device=dev)
    o, o_fp8 = torch.empty_like(x), torch.empty_like(x)
    entry = {"M": M, "C": C}

    # ---- FF1
    assert ops.fp8_linear_k64_supported(2 * inner, C, ops.EPI_GEGLU)
    ops.layernorm(x, gamma, beta, 1e-5, out=xn)
    xq = tuple(t.clone() for t in ops.layernorm_e4m3(x, gamma, beta, 1e-5))              # rows quantised beforehand: the kernel's own time
    before = ops.fp8_k64_launch_counts()
    arms = {"bf16": lambda: ops.linear(xn, w1, b1, epilogue=ops.EPI_GEGLU, out=h),
            "fp8_kernel": lambda: ops.linear_fp8_k64(xq, w1_8, w1_e, b1, epilogue=ops.EPI_GEGLU, out=h_fp8),
            "ln_bf16": lambda: ops.layernorm(x, gamma, beta, 1e-5, out=xn),
            "ln_e4m3": lambda: ops.layernorm_e4m3(x, gamma, beta, 1e-5),
            "bf16_site": lambda: ops.linear(ops.layernorm(x, gamma, beta, 1e-5, out=xn), w1, b1, epilogue=ops.EPI_GEGLU, out=h),
            "fp8_site": lambda: ops.linear_fp8_k64(ops.layernorm_e4m3(x, gamma, beta, 1e-5), w1_8, w1_e, b1, epilogue=ops.EPI_GEGLU, out=h_fp8)}
    with ops.dispatched() as d:
        arms["bf16"]()
    r = interleaved(arms, args.reps)
    assert ops.fp8_k64_launch_counts()["ln"] > before["ln"]                                  # the fused LayerNorm ran, not its fall-back
    flop = 2.0 * M * 2 * inner * C
    ratios(r, flop, "bf16", "fp8_kernel", (r["bf16_site"]["median_ms"], r["fp8_site"]["median_ms"]))
    r["fp8_site_tflops"] = round(flop / r["fp8_site"]["median_ms"] * 1e-9, 1)
    r["speedup_ln"] = round(r["ln_bf16"]["median_ms"] / r["ln_e4m3"]["median_ms"], 3)
    r["rel_fro_vs_bf16"] = rel(h_fp8, h)
    r["shape"] = {"N": 2 * inner, "K": C, "gflop": round(flop * 1e-9, 1), "bf16_kernels": d.counts}
    entry["ff1"] = r
    print(f"# {name} ff1: {json.dumps(r)}", file=sys.stderr, flush=True)

    # ---- FF2
    assert ops.fp8_linear_k64_supported(C, inner, ops.EPI_RESID)
    hq = ops.quant_rows_e4m3(h)
    hq_ws = (torch.empty_like(hq[0]), torch.empty_like(hq[1]))
    arms = {"bf16": lambda: ops.linear(h, w2, b2, epilogue=ops.EPI_RESID, resid=x, out=o),
            "fp8_kernel": lambda: ops.linear_fp8_k64(hq, w2_8, w2_e, b2, epilogue=ops.EPI_RESID, resid=x, out=o_fp8),
            "fp8_quant": lambda: ops.quant_rows_e4m3(h, out=hq_ws),
            "fp8_path": lambda: ops.linear_fp8_k64(h, w2_8, w2_e, b2, epilogue=ops.EPI_RESID, resid=x, out=o_fp8)}
    with ops.dispatched() as d:
        arms["bf16"]()
    r = interleaved(arms, args.reps)
    flop = 2.0 * M * C * inner
    ratios(r, flop, "bf16", "fp8_kernel", (r["bf16"]["median_ms"], r["fp8_path"]["median_ms"]))
    r["fp8_path_tflops"] = round(flop / r["fp8_path"]["median_ms"] * 1e-9, 1)
    r["rel_fro_vs_bf16"] = rel(o_fp8, o)
    r["shape"] = {"N": C, "K": inner, "gflop": round(flop * 1e-9, 1), "bf16_kernels": d.counts}
    entry["ff2"] = r
    print(f"# {name} ff2: {json.dumps(r)}", file=sys.stderr, flush=True)
    result["gemms"][name] = entry
    del x, xn, h, h_fp8, o, o_fp8, w1, w2, w1_8, w2_8, xq, hq, hq_ws, arms
    torch.cuda.empty_cache()


ARMS = (("off", None, False), ("ff1", ("ff1",), False), ("ff2", ("ff2",), False), ("ff1_ff2", ("ff1", "ff2"), False), ("conv", None, True),
        ("conv_ff1_ff2", ("ff1", "ff2"), True))


def measure_step(name, model, run):
    """`run()` under every arm of ARMS: the switches are set outside the timed window, round by round"""
    t, outs, launches = {a[0]: [] for a in ARMS}, {}, {}
    with torch.no_grad():
        for rep in range(2 + args.step_reps):                                   # two warm rounds
            for arm, sites, conv in ARMS:
                layers.set_ff_precision(model, "fp8" if sites else "bf16", sites or layers.FF_SITES)
                layers.set_conv_precision(model, "fp8" if conv else "bf16")
                before = ops.fp8_k64_launch_counts()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = run()
                e1.record()
                e1.synchronize()
                after = ops.fp8_k64_launch_counts()
                launches[arm] = {k: after[k] - before[k] for k in after}
                if rep == 1:
                    outs[arm] = out.clone()
                if rep >= 2:
                    t[arm].append(e0.elapsed_time(e1))
    layers.set_ff_precision(model, "bf16")
    layers.set_conv_precision(model, "bf16")
    r = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for k, v in t.items()}
    assert launches["off"] == {"gemm": 0, "ln": 0} and launches["conv"] == {"gemm": 0, "ln": 0}
    for arm, _, _ in ARMS[1:]:
        r[arm]["k64_launches_per_call"] = launches[arm]
        r[arm]["rel_fro_vs_off"] = rel(outs[arm], outs["off"])
        r[arm]["saved_ms"] = round(r["off"]["median_ms"] - r[arm]["median_ms"], 3)
        r[arm]["speedup_vs_off"] = round(r["off"]["median_ms"] / r[arm]["median_ms"], 4)
    r["conv_ff1_ff2"]["speedup_vs_conv"] = round(r["conv"]["median_ms"] / r["conv_ff1_ff2"]["median_ms"], 4)
    result.setdefault("steps", {})[name] = r
    print(f"# {name}: {json.dumps(r)}", file=sys.stderr, flush=True)


if not args.no_steps:
    if args.open_gates:
        layers.FF_FP8_MIN_ROWS = layers.FF2_FP8_MIN_ROWS = layers.FF2_FP8_MIN_WIDTH = 0
    result["step_reps"], result["gates_steps"] = args.step_reps, gates()
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
