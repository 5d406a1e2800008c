"""The opt-in fp8 (e4m3) 3x3 convolution against the bf16 implicit GEMM it would replace.

(a) per shape -- DynamiCrafter-1024's ResBlock levels at 32 frames of the CFG pair (32 x 72 x 128 x 320 -> 320, 32 x 36 x 64 x 640 -> 640,
    32 x 18 x 32 x 1280 -> 1280, and the deepest, 32 x 9 x 16 x 1280 -> 1280: 90 tiles of 256 x 256, where the bf16 path runs 128 x 128 tiles) and
    SVD's level 0 (workloads.svd_step: 28 x 72 x 128 x 320 -> 320), bias, no residual, gaussian operands: the bf16 launch (ops.conv_implicit ->
    mrag_conv_bf16, the path the switch leaves), the fp8 kernel alone (activations quantised beforehand), the per-pixel quantiser alone, and the
    two as ops.conv_implicit_fp8 issues them.  TFLOP/s = 2 M Cout 9 Cin over the time.
(b) whole steps with layers.set_conv_precision off and on: the DynamiCrafter-1024 CFG UNet step and the SVD CFG step (workloads.py), and the
    DynamiCrafter KL-VAE decode of 16 x 576 x 1024; the relative Frobenius distance of the fp8 output from the bf16 one beside the times.

One process, the arms interleaved round by round, HIP events around each call group, medians and minima after warm-up.  Every comparison is against
the bf16 path, never against the fp8 code itself.

    python tools/conv_fp8_measure.py [--reps R] [--step-reps R] [--no-steps] [--out FILE]      # prints one JSON object"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import _lib, layers, ops, workloads

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--step-reps", type=int, default=7)
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


def conv8_alone(x8, x_exp, w8, w_exp, bias, out, N, H, W, Cin, Cout):
    """mrag_conv_fp8 on activations quantised beforehand: the kernel's own time"""
    a = _lib.ConvFp8Args()
    a.x8, a.W8, a.x_exp, a.w_exp, a.bias, a.y = (ctypes.c_void_p(t.data_ptr()) for t in (x8, w8, x_exp, w_exp, bias, out))
    a.N, a.H, a.Wd, a.Cin, a.Cout, a.stride, a.epilogue = N, H, W, Cin, Cout, 1, ops.EPI_NONE
    L = _lib.lib()
    return lambda: _lib.check(L.mrag_conv_fp8(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a)), "mrag_conv_fp8")


def rel(a, b):
    a, b = a.float(), b.float()
    return round(((a - b).norm() / b.norm()).item(), 5)


result = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
for name, (N, H, W, Cin, Cout) in (("dc_level0", (32, 72, 128, 320, 320)), ("dc_level1", (32, 36, 64, 640, 640)), ("dc_level2", (32, 18, 32, 1280, 1280)),
                                   ("dc_level3", (32, 9, 16, 1280, 1280)),
                                   ("svd_level0", (28, 72, 128, 320, 320))):
    assert ops.conv_fp8_supported(N, H, W, Cin, Cout)
    x, wk, bias = rnd(N, H, W, Cin), rnd(Cout, 9 * Cin, std=(9 * Cin) ** -0.5), rnd(Cout, std=0.02)
    w8, w_exp = ops.quant_rows_e4m3(wk)
    x8, x_exp = ops.quant_rows_e4m3(x.view(-1, Cin))
    out8 = torch.empty(N, H, W, Cout, dtype=torch.bfloat16, device=dev)
    arms = {"bf16": lambda: ops.conv_implicit(x, wk, bias, ops.CONV_3X3),
            "fp8_path": lambda: ops.conv_implicit_fp8(x, w8, w_exp, bias, out=out8),
            "fp8_kernel": conv8_alone(x8, x_exp, w8, w_exp, bias, out8, N, H, W, Cin, Cout),
            "fp8_quant": lambda: ops.quant_rows_e4m3(x.view(-1, Cin), out=(x8, x_exp))}
    with ops.dispatched() as d:
        ref = arms["bf16"]()
    r = interleaved(arms, args.reps)
    flop = 2.0 * N * H * W * Cout * 9 * Cin
    r["bf16_tflops"] = round(flop / r["bf16"]["median_ms"] * 1e-9, 1)
    r["fp8_kernel_tflops"] = round(flop / r["fp8_kernel"]["median_ms"] * 1e-9, 1)
    r["fp8_path_tflops"] = round(flop / r["fp8_path"]["median_ms"] * 1e-9, 1)
    r["speedup_path_vs_bf16"] = round(r["bf16"]["median_ms"] / r["fp8_path"]["median_ms"], 3)
    r["speedup_kernel_vs_bf16"] = round(r["bf16"]["median_ms"] / r["fp8_kernel"]["median_ms"], 3)
    r["rel_fro_vs_bf16"] = rel(ops.conv_implicit_fp8(x, w8, w_exp, bias), ref)
    r["shape"] = {"N": N, "H": H, "W": W, "Cin": Cin, "Cout": Cout, "gflop": round(flop * 1e-9, 1), "bf16_kernels": d.counts}
    result["shapes"][name] = r
    print(f"# {name}: {json.dumps(r)}", file=sys.stderr, flush=True)
    del x, wk, bias, w8, w_exp, x8, x_exp, out8, arms, ref
    torch.cuda.empty_cache()


def measure_step(name, model, run):
    """`run()` with the model's 3x3 convolutions in bf16 (off) / fp8 (on): the precision is set outside the timed window, round by round"""
    t, outs, launches = {"off": [], "on": []}, {}, {}
    with torch.no_grad():
        for rep in range(2 + args.step_reps):                                   # two warm rounds
            for arm, precision in (("off", "bf16"), ("on", "fp8")):
                layers.set_conv_precision(model, precision)
                before = ops.conv_fp8_launch_counts()["conv"]
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[arm] = run()
                e1.record()
                e1.synchronize()
                launches[arm] = ops.conv_fp8_launch_counts()["conv"] - before
                if rep >= 2:
                    t[arm].append(e0.elapsed_time(e1))
    layers.set_conv_precision(model, "bf16")
    r = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for k, v in t.items()}
    assert launches["off"] == 0 and launches["on"] > 0
    r["fp8_conv_launches_per_call"] = launches["on"]
    r["rel_fro_on_vs_off"] = rel(outs["on"], outs["off"])
    r["saved_ms"] = round(r["off"]["median_ms"] - r["on"]["median_ms"], 3)
    r["speedup_on_vs_off"] = round(r["off"]["median_ms"] / r["on"]["median_ms"], 4)
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
    del net, step, lat, reset
    torch.cuda.empty_cache()

    from motionrag_amd import dynamicrafter_vae as V
    torch.manual_seed(0)
    vae = V.AutoencoderKL(dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
                               attn_resolutions=[], dropout=0.0), embed_dim=4).to(dev, torch.bfloat16)
    z = (torch.randn(1, 4, 16, 72, 128, device=dev) * 0.18215).to(torch.bfloat16)
    measure_step("dc_vae_decode", vae, lambda: V.decode_first_stage(vae, z))

text = json.dumps(result, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
