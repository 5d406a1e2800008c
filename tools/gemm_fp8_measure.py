"""The opt-in fp8 (e4m3) linear path against the bf16 kernels it would replace, on the DiT's shapes (profiles/gemm_fp8_measure.json).

(a) per site at M = 35 552 rows (2 x 17 776), (N, K) = QKV (9216, 3072), to_out (3072, 3072), FF1 (12288, 3072), FF2 (3072, 12288), each with its
    production epilogue, random gaussian operands: the bf16 launch (ops.linear; for QKV the fused ops.qkv_linear_qknorm_rope), the fp8 GEMM alone
    (activations quantised beforehand), the row quantiser alone, their sum, the two as ops.linear_fp8 issues them, and for QKV the stand-alone
    norm / RoPE kernel the fp8 arm needs behind its GEMM.  TFLOP/s = 2 M N K over the time.
(b) the DiT CFG step (bench.build_models: 42 layers, 13 latent frames, batch 2) in bf16, with all four sites in fp8, and with each site alone.

One process, the arms interleaved round by round, HIP events around each call group, >= 20 timed rounds after warm-up (the step: --step-reps);
medians and minima.  The rule the numbers decide (against the bf16 kernels, not against the fp8 code itself): a site whose quantiser + GEMM is not
faster than its bf16 launch leaves cogvideox.set_linear_precision's default `sites`.

    python tools/gemm_fp8_measure.py [--rows M] [--reps R] [--layers L] [--step-reps R] [--no-step] [--out FILE]      # prints one JSON object"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import _lib, cogvideox, ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=17776, help="rows per CFG sample (the judged shape: 226 text + 17 550 video tokens)")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--layers", type=int, default=42)
ap.add_argument("--step-reps", type=int, default=5)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback and no CPU figure"
dev = "cuda"
torch.cuda.set_device(0)
S, B, TEXT, D, H = args.rows, 2, 226, 3072, 48
M = B * S
gen = torch.Generator(device=dev).manual_seed(7)
rnd = lambda *shape, std=1.0: (torch.randn(*shape, generator=gen, device=dev) * std).to(torch.bfloat16)


def timed(fn, inner=2):
    """device milliseconds per call of fn (HIP events around `inner` back-to-back calls: a call here is 0.1-5 ms of device work, the enqueue ~20 us)"""
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


def gemm8_alone(a8, a_exp, w8, w_exp, bias, out, epilogue, **kw):
    """mrag_gemm_fp8 on operands quantised beforehand: the GEMM's own time"""
    a = _lib.GemmFp8Args()
    a.A8, a.W8, a.a_exp, a.w_exp, a.bias, a.C = (ctypes.c_void_p(t.data_ptr()) for t in (a8, w8, a_exp, w_exp, bias, out))
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.epilogue = a8.shape[0], w8.shape[0], a8.shape[1], a8.stride(0), w8.stride(0), out.stride(0), epilogue
    if "resid" in kw:
        a.resid, a.ldr = ctypes.c_void_p(kw["resid"].data_ptr()), kw["resid"].stride(0)
        a.gate0, a.gate1 = ctypes.c_void_p(kw["gate0"].data_ptr()), ctypes.c_void_p(kw["gate1"].data_ptr())
        a.rows_per_batch, a.split, a.gate_stride = kw["rows_per_batch"], kw["split"], kw["gate_stride"]
    L = _lib.lib()
    return lambda: _lib.check(L.mrag_gemm_fp8(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a)), "mrag_gemm_fp8")


result = {"rows": M, "reps": args.reps, "device": torch.cuda.get_device_name(0), "sites": {}}
mod = rnd(B, 6 * D, std=0.05)                                  # AdaLN-zero gates: column slices of a modulation row
gate_kw = dict(gate0=mod[:, :D], gate1=mod[:, D:2 * D], rows_per_batch=S, split=TEXT, gate_stride=mod.stride(0))
cos, sin = (torch.randn(S - TEXT, 64, generator=gen, device=dev) for _ in range(2))
ones, zeros = torch.ones(64, dtype=torch.bfloat16, device=dev), torch.zeros(64, dtype=torch.bfloat16, device=dev)
qk = dict(eps=1e-6, q_premul=ops.LOG2E * 64 ** -0.5)

for site, N, K, epi in (("qkv", 3 * D, D, ops.EPI_NONE), ("to_out", D, D, ops.EPI_GATE_RESID), ("ff1", 4 * D, D, ops.EPI_GELU_TANH),
                        ("ff2", D, 4 * D, ops.EPI_GATE_RESID)):
    x, w, bias = rnd(B, S, K), rnd(N, K, std=0.02), rnd(N, std=0.02)
    w8, w_exp = ops.quant_rows_e4m3(w)
    a8, a_exp = ops.quant_rows_e4m3(x)
    gated = epi == ops.EPI_GATE_RESID
    out = rnd(B, S, N) if gated else torch.empty(B, S, N, dtype=torch.bfloat16, device=dev)      # the gated sites update the residual stream in place
    out8 = out.clone()
    kw = dict(resid=out, **gate_kw) if gated else {}
    kw8 = dict(resid=out8, **gate_kw) if gated else {}
    arms = {}
    if site == "qkv":
        arms["bf16"] = lambda: ops.qkv_linear_qknorm_rope(x, w, bias, H, ones, zeros, ones, zeros, cos, sin, TEXT, out=out, **qk)
        arms["fp8_normrope"] = lambda: ops.qknorm_rope_(out8, H, ones, zeros, ones, zeros, cos, sin, TEXT, **qk)
        arms["fp8_path"] = lambda: (ops.linear_fp8(x, w8, w_exp, bias, out=out8), ops.qknorm_rope_(out8, H, ones, zeros, ones, zeros, cos, sin, TEXT, **qk))
    else:
        arms["bf16"] = lambda: ops.linear(x, w, bias, out=out, epilogue=epi, **kw)
        arms["fp8_path"] = lambda: ops.linear_fp8(x, w8, w_exp, bias, out=out8, epilogue=epi, **kw8)
    arms["fp8_gemm"] = gemm8_alone(a8, a_exp, w8, w_exp, bias, out8.view(M, N), epi, **({k: (v.view(M, N) if k == "resid" else v) for k, v in kw8.items()}))
    arms["fp8_quant"] = lambda: ops.quant_rows_e4m3(x, out=(a8, a_exp))
    with ops.dispatched() as d:
        arms["bf16"]()
    r = interleaved(arms, args.reps)
    flop = 2.0 * M * N * K
    extra = r["fp8_normrope"]["median_ms"] if site == "qkv" else 0.0
    r["fp8_sum_ms"] = round(r["fp8_gemm"]["median_ms"] + r["fp8_quant"]["median_ms"] + extra, 4)
    r["bf16_tflops"] = round(flop / r["bf16"]["median_ms"] * 1e-9, 1)
    r["fp8_gemm_tflops"] = round(flop / r["fp8_gemm"]["median_ms"] * 1e-9, 1)
    r["fp8_path_tflops"] = round(flop / r["fp8_path"]["median_ms"] * 1e-9, 1)
    r["speedup_path_vs_bf16"] = round(r["bf16"]["median_ms"] / r["fp8_path"]["median_ms"], 3)
    r["fp8_faster"] = r["fp8_path"]["median_ms"] < r["bf16"]["median_ms"] and r["fp8_sum_ms"] < r["bf16"]["median_ms"]
    r["shape"] = {"M": M, "N": N, "K": K, "epilogue": epi, "bf16_kernels": d.counts}
    result["sites"][site] = r
    print(f"# {site}: {json.dumps(r)}", file=sys.stderr, flush=True)
    del x, w, bias, w8, w_exp, a8, a_exp, out, out8, arms, kw, kw8
    torch.cuda.empty_cache()

if not args.no_step:
    import bench                                                # the judged workload's model and inputs, by import
    lat_frames = 13
    dit, cam, pipe = bench.build_models(dev, args.layers, lat_frames)
    g = torch.Generator().manual_seed(1234)
    latents = torch.randn(1, lat_frames, 16, 60, 90, generator=g).to(dev, torch.bfloat16)
    image_latents = torch.randn(1, lat_frames, 16, 60, 90, generator=g).to(dev, torch.bfloat16)
    prompt = torch.randn(2, 226, 4096, generator=g).to(dev, torch.bfloat16)
    ref_videos = torch.zeros(1, 9, 16, 3, 8, 8, dtype=torch.bfloat16, device=dev)
    image = torch.zeros(1, 3, 8, 8, dtype=torch.bfloat16, device=dev)
    pipe.action_emb = pipe.prepare_action_embeddings(ref_videos, None, do_classifier_free_guidance=True, image=image)
    rope_ip = pipe._prepare_rotary_positional_embeddings(lat_frames, 30, 45, dev)
    timestep = torch.full((2,), 981.0, dtype=torch.float32, device=dev)
    outs = {}

    def step_arm(name, precision, sites=cogvideox.LINEAR_SITES):
        def run():
            cogvideox.set_linear_precision(dit, precision, sites)
            outs[name] = dit(latents, prompt, timestep, image_rotary_emb=rope_ip, image_latents=image_latents, batch=2)
            cogvideox.set_linear_precision(dit, "bf16")
        return run
    arms = {"bf16": step_arm("bf16", "bf16"), "fp8_all_sites": step_arm("fp8_all_sites", "fp8")}
    for s in cogvideox.LINEAR_SITES:
        arms["fp8_" + s] = step_arm("fp8_" + s, "fp8", (s,))
    r = interleaved(arms, args.step_reps, warm=1, inner=1)
    ref = outs["bf16"].float()
    r["rel_fro_vs_bf16_step"] = {k: round(((v.float() - ref).norm() / ref.norm()).item(), 5) for k, v in outs.items() if k != "bf16"}
    r["layers"], r["step_reps"] = args.layers, args.step_reps
    r["saved_ms_all_sites"] = round(r["bf16"]["median_ms"] - r["fp8_all_sites"]["median_ms"], 2)
    result["dit_cfg_step"] = r

text = json.dumps(result, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
