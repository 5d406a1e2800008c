"""The opt-in MXFP6 (e2m3, block-scaled) linear path against the bf16 and fp8 launches it stands beside, on the DiT's shapes (DESIGN 3.7,
profiles/gemm_mxfp6.txt).

(a) per site at M = 35 552 rows (2 x 17 776), (N, K) = QKV (9216, 3072), to_out (3072, 3072), FF1 (12288, 3072), FF2 (3072, 12288), each with its
    production epilogue, random gaussian operands, three arms: the bf16 launch (ops.linear; for QKV the fused ops.qkv_linear_qknorm_rope), the fp8
    path (ops.linear_fp8) and the MXFP6 path (ops.linear_mxfp6) -- each low-precision arm as the model issues it (quantiser + GEMM; for QKV plus the
    stand-alone norm / RoPE kernel), its GEMM alone on operands quantised beforehand, and its quantiser alone.  TFLOP/s = 2 M N K over the time.
(b) the DiT CFG step (bench.build_models: 42 layers, 13 latent frames, batch 2) with each switch: bf16, fp8, mxfp6.

One process, the arms interleaved round by round, HIP events around each call group; medians and minima.  The rule the numbers decide: a site whose
MXFP6 path is not faster than its fp8 path leaves the default `sites` of set_linear_precision(model, "mxfp6").

    python tools/gemm_mxfp6_measure.py [--rows M] [--reps R] [--layers L] [--step-reps R] [--no-step] [--out FILE]      # prints one JSON object"""
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
ptr = lambda t: ctypes.c_void_p(t.data_ptr())


def timed(fn, inner=2):
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


def gemm_alone(entry, N, K, A, W, bias, out, epilogue, tail=(), **fields):
    """mrag_gemm_fp8 / mrag_gemm_mxfp6 on operands quantised beforehand: the GEMM's own time"""
    a = _lib.GemmFp8Args()
    a.A8, a.W8, a.bias, a.C = ptr(A), ptr(W), ptr(bias), ptr(out)
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.epilogue = M, N, K, K, K, out.stride(0), epilogue
    for k, v in fields.items():
        setattr(a, k, ptr(v) if isinstance(v, torch.Tensor) else v)
    L = _lib.lib()
    extra = tuple(ptr(t) for t in tail)
    return lambda: _lib.check(getattr(L, entry)(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a), *extra), entry)


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
    w6, w6s = ops.quant_rows_mxfp6(w)
    a6, a6s = ops.quant_rows_mxfp6(x)
    gated = epi == ops.EPI_GATE_RESID
    outs = {k: (rnd(B, S, N) if gated else torch.empty(B, S, N, dtype=torch.bfloat16, device=dev)) for k in ("bf16", "fp8", "mxfp6")}   # the gated sites update the residual stream in place
    kws = {k: (dict(resid=o, **gate_kw) if gated else {}) for k, o in outs.items()}
    raw = lambda k: dict(resid=outs[k].view(M, N), ldr=N, **{f: v for f, v in gate_kw.items()}) if gated else {}
    nr = lambda o: ops.qknorm_rope_(o, H, ones, zeros, ones, zeros, cos, sin, TEXT, **qk)
    arms = {}
    if site == "qkv":
        arms["bf16"] = lambda: ops.qkv_linear_qknorm_rope(x, w, bias, H, ones, zeros, ones, zeros, cos, sin, TEXT, out=outs["bf16"], **qk)
        arms["normrope"] = lambda: nr(outs["fp8"])
        arms["fp8_path"] = lambda: (ops.linear_fp8(x, w8, w_exp, bias, out=outs["fp8"]), nr(outs["fp8"]))
        arms["mxfp6_path"] = lambda: (ops.linear_mxfp6(x, w6, w6s, bias, out=outs["mxfp6"]), nr(outs["mxfp6"]))
    else:
        arms["bf16"] = lambda: ops.linear(x, w, bias, out=outs["bf16"], epilogue=epi, **kws["bf16"])
        arms["fp8_path"] = lambda: ops.linear_fp8(x, w8, w_exp, bias, out=outs["fp8"], epilogue=epi, **kws["fp8"])
        arms["mxfp6_path"] = lambda: ops.linear_mxfp6(x, w6, w6s, bias, out=outs["mxfp6"], epilogue=epi, **kws["mxfp6"])
    arms["fp8_gemm"] = gemm_alone("mrag_gemm_fp8", N, K, a8, w8, bias, outs["fp8"].view(M, N), epi, a_exp=a_exp, w_exp=w_exp, **raw("fp8"))
    arms["mxfp6_gemm"] = gemm_alone("mrag_gemm_mxfp6", N, K, a6, w6, bias, outs["mxfp6"].view(M, N), epi, tail=(a6s, w6s), **raw("mxfp6"))
    arms["fp8_quant"] = lambda: ops.quant_rows_e4m3(x, out=(a8, a_exp))
    arms["mxfp6_quant"] = lambda: ops.quant_rows_mxfp6(x, out=(a6, a6s))
    r = interleaved(arms, args.reps)
    flop = 2.0 * M * N * K
    for k in ("bf16", "fp8_path", "fp8_gemm", "mxfp6_path", "mxfp6_gemm"):
        r[k]["tflops"] = round(flop / r[k]["median_ms"] * 1e-9, 1)
    r["mxfp6_gemm_vs_fp8_gemm"] = round(r["fp8_gemm"]["median_ms"] / r["mxfp6_gemm"]["median_ms"], 3)
    r["mxfp6_path_vs_fp8_path"] = round(r["fp8_path"]["median_ms"] / r["mxfp6_path"]["median_ms"], 3)
    r["mxfp6_path_vs_bf16"] = round(r["bf16"]["median_ms"] / r["mxfp6_path"]["median_ms"], 3)
    r["fp8_path_vs_bf16"] = round(r["bf16"]["median_ms"] / r["fp8_path"]["median_ms"], 3)
    r["shape"] = {"M": M, "N": N, "K": K, "epilogue": epi}
    result["sites"][site] = r
    print(f"# {site}: {json.dumps(r)}", file=sys.stderr, flush=True)
    del x, w, bias, w8, w_exp, a8, a_exp, w6, w6s, a6, a6s, outs, kws, arms
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
    step_out = {}

    def step_arm(precision):
        def run():
            cogvideox.set_linear_precision(dit, precision)
            step_out[precision] = dit(latents, prompt, timestep, image_rotary_emb=rope_ip, image_latents=image_latents, batch=2)
            cogvideox.set_linear_precision(dit, "bf16")
        return run
    r = interleaved({p: step_arm(p) for p in ("bf16", "fp8", "mxfp6")}, args.step_reps, warm=1, inner=1)
    ref = step_out["bf16"].float()
    r["rel_fro_vs_bf16_step"] = {k: round(((v.float() - ref).norm() / ref.norm()).item(), 5) for k, v in step_out.items() if k != "bf16"}
    r["layers"], r["step_reps"] = args.layers, args.step_reps
    r["saved_ms_fp8"] = round(r["bf16"]["median_ms"] - r["fp8"]["median_ms"], 2)
    r["saved_ms_mxfp6"] = round(r["bf16"]["median_ms"] - r["mxfp6"]["median_ms"], 2)
    result["dit_cfg_step"] = r

text = json.dumps(result, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
