"""The MFMA attention for head dims other than 64 (ops.attention_hd, attn_hd.hip) against the fp32-FMA kernel it can replace (ops.attention_small), and what
either is of a CLIP-ViT-H tower pass.

(a) the kernel alone, CLIP-ViT-H/14's attention (16 heads of 80) on a fused [B, S, 3, 16, 80] buffer as the tower lays it out:
      (B, S) = (1, 257), (2, 257), (64, 257)   attention_small against attention_hd
      (B, S) = (1, 577), (1, 1025)             attention_hd alone: attention_small refuses these (K and V of a head beyond its LDS)
    A sample is `--launches` back-to-back launches between two HIP events, divided by their number: one launch is a few microseconds to a few hundred.
(b) one full tower pass (clip_vision.CLIPVisionModelWithProjection at its defaults: 32 layers x 1280, 257 tokens, random weights) at B = 1 and B = 2 with
    clip_vision.set_attention_kernel "fma" (the default) and "mfma", and the relative L2 distance of the two arms' last_hidden_state.

One process, the arms interleaved round by round, medians and minima after warm-up.

    python tools/attn_hd_measure.py [--reps R] [--launches N] [--layers L] [--out FILE]      # prints one JSON object"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import clip_vision, ops

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback and no CPU figure"
dev = "cuda"
torch.cuda.set_device(0)
H, D = 16, 80


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(arms, reps, per=1, warm=2):
    for fn in arms.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn) / per)
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5)} for k, v in t.items()}


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "launches_per_sample": args.launches, "heads": H, "head_dim": D, "kernel_alone": {}, "tower": {}}
gen = torch.Generator(device=dev).manual_seed(11)
for B, S in ((1, 257), (2, 257), (64, 257), (1, 577), (1, 1025)):
    qkv = (torch.randn(B, S, 3, H, D, generator=gen, device=dev) * 0.7).to(torch.bfloat16)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    out = torch.empty(B, S, H * D, dtype=torch.bfloat16, device=dev)

    def many(op):
        def f():
            for _ in range(args.launches):
                op(q, k, v, out=out)
        return f
    arms = {"attention_hd": many(ops.attention_hd)}
    both = S * D <= ops.ATTN_SMALL_MAX_KEY_ELEMS
    if both:
        arms = {"attention_small": many(ops.attention_small), **arms}
    r = interleaved(arms, args.reps, per=args.launches)
    r["flops"] = 4 * B * H * S * S * D
    r["attention_hd"]["tflops"] = round(r["flops"] / (r["attention_hd"]["median_ms"] * 1e-3) / 1e12, 2)
    if both:
        r["speedup_hd_vs_small"] = round(r["attention_small"]["median_ms"] / r["attention_hd"]["median_ms"], 2)
        r["rel_l2_hd_vs_small"] = float(f"{rel(ops.attention_hd(q, k, v), ops.attention_small(q, k, v)):.3e}")
    else:
        r["attention_small"] = "refused (Skv * head_dim > 32 768)"
    result["kernel_alone"][f"B={B} S={S}"] = r
    print(f"# B={B} S={S}: {json.dumps(r)}", file=sys.stderr, flush=True)

torch.manual_seed(0)
tower = clip_vision.CLIPVisionModelWithProjection(num_hidden_layers=args.layers).to(dev, torch.bfloat16)
for B in (1, 2):
    pix = torch.randn(B, 3, 224, 224, generator=gen, device=dev).to(torch.bfloat16)

    def run(kernel):
        def f():
            clip_vision.set_attention_kernel(tower, kernel)
            return tower(pix).last_hidden_state
        return f
    n0 = ops.attn_hd_launch_counts()
    on = run("mfma")()
    launches = ops.attn_hd_launch_counts() - n0
    off = run("fma")()
    r = interleaved({"fma": run("fma"), "mfma": run("mfma")}, args.reps)
    r["mfma"]["attention_hd_launches"] = launches
    r["speedup_mfma_vs_fma"] = round(r["fma"]["median_ms"] / r["mfma"]["median_ms"], 3)
    r["rel_l2_mfma_vs_fma_last_hidden_state"] = float(f"{rel(on, off):.3e}")
    ka = result["kernel_alone"][f"B={B} S=257"]
    r["attention_share_of_pass"] = {k: round(args.layers * ka[a]["median_ms"] / r[k]["median_ms"], 3) for k, a in (("fma", "attention_small"), ("mfma", "attention_hd"))}
    result["tower"][f"B={B}"] = r
    print(f"# tower B={B}: {json.dumps(r)}", file=sys.stderr, flush=True)
clip_vision.set_attention_kernel(tower, "fma")
result["tower"]["layers"] = args.layers

text = json.dumps(result, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
