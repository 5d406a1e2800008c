"""The opt-in fp8 (e4m3) joint attention against the bf16 kernel it would replace, on the DiT's shapes.

(B, H, Sq, Skv) = (2, 48, 17 776, 17 776) -- 49 frames at 480 x 720, 17 776 % 128 = 112 -- and (2, 48, 6 976, 6 976) -- the shipped 17-frame configuration,
6 976 % 128 = 64: the second sub-tile of the last stage is all padding -- with a pre-scaled Q (q_prescaled: what the QKV GEMM's epilogue hands over), random
gaussian operands as strided views of one fused [B, S, 3, H, 64] buffer.  Arms, interleaved round by round in one process, HIP events around each call:
    bf16        ops.attention(q, k, v, q_prescaled=True)                     the shipped kernel
    fp8         ops.joint_attention_fp8(q, k, v, q_prescaled=True)           memset + amax + quantise + attention kernel
    fp8_quant   the same entry point with MRAG_ATTN_TUNE_FP8_QUANT_ONLY       memset + amax + quantise alone
fp8_kernel = fp8 - fp8_quant (medians): the attention kernel alone.  TFLOP/s = 4 B H Sq Skv 64 over the time.  No threshold is attached: the path is opt-in
whatever the sign.

    python tools/attn_fp8_joint_measure.py [--reps R] [--shapes 17776,6976] [--out FILE]      # prints one JSON object"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--shapes", type=str, default="17776,6976", help="joint sequence lengths (Sq = Skv)")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback and no CPU figure"
dev = "cuda"
torch.cuda.set_device(0)
B, H = 2, 48
gen = torch.Generator(device=dev).manual_seed(7)


def timed(fn):
    """device milliseconds of one call of fn (HIP events; a call here is milliseconds of device work, the enqueue ~20 us)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(arms, reps, warm=2):
    for fn in arms.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for k, v in t.items()}


def quant_only(q, k, v, out):
    """mrag_attn_joint_fwd_fp8 with the developer knob that returns in front of the attention kernel: the argument block ops.joint_attention_fp8 builds"""
    a, _, _ = ops._attention_args(q, k, v, out, None, None, 1, None, 1.0, True, None, True)
    a.tuning |= ops.ATTN_TUNE_FP8_QUANT_ONLY
    ws = ops._attn_workspace(q.device, _lib.lib().mrag_attn_joint_fp8_workspace_bytes(a.B, a.H, a.Sq, a.Skv), "fp8")
    a.workspace, a.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), ws.numel()
    L = _lib.lib()
    return lambda: _lib.check(L.mrag_attn_joint_fwd_fp8(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(a)), "mrag_attn_joint_fwd_fp8")


result = {"B": B, "H": H, "reps": args.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
for S in (int(s) for s in args.shapes.split(",")):
    qkv = (torch.randn(B, S, 3, H, 64, generator=gen, device=dev) * torch.tensor([1.5 * 0.125 * ops.LOG2E, 0.7, 2.0], device=dev).view(1, 1, 3, 1, 1)).to(torch.bfloat16)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    out16, out8 = (torch.empty(B, S, H * 64, dtype=torch.bfloat16, device=dev) for _ in range(2))
    arms = {"bf16": lambda: ops.attention(q, k, v, out=out16, q_prescaled=True),
            "fp8": lambda: ops.joint_attention_fp8(q, k, v, out=out8, q_prescaled=True),
            "fp8_quant": quant_only(q, k, v, out8)}
    with ops.dispatched() as d:
        arms["bf16"](), arms["fp8"]()
    r = interleaved(arms, args.reps)
    flop = 4.0 * B * H * S * S * 64
    r["fp8_kernel_ms"] = round(r["fp8"]["median_ms"] - r["fp8_quant"]["median_ms"], 4)
    r["bf16_tflops"] = round(flop / r["bf16"]["median_ms"] * 1e-9, 1)
    r["fp8_tflops"] = round(flop / r["fp8"]["median_ms"] * 1e-9, 1)
    r["fp8_kernel_tflops"] = round(flop / r["fp8_kernel_ms"] * 1e-9, 1)
    r["speedup_fp8_vs_bf16"] = round(r["bf16"]["median_ms"] / r["fp8"]["median_ms"], 3)
    r["rel_fro_fp8_vs_bf16"] = round(((out8.float() - out16.float()).norm() / out16.float().norm()).item(), 5)
    r["shape"] = {"B": B, "H": H, "Sq": S, "Skv": S, "Skv_mod_128": S % 128, "q_prescaled": True, "kernels": d.counts}
    result["shapes"][str(S)] = r
    print(f"# S = {S}: {json.dumps(r)}", file=sys.stderr, flush=True)
    del qkv, q, k, v, out16, out8, arms
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
