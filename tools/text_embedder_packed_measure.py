"""The text embedder's packed path against the grouped path it would replace.

(a) per encode -- SentenceEmbedder.encode over `--n` captions (gte-base-en-v1.5's geometry, gte_ref.CONFIG_BASE, random weights):
      arm A  packed=False: one forward pass per distinct token count (what every caller runs today)
      arm B  packed=True:  passes of at most --max-tokens tokens through NewModel.forward_packed / ops.attention_varlen
    on two caption sets: `captions`, rag.synthetic_captions through a WordPiece-like stand-in (words cut into pieces of three characters, digits one by one),
    and `spread`, one to eight of those captions joined, which spreads the token counts over the 10 to 150 of real motion captions.  Beside the times:
    the forward passes each arm made, the token count, and the padded token count of one rectangular batch.
(b) the attention kernel alone -- ops.attention_varlen at the cu_seqlens of the sorted caption set (passes of --max-tokens) against the sum of the per-length
    ops.attention launches of the grouped path, 12 heads.

One process, the arms interleaved round by round, HIP events around each call, medians and minima after warm-up.  Every comparison is against the grouped
path of the same tree, never against the packed code itself.

    python tools/text_embedder_packed_measure.py [--n N] [--reps R] [--max-tokens T] [--out FILE]      # prints one JSON object"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import ops, rag
from motionrag_amd.text_embedder import NewModel, SentenceEmbedder, pack_lengths, plan_passes
from oracle import gte_ref

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--max-tokens", type=int, default=32768)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback and no CPU figure"
dev = "cuda"
torch.cuda.set_device(0)


def tok(texts):
    """WordPiece-like stand-in: [CLS], every word cut into pieces of three characters (digits one by one), [SEP]; ids by hash into the vocabulary"""
    out = []
    for t in texts:
        ids = [101]
        for w in t.replace(":", " : ").split():
            pieces = list(w) if w.isdigit() else [w[i:i + 3] for i in range(0, len(w), 3)]
            ids += [1000 + (sum(map(ord, p)) * 31 + len(p)) % 29000 for p in pieces]
        out.append(ids + [102])
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(arms, reps, warm=1):
    for fn in arms.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn))
    return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)} for k, v in t.items()}


torch.manual_seed(0)
model = NewModel(**gte_ref.CONFIG_BASE).to(dev, torch.bfloat16)
H = model.config.num_attention_heads
base = [a["motion_caption"] for a in rag.synthetic_captions(8 * args.n)]
SETS = {"captions": base[:args.n],
        "spread": [" ".join(base[8 * i:8 * i + 1 + (i * 5) % 8]) for i in range(args.n)]}
result = {"device": torch.cuda.get_device_name(0), "n_texts": args.n, "reps": args.reps, "max_tokens": args.max_tokens, "config": "gte_ref.CONFIG_BASE, random weights",
          "sets": {}}

for name, texts in SETS.items():
    lengths = [len(t) for t in tok(texts)]
    order = sorted(range(len(texts)), key=lambda i: lengths[i])
    passes = plan_passes(lengths, order, args.max_tokens)
    grouped, packed = SentenceEmbedder(model, tok), SentenceEmbedder(model, tok, packed=True, max_tokens=args.max_tokens)
    n0 = ops.attn_varlen_launch_counts()
    Ep = packed.encode(texts)
    varlen_launches = ops.attn_varlen_launch_counts() - n0
    Eg = grouped.encode(texts)
    r = interleaved({"grouped": lambda: grouped.encode(texts), "packed": lambda: packed.encode(texts)}, args.reps)
    r["grouped"]["forward_passes"] = len(set(lengths))
    r["packed"]["forward_passes"] = len(passes)
    r["packed"]["varlen_attention_launches"] = varlen_launches
    r["speedup_packed_vs_grouped"] = round(r["grouped"]["median_ms"] / r["packed"]["median_ms"], 3)
    r["min_cosine_packed_vs_grouped"] = round((Ep * Eg).sum(1).min().item(), 5)
    r["tokens"] = {"total": sum(lengths), "shortest": min(lengths), "longest": max(lengths), "distinct_lengths": len(set(lengths)),
                   "padded_rectangular_batch": len(lengths) * max(lengths)}

    # (b) the attention kernel alone, on a fused QKV buffer as the model lays it out
    gen = torch.Generator(device=dev).manual_seed(7)
    by_len = {}
    for n in lengths:
        by_len[n] = by_len.get(n, 0) + 1
    fixed = [torch.randn(b, n, 3, H, 64, generator=gen, device=dev).to(torch.bfloat16) for n, b in sorted(by_len.items())]
    fixed_out = [torch.empty(t.shape[0], t.shape[1], H * 64, dtype=torch.bfloat16, device=dev) for t in fixed]
    var = []
    for rows in passes:
        cu, _, _ = pack_lengths([lengths[i] for i in rows])
        T = int(cu[-1])
        var.append((torch.randn(T, 3, H, 64, generator=gen, device=dev).to(torch.bfloat16), cu.to(dev), lengths[rows[-1]],
                    torch.empty(T, H * 64, dtype=torch.bfloat16, device=dev)))

    def attn_fixed():
        for t, o in zip(fixed, fixed_out):
            ops.attention(t[:, :, 0], t[:, :, 1], t[:, :, 2], out=o)

    def attn_varlen():
        for t, cu, longest, o in var:
            ops.attention_varlen(t[:, 0], t[:, 1], t[:, 2], cu, longest, out=o)
    with ops.dispatched() as d:
        attn_fixed()
    a = interleaved({"per_length_launches": attn_fixed, "varlen": attn_varlen}, max(args.reps, 10), warm=2)
    a["per_length_launches"]["launches"] = len(fixed)
    a["per_length_launches"]["kernels"] = d.counts
    a["varlen"]["launches"] = len(var)
    a["speedup_varlen_vs_per_length"] = round(a["per_length_launches"]["median_ms"] / a["varlen"]["median_ms"], 3)
    r["attention_alone_one_layer"] = a
    result["sets"][name] = r
    print(f"# {name}: {json.dumps(r)}", file=sys.stderr, flush=True)
    del fixed, fixed_out, var
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
