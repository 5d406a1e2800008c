"""Device times of the text-then-image retrieval batch (RAGDatabase.text_image_search_batch: ops.topk + ops.topk_rerank) at 10 000 rows x 256 queries,
top_k = (21, 9), 768-d text and 1 024-d image columns, beside what a caller without the re-rank kernel can do: the text search alone at k = 21 (scan form)
and k = 12 (fan-out form), and stage 2 as 256 separate ops.topk calls on 21-row sub-tables gathered beforehand.  One process, variants interleaved, HIP
events; every timed group is enqueued behind a blocker (1 GiB device copies) so that the events bracket device work, not the host's enqueue -- the
blocker's time and the host's enqueue time are printed beside each figure (the first must exceed the second).  DESIGN 3.7k, profiles/topk_rerank_text_image.txt.

    python tools/topk_rerank_measure.py [--quick] [--out FILE]      # prints one JSON object"""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from motionrag_amd import _lib, ops

quick = "--quick" in sys.argv
dev = "cuda"
torch.cuda.set_device(0)
rng = np.random.default_rng(1)
def unit(n, d):
    x = rng.standard_normal((n, d)).astype(np.float32); return x / np.linalg.norm(x, axis=1, keepdims=True)
N, Q, K0, K1 = 10000, 256, 21, 9
text, img = torch.from_numpy(unit(N, 768)).to(dev), torch.from_numpy(unit(N, 1024)).to(dev)
qt, qi = torch.from_numpy(unit(Q, 768)).to(dev), torch.from_numpy(unit(Q, 1024)).to(dev)
group = torch.arange(N, dtype=torch.int32, device=dev)
excl = torch.from_numpy(rng.integers(0, N, Q).astype(np.int32)).to(dev)
o21 = (torch.empty(Q, K0, dtype=torch.int32, device=dev), torch.empty(Q, K0, dtype=torch.float32, device=dev))
o12 = (torch.empty(Q, 12, dtype=torch.int32, device=dev), torch.empty(Q, 12, dtype=torch.float32, device=dev))
o9 = tuple(torch.empty(Q, K1, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32))
o1 = (torch.empty(1, K1, dtype=torch.int32, device=dev), torch.empty(1, K1, dtype=torch.float32, device=dev))

def stage1_k21(): ops.topk(text, qt, K0, group=group, exclude=excl, postfilter=True, out=o21)
def stage1_k12(): ops.topk(text, qt, 12, group=group, exclude=excl, postfilter=True, out=o12)
def rerank(): ops.topk_rerank(img, qi, o21[0], K1, out=o9)
def both(): stage1_k21(); rerank()
stage1_k21(); torch.cuda.synchronize()
cand = o21[0].clone()
subs = [img[cand[q].clamp(min=0).long()].contiguous() for q in range(Q)]       # gathered 21-row sub-tables, prepared OUTSIDE the timed region
qis = [qi[q:q + 1].contiguous() for q in range(Q)]
def stage2_loop():
    for q in range(Q):
        ops.topk(subs[q], qis[q], K1, out=o1)

blk_src = torch.empty(1 << 30, dtype=torch.uint8, device=dev); blk_dst = torch.empty_like(blk_src)
def blocker(n):
    for _ in range(n): blk_dst.copy_(blk_src)

def timed(fn, inner, nblock):
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    torch.cuda.synchronize()
    e0.record(); blocker(nblock); e1.record()
    t = time.perf_counter()
    for _ in range(inner): fn()
    host = time.perf_counter() - t
    e2.record(); torch.cuda.synchronize()
    return e1.elapsed_time(e2) * 1e3 / inner, e0.elapsed_time(e1) * 1e3, host * 1e6      # us per call, blocker us, host enqueue us (whole group)

variants = {"both_launches": (both, 20, 4), "rerank_alone": (rerank, 40, 4), "text_k21_scan": (stage1_k21, 20, 4), "text_k12_fanout": (stage1_k12, 20, 4),
            "stage2_as_256_topk_calls": (stage2_loop, 1, 40)}
for fn, _, _ in variants.values():
    fn(); fn()
torch.cuda.synchronize()
rounds = 3 if quick else 15
res = {k: [] for k in variants}
aux = {k: [] for k in variants}
for r in range(rounds):
    for name, (fn, inner, nb) in variants.items():
        us, blk, host = timed(fn, inner, nb)
        res[name].append(us); aux[name].append((blk, host))
out = {"rows": N, "queries": Q, "top_k": [K0, K1], "dims": [768, 1024], "rounds": rounds}
for name in variants:
    out[name] = {"median_us": round(statistics.median(res[name]), 1), "min_us": round(min(res[name]), 1), "max_us": round(max(res[name]), 1),
                 "blocker_us_median": round(statistics.median(a[0] for a in aux[name]), 0), "host_enqueue_us_median": round(statistics.median(a[1] for a in aux[name]), 0)}
if not quick:
    # unblocked, as a caller sees it: host clock around the call + synchronize
    def wall(fn, n=50):
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(n): fn()
        torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e6
    out["wall_us_per_call_with_sync_at_end"] = {k: round(wall(v[0], 50 if v[1] > 1 else 5), 1) for k, v in variants.items()}
    L = _lib.lib(); st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cp = lambda: _lib.check(L.mrag_probe_stream_copy(st, ctypes.c_void_p(blk_src.data_ptr()), ctypes.c_void_p(blk_dst.data_ptr()), blk_src.numel(), 0), "copy")
    cp(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20): cp()
    b.record(); torch.cuda.synchronize()
    out["stream_copy_TBps"] = round(2 * blk_src.numel() / (a.elapsed_time(b) / 20 * 1e-3) / 1e12, 3)
    with ops.dispatched() as d: both()
    out["dispatch_both"] = d.counts
    with ops.dispatched() as d: stage1_k12()
    out["dispatch_k12"] = d.counts
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
