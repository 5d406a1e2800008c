"""Device times of the wide fan-out lists (ops.topk(order="mfma" / "mfma_stream") at 17 <= k <= 32) beside the scan form they replace and the existing fan-out
form at k <= 16, with the post-filter, 768-d rows:
  10 000 rows x 256 queries: k = 21 "chain16" (the baseline: what order="auto" runs for this call), k = 21 "mfma" (wide dense form), k = 21 "mfma_stream" (wide
    streaming form), k = 32 "mfma", k = 12 and k = 16 "mfma" (the existing form: the floor), and the two launches of RAGDatabase.text_image_search_batch at
    top_k = (21, 9) -- ops.topk + ops.topk_rerank on a 1 024-d image column -- with stage 1 as `wide_fanout=False` ("auto") and `=True` ("mfma") issue it;
  10^6 rows x 256 queries (the plan streams): the three k = 21 arms.
One process, arms interleaved, HIP events; every timed group is enqueued behind a blocker (1 GiB device copies) so that the events bracket device work, not the
host's enqueue -- the blocker's time and the host's enqueue time are printed beside each figure (the first must exceed the second).  Medians with min / max over
the rounds.  DESIGN 3.7q, profiles/topk_wide_fanout.txt.

    python tools/topk_wide_measure.py [--quick] [--no-large] [--out FILE]      # prints one JSON object"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from motionrag_amd import ops

quick = "--quick" in sys.argv
dev = "cuda"
torch.cuda.set_device(0)
gen = torch.Generator(device=dev).manual_seed(1)
def unit(n, d):
    x = torch.randn(n, d, generator=gen, device=dev, dtype=torch.float32); return x / x.norm(dim=1, keepdim=True)
Q = 256
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

def measure(variants, rounds):
    for fn, _, _ in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    aux = {k: [] for k in variants}
    for _ in range(rounds):
        for name, (fn, inner, nb) in variants.items():
            us, blk, host = timed(fn, inner, nb)
            res[name].append(us); aux[name].append((blk, host))
    out = {}
    for name, (fn, _, _) in variants.items():
        with ops.dispatched() as d: fn()
        out[name] = {"median_us": round(statistics.median(res[name]), 1), "min_us": round(min(res[name]), 1), "max_us": round(max(res[name]), 1),
                     "blocker_us_median": round(statistics.median(a[0] for a in aux[name]), 0),
                     "host_enqueue_us_median": round(statistics.median(a[1] for a in aux[name]), 0), "dispatch": d.counts}
    return out

def arms(N, with_batch):
    text, qt = unit(N, 768), unit(Q, 768)
    group = torch.arange(N, dtype=torch.int32, device=dev)
    excl = torch.randint(0, N, (Q,), generator=gen, device=dev, dtype=torch.int32)
    outs = {k: (torch.empty(Q, k, dtype=torch.int32, device=dev), torch.empty(Q, k, dtype=torch.float32, device=dev)) for k in (12, 16, 21, 32)}
    def search(k, order):
        return lambda: ops.topk(text, qt, k, group=group, exclude=excl, postfilter=True, out=outs[k], order=order)
    v = {"k21_chain16_scan": search(21, "chain16"), "k21_mfma": search(21, "mfma"), "k21_mfma_stream": search(21, "mfma_stream")}
    if with_batch:
        v.update({"k32_mfma": search(32, "mfma"), "k12_mfma": search(12, "mfma"), "k16_mfma": search(16, "mfma")})
        img, qi = unit(N, 1024), unit(Q, 1024)
        o9 = tuple(torch.empty(Q, 9, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32))
        def batch(order):
            s1 = search(21, order)
            def run():
                s1(); ops.topk_rerank(img, qi, outs[21][0], 9, out=o9)
            return run
        v.update({"batch_21_9_flag_off": batch("auto"), "batch_21_9_flag_on": batch("mfma")})
    return v

out = {"queries": Q, "dim": 768, "postfilter": True}
small = arms(10000, True)
out["rows_10000"] = dict(rounds=3 if quick else 15, **measure({k: (fn, 20, 4) for k, fn in small.items()}, 3 if quick else 15))
del small
if "--no-large" not in sys.argv:
    large = arms(10 ** 6, False)
    out["rows_1000000"] = dict(rounds=2 if quick else 7, **measure({k: (fn, 3, 4) for k, fn in large.items()}, 2 if quick else 7))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
