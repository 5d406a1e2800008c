"""Record what every `motionrag_amd.ops` call of a pytest run returned, to compare two trees that must launch the same work (a host-side refactor against its
parent: same library, same tests, the traces must be equal).

    python tools/ops_trace.py OUT.json <pytest arguments...>

Wraps every public function of `motionrag_amd.ops`; a call that returns a tensor or a tuple of tensors appends (op name, shape, dtype, sha1 of the result's
bytes) -- one entry per tensor -- to the sequence of the test that is running (a plugin object handed to `pytest.main` supplies the test id; no pytest setting
and no conftest changes; the same object seeds torch's global generators with 0 before each test, so that weights a test draws without a seed of its own are the
same in both runs).  Calls between tests (module-level fixtures) go under "<outside>".  OUT.json holds the per-test sequences, one sha256 over all of
them, and the final `ops.dispatch_counts()`.  One process, nothing spawned; forwards that a test runs in worker processes are not seen.  The hashes read every
result back to the host, so the run is slower than the plain suite: it is a comparison tool, not a timing one.  Exit status: pytest's.

    python tools/ops_trace.py --diff A.json B.json      # test ids in both files whose sequences differ, and whether the dispatch counts are equal
"""
import functools
import hashlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUTSIDE = "<outside>"


def diff(path_a: str, path_b: str) -> int:
    with open(path_a) as fa, open(path_b) as fb:
        a, b = json.load(fa), json.load(fb)
    both = sorted(set(a["tests"]) & set(b["tests"]))
    bad = [t for t in both if a["tests"][t] != b["tests"][t]]
    for t in bad:
        sa, sb = a["tests"][t], b["tests"][t]
        i = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), min(len(sa), len(sb)))
        print(f"DIFF {t}: {len(sa)} / {len(sb)} entries, first difference at {i}: {sa[i] if i < len(sa) else None} / {sb[i] if i < len(sb) else None}")
    counts = a["dispatch_counts"] == b["dispatch_counts"]
    print(json.dumps({"tests_in_both": len(both), "only_in_a": len(set(a["tests"]) - set(b["tests"])), "only_in_b": len(set(b["tests"]) - set(a["tests"])),
                      "entries_compared": sum(len(a["tests"][t]) for t in both), "tests_that_differ": len(bad), "dispatch_counts_equal": counts,
                      "sha256": [a["sha256"], b["sha256"]]}))
    return 1 if bad or not counts else 0


def main(argv) -> int:
    if len(argv) == 3 and argv[0] == "--diff":
        return diff(argv[1], argv[2])
    if not argv or argv[0].startswith("-"):
        print(__doc__, file=sys.stderr)
        return 2
    import pytest
    import torch
    from motionrag_amd import ops
    trace, current = {}, [OUTSIDE]

    class Plugin:
        def pytest_runtest_logstart(self, nodeid, location):
            current[0] = nodeid
            torch.manual_seed(0)          # torch seeds its global generators from entropy: a test that draws weights without a seed of its own must draw the same ones in both runs

        def pytest_runtest_logfinish(self, nodeid, location):
            current[0] = OUTSIDE

    def record(name, t):
        if t.is_cuda and torch.cuda.is_current_stream_capturing():          # nothing may be read back while a graph is captured: the call is still listed
            sha1 = "captured"
        else:
            sha1 = hashlib.sha1(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
        trace.setdefault(current[0], []).append([name, list(t.shape), str(t.dtype), sha1])

    def wrap(name, fn):
        @functools.wraps(fn)
        def traced(*a, **kw):
            r = fn(*a, **kw)
            rs = r if isinstance(r, tuple) else (r,)
            if rs and all(isinstance(t, torch.Tensor) for t in rs):
                for t in rs:
                    record(name, t)
            return r
        return traced

    for name, fn in list(vars(ops).items()):
        if not name.startswith("_") and inspect.isfunction(fn) and fn.__module__ == ops.__name__:
            setattr(ops, name, wrap(name, fn))
    status = int(pytest.main(argv[1:], plugins=[Plugin()]))
    try:
        counts = ops.dispatch_counts()
    except Exception as e:                                   # no library (a CPU-only run): the trace is still worth writing
        counts = {"error": repr(e)}
    digest = hashlib.sha256(json.dumps(trace, sort_keys=True).encode()).hexdigest()
    os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
    with open(argv[0], "w") as f:
        json.dump({"tests": trace, "sha256": digest, "dispatch_counts": counts}, f)
    print(f"ops_trace: {sum(len(v) for v in trace.values())} results of {len(trace)} tests, sha256 {digest} -> {argv[0]}")
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
