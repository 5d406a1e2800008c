"""CPU suite of the wide fan-out lists (17 <= k <= 32 behind an explicit `order` of "mfma" / "mfma_stream" / "mfma_nowait"): the added C-ABI symbol
`mrag_topk_workspace_bytes_k`, the unchanged ABI version and dispatch names, the argument checks of `mrag_topk_f32` that return before anything is launched,
the conditions that make the fixtures of tests/test_gpu_topk_wide.py meaningful -- asserted here on the C oracle alone --, and `RAGDatabase`'s new keyword.
No compute calls on a device: the kernels are exercised by tests/test_gpu_topk_wide.py, which imports the fixture builders below."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def near_duplicate_fixture():
    """3 000 x 768 rows of 8 x N(0, 1) (unnormalised: |x|^2 ~ 49 000, an fp32 ulp of |q|^2 + |x|^2 is ~ 8e-3), 64 queries.  Query c < 32 IS the centre of a
    cluster of 40 rows, rows 40 c .. 40 c + 39 = centre + r_i x unit noise with r_i linear from 0.010 to 0.020: true squared distances 1e-4 .. 4e-4, far
    under the expansion's error, so the first score orders a cluster as noise (some scores negative) and only the second scoring tells its rows apart."""
    rng = np.random.default_rng(317)
    db = (8.0 * rng.standard_normal((3000, 768))).astype(np.float32)
    q = (8.0 * rng.standard_normal((64, 768))).astype(np.float32)
    radius = np.linspace(0.010, 0.020, 40).astype(np.float32)
    for c in range(32):
        centre = q[c]
        db[40 * c:40 * c + 40] = centre[None, :] + radius[:, None] * unit(rng, 40, 768)
    return db, q


def second_scoring_reaches_past_rank_16(db, q, k):
    """(rows, dist of oracle mode f32mfma; number of the 32 clustered queries whose list differs from the expansion-only mode at a rank >= 17)"""
    from oracle import topk_ref
    rows, dist = topk_ref.topk(db, q, k, "l2", mode="f32mfma")
    raw_rows, raw_dist = topk_ref.topk(db, q, k, "l2", mode="f32mfma_raw")
    moved = int((rows[:32, 16:] != raw_rows[:32, 16:]).any(axis=1).sum())
    return rows, dist, moved, raw_dist


def float64_rank_fixture():
    """10 000 x 768 unit rows, 64 queries; the first 16 next to a row whose group they exclude (the rule of test_topk_baseline_size_ranks_equal_float64_oracle)"""
    rng = np.random.default_rng(1)
    db, q = unit(rng, 10000, 768), unit(rng, 64, 768)
    group = np.arange(10000, dtype=np.int32)
    excl = rng.integers(0, 10000, 64).astype(np.int32)
    q[:16] = db[excl[:16]] + 0.01 * q[:16]
    return db, q, group, excl


def float64_rank_rule(want_r, want_d, k):
    """want_* = the float64 oracle's k + 1 nearest: -> (safe [Q, k] bool, rows [Q, k], dist [Q, k]).  A rank is compared when both neighbouring float64
    gaps exceed 2 tol, tol = 1e-6 max(|d|, 1) (the fp32 rounding bound of a 768-term sum on distances <= 2)"""
    gap = np.diff(want_d, axis=1)
    tol = 1e-6 * np.maximum(np.abs(want_d[:, :k]), 1.0)
    safe = np.ones(tol.shape, bool)
    safe &= gap > 2 * tol
    safe[:, 1:] &= gap[:, :-1] > 2 * tol[:, 1:]
    return safe, want_r[:, :k], want_d[:, :k]


def test_workspace_symbol_abi_version_and_dispatch_names():
    from motionrag_amd import _lib
    from test_rag_text_image_cpu import OLD_DISPATCH_NAMES
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    assert re.search(r"\bint64_t\s+mrag_topk_workspace_bytes_k\s*\(\s*int64_t\s+n_rows\s*,\s*int32_t\s+n_queries\s*,\s*int32_t\s+k\s*\)", hdr)
    assert "mrag_topk_workspace_bytes_k" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mrag_topk_workspace_bytes_k")
    assert _lib.ABI_VERSION == 11
    L = _lib.lib()
    assert L.mrag_abi_version() == 11                                             # an added entry point does not move it
    assert L.mrag_topk_workspace_bytes_k.argtypes == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    assert L.mrag_topk_workspace_bytes_k.restype is ctypes.c_int64
    assert len(L.mrag_topk_f32.argtypes) == 16                                     # no existing signature changed
    n = L.mrag_dispatch_counts(None, 0)
    names = [L.mrag_dispatch_name(i).decode() for i in range(n)]
    assert names == OLD_DISPATCH_NAMES + ["TOPK_RERANK"]                          # the wide launches count under the existing ids


GRID = [(10000, 256), (10 ** 6, 256), (70, 3), (66000, 64), (130, 16), (3000, 130), (20000, 256), (12000, 300), (70001, 40), (5000, 20), (9000, 300), (4000, 15),
        (10 ** 7, 16), (10 ** 6, 1000), (32768, 600)]


def test_workspace_bytes_by_k():
    from motionrag_amd import _lib
    _lib.build()
    L = _lib.lib()
    for N, Q in GRID:
        old = L.mrag_topk_workspace_bytes(N, Q)
        assert old > 0
        for k in range(1, 17):
            assert L.mrag_topk_workspace_bytes_k(N, Q, k) == old, (N, Q, k)
        prev = old
        for k in range(17, 33):
            w = L.mrag_topk_workspace_bytes_k(N, Q, k)
            assert w >= old and w >= prev, (N, Q, k, w, old, prev)                  # never smaller than the plain need, monotone in k
            prev = w
    assert L.mrag_topk_workspace_bytes_k(0, 16, 21) == 0 and L.mrag_topk_workspace_bytes_k(100, 0, 21) == 0      # as the plain function answers them


def test_argument_checks_return_before_any_launch():
    """fake (16-byte aligned) pointers: every call below must return from the argument checks"""
    from motionrag_amd import _lib
    _lib.build()
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    big = 1 << 40

    def call(nq, k, order, ws_bytes, n_rows=3000, dim=64):
        return L.mrag_topk_f32(None, one, None, n_rows, dim, one, None, nq, k, 0, one, one, one, ws_bytes, 0, order)
    for order in (2, 3, 4):
        assert call(64, 33, order, big) == -2                                     # k > 32: MRAG_ENOTSUP
        assert call(15, 21, order, big) == -2                                     # fewer than 16 queries
        assert call(15, 12, order, big) == -2                                     # (as before the wide lists)
        need = L.mrag_topk_workspace_bytes_k(3000, 64, 21)
        assert call(64, 21, order, need - 1) == -1                                # a workspace one byte short of the need of k = 21: MRAG_EINVAL
        assert call(64, 32, order, L.mrag_topk_workspace_bytes_k(3000, 64, 32) - 1) == -1
    assert call(64, 65, 2, big) == -2 and call(64, 0, 2, big) == -2
    assert call(64, 12, 2, L.mrag_topk_workspace_bytes(3000, 64) - 1) == -1       # k <= 16: the check it always was
    assert call(64, 21, 0, L.mrag_topk_workspace_bytes(3000, 64) - 1) == -1       # orders 0 / 1 at k = 21: against the plain need
    assert call(64, 21, 5, big) == -1 and call(64, 21, -1, big) == -1             # no such order
    assert call(64, 21, 2, big, dim=66) == -2                                     # dim % 4


@pytest.mark.parametrize("k", [17, 21, 32])
def test_near_duplicate_fixture_needs_the_second_scoring_past_rank_16(k):
    """what tests/test_gpu_topk_wide.py::test_second_scoring_past_rank_16 relies on, on the oracle alone: with the second scoring the lists of the clustered
    queries differ from the expansion-only lists at ranks >= 17 (measured: 31 - 32 of 32 queries at every k), some expansion scores are negative, and the
    re-scored distances are the exact ones (1e-4 .. 4e-4, ascending)"""
    db, q = near_duplicate_fixture()
    rows, dist, moved, raw_dist = second_scoring_reaches_past_rank_16(db, q, k)
    print(f"k = {k}: {moved} of 32 clustered queries differ from the expansion-only list at ranks >= 17; most negative expansion score {raw_dist.min():.3e}")
    assert moved >= 8
    assert (raw_dist[:32] < 0).any()
    assert (rows[:32] // 40 == np.arange(32)[:, None]).all()                      # every list stays inside the query's own cluster of 40
    assert (np.diff(dist, axis=1) >= 0).all() and dist[:32].min() > 0.5e-4 and dist[:32].max() < 5e-4


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_oracle_fanout_mode_ranks_like_float64_at_k21(metric):
    """the reference of tests/test_gpu_topk_wide.py::test_ranks_equal_float64 stays inside that test's bounds by itself: oracle mode f32mfma at k = 21
    against float64 under the gap rule (more than 98 % of the ranks compared, compared ranks equal, |d - d64| <= 2e-6)"""
    from oracle import topk_ref
    db, q, group, excl = float64_rank_fixture()
    want_r, want_d = topk_ref.topk(db, q, 22, metric, group, excl, mode="f64")
    safe, wr, wd = float64_rank_rule(want_r, want_d, 21)
    rows, dist = topk_ref.topk(db, q, 21, metric, group, excl, mode="f32mfma")
    print(f"{metric}: {100 * safe.mean():.2f} % of the ranks compared, max |d - d64| = {np.abs(dist - wd).max():.3e}")
    assert safe.mean() > 0.98
    assert np.array_equal(rows[safe], wr[safe])
    np.testing.assert_allclose(dist, wd, rtol=0, atol=2e-6)


def test_ragdatabase_accepts_the_flag_and_still_refuses_a_cpu_device(tmp_path):
    from motionrag_amd import ops, rag
    rows = [{"text": f"t{i}", "id": i, "uid": f"x/{i}", "dataset": "x", "video": f"v{i // 2}", "start_sec": 0.0, "end_sec": 1.0} for i in range(4)]
    vec = np.ones((4, 8), np.float32)
    for flag in (False, True):
        with pytest.raises(ops.HipOnly):
            rag.RAGDatabase.from_arrays(vec, rows, device="cpu", wide_fanout=flag)
    rag.add_to_db(rows, vec, text_name="t", db_path=str(tmp_path))
    with pytest.raises(ops.HipOnly):
        rag.RAGDatabase(str(tmp_path), "t", device="cpu", wide_fanout=True)
    # which `order` a batch search passes on: the fan-out form by name only for 16 or more queries at 16 < top_k <= 32 with the flag set
    db = rag.RAGDatabase.__new__(rag.RAGDatabase)
    db.wide_fanout = False
    assert all(db._batch_order(nq, k) == "auto" for nq in (1, 15, 16, 256) for k in (12, 16, 17, 21, 32, 33))
    db.wide_fanout = True
    got = {(nq, k): db._batch_order(nq, k) for nq in (1, 15, 16, 256) for k in (12, 16, 17, 21, 32, 33)}
    assert {key for key, o in got.items() if o == "mfma"} == {(nq, k) for nq in (16, 256) for k in (17, 21, 32)} and set(got.values()) == {"auto", "mfma"}
    import inspect
    for fn in (rag.RAGDatabase.__init__, rag.RAGDatabase.from_arrays):
        assert inspect.signature(fn).parameters["wide_fanout"].default is False
