"""GPU suite of the wide fan-out lists: `ops.topk(order="mfma" | "mfma_stream" | "mfma_nowait")` at 17 <= k <= 32, bit for bit against mode f32mfma of the
UNCHANGED C oracle (oracle/topk_oracle.c: keep = max(16, k) candidates under the first score, "l2" scores those again in the chain-16 form and re-ranks them) in
every shape of the plan, and `RAGDatabase(wide_fanout=True)` on top of it.  Before the wide lists every fan-out call below returned MRAG_ENOTSUP.  The fixture
builders and the conditions that keep the fixtures meaningful live in tests/test_topk_wide_cpu.py (asserted there on the oracle alone)."""
import ctypes

import numpy as np
import pytest
import torch

from test_topk_wide_cpu import float64_rank_fixture, float64_rank_rule, near_duplicate_fixture, second_scoring_reaches_past_rank_16, unit

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _wide_plan(N, Q):
    """plan_mfma(n_rows, nq, list = 32) of topk.hip restated: (32-query tiles per workgroup TN, waves / 4 WN, workgroups along the table, row blocks per workgroup).
    The wide tile stops at TN = 4 (the 256-query workgroup's 32-deep lists exceed the CU's LDS) and the workgroup is always four waves."""
    blocks, qtiles = -(-N // 128), -(-Q // 32)
    widest = next(t for t in (4, 2, 1) if t <= qtiles)
    TN = widest
    for t in (1, 2, 4):
        if t <= widest and blocks * -(-qtiles // t) <= (512 if t == 1 else 256):
            TN = t
            break
    QB = 32 * TN
    stages = {4: 3, 2: 4, 1: 3}[TN]
    lds = stages * (128 + QB) * 128 + QB * (32 + 1 + 8 + 1) * 8 + 4 * 32 * 4
    assert lds <= 160 * 1024
    gy = -(-Q // QB)
    per_cu = max(1, min(2, (160 * 1024) // lds))
    parts = max(1, min(blocks, -(-256 * per_cu // gy)))
    bpp = -(-blocks // parts)
    return TN, 1, -(-blocks // bpp), bpp


# (N, Q, D, k) -> launch shape of order="mfma", streaming instantiation (TN, WN) and row blocks per workgroup of the wide plan
_SHAPES = {
    (3000, 130, 256, 21): ("one", (1, 1), 1),       # one launch, more than 128 queries
    (130, 16, 32, 32): ("one", (1, 1), 1),          # a table smaller than a row block, the fewest queries, a full list
    (5000, 20, 100, 17): ("one", (1, 1), 1),        # D no multiple of the 32-feature slab, the first depth past 16
    (9000, 300, 64, 32): ("one", (4, 1), 1),        # more than one query block
    (20000, 256, 64, 21): ("two", (4, 1), 2),       # two launches
    (66000, 64, 64, 32): ("stream", (2, 1), 3),     # streams by plan: warm lists and the shared threshold across a workgroup's row blocks
    (70001, 40, 128, 21): ("stream", (2, 1), 3),    # streams, ragged last block
    (12000, 300, 64, 21): ("one", (4, 1), 2),       # "mfma_stream": the 128-query tile with more than one row block per workgroup
}


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("N,Q,D,k", list(_SHAPES))
def test_wide_fanout_bit_exact(hip, metric, N, Q, D, k):
    """rows AND distances of the three fan-out orders against oracle mode f32mfma, both metrics, both filter orders, an exact tie, queries next to a row of the
    excluded video; dispatch counts in the vocabulary of test_gpu_kernels.  The wide plan can pick the streaming instantiations (TN, WN) = (1, 1), (2, 1) and
    (4, 1), each per metric (the eight-wave (2, 2) tile is not built at depth 32: it spilled the insertion chain to scratch).  Reached by:
      (1, 1): (3000, 130), (130, 16), (5000, 20) under "mfma_stream";   (2, 1): (66000, 64), (70001, 40) under both orders;
      (4, 1): (9000, 300) with one row block per workgroup, (20000, 256) and (12000, 300) with two, under "mfma_stream".
    The dense instantiations of depth 32 ("l2"): 32 queries per workgroup (130, 16), (5000, 20); the wider tiles by the larger batches; the finishing
    launch by (20000, 256)."""
    from motionrag_amd import ops
    from oracle import topk_ref
    from test_gpu_kernels import _FANOUT_COUNTS, _fanout_shape
    shape, inst, bpp = _SHAPES[(N, Q, D, k)]
    assert _fanout_shape(N, Q) == shape
    TN, WN, parts, got_bpp = _wide_plan(N, Q)
    assert (TN, WN) == inst and got_bpp == bpp, (TN, WN, parts, got_bpp)
    if N in (66000, 12000):
        assert got_bpp > 1                                                         # more than one row block per workgroup
    rng = np.random.default_rng(N + Q)
    db, q = unit(rng, N, D), unit(rng, Q, D)
    db[N // 2] = db[N // 3]                                                        # an exact tie: (distance, row) order decides
    group = (np.arange(N) // 2).astype(np.int32)
    excl = group[rng.integers(0, N, Q)].astype(np.int32)
    q[: Q // 4] = db[(2 * excl[: Q // 4])] + 0.01 * q[: Q // 4]                    # queries next to a row of the excluded video
    dbd, qd, gd, ed = (torch.from_numpy(a).to(DEV) for a in (db, q, group, excl))
    for post in (False, True):
        want_r, want_d = topk_ref.topk(db, q, k, metric, group, excl, mode="f32mfma", postfilter=post)
        for order in ("mfma", "mfma_stream") + (("mfma_nowait",) if shape == "one" else ()):
            with ops.dispatched() as d:
                rows, dist = ops.topk(dbd, qd, k, metric=metric, group=gd, exclude=ed, postfilter=post, order=order)
            assert d.counts == _FANOUT_COUNTS["stream" if order == "mfma_stream" else shape], (order, d.counts)
            np.testing.assert_array_equal(rows.cpu().numpy(), want_r, err_msg=f"{order} post={post}")
            np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32), err_msg=f"{order} post={post}")


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_fewer_rows_than_k(hip, metric):
    """a 20-row table at k = 21; a 40-row table whose pre-filter leaves 10 rows; the post-filter on the same table: tails are row -1 / +inf, survivors move up"""
    from motionrag_amd import ops
    from oracle import topk_ref
    rng = np.random.default_rng(20)
    db, q = rng.standard_normal((20, 32)).astype(np.float32), rng.standard_normal((16, 32)).astype(np.float32)
    want_r, want_d = topk_ref.topk(db, q, 21, metric, mode="f32mfma")
    assert (want_r[:, :20] >= 0).all() and (want_r[:, 20] == -1).all() and np.isposinf(want_d[:, 20]).all()
    for order in ("mfma", "mfma_stream", "mfma_nowait"):
        rows, dist = ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), 21, metric=metric, order=order)
        np.testing.assert_array_equal(rows.cpu().numpy(), want_r, err_msg=order)
        np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32), err_msg=order)
    db = rng.standard_normal((40, 32)).astype(np.float32)
    group = np.zeros(40, np.int32)
    group[rng.permutation(40)[:10]] = 1
    excl = np.zeros(16, np.int32)
    excl[15] = 7                                                                   # an id no row carries: that query keeps all of its 21
    dbd, qd, gd, ed = (torch.from_numpy(a).to(DEV) for a in (db, q, group, excl))
    for post in (False, True):
        want_r, want_d = topk_ref.topk(db, q, 21, metric, group, excl, mode="f32mfma", postfilter=post)
        n_found = (want_r >= 0).sum(axis=1)
        if not post:
            assert (n_found[:15] == 10).all() and n_found[15] == 21
        else:
            assert (n_found[:15] <= 10).all() and n_found[:15].min() < 10 and n_found[15] == 21      # the 21 nearest of 40 hold some of the 10 passing rows
        for order in ("mfma", "mfma_stream"):
            rows, dist = ops.topk(dbd, qd, 21, metric=metric, group=gd, exclude=ed, postfilter=post, order=order)
            rows, dist = rows.cpu().numpy(), dist.cpu().numpy()
            np.testing.assert_array_equal(rows, want_r, err_msg=f"{order} post={post}")
            np.testing.assert_array_equal(dist, want_d.astype(np.float32), err_msg=f"{order} post={post}")
            for i in range(16):                                                    # found rows first, in ascending distance; then the tail
                assert (rows[i, :n_found[i]] >= 0).all() and (rows[i, n_found[i]:] == -1).all() and np.isposinf(dist[i, n_found[i]:]).all()
                assert (group[rows[i, :n_found[i]]] != excl[i]).all()


@pytest.mark.parametrize("k", [17, 21, 32])
def test_second_scoring_past_rank_16(hip, k):
    """near-duplicate clusters on unnormalised 768-d rows: the first score orders a cluster as noise, so the list is right only when all max(16, k) selected
    candidates are scored again and re-ranked over the whole depth -- a second scoring that stopped at 16 fails here (the fixture's own condition is asserted:
    at least 8 clustered queries whose list differs from the expansion-only list at a rank >= 17; measured 31 - 32 of 32)"""
    from motionrag_amd import ops
    db, q = near_duplicate_fixture()
    want_r, want_d, moved, _ = second_scoring_reaches_past_rank_16(db, q, k)
    assert moved >= 8
    dbd, qd = torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV)
    for order in ("mfma", "mfma_stream"):
        rows, dist = ops.topk(dbd, qd, k, metric="l2", order=order)
        np.testing.assert_array_equal(rows.cpu().numpy(), want_r, err_msg=order)
        np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32), err_msg=order)


@pytest.mark.parametrize("k", [21, 32])
def test_mass_ties(hip, k):
    """600 identical rows: more scores at the bound than dense_select's compaction array holds (its per-wave path), and 600 equal-distance insertions into the
    streaming lists; the result is the lowest row numbers in order"""
    from motionrag_amd import ops
    from oracle import topk_ref
    rng = np.random.default_rng(600)
    db = unit(rng, 3000, 64)
    db[1000:1600] = db[1000]
    q = (db[1000][None, :] + 0.01 * unit(rng, 32, 64)).astype(np.float32)
    dbd, qd = torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV)
    for metric in ("l2", "dot"):
        want_r, want_d = topk_ref.topk(db, q, k, metric, mode="f32mfma")
        assert (want_r == np.arange(1000, 1000 + k)[None, :]).all()
        for order in ("mfma", "mfma_stream", "mfma_nowait"):
            rows, dist = ops.topk(dbd, qd, k, metric=metric, order=order)
            np.testing.assert_array_equal(rows.cpu().numpy(), want_r, err_msg=f"{metric} {order}")
            np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32), err_msg=f"{metric} {order}")


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_ranks_equal_float64(hip, metric):
    """the rule of test_gpu_kernels.py::test_topk_baseline_size_ranks_equal_float64_oracle at k = 21: 10 000 x 768 unit rows, 64 queries, order="mfma"; a rank
    is compared when both neighbouring float64 gaps exceed 2 x 1e-6 x max(|d|, 1); compared ranks are equal, every distance within 2e-6, more than 98 % of
    the ranks compared (the oracle's own f32mfma mode: 99.4 % compared, |d - d64| <= 2.3e-7 -- tests/test_topk_wide_cpu.py)"""
    from motionrag_amd import ops
    from oracle import topk_ref
    db, q, group, excl = float64_rank_fixture()
    rows, dist = ops.topk(torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV), 21, metric=metric, group=torch.from_numpy(group).to(DEV),
                          exclude=torch.from_numpy(excl).to(DEV), order="mfma")
    rows, dist = rows.cpu().numpy(), dist.cpu().numpy()
    want_r, want_d = topk_ref.topk(db, q, 22, metric, group, excl, mode="f64")        # one more: the gap below rank 21 matters too
    safe, wr, wd = float64_rank_rule(want_r, want_d, 21)
    print(f"{metric}: {100 * safe.mean():.2f} % of the ranks compared, max |d - d64| = {np.abs(dist - wd).max():.3e}")
    assert safe.mean() > 0.98
    assert np.array_equal(rows[safe], wr[safe])
    np.testing.assert_allclose(dist, wd, rtol=0, atol=2e-6)
    assert not np.any(rows == excl[:, None])


def test_determinism_capture_and_shared_workspace(hip):
    """ONE workspace (sized by mrag_topk_workspace_bytes_k) serves, on one stream: k = 12, then k = 21 twice (bit-equal), then a captured graph of the k = 21
    call replayed twice (equal to the eager result), then k = 12 again (the bits of the first k = 12 call) -- in the dense and in the streaming form: the
    wide calls leave the counters and the workspace as every other call expects them"""
    from motionrag_amd import _lib, ops
    from oracle import topk_ref
    L = _lib.lib()
    rng = np.random.default_rng(6)
    N, Q, D = 6000, 48, 96
    db, q = rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((Q, D)).astype(np.float32)
    dbd, qd = torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV)
    want = {k: topk_ref.topk(db, q, k, "l2", mode="f32mfma") for k in (12, 21)}
    ws = torch.zeros(L.mrag_topk_workspace_bytes_k(N, Q, 21), dtype=torch.uint8, device=DEV)
    assert ws.numel() >= L.mrag_topk_workspace_bytes(N, Q)
    out = {k: (torch.empty(Q, k, dtype=torch.int32, device=DEV), torch.empty(Q, k, dtype=torch.float32, device=DEV)) for k in (12, 21)}
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731

    def call(k, order):
        rc = L.mrag_topk_f32(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(dbd), None, N, D, p(qd), None, Q, k, 0, p(out[k][0]), p(out[k][1]),
                             p(ws), ws.numel(), 0, ops.TOPK_ORDER[order])
        assert rc == 0, (k, order, rc)

    def result(k):
        torch.cuda.synchronize()
        r, d = out[k][0].cpu().numpy().copy(), out[k][1].cpu().numpy().copy()
        out[k][0].fill_(-7); out[k][1].fill_(-7.0)
        return r, d

    def check(got, k, what):
        np.testing.assert_array_equal(got[0], want[k][0], err_msg=what)
        np.testing.assert_array_equal(got[1], want[k][1].astype(np.float32), err_msg=what)

    for order in ("mfma", "mfma_stream"):
        with ops.dispatched() as d:
            call(12, order)
        assert d.counts == ({"TOPK_DENSE": 1} if order == "mfma" else {"TOPK_MFMA": 1, "TOPK_MERGE": 1}), d.counts
        check(result(12), 12, f"{order}: k = 12 before")
        with ops.dispatched() as d:
            call(21, order)
        assert d.counts == ({"TOPK_DENSE": 1} if order == "mfma" else {"TOPK_MFMA": 1, "TOPK_MERGE": 1}), d.counts
        first = result(21)
        check(first, 21, f"{order}: k = 21")
        call(21, order)
        again = result(21)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call(21, order)
        for it in range(2):
            graph.replay()
            check(result(21), 21, f"{order}: replay {it}")
        call(12, order)
        check(result(12), 12, f"{order}: k = 12 after")


def test_refusals_and_the_automatic_order(hip):
    from motionrag_amd import _lib, ops
    from oracle import topk_ref
    rng = np.random.default_rng(7)
    db, q = unit(rng, 3000, 64), unit(rng, 64, 64)
    dbd, qd = torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV)
    for order in ("mfma", "mfma_stream", "mfma_nowait"):
        with pytest.raises(_lib.HipError, match="MRAG_ENOTSUP"):
            ops.topk(dbd, qd, 33, order=order)                                    # k > 32
        with pytest.raises(_lib.HipError, match="MRAG_ENOTSUP"):
            ops.topk(dbd, qd[:15].contiguous(), 21, order=order)                  # fewer than 16 queries
    want_r, want_d = topk_ref.topk(db, q, 21, "l2", mode="f32chain")
    with ops.dispatched() as d:
        rows, dist = ops.topk(dbd, qd, 21, order="auto")                          # the automatic order at k = 21 is what it was: the scan form
    assert d.counts == {"TOPK_SCAN": 1, "TOPK_MERGE": 1}, d.counts
    np.testing.assert_array_equal(rows.cpu().numpy(), want_r)
    np.testing.assert_array_equal(dist.cpu().numpy(), want_d.astype(np.float32))


def _database_fixture():
    from test_gpu_rag_text_image import _table, _unit
    rng = np.random.default_rng(21)
    N, Q = 4000, 256
    text, img, meta, group = _table(rng, N, 768, 1024)
    near = rng.integers(0, N, Q)
    q_text = _unit(rng, Q, 768)
    q_text[:128] = text[near[:128]] + 0.01 * q_text[:128]
    q_img = img[near] + 0.05 * _unit(rng, Q, 1024)
    where = [f'video != "{meta[int(i)]["video"]}"' for i in near]
    where[200] = None
    excl = group[near].copy()
    excl[200] = -1
    return text, img, meta, group, q_text, q_img, where, excl


@pytest.mark.parametrize("prefilter", [None, True])
def test_database_with_the_flag(hip, prefilter):
    """RAGDatabase(wide_fanout=True), set up as test_gpu_rag_text_image.py::test_text_image_search_equals_the_composition (4 000 rows, 256 queries, (21, 9)): the
    batch equals stage-1 oracle f32mfma -> gathered oracle in both filter orders, without a scan launch and with exactly one re-rank launch;
    text_search_batch(k = 21) equals oracle f32mfma"""
    from motionrag_amd import ops, rag
    from oracle import topk_ref
    from test_gpu_rag_text_image import _compose, _expected_results
    text, img, meta, group, q_text, q_img, where, excl = _database_fixture()
    select = ["video", "start_sec", "end_sec"]
    db = rag.RAGDatabase.from_arrays(text, meta, device=DEV, image_vectors=img, wide_fanout=True)
    assert db.wide_fanout is True
    post = prefilter is None
    c, cd = topk_ref.topk(text, q_text, 21, "l2", group, excl, mode="f32mfma", postfilter=post)
    short = int((c < 0).any(axis=1).sum())
    assert (short >= 32) if post else (short == 0)
    wr, _, wd = _compose(img, q_img, c, 9, "l2")
    with ops.dispatched() as d:
        got = db.text_image_search_batch(q_text, q_img, (21, 9), where=where, select=select, prefilter=prefilter)
    assert got == _expected_results(meta, wr, wd, select)
    assert "TOPK_SCAN" not in d.counts and d.counts == {"TOPK_DENSE": 1, "TOPK_RERANK": 1}, d.counts
    with ops.dispatched() as d:
        got_text = db.text_search_batch(q_text, 21, where=where, select=select, prefilter=prefilter)
    assert got_text == _expected_results(meta, c, cd, select) and d.counts == {"TOPK_DENSE": 1}, d.counts


def test_database_without_the_flag_and_single_queries(hip):
    """flag off: counts and results are the scan form's, as before; a single-query call ignores the flag; the flag may be set on a live database"""
    from motionrag_amd import ops, rag
    from oracle import topk_ref
    from test_gpu_rag_text_image import _compose, _expected_results
    text, img, meta, group, q_text, q_img, where, excl = _database_fixture()
    select = ["video", "start_sec", "end_sec"]
    db = rag.RAGDatabase.from_arrays(text, meta, device=DEV, image_vectors=img)
    assert db.wide_fanout is False
    c, _ = topk_ref.topk(text, q_text, 21, "l2", group, excl, mode="f32chain", postfilter=True)
    wr, _, wd = _compose(img, q_img, c, 9, "l2")
    want = _expected_results(meta, wr, wd, select)
    with ops.dispatched() as d:
        got = db.text_image_search_batch(q_text, q_img, (21, 9), where=where, select=select)
    assert got == want and d.counts == {"TOPK_SCAN": 1, "TOPK_MERGE": 1, "TOPK_RERANK": 1}, d.counts
    singles = {}
    for flag in (False, True):
        db.wide_fanout = flag                                                      # an attribute: may be set later
        with ops.dispatched() as d:
            singles[flag] = [db.text_image_search(q_text[i], q_img[i], top_k=(21, 9), where=where[i], select=select) for i in (0, 5, 200)]
        assert "TOPK_DENSE" not in d.counts and "TOPK_MFMA" not in d.counts and d.counts.get("TOPK_RERANK") == 3, d.counts
        assert singles[flag] == [want[i] for i in (0, 5, 200)]
        with ops.dispatched() as d:
            db.text_search_batch(q_text[:15], 21, where=where[:15], select=select)   # fewer than 16 queries: the scan form either way
        assert "TOPK_DENSE" not in d.counts and "TOPK_MFMA" not in d.counts, d.counts
    # flag on, k <= 16 or k > 32: the automatic order, as without the flag
    with ops.dispatched() as d:
        db.text_search_batch(q_text, 12, where=where, select=select)
    assert d.counts == {"TOPK_DENSE": 1}, d.counts
    with ops.dispatched() as d:
        db.text_search_batch(q_text, 33, where=where, select=select)
    assert d.counts == {"TOPK_SCAN": 1, "TOPK_MERGE": 1}, d.counts
