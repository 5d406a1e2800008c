"""GPU suite of the text-then-image retrieval (`ref_video_type: rag_text_image`, src/data/rag.py:82-130, src/data/datamodule.py:239-245): the gathered
re-rank kernel (mrag_topk_rerank_f32) bit for bit against the COMPOSED oracle -- oracle/topk_oracle.c run on each query's own gathered rows, in list
order --, its ranks against float64, and the database methods built on it.  LanceDB is not installed, so the two-stage semantics are the cited ones
(module docstring of motionrag_amd/rag.py), not an executed reference."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _compose(img, q_img, cand, k, metric, mode="f32chain"):
    """the expected re-rank: query q's present candidates (entries inside [0, N)), in list order, are a table of their own that the unchanged oracle
    searches; its row numbers are indices into that table, i.e. ordered like the positions in the list -> (distance asc, position asc).
    Returns rows / positions int32 [Q, k] (-1 = missing) and distances [Q, k] (float64 holding the fp32 value, or float64 in mode 'f64'; +inf = missing)."""
    from oracle import topk_ref
    Q, N = cand.shape[0], img.shape[0]
    rows, pos, dist = np.full((Q, k), -1, np.int32), np.full((Q, k), -1, np.int32), np.full((Q, k), np.inf, np.float64)
    for q in range(Q):
        present = np.flatnonzero((cand[q] >= 0) & (cand[q] < N))
        if len(present) == 0:
            continue
        kk = min(k, len(present))
        sub = img[cand[q, present]]
        if mode == "f64":
            r, d = topk_ref.topk_numpy(sub, q_img[q:q + 1], kk, metric)
        else:
            r, d = topk_ref.topk(sub, q_img[q:q + 1], kk, metric, mode=mode)
        pos[q, :kk] = present[r[0]]
        rows[q, :kk] = cand[q, pos[q, :kk]]
        dist[q, :kk] = d[0]
    return rows, pos, dist


def _rerank(img_d, q_img, cand, k, metric):
    from motionrag_amd import ops
    rows, pos, dist = ops.topk_rerank(img_d, torch.from_numpy(q_img).to(DEV), torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).to(DEV), k, metric=metric)
    return rows.cpu().numpy(), pos.cpu().numpy(), dist.cpu().numpy()


def _assert_bit_exact(got, want, what):
    (gr, gp, gd), (wr, wp, wd) = got, want
    assert gr.dtype == np.int32 and gp.dtype == np.int32 and gd.dtype == np.float32
    assert np.array_equal(gr, wr), what
    assert np.array_equal(gp, wp), what
    assert np.array_equal(gd, wd.astype(np.float32)), what


N_TAB = 3000
_SHAPES = [(nq, dim, n_cand, kind) for nq in (3,) for dim in (64, 100, 768, 1024) for n_cand in (1, 16, 21, 64) for kind in ("one", "nine", "all")]
_SHAPES += [(nq, dim, n_cand, kind) for nq in (1, 256, 1000) for (dim, n_cand, kind) in ((768, 21, "nine"), (1024, 64, "all"), (100, 16, "one"), (64, 1, "one"))]


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_rerank_bit_exact_against_the_composed_oracle(hip, metric):
    """rows, positions and distances equal the composition for every (n_queries, dim, n_cand, k) of the grid on unnormalised N(0, 1) data (bit-exactness
    needs no gap condition): dim in {64, 100, 768, 1 024}, n_cand in {1, 16, 21, 64}, k in {1, 9, n_cand}, n_queries in {1, 3, 256, 1 000}"""
    for dim in (64, 100, 768, 1024):
        rng = np.random.default_rng(1000 + dim)
        img = rng.standard_normal((N_TAB, dim)).astype(np.float32)
        img_d = torch.from_numpy(img).to(DEV)
        for nq, d, n_cand, kind in _SHAPES:
            if d != dim:
                continue
            k = {"one": 1, "nine": min(9, n_cand), "all": n_cand}[kind]
            q_img = rng.standard_normal((nq, dim)).astype(np.float32)
            cand = rng.integers(0, N_TAB, (nq, n_cand)).astype(np.int32)
            _assert_bit_exact(_rerank(img_d, q_img, cand, k, metric), _compose(img, q_img, cand, k, metric), (metric, nq, dim, n_cand, k))


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_rerank_holes_duplicates_absent_lists_and_ties(hip, metric):
    from motionrag_amd import ops
    rng = np.random.default_rng(7)
    N, dim, n_cand = 500, 768, 21
    img = rng.standard_normal((N, dim)).astype(np.float32)
    img[401] = img[17]                                                  # two identical table rows: equal distances to every query
    img[402] = img[17]
    img_d = torch.from_numpy(img).to(DEV)
    q_img = rng.standard_normal((8, dim)).astype(np.float32)
    cand = np.stack([rng.permutation(np.arange(18, 400))[:n_cand] for _ in range(8)]).astype(np.int32)
    cand[0, 15:] = -1                                                   # the tail of a short stage-1 list
    cand[1, [0, 3, 20]] = -1                                            # holes anywhere
    cand[1, 7], cand[1, 9] = N, 2 ** 30                                 # outside [0, n_rows): absent
    cand[2, 5] = cand[2, 11]                                            # the same row twice: each entry counts
    cand[3, :] = -1                                                     # every entry absent
    cand[4, :] = cand[4, 0]                                             # one row, 21 times: 21 equal distances, order = position
    cand[5, 2], cand[5, 9], cand[5, 14] = 402, 17, 401                  # identical rows in one list: position order 2 < 9 < 14 although row 402 > 17
    cand[6, 1:] = -1                                                    # a single present entry
    for k in (1, 9, n_cand):
        got = _rerank(img_d, q_img, cand, k, metric)
        _assert_bit_exact(got, _compose(img, q_img, cand, k, metric), (metric, k))
        gr, gp, gd = got
        assert np.all(gr[3] == -1) and np.all(gp[3] == -1) and np.all(np.isposinf(gd[3]))
        assert gp[4].tolist() == list(range(k)) and np.all(gr[4] == cand[4, 0]) and np.all(gd[4] == gd[4, 0])
        assert gr[6, 0] == cand[6, 0] and np.all(gr[6, 1:] == -1)
    gr, gp, gd = _rerank(img_d, q_img, cand, n_cand, metric)
    assert np.count_nonzero(gr[0] >= 0) == 15 and np.count_nonzero(gr[1] >= 0) == 16
    at = [int(np.flatnonzero(gp[5] == p)[0]) for p in (2, 9, 14)]
    assert at[1] == at[0] + 1 and at[2] == at[0] + 2 and gr[5, at].tolist() == [402, 17, 401] and gd[5, at[0]] == gd[5, at[1]] == gd[5, at[2]]
    both = np.sort(gp[2][gr[2] == cand[2, 5]])
    assert both.tolist() == [5, 11]
    # out = caller's buffers, out_pos optional at the C ABI
    out = (torch.empty(8, 9, dtype=torch.int32, device=DEV), torch.empty(8, 9, dtype=torch.int32, device=DEV), torch.empty(8, 9, dtype=torch.float32, device=DEV))
    r2, p2, d2 = ops.topk_rerank(img_d, torch.from_numpy(q_img).to(DEV), torch.from_numpy(cand).to(DEV), 9, metric=metric, out=out)
    assert r2 is out[0] and np.array_equal(r2.cpu().numpy(), gr[:, :9]) and np.array_equal(p2.cpu().numpy(), gp[:, :9]) and np.array_equal(d2.cpu().numpy(), gd[:, :9])
    from motionrag_amd import _lib
    import ctypes
    r3, d3 = torch.full((8, 9), 7, dtype=torch.int32, device=DEV), torch.empty(8, 9, dtype=torch.float32, device=DEV)
    qd, cd = torch.from_numpy(q_img).to(DEV), torch.from_numpy(cand).to(DEV)
    rc = _lib.lib().mrag_topk_rerank_f32(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.c_void_p(img_d.data_ptr()), N, dim, ctypes.c_void_p(qd.data_ptr()), 8,
                                         ctypes.c_void_p(cd.data_ptr()), n_cand, 9, {"l2": 0, "dot": 1}[metric], ctypes.c_void_p(r3.data_ptr()), None, ctypes.c_void_p(d3.data_ptr()))
    assert rc == 0 and np.array_equal(r3.cpu().numpy(), gr[:, :9]) and np.array_equal(d3.cpu().numpy(), gd[:, :9])
    with pytest.raises(ValueError):
        ops.topk_rerank(img_d, qd, cd, 22, metric=metric)              # k > n_cand


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_rerank_distances_do_not_depend_on_the_call_shape(hip, metric):
    """the same (query, row) pairs get, bit for bit, the distances `ops.topk(order="chain16")` gives them in a scan of the whole table"""
    from motionrag_amd import ops
    for dim, nq in ((768, 8), (100, 256), (1024, 40)):
        rng = np.random.default_rng(dim)
        tab = rng.standard_normal((N_TAB, dim)).astype(np.float32)
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        tab_d, q_d = torch.from_numpy(tab).to(DEV), torch.from_numpy(q).to(DEV)
        rows1, dist1 = ops.topk(tab_d, q_d, 21, metric=metric, order="chain16")
        rows2, pos2, dist2 = ops.topk_rerank(tab_d, q_d, rows1, 21, metric=metric)          # stage-1 rows straight from its output buffer
        assert torch.equal(dist2, dist1) and torch.equal(rows2, rows1)
        assert torch.equal(pos2, torch.arange(21, dtype=torch.int32, device=DEV).expand(nq, 21))
        perm = torch.from_numpy(rng.permutation(21)).to(DEV)
        rows3, pos3, dist3 = ops.topk_rerank(tab_d, q_d, rows1[:, perm].contiguous(), 21, metric=metric)   # the list in another order: same bits per pair
        assert torch.equal(dist3, dist1) and torch.equal(rows3, rows1)


def test_rerank_ranks_equal_float64_on_stage1_lists(hip):
    """The rule of tests/test_gpu_kernels.py::test_topk_baseline_size_ranks_equal_float64_oracle, per rank: 10 000 x 768 unit-norm text column, unit-norm 768-d
    and 1 024-d image columns, 256 queries (the first 64 are `row + 0.01 x noise`), candidates = the 21-row stage-1 lists, k = 9.  k + 1 ranks are taken from
    the float64 composition so that the gap below the last returned rank counts; a rank is compared when both neighbouring float64 gaps exceed
    2 x 1e-6 x max(|d|, 1); compared ranks must be equal, every distance within 2e-6 absolute, and more than 98 % of the ranks compared (the oracle's own
    fp32 mode compares 99.8 % or more of them on this data and differs from float64 by at most 3.3e-7)."""
    from oracle import topk_ref
    rng = np.random.default_rng(1)
    N, Q, K0, K = 10000, 256, 21, 9
    text, q_text = _unit(rng, N, 768), _unit(rng, Q, 768)
    near = rng.integers(0, N, Q)
    q_text[:64] = text[near[:64]] + 0.01 * q_text[:64]
    cand, _ = topk_ref.topk(text, q_text, K0, "l2", mode="f32chain")
    for dim in (768, 1024):
        img, q_img = _unit(rng, N, dim), _unit(rng, Q, dim)
        q_img[:64] = img[near[:64]] + 0.01 * q_img[:64]
        img_d = torch.from_numpy(img).to(DEV)
        for metric in ("l2", "dot"):
            rows, pos, dist = _rerank(img_d, q_img, cand, K, metric)
            want_r, want_p, want_d = _compose(img, q_img, cand, K + 1, metric, mode="f64")
            gap = np.diff(want_d, axis=1)
            tol = 1e-6 * np.maximum(np.abs(want_d[:, :K]), 1.0)
            safe = np.ones((Q, K), bool)
            safe &= gap > 2 * tol
            safe[:, 1:] &= gap[:, :-1] > 2 * tol[:, 1:]
            print(f"dim {dim} {metric}: {100 * safe.mean():.2f} % of the ranks compared, max |d - d64| = {np.abs(dist - want_d[:, :K]).max():.3e}")
            assert safe.mean() > 0.98
            assert np.array_equal(rows[safe], want_r[:, :K][safe]) and np.array_equal(pos[safe], want_p[:, :K][safe])
            np.testing.assert_allclose(dist, want_d[:, :K], rtol=0, atol=2e-6)


def _table(rng, n, d_text, d_img, per_video=5):
    text, img = _unit(rng, n, d_text), _unit(rng, n, d_img)
    rows = [{"text": f"caption {i}", "id": i, "uid": f"x/{i}", "dataset": "x", "video": f"video_{i // per_video:05d}.mp4", "start_sec": float(i % per_video),
             "end_sec": float(i % per_video + 1)} for i in range(n)]
    return text, img, rows, (np.arange(n) // per_video).astype(np.int32)


def _expected_results(rows_meta, rows, dist, select):
    out = []
    for r, d in zip(rows, dist):
        out.append([{**{c: rows_meta[int(i)][c] for c in select}, "_distance": float(np.float32(x))} for i, x in zip(r, d) if i >= 0])
    return out


def test_image_search_over_the_whole_table(hip):
    from motionrag_amd import rag
    from oracle import topk_ref
    rng = np.random.default_rng(11)
    N, Q = 4000, 64
    text, img, meta, group = _table(rng, N, 128, 256)
    near = rng.integers(0, N, Q)
    q_img = img[near] + 0.01 * _unit(rng, Q, 256)
    where = [f'video != "{meta[int(i)]["video"]}"' for i in near]
    select = ["video", "start_sec", "end_sec"]
    for image_metric in ("l2", "dot"):
        for prefilter in (False, True):
            db = rag.RAGDatabase.from_arrays(text, meta, device=DEV, image_vectors=img, image_metric=image_metric, prefilter=prefilter)
            assert db.image_vectors is None                                                    # uploaded by the first search that needs it
            for i in (0, 1, 2, 63):
                wr, wd = topk_ref.topk(img, q_img[i:i + 1], 10, image_metric, mode="f32chain")
                assert db.image_search(q_img[i], top_k=10, select=select) == _expected_results(meta, wr, wd, select)[0]
                assert db.vector_search(q_img[i], vector_column_name="image_embedding", top_k=10, select=select) == _expected_results(meta, wr, wd, select)[0]
                wr, wd = topk_ref.topk(img, q_img[i:i + 1], 10, image_metric, group, group[near[i:i + 1]], mode="f32chain", postfilter=not prefilter)
                got = db.image_search(q_img[i], top_k=10, where=where[i], select=select)
                assert got == _expected_results(meta, wr, wd, select)[0]
                assert len(got) == (10 if prefilter else 9)                                        # post-filter: the query's own row was the nearest of the 10 and leaves
            assert db.image_vectors is not None and tuple(db.image_vectors.shape) == (N, 256)
            wr, wd = topk_ref.topk(img, q_img, 10, image_metric, group, group[near], mode="f32mfma", postfilter=not prefilter)     # >= 16 queries, k <= 16: the fan-out form
            assert db.image_search_batch(q_img, 10, where=where, select=select) == _expected_results(meta, wr, wd, select)
            full = db.image_search(q_img[0], top_k=3)                                           # select=None: the schema columns + _distance
            assert list(full[0]) == list(rag.SCHEMA) + ["_distance"]
            with pytest.raises(NotImplementedError):
                db.image_search(q_img[0], table=object())
    plain = rag.RAGDatabase.from_arrays(text, meta, device=DEV)
    for call in (lambda: plain.image_search(q_img[0]), lambda: plain.text_image_search(text[0], q_img[0]),
                 lambda: plain.text_image_search_batch(text[:2], q_img[:2]), lambda: plain.vector_search(q_img[0], vector_column_name="image_embedding")):
        with pytest.raises(ValueError, match="image_vectors.npy"):
            call()
    with pytest.raises(ValueError):
        plain.vector_search(text[0], vector_column_name="audio_embedding")


def test_text_image_search_equals_the_composition(hip):
    """single query == row i of the batch == stage-1 oracle -> gathered oracle, with the post-filter (short stage-1 lists: groups of 5 rows per video,
    queries at `row + 0.01 x noise`) and with prefilter=True; one TOPK_RERANK launch per batch call beside the text search's own kernels"""
    from motionrag_amd import ops, rag
    from oracle import topk_ref
    rng = np.random.default_rng(21)
    N, Q, K0, K1 = 4000, 256, 21, 9
    text, img, meta, group = _table(rng, N, 768, 1024)
    near = rng.integers(0, N, Q)
    q_text = _unit(rng, Q, 768)
    q_text[:128] = text[near[:128]] + 0.01 * q_text[:128]
    q_img = img[near] + 0.05 * _unit(rng, Q, 1024)
    where = [f'video != "{meta[int(i)]["video"]}"' for i in near]
    where[200] = None                                                                          # a batch may mix filtered and unfiltered queries
    excl = group[near].copy()
    excl[200] = -1
    select = ["video", "start_sec", "end_sec"]
    for metric, image_metric in (("l2", "l2"), ("dot", "l2"), ("l2", "dot")):
        db = rag.RAGDatabase.from_arrays(text, meta, device=DEV, metric=metric, image_vectors=img, image_metric=image_metric)
        for prefilter in (None, True):
            post = prefilter is None
            c, _ = topk_ref.topk(text, q_text, K0, metric, group, excl, mode="f32chain", postfilter=post)       # k = 21 > 16: the scan form
            short = int((c < 0).any(axis=1).sum())
            assert (short >= 32) if post else (short == 0)                                     # the post-filtered lists of near-duplicate queries lose their own video's clips
            wr, _, wd = _compose(img, q_img, c, K1, image_metric)
            want = _expected_results(meta, wr, wd, select)
            with ops.dispatched() as d_text:
                db.text_search_batch(q_text, K0, where=where, select=select, prefilter=prefilter)
            with ops.dispatched() as d_both:
                got = db.text_image_search_batch(q_text, q_img, (K0, K1), where=where, select=select, prefilter=prefilter)
            assert got == want
            assert "TOPK_RERANK" not in d_text.counts and d_both.counts == {**d_text.counts, "TOPK_RERANK": 1}
            assert all(set(r) == {"video", "start_sec", "end_sec", "_distance"} for res in got for r in res)
            for i in (0, 1, 5, 127, 200, 255):
                with ops.dispatched() as d_one:
                    one = db.text_image_search(q_text[i], q_img[i], top_k=(K0, K1), where=where[i], select=select, prefilter=prefilter)
                assert one == got[i] and d_one.counts.get("TOPK_RERANK") == 1
            with ops.dispatched() as d_text1:
                db.text_search(q_text[3], top_k=K0, where=where[3], prefilter=prefilter)
            with ops.dispatched() as d_one:
                db.text_image_search(q_text[3], q_img[3], top_k=(K0, K1), where=where[3], prefilter=prefilter)
            assert d_one.counts == {**d_text1.counts, "TOPK_RERANK": 1}
        # a stage 1 of k <= 16 runs the fan-out form for a batch: the composition starts from the oracle's "f32mfma" mode
        c, _ = topk_ref.topk(text, q_text, 12, metric, group, excl, mode="f32mfma", postfilter=True)
        wr, _, wd = _compose(img, q_img, c, 5, image_metric)
        assert db.text_image_search_batch(q_text, q_img, (12, 5), where=where, select=select) == _expected_results(meta, wr, wd, select)
        # fewer than top_k[1] rows come back when stage 1 returned fewer
        lens = [len(r) for r in db.text_image_search_batch(q_text, q_img, (5, 5), where=where, select=select)]
        assert min(lens) < 5 and max(lens) == 5
        full = db.text_image_search(q_text[0], q_img[0], top_k=(6, 2))
        assert list(full[0]) == list(rag.SCHEMA) + ["_distance"]
        for bad in ((65, 9), (9, 10), (9, 0), 9):
            with pytest.raises(ValueError):
                db.text_image_search(q_text[0], q_img[0], top_k=bad)
        with pytest.raises(NotImplementedError):
            db.text_image_search(q_text[0], q_img[0], table=object())


def test_attach_ref_videos_rag_text_image_fan_out(hip):
    """BASELINE config #1's synthetic table (10 000 captions, hash embedder) + a seeded image column, 1 000 annotations, ref_video_num = 9"""
    from motionrag_amd import rag
    from oracle import topk_ref
    N, A, n = 10000, 1000, 9
    caps = rag.synthetic_captions(N)
    embed = rag.hash_embedder(768)
    meta = rag.prepare_annotations(caps, text_name="motion_caption")
    text = np.stack([embed(r["text"]) for r in meta])
    rng = np.random.default_rng(3)
    img = _unit(rng, N, 1024)
    db = rag.RAGDatabase.from_arrays(text, meta, device=DEV, image_vectors=img)
    picks = np.sort(rng.permutation(N)[:A])
    q_img = (img[picks] + 0.05 * _unit(rng, A, 1024)).astype(np.float32)
    annos = [{**caps[int(i)], "text_embedding": text[i], "image_embedding": q_img[j]} for j, i in enumerate(picks)]
    group = np.arange(N, dtype=np.int32)                                                       # every synthetic caption is its own video
    out = rag.attach_ref_videos([dict(a) for a in annos], db, n, ref_video_type="rag_text_image")
    c, _ = topk_ref.topk(text, text[picks], 2 * n + 3, "l2", group, picks.astype(np.int32), mode="f32chain", postfilter=True)
    wr, _, wd = _compose(img, q_img, c, n, "l2")
    want = _expected_results(meta, wr, wd, ["video", "start_sec", "end_sec"])
    for a, w in zip(out, want):
        assert len(a["ref_videos"]) <= n and a["ref_videos"] == w
        assert all(list(r) == ["video", "start_sec", "end_sec", "_distance"] and r["video"] != a["video"] for r in a["ref_videos"])
    # `rag_text` is what it was: the chunks of 256 through text_search_batch
    out_t = rag.attach_ref_videos([dict(a) for a in annos], db, n, ref_video_type="rag_text")
    for i in range(0, A, 256):
        part = annos[i:i + 256]
        res = db.text_search_batch(np.stack([a["text_embedding"] for a in part]), top_k=n + 3, where=[f'video != "{a["video"]}"' for a in part],
                                   select=["video", "start_sec", "end_sec"])
        assert [a["ref_videos"] for a in out_t[i:i + 256]] == res
    assert rag.attach_ref_videos([dict(a) for a in annos[:3]], db, 1, ref_video_type="gt")[2]["ref_videos"][0]["video"] == annos[2]["video"]
