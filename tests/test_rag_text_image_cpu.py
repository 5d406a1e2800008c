"""CPU suite of the text-then-image retrieval (`ref_video_type: rag_text_image`): the new C-ABI symbol and dispatch id, the image column's
table I/O (create / append / reopen / partial-column refusal / interrupted append / tables without the column), `ops.topk_rerank`'s refusal of CPU
tensors and the host-only `ref_video_type`s of `attach_ref_videos`.  No compute calls: the kernel is exercised by tests/test_gpu_rag_text_image.py."""
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the dispatch ids as they stood before MRAG_K_TOPK_RERANK was appended: none of them may move
OLD_DISPATCH_NAMES = [
    "GEMM_W4", "GEMM_W4_QKNORM_ROPE", "GEMM_W4_GEGLU", "GEMM_256x256", "GEMM_256x320", "GEMM_256x128", "GEMM_128x128", "GEMM_STREAMK_TAIL", "GEMM_N320K320", "GEMM_192x256",
    "CONV3_W4", "CONV3_256x256", "CONV3_256x320", "CONV3_256x128", "CONV3_128x128", "CONV3_192x256",
    "CONVT_W4", "CONVT_256x256", "CONVT_256x320", "CONVT_128x128", "CONVT_192x256", "CONVT_256x128",
    "ATTN16", "ATTN16_KSPLIT", "ATTN_FLASH", "ATTN_FLASH_KSPLIT", "ATTN_COMBINE", "ATTN_TINY", "ATTN_SMALL", "ATTN_FP8", "IP_ATTN_FOLDED",
    "LAYERNORM", "LAYERNORM_ROWS", "QKNORM_ROPE", "GN_STATS", "GN_FOLD", "GN_APPLY", "GN_APPLY_MOD", "LAYERNORM_STREAM", "GN_STATS_FOLD",
    "TOPK_SCAN", "TOPK_SCAN_FUSED_MERGE", "TOPK_MERGE", "TOPK_MFMA", "GEMM_W4_TAIL_RECT", "GEMM_W4_BATCHED_W", "GEMM_SKINNY_LNA", "TOPK_DENSE", "TOPK_DENSE_FINISH", "GEMM_SKINNY"]


def _rows(n, start=0):
    return [{"text": f"t{i}", "id": i, "uid": f"x/{i}", "dataset": "x", "video": f"v{i // 2}", "start_sec": 0.0, "end_sec": 1.0} for i in range(start, start + n)]


def test_rerank_symbol_abi_version_and_dispatch_id():
    import ctypes
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    assert re.search(r"\bint\s+mrag_topk_rerank_f32\s*\(", hdr) and "mrag_topk_rerank_f32" in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 11
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mrag_topk_rerank_f32")
    L = _lib.lib()
    assert L.mrag_abi_version() == 11
    assert len(L.mrag_topk_rerank_f32.argtypes) == 13
    n = L.mrag_dispatch_counts(None, 0)
    names = [L.mrag_dispatch_name(i).decode() for i in range(n)]
    assert names[:len(OLD_DISPATCH_NAMES)] == OLD_DISPATCH_NAMES                # no existing id moved
    assert names[len(OLD_DISPATCH_NAMES):] == ["TOPK_RERANK"]                   # appended directly in front of MRAG_K_COUNT
    enum = re.search(r"enum mrag_kernel_id \{(.*?)\};", hdr, re.S).group(1)
    ids = re.findall(r"\b(MRAG_K_[A-Za-z0-9_]+)\b", re.sub(r"/\*.*?\*/", "", enum, flags=re.S))
    assert ids[-2:] == ["MRAG_K_TOPK_RERANK", "MRAG_K_COUNT"] and [i[len("MRAG_K_"):] for i in ids[:-1]] == names
    # argument checks that need no GPU: they return before anything is launched
    one = ctypes.c_void_p(16)
    assert L.mrag_topk_rerank_f32(None, None, 4, 8, one, 1, one, 2, 1, 0, one, None, one) == -1                # null db
    assert L.mrag_topk_rerank_f32(None, one, 4, 8, one, 1, one, 2, 3, 0, one, None, one) == -1                 # k > n_cand
    assert L.mrag_topk_rerank_f32(None, one, 4, 8, one, 1, one, 65, 3, 0, one, None, one) == -2                # n_cand > 64
    assert L.mrag_topk_rerank_f32(None, one, 4, 6, one, 1, one, 2, 1, 0, one, None, one) == -2                 # dim % 4
    assert L.mrag_topk_rerank_f32(None, ctypes.c_void_p(20), 4, 8, one, 1, one, 2, 1, 0, one, None, one) == -1  # alignment
    assert L.mrag_topk_rerank_f32(None, one, 4, 8, one, 1, one, 2, 1, 2, one, None, one) == -1                 # metric


def test_image_column_create_append_reopen(tmp_path):
    from motionrag_amd import rag
    rng = np.random.default_rng(0)
    t0, i0 = rng.standard_normal((3, 32)).astype(np.float32), rng.standard_normal((3, 16)).astype(np.float32)
    t1, i1 = rng.standard_normal((2, 32)).astype(np.float32), rng.standard_normal((2, 16)).astype(np.float32)
    rag.add_to_db(_rows(3), t0, text_name="t", db_path=str(tmp_path), image_embeddings=i0)
    rag.add_to_db(_rows(2, 3), t1, text_name="t", db_path=str(tmp_path), image_embeddings=i1)
    vec = np.load(tmp_path / "t" / "vectors.npy", mmap_mode="r")
    img = np.load(tmp_path / "t" / "image_vectors.npy", mmap_mode="r")
    assert vec.shape == (5, 32) and img.shape == (5, 16) and img.dtype == np.float32
    assert np.array_equal(vec, np.concatenate([t0, t1])) and np.array_equal(img, np.concatenate([i0, i1]))
    assert rag._read_meta(str(tmp_path / "t")).column("id").to_pylist() == [0, 1, 2, 3, 4]
    assert sorted(os.listdir(tmp_path / "t")) == ["image_vectors.npy", "meta.arrow", "vectors.npy"]      # no temporary file left behind
    with pytest.raises(ValueError):                                     # image dimension mismatch on append
        rag.add_to_db(_rows(1, 5), np.ones((1, 32), np.float32), text_name="t", db_path=str(tmp_path), image_embeddings=np.ones((1, 8), np.float32))
    with pytest.raises(ValueError):                                     # one image embedding per annotation
        rag.add_to_db(_rows(2, 5), np.ones((2, 32), np.float32), text_name="t", db_path=str(tmp_path), image_embeddings=np.ones((1, 16), np.float32))
    for bad in (6, 1028):                                               # D_img % 4 == 0 and <= 1 024, refused before a table is created
        with pytest.raises(ValueError):
            rag.add_to_db(_rows(1), np.ones((1, 32), np.float32), text_name="bad", db_path=str(tmp_path), image_embeddings=np.ones((1, bad), np.float32))
        assert not os.path.exists(tmp_path / "bad")
    assert np.load(tmp_path / "t" / "image_vectors.npy").shape == (5, 16) and np.load(tmp_path / "t" / "vectors.npy").shape == (5, 32)


def _snapshot(tdir):
    return {f: open(os.path.join(tdir, f), "rb").read() for f in sorted(os.listdir(tdir))}


def test_partial_image_column_is_refused_with_the_files_untouched(tmp_path):
    from motionrag_amd import rag
    rag.add_to_db(_rows(3), np.ones((3, 32), np.float32), text_name="with", db_path=str(tmp_path), image_embeddings=np.ones((3, 16), np.float32))
    rag.add_to_db(_rows(3), np.ones((3, 32), np.float32), text_name="without", db_path=str(tmp_path))
    before = {n: _snapshot(tmp_path / n) for n in ("with", "without")}
    with pytest.raises(ValueError, match="all rows or for none"):
        rag.add_to_db(_rows(1, 3), np.ones((1, 32), np.float32), text_name="with", db_path=str(tmp_path))
    with pytest.raises(ValueError, match="all rows or for none"):
        rag.add_to_db(_rows(1, 3), np.ones((1, 32), np.float32), text_name="without", db_path=str(tmp_path), image_embeddings=np.ones((1, 16), np.float32))
    assert {n: _snapshot(tmp_path / n) for n in ("with", "without")} == before
    assert "image_vectors.npy" not in before["without"]


def test_interrupted_append_with_an_image_column_is_repaired(tmp_path):
    """add_to_db replaces vectors.npy, image_vectors.npy, then meta.arrow: a crash after the first or the second rename leaves orphan vectors of one or of
    both kinds.  The next append drops them (the first `num_rows` vectors are the table before the interrupted append)."""
    from motionrag_amd import rag
    for name, orphan_text, orphan_img in (("a", 2, 0), ("b", 2, 2), ("c", 0, 2)):
        rag.add_to_db(_rows(3), np.ones((3, 8), np.float32), text_name=name, db_path=str(tmp_path), image_embeddings=4 * np.ones((3, 4), np.float32))
        vp, ip = tmp_path / name / "vectors.npy", tmp_path / name / "image_vectors.npy"
        if orphan_text:
            np.save(vp, np.concatenate([np.load(vp), 2 * np.ones((orphan_text, 8), np.float32)]))
        if orphan_img:
            np.save(ip, np.concatenate([np.load(ip), 5 * np.ones((orphan_img, 4), np.float32)]))
        rag.add_to_db(_rows(2, 3), 3 * np.ones((2, 8), np.float32), text_name=name, db_path=str(tmp_path), image_embeddings=6 * np.ones((2, 4), np.float32))
        assert np.load(vp)[:, 0].tolist() == [1.0, 1.0, 1.0, 3.0, 3.0], name
        assert np.load(ip)[:, 0].tolist() == [4.0, 4.0, 4.0, 6.0, 6.0], name
        assert rag._read_meta(str(tmp_path / name)).column("id").to_pylist() == [0, 1, 2, 3, 4]


def test_tables_open_as_before_the_interrupted_append_and_without_the_image_file(tmp_path, monkeypatch):
    """RAGDatabase.__init__ up to the device step (stubbed: no GPU here): which host arrays it opens"""
    from motionrag_amd import rag
    seen = {}

    def fake_init(self, device, metric, embedder, image_metric="l2"):
        seen["n"], seen["img"], seen["image_metric"] = self.vectors_host.shape[0], self.image_vectors_host, image_metric
    monkeypatch.setattr(rag.RAGDatabase, "_init_device", fake_init)
    rag.add_to_db(_rows(3), np.ones((3, 8), np.float32), text_name="t", db_path=str(tmp_path), image_embeddings=4 * np.ones((3, 4), np.float32))
    db = rag.RAGDatabase(str(tmp_path), "t", image_metric="dot")
    assert seen["n"] == 3 and seen["img"].shape == (3, 4) and seen["image_metric"] == "dot" and db.meta.num_rows == 3
    ip = tmp_path / "t" / "image_vectors.npy"
    np.save(ip, np.concatenate([np.load(ip), 5 * np.ones((2, 4), np.float32)]))          # crash after the image file's rename... of an append that
    vp = tmp_path / "t" / "vectors.npy"                                                  # had replaced the text vectors too
    np.save(vp, np.concatenate([np.load(vp), 2 * np.ones((2, 8), np.float32)]))
    with pytest.warns(UserWarning, match="interrupted add_to_db"):
        db = rag.RAGDatabase(str(tmp_path), "t")
    assert seen["n"] == 3 and seen["img"].shape == (3, 4) and np.all(np.asarray(seen["img"]) == 4) and db.meta.num_rows == 3
    # a table written by an earlier version: no image file -> opens unchanged, meta readable, no image column
    rag.add_to_db(_rows(3), np.ones((3, 8), np.float32), text_name="old", db_path=str(tmp_path))
    assert not os.path.exists(tmp_path / "old" / "image_vectors.npy")
    db = rag.RAGDatabase(str(tmp_path), "old")
    assert seen["n"] == 3 and seen["img"] is None and db.meta.column("video").to_pylist() == ["v0", "v0", "v1"]
    with pytest.raises(ValueError, match="image_vectors.npy"):
        db._image_column()


def test_topk_rerank_refuses_cpu_tensors():
    from motionrag_amd import ops
    with pytest.raises(ops.HipOnly):
        ops.topk_rerank(torch.zeros(4, 32), torch.zeros(1, 32), torch.zeros(1, 2, dtype=torch.int32), 1)


def test_attach_ref_videos_host_only_types():
    from motionrag_amd import rag
    annos = [{"video": f"v{i}.mp4", "start_sec": float(i), "end_sec": i + 2.0, "motion_caption": "x"} for i in range(20)]
    out = rag.attach_ref_videos([dict(a) for a in annos], None, 1, ref_video_type="gt")
    assert [a["ref_videos"] for a in out] == [[{"video": a["video"], "start_sec": a["start_sec"], "end_sec": a["end_sec"], "_distance": 0}] for a in annos]
    with pytest.raises(ValueError):
        rag.attach_ref_videos([dict(a) for a in annos], None, 9, ref_video_type="gt")          # datamodule.py:224
    a1 = rag.attach_ref_videos([dict(a) for a in annos], None, 4, ref_video_type="random", rng=random.Random(7))
    a2 = rag.attach_ref_videos([dict(a) for a in annos], None, 4, ref_video_type="random", rng=random.Random(7))
    assert [a["ref_videos"] for a in a1] == [a["ref_videos"] for a in a2]
    r = random.Random(7)
    for a in a1:
        want = r.choices(annos, k=7)                                                            # ref_video_num + 3 draws with replacement, per annotation
        assert a["ref_videos"] == [{"video": o["video"], "start_sec": o["start_sec"], "end_sec": o["end_sec"], "_distance": 0} for o in want]
    with pytest.raises(ValueError, match="Invalid ref_video_type."):
        rag.attach_ref_videos([dict(a) for a in annos], None, 4, ref_video_type="rag_image")
    with pytest.raises(ValueError):
        rag.attach_ref_videos([dict(a) for a in annos], None, 4, ref_video_type="rag_text_image")   # the two search types need a database
