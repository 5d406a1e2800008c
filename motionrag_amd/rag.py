"""Retrieval over the reference-motion database: flat-scan top-k on the GPU.

Host-side mirror of the reference's retrieval interface:

    reference                                              here
    src/data/rag.py:11-80      RAGDatabase.text_search       RAGDatabase.text_search (same arguments / result rows)
    tools/build_rag_database.py:16-74  add_to_db, prepare_annotations   add_to_db, prepare_annotations
    src/data/datamodule.py:231-236     per-annotation search fan-out     RAGDatabase.text_search_batch (one launch)
    src/data/rag.py:82-130     image_search, text_image_search       RAGDatabase.image_search, text_image_search[_batch]
    src/data/datamodule.py:222-255     the four `ref_video_type`s          attach_ref_videos

The reference delegates storage and search to lancedb==0.14.0 (Rust) and embedding to
sentence-transformers (both third-party, not installed here).  This module keeps the table as
`<db_path>/<table_name>/{vectors.npy, meta.arrow}`: fp32 [N, D] read through a memory map and uploaded to HBM in
chunks (the host never holds a second copy), and the reference's row schema as an Arrow IPC file that is memory-mapped
and read LAZILY -- only the `video` column is touched when the table opens (dictionary-encoded into the int32 group ids
of the `video != self` filter); result rows are `take`n from the mapped columns.  Sized for what the scan was measured
at (10^7 rows: 30.7 GB of vectors, no per-row Python objects); tables written by round 2 (`meta.json`) still open.
Scoring: libmrag_hip.so's `mrag_topk_f32` (sequential-fmaf distances, deterministic ties).
A table may carry a second vector column, `image_vectors.npy` (fp32 [N, D_img], the reference's `image_embedding`): for all of its rows or for none.  It
is uploaded on the first search that needs it.  `text_image_search` (`ref_video_type: rag_text_image`) is the reference's two stages as two launches: the
text search, then `mrag_topk_rerank_f32` ranking exactly the rows stage 1 returned -- in stage-1 rank order, the reference's temporary table -- by image
distance (`image_metric`, "l2": a LanceDB table without an index).  LanceDB is absent here, so these semantics are cited from src/data/rag.py:101-130, not
executed; with `select=None` we return the schema columns plus the image `_distance` (the reference's temporary table would also carry stage 1's columns).

Filter order.  The reference builds `table.search(v).limit(k)...where(where)` (src/data/rag.py:54-58), i.e. lancedb 0.14.0's
`LanceQueryBuilder.where(where, prefilter=False)` (lancedb/query.py of that release: "prefilter: bool, default False -- if True, apply the
filter before vector search, otherwise the filter is applied on the result of vector search"; the default only became True in later
releases).  That is a POST-filter: the k nearest rows are taken first, rows failing `video != "<self>"` are then dropped, and FEWER than k
rows can come back.  `RAGDatabase(prefilter=False)` (the default) reproduces this order in the kernel's final merge; `prefilter=True`
excludes rows before selection (always k results while k rows pass).  lancedb is not installed here, so the default is cited, not executed:
if a deployment's lancedb applies the filter first, construct with `prefilter=True`.  The reference over-fetches `ref_video_num + 3`
(datamodule.py:234) and keeps the first `ref_video_num` (dataset.py:296): the two orders differ for a query only when more than 3 of its 12
nearest rows are clips of its own video; `get_ref_videos` then pads with zero videos (and, like the reference, a shorter distance list).
Text
inputs need an `embedder` callable (text -> [D] fp32); the shipped data path always passes embeddings
(datamodule.py:233 hands `anno['text_embedding']`).
"""
from __future__ import annotations

import json
import os
import re
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import ops

_WHERE_RE = re.compile(r"^\s*video\s*!=\s*([\"'])(.*)\1\s*$")
SCHEMA = ("text", "id", "uid", "dataset", "video", "start_sec", "end_sec")


def prepare_annotations(annotations: List[dict], text_name: str = "llm_caption", dataset_name: str = "coin") -> List[dict]:
    """tools/build_rag_database.py:55-74"""
    return [{"text": a[text_name] if a[text_name] is not None else "", "id": a["id"], "uid": dataset_name + "/" + str(a["id"]),
             "dataset": dataset_name, "video": a["video"], "start_sec": a["start_sec"], "end_sec": a["end_sec"]} for a in annotations]


_ARROW_TYPES = {"text": "string", "id": "int64", "uid": "string", "dataset": "string", "video": "string", "start_sec": "float64", "end_sec": "float64"}
UPLOAD_CHUNK_BYTES = 256 << 20


def _rows_to_table(rows: List[dict]):
    import pyarrow as pa
    cols = {}
    for k in SCHEMA:
        vals = [r.get(k) for r in rows]                  # partial rows (tests, ad-hoc tables): missing fields are nulls
        try:
            cols[k] = pa.array(vals, type=getattr(pa, _ARROW_TYPES[k])())
        except (pa.ArrowInvalid, pa.ArrowTypeError):      # e.g. string ids: keep what the annotations carry
            cols[k] = pa.array(vals)
    return pa.table(cols)


def _read_meta(tdir: str):
    """the table's metadata as a (memory-mapped, zero-copy) Arrow table; round-2 tables carry meta.json instead"""
    import pyarrow as pa
    apath = os.path.join(tdir, "meta.arrow")
    if os.path.exists(apath):
        return pa.ipc.open_file(pa.memory_map(apath, "r")).read_all()
    with open(os.path.join(tdir, "meta.json")) as f:
        return _rows_to_table(json.load(f))


IMAGE_FILE = "image_vectors.npy"


def _truncate_vectors(path: str, n: int) -> None:
    """drop the orphan vectors of an interrupted append: keep the first `n` rows (atomic replace)"""
    keep = np.ascontiguousarray(np.load(path, mmap_mode="r")[:n])
    np.save(path + ".repair.npy", keep)
    os.replace(path + ".repair.npy", path)


def _append_vectors(path: str, new: np.ndarray) -> None:
    """create `path` or append `new` to it: the old rows are streamed through the page cache, never loaded whole; one atomic replace"""
    if not os.path.exists(path):
        np.save(path, new)
        return
    old = np.load(path, mmap_mode="r")
    tmp = path + ".tmp.npy"
    out = np.lib.format.open_memmap(tmp, mode="w+", dtype=np.float32, shape=(old.shape[0] + new.shape[0], old.shape[1]))
    step = max(1, UPLOAD_CHUNK_BYTES // (4 * old.shape[1]))
    for i in range(0, old.shape[0], step):
        j = min(i + step, old.shape[0])
        out[i:j] = old[i:j]
    out[old.shape[0]:] = new
    out.flush()
    del out, old
    os.replace(tmp, path)


def add_to_db(annotations: List[dict], embeddings: Optional[np.ndarray] = None, embedder: Optional[Callable] = None,
              text_name: str = "llm_caption", db_path: str = "../data/rag.db", image_embeddings: Optional[np.ndarray] = None) -> None:
    """tools/build_rag_database.py:16-52: append rows (+ their text embeddings, + their image embeddings) to table `text_name`.  Needs pyarrow >= 14 (as
    RAGDatabase does).  `image_embeddings` [N, D_img] fills the `image_embedding` column (image_vectors.npy): a table has it for all rows or for none.
    Append order: vectors.npy is replaced first, image_vectors.npy second, meta.arrow last (atomic renames); a reader that opens the table between them -- or
    after a crash there -- sees more vectors than rows and opens the table as it was before the append (RAGDatabase.__init__)."""
    import pyarrow as pa
    tdir = os.path.join(db_path, text_name)
    vec_path, img_path, meta_path = os.path.join(tdir, "vectors.npy"), os.path.join(tdir, IMAGE_FILE), os.path.join(tdir, "meta.arrow")
    # ---- everything that can be refused is refused before a file is touched
    if embeddings is None:
        if embedder is None:
            raise ValueError("add_to_db needs `embeddings` or an `embedder` (sentence-transformers is third-party)")
        embeddings = np.stack([np.asarray(embedder(a["text"]), dtype=np.float32) for a in annotations])
    embeddings = np.ascontiguousarray(embeddings, dtype=np.float32)
    if embeddings.shape[0] != len(annotations):
        raise ValueError("one embedding per annotation")
    if image_embeddings is not None:
        image_embeddings = np.ascontiguousarray(image_embeddings, dtype=np.float32)
        if image_embeddings.ndim != 2 or image_embeddings.shape[0] != len(annotations):
            raise ValueError("one image embedding per annotation")
        if image_embeddings.shape[1] % 4 != 0 or not 0 < image_embeddings.shape[1] <= 1024:
            raise ValueError(f"image embeddings: dimension {image_embeddings.shape[1]} is not a multiple of 4 up to 1 024 (the limit of mrag_topk_f32)")
    n_meta = _read_meta(tdir).num_rows if (os.path.exists(meta_path) or os.path.exists(os.path.join(tdir, "meta.json"))) else None
    if os.path.exists(vec_path):
        old = np.load(vec_path, mmap_mode="r")
        n_old = old.shape[0] if n_meta is None else min(n_meta, old.shape[0])      # rows of the table as it opens (orphans of an interrupted append excluded)
        if old.shape[1] != embeddings.shape[1]:
            raise ValueError(f"table holds {old.shape[1]}-dimensional vectors, got {embeddings.shape[1]}")
        del old
        if (os.path.exists(img_path) and image_embeddings is None) or (n_old > 0 and not os.path.exists(img_path) and image_embeddings is not None):
            raise ValueError(f"{tdir}: the image column is held for all rows or for none -- the table " +
                             ("has one and this append brings no `image_embeddings`" if os.path.exists(img_path) else
                              f"has none ({IMAGE_FILE} is absent) and this append brings `image_embeddings`"))
        if image_embeddings is not None and os.path.exists(img_path):
            d_img = np.load(img_path, mmap_mode="r").shape[1]
            if d_img != image_embeddings.shape[1]:
                raise ValueError(f"table holds {d_img}-dimensional image vectors, got {image_embeddings.shape[1]}")
    if n_meta is not None:                                  # an interrupted append: drop its orphan vectors (of either kind) before appending again
        for path in (vec_path, img_path):
            if os.path.exists(path) and np.load(path, mmap_mode="r").shape[0] > n_meta:
                _truncate_vectors(path, n_meta)
    os.makedirs(tdir, exist_ok=True)
    table = _rows_to_table(annotations)
    appending = os.path.exists(vec_path)
    _append_vectors(vec_path, embeddings)
    if image_embeddings is not None:
        _append_vectors(img_path, image_embeddings)
    if appending:
        table = pa.concat_tables([_read_meta(tdir), table], promote_options="default")
    tmp = meta_path + ".tmp"
    with pa.OSFile(tmp, "wb") as sink, pa.ipc.new_file(sink, table.schema) as w:
        w.write_table(table)
    os.replace(tmp, meta_path)
    legacy = os.path.join(tdir, "meta.json")
    if os.path.exists(legacy):
        os.remove(legacy)


class RAGDatabase:
    """src/data/rag.py:11-15; `metric` is LanceDB's: 'l2' (its default without an index; `_distance` is the squared
    L2 distance) or 'dot' (`_distance = 1 - dot`, the metric of the index build_rag_database.py:52 creates).  `image_metric`: the metric of searches
    over the image column ('l2': the reference builds no index on `image_embedding`, and text_image_search's temporary table never has one).

    `wide_fanout` (default False; an attribute that may be set later): batch searches of 16 or more queries with 16 < top_k <= 32 -- text_search_batch,
    image_search_batch and stage 1 of text_image_search_batch, e.g. the 21 rows `rag_text_image` asks for -- run the fan-out form (`ops.topk(order="mfma")`:
    one pass over the table per 128 queries) instead of the scan form's pass per 16 queries.  What changes: WHICH rows make the list at its edge follows the
    fan-out form's selection ("l2": the top_k nearest under the expanded score |q|^2 + |x|^2 - 2 q.x, scored again exactly and re-ranked; a row closer than
    the expansion's error to the top_k-th may swap with it), as batches at top_k <= 16 already behave; the distance a row is given does not depend on the
    form.  Single-query calls (and batches of fewer than 16) stay on the scan form.  Off by default because it moves results that were pinned before the
    wide lists existed."""

    def __init__(self, db_path: str, table_name: str, device: str = "cuda", metric: str = "l2", embedder: Optional[Callable] = None,
                 prefilter: bool = False, image_metric: str = "l2", wide_fanout: bool = False):
        self.prefilter = bool(prefilter)          # lancedb's `where(..., prefilter=)`; False = its 0.14.0 default (module docstring)
        self.wide_fanout = bool(wide_fanout)
        tdir = os.path.join(db_path, table_name)
        self.vectors_host = np.load(os.path.join(tdir, "vectors.npy"), mmap_mode="c")      # a copy-on-write view of the file (never written): pages stream through on upload
        self._image_path = os.path.join(tdir, IMAGE_FILE)
        self.image_vectors_host = np.load(self._image_path, mmap_mode="c") if os.path.exists(self._image_path) else None   # tables of earlier versions: no image column
        self.meta = _read_meta(tdir)
        n_img = self.meta.num_rows if self.image_vectors_host is None else self.image_vectors_host.shape[0]
        if self.vectors_host.shape[0] > self.meta.num_rows or n_img > self.meta.num_rows:
            # add_to_db appends by replacing vectors.npy, image_vectors.npy and THEN meta.arrow: a crash (or an open) between the renames leaves new vectors
            # without their rows.  The table is append-only, so its first `num_rows` vectors are exactly the table before that append: open that.
            import warnings
            warnings.warn(f"{tdir}: {self.vectors_host.shape[0]} vectors" + (f" / {n_img} image vectors" if self.image_vectors_host is not None else "") +
                          f" but {self.meta.num_rows} metadata rows -- an interrupted add_to_db; opening the {self.meta.num_rows} complete rows (re-run the append)")
            self.vectors_host = self.vectors_host[:self.meta.num_rows]
            if self.image_vectors_host is not None:
                self.image_vectors_host = self.image_vectors_host[:self.meta.num_rows]
        self._init_device(device, metric, embedder, image_metric)

    @classmethod
    def from_arrays(cls, vectors: np.ndarray, rows, device: str = "cuda", metric: str = "l2", embedder=None, prefilter: bool = False,
                    image_vectors: Optional[np.ndarray] = None, image_metric: str = "l2", wide_fanout: bool = False) -> "RAGDatabase":
        """`rows`: list of row dicts in the reference's schema, or an Arrow table with those columns; `image_vectors` [N, D_img]: the image column;
        `wide_fanout`: see the class docstring"""
        self = cls.__new__(cls)
        self.prefilter = bool(prefilter)
        self.wide_fanout = bool(wide_fanout)
        self.vectors_host = vectors if (isinstance(vectors, np.ndarray) and vectors.dtype == np.float32) else np.ascontiguousarray(vectors, dtype=np.float32)
        self._image_path = IMAGE_FILE
        self.image_vectors_host = None if image_vectors is None else (
            image_vectors if (isinstance(image_vectors, np.ndarray) and image_vectors.dtype == np.float32) else np.ascontiguousarray(image_vectors, dtype=np.float32))
        self.meta = _rows_to_table(rows) if isinstance(rows, list) else rows
        self._init_device(device, metric, embedder, image_metric)
        return self

    def _init_device(self, device, metric, embedder, image_metric="l2"):
        import pyarrow as pa
        import pyarrow.compute as pc
        if metric not in ("l2", "dot"):
            raise ValueError(f"Invalid metric: {metric}")
        if image_metric not in ("l2", "dot"):
            raise ValueError(f"Invalid image_metric: {image_metric}")
        self.metric, self.embedder, self.image_metric = metric, embedder, image_metric
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ops.HipOnly("RAGDatabase scores on the GPU only (libmrag_hip.so); there is no CPU search path")
        N, D = self.vectors_host.shape
        if self.meta.num_rows != N:
            raise ValueError(f"{N} vectors but {self.meta.num_rows} metadata rows")
        if self.image_vectors_host is not None:
            if self.image_vectors_host.ndim != 2 or self.image_vectors_host.shape[0] != N:
                raise ValueError(f"{self.image_vectors_host.shape[0]} image vectors but {N} rows: the image column is held for all rows or for none")
            if self.image_vectors_host.shape[1] % 4 != 0 or not 0 < self.image_vectors_host.shape[1] <= 1024:
                raise ValueError(f"image vectors: dimension {self.image_vectors_host.shape[1]} is not a multiple of 4 up to 1 024 (the limit of mrag_topk_f32)")
        # group id of a row = index of its video among the distinct videos in order of first appearance (the `video != "<name>"` filter of
        # datamodule.py:235 compares ids in the kernel): one dictionary encoding of ONE column, no per-row Python objects
        enc = pc.dictionary_encode(self.meta.column("video").combine_chunks() if self.meta.num_rows else pa.array([], pa.string()))
        self._videos = enc.dictionary
        self.group = torch.from_numpy(np.array(enc.indices.to_numpy(zero_copy_only=False), dtype=np.int32)).to(self.device)     # np.array: a writable copy
        self.vectors = self._upload(self.vectors_host)                                     # resident in HBM for every search
        self.image_vectors = None                                                          # uploaded by the first search that needs it (_image_column)
        self._plans = {}
        import threading
        self._lock = threading.Lock()

    def _upload(self, host: np.ndarray) -> torch.Tensor:
        N, D = host.shape
        dev = torch.empty(N, D, dtype=torch.float32, device=self.device)
        step = max(1, UPLOAD_CHUNK_BYTES // (4 * D))
        for i in range(0, N, step):                                                        # chunked: the host side is the page cache of the mapped file
            dev[i:i + step].copy_(torch.from_numpy(np.ascontiguousarray(host[i:i + step])))
        return dev

    def _image_column(self) -> torch.Tensor:
        """the image column in HBM: uploaded on the first search that needs it (a text-only user pays nothing)"""
        if self.image_vectors_host is None:
            raise ValueError(f"this table has no image column ({self._image_path} is missing): build it with add_to_db(..., image_embeddings=...)")
        with self._lock:
            if self.image_vectors is None:
                self.image_vectors = self._upload(self.image_vectors_host)
        return self.image_vectors

    def __len__(self):
        return self.meta.num_rows

    def _batch_order(self, n_queries: int, top_k: int) -> str:
        """`order` of a batch search's ops.topk: the fan-out form by name for the wide lists when `wide_fanout` is set, else the automatic choice"""
        return "mfma" if (getattr(self, "wide_fanout", False) and n_queries >= 16 and 16 < top_k <= 32) else "auto"

    @property
    def rows(self) -> List[dict]:
        """every row as a dict (debugging / small tables; searches never build this)"""
        return self.meta.to_pylist()

    # ---- result formatting (rag.py:17-34) ----
    def _format(self, rows_idx: np.ndarray, dist: np.ndarray, select: Optional[Sequence[str]], output_format: str):
        import pyarrow as pa
        cols = list(select) if select is not None else list(SCHEMA)
        keep = rows_idx >= 0
        hit = self.meta.select(cols).take(pa.array(rows_idx[keep].astype(np.int64)))      # only the requested columns of the hit rows leave the map
        hit = hit.append_column("_distance", pa.array(dist[keep].astype(np.float64)))
        if output_format in ("dict", "list"):
            return hit.to_pylist()
        if output_format == "pandas":
            return hit.to_pandas()
        if output_format == "pyarrow":
            return hit
        raise ValueError(f"Invalid format: {output_format}")

    def _exclude_id(self, where: Optional[str]) -> int:
        """`where` of the reference is an SQL string handed to LanceDB (src/data/rag.py:36-61); the one filter the shipped data path builds is
        `video != "<name>"` (datamodule.py:235), evaluated here as an id comparison inside the scan.  Anything else is refused up front."""
        if where is None:
            return -1
        m = _WHERE_RE.match(where)
        if not m:
            raise ValueError(f"unsupported `where` filter {where!r}: this scan evaluates only the reference's own `video != \"<name>\"` "
                             f"(src/data/datamodule.py:235); a general SQL predicate needs LanceDB")
        import pyarrow as pa
        import pyarrow.compute as pc
        idx = pc.index_in(pa.scalar(m.group(2)), value_set=self._videos).as_py()
        return -1 if idx is None else int(idx)

    def _exclude_ids(self, where: Sequence[Optional[str]]) -> List[int]:
        """one id per query; the names of a batch are looked up in ONE pass over the distinct videos"""
        import pyarrow as pa
        import pyarrow.compute as pc
        names = []
        for w in where:
            if w is None:
                names.append(None)
                continue
            m = _WHERE_RE.match(w)
            if not m:
                self._exclude_id(w)          # raises the descriptive error
            names.append(m.group(2))
        idx = pc.index_in(pa.array(names, pa.string()), value_set=self._videos).to_pylist()
        return [-1 if (i is None or n is None) else int(i) for i, n in zip(idx, names)]

    def _embed(self, text) -> np.ndarray:
        if isinstance(text, str):
            if self.embedder is None:
                raise ValueError("text queries need an `embedder`; the data path passes embeddings (datamodule.py:233)")
            text = self.embedder(text)
        if isinstance(text, torch.Tensor):
            text = text.detach().float().cpu().numpy()
        return np.ascontiguousarray(text, dtype=np.float32).reshape(-1)

    def _queries(self, embeddings) -> torch.Tensor:
        if isinstance(embeddings, torch.Tensor):
            return embeddings.to(self.device, torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32)).to(self.device)

    def text_search_batch(self, embeddings, top_k: int = 10, where: Optional[Sequence[Optional[str]]] = None,
                          select: Optional[Sequence[str]] = None, output_format: str = "dict", prefilter: Optional[bool] = None):
        """all queries of datamodule.py:231-236 in one launch: embeddings [Q, D]; `where` one filter per query.  `prefilter` overrides the
        database's filter order for this call (None = `self.prefilter`); with the post-filter a query may return fewer than `top_k` rows."""
        return self._column_search_batch("text", embeddings, top_k, where, select, output_format, prefilter)

    def image_search_batch(self, image_embeddings, top_k: int = 10, where: Optional[Sequence[Optional[str]]] = None,
                           select: Optional[Sequence[str]] = None, output_format: str = "dict", prefilter: Optional[bool] = None):
        """text_search_batch over the image column of the whole table (metric `image_metric`)"""
        return self._column_search_batch("image", image_embeddings, top_k, where, select, output_format, prefilter)

    def _column_search_batch(self, column: str, embeddings, top_k, where, select, output_format, prefilter):
        post = not (self.prefilter if prefilter is None else prefilter)
        vectors, metric = (self.vectors, self.metric) if column == "text" else (self._image_column(), self.image_metric)
        q = self._queries(embeddings)
        Q = q.shape[0]
        group = exclude = None
        if where is not None and any(w is not None for w in where):
            exclude = torch.tensor(self._exclude_ids(where), dtype=torch.int32, device=self.device)       # every filter parsed BEFORE anything launches
            group = self.group
        if Q <= 4 and top_k <= 64:       # the interactive search (rag.py:63-80): a prepared plan -- one C-ABI call = one launch, no allocation
            # a plan owns its workspace, arrival counters included: one per (Q, k, STREAM) so that searches issued from different streams never share
            # counters, and a lock so that two host threads on one stream cannot interleave the copy-in / launch / read-out of one plan
            key = (Q, top_k, torch.cuda.current_stream(self.device).cuda_stream, post) + (() if column == "text" else (column,))
            with self._lock:
                plan = self._plans.get(key)
                if plan is None:
                    plan = self._plans[key] = ops.TopkPlan(vectors, Q, top_k, metric=metric, group=self.group, postfilter=post)
                plan.queries.copy_(q)
                if exclude is not None:
                    plan.exclude.copy_(exclude)
                else:
                    plan.exclude.fill_(-1)
                rows, dist = plan.run()
                rows, dist = rows.cpu().numpy(), dist.cpu().numpy()
            self._note_short(rows, top_k, post, exclude is not None)
            return [self._format(rows[i], dist[i], select, output_format) for i in range(Q)]
        else:
            rows, dist = ops.topk(vectors, q, top_k, metric=metric, group=group, exclude=exclude, postfilter=post, order=self._batch_order(Q, top_k))
        rows, dist = rows.cpu().numpy(), dist.cpu().numpy()
        self._note_short(rows, top_k, post, exclude is not None)
        return [self._format(rows[i], dist[i], select, output_format) for i in range(Q)]

    def text_image_search_batch(self, text_embeddings, image_embeddings, top_k=(20, 10), where: Optional[Sequence[Optional[str]]] = None,
                                select: Optional[Sequence[str]] = None, output_format: str = "dict", prefilter: Optional[bool] = None):
        """src/data/rag.py:101-130 for all queries of datamodule.py:239-245 at once: text_embeddings [Q, D], image_embeddings [Q, D_img], `where` one
        filter per query.  Stage 1 = the text search for `top_k[0]` rows with `where` in the filter order (a post-filtered list can be short); stage 2 =
        exactly those rows -- the reference's temporary table, in stage-1 rank order -- ranked by image distance (`image_metric`), no filter, first
        `top_k[1]`; `_distance` is the image distance; equal image distances keep their stage-1 order.  Two launches on the current stream: stage 1's
        rows go from its output buffer straight into the re-rank on the device; one copy to the host at the end."""
        try:
            k0, k1 = (int(t) for t in top_k)
        except (TypeError, ValueError):
            raise ValueError("text_image_search: top_k = (rows of the text stage, rows of the image stage)") from None
        if not (1 <= k1 <= k0 <= 64):
            raise ValueError(f"text_image_search: 1 <= top_k[1] <= top_k[0] <= 64 (the re-rank kernel's list length), got {tuple(top_k)}")
        post = not (self.prefilter if prefilter is None else prefilter)
        image_vectors = self._image_column()                                                   # a table without the column is refused before anything launches
        q, qi = self._queries(text_embeddings), self._queries(image_embeddings)
        Q = q.shape[0]
        if q.dim() != 2 or qi.dim() != 2 or qi.shape[0] != Q or q.shape[1] != self.vectors.shape[1] or qi.shape[1] != image_vectors.shape[1]:
            raise ValueError(f"text_image_search: text embeddings [Q, {self.vectors.shape[1]}] and image embeddings [Q, {image_vectors.shape[1]}] expected, "
                             f"got {tuple(q.shape)} and {tuple(qi.shape)}")
        if Q == 0:
            return []
        group = exclude = None
        if where is not None and any(w is not None for w in where):
            exclude = torch.tensor(self._exclude_ids(where), dtype=torch.int32, device=self.device)
            group = self.group
        cand, _ = ops.topk(self.vectors, q, k0, metric=self.metric, group=group, exclude=exclude, postfilter=post, order=self._batch_order(Q, k0))
        rows, _, dist = ops.topk_rerank(image_vectors, qi, cand, k1, metric=self.image_metric)
        both = torch.stack((rows, dist.view(torch.int32))).cpu().numpy()                        # ONE copy to the host
        rows, dist = both[0], both[1].view(np.float32)
        self._note_short(rows, k1, post, exclude is not None)
        return [self._format(rows[i], dist[i], select, output_format) for i in range(Q)]

    def _note_short(self, rows: np.ndarray, top_k: int, post: bool, filtered: bool) -> None:
        """ONE warning per database when the post-filter order hands back fewer than `top_k` rows: a deployment whose LanceDB pre-filters would have
        got `top_k` there (`RAGDatabase(prefilter=True)` is that order)."""
        if post and filtered and top_k <= len(self) and not getattr(self, "_short_noted", False) and (rows < 0).any():
            import warnings
            self._short_noted = True
            short = int((rows < 0).any(axis=1).sum())
            warnings.warn(f"RAGDatabase: {short} of {rows.shape[0]} filtered searches returned fewer than top_k={top_k} rows -- the `where` filter is applied AFTER the "
                          "k nearest rows were taken (lancedb 0.14.0's `where(..., prefilter=False)`, src/data/rag.py:57-58); the consumer pads the missing "
                          "references with zero clips.  RAGDatabase(prefilter=True) filters before the selection.  (reported once per database)")

    def vector_search(self, vector, vector_column_name: str = None, top_k: int = 10, table=None, where: str = None,
                      select: List[str] = None, nprobes: int = 50, refine_factor: int = 30, output_format: str = "dict",
                      prefilter: Optional[bool] = None):
        """rag.py:36-61 (flat scan: nprobes / refine_factor only matter for LanceDB's IVF index and are accepted for
        signature compatibility).  Columns: `text_embedding` (the default) and `image_embedding`."""
        if vector_column_name not in (None, "text_embedding", "image_embedding"):
            raise ValueError(f"no vector column {vector_column_name!r}: the table holds `text_embedding` and (optionally) `image_embedding`")
        if table is not None:
            raise NotImplementedError("searching a caller's temporary table is not supported: the temporary table of the two-stage search is internal")
        emb = self._embed(vector)[None]
        return self._column_search_batch("image" if vector_column_name == "image_embedding" else "text", emb, top_k, [where], select, output_format, prefilter)[0]

    def text_search(self, text, top_k: int = 10, table=None, where: str = None, select: List[str] = None, nprobes: int = 50,
                    refine_factor: int = 30, output_format: str = "dict", prefilter: Optional[bool] = None):
        """rag.py:63-80 (`prefilter`: not a reference argument; None = the database's filter order)"""
        return self.vector_search(text, vector_column_name="text_embedding", top_k=top_k, table=table, where=where, select=select,
                                  nprobes=nprobes, refine_factor=refine_factor, output_format=output_format, prefilter=prefilter)

    def image_search(self, image_embedding, top_k: int = 10, table=None, where: str = None, select: List[str] = None, nprobes: int = 50,
                     refine_factor: int = 30, output_format: str = "dict", prefilter: Optional[bool] = None):
        """rag.py:82-99: the image column of the whole table, metric `image_metric`"""
        return self.vector_search(image_embedding, vector_column_name="image_embedding", top_k=top_k, table=table, where=where, select=select,
                                  nprobes=nprobes, refine_factor=refine_factor, output_format=output_format, prefilter=prefilter)

    def text_image_search(self, text, image_embedding, top_k=(20, 10), table=None, where: str = None, select: List[str] = None, nprobes: int = 50,
                          refine_factor: int = 30, output_format: str = "dict", prefilter: Optional[bool] = None):
        """rag.py:101-130: text_image_search_batch with one query"""
        if table is not None:
            raise NotImplementedError("searching a caller's temporary table is not supported: the temporary table of the two-stage search is internal")
        return self.text_image_search_batch(self._embed(text)[None], self._embed(image_embedding)[None], top_k, [where], select, output_format, prefilter)[0]


# ---------------------------------------------------------------------------------------------- callers either side of the search
def attach_ref_videos(annotations: List[dict], db: Optional["RAGDatabase"] = None, ref_video_num: int = 9, *, ref_video_type: str = "rag_text",
                      chunk: int = 256, rng=None) -> List[dict]:
    """The reference-video fan-out of src/data/datamodule.py:222-265: `anno['ref_videos']` = rows of `['video', 'start_sec', 'end_sec']` + `_distance`.
      'rag_text'        every annotation searches with its own `text_embedding`, over-fetches `ref_video_num + 3` rows (:234) and excludes its own
                        video (`where = 'video != "<self>"'`, :235);
      'rag_text_image'  text_image_search with `top_k = (2 * ref_video_num + 3, ref_video_num)` and the annotation's `image_embedding` (:239-245);
      'gt'              the annotation's own clip, `_distance` 0; `ref_video_num` must be 1 (:223-229);
      'random'          `ref_video_num + 3` draws with replacement from the annotations, `_distance` 0 (:247-253); `rng`: a `random.Random` to seed it.
    The reference runs one LanceDB query per annotation in a 64-process pool; here the queries of a chunk are ONE batched search ('gt' / 'random' are
    host-only and need no `db`)."""
    if ref_video_type == "gt":
        if ref_video_num != 1:
            raise ValueError("ref_video_num must be 1 when ref_video_type is GT")
        for a in annotations:
            a["ref_videos"] = [{"video": a["video"], "start_sec": a["start_sec"], "end_sec": a["end_sec"], "_distance": 0}]
        return annotations
    if ref_video_type == "random":
        import random as _random
        rng = rng or _random
        for a in annotations:
            a["ref_videos"] = [{"video": o["video"], "start_sec": o["start_sec"], "end_sec": o["end_sec"], "_distance": 0}
                               for o in rng.choices(annotations, k=ref_video_num + 3)]
        return annotations
    if ref_video_type not in ("rag_text", "rag_text_image"):
        raise ValueError("Invalid ref_video_type.")
    if db is None:
        raise ValueError(f"ref_video_type {ref_video_type!r} needs a RAGDatabase")
    select = ["video", "start_sec", "end_sec"]
    for i in range(0, len(annotations), chunk):
        part = annotations[i:i + chunk]
        q = np.stack([np.asarray(a["text_embedding"], dtype=np.float32) for a in part])
        where = [f'video != "{a["video"]}"' for a in part]
        if ref_video_type == "rag_text":
            res = db.text_search_batch(q, top_k=ref_video_num + 3, where=where, select=select)
        else:
            qi = np.stack([np.asarray(a["image_embedding"], dtype=np.float32) for a in part])
            res = db.text_image_search_batch(q, qi, top_k=(2 * ref_video_num + 3, ref_video_num), where=where, select=select)
        for a, r in zip(part, res):
            a["ref_videos"] = r
    return annotations


def get_ref_videos(video_info: dict, video: torch.Tensor, load_clip: Callable[[dict], torch.Tensor], ref_video_num: int = 9,
                   video_length: Optional[int] = None, uncond_video_ratio: float = 0.0, rng=None):
    """The consumer contract of src/data/dataset.py:285-312 (`VideoDataset.get_ref_videos`): video [1, T, C, H, W] ->
    (ref_videos [K, T, C, H, W], distance list).  The first `ref_video_num` retrieved rows are used (most similar first); a reference that
    IS the target clip re-uses `video`; a dropped (unconditional-training) reference or one whose clip fails to load leaves a ZERO video and
    distance 1.0 (:292, :306-310).  `load_clip(row) -> [1, T, C, H, W]` stands for the dataset's video reader (out of scope)."""
    import random as _random
    rng = rng or _random
    T = video_length if video_length is not None else video.shape[1]
    ref_videos = torch.zeros(ref_video_num, T, *video.shape[2:], dtype=video.dtype, device=video.device)
    distance: List[float] = []
    for i, v in enumerate(video_info.get("ref_videos", [])[:ref_video_num]):
        if rng.random() > uncond_video_ratio:
            try:
                ref = video if v["video"] == video_info["video"] else load_clip(v)
                ref_videos[i] = ref
                distance.append(v["_distance"])
            except Exception as e:          # noqa: BLE001 -- the reference swallows reader errors the same way
                print(f"Rag read video Error: {e}")
                distance.append(1.0)
        else:
            distance.append(1.0)
    return ref_videos, distance


_ADJ = ("slow", "fast", "shaky", "smooth", "sudden", "gentle", "circular", "zigzag", "rising", "falling")
_NOUN = ("camera", "person", "dog", "car", "bird", "wave", "hand", "crowd", "leaf", "train")
_VERB = ("pans left", "pans right", "zooms in", "zooms out", "walks forward", "turns around", "jumps", "rotates", "drifts", "stops")


def synthetic_captions(n: int = 10000) -> List[dict]:
    """BASELINE config #1 / SURVEY 8d: `n` synthetic motion captions `clip {i}: a {adj} {noun} {verb}` in the reference's annotation schema"""
    return [{"motion_caption": f"clip {i}: a {_ADJ[i % 10]} {_NOUN[(i // 10) % 10]} {_VERB[(i // 100) % 10]}", "id": i, "video": f"clip_{i:06d}.mp4",
             "start_sec": 0.0, "end_sec": 4.0} for i in range(n)]


def hash_embedder(dim: int = 768) -> Callable[[str], np.ndarray]:
    """Offline stand-in for sentence-transformers' gte-base-en-v1.5 (third-party weights, no network): a unit-normalised N(0, 1) vector
    seeded by the caption's hash -- deterministic, `dim`-dimensional, fp32."""
    import hashlib

    def embed(text: str) -> np.ndarray:
        seed = int.from_bytes(hashlib.sha256(text.encode("utf-8")).digest()[:8], "little")
        v = np.random.default_rng(seed).standard_normal(dim).astype(np.float32)
        return v / np.linalg.norm(v)

    return embed
