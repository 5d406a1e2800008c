"""Query / caption text embedder of the retrieval row on the HIP kernels: the encoder the reference registers as the LanceDB table's embedding
function -- sentence-transformers `Alibaba-NLP/gte-base-en-v1.5` in bf16 (`tools/build_rag_database.py:16-33`; `src/data/rag.py:13-15` moves it to the query
device; `table.search(text)` embeds the query with it).

The model class is remote code (`NewModel`, trust_remote_code) behind two third-party wrappers, none of them installed here: `NewModel` below carries the
published parameter names (`embeddings.word_embeddings`, `encoder.layer.N.attention.{qkv_proj, o_proj}`, `attn_ln`, `mlp.{up_gate_proj, down_proj}`, `mlp_ln`), so
the checkpoint's `model.safetensors` loads unchanged; the arithmetic follows `oracle/gte_ref.py` -- PARITY UNPINNED, verify against the real model before use.

Data path per layer (bf16 rows, fp32 accumulation; no padding and no mask: sequences of one length batched together, or -- `forward_packed`, `SentenceEmbedder(packed=True)`,
right-padded `forward` -- sequences of any lengths packed into one row matrix, with `mrag_attn_varlen_fwd_bf16` as the attention):
  qkv_proj + rotary embedding   one GEMM with the RoPE epilogue (`mrag_gemm_bf16`, EPI_QKNORM_ROPE without the LayerNorm): the checkpoint's `rotate_half` pairing
                                (i, i + 32) becomes the kernel's interleaved pairing (2i, 2i + 1) by permuting the q / k output rows once at load time -- a
                                permutation of head dimensions applied to q and k alike leaves q . k unchanged
  attention                     `mrag_attn_fwd_bf16` (12 heads of 64)
  o_proj + residual, post-LN    GEMM with the residual epilogue, `mrag_layernorm_bf16`
  gated MLP                     up_gate_proj as one GEMM with the `up * gelu_erf(gate)` epilogue, down_proj + residual, post-LN
  sentence embedding            first ([CLS]) token, L2-normalised in fp32 (`normalize=True` of the LanceDB wrapper)
GPU only; no CPU fallback."""
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Sequence

import torch
from torch import nn

from . import ops
from .layers import CACHE, Holder, bf16


class NewModel(nn.Module):
    """`Alibaba-NLP/new-impl` NewModel as gte-base-en-v1.5 configures it (rope + NTK factor 2, packed qkv, gated GELU MLP, post-norm, no token types)"""

    def __init__(self, vocab_size: int = 30528, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12, intermediate_size: int = 3072,
                 layer_norm_eps: float = 1e-12, max_position_embeddings: int = 8192, rope_theta: float = 500000.0, rope_scaling_factor: float = 2.0, **_unused):
        super().__init__()
        if hidden_size != 64 * num_attention_heads:
            raise NotImplementedError("the gfx950 attention kernels are built for head_dim 64")
        self.config = SimpleNamespace(vocab_size=vocab_size, hidden_size=hidden_size, num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                                      intermediate_size=intermediate_size, layer_norm_eps=layer_norm_eps, max_position_embeddings=max_position_embeddings,
                                      rope_theta=rope_theta, rope_scaling_factor=rope_scaling_factor)
        self.embeddings = Holder()
        self.embeddings.word_embeddings = nn.Embedding(vocab_size, hidden_size, padding_idx=0)
        self.embeddings.LayerNorm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        layers = []
        for _ in range(num_hidden_layers):
            lyr = Holder()
            lyr.attention = Holder()
            lyr.attention.qkv_proj = nn.Linear(hidden_size, 3 * hidden_size)
            lyr.attention.o_proj = nn.Linear(hidden_size, hidden_size)
            lyr.attn_ln = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
            lyr.mlp = Holder()
            lyr.mlp.up_gate_proj = nn.Linear(hidden_size, 2 * intermediate_size, bias=False)
            lyr.mlp.down_proj = nn.Linear(intermediate_size, hidden_size)
            lyr.mlp_ln = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
            layers.append(lyr)
        self.encoder = Holder()
        self.encoder.layer = nn.ModuleList(layers)
        self._rope_cache: Dict = {}

    def _rope(self, S: int, device):
        """fp32 [S, 64] tables in the kernel's interleaved layout: columns 2i and 2i + 1 carry frequency i.  NTK scaling: the published class builds its cache for
        factor * max_position_embeddings positions, so every position uses inv_freq_i = (theta * factor)^(-2i/64) / factor^(2/64)."""
        key = (S, str(device))
        if key not in self._rope_cache:
            c = self.config
            inv = 1.0 / ((c.rope_theta * c.rope_scaling_factor) ** (torch.arange(0, 64, 2, dtype=torch.float32) / 64)) / c.rope_scaling_factor ** (2.0 / 64)
            ang = torch.arange(S, dtype=torch.float32)[:, None] * inv[None, :]
            ang = ang.repeat_interleave(2, dim=1)
            if len(self._rope_cache) >= 64:                                     # one table per sequence length the builder meets; bounded
                self._rope_cache.clear()
            self._rope_cache[key] = (ang.cos().contiguous().to(device), ang.sin().contiguous().to(device))
        return self._rope_cache[key]

    @staticmethod
    def _qkv_interleaved(lin: nn.Linear, heads: int):
        """q and k output rows of every head re-ordered (i, i + 32) -> (2i, 2i + 1): `rotate_half` RoPE on the checkpoint's layout == interleaved RoPE on this one"""
        def build():
            d = lin.weight.shape[1]
            per_head = torch.stack([torch.arange(32), torch.arange(32) + 32], dim=1).reshape(-1)                 # [0, 32, 1, 33, ...]
            qk = (torch.arange(heads)[:, None] * 64 + per_head[None, :]).reshape(-1)
            rows = torch.cat([qk, d + qk, 2 * d + torch.arange(d)]).to(lin.weight.device)
            return bf16(lin.weight)[rows].contiguous(), bf16(lin.bias)[rows].contiguous()
        return CACHE.get(("gte_qkv", id(lin)), (lin.weight, lin.bias), build)

    def _layers(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, attend) -> torch.Tensor:
        """the encoder layers on x [B, S, hidden] (already embedded and normalised); `attend(qkv [B, S, 3 * hidden]) -> [B, S, hidden]` is the attention of the layout"""
        c = self.config
        H = c.num_attention_heads
        for lyr in self.encoder.layer:
            att, mlp = lyr.attention, lyr.mlp
            wqkv, bqkv = self._qkv_interleaved(att.qkv_proj, H)
            a = attend(ops.qkv_linear_qknorm_rope(x, wqkv, bqkv, H, None, None, None, None, cos, sin, 0))
            x = ops.linear(a, bf16(att.o_proj.weight), bf16(att.o_proj.bias), epilogue=ops.EPI_RESID, resid=x)
            x = ops.layernorm(x, bf16(lyr.attn_ln.weight), bf16(lyr.attn_ln.bias), c.layer_norm_eps)
            wg = CACHE.get(("gte_geglu", id(mlp.up_gate_proj)), mlp.up_gate_proj.weight, lambda: ops.geglu_interleave(bf16(mlp.up_gate_proj.weight), None)[0])
            g = ops.linear(x, wg, epilogue=ops.EPI_GEGLU)                                   # [up | gate] -> up * gelu_erf(gate)
            x = ops.linear(g, bf16(mlp.down_proj.weight), bf16(mlp.down_proj.bias), epilogue=ops.EPI_RESID, resid=x)
            x = ops.layernorm(x, bf16(lyr.mlp_ln.weight), bf16(lyr.mlp_ln.bias), c.layer_norm_eps)
        return x

    def _embed(self, input_ids: torch.Tensor) -> torch.Tensor:
        emb, c = self.embeddings, self.config
        return ops.layernorm(bf16(emb.word_embeddings.weight)[input_ids].contiguous(), bf16(emb.LayerNorm.weight), bf16(emb.LayerNorm.bias), c.layer_norm_eps)

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, **_unused):
        """input_ids [B, S] -> object with `.last_hidden_state` [B, S, hidden] bf16 (`[0]` works too).  Without padding (no `attention_mask`, or all ones) the batch
        runs as it is; a RIGHT-padded `attention_mask` packs the valid tokens, runs `forward_packed` and returns zeros at the padded positions (one read-back of the
        row lengths).  A mask with a hole or with left padding is not taken."""
        if not input_ids.is_cuda:
            raise ops.HipOnly("NewModel: GPU tensors only")
        B, S = input_ids.shape
        H, d = self.config.num_attention_heads, self.config.hidden_size
        if attention_mask is not None and tuple(attention_mask.shape) != (B, S):
            raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not match input_ids {(B, S)}")
        lengths = None if attention_mask is None else mask_lengths(attention_mask)          # the one read-back; all ones -> the unpadded path below
        if lengths is not None and lengths.numel() and int(lengths.min()) < S:
            cu, positions, index = pack_lengths(lengths, S)
            out = torch.zeros(B * S, d, dtype=torch.bfloat16, device=input_ids.device)
            if index.numel():
                index = index.to(input_ids.device)
                out[index] = self.forward_packed(input_ids.reshape(-1)[index], cu.to(input_ids.device), int(lengths.max()), positions.to(input_ids.device))
            return _Output(out.view(B, S, d))
        cos, sin = self._rope(S, input_ids.device)
        return _Output(self._layers(self._embed(input_ids), cos, sin, lambda qkv: ops.attention(*qkv.view(B, S, 3, H, 64).unbind(2))))

    @torch.no_grad()
    def forward_packed(self, input_ids_flat: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int, positions: torch.Tensor) -> torch.Tensor:
        """sequences of their own lengths in one pass: input_ids_flat [T] (sequence i is [cu_seqlens[i], cu_seqlens[i + 1])), cu_seqlens int32 [B + 1] on the device,
        max_seqlen a Python int, positions [T] (each token's index inside its own sequence; `pack_lengths` makes all three) -> [T, hidden] bf16.  The row-wise kernels
        see one batch of T rows; the RoPE tables are gathered by position once per call; attention is `ops.attention_varlen`.  Nothing is read back from the device."""
        if not input_ids_flat.is_cuda:
            raise ops.HipOnly("NewModel: GPU tensors only")
        if input_ids_flat.dim() != 1 or positions.shape != input_ids_flat.shape:
            raise ValueError(f"input_ids_flat and positions: expected two [T] tensors, got {tuple(input_ids_flat.shape)} and {tuple(positions.shape)}")
        T, H = input_ids_flat.numel(), self.config.num_attention_heads
        cos, sin = (t.index_select(0, positions.long()) for t in self._rope(max_seqlen, input_ids_flat.device))
        x = self._layers(self._embed(input_ids_flat[None]), cos, sin,
                         lambda qkv: ops.attention_varlen(*qkv.view(T, 3, H, 64).unbind(1), cu_seqlens, max_seqlen).view(1, T, H * 64))
        return x[0]


def mask_lengths(attention_mask: torch.Tensor) -> torch.Tensor:
    """`attention_mask` [B, S] (nonzero = token; any device) -> the row lengths as a CPU int64 [B], in ONE read-back.  Only right padding is taken: a row must be
    ones followed by zeros (an empty row is allowed)."""
    if attention_mask.dim() != 2:
        raise ValueError(f"attention_mask: expected [B, S], got {tuple(attention_mask.shape)}")
    m = attention_mask != 0
    lengths = m.sum(1)
    prefix = torch.arange(m.shape[1], device=m.device)[None, :] < lengths[:, None]
    host = torch.cat([lengths, (m == prefix).all(1).long()]).cpu()
    lengths, ok = host[:m.shape[0]], host[m.shape[0]:]
    if not bool(ok.all()):
        raise NotImplementedError("attention_mask with a hole or with left padding: only right-padded batches (ones, then zeros, in every row) are packed")
    return lengths


def pack_lengths(lengths, S: Optional[int] = None):
    """host side of the packed layout, CPU tensors in and out: lengths [B] -> (cu_seqlens int32 [B + 1], positions int64 [T], index int64 [T]).  Packed row r belongs
    to sequence i with cu_seqlens[i] <= r < cu_seqlens[i + 1], at position positions[r] of it; index[r] = i * S + positions[r] is its place in a [B, S] padded batch
    flattened to [B * S] rows (S defaults to the longest length) -- the index that gathers the valid tokens out of a padded batch and scatters packed rows back."""
    lengths = torch.as_tensor(lengths, dtype=torch.int64, device="cpu").reshape(-1)
    if lengths.numel() and int(lengths.min()) < 0:
        raise ValueError("pack_lengths: negative length")
    longest = int(lengths.max()) if lengths.numel() else 0
    S = longest if S is None else S
    if S < longest:
        raise ValueError(f"pack_lengths: S = {S} is shorter than the longest sequence ({longest})")
    cu = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
    cu[1:] = lengths.cumsum(0)
    if int(cu[-1]) >= 1 << 31:
        raise ValueError("pack_lengths: more than 2^31 - 1 tokens")
    seq = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    positions = torch.arange(int(cu[-1])) - cu[seq]
    return cu.to(torch.int32), positions, seq * S + positions


def plan_passes(lengths: Sequence[int], order: Sequence[int], max_tokens: int) -> List[List[int]]:
    """cut the texts, taken in `order`, into forward passes of at most `max_tokens` tokens in all; a text longer than the budget is a pass of its own"""
    if max_tokens < 1:
        raise ValueError("max_tokens must be positive")
    passes: List[List[int]] = []
    total = 0
    for i in order:
        if not passes or total + lengths[i] > max_tokens:
            passes.append([])
            total = 0
        passes[-1].append(i)
        total += lengths[i]
    return passes


class _Output(tuple):
    def __new__(cls, hidden):
        o = super().__new__(cls, (hidden,))
        o.last_hidden_state = hidden
        return o


class SentenceEmbedder:
    """text -> fp32 [768] unit vector: what `RAGDatabase(..., embedder=)` / `add_to_db(..., embedder=)` take in place of the reference's LanceDB embedding function.
    `tokenizer(texts) -> list of token-id lists` ([CLS] ... [SEP] included, no padding) is the model's WordPiece tokenizer -- third-party data (vocab.txt), supplied
    by the caller.  packed=False: texts are grouped by token count so that every forward pass is an unpadded batch -- one pass per distinct count.  packed=True:
    texts of all lengths share a pass (`NewModel.forward_packed`): sorted by (token count, token ids), cut into passes of at most `max_tokens` tokens, a longer
    single text being a pass of its own.  The sort keeps the workgroups of an attention launch similar in length and makes the packed input -- so every bit of
    the result -- independent of the order of `texts`."""

    def __init__(self, model: NewModel, tokenizer: Callable[[Sequence[str]], List[List[int]]], normalize: bool = True, max_length: int = 8192,
                 packed: bool = False, max_tokens: int = 32768):
        self.model, self.tokenizer, self.normalize, self.max_length = model, tokenizer, normalize, max_length
        self.packed, self.max_tokens = packed, max_tokens

    def ndims(self) -> int:
        return self.model.config.hidden_size

    def _finish(self, cls: torch.Tensor) -> torch.Tensor:
        cls = cls.float()
        return cls / cls.norm(dim=1, keepdim=True).clamp_min(1e-12) if self.normalize else cls

    @torch.no_grad()
    def encode(self, texts: Sequence[str]) -> torch.Tensor:
        dev = next(self.model.parameters()).device
        ids = [t[:self.max_length] for t in self.tokenizer(list(texts))]
        out = torch.empty(len(ids), self.ndims(), dtype=torch.float32, device=dev)
        if self.packed:
            return self._encode_packed(ids, out)
        by_len: Dict[int, List[int]] = {}
        for i, t in enumerate(ids):
            by_len.setdefault(len(t), []).append(i)
        for n, rows in by_len.items():
            batch = torch.tensor([ids[i] for i in rows], dtype=torch.long, device=dev)
            out[torch.tensor(rows, device=dev)] = self._finish(self.model(batch).last_hidden_state[:, 0])
        return out

    def _encode_packed(self, ids: List[List[int]], out: torch.Tensor) -> torch.Tensor:
        if any(len(t) == 0 for t in ids):
            raise ValueError("SentenceEmbedder: the tokenizer returned an empty token list (every text carries at least [CLS])")
        lengths = [len(t) for t in ids]
        order = sorted(range(len(ids)), key=lambda i: (lengths[i], ids[i]))
        for rows in plan_passes(lengths, order, self.max_tokens):
            cu, positions, _ = pack_lengths([lengths[i] for i in rows])
            flat = torch.tensor([tok for i in rows for tok in ids[i]], dtype=torch.long).to(out.device)
            cu = cu.to(out.device)
            x = self.model.forward_packed(flat, cu, lengths[rows[-1]], positions.to(out.device))
            out[torch.tensor(rows, device=out.device)] = self._finish(x.index_select(0, cu[:-1].long()))        # each sequence's first ([CLS]) row
        return out

    def __call__(self, text: str):
        return self.encode([text])[0].cpu().numpy()
