"""The text embedder's packed path on the GPU (reduced model of test_gpu_text_embedder.py): NewModel.forward on a right-padded batch against the oracle with the
same attention mask; SentenceEmbedder(packed=True) against the oracle, against the grouped path and under a shuffle of its input; how many varlen attention
launches an encode makes; a packed database searched end to end."""
import random

import pytest
import torch

from oracle import gte_ref as R
from test_gpu_text_embedder import SMALL, _model, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


def tok(texts):                                                                # the stand-in WordPiece of test_gpu_text_embedder.py: [CLS], one id per word, [SEP]
    return [[101] + [2 + (sum(map(ord, w)) % 500) for w in t.split()] + [102] for t in texts]


def _texts(n=40, seed=0):
    rng = random.Random(seed)
    words = ["dog", "runs", "pour", "milk", "bowl", "cat", "sleeps", "cut", "onion", "open", "door", "slowly", "walk", "stir", "a", "the", "into", "and"]
    texts = [" ".join(rng.choice(words) + str(rng.randint(0, 99)) for _ in range(rng.randint(1, 60))) for _ in range(n - 2)]
    return texts + ["stir", texts[3]]                                          # a 1-word text and a duplicate


@pytest.fixture(scope="module")
def small():
    m, sd = _model(SMALL, 5)
    texts = _texts()
    want = torch.cat([R.sentence_embedding(sd, SMALL, torch.tensor(tok([t]))) for t in texts])          # computed once, never written to
    return m, sd, texts, want


def test_padded_forward_matches_the_oracle(hip):
    m, sd = _model(SMALL, 3)
    lengths = [5, 37, 1, 64, 70]
    ids = torch.randint(1, 512, (5, 70), generator=torch.Generator().manual_seed(70))
    mask = (torch.arange(70)[None, :] < torch.tensor(lengths)[:, None]).long()
    ids = ids * mask                                                           # [PAD] = 0 at the padded positions, as a tokenizer leaves them
    want = R.encoder(sd, SMALL, ids, mask)
    got = m(ids.to(DEV), attention_mask=mask.to(DEV)).last_hidden_state
    assert got.shape == (5, 70, 128) and got.dtype == torch.bfloat16
    valid = mask.bool()
    assert rel(got.cpu()[valid], want[valid]) < 2e-2
    for b, n in enumerate(lengths):                                            # and row by row: a short row cannot hide behind a long one
        assert rel(got[b, :n], want[b, :n]) < 2e-2, (b, n)
    assert (got.cpu()[~valid] == 0).all()                                      # exact zeros at the padded positions
    for bad in ([[1, 0, 1]], [[0, 1, 1]]):                                     # a hole, left padding
        with pytest.raises(NotImplementedError, match="hole|left padding"):
            m(torch.ones(1, 3, dtype=torch.long, device=DEV), attention_mask=torch.tensor(bad, device=DEV))


def test_all_ones_mask_launches_what_no_mask_launches(hip):
    from motionrag_amd import ops
    m, _ = _model(SMALL, 3)
    ids = torch.randint(1, 512, (3, 37), generator=torch.Generator().manual_seed(1)).to(DEV)
    m(ids)
    before = ops.attn_varlen_launch_counts()
    with ops.dispatched() as plain:
        a = m(ids)[0]
    with ops.dispatched() as ones:
        b = m(ids, attention_mask=torch.ones_like(ids))[0]
    assert plain.counts == ones.counts and plain.counts and torch.equal(a, b)
    assert ops.attn_varlen_launch_counts() == before


def test_packed_encode_matches_oracle_grouped_path_and_any_order(hip, small):
    from motionrag_amd.text_embedder import SentenceEmbedder
    m, _, texts, want = small
    E = SentenceEmbedder(m, tok, packed=True).encode(texts)
    G = SentenceEmbedder(m, tok).encode(texts)
    assert E.shape == (len(texts), 128) and E.dtype == torch.float32
    assert torch.allclose(E.norm(dim=1), torch.ones(len(texts), device=DEV), atol=1e-5)
    for i in range(len(texts)):
        assert rel(E[i:i + 1], want[i:i + 1]) < 1.5e-2, i
        assert rel(E[i:i + 1], G[i:i + 1]) < 1.5e-2, i
    # the packed input is sorted by (token count, token ids): it is the same tensor for every order of `texts`, so the rows are the same bits
    perm = list(range(len(texts)))
    random.Random(3).shuffle(perm)
    assert torch.equal(SentenceEmbedder(m, tok, packed=True).encode([texts[i] for i in perm]), E[torch.tensor(perm, device=DEV)])
    small_budget = SentenceEmbedder(m, tok, packed=True, max_tokens=64).encode(texts)                   # other passes, the same embeddings
    for i in range(len(texts)):
        assert rel(small_budget[i:i + 1], want[i:i + 1]) < 1.5e-2, i


def test_launch_counts_per_encode(hip, small):
    from motionrag_amd import ops
    from motionrag_amd.text_embedder import SentenceEmbedder, plan_passes
    m, _, texts, _ = small
    layers = SMALL["num_hidden_layers"]
    n0 = ops.attn_varlen_launch_counts()
    SentenceEmbedder(m, tok, packed=True).encode(texts)                                                 # everything inside one 32 768-token budget
    n1 = ops.attn_varlen_launch_counts()
    assert n1 - n0 == layers
    lengths = [len(t) for t in tok(texts)]
    passes = plan_passes(lengths, sorted(range(len(texts)), key=lambda i: lengths[i]), 64)
    assert len(passes) > 3
    SentenceEmbedder(m, tok, packed=True, max_tokens=64).encode(texts)
    n2 = ops.attn_varlen_launch_counts()
    assert n2 - n1 == layers * len(passes)
    SentenceEmbedder(m, tok).encode(texts)                                                              # packed=False: the grouped path, no varlen launch
    assert ops.attn_varlen_launch_counts() == n2


def test_packed_database_end_to_end(hip, small, tmp_path):
    from motionrag_amd import rag
    from motionrag_amd.text_embedder import SentenceEmbedder
    m = small[0]
    emb = SentenceEmbedder(m, tok, packed=True)
    texts = ["a dog runs", "pour the milk into the bowl", "a cat sleeps", "cut the onion", "open the door slowly and walk in", "stir"]
    annos = [{"llm_caption": t, "id": i, "video": f"v{i}.mp4", "start_sec": 0.0, "end_sec": 1.0} for i, t in enumerate(texts)]
    rag.add_to_db(rag.prepare_annotations(annos), embedder=emb, db_path=str(tmp_path))
    db = rag.RAGDatabase(str(tmp_path), "llm_caption", device="cuda", embedder=emb)
    hits = db.text_search("cut the onion", top_k=2)
    assert hits[0]["text"] == "cut the onion" and hits[0]["_distance"] < 1e-3
