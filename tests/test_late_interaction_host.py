"""CPU: the host half of late-interaction re-ranking -- the float64 score, ids (markers, truncation, skiplist), config
and layout refusals, ``predict`` / ``rank`` / ``search_reranked`` over a fake encoder, the PyTorch reference against the
committed transformers goldens, and the condition of the GPU ranking check."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd import late_interaction as li
from claude_semantic_search_amd.tokenizer import HashTokenizer

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402
import li_reference as lr  # noqa: E402


# ---- maxsim_numpy ---------------------------------------------------------------------------------------------------------
def test_maxsim_numpy_against_a_triple_loop():
    rng = np.random.default_rng(0)
    for mq, md, P in [(1, 1, 32), (3, 7, 32), (17, 33, 96), (64, 5, 128)]:
        q, d = rng.standard_normal((mq, P)), rng.standard_normal((md, P))
        keep = rng.integers(0, 2, md)
        keep[int(rng.integers(0, md))] = 1
        for kp in (None, keep):
            want = 0.0
            for s in range(mq):
                best = -np.inf
                for t in range(md):
                    if kp is not None and not kp[t]:
                        continue
                    dot = 0.0
                    for c in range(P):
                        dot += q[s, c] * d[t, c]
                    best = max(best, dot)
                want += best
            assert abs(li.maxsim_numpy(q, d, kp) - want) <= 1e-12 * mq * P
    with pytest.raises(ValueError, match="no kept token"):
        li.maxsim_numpy(np.ones((2, 4)), np.ones((3, 4)), [0, 0, 0])
    with pytest.raises(ValueError, match="2 keep flags for 3 doc tokens"):
        li.maxsim_numpy(np.ones((2, 4)), np.ones((3, 4)), [1, 0])


def test_bf16_conversions_round_to_nearest_even():
    import torch

    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32)
    x[:4] = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 2.0 ** -126]      # two ties, a signed zero, the smallest normal
    want = torch.from_numpy(x).bfloat16()
    assert np.array_equal(li.f32_to_bf16(x), want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(li.bf16_to_f32(li.f32_to_bf16(x)), want.float().numpy())
    assert li.maxsim_numpy(li.f32_to_bf16(x[:64].reshape(2, 32)), li.f32_to_bf16(x[64:160].reshape(3, 32))) == \
        li.maxsim_numpy(want.float().numpy()[:64].reshape(2, 32), want.float().numpy()[64:160].reshape(3, 32))


# ---- ids --------------------------------------------------------------------------------------------------------------------
def test_markers_truncation_and_the_skiplist():
    ids = [101] + list(range(1000, 1010)) + [102]
    assert li.build_side(ids, 1, 64) == [101, 1] + ids[1:]
    assert li.build_side(ids, None, 64) == ids
    assert li.build_side(ids, 2, 13) == [101, 2] + ids[1:]                  # exactly the limit: nothing dropped
    assert li.build_side(ids, 2, 8) == [101, 2, 1000, 1001, 1002, 1003, 1004, 102]
    assert li.build_side(ids, None, 5) == [101, 1000, 1001, 1002, 102]
    assert li.build_side([101, 102], 1, 3) == [101, 1, 102]
    with pytest.raises(ValueError, match="max_length=2"):
        li.build_side(ids, 1, 2)
    k = li.keep_flags([101, 2, 1000, 1012, 1001, 1013, 102], {1012, 1013})
    assert k.dtype == np.uint8 and k.tolist() == [1, 1, 1, 0, 1, 0, 1]
    assert li.keep_flags([5, 6], ()).tolist() == [1, 1]


# ---- config and layout ------------------------------------------------------------------------------------------------------
def _config(**over):
    c = {"architectures": ["HF_ColBERT"], "model_type": "bert", "hidden_act": "gelu", "hidden_size": 384,
         "num_attention_heads": 12, "num_hidden_layers": 6, "intermediate_size": 1536, "vocab_size": 30522,
         "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12, "pad_token_id": 0}
    c.update(over)
    return c


def _dir(tmp_path, **over):
    (tmp_path / "config.json").write_text(json.dumps(_config(**over)))
    return tmp_path


def test_config_of_a_colbert_directory(tmp_path):
    cfg = li.parse_late_interaction_config(_dir(tmp_path))
    assert (cfg["arch"], cfg["hidden"], cfg["num_layers"], cfg["pooling"]) == ("bert", 384, 6, "cls")


@pytest.mark.parametrize("over,field", [({"model_type": "mpnet"}, "model_type"), ({"model_type": "roberta"}, "model_type"),
                                        ({"hidden_act": "relu"}, "hidden_act"), ({"hidden_size": 512}, "hidden_size"),
                                        ({"num_attention_heads": 4}, "head_dim"), ({"type_vocab_size": 1}, "type_vocab_size"),
                                        ({"position_embedding_type": "relative_key"}, "position_embedding_type")])
def test_config_refusals_name_the_field(tmp_path, over, field):
    with pytest.raises(ValueError, match=field):
        li.parse_late_interaction_config(_dir(tmp_path, **over))


def test_layout_of_the_state_dict():
    sd = {"bert.embeddings.word_embeddings.weight": np.zeros((10, 384), np.float32),
          "linear.weight": np.ones((96, 384), np.float32)}
    body, W = li.split_projection(sd, 384)
    assert list(body) == ["bert.embeddings.word_embeddings.weight"] and W.shape == (96, 384)
    body, W = li.split_projection({k: v for k, v in sd.items() if k != "linear.weight"}, 384)
    assert W is None and len(body) == 1                                      # no projection: P = H
    for shape in [(96, 768), (100, 384), (160, 384), (16, 384), (384,)]:
        with pytest.raises(ValueError, match="linear.weight"):
            li.split_projection({"linear.weight": np.zeros(shape, np.float32)}, 384)
    with pytest.raises(ValueError, match="linear.bias"):
        li.split_projection(dict(sd, **{"linear.bias": np.zeros(96, np.float32)}), 384)


def test_synthetic_projection_is_the_reference_one():
    w = lr.synth_weights(br.BertCfg(num_layers=1, vocab=1000, **br.SMALL), 7, 96)
    assert np.array_equal(li.synth_projection(384, 96, 7), w["linear.weight"].numpy())


# ---- a fake encoder -----------------------------------------------------------------------------------------------------------
class FakeEncoder:
    """The late-interaction surface of MpnetEncoder on the host: a token's vector depends on its id and position."""

    P = 32

    def __init__(self):
        self.cfg = dict(vocab=30522, pad_id=0, max_seq_len=64, hidden=384)
        self.tokenizer = HashTokenizer(30522)
        self.token_dim = self.P
        self.calls = []
        self.closed = False

    def tokenize(self, texts):
        return [self.tokenizer.encode(t, 64) for t in texts]

    def _vec(self, tok, pos):
        v = np.random.default_rng(tok * 131 + pos).standard_normal(self.P)
        return li.f32_to_bf16((v / np.linalg.norm(v)).astype(np.float32))

    def encode_tokens_ids(self, batch, normalize=True):
        self.calls.append(("tokens", [list(s) for s in batch]))
        return [np.stack([self._vec(t, p) for p, t in enumerate(s)]) for s in batch]

    def maxsim(self, q_mats, d_mats, pairs=None, keep=None):
        if pairs is None:
            pairs = [(i, j) for i in range(len(q_mats)) for j in range(len(d_mats))]
        return np.array([li.maxsim_numpy(q_mats[i], d_mats[j], None if keep is None else keep[j]) for i, j in pairs],
                        dtype=np.float32)

    def score_late_ids(self, batch, q_mats, pairs=None, keep=None):
        self.calls.append(("late", [list(s) for s in batch], len(q_mats)))
        d = [np.stack([self._vec(t, p) for p, t in enumerate(s)]) for s in batch]
        return self.maxsim(q_mats, d, pairs, keep)

    def close(self):
        self.closed = True


PAIRS = [("how do kernels launch", "a kernel is launched on a stream, with a grid."),
         ("what is lds", "lds is memory shared by a block"),
         ("how do kernels launch", "x " * 80),
         ("what is lds", "short"),
         ("how do kernels launch", "lds is memory shared by a block")]


def test_predict_encodes_each_query_once_and_returns_input_order():
    fake = FakeEncoder()
    model = li.LateInteraction(None, encoder=fake, query_length=8, document_length=40, skip_ids=[fake.tokenizer.encode(",")[1]])
    out = model.predict(PAIRS, batch_size=2)
    token_calls = [c for c in fake.calls if c[0] == "tokens"]
    assert len(token_calls) == 1 and len(token_calls[0][1]) == 2             # two distinct queries, one batch
    late = [c for c in fake.calls if c[0] == "late"]
    lens = [len(s) for c in late for s in c[1]]
    assert lens == sorted(lens, reverse=True) and max(lens) == 40 and len(late) == 3
    # input order: each score is the float64 MaxSim of its own pair
    q_ids, d_ids = model.query_ids([p[0] for p in PAIRS]), model.document_ids([p[1] for p in PAIRS])
    assert all(len(q) <= 8 and q[1] == 1 for q in q_ids) and all(d[1] == 2 for d in d_ids)
    for n in range(len(PAIRS)):
        qm = np.stack([fake._vec(t, p) for p, t in enumerate(q_ids[n])])
        dm = np.stack([fake._vec(t, p) for p, t in enumerate(d_ids[n])])
        assert out[n] == np.float32(li.maxsim_numpy(qm, dm, li.keep_flags(d_ids[n], model.skip_ids)))
    assert out.dtype == np.float32 and model.predict([]).shape == (0,)
    with pytest.raises(ValueError, match="activation"):
        model.predict(PAIRS, activation="sigmoid")
    # kept matrices give the same scores without the forward path
    qm, _ = model.encode_queries(["what is lds"])
    dm, keep = model.encode_documents([PAIRS[1][1], PAIRS[3][1]])
    assert np.array_equal(model.score(qm, dm, keep=keep), out[[1, 3]])


def test_rank_has_the_shape_of_cross_encoder_rank():
    model = li.LateInteraction(None, encoder=FakeEncoder())
    docs = [p[1] for p in PAIRS]
    hits = model.rank("what is lds", docs, top_k=3, return_documents=True)
    assert len(hits) == 3 and set(hits[0]) == {"corpus_id", "score", "text"}
    assert all(hits[i]["score"] >= hits[i + 1]["score"] for i in range(2)) and hits[0]["text"] == docs[hits[0]["corpus_id"]]
    assert hits[0]["corpus_id"] in (1, 4)                                  # the two copies of the matching text tie: lower id
    assert hits[0]["corpus_id"] == 1


def test_knobs_are_checked():
    for kw, msg in [(dict(query_length=65), "query_length=65"), (dict(query_length=2), "query_length=2"),
                    (dict(document_length=65), "document_length=65"), (dict(query_marker_id=0), "query_marker_id=0"),
                    (dict(document_marker_id=40000), "document_marker_id=40000")]:
        with pytest.raises(ValueError, match=msg):
            li.LateInteraction(None, encoder=FakeEncoder(), **kw)
    fake = FakeEncoder()
    with pytest.raises(ValueError, match="query_length=65"):
        li.LateInteraction(None, encoder=fake, query_length=65)
    assert not fake.closed                                                   # a caller's encoder stays open ...
    m = li.LateInteraction(None, encoder=fake, query_marker_id=None, document_marker_id=None)
    assert m.query_ids(["a b"])[0] == FakeEncoder().tokenize(["a b"])[0]
    m.close()
    assert not fake.closed                                                   # ... also after close()


def test_search_reranked_takes_a_late_interaction_model(tmp_path):
    from claude_semantic_search_amd.storage import HybridStorage, Reranked, SearchConfig, SearchResult

    model = li.LateInteraction(None, encoder=FakeEncoder())
    texts = [p[1] for p in PAIRS]
    hits = [SearchResult(chunk_id=f"c{i}", similarity=1.0 - 0.1 * i, text=t) for i, t in enumerate(texts)]

    class Store:
        search_reranked = HybridStorage.search_reranked

        def search(self, query_embedding, cfg, filters):
            return [SearchResult(chunk_id=h.chunk_id, similarity=h.similarity, text=h.text) for h in hits]

    res = Store().search_reranked("what is lds", None, model, SearchConfig(top_k=3), None, fetch=5)
    want = model.predict([("what is lds", t) for t in texts])
    assert len(res) == 3 and all(isinstance(r, Reranked) for r in res)
    assert [r.rank_before for r in res] == np.argsort(-want, kind="stable")[:3].tolist()
    assert [r.score for r in res] == [float(want[r.rank_before]) for r in res]


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,geo", [("li_small_2layer", "small"), ("li_base_2layer", "base")])
def test_reference_matches_the_transformers_goldens(name, geo):
    g = np.load(HERE / "golden" / f"{name}.npz")
    cfg = br.BertCfg(num_layers=int(g["num_layers"]), pooling="cls", **lr.GEOS[geo])
    w = lr.synth_weights(cfg, int(g["wseed"]), int(g["width"]))
    batch = br.synth_batch(cfg, g["lengths"].tolist(), int(g["bseed"]))
    qb = br.synth_batch(cfg, g["query_lengths"].tolist(), int(g["qseed"]))
    rd, rq = [lr.token_vectors(w, cfg, ids) for ids in batch], [lr.token_vectors(w, cfg, ids) for ids in qb]
    pairs = [(i, j) for i in range(len(qb)) for j in range(len(batch))]
    assert np.abs(rd[0] - g["tokens0"]).max() <= 1e-5
    assert np.abs(lr.scores(rq, rd, pairs) - g["scores"].reshape(-1)).max() <= 1e-5
    # the reference's fp32 scorer against the float64 restatement of the product
    want = np.array([li.maxsim_numpy(rq[i], rd[j]) for i, j in pairs])
    assert np.abs(lr.scores(rq, rd, pairs) - want).max() <= 1e-5


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_ranking_check_binds(geo, compute):
    """The GPU ranking check compares orders only where the reference scores differ by more than twice the bar: with
    the reference alone, that binds at least half of the adjacent pairs of RANK_CASE in both modes."""
    cfg = br.BertCfg(num_layers=2, pooling="cls", **lr.GEOS[geo])
    w = lr.synth_weights(cfg, lr.WSEEDS[geo], lr.WIDTH[geo])
    q_ids = lr.queries(cfg)[2]
    docs = br.synth_batch(cfg, lr.RANK_CASE, lr.BSEED)
    q, d = lr.token_vectors(w, cfg, q_ids), [lr.token_vectors(w, cfg, ids) for ids in docs]
    vmin = min(float(np.linalg.norm(lr.token_vectors(w, cfg, ids, normalize=False), axis=1).min())
               for ids in docs + lr.queries(cfg))
    eps = lr.fp32_token_eps(w, cfg, vmin)
    bar = lr.BF16_SCORE_BAR if compute == "bf16" else lr.fp32_score_bar(eps, eps, len(q_ids), lr.WIDTH[geo])
    ref = lr.scores([q], d, [(0, j) for j in range(len(d))])
    _, mask = lr.binding_pairs(ref, bar)
    print(f"[li host] {geo} {compute}: bar {bar:.3e}, binds {int(mask.sum())} of {mask.size}")
    assert 2 * int(mask.sum()) >= mask.size
