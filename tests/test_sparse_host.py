"""CPU: the host half of learned sparse encoding -- config and head parsing with every refusal, the tied decoder, the
float64 dot product, ``SparseEncoder`` over a fake encoder (``encode`` / ``score`` / ``predict`` / ``rank`` /
``decode`` / ``expansion`` / ``search_reranked``), the PyTorch reference against the committed transformers goldens, the
sparsity of the synthetic head and the condition of the GPU ranking check."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd import sparse_encoder as se
from claude_semantic_search_amd.tokenizer import HashTokenizer

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402
import splade_reference as sr  # noqa: E402

P = "cls.predictions."


# ---- sparse_dot_numpy -------------------------------------------------------------------------------------------------------
def test_sparse_dot_against_a_dense_dot():
    rng = np.random.default_rng(0)
    for nq, nd, V in [(1, 1, 4), (5, 9, 12), (64, 256, 400), (0, 7, 10)]:
        q = se.SparseVector(rng.permutation(V)[:nq].astype(np.int32), rng.random(nq).astype(np.float32))
        d = se.SparseVector(rng.permutation(V)[:nd].astype(np.int32), rng.random(nd).astype(np.float32))
        dq, dd = np.zeros(V), np.zeros(V)
        dq[q.terms], dd[d.terms] = q.weights, d.weights
        got = se.sparse_dot_numpy(q, d)
        assert got.dtype == np.float32
        assert abs(float(got) - dq @ dd) <= 2.0 ** -23 * max(1.0, dq @ dd)     # one rounding of the float64 sum
    assert se.sparse_dot_numpy(se.SparseVector(np.array([3], np.int32), np.array([2.0], np.float32)),
                               se.SparseVector(np.array([4], np.int32), np.array([5.0], np.float32))) == 0.0


# ---- config and layout ------------------------------------------------------------------------------------------------------
def _config(**over):
    c = {"architectures": ["BertForMaskedLM"], "model_type": "bert", "hidden_act": "gelu", "hidden_size": 384,
         "num_attention_heads": 12, "num_hidden_layers": 6, "intermediate_size": 1536, "vocab_size": 30522,
         "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12, "pad_token_id": 0}
    c.update(over)
    return c


def _dir(tmp_path, **over):
    (tmp_path / "config.json").write_text(json.dumps(_config(**over)))
    return tmp_path


def test_config_of_a_masked_lm_directory(tmp_path):
    cfg = se.parse_sparse_config(_dir(tmp_path))
    assert (cfg["arch"], cfg["hidden"], cfg["num_layers"], cfg["vocab"]) == ("bert", 384, 6, 30522)


@pytest.mark.parametrize("over,field", [({"model_type": "mpnet"}, "model_type"), ({"model_type": "distilbert"}, "model_type"),
                                        ({"hidden_act": "relu"}, "hidden_act"), ({"hidden_size": 512}, "hidden_size"),
                                        ({"num_attention_heads": 4}, "head_dim"), ({"type_vocab_size": 1}, "type_vocab_size"),
                                        ({"position_embedding_type": "relative_key"}, "position_embedding_type")])
def test_config_refusals_name_the_field(tmp_path, over, field):
    with pytest.raises(ValueError, match=field):
        se.parse_sparse_config(_dir(tmp_path, **over))


def _state_dict(H=384, V=50, tied=True, bias="bias", prefix="bert."):
    rng = np.random.default_rng(1)
    sd = {prefix + "embeddings.word_embeddings.weight": rng.random((V, H)).astype(np.float32),
          P + "transform.dense.weight": rng.random((H, H)).astype(np.float32),
          P + "transform.dense.bias": rng.random(H).astype(np.float32),
          P + "transform.LayerNorm.weight": rng.random(H).astype(np.float32),
          P + "transform.LayerNorm.bias": rng.random(H).astype(np.float32)}
    b = rng.random(V).astype(np.float32)
    for name in bias.split("+"):
        sd[P + name] = b.copy()
    if not tied:
        sd[P + "decoder.weight"] = rng.random((V, H)).astype(np.float32)
    return sd


def test_layout_of_the_state_dict():
    for tied in (True, False):
        for bias in ("bias", "decoder.bias", "bias+decoder.bias"):
            sd = _state_dict(tied=tied, bias=bias)
            body, head = se.split_mlm_head(sd, 384, 50)
            assert list(body) == ["bert.embeddings.word_embeddings.weight"]
            assert (head["decoder_w"] is None) == tied
            assert np.array_equal(head["decoder_b"], sd[P + bias.split("+")[0]])
            assert head["dense_w"].shape == (384, 384) and head["ln_g"].shape == (384,)
    # names that carry "bert." on the head as well
    sd = {("bert." + k if k.startswith("cls.") else k): v for k, v in _state_dict().items()}
    body, head = se.split_mlm_head(sd, 384, 50)
    assert len(body) == 1 and head["dense_b"].shape == (384,)


def test_layout_refusals_name_the_tensor():
    for key in ("transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight", "transform.LayerNorm.bias"):
        sd = _state_dict()
        del sd[P + key]
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            se.split_mlm_head(sd, 384, 50)
        sd = _state_dict()
        sd[P + key] = np.zeros((3, 5), np.float32)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            se.split_mlm_head(sd, 384, 50)
    sd = _state_dict()
    del sd[P + "bias"]
    with pytest.raises(ValueError, match=r"cls\.predictions\.bias"):
        se.split_mlm_head(sd, 384, 50)
    sd = _state_dict(bias="bias+decoder.bias")
    sd[P + "decoder.bias"][7] += 1
    with pytest.raises(ValueError, match="differ"):
        se.split_mlm_head(sd, 384, 50)
    sd = _state_dict(tied=False)
    sd[P + "decoder.weight"] = np.zeros((51, 384), np.float32)
    with pytest.raises(ValueError, match=r"decoder\.weight"):
        se.split_mlm_head(sd, 384, 50)
    with pytest.raises(ValueError, match=r"cls\.predictions\.bias of shape"):
        se.split_mlm_head(_state_dict(V=49), 384, 50)
    with pytest.raises(ValueError, match="seq_relationship|unsupported tensor"):
        se.split_mlm_head(dict(_state_dict(), **{P + "extra": np.zeros(1, np.float32)}), 384, 50)


def test_synthetic_head_is_the_reference_one_and_tied():
    cfg = br.BertCfg(num_layers=1, vocab=1000, **br.SMALL)
    w = sr.synth_weights(cfg, 7)
    h = se.synth_mlm_head(384, 1000, 7)
    assert h["decoder_w"] is None and sr.decoder(w) is w["embeddings.word_embeddings.weight"]
    assert np.array_equal(h["dense_w"], w[P + "transform.dense.weight"].numpy())
    assert np.array_equal(h["decoder_b"], w[P + "bias"].numpy())
    assert abs(float(h["decoder_b"].mean()) - se.SYNTH_BIAS_SIGMAS * 0.02 * np.sqrt(384)) < 0.01


# ---- SparseEncoder over a fake encoder ----------------------------------------------------------------------------------------
class FakeEncoder:
    """The sparse surface of MpnetEncoder on the PyTorch reference (1 layer, 600 terms); counts what it encodes."""

    def __init__(self):
        self.rcfg = br.BertCfg(num_layers=1, vocab=600, pooling="cls", normalize=False, **br.SMALL)
        self.cfg = self.rcfg.encoder_overrides()
        self.w = sr.synth_weights(self.rcfg, 5, bias_sigmas=-2.0)
        self.tokenizer = HashTokenizer(600)
        self.max_seq_length = 64
        self.encoded = []
        self.closed = False

    def tokenize(self, texts):
        return [self.tokenizer.encode(t, 64) for t in texts]

    def encode_sparse_ids(self, batch, m, return_dense=False, return_rows=False):
        self.encoded += [tuple(ids) for ids in batch]
        tops = [sr.topm(sr.sparse(self.w, self.rcfg, ids)["z"], m) for ids in batch]
        return (np.stack([t[0] for t in tops]), np.stack([t[1] for t in tops]), np.array([t[2] for t in tops], np.int32))

    def close(self):
        self.closed = True


@pytest.fixture(scope="module")
def fake():
    return FakeEncoder()


TEXTS = ["alpha beta gamma", "delta", "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu", "beta beta beta"]


def test_encode_returns_vectors_in_input_order(fake):
    enc = se.SparseEncoder(None, encoder=fake)
    vecs = enc.encode(TEXTS, batch_size=2, max_terms=16)
    for text, v in zip(TEXTS, vecs):
        t, w, nnz = sr.topm(sr.sparse(fake.w, fake.rcfg, fake.tokenizer.encode(text, 64))["z"], 16)
        k = min(16, nnz)
        assert v.terms.dtype == np.int32 and v.weights.dtype == np.float32
        assert np.array_equal(v.terms, t[:k]) and np.array_equal(v.weights, w[:k])
        assert np.all(np.diff(v.weights) <= 0) and (v.weights > 0).all()
    assert len(enc.encode_queries(TEXTS[:1])[0].terms) <= 64 and len(enc.encode_documents(TEXTS[:1])[0].terms) <= 256
    with pytest.raises(ValueError, match="max_terms"):
        enc.encode(TEXTS, max_terms=513)
    enc.close()
    assert not fake.closed                                   # an injected encoder stays the caller's


def test_score_predict_and_query_deduplication(fake):
    enc = se.SparseEncoder(None, encoder=fake)
    q, d = enc.encode_queries(TEXTS[:2]), enc.encode_documents(TEXTS)
    s = enc.score(q, d)
    assert s.shape == (8,) and s.dtype == np.float32
    assert all(s[i * 4 + j] == se.sparse_dot_numpy(q[i], d[j]) for i in range(2) for j in range(4))
    assert np.array_equal(enc.score(q, d, [(1, 2), (0, 0)]), s[[6, 0]])
    fake.encoded.clear()
    pairs = [(TEXTS[0], TEXTS[2]), (TEXTS[1], TEXTS[0]), (TEXTS[0], TEXTS[3]), (TEXTS[0], TEXTS[1])]
    got = enc.predict(pairs, batch_size=3)
    assert np.array_equal(got, np.array([s[2], s[4], s[3], s[1]], np.float32))
    assert len(fake.encoded) == 2 + 4                        # two distinct queries once each, every text once
    assert enc.predict([]).shape == (0,)
    with pytest.raises(ValueError, match="activation"):
        enc.predict(pairs, activation="sigmoid")


def test_rank_orders_by_score_and_ties_go_to_the_lower_id(fake):
    enc = se.SparseEncoder(None, encoder=fake)
    docs = [TEXTS[2], TEXTS[0], TEXTS[2], TEXTS[1]]          # documents 0 and 2 tie exactly
    hits = enc.rank(TEXTS[0], docs, return_documents=True)
    scores = enc.predict([(TEXTS[0], t) for t in docs])
    assert [h["corpus_id"] for h in hits] == sorted(range(4), key=lambda i: (-scores[i], i))
    assert hits[0]["text"] == docs[hits[0]["corpus_id"]]
    pos = {h["corpus_id"]: n for n, h in enumerate(hits)}
    assert scores[0] == scores[2] and pos[0] < pos[2]
    assert len(enc.rank(TEXTS[0], docs, top_k=2)) == 2


def test_decode_and_expansion(fake):
    enc = se.SparseEncoder(None, encoder=fake)
    v = enc.encode([TEXTS[2]])[0]
    dec = enc.decode(v, 5)
    assert dec == [(f"#{int(t)}", float(w)) for t, w in zip(v.terms[:5], v.weights[:5])]
    assert len(enc.decode(v)) == len(v.terms)
    own = set(fake.tokenizer.encode(TEXTS[2], 64))
    exp = enc.expansion(TEXTS[2], n=4)
    assert 0 < len(exp) <= 4 and all(int(w[1:]) not in own for w, _ in exp)
    assert [w for w, _ in exp] == [f"#{int(t)}" for t in v.terms if int(t) not in own][:4]

    class Words:                                             # a tokenizer with a word list
        vocab = {f"word{i}": i for i in range(600)}
    enc.tokenizer = Words()
    assert enc.decode(v, 1)[0][0] == f"word{int(v.terms[0])}"


def test_search_reranked_accepts_a_sparse_encoder(fake):
    """HybridStorage.search_reranked asks its reranker for predict(pairs) alone."""
    import inspect

    from claude_semantic_search_amd.storage import HybridStorage

    src = inspect.getsource(HybridStorage.search_reranked)
    assert "reranker.predict(" in src and "reranker.encoder" not in src and "score_pair_ids" not in src
    enc = se.SparseEncoder(None, encoder=fake)
    assert enc.predict([(TEXTS[0], TEXTS[2])]).shape == (1,)


# ---- the reference against the transformers goldens ---------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["small", "base"])
def test_reference_against_goldens(geo):
    g = np.load(HERE / "golden" / f"splade_{geo}_2layer.npz")
    cfg = br.BertCfg(num_layers=int(g["num_layers"]), pooling="cls", **sr.GEOS[geo])
    w = sr.synth_weights(cfg, int(g["wseed"]))
    batch = br.synth_batch(cfg, g["lengths"].tolist(), int(g["bseed"]))
    umin = np.inf
    for b, ids in enumerate(batch):
        r = sr.sparse(w, cfg, ids)
        umin = min(umin, r["umin"])
        assert int((r["z"] > 0).sum()) == int(g["nnz"][b]) or abs(int((r["z"] > 0).sum()) - int(g["nnz"][b])) <= 2
        k = min(32, int(g["nnz"][b]))
        # every golden term carries the golden weight to 1e-5 (the order of near-equal weights may differ)
        assert np.abs(r["w"][g["terms"][b][:k]] - g["weights"][b][:k]).max() <= 1e-5
        assert abs(float(r["w"].astype(np.float64).sum()) - float(g["wsum"][b])) <= 1e-5 * max(1, int(g["nnz"][b]))
    assert abs(umin - float(g["umin"])) <= 1e-4


# ---- the synthetic head is sparse on both sides of the cut --------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["small", "base"])
def test_synthetic_documents_split_at_the_cut(geo):
    """With the reference alone: of the GPU tests' documents some have nnz > m (the cut binds) and some 0 < nnz < m (the
    padding binds), m = 256."""
    cfg = br.BertCfg(num_layers=2, pooling="cls", **sr.GEOS[geo])
    w = sr.synth_weights(cfg, sr.WSEEDS[geo])
    lens = sorted({n for case in sr.CASES for n in case})
    nnz = [int((sr.sparse(w, cfg, ids)["z"] > 0).sum()) for ids in br.synth_batch(cfg, lens, sr.BSEED)]
    print(f"[sparse] {geo}: lengths {lens} -> nnz {nnz}")
    assert sum(n > sr.M for n in nnz) >= 3 and sum(0 < n < sr.M for n in nnz) >= 3 and min(nnz) > 0


# ---- the ranking check of the end-to-end GPU test binds -----------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["bf16", "fp32"])
@pytest.mark.parametrize("tied", [True, False], ids=["tied", "untied"])
def test_ranking_check_binds(tied, compute):
    """Counts, with the reference alone, the adjacent document pairs (in the reference's order) whose scores differ by
    more than twice the score bar, for every leg of the end-to-end GPU test (tied and untied decoder, both compute
    modes, each at the z bar that leg runs under: ``splade_reference.e2e_z_bar``): the GPU test compares the order on
    exactly those, through the same ``e2e_ranking``.  Most must be bound (more than half: at least 2 of the 3), or the
    check would say little."""
    cfg = sr.e2e_cfg()
    w = sr.e2e_weights(tied)
    rq = sr.sparse(w, cfg, sr.e2e_ids(sr.E2E_QUERY))
    rd = [sr.sparse(w, cfg, sr.e2e_ids(t)) for t in sr.e2e_documents()]
    zbar = sr.e2e_z_bar(w, compute, [rq] + rd)
    scores, bars, order, bound = sr.e2e_ranking(rq, rd, zbar)
    nnz = [int((r["z"] > 0).sum()) for r in [rq] + rd]
    print(f"[sparse] end-to-end {'tied' if tied else 'untied'} {compute}: z bar {zbar:.3e}, nnz {nnz}, score bars "
          f"{np.round(bars[order], 4).tolist()}, scores {np.round(scores[order], 4).tolist()}, bound pairs "
          f"{int(bound.sum())} of {bound.size}")
    assert min(nnz) >= 6        # every text has terms to decode, the last six beyond its own words
    assert bound.size == 3 and int(bound.sum()) >= 2
