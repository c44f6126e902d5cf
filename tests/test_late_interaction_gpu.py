"""GPU: late-interaction token vectors and scores (css_encoder_forward_tokens / css_encoder_maxsim /
css_encoder_forward_maxsim, LateInteraction, search_reranked) against the fp32 PyTorch reference
(tests/li_reference.py) and the committed transformers goldens.

Bars (tests/li_reference.py): fp32 mode the 1e-4 hidden-state bar pushed through projection, normalisation and the dot
(``fp32_token_eps`` / ``fp32_cos_bar`` / ``fp32_score_bar``, computed from the case's weights); bf16 mode
``BF16_COS_BAR`` / ``BF16_SCORE_BAR`` = 2 x the largest figure measured on the device over the cases of tests 4 and 5
(2-layer models), ``BF16_*_BAR_6LAYER`` = 2 x the figure of test 8 (DESIGN.md 3.3d has the per-test maxima).  Every
test prints its figures before it asserts."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd.late_interaction import bf16_to_f32
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402
import li_reference as lr  # noqa: E402

pytestmark = pytest.mark.gpu


def _cfg(geo, layers=2, vocab=30522):
    return br.BertCfg(num_layers=layers, vocab=vocab, pooling="cls", **lr.GEOS[geo])


@functools.lru_cache(maxsize=None)
def _weights(geo, proj=True):
    return lr.synth_weights(_cfg(geo), lr.WSEEDS[geo], lr.WIDTH[geo] if proj else None)


@functools.lru_cache(maxsize=None)
def _side(geo, proj, lens, seed):
    """(batch, reference unit token matrices, smallest reference ||v|| before normalisation); computed once, shared."""
    cfg, w = _cfg(geo), _weights(geo, proj)
    batch = br.synth_batch(cfg, list(lens), seed)
    ref = [lr.token_vectors(w, cfg, ids) for ids in batch]
    vmin = min(float(np.linalg.norm(lr.token_vectors(w, cfg, ids, normalize=False), axis=1).min()) for ids in batch)
    return batch, ref, vmin


def _queries(geo, proj):
    return _side(geo, proj, tuple(lr.QUERY_LENS), lr.QSEED)


def _enc(geo, compute, proj=True):
    enc = MpnetEncoder(synthetic_seed=lr.WSEEDS[geo], compute=compute, cfg_overrides=_cfg(geo).encoder_overrides())
    if proj:
        enc.set_token_projection(_weights(geo, True)["linear.weight"].numpy())
    return enc


class Bars:
    """The bars of one (geometry, mode, case): ``cos`` on 1 - cos of a token vector, ``score(m)`` on a score."""

    def __init__(self, geo, compute, proj, vmin):
        self.P = lr.WIDTH[geo] if proj else lr.GEOS[geo]["hidden"]
        self.bf16 = compute == "bf16"
        self.eps = lr.fp32_token_eps(_weights(geo, proj), _cfg(geo), vmin)

    @property
    def cos(self):
        return lr.BF16_COS_BAR if self.bf16 else lr.fp32_cos_bar(self.eps)

    def score(self, m):
        return lr.BF16_SCORE_BAR if self.bf16 else lr.fp32_score_bar(self.eps, self.eps, m, self.P)


def _check_tokens(mats, ref, bars, what):
    gap = max(lr.cosine_gap(bf16_to_f32(m), r) for m, r in zip(mats, ref))
    print(f"[li] {what}: max 1 - cos = {gap:.3e} (bar {bars.cos:.3e})")
    assert [m.shape for m in mats] == [r.shape for r in ref]
    assert gap <= bars.cos, (what, gap, bars.cos)
    return gap


def _check_scores(out, ref, ms, bars, what):
    err = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    bar = np.array([bars.score(m) for m in ms])
    print(f"[li] {what}: max |score - ref| = {err.max():.3e} (bar {bar.min():.3e} .. {bar.max():.3e})")
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert (err <= bar).all(), (what, err.max(), bar)
    return float(err.max())


def _check_order(out, ref, bar, what):
    """The device's order equals the reference's wherever the reference scores differ by more than twice the bar; that
    must bind at least half of the adjacent pairs (a property of the reference alone)."""
    order, mask = lr.binding_pairs(ref, bar)
    print(f"[li] {what}: the order check binds {int(mask.sum())} of {mask.size} adjacent pairs")
    assert 2 * int(mask.sum()) >= mask.size, (what, mask)
    for i in range(len(ref)):
        for j in range(len(ref)):
            if float(ref[i]) - float(ref[j]) > 2 * bar:
                assert out[i] > out[j], (what, i, j, ref[i], ref[j], out[i], out[j])


def _run_case(enc, geo, compute, proj, lens, q_dev, what):
    qb, qref, qvmin = _queries(geo, proj)
    batch, dref, dvmin = _side(geo, proj, tuple(lens), lr.BSEED)
    bars = Bars(geo, compute, proj, min(qvmin, dvmin))
    mats = enc.encode_tokens_ids(batch)
    gap = _check_tokens(mats, dref, bars, f"{what} tokens")
    pairs = [(i, j) for i in range(len(qb)) for j in range(len(batch))]
    ref = lr.scores(qref, dref, pairs)
    out = enc.maxsim(q_dev, mats)
    err = _check_scores(out, ref, [len(qb[i]) for i, _ in pairs], bars, f"{what} scores")
    fused = enc.score_late_ids(batch, q_dev)
    assert np.array_equal(out.view(np.uint32), fused.view(np.uint32))      # one call returns the bits of the two
    return gap, err, bars, out, ref, pairs


# ---- 4. token vectors and scores against the reference ----------------------------------------------------------------------
@pytest.mark.parametrize("proj", [True, False], ids=["proj", "hidden"])
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_tokens_and_scores_match_the_reference(geo, compute, proj):
    enc = _enc(geo, compute, proj)
    qb, qref, qvmin = _queries(geo, proj)
    q_dev = enc.encode_tokens_ids(qb)
    _check_tokens(q_dev, qref, Bars(geo, compute, proj, qvmin), f"test4 {geo} {compute} proj={proj} queries")
    gaps, errs = [], []
    for lens in lr.CASES:
        gap, err, *_ = _run_case(enc, geo, compute, proj, lens, q_dev, f"test4 {geo} {compute} proj={proj} {lens}")
        gaps.append(gap)
        errs.append(err)
    print(f"[li] test4 {geo} {compute} proj={proj}: largest 1 - cos {max(gaps):.3e}, largest |score - ref| {max(errs):.3e}")
    enc.close()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_ranking_matches_the_reference(geo, compute):
    enc = _enc(geo, compute)
    qb, _, _ = _queries(geo, True)
    q_dev = enc.encode_tokens_ids(qb)
    _, _, bars, out, ref, pairs = _run_case(enc, geo, compute, True, lr.RANK_CASE, q_dev, f"rank {geo} {compute}")
    sel = [n for n, (i, _) in enumerate(pairs) if i == 2]                   # the 32-token query
    _check_order(out[sel], ref[sel], bars.score(32), f"rank {geo} {compute}")
    enc.close()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("name,geo", [("li_small_2layer", "small"), ("li_base_2layer", "base")])
def test_goldens(name, geo, compute):
    """Scores and one token matrix of transformers' BertModel + torch.nn.Linear (tests/golden/make_li_goldens.py)."""
    g = np.load(HERE / "golden" / f"{name}.npz")
    assert int(g["wseed"]) == lr.WSEEDS[geo] and int(g["width"]) == lr.WIDTH[geo]
    cfg = _cfg(geo)
    qb = br.synth_batch(cfg, g["query_lengths"].tolist(), int(g["qseed"]))
    batch = br.synth_batch(cfg, g["lengths"].tolist(), int(g["bseed"]))
    enc = _enc(geo, compute)
    bars = Bars(geo, compute, True, float(g["vmin"]))
    q_dev, mats = enc.encode_tokens_ids(qb), enc.encode_tokens_ids(batch)
    _check_tokens(mats[:1], [g["tokens0"]], bars, f"golden {geo} {compute} tokens of doc 0")
    pairs = [(i, j) for i in range(len(qb)) for j in range(len(batch))]
    _check_scores(enc.maxsim(q_dev, mats), g["scores"].reshape(-1), [len(qb[i]) for i, _ in pairs], bars,
                  f"golden {geo} {compute} scores")
    enc.close()


# ---- 5. a batch of >= 1024 tokens --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["small", "base"])
def test_bf16_batch_of_over_1024_tokens(geo):
    """The LayerNorm-folded path at hidden 768 (blocked bf16 rows + statistics), the wide GEMM tiles at hidden 384:
    within the bars, the same bits on a second call, within the bars again with the running-maximum attention pass,
    and forward_maxsim returns the bits of forward_tokens followed by maxsim."""
    assert sum(lr.BIG_CASE) >= 1024
    enc = _enc(geo, "bf16")
    qb, _, _ = _queries(geo, True)
    q_dev = enc.encode_tokens_ids(qb)
    gap, err, bars, out, ref, pairs = _run_case(enc, geo, "bf16", True, lr.BIG_CASE, q_dev, f"test5 {geo} bf16")
    batch = _side(geo, True, tuple(lr.BIG_CASE), lr.BSEED)[0]
    if geo == "base":
        with pytest.raises(RuntimeError, match="folded"):                  # the folded path ran: x32 does not exist
            enc.debug_read("x32", (sum(lr.BIG_CASE), 768))
    mats = enc.encode_tokens_ids(batch)
    again, toks = enc.score_late_ids(batch, q_dev, return_tokens=True)
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32))
    assert all(np.array_equal(a, b) for a, b in zip(mats, toks))
    assert all(np.array_equal(a, b) for a, b in zip(mats, enc.encode_tokens_ids(batch)))
    keep = [np.ones(n, np.uint8) for n in lr.BIG_CASE]
    for k in keep:
        k[1::3] = 0
    kept = enc.score_late_ids(batch, q_dev, keep=keep)
    assert np.array_equal(kept.view(np.uint32), enc.maxsim(q_dev, mats, keep=keep).view(np.uint32))
    assert (kept <= out).all() and (kept < out).any()
    enc.set_attention_range(0.0)
    _run_case(enc, geo, "bf16", True, lr.BIG_CASE, q_dev, f"test5 {geo} bf16 range=0")
    print(f"[li] test5 {geo}: largest 1 - cos {gap:.3e}, largest |score - ref| {err:.3e}")
    enc.close()


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------
def _toy_vocab(rng):
    import string

    words = sorted({"".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(2, 8))) for _ in range(1500)})
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    vocab += list(string.punctuation) + list(string.digits) + list(string.ascii_lowercase)
    vocab += ["##" + c for c in string.ascii_lowercase] + words
    return list(dict.fromkeys(vocab)), words


def _write_colbert_checkpoint(d: Path, cfg, w, vocab_words):
    from safetensors.numpy import save_file

    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({
        "architectures": ["HF_ColBERT"], "model_type": "bert", "hidden_act": "gelu", "hidden_size": cfg.hidden,
        "num_attention_heads": cfg.heads, "num_hidden_layers": cfg.num_layers, "intermediate_size": cfg.ffn,
        "vocab_size": cfg.vocab, "max_position_embeddings": cfg.max_pos, "type_vocab_size": 2,
        "layer_norm_eps": cfg.ln_eps, "pad_token_id": 0}))
    sd = {("" if k == "linear.weight" else "bert.") + k: v.numpy() for k, v in w.items()}
    save_file(sd, str(d / "model.safetensors"))
    (d / "vocab.txt").write_text("\n".join(vocab_words) + "\n", encoding="utf-8")
    (d / "tokenizer_config.json").write_text(json.dumps({"do_lower_case": True}))


def test_checkpoint_end_to_end_rank_and_search_reranked(tmp_path):
    import random
    import string

    from claude_semantic_search_amd import Chunk, HybridStorage, LateInteraction, Reranked, SearchConfig, StorageConfig
    from claude_semantic_search_amd import synth

    rng = random.Random(5)
    vocab, words = _toy_vocab(rng)
    cfg = br.BertCfg(num_layers=6, vocab=len(vocab), pooling="cls", **br.SMALL)
    w = lr.synth_weights(cfg, 21, 96)
    _write_colbert_checkpoint(tmp_path / "colbert-small", cfg, w, vocab)
    skip = [vocab.index(c) for c in string.punctuation]
    li = LateInteraction(str(tmp_path / "colbert-small"), document_length=128, skip_ids=skip)
    assert li.cfg["num_layers"] == 6 and li.token_dim == 96 and (li.query_marker_id, li.document_marker_id) == (1, 2)

    def text(lo, hi):
        return " ".join(rng.choice(words) for _ in range(rng.randint(lo, hi))) + rng.choice(["", ".", " x=1!"])

    query = text(20, 28)
    lens = [2, 3, 4, 5, 6, 8, 10, 12, 15, 18, 22, 27, 33, 40, 150]         # (the last one is truncated)
    docs = [text(n, n) for n in lens]
    pairs = [(query, d) for d in docs] + [(text(80, 90), docs[3])]          # (a query that is cut to 32 tokens)
    out = li.predict(pairs, batch_size=8)
    # the reference on the same ids
    qids, dids = li.query_ids([p[0] for p in pairs]), li.document_ids([p[1] for p in pairs])
    assert max(map(len, dids)) == 128 and len(qids[-1]) == 32 and qids[0][1] == 1 and dids[0][1] == 2
    keep = li._keep(dids)
    assert any((k == 0).any() for k in keep) and all(k[0] == 1 and k[-1] == 1 for k in keep)
    qref = [lr.token_vectors(w, cfg, ids) for ids in qids]
    dref = [lr.token_vectors(w, cfg, ids) for ids in dids]
    ref = lr.scores(qref, dref, [(n, n) for n in range(len(pairs))], keep)
    q_dev, _ = li.encode_queries([query])
    gap = lr.cosine_gap(bf16_to_f32(q_dev[0]), qref[0])
    d_dev, d_keep = li.encode_documents(docs)
    gap = max([gap] + [lr.cosine_gap(bf16_to_f32(m), r) for m, r in zip(d_dev, dref)])
    err = float(np.abs(out - ref).max())
    print(f"[li] test8 small bf16 6 layers: max 1 - cos = {gap:.3e} (bar {lr.BF16_COS_BAR_6LAYER:.3e}), "
          f"max |score - ref| = {err:.3e} (bar {lr.BF16_SCORE_BAR_6LAYER:.3e})")
    assert gap <= lr.BF16_COS_BAR_6LAYER and err <= lr.BF16_SCORE_BAR_6LAYER
    assert np.array_equal(out, li.predict(pairs, batch_size=8))            # the same batches: the same bits
    cached = li.score(q_dev, d_dev, keep=d_keep)                           # kept matrices: no forward pass
    assert np.abs(cached - ref[:len(docs)]).max() <= lr.BF16_SCORE_BAR_6LAYER
    assert li.predict([]).shape == (0,)

    ranked = li.rank(query, docs, return_documents=True)
    got = [h["corpus_id"] for h in ranked]
    assert sorted(got) == list(range(len(docs))) and all(h["text"] == docs[h["corpus_id"]] for h in ranked)
    scores = np.empty(len(docs), np.float32)
    for h in ranked:
        scores[h["corpus_id"]] = h["score"]
    _check_order(scores, ref[:len(docs)], lr.BF16_SCORE_BAR_6LAYER, "test8 rank")
    assert [h["corpus_id"] for h in li.rank(query, docs, top_k=3)] == got[:3]

    texts = [text(3, 60) for _ in range(120)]
    emb = synth.rows(120, 64, 9)
    chunks = [Chunk(f"c{i:04d}", t, {"project_name": "p"}, emb[i]) for i, t in enumerate(texts)]
    with HybridStorage(StorageConfig(data_dir=str(tmp_path / "store"), embedding_dim=64, auto_save=False)) as st:
        st.add_chunks(chunks)
        q = emb[17] + 0.5 * emb[40]
        plain = st.search(q, SearchConfig(top_k=30), None)
        res = st.search_reranked(query, q, li, SearchConfig(top_k=10), None, fetch=30)
        assert len(res) == 10 and all(isinstance(r, Reranked) for r in res)
        allp = li.predict([(query, p.text) for p in plain])
        assert [r.score for r in res] == [float(allp[r.rank_before]) for r in res]
        assert [r.rank_before for r in res] == np.argsort(-allp, kind="stable")[:10].tolist()
    li.close()
