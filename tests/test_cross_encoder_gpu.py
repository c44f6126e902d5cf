"""GPU: cross-encoder re-ranking (css_encoder_set_head / css_encoder_forward_pairs, CrossEncoder, search_reranked)
against the fp32 PyTorch reference (tests/ce_reference.py) and the committed transformers goldens.

Bars (tests/ce_reference.py): fp32 mode ``fp32_bar`` (the 1e-4 hidden-state bar pushed through the head); bf16 mode
``BF16_BAR`` = 2 x the largest |logit - fp32 reference| measured on the device over the cases of tests 1, 2, 5 and 7
(DESIGN.md 3.3c has the per-test maxima).  Every test prints its figure before it asserts."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402
import ce_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu

BSEED = cr.BSEED


def _cfg(geo, layers=2, vocab=30522, pooling="mean"):
    return br.BertCfg(num_layers=layers, vocab=vocab, pooling=pooling, normalize=False, **cr.GEOS[geo])


@functools.lru_cache(maxsize=4)
def _weights(geo, layers=2, vocab=30522):
    return cr.synth_weights(_cfg(geo, layers, vocab), cr.WSEEDS[geo])


@functools.lru_cache(maxsize=None)
def _case(geo, lens, segs):
    """(batch, reference logits) of one case; computed once and shared."""
    cfg = _cfg(geo)
    batch = cr.synth_pair_batch(cfg, lens, segs, BSEED)
    return batch, cr.logits(_weights(geo), cfg, batch, segs)


def _enc(geo, compute, layers=2, vocab=30522, pooling="mean", head=True):
    cfg = _cfg(geo, layers, vocab, pooling)
    enc = MpnetEncoder(synthetic_seed=cr.WSEEDS[geo], compute=compute, cfg_overrides=cfg.encoder_overrides())
    if head:
        enc.set_head(*cr.head_arrays(_weights(geo, layers, vocab)))
    return enc


def _bar(geo, compute, layers=2, vocab=30522):
    return cr.fp32_bar(_weights(geo, layers, vocab)) if compute == "fp32" else cr.BF16_BAR


def _check(out, ref, bar, what):
    err = float(np.abs(out - ref).max())
    print(f"[ce] {what}: max |logit - ref| = {err:.3e} (bar {bar:.3e})")
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert err <= bar, (what, err, bar)


# ---- 1. logits against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_logits_match_the_reference(geo, compute):
    enc = _enc(geo, compute)
    for lens, segs in cr.CASES:
        batch, ref = _case(geo, tuple(lens), tuple(segs))
        _check(enc.score_pair_ids(batch, segs), ref, _bar(geo, compute), f"test1 {geo} {compute} {lens}")
    enc.close()


# ---- 2. a batch of >= 1024 tokens -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["small", "base"])
def test_bf16_batch_of_over_1024_tokens(geo):
    """The LayerNorm-folded path at hidden 768, the wide GEMM tiles at hidden 384: within the bar, the same bits on a
    second call, and within the bar again with the running-maximum attention pass."""
    lens, segs = cr.BIG_CASE
    assert sum(lens) >= 1024
    batch, ref = _case(geo, tuple(lens), tuple(segs))
    enc = _enc(geo, "bf16")
    out = enc.score_pair_ids(batch, segs)
    _check(out, ref, cr.BF16_BAR, f"test2 {geo} bf16")
    assert np.array_equal(out, enc.score_pair_ids(batch, segs))
    enc.set_attention_range(0.0)
    _check(enc.score_pair_ids(batch, segs), ref, cr.BF16_BAR, f"test2 {geo} bf16 range=0")
    enc.close()


# ---- 3. the tie to the verified path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_single_segment_pairs_leave_the_bits_of_the_plain_forward(geo, compute):
    lens = [128, 6, 64, 33, 255]
    cfg = _cfg(geo)
    T, H = sum(lens), cfg.hidden
    assert T < 1024
    batch = br.synth_batch(cfg, lens, BSEED)
    enc = _enc(geo, compute)
    enc.encode_ids(batch, normalize=False)
    x_plain = enc.debug_read("x32", (T, H))
    first = enc.score_pair_ids(batch, lens)            # seg_start == len: every token has type 0
    x_pairs = enc.debug_read("x32", (T, H))
    assert np.array_equal(x_plain.view(np.uint32), x_pairs.view(np.uint32))
    # ... and a real segment start moves them (the comparison above is not vacuous)
    enc.score_pair_ids(batch, [2] * len(lens))
    assert not np.array_equal(x_plain, enc.debug_read("x32", (T, H)))
    enc.encode_ids(batch)
    assert np.array_equal(first.view(np.uint32), enc.score_pair_ids(batch, lens).view(np.uint32))
    enc.close()


@pytest.mark.parametrize("geo", ["small", "base"])
def test_graph_replay_of_encode_ids_survives_a_pair_call(geo):
    """One sequence of 12 tokens: eager, captured, replayed; a pair call in between changes none of its bits."""
    cfg = _cfg(geo)
    batch = br.synth_batch(cfg, [12], BSEED)
    enc = _enc(geo, "bf16")
    a = enc.encode_ids(batch)
    b = enc.encode_ids(batch)
    p = enc.score_pair_ids(batch, [5])
    c = enc.encode_ids(batch)
    assert np.array_equal(a, b) and np.array_equal(b, c)
    assert np.array_equal(p, enc.score_pair_ids(batch, [5]))
    assert np.array_equal(c, enc.encode_ids(batch))
    enc.close()


# ---- 4. the head alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["small", "base"])
def test_head_alone_against_float64(geo):
    """Single-segment sequences through a 1-layer CLS encoder: the logits are the float64 numpy head of the rows that
    encode_ids returns, to 1e-5 * (|bc| + sum |wc|) -- the inputs are the same fp32 rows, so only the rounding of two
    fp32 reductions of <= 768 terms and tanhf remains."""
    vocab = 1000
    w = _weights(geo, 1, vocab)
    wp, bp, wc, bc = (a.astype(np.float64) for a in cr.head_arrays(w))
    tol = 1e-5 * (abs(bc[0]) + np.abs(wc).sum())
    enc = _enc(geo, "fp32", layers=1, vocab=vocab, pooling="cls")
    cfg = _cfg(geo, 1, vocab, "cls")
    for B in (1, 7, 8, 9, 17):
        lens = [3 + (5 * i) % 11 for i in range(B)]
        batch = br.synth_batch(cfg, lens, BSEED + B)
        rows = enc.encode_ids(batch, normalize=False).astype(np.float64)
        want = np.tanh(rows @ wp.T + bp) @ wc + bc[0]
        got = enc.score_pair_ids(batch, lens)
        err = float(np.abs(got - want).max())
        print(f"[ce] test4 {geo} B={B}: max |logit - float64 head| = {err:.3e} (tol {tol:.3e})")
        assert got.shape == (B,) and err <= tol, (B, err, tol)
    enc.close()


# ---- 5. the committed goldens ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("name,geo", [("ce_small_2layer", "small"), ("ce_base_2layer", "base")])
def test_committed_goldens_on_the_device(name, geo, compute):
    g = np.load(HERE / "golden" / f"{name}.npz")
    cfg = _cfg(geo, int(g["num_layers"]))
    lens, segs = g["lengths"].tolist(), g["seg_starts"].tolist()
    batch = cr.synth_pair_batch(cfg, lens, segs, int(g["bseed"]))
    w = cr.synth_weights(cfg, int(g["wseed"]))
    enc = MpnetEncoder(synthetic_seed=int(g["wseed"]), compute=compute, cfg_overrides=cfg.encoder_overrides())
    enc.set_head(*cr.head_arrays(w))
    bar = cr.fp32_bar(w) if compute == "fp32" else cr.BF16_BAR
    _check(enc.score_pair_ids(batch, segs), g["logits"].astype(np.float32), bar, f"test5 {geo} {compute}")
    enc.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_errors():
    from claude_semantic_search_amd import _native as nat

    menc = MpnetEncoder(synthetic_seed=1, compute="fp32", cfg_overrides={"num_layers": 1, "vocab": 1000})
    H = 768
    z = np.zeros
    with pytest.raises(RuntimeError, match="not a BERT model") as ei:
        menc.set_head(z((H, H), np.float32), z(H, np.float32), z(H, np.float32), z(1, np.float32))
    assert ei.value.code == nat.CSS_ERR_INVALID
    with pytest.raises(RuntimeError, match="not a BERT model") as ei:
        menc.score_pair_ids([[0, 5, 2]], [2])
    assert ei.value.code == nat.CSS_ERR_INVALID
    menc.close()

    cfg = _cfg("small", 1, 1000)
    batch = br.synth_batch(cfg, [6, 9], BSEED)
    enc = _enc("small", "fp32", layers=1, vocab=1000, head=False)
    with pytest.raises(RuntimeError, match="no classification head") as ei:
        enc.score_pair_ids(batch, [3, 3])
    assert ei.value.code == nat.CSS_ERR_STATE
    for bad in ((H, 384), (384,), (383, 384)):
        with pytest.raises(ValueError, match="pooler_w has shape"):
            enc.set_head(z(bad, np.float32), z(384, np.float32), z(384, np.float32), z(1, np.float32))
    with pytest.raises(ValueError, match="cls_w has shape"):
        enc.set_head(z((384, 384), np.float32), z(384, np.float32), z((2, 384), np.float32), z(1, np.float32))
    enc.set_head(*cr.head_arrays(_weights("small", 1, 1000)))
    good = enc.score_pair_ids(batch, [3, 9])
    with pytest.raises(RuntimeError, match=r"sequence 1 has seg_start 0 outside \[1, 9\]"):
        enc.score_pair_ids(batch, [3, 0])
    with pytest.raises(RuntimeError, match=r"sequence 0 has seg_start 7 outside \[1, 6\]"):
        enc.score_pair_ids(batch, [7, 3])
    with pytest.raises(ValueError, match="seg_starts for 2 sequences"):
        enc.score_pair_ids(batch, [3])
    assert np.array_equal(good, enc.score_pair_ids(batch, [3, 9]))   # the encoder stays usable
    enc.close()


def test_synthetic_mode_has_the_reference_head():
    """CrossEncoder(synthetic_seed=...): the body from css_encoder_init_synthetic, the head from synth on the host --
    the model of tests/ce_reference.py."""
    from claude_semantic_search_amd import CrossEncoder

    seed = cr.WSEEDS["small"]
    ce = CrossEncoder(None, compute="fp32", synthetic_seed=seed, cfg_overrides={"num_layers": 2}, max_length=32)
    pairs = [("what is a kernel", "a kernel is a function that runs on the device"), ("short", "x " * 60), ("", "b")]
    ids, segs = ce.tokenize_pairs(pairs)
    assert max(map(len, ids)) == 32 and ids[2] == [ce.cls_id, ce.sep_id, ids[2][2], ce.sep_id] and segs[2] == 2
    ref = cr.logits(_weights("small"), _cfg("small"), ids, segs)
    _check(ce.predict(pairs), ref, _bar("small", "fp32"), "synthetic mode small fp32")
    ce.close()


# ---- 7. end to end --------------------------------------------------------------------------------------------------------
def _toy_vocab(rng):
    import string

    words = sorted({"".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(2, 8))) for _ in range(1500)})
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    vocab += list(string.punctuation) + list(string.digits) + list(string.ascii_lowercase)
    vocab += ["##" + c for c in string.ascii_lowercase] + words
    return list(dict.fromkeys(vocab)), words


def _write_ce_checkpoint(d: Path, cfg, w, vocab_words):
    from safetensors.numpy import save_file

    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({
        "architectures": ["BertForSequenceClassification"], "model_type": "bert", "hidden_act": "gelu",
        "hidden_size": cfg.hidden, "num_attention_heads": cfg.heads, "num_hidden_layers": cfg.num_layers,
        "intermediate_size": cfg.ffn, "vocab_size": cfg.vocab, "max_position_embeddings": cfg.max_pos,
        "type_vocab_size": 2, "layer_norm_eps": cfg.ln_eps, "pad_token_id": 0, "id2label": {"0": "LABEL_0"},
        "label2id": {"LABEL_0": 0}}))
    sd = {("" if k.startswith("classifier.") else "bert.") + k: v.numpy() for k, v in w.items()}
    save_file(sd, str(d / "model.safetensors"))
    (d / "vocab.txt").write_text("\n".join(vocab_words) + "\n", encoding="utf-8")
    (d / "tokenizer_config.json").write_text(json.dumps({"do_lower_case": True}))


def test_checkpoint_end_to_end_predict_rank_and_search_reranked(tmp_path):
    import random

    from claude_semantic_search_amd import Chunk, CrossEncoder, HybridStorage, Reranked, SearchConfig, StorageConfig
    from claude_semantic_search_amd import synth

    rng = random.Random(5)
    vocab, words = _toy_vocab(rng)
    cfg = br.BertCfg(num_layers=6, vocab=len(vocab), pooling="cls", normalize=False, **br.SMALL)
    w = cr.synth_weights(cfg, 21)
    _write_ce_checkpoint(tmp_path / "ce-minilm", cfg, w, vocab)
    ce = CrossEncoder(str(tmp_path / "ce-minilm"), max_length=128)
    assert ce.cfg["num_layers"] == 6 and ce.cfg["hidden"] == 384 and ce.max_length == 128

    def text(lo, hi):
        return " ".join(rng.choice(words) for _ in range(rng.randint(lo, hi))) + rng.choice(["", ".", " x=1!"])

    query = text(4, 9)
    docs = [text(3, 90) for _ in range(19)] + [text(150, 160)]            # (the last one is truncated)
    pairs = [(query, d) for d in docs] + [(text(140, 150), text(3, 5)), ("", text(3, 5)), (text(3, 5), "")]
    out = ce.predict(pairs, batch_size=8)
    # the reference on build_pair of the same tokens
    ids = [cr.build_pair(ce._side_ids([a])[0], ce._side_ids([b])[0], ce.cls_id, ce.sep_id, 128) for a, b in pairs]
    assert max(len(i) for i, _ in ids) == 128 and (ce.cls_id, ce.sep_id) == (vocab.index("[CLS]"), vocab.index("[SEP]"))
    ref = cr.logits(w, cfg, [i for i, _ in ids], [s for _, s in ids])
    print(f"[ce] test7 reference logits: n {ref.size} mean {ref.mean():.4e} std {ref.std():.3e}")
    _check(out, ref, cr.BF16_BAR, "test7 small bf16 6 layers")
    assert np.array_equal(out, ce.predict(pairs, batch_size=8))            # the same batches: the same bits
    _check(ce.predict(pairs, batch_size=32), ref, cr.BF16_BAR, "test7 small bf16 6 layers, one batch")
    sig = ce.predict(pairs[:5], activation="sigmoid")
    assert np.allclose(sig, 1 / (1 + np.exp(-out[:5].astype(np.float64))), atol=2 * cr.BF16_BAR)
    assert ce.predict([]).shape == (0,) and ce.predict([]).dtype == np.float32

    ranked = ce.rank(query, docs, return_documents=True)
    got = [h["corpus_id"] for h in ranked]
    assert sorted(got) == list(range(len(docs))) and all(h["text"] == docs[h["corpus_id"]] for h in ranked)
    assert all(ranked[i]["score"] >= ranked[i + 1]["score"] for i in range(len(ranked) - 1))
    pos = {c: i for i, c in enumerate(got)}
    rd = ref[: len(docs)]
    for i in range(len(docs)):          # the reference's order wherever its logits differ by more than twice the bar
        for j in range(len(docs)):
            if rd[i] - rd[j] > 2 * cr.BF16_BAR:
                assert pos[i] < pos[j], (i, j, rd[i], rd[j])
    assert [h["corpus_id"] for h in ce.rank(query, docs, top_k=3)] == got[:3]

    # search_reranked over 200 chunks; the index is 64-dimensional (the reranker's hidden size need not match it)
    texts = [text(3, 60) for _ in range(200)]
    emb = synth.rows(200, 64, 9)
    chunks = [Chunk(f"c{i:04d}", t, {"project_name": "p" if i % 2 else "q"}, emb[i]) for i, t in enumerate(texts)]
    with HybridStorage(StorageConfig(data_dir=str(tmp_path / "store"), embedding_dim=64, auto_save=False)) as st:
        st.add_chunks(chunks)
        q = emb[17] + 0.5 * emb[40]
        plain_before = st.search(q, SearchConfig(top_k=50), None)
        dead = [plain_before[0].chunk_id, plain_before[3].chunk_id]
        for cid in dead:
            assert st.delete_chunk(cid)
        plain = st.search(q, SearchConfig(top_k=50), None)
        res = st.search_reranked(query, q, ce, SearchConfig(top_k=10), None, fetch=50)
        assert len(res) == 10 and all(isinstance(r, Reranked) for r in res)
        assert not set(dead) & {r.result.chunk_id for r in res}
        for r in res:
            assert plain[r.rank_before].chunk_id == r.result.chunk_id
            assert r.result.similarity == plain[r.rank_before].similarity
        # score = predict on the texts: the same bits for the same fifty pairs, within the bar for the ten alone
        # (another batch composition takes another GEMM tile walk)
        allp = ce.predict([(query, p.text) for p in plain])
        assert [r.score for r in res] == [float(allp[r.rank_before]) for r in res]
        want = ce.predict([(query, r.result.text) for r in res])
        assert np.abs(np.array([r.score for r in res], np.float32) - want).max() <= cr.BF16_BAR
        assert [r.rank_before for r in res] == np.argsort(-allp, kind="stable")[:10].tolist()   # the ten best of fifty
        only_p = st.search_reranked(query, q, ce, SearchConfig(top_k=5), {"project_name": "p"}, fetch=20)
        assert len(only_p) == 5 and all(r.result.metadata["project_name"] == "p" for r in only_p)
    ce.close()
