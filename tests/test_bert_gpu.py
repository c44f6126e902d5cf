"""GPU: BERT sentence encoders (all-MiniLM-L6-v2 / bge-small geometry: hidden 384, 12 x 32 heads; bge-base geometry:
hidden 768, 12 x 64) through the C ABI against the fp32 PyTorch reference (tests/bert_reference.py) and the committed
transformers goldens.  Bars as the MPNet suite's: fp32 mode <= 1e-4 max abs; bf16 mode min cosine > 1 - 1e-3 and max
abs < 2e-2."""
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

pytestmark = pytest.mark.gpu

GEOS = {"small": br.SMALL, "base": br.BASE}
WSEED, BSEED = 7, 11


@functools.lru_cache(maxsize=4)
def _weights(geo: str, layers: int, vocab: int = 30522):
    return br.synth_weights(br.BertCfg(num_layers=layers, vocab=vocab, **GEOS[geo]), WSEED)


def _case(geo, layers, pooling, lengths, vocab=30522):
    cfg = br.BertCfg(num_layers=layers, vocab=vocab, pooling=pooling, **GEOS[geo])
    batch = br.synth_batch(cfg, lengths, BSEED)
    return cfg, batch, br.encode(_weights(geo, layers, vocab), cfg, batch)


def _enc(cfg, compute):
    return MpnetEncoder(synthetic_seed=WSEED, compute=compute, cfg_overrides=cfg.encoder_overrides())


def _check(out, ref, compute):
    err = np.abs(out - ref).max()
    if compute == "fp32":
        assert err < 1e-4, err
    else:
        cos = (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))
        assert err < 2e-2 and cos.min() > 1 - 1e-3, (err, cos.min())


LENGTH_SETS = [[1], [2, 7, 31], [128, 5, 64, 33], [383, 384, 2, 255]]


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("pooling", ["mean", "cls"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_two_layers_match_the_reference(geo, pooling, compute):
    for i, lengths in enumerate(LENGTH_SETS):
        cfg, batch, ref = _case(geo, 2, pooling, lengths)
        if i == 0:
            enc = _enc(cfg, compute)
            assert enc.get_sentence_embedding_dimension() == cfg.hidden
        _check(enc.encode_ids(batch), ref, compute)
    enc.close()


@pytest.mark.parametrize("pooling", ["mean", "cls"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_bf16_batch_of_over_1024_tokens_is_reproducible(geo, pooling):
    """>= 1024 tokens: the LayerNorm-folded path at hidden 768, the wide GEMM tiles at hidden 384; both attention
    passes (the guarded reference-free pass and the forced running-maximum pass) agree with the reference; the same
    batch gives the same bits twice."""
    lengths = [384, 383, 255, 128, 31, 7, 2, 1, 200, 100]
    cfg, batch, ref = _case(geo, 2, pooling, lengths)
    assert sum(lengths) >= 1024
    enc = _enc(cfg, "bf16")
    out = enc.encode_ids(batch)
    _check(out, ref, "bf16")
    assert np.array_equal(out, enc.encode_ids(batch))
    enc.set_attention_range(0.0)
    _check(enc.encode_ids(batch), ref, "bf16")
    enc.close()


def test_minilm_l6_geometry_six_layers():
    for compute in ("bf16", "fp32"):
        cfg, batch, ref = _case("small", 6, "mean", [384, 77, 12, 1, 250, 300, 40])
        enc = _enc(cfg, compute)
        _check(enc.encode_ids(batch), ref, compute)
        enc.close()


@pytest.mark.parametrize("geo,pooling", [("small", "mean"), ("small", "cls"), ("base", "cls")])
def test_single_query_graph_replay(geo, pooling):
    """One short query, three times: eager, captured, replayed -- same bits, within the bf16 bar."""
    cfg, batch, ref = _case(geo, 2, pooling, [12])
    enc = _enc(cfg, "bf16")
    outs = [enc.encode_ids(batch) for _ in range(3)]
    _check(outs[0], ref, "bf16")
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    cfg2, batch2, ref2 = _case(geo, 2, pooling, [5, 40])   # a small multi-sequence batch (<= 64 tokens)
    for _ in range(3):
        _check(enc.encode_ids(batch2), ref2, "bf16")
    enc.close()


@pytest.mark.parametrize("name,geo", [("bert_small_2layer", "small"), ("bert_base_2layer", "base")])
def test_committed_goldens_on_the_device(name, geo):
    g = np.load(HERE / "golden" / f"{name}.npz")
    for pooling in ("mean", "cls"):
        cfg = br.BertCfg(num_layers=int(g["num_layers"]), pooling=pooling, **GEOS[geo])
        batch = br.synth_batch(cfg, g["lengths"].tolist(), int(g["bseed"]))
        for compute in ("fp32", "bf16"):
            enc = MpnetEncoder(synthetic_seed=int(g["wseed"]), compute=compute, cfg_overrides=cfg.encoder_overrides())
            _check(enc.encode_ids(batch), g["emb_" + pooling], compute)
            enc.close()


def _state_dict(cfg):
    return {k: v.numpy() for k, v in br.synth_weights(cfg, WSEED).items()}


def test_strict_loading_of_bert_tensors():
    cfg = br.BertCfg(num_layers=1, vocab=1000)
    sd = _state_dict(cfg)
    enc = _enc(cfg, "fp32")
    enc.load_state_dict(sd)   # complete: accepted
    bad = dict(sd)
    del bad["encoder.layer.0.attention.self.key.bias"]
    with pytest.raises(RuntimeError, match="no tensor for 'encoder.layer.0.attention.self.key.bias'"):
        enc.load_state_dict(bad)
    dup = dict(sd, **{"bert.embeddings.LayerNorm.weight": sd["embeddings.LayerNorm.weight"]})
    with pytest.raises(RuntimeError, match="more than once"):
        enc.load_state_dict(dup)
    wrong = dict(sd, **{"encoder.layer.0.attention.self.query.weight": np.zeros((384, 383), np.float32)})
    with pytest.raises(RuntimeError, match="elements"):
        enc.load_state_dict(wrong)
    # MPNet names are unknown to a BERT encoder
    from oracle import mpnet_oracle as mo

    mp = {k: v.numpy() for k, v in mo.synth_weights(mo.MpnetCfg(num_layers=1, vocab=1000), 1).items()}
    for name in ("encoder.layer.0.attention.attn.q.weight", "encoder.relative_attention_bias.weight"):
        with pytest.raises(RuntimeError, match="unknown parameter"):
            enc.load_state_dict(dict(sd, **{name: mp[name]}))
    enc.close()
    # ... and BERT names to an MPNet encoder
    menc = MpnetEncoder(synthetic_seed=1, compute="fp32", cfg_overrides={"num_layers": 1, "vocab": 1000})
    bsd = _state_dict(br.BertCfg(num_layers=1, vocab=1000, **br.BASE))
    for name in ("encoder.layer.0.attention.self.query.weight", "embeddings.token_type_embeddings.weight",
                 "encoder.layer.0.attention.output.dense.bias"):
        with pytest.raises(RuntimeError, match="unknown parameter"):
            menc.load_state_dict(dict(mp, **{name: bsd[name]}))
    menc.close()


def _write_st_checkpoint(d: Path, cfg, w, vocab_words):
    """sentence-transformers layout: config.json, model.safetensors, vocab.txt, tokenizer_config.json, modules.json,
    1_Pooling/config.json, 2_Normalize/."""
    from safetensors.numpy import save_file

    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({
        "model_type": "bert", "hidden_act": "gelu", "hidden_size": cfg.hidden, "num_attention_heads": cfg.heads,
        "num_hidden_layers": cfg.num_layers, "intermediate_size": cfg.ffn, "vocab_size": cfg.vocab,
        "max_position_embeddings": cfg.max_pos, "type_vocab_size": 2, "layer_norm_eps": cfg.ln_eps, "pad_token_id": 0}))
    sd = {k: v.numpy() for k, v in w.items()}
    sd["pooler.dense.weight"] = np.zeros((cfg.hidden, cfg.hidden), np.float32)
    sd["pooler.dense.bias"] = np.zeros((cfg.hidden,), np.float32)
    save_file(sd, str(d / "model.safetensors"))
    (d / "vocab.txt").write_text("\n".join(vocab_words) + "\n", encoding="utf-8")
    (d / "tokenizer_config.json").write_text(json.dumps({"do_lower_case": True}))
    (d / "sentence_bert_config.json").write_text(json.dumps({"max_seq_length": 256, "do_lower_case": False}))
    st = "sentence_transformers.models."
    (d / "modules.json").write_text(json.dumps([
        {"idx": 0, "name": "0", "path": "", "type": st + "Transformer"},
        {"idx": 1, "name": "1", "path": "1_Pooling", "type": st + "Pooling"},
        {"idx": 2, "name": "2", "path": "2_Normalize", "type": st + "Normalize"}]))
    (d / "1_Pooling").mkdir()
    (d / "1_Pooling" / "config.json").write_text(json.dumps({
        "word_embedding_dimension": cfg.hidden, "pooling_mode_cls_token": cfg.pooling == "cls",
        "pooling_mode_mean_tokens": cfg.pooling == "mean", "pooling_mode_max_tokens": False,
        "pooling_mode_mean_sqrt_len_tokens": False}))
    (d / "2_Normalize").mkdir()


def test_minilm_checkpoint_end_to_end_through_generator_and_storage(tmp_path):
    import random
    import string

    from claude_semantic_search_amd import Chunk, EmbeddingConfig, EmbeddingGenerator, HybridStorage, SearchConfig, StorageConfig

    rng = random.Random(3)
    words = sorted({"".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(2, 8))) for _ in range(1500)})
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    vocab += list(string.punctuation) + list(string.digits) + list(string.ascii_lowercase)
    vocab += ["##" + c for c in string.ascii_lowercase] + words
    vocab = list(dict.fromkeys(vocab))
    cfg = br.BertCfg(num_layers=6, vocab=len(vocab), pooling="mean", **br.SMALL)
    w = br.synth_weights(cfg, 21)
    _write_st_checkpoint(tmp_path / "all-MiniLM-L6-v2", cfg, w, vocab)

    texts = [" ".join(rng.choice(words) for _ in range(rng.randint(3, 120))) + rng.choice(["", ".", " X=1!"])
             for _ in range(200)]
    gen = EmbeddingGenerator(EmbeddingConfig(model_name=str(tmp_path / "all-MiniLM-L6-v2"), batch_size=32,
                                             show_progress=False, embeddings_as_arrays=True))
    chunks = [Chunk(f"c{i:04d}", t, {"project_name": "p"}) for i, t in enumerate(texts)]
    emb = gen.generate_embeddings(chunks)
    assert emb.shape == (200, 384) and gen.embedding_dimension == 384
    assert gen.model.get_sentence_embedding_dimension() == 384
    ids = gen.model.tokenize(texts)
    ref = br.encode(w, cfg, [list(map(int, s)) for s in ids])
    _check(emb, ref, "bf16")

    with HybridStorage(StorageConfig(data_dir=str(tmp_path / "store"), embedding_dim=384, auto_save=False)) as st:
        st.add_chunks(chunks)
        for qi in (0, 17, 123, 199):
            q = gen.generate_single_embedding(texts[qi])
            res = st.search(q, SearchConfig(top_k=10), None)
            qn = q / (np.linalg.norm(q) + 1e-8)
            en = emb / (np.linalg.norm(emb, axis=1, keepdims=True) + 1e-8)
            scores = en @ qn
            want = [f"c{i:04d}" for i in np.argsort(-scores, kind="stable")[:10]]
            got = [r.chunk_id for r in res]
            assert got[0] == f"c{qi:04d}"
            # same top-k set (ties of near-equal scores may swap neighbours)
            assert set(got) == set(want) or np.allclose(sorted(scores)[-10:][0], sorted(r.similarity for r in res)[0],
                                                        atol=1e-5), (got, want)
    gen.model.close()
