"""CPU: BERT sentence-encoder support without a GPU -- config parsing of sentence-transformers directories,
the BERT test reference against the committed goldens (and live transformers), the WordPiece front end on a BERT
vocabulary, and the C ABI's checks of the new css_encoder_cfg fields."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.mpnet_encoder import parse_model_config

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402

ST = "sentence_transformers.models."


def _st_dir(d: Path, hf: dict, pooling: dict = None, modules=("Transformer", "Pooling", "Normalize")) -> Path:
    """A sentence-transformers layout: config.json at the root, modules.json, 1_Pooling/config.json."""
    d.mkdir(parents=True, exist_ok=True)
    (d / "config.json").write_text(json.dumps(hf))
    paths = {"Transformer": "", "Pooling": "1_Pooling", "Normalize": "2_Normalize", "Dense": "2_Dense"}
    (d / "modules.json").write_text(json.dumps([{"idx": i, "name": str(i), "path": paths[m], "type": ST + m}
                                               for i, m in enumerate(modules)]))
    (d / "1_Pooling").mkdir(exist_ok=True)
    p = {"word_embedding_dimension": hf.get("hidden_size", 768), "pooling_mode_cls_token": False,
         "pooling_mode_mean_tokens": True, "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False,
         "pooling_mode_weightedmean_tokens": False, "pooling_mode_lasttoken": False}
    p.update(pooling or {})
    (d / "1_Pooling" / "config.json").write_text(json.dumps(p))
    return d


MINILM = {"model_type": "bert", "hidden_act": "gelu", "hidden_size": 384, "num_attention_heads": 12,
          "num_hidden_layers": 6, "intermediate_size": 1536, "vocab_size": 30522, "max_position_embeddings": 512,
          "type_vocab_size": 2, "layer_norm_eps": 1e-12, "pad_token_id": 0}
BGE_BASE = dict(MINILM, hidden_size=768, num_hidden_layers=12, intermediate_size=3072)
CLS = {"pooling_mode_cls_token": True, "pooling_mode_mean_tokens": False}


def test_minilm_like_directory_parses(tmp_path):
    cfg = parse_model_config(_st_dir(tmp_path / "m", MINILM))
    assert (cfg["arch"], cfg["hidden"], cfg["heads"], cfg["ffn"], cfg["num_layers"]) == ("bert", 384, 12, 1536, 6)
    assert (cfg["pooling"], cfg["normalize"], cfg["pad_id"], cfg["max_pos"]) == ("mean", True, 0, 512)
    assert cfg["ln_eps"] == 1e-12 and cfg["max_seq_len"] == 512


def test_bge_like_directory_parses(tmp_path):
    cfg = parse_model_config(_st_dir(tmp_path / "b", BGE_BASE, CLS))
    assert (cfg["arch"], cfg["hidden"], cfg["heads"], cfg["pooling"], cfg["normalize"]) == ("bert", 768, 12, "cls", True)
    cfg = parse_model_config(_st_dir(tmp_path / "c", BGE_BASE, CLS, modules=("Transformer", "Pooling")))
    assert cfg["normalize"] is False


def test_bert_defaults_without_optional_keys(tmp_path):
    hf = {k: v for k, v in MINILM.items() if k not in ("layer_norm_eps", "pad_token_id", "max_position_embeddings")}
    cfg = parse_model_config(_st_dir(tmp_path / "m", hf))
    assert (cfg["ln_eps"], cfg["pad_id"], cfg["max_pos"]) == (1e-12, 0, 512)


def test_mpnet_directory_keeps_its_meaning(tmp_path):
    d = tmp_path / "mp"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"model_type": "mpnet", "num_hidden_layers": 2}))
    cfg = parse_model_config(d)
    assert (cfg["arch"], cfg["hidden"], cfg["pad_id"], cfg["max_pos"], cfg["ln_eps"]) == ("mpnet", 768, 1, 514, 1e-5)
    assert (cfg["pooling"], cfg["normalize"], cfg["max_seq_len"], cfg["num_layers"]) == ("mean", True, 384, 2)


@pytest.mark.parametrize("hf,pool,modules,field", [
    (dict(MINILM, model_type="roberta"), None, None, "model_type"),
    (dict(MINILM, hidden_act="relu"), None, None, "hidden_act"),
    (dict(MINILM, num_attention_heads=8), None, None, "head_dim"),
    (MINILM, {"pooling_mode_max_tokens": True, "pooling_mode_mean_tokens": False}, None, "pooling_mode_max_tokens"),
    (MINILM, {"pooling_mode_weightedmean_tokens": True, "pooling_mode_mean_tokens": False}, None,
     "pooling_mode_weightedmean_tokens"),
    (MINILM, {"pooling_mode_lasttoken": True, "pooling_mode_mean_tokens": False}, None, "pooling_mode_lasttoken"),
    (MINILM, None, ("Transformer", "Pooling", "Dense", "Normalize"), "Dense"),
    (dict(MINILM, hidden_size=512, num_attention_heads=8), None, None, "hidden_size"),
    (dict(MINILM, type_vocab_size=4), None, None, "type_vocab_size"),
])
def test_unsupported_fields_raise_naming_the_field(tmp_path, hf, pool, modules, field):
    d = _st_dir(tmp_path / "x", hf, pool, modules or ("Transformer", "Pooling", "Normalize"))
    with pytest.raises(ValueError, match=field):
        parse_model_config(d)


@pytest.mark.parametrize("name,geo", [("bert_small_2layer", br.SMALL), ("bert_base_2layer", br.BASE)])
def test_reference_matches_the_committed_goldens(name, geo):
    g = np.load(HERE / "golden" / f"{name}.npz")
    cfg = br.BertCfg(num_layers=int(g["num_layers"]), **geo)
    w = br.synth_weights(cfg, int(g["wseed"]))
    batch = br.synth_batch(cfg, g["lengths"].tolist(), int(g["bseed"]))
    for pooling in ("mean", "cls"):
        cfg.pooling = pooling
        err = np.abs(br.encode(w, cfg, batch) - g["emb_" + pooling]).max()
        assert err <= 2e-6, (pooling, err)


def test_reference_matches_live_transformers():
    pytest.importorskip("transformers")
    sys.path.insert(0, str(HERE / "golden"))
    import make_bert_goldens as mk

    for geo in (br.SMALL, br.BASE):
        cfg = br.BertCfg(num_layers=1, vocab=2000, **geo)
        w = br.synth_weights(cfg, 3)
        batch = br.synth_batch(cfg, [1, 9, 70], 5)
        for pooling in ("mean", "cls"):
            cfg.pooling = pooling
            assert np.abs(mk.hf_encode(cfg, w, batch) - br.encode(w, cfg, batch)).max() <= 2e-6


def _bert_vocab(path: Path):
    import random
    import string

    rng = random.Random(5)
    words = sorted({"".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(2, 8))) for _ in range(400)})
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    vocab += list(string.punctuation) + list(string.digits) + list(string.ascii_lowercase)
    vocab += ["##" + c for c in string.ascii_lowercase + string.digits] + words + ["##" + w for w in words[:100]]
    vocab += ["cafe", "naive", "über", "hello", "world", "##ing", "run", "的", "中"]
    path.write_text("\n".join(dict.fromkeys(vocab)) + "\n", encoding="utf-8")
    return words


TEXTS = ["Hello World!", "running HELLO, world... 42x", "Café naïve über ÜBER", "  tabs\tand\nnewlines  ",
         "中的 mixed 中文 text", "don't stop-believing (a+b)=c", "", "x" * 150]


def test_wordpiece_ids_equal_bert_tokenizer_on_a_bert_vocab(tmp_path):
    tr = pytest.importorskip("transformers")
    from claude_semantic_search_amd.tokenizer import WordPieceTokenizer, make_wordpiece

    vp = tmp_path / "vocab.txt"
    words = _bert_vocab(vp)
    hf = tr.BertTokenizer(str(vp), do_lower_case=True)
    texts = TEXTS + [" ".join(words[i:i + 9]) + " " + words[i] + "s" for i in range(0, 300, 30)]
    for tok in (make_wordpiece(str(vp), lower=True), WordPieceTokenizer(str(vp), lower=True)):
        assert tok.bos == hf.cls_token_id and tok.eos == hf.sep_token_id
        for t in texts:
            for L in (512, 8):
                want = hf(t, truncation=True, max_length=L)["input_ids"]
                assert tok.encode(t, L) == want, (type(tok).__name__, t, L)
        if hasattr(tok, "encode_batch"):
            got = [[int(i) for i in ids] for ids in tok.encode_batch(texts, 64)]
            assert got == [hf(t, truncation=True, max_length=64)["input_ids"] for t in texts]


def _cfg(**kw):
    base = dict(num_layers=2, hidden=384, heads=12, ffn=1536, vocab=30522, max_pos=512, rel_buckets=0, pad_id=0,
                max_seq_len=512, ln_eps=1e-12, compute=0, arch=1, pooling=0)
    base.update(kw)
    return nat.EncoderCfg(*[base[f] for f, _ in nat.EncoderCfg._fields_])


@pytest.mark.parametrize("kw,msg", [(dict(arch=2), "arch"), (dict(pooling=2), "pooling"),
                                    (dict(hidden=512, heads=8), "hidden"), (dict(heads=8), "head_dim"),
                                    (dict(arch=0), "hidden"), (dict(max_pos=500), "max_pos")])
def test_create_rejects_bad_bert_configs_before_touching_a_device(kw, msg):
    h = ctypes.c_void_p()
    rc = nat.lib().css_encoder_create(ctypes.byref(_cfg(**kw)), 0, ctypes.byref(h))
    assert rc == nat.CSS_ERR_INVALID and msg in nat.last_error(), nat.last_error()


def test_create_accepts_both_bert_geometries_up_to_the_device_check():
    if nat.device_count() > 0:
        pytest.skip("a HIP device is present (the GPU suite creates these encoders)")
    for kw in (dict(), dict(hidden=768, ffn=3072, pooling=1)):
        h = ctypes.c_void_p()
        assert nat.lib().css_encoder_create(ctypes.byref(_cfg(**kw)), 0, ctypes.byref(h)) == nat.CSS_ERR_NO_DEVICE
