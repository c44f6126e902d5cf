"""CPU: the host half of cross-encoder re-ranking -- pair building, config parsing, ranking, the PyTorch reference
against the committed transformers goldens, and the segment-effect condition of the GPU cases."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd import cross_encoder as ce

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402
import ce_reference as cr  # noqa: E402

CLS, SEP = 101, 102


def _ids(n, base):
    return list(range(base, base + n))


# ---- build_pair ---------------------------------------------------------------------------------------------------------
def test_build_pair_without_truncation():
    a, b = _ids(3, 1000), _ids(4, 2000)
    ids, seg = ce.build_pair(a, b, CLS, SEP, 64)
    assert ids == [CLS] + a + [SEP] + b + [SEP] and seg == 5 and ids[seg] == b[0]
    assert ce.build_pair(a, b, CLS, SEP, 10) == (ids, seg)          # exactly max_length: nothing dropped


def test_build_pair_truncates_the_longer_side_first():
    a, b = _ids(30, 1000), _ids(5, 2000)
    ids, seg = ce.build_pair(a, b, CLS, SEP, 20)
    assert ids == [CLS] + a[:12] + [SEP] + b + [SEP] and seg == 14 and len(ids) == 20
    ids, seg = ce.build_pair(b, a, CLS, SEP, 20)
    assert ids == [CLS] + b + [SEP] + a[:12] + [SEP] and seg == 7
    # both sides cut: the longer one first, then alternately -- a 13 / b 12 into 17 tokens: a, then b, a, b, ...
    ids, seg = ce.build_pair(_ids(13, 1000), _ids(12, 2000), CLS, SEP, 20)
    assert seg - 2 == 9 and len(ids) - seg - 1 == 8


def test_build_pair_at_equal_lengths_drops_from_b():
    a, b = _ids(12, 1000), _ids(12, 2000)
    ids, seg = ce.build_pair(a, b, CLS, SEP, 26)
    assert ids == [CLS] + a + [SEP] + b[:11] + [SEP] and seg == 14
    ids, seg = ce.build_pair(a, b, CLS, SEP, 20)                   # 7 drops: b a b a b a b
    assert ids == [CLS] + a[:9] + [SEP] + b[:8] + [SEP] and seg == 11


def test_build_pair_with_an_empty_side():
    b = _ids(9, 2000)
    assert ce.build_pair([], b, CLS, SEP, 64) == ([CLS, SEP] + b + [SEP], 2)
    assert ce.build_pair([], b, CLS, SEP, 8) == ([CLS, SEP] + b[:5] + [SEP], 2)
    assert ce.build_pair(b, [], CLS, SEP, 64) == ([CLS] + b + [SEP, SEP], 11)
    assert ce.build_pair(b, [], CLS, SEP, 8) == ([CLS] + b[:5] + [SEP, SEP], 7)
    assert ce.build_pair([], [], CLS, SEP, 3) == ([CLS, SEP, SEP], 2)
    with pytest.raises(ValueError, match="max_length=2"):
        ce.build_pair([], [], CLS, SEP, 2)


def test_build_pair_bounds_and_agreement_with_the_reference_restatement():
    rng = np.random.default_rng(0)
    for _ in range(300):
        la, lb, L = int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(3, 48))
        a, b = _ids(la, 1000), _ids(lb, 2000)
        ids, seg = ce.build_pair(a, b, CLS, SEP, L)
        assert len(ids) <= L and len(ids) == min(L, la + lb + 3)
        assert 2 <= seg <= len(ids) - 1 and ids[0] == CLS and ids[seg - 1] == SEP and ids[-1] == SEP
        assert (ids, seg) == cr.build_pair(a, b, CLS, SEP, L)
        na, nb = seg - 2, len(ids) - seg - 1
        assert ids[1:seg - 1] == a[:na] and ids[seg:-1] == b[:nb]


# ---- config parsing -----------------------------------------------------------------------------------------------------
def _config(**over):
    c = {"architectures": ["BertForSequenceClassification"], "model_type": "bert", "hidden_act": "gelu",
         "hidden_size": 384, "num_attention_heads": 12, "num_hidden_layers": 6, "intermediate_size": 1536,
         "vocab_size": 30522, "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12,
         "pad_token_id": 0, "id2label": {"0": "LABEL_0"}, "label2id": {"LABEL_0": 0}}
    c.update(over)
    return {k: v for k, v in c.items() if v is not None}


def _dir(tmp_path, name, **over):
    d = tmp_path / name
    d.mkdir()
    (d / "config.json").write_text(json.dumps(_config(**over)))
    return d


def test_config_of_a_minilm_cross_encoder(tmp_path):
    cfg = ce.parse_cross_encoder_config(_dir(tmp_path, "ok"))
    assert (cfg["arch"], cfg["hidden"], cfg["heads"], cfg["num_layers"], cfg["ffn"]) == ("bert", 384, 12, 6, 1536)
    assert cfg["pooling"] == "cls" and cfg["normalize"] is False and cfg["max_seq_len"] == 512
    cfg = ce.parse_cross_encoder_config(_dir(tmp_path, "ok2", id2label=None, label2id=None, num_labels=1, hidden_size=768))
    assert cfg["hidden"] == 768


def test_config_refusals_name_the_field(tmp_path):
    with pytest.raises(ValueError, match="model_type 'roberta'"):
        ce.parse_cross_encoder_config(_dir(tmp_path, "roberta", model_type="roberta"))
    with pytest.raises(ValueError, match="num_labels: 2 labels"):
        ce.parse_cross_encoder_config(_dir(tmp_path, "two", num_labels=2, id2label=None, label2id=None))
    with pytest.raises(ValueError, match="id2label: 2 labels"):
        ce.parse_cross_encoder_config(_dir(tmp_path, "two_b", id2label={"0": "no", "1": "yes"}))
    with pytest.raises(ValueError, match="num_labels: 2 labels"):      # neither written: transformers' default of two
        ce.parse_cross_encoder_config(_dir(tmp_path, "none", id2label=None, label2id=None))
    with pytest.raises(ValueError, match="hidden_size 128"):
        ce.parse_cross_encoder_config(_dir(tmp_path, "h128", hidden_size=128, num_attention_heads=2))
    with pytest.raises(ValueError, match="hidden_act 'relu'"):
        ce.parse_cross_encoder_config(_dir(tmp_path, "relu", hidden_act="relu"))


def test_a_checkpoint_without_the_head_is_refused():
    cfg = br.BertCfg(num_layers=1, vocab=50, **br.SMALL)
    w = {k: v.numpy() for k, v in cr.synth_weights(cfg, 3).items()}
    sd = {("" if k.startswith("classifier.") else "bert.") + k: v for k, v in w.items()}
    body, head = ce.split_state_dict(sd)
    assert sorted(head) == sorted(["pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias"])
    assert len(body) == len(sd) - 4 and not any("pooler" in k or "classifier" in k for k in body)
    assert ce.split_state_dict(w)[1].keys() == head.keys()          # names without the bert. prefix
    for drop in ("classifier.weight", "bert.pooler.dense.bias"):
        bad = {k: v for k, v in sd.items() if k != drop}
        with pytest.raises(ValueError, match=drop.replace("bert.", "") + r".*not a cross-encoder"):
            ce.split_state_dict(bad)


def test_synthetic_head_is_the_reference_head():
    for geo in ("small", "base"):
        cfg = br.BertCfg(num_layers=1, vocab=50, **cr.GEOS[geo])
        wp, bp, wc, bc = cr.head_arrays(cr.synth_weights(cfg, 7))
        h = ce.synth_head(cfg.hidden, 7)
        assert np.array_equal(h["pooler_w"], wp) and np.array_equal(h["pooler_b"], bp)
        assert np.array_equal(h["cls_w"], wc) and np.array_equal(h["cls_b"], bc)
        assert abs(wp.std() - 0.02) < 1e-3 and abs(wc.std() - 0.05) < 1e-2
    ids = {tid for tid, _ in ce.HEAD_SYNTH.values()}
    assert len(ids) == 4 and all(5 < t < 16 for t in ids)             # free: the body uses 0-5 and 16 + 16 layer + 0..15


# ---- rank -----------------------------------------------------------------------------------------------------------------
class _Stub(ce.CrossEncoder):
    """rank() over a fixed score per document (no encoder)."""

    def __init__(self, scores):
        self.scores = scores
        self.seen = None

    def predict(self, pairs, batch_size=32, activation=None):
        self.seen = list(pairs)
        return np.asarray([self.scores[d] for _, d in pairs], dtype=np.float32)


def test_rank_order_ties_top_k_and_documents():
    docs = ["a", "b", "c", "d", "e"]
    stub = _Stub({"a": 0.5, "b": 2.0, "c": 0.5, "d": -1.0, "e": 2.0})
    hits = stub.rank("q", docs)
    assert stub.seen == [("q", d) for d in docs]
    assert [h["corpus_id"] for h in hits] == [1, 4, 0, 2, 3]          # best first, ties to the lower corpus_id
    assert [h["score"] for h in hits] == [2.0, 2.0, 0.5, 0.5, -1.0] and all(set(h) == {"corpus_id", "score"} for h in hits)
    assert [h["corpus_id"] for h in stub.rank("q", docs, top_k=2)] == [1, 4]
    assert stub.rank("q", docs, top_k=0) == [] and len(stub.rank("q", docs, top_k=99)) == 5
    hits = stub.rank("q", docs, top_k=3, return_documents=True)
    assert [(h["corpus_id"], h["text"]) for h in hits] == [(1, "b"), (4, "e"), (0, "a")]
    assert stub.rank("q", []) == []


# ---- the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,geo", [("ce_small_2layer", "small"), ("ce_base_2layer", "base")])
def test_reference_matches_the_committed_goldens(name, geo):
    g = np.load(HERE / "golden" / f"{name}.npz")
    cfg = br.BertCfg(num_layers=int(g["num_layers"]), pooling="cls", normalize=False, **cr.GEOS[geo])
    lens, segs = g["lengths"].tolist(), g["seg_starts"].tolist()
    batch = cr.synth_pair_batch(cfg, lens, segs, int(g["bseed"]))
    ref = cr.logits(cr.synth_weights(cfg, int(g["wseed"])), cfg, batch, segs)
    assert np.abs(ref - g["logits"]).max() <= 1e-5


@pytest.mark.parametrize("geo", ["small", "base"])
def test_segment_effect_of_the_gpu_cases(geo):
    """For every case of the GPU tests, the reference logits computed with ALL token types 0 differ from the true ones
    by more than 10 x the bf16 bar: a kernel that drops the type row cannot pass."""
    cfg = br.BertCfg(num_layers=2, pooling="cls", normalize=False, **cr.GEOS[geo])
    w = cr.synth_weights(cfg, cr.WSEEDS[geo])
    g = np.load(HERE / "golden" / f"ce_{geo}_2layer.npz")
    cases = cr.CASES + [cr.BIG_CASE, (g["lengths"].tolist(), g["seg_starts"].tolist())]
    seen, weak = set(), []
    for lens, segs in cases:
        batch = cr.synth_pair_batch(cfg, lens, segs, cr.BSEED)
        d = np.abs(cr.logits(w, cfg, batch, segs) - cr.logits(w, cfg, batch, lens))
        print(f"[ce] segment effect {geo} {lens} {segs}: max {d.max():.3e} (10 x bar = {10 * cr.BF16_BAR:.3e})")
        if not d.max() > 10 * cr.BF16_BAR:
            weak.append((lens, segs, float(d.max())))
        for l, s in zip(lens, segs):
            seen |= {"1"} if s == 1 else {"2"} if s == 2 else {"len"} if s == l else {"len-1"} if s == l - 1 else {"mid"}
    assert not weak, weak
    assert seen == {"1", "2", "mid", "len-1", "len"}
