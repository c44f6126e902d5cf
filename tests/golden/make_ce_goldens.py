"""Generates tests/golden/ce_*.npz.

    python tests/golden/make_ce_goldens.py

The expected logits come from the in-container ``transformers.BertForSequenceClassification`` (one label) built from a
config, with the seeded synthetic weights of ``tests/ce_reference.py`` loaded through ``load_state_dict``, on padded
batches with their attention mask and per-token type ids.  ``tests/ce_reference.py`` is run next to it and must agree
to 1e-5.  Where a slow ``BertTokenizer`` can be built from a toy ``vocab.txt``, ``build_pair`` (the product's and the
reference's) is also checked against ``tokenizer(a, b, truncation=True, max_length=L)``: ids and type ids.

ce_small_2layer.npz: hidden 384, 12 heads x 32, ffn 1536, 2 layers.
ce_base_2layer.npz:  hidden 768, 12 heads x 64, ffn 3072, 2 layers.
Each holds ``logits`` [8] for the lengths / seg_starts below, weights seeds ``ce_reference.WSEEDS``, token
seed 11.  Inputs are regenerated
from the seeds at test time; only outputs are stored.
"""
import random
import string
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import bert_reference as br  # noqa: E402
import ce_reference as cr  # noqa: E402

OUT = Path(__file__).resolve().parent
LENGTHS = [5, 7, 31, 64, 128, 255, 383, 384]
SEG_STARTS = [3, 2, 16, 63, 64, 2, 200, 1]
BSEED = 11


def hf_logits(cfg: br.BertCfg, w, batch, seg_starts, chunk=4) -> np.ndarray:
    from transformers import BertConfig, BertForSequenceClassification

    hf = BertForSequenceClassification(BertConfig(
        vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.heads,
        intermediate_size=cfg.ffn, hidden_act="gelu", max_position_embeddings=cfg.max_pos, type_vocab_size=2,
        layer_norm_eps=cfg.ln_eps, pad_token_id=cfg.pad_id, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
        classifier_dropout=0.0, num_labels=1)).eval()
    sd = {("" if k.startswith("classifier.") else "bert.") + k: v for k, v in w.items()}
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
    outs = []
    for c0 in range(0, len(batch), chunk):
        part, segs = batch[c0:c0 + chunk], seg_starts[c0:c0 + chunk]
        Lmax = max(len(s) for s in part)
        ids = torch.full((len(part), Lmax), cfg.pad_id, dtype=torch.long)
        mask = torch.zeros((len(part), Lmax), dtype=torch.long)
        types = torch.zeros((len(part), Lmax), dtype=torch.long)
        for b, (s, g) in enumerate(zip(part, segs)):
            ids[b, :len(s)] = torch.tensor(s)
            mask[b, :len(s)] = 1
            types[b, g:len(s)] = 1
        with torch.no_grad():
            outs.append(hf(input_ids=ids, attention_mask=mask, token_type_ids=types).logits[:, 0].numpy())
    return np.concatenate(outs).astype(np.float32)


def check_build_pair():
    """build_pair against a slow BertTokenizer over a toy vocabulary; returns False when none can be built."""
    # the SLOW (Python) tokenizer: its longest_first is the rule build_pair restates.  transformers 5's BertTokenizer
    # is backed by the `tokenizers` library, whose LongestFirst gives the odd token of a pair cut on both sides to the
    # longer side (to b at equal lengths) where the Python rule gives it to a.
    try:
        from transformers.models.bert.tokenization_bert_legacy import BertTokenizerLegacy as BertTokenizer
    except Exception as e:  # pragma: no cover
        print(f"build_pair: no slow BertTokenizer here ({e}); not checked against transformers")
        return False
    from claude_semantic_search_amd.cross_encoder import build_pair
    from claude_semantic_search_amd.tokenizer import WordPieceTokenizer

    rng = random.Random(3)
    words = sorted({"".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(2, 8))) for _ in range(300)})
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(string.punctuation) + list(string.ascii_lowercase)
    vocab += ["##" + c for c in string.ascii_lowercase] + words
    with tempfile.TemporaryDirectory() as d:
        vp = Path(d) / "vocab.txt"
        vp.write_text("\n".join(vocab) + "\n", encoding="utf-8")
        try:
            tk = BertTokenizer(str(vp), do_lower_case=True)
        except Exception as e:  # pragma: no cover
            print(f"build_pair: BertTokenizer could not be built from vocab.txt ({e}); not checked against transformers")
            return False
        ours = WordPieceTokenizer(str(vp), lower=True)
        n = 0
        for la, lb, L in [(3, 4, 64), (30, 5, 20), (5, 30, 20), (12, 12, 20), (13, 12, 20), (40, 40, 16), (0, 9, 8),
                          (9, 0, 8), (1, 1, 5), (6, 2, 9)]:
            for _ in range(5):
                a = " ".join(rng.choice(words) for _ in range(la))
                b = " ".join(rng.choice(words) for _ in range(lb))
                enc = tk(a, b, truncation=True, max_length=L, return_token_type_ids=True)
                a_ids, b_ids = ours.encode(a, 10 ** 6)[1:-1], ours.encode(b, 10 ** 6)[1:-1]
                for fn in (build_pair, cr.build_pair):
                    ids, seg = fn(a_ids, b_ids, ours.bos, ours.eos, L)
                    assert ids == list(enc["input_ids"]), (la, lb, L, ids, enc["input_ids"])
                    assert [int(i >= seg) for i in range(len(ids))] == list(enc["token_type_ids"]), (la, lb, L)
                n += 1
    print(f"build_pair: {n} pairs match BertTokenizer(a, b, truncation=True) in ids and type ids")
    return True


def main():
    check_build_pair()
    for name, geo in (("ce_small_2layer", "small"), ("ce_base_2layer", "base")):
        cfg = br.BertCfg(num_layers=2, pooling="cls", normalize=False, **cr.GEOS[geo])
        w = cr.synth_weights(cfg, cr.WSEEDS[geo])
        batch = cr.synth_pair_batch(cfg, LENGTHS, SEG_STARTS, BSEED)
        hf = hf_logits(cfg, w, batch, SEG_STARTS)
        ref = cr.logits(w, cfg, batch, SEG_STARTS)
        err = np.abs(hf - ref).max()
        assert err <= 1e-5, (name, err)
        print(f"{name}: |transformers - ce_reference| = {err:.2e}; logits {np.round(hf, 4).tolist()}")
        np.savez_compressed(OUT / f"{name}.npz", lengths=np.array(LENGTHS, np.int32),
                            seg_starts=np.array(SEG_STARTS, np.int32), wseed=cr.WSEEDS[geo], bseed=BSEED, num_layers=2, logits=hf)


if __name__ == "__main__":
    main()
