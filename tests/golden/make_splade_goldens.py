"""Generates tests/golden/splade_*.npz.

    python tests/golden/make_splade_goldens.py

The expected logits and weights come from the in-container ``transformers.BertForMaskedLM`` built from a config (tied
word embeddings), with the seeded synthetic weights of ``tests/splade_reference.py`` loaded through
``load_state_dict``, on padded batches with their attention mask; a text's weight for term v is
``max over its un-padded tokens of log(1 + relu(logit[t, v]))``.  ``tests/splade_reference.py`` is run next to it and
must agree to 1e-5 (on the per-term maximum of the logits and on w); the measured figures are printed.

splade_small_2layer.npz: hidden 384, 12 heads x 32, ffn 1536, 2 layers.
splade_base_2layer.npz:  hidden 768, 12 heads x 64, ffn 3072, 2 layers.
Each holds, per sequence of the lengths below, ``nnz``, the 32 best ``(term, weight)``, ``wsum`` = sum(w) and for the
case ``umin``, the smallest per-token standard deviation of u (which the fp32 bar needs).  Inputs are regenerated from
the seeds at test time; only outputs are stored.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import bert_reference as br  # noqa: E402
import splade_reference as sr  # noqa: E402

OUT = Path(__file__).resolve().parent
LENGTHS = [1, 5, 7, 31, 64, 128, 255, 384]
BSEED = 11
TOP = 32
TOL = 1e-5


def hf_logit_max(cfg: br.BertCfg, w, batch, chunk=4):
    """Per sequence ``(max_t logit [V], smallest per-token std of u)``."""
    from transformers import BertConfig, BertForMaskedLM

    hf = BertForMaskedLM(BertConfig(
        vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.heads,
        intermediate_size=cfg.ffn, hidden_act="gelu", max_position_embeddings=cfg.max_pos, type_vocab_size=2,
        layer_norm_eps=cfg.ln_eps, pad_token_id=cfg.pad_id, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
        tie_word_embeddings=True)).eval()
    sd = {("bert." + k if not k.startswith("cls.") else k): v for k, v in w.items()}
    sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
    sd["cls.predictions.decoder.bias"] = sd["cls.predictions.bias"]
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
    us = []
    hook = hf.cls.predictions.transform.transform_act_fn
    if isinstance(hook, torch.nn.Module):
        handle = hook.register_forward_hook(lambda mod, inp, out: us.append(out))
    else:   # a plain function: take u from the dense layer's output instead
        handle = hf.cls.predictions.transform.dense.register_forward_hook(
            lambda mod, inp, out: us.append(torch.nn.functional.gelu(out)))
    out, umin = [], np.inf
    for c0 in range(0, len(batch), chunk):
        part = batch[c0:c0 + chunk]
        Lmax = max(len(s) for s in part)
        ids = torch.full((len(part), Lmax), cfg.pad_id, dtype=torch.long)
        mask = torch.zeros((len(part), Lmax), dtype=torch.long)
        for b, s in enumerate(part):
            ids[b, :len(s)] = torch.tensor(s)
            mask[b, :len(s)] = 1
        us.clear()
        with torch.no_grad():
            logits = hf(input_ids=ids, attention_mask=mask).logits
        for b, s in enumerate(part):
            out.append(logits[b, :len(s)].max(dim=0).values.numpy().astype(np.float32))
            umin = min(umin, float(us[0][b, :len(s)].double().std(dim=1, unbiased=False).min()))
    handle.remove()
    return out, umin


def main():
    for name, geo in (("splade_small_2layer", "small"), ("splade_base_2layer", "base")):
        cfg = br.BertCfg(num_layers=2, pooling="cls", **sr.GEOS[geo])
        w = sr.synth_weights(cfg, sr.WSEEDS[geo])
        batch = br.synth_batch(cfg, LENGTHS, BSEED)
        hf_l, hf_umin = hf_logit_max(cfg, w, batch)
        ref = [sr.sparse(w, cfg, ids) for ids in batch]
        lerr = max(float(np.abs(a - r["logit_max"]).max()) for a, r in zip(hf_l, ref))
        hf_w = [np.log1p(np.maximum(a, 0).astype(np.float64)).astype(np.float32) for a in hf_l]
        werr = max(float(np.abs(a - r["w"]).max()) for a, r in zip(hf_w, ref))
        ref_umin = min(r["umin"] for r in ref)
        print(f"{name}: |transformers - splade_reference| = {lerr:.2e} (logit maxima), {werr:.2e} (w); "
              f"umin {hf_umin:.4f} (reference {ref_umin:.4f}); nnz {[int((a > 0).sum()) for a in hf_l]}")
        assert lerr <= TOL and werr <= TOL, (name, lerr, werr)
        tops = [sr.topm(np.maximum(a, 0), TOP) for a in hf_l]
        np.savez_compressed(OUT / f"{name}.npz", lengths=np.array(LENGTHS, np.int32), wseed=sr.WSEEDS[geo], bseed=BSEED,
                            num_layers=2, umin=np.float32(hf_umin), nnz=np.array([t[2] for t in tops], np.int32),
                            terms=np.stack([t[0] for t in tops]), weights=np.stack([t[1] for t in tops]),
                            wsum=np.array([a.astype(np.float64).sum() for a in hf_w], np.float64))


if __name__ == "__main__":
    main()
