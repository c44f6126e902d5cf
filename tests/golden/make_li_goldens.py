"""Generates tests/golden/li_*.npz.

    python tests/golden/make_li_goldens.py

The expected token vectors and MaxSim scores come from the in-container ``transformers.BertModel`` built from a config
plus one ``torch.nn.Linear(H, P, bias=False)``, with the seeded synthetic weights of ``tests/li_reference.py`` loaded
through ``load_state_dict``, on padded batches with their attention mask; every token row is L2-normalised and the
score is ``sum_s max_t q_s . d_t`` over the un-padded rows.  ``tests/li_reference.py`` is run next to it and must agree
to 1e-5 (token-vector components and scores); the measured figures are printed.

li_small_2layer.npz: hidden 384, 12 heads x 32, ffn 1536, 2 layers, P = 96.
li_base_2layer.npz:  hidden 768, 12 heads x 64, ffn 3072, 2 layers, P = 128.
Each holds ``scores`` [3, 8] (queries x docs) for the lengths below, ``tokens0`` (the unit token matrix of doc 0) and
``vmin`` (the smallest token-vector norm before normalisation, which the fp32 bar needs).  Inputs are regenerated from
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
import li_reference as lr  # noqa: E402

OUT = Path(__file__).resolve().parent
LENGTHS = [5, 7, 31, 64, 128, 255, 383, 384]
QUERY_LENGTHS = [4, 17, 32]
BSEED, QSEED = 11, 23


def hf_token_vectors(cfg: br.BertCfg, w, batch, chunk=4):
    """Per sequence ``(unit rows [L, P], smallest norm before normalisation)``."""
    from transformers import BertConfig, BertModel

    hf = BertModel(BertConfig(
        vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.heads,
        intermediate_size=cfg.ffn, hidden_act="gelu", max_position_embeddings=cfg.max_pos, type_vocab_size=2,
        layer_norm_eps=cfg.ln_eps, pad_token_id=cfg.pad_id, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0),
        add_pooling_layer=False).eval()
    missing, unexpected = hf.load_state_dict({k: v for k, v in w.items() if k != "linear.weight"}, strict=False)
    assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
    lin = torch.nn.Linear(cfg.hidden, w["linear.weight"].shape[0], bias=False)
    lin.load_state_dict({"weight": w["linear.weight"]})
    rows, vmin = [], np.inf
    for c0 in range(0, len(batch), chunk):
        part = batch[c0:c0 + chunk]
        Lmax = max(len(s) for s in part)
        ids = torch.full((len(part), Lmax), cfg.pad_id, dtype=torch.long)
        mask = torch.zeros((len(part), Lmax), dtype=torch.long)
        for b, s in enumerate(part):
            ids[b, :len(s)] = torch.tensor(s)
            mask[b, :len(s)] = 1
        with torch.no_grad():
            v = lin(hf(input_ids=ids, attention_mask=mask).last_hidden_state)
            u = torch.nn.functional.normalize(v, p=2, dim=2, eps=1e-12)
        for b, s in enumerate(part):
            rows.append(u[b, :len(s)].numpy().astype(np.float32))
            vmin = min(vmin, float(v[b, :len(s)].norm(dim=1).min()))
    return rows, vmin


def main():
    for name, geo in (("li_small_2layer", "small"), ("li_base_2layer", "base")):
        cfg = br.BertCfg(num_layers=2, pooling="cls", **lr.GEOS[geo])
        w = lr.synth_weights(cfg, lr.WSEEDS[geo], lr.WIDTH[geo])
        batch = br.synth_batch(cfg, LENGTHS, BSEED)
        qb = br.synth_batch(cfg, QUERY_LENGTHS, QSEED)
        hd, vd = hf_token_vectors(cfg, w, batch)
        hq, vq = hf_token_vectors(cfg, w, qb)
        rd = [lr.token_vectors(w, cfg, ids) for ids in batch]
        rq = [lr.token_vectors(w, cfg, ids) for ids in qb]
        pairs = [(i, j) for i in range(len(qb)) for j in range(len(batch))]
        hs, rs = lr.scores(hq, hd, pairs), lr.scores(rq, rd, pairs)
        terr = max(float(np.abs(a - b).max()) for a, b in zip(hd + hq, rd + rq))
        serr = float(np.abs(hs - rs).max())
        assert terr <= 1e-5 and serr <= 1e-5, (name, terr, serr)
        print(f"{name}: |transformers - li_reference| = {terr:.2e} (token components), {serr:.2e} (scores); "
              f"vmin {min(vd, vq):.3f}; scores of query 2 {np.round(hs.reshape(3, -1)[2], 3).tolist()}")
        np.savez_compressed(OUT / f"{name}.npz", lengths=np.array(LENGTHS, np.int32),
                            query_lengths=np.array(QUERY_LENGTHS, np.int32), wseed=lr.WSEEDS[geo], bseed=BSEED, qseed=QSEED,
                            width=lr.WIDTH[geo], num_layers=2, vmin=np.float32(min(vd, vq)), tokens0=hd[0],
                            scores=hs.reshape(len(qb), len(batch)))


if __name__ == "__main__":
    main()
