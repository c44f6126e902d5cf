"""GPU, end to end: ``SparseEncoder`` on a 6-layer hidden-384 masked-LM checkpoint directory written by the test (tied
and untied decoder, real WordPiece tokenisation) against the fp32 PyTorch reference, and ``search_reranked``."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import splade_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu


def _write_checkpoint(d: Path, cfg, w, tied: bool):
    from safetensors.numpy import save_file

    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({
        "architectures": ["BertForMaskedLM"], "model_type": "bert", "hidden_act": "gelu", "hidden_size": cfg.hidden,
        "num_attention_heads": cfg.heads, "num_hidden_layers": cfg.num_layers, "intermediate_size": cfg.ffn,
        "vocab_size": cfg.vocab, "max_position_embeddings": cfg.max_pos, "type_vocab_size": 2,
        "layer_norm_eps": cfg.ln_eps, "pad_token_id": 0}))
    sd = {("" if k.startswith("cls.") else "bert.") + k: v.numpy() for k, v in w.items()}
    if not tied:   # an untied decoder: its own matrix, and the bias under both of its names
        sd[sr.P + "decoder.weight"] = np.ascontiguousarray(w[sr.P + "decoder.weight"].numpy())
        sd[sr.P + "decoder.bias"] = sd[sr.P + "bias"].copy()
    save_file(sd, str(d / "model.safetensors"))
    (d / "vocab.txt").write_text("\n".join(sr.E2E_WORDS) + "\n", encoding="utf-8")
    (d / "tokenizer_config.json").write_text(json.dumps({"do_lower_case": True}))


@pytest.mark.parametrize("compute", ["bf16", "fp32"])
@pytest.mark.parametrize("tied", [True, False], ids=["tied", "untied"])
def test_checkpoint_end_to_end(tmp_path, tied, compute):
    """Every leg runs under its own bar on z (``splade_reference.e2e_z_bar``: bf16 twice the measured 6-layer figure,
    fp32 the propagated bound); ``test_sparse_host.py::test_ranking_check_binds`` counts, per leg, the adjacent pairs
    that the order check below binds."""
    from claude_semantic_search_amd import Chunk, HybridStorage, Reranked, SearchConfig, SparseEncoder, StorageConfig, synth

    cfg = sr.e2e_cfg()
    w = sr.e2e_weights(tied)
    _write_checkpoint(tmp_path / "splade-small", cfg, w, tied)
    docs, query = sr.e2e_documents(), sr.E2E_QUERY
    rq = sr.sparse(w, cfg, sr.e2e_ids(query))
    rd = [sr.sparse(w, cfg, sr.e2e_ids(t)) for t in docs]
    zbar = sr.e2e_z_bar(w, compute, [rq] + rd)
    what = f"{'tied' if tied else 'untied'} {compute}"
    with SparseEncoder(str(tmp_path / "splade-small"), compute=compute) as enc:
        assert enc.cfg["num_layers"] == 6 and enc.cfg["vocab"] == sr.E2E_VOCAB
        assert enc.text_ids([query, docs[3]]) == [sr.e2e_ids(query), sr.e2e_ids(docs[3])]
        # the 6-layer bar on z, measured through the dense output of the same ids
        ids = [sr.e2e_ids(t) for t in [query] + docs]
        z = enc.encoder.encode_sparse_ids(ids, 256, return_dense=True)[3]
        worst = max(float(np.abs(z[i] - r["z"]).max()) for i, r in enumerate([rq] + rd))
        print(f"[sparse e2e] {what} 6 layers: max |z - z_ref| = {worst:.3e} (bar {zbar:.3e})")
        assert worst <= zbar
        qv, dv = enc.encode_queries([query])[0], enc.encode_documents(docs, batch_size=3)
        for v, r, m in [(qv, rq, 64)] + [(v, r, 256) for v, r in zip(dv, rd)]:
            assert 0 < len(v.terms) <= m
            assert np.abs(v.weights - r["w"][v.terms]).max() <= zbar      # log1p o relu is 1-Lipschitz
            assert np.all(np.diff(v.weights) <= 0)
        ref, bars, order, bound = sr.e2e_ranking(rq, rd, zbar)
        out = enc.predict([(query, t) for t in docs], batch_size=3)
        assert np.array_equal(out, enc.score([qv], dv))
        err = np.abs(out.astype(np.float64) - ref)
        print(f"[sparse e2e] {what}: max |score - ref| = {err.max():.3e}, bars {np.round(bars, 4).tolist()}, the order "
              f"check binds {int(bound.sum())} of {bound.size} adjacent pairs")
        assert (err <= bars).all()
        ranked = enc.rank(query, docs, return_documents=True)
        got = [h["corpus_id"] for h in ranked]
        assert sorted(got) == list(range(len(docs))) and all(h["text"] == docs[h["corpus_id"]] for h in ranked)
        pos = {c: n for n, c in enumerate(got)}
        for a, b, must in zip(order[:-1], order[1:], bound):
            assert not must or pos[int(a)] < pos[int(b)]
        assert [h["corpus_id"] for h in enc.rank(query, docs, top_k=3)] == got[:3]
        # reading a vector
        dec = enc.decode(dv[-1], 5)
        assert [wd for wd, _ in dec] == [sr.E2E_WORDS[int(t)] for t in dv[-1].terms[:5]]
        own = set(sr.e2e_ids(docs[-1]))
        exp = enc.expansion(docs[-1], n=6)
        assert len(exp) == 6 and all(sr.E2E_WORDS.index(wd) not in own for wd, _ in exp)
        if not tied or compute != "bf16":
            return
        rng = np.random.default_rng(2)
        texts = [" ".join(f"w{int(i)}" for i in rng.integers(0, sr.E2E_VOCAB - 4, size=int(rng.integers(3, 60)))) for _ in range(60)]
        emb = synth.rows(60, 64, 9)
        chunks = [Chunk(f"c{i:04d}", t, {"project_name": "p"}, emb[i]) for i, t in enumerate(texts)]
        with HybridStorage(StorageConfig(data_dir=str(tmp_path / "store"), embedding_dim=64, auto_save=False)) as st:
            st.add_chunks(chunks)
            q = emb[17] + 0.5 * emb[40]
            plain = st.search(q, SearchConfig(top_k=30), None)
            res = st.search_reranked(query, q, enc, SearchConfig(top_k=10), None, fetch=30)
            assert len(res) == 10 and all(isinstance(r, Reranked) for r in res)
            allp = enc.predict([(query, p.text) for p in plain])
            assert [r.score for r in res] == [float(allp[r.rank_before]) for r in res]
            assert [r.rank_before for r in res] == np.argsort(-allp, kind="stable")[:10].tolist()
