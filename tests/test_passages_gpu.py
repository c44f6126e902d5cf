"""GPU: span pooling on the encoder (``css_encoder_forward_spans``: k_span_pool on the unfolded paths, k_span_pool_ln on
the LayerNorm-folded one) and ``best_passages`` on top of it.  2-layer synthetic encoders, as tests/test_encoder_gpu.py
builds them.

Span set per sequence of length ``len`` (``_spans``): [0,1), [len-1,len), [0,len), [3,4), [15,17) (crosses a 16-token
block), [16,32), the overlapping [5,30) and [10,20), the latter twice -- each where ``len`` allows --, sequences listed
last to first, one sequence without a span.  Lengths are no multiples of 16, so cu[b] % 16 != 0 and the global-token
classes of the blocked layout are exercised."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd._native import CssError
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # unit roundoff of fp32
LENGTHS = [5, 17, 33, 64, 21, 47]   # 187 tokens: the unfolded paths; cu = 0, 5, 22, 55, 119, 140
NO_SPAN = 4                          # the sequence that gets no span
FOLDED_LENGTHS = [40] * 26           # 1040 tokens: forward_folded_bf16 (>= 1024)
TILING = [(0, 7), (7, 16), (16, 17), (17, 33), (33, 40)]   # spans that tile a sequence of 40 tokens

# bf16 mode against the fp32 oracle, 1 - cos per span, worst over the three SEEDS at the shapes of this file (measured on
# one MI355X with these very tests; the same batch gives the same bits, so the spread is across inputs only):
#   small-batch path  spans of 1 token 8.31e-6, of 2..3 tokens 7.32e-6, of >= 4 tokens 7.12e-6
#   folded path       spans of 1 token 9.57e-6, of 2..3 tokens 9.25e-6, of >= 4 tokens 7.42e-6
# Every span, single tokens included, stays two orders of magnitude inside the project's whole-sequence bound 1 - 1e-3.
# Asserted: twice the worst measured deficit (a factor of two for unseen seeds).
BF16_SPAN_DEFICIT_MEASURED = 9.57e-6
BF16_SPAN_DEFICIT_BOUND = 2 * BF16_SPAN_DEFICIT_MEASURED
SEEDS = [(7, 11), (8, 12), (9, 13)]     # (weights, batch)


def _spans(lengths, skip):
    out = []
    for b in reversed(range(len(lengths))):
        if b == skip:
            continue
        L = lengths[b]
        for lo, hi in [(0, 1), (L - 1, L), (0, L), (3, 4), (15, 17), (16, 32), (5, 30), (10, 20), (10, 20)]:
            if 0 <= lo < hi <= L:
                out.append((b, lo, hi))
    return out


def _mpnet(layers=2):
    from oracle import mpnet_oracle as mo

    return mo, mo.MpnetCfg(num_layers=layers)


@functools.lru_cache(maxsize=8)
def _oracle_rows(wseed, bseed, lengths):
    """fp32 oracle: the [L, H] last hidden state of every sequence (computed once per case, shared)."""
    import torch

    mo, cfg = _mpnet()
    batch = mo.synth_batch(cfg, list(lengths), seed=bseed)
    w = mo.synth_weights(cfg, wseed)
    with torch.no_grad():
        rows = [mo.encode_tokens(w, cfg, ids).double().numpy() for ids in batch]
    for r in rows:
        r.setflags(write=False)
    return batch, rows


def _oracle_spans(rows, spans):
    m = np.stack([rows[b][lo:hi].mean(0) for b, lo, hi in spans])
    return m / np.linalg.norm(m, axis=1, keepdims=True)


def _bert(geo, pooling):
    import bert_reference as br

    cfg = br.BertCfg(num_layers=2, pooling=pooling, **(br.SMALL if geo == "small" else br.BASE))
    return cfg, br.synth_batch(cfg, LENGTHS, 11)


def _encoder(kind, compute):
    """(encoder, batch) of the unfolded-path cases."""
    if kind == "mpnet":
        mo, cfg = _mpnet()
        return MpnetEncoder(synthetic_seed=7, compute=compute, cfg_overrides={"num_layers": 2}), mo.synth_batch(cfg, LENGTHS, seed=11)
    cfg, batch = _bert("small", "mean")
    return MpnetEncoder(synthetic_seed=7, compute=compute, cfg_overrides=cfg.encoder_overrides()), batch


# ---- 1. exactness on the device's own rows (unfolded paths)

@pytest.mark.parametrize("kind,compute", [("mpnet", "fp32"), ("mpnet", "bf16"), ("bert384", "fp32"), ("bert384", "bf16")])
def test_span_rows_are_the_means_of_the_devices_own_token_rows(kind, compute):
    enc, batch = _encoder(kind, compute)
    H = enc.get_sentence_embedding_dimension()
    assert H == (768 if kind == "mpnet" else 384)
    spans = _spans(LENGTHS, NO_SPAN)
    cu = np.concatenate([[0], np.cumsum(LENGTHS)])
    T = int(cu[-1])
    q = np.random.default_rng(1).standard_normal(H).astype(np.float32)
    seq, raw, raw_scores = enc.encode_spans_ids(batch, spans, normalize=False, query=q)
    x = enc.debug_read("x32", (T, H)).astype(np.float64)          # the device's own final hidden states
    assert np.array_equal(seq, enc.encode_ids(batch, normalize=False))
    seq_n, out, scores = enc.encode_spans_ids(batch, spans, normalize=True, query=q)
    assert np.array_equal(enc.debug_read("x32", (T, H)).astype(np.float64), x)     # same forward, same rows
    assert np.array_equal(seq_n, enc.encode_ids(batch, normalize=True))
    enc.close()
    worst = 0.0
    for s, (b, lo, hi) in enumerate(spans):
        rows = x[cu[b] + lo:cu[b] + hi]
        n = hi - lo
        m = rows.mean(0)
        # an fp32 running sum of n terms is off by at most n u sum|x| (n - 1 additions, then the rounding of the
        # division), the mean by that over n
        delta = U * np.abs(rows).sum(0)
        err = np.abs(raw[s] - m)
        assert (err <= delta).all(), (s, (b, lo, hi), float((err / np.maximum(delta, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(delta, 1e-300)).max())) if n > 1 else worst
        if n == 1:
            assert np.array_equal(raw[s], rows[0].astype(np.float32))      # one row: the row itself
        # Normalised row r = m / ||m|| against v / nrm of the device, v = m + dv with |dv_c| <= delta_c:
        #   |v_c / nrm - r_c| <= delta_c / ||m|| + |r_c| | ||m|| / nrm - 1 | + u |r_c|              (the division)
        #   | nrm - ||m|| | <= ||delta||_2 + 8 u ||m||: the squares (u each), a summation tree of depth 12 (3 per
        #   thread, 6 wave steps, 3 partials) and the square root: (13 u) / 2 + u <= 8 u on the norm
        nm = np.linalg.norm(m)
        r = m / nm
        bound = delta / nm + np.abs(r) * (np.linalg.norm(delta) / nm + 8 * U) + U * np.abs(r)
        bound = bound * (1 + 1e-3)                                           # second-order terms of the above
        assert (np.abs(out[s] - r) <= bound).all(), (s, (b, lo, hi))
        # scores: the fp32 dot of q with the row AS WRITTEN, same tree of depth 12 after the products: 13 u sum|q v|
        for got, row in ((scores[s], out[s]), (raw_scores[s], raw[s])):
            exact = float(q.astype(np.float64) @ row.astype(np.float64))
            assert abs(float(got) - exact) <= 13 * U * float(np.abs(q.astype(np.float64) * row).sum()), (s, got, exact)
    print(f"[{kind} {compute}] worst |span_out - mean| / (u sum|x|) over spans of > 1 token: {worst:.3f}")


# ---- 2. oracle parity

def test_fp32_mode_span_rows_match_the_oracle():
    batch, rows = _oracle_rows(7, 11, tuple(LENGTHS))
    spans = _spans(LENGTHS, NO_SPAN)
    enc = MpnetEncoder(synthetic_seed=7, compute="fp32", cfg_overrides={"num_layers": 2})
    seq, out, _ = enc.encode_spans_ids(batch, spans)
    assert np.array_equal(seq, enc.encode_ids(batch))
    enc.close()
    err = np.abs(out - _oracle_spans(rows, spans)).max()
    print(f"fp32 mode: max |span_out - oracle| = {err:.2e}")
    assert err < 1e-4, err        # the project's 2-layer bound for pooled rows (test_committed_goldens_2layer_and_probes)


def bf16_span_deficits(wseed, bseed, lengths, skip, extra=()):
    """1 - cos of every span row of a bf16 encoder against the fp32 oracle, by span length class."""
    batch, rows = _oracle_rows(wseed, bseed, tuple(lengths))
    spans = _spans(lengths, skip) + list(extra)
    enc = MpnetEncoder(synthetic_seed=wseed, compute="bf16", cfg_overrides={"num_layers": 2})
    seq, out, _ = enc.encode_spans_ids(batch, spans)
    assert np.array_equal(seq, enc.encode_ids(batch))
    folded = False
    try:
        enc.debug_read("x32", (sum(lengths), 768))
    except RuntimeError:
        folded = True                                  # x32 is not materialised on the LayerNorm-folded path
    enc.close()
    assert np.abs(np.linalg.norm(out, axis=1) - 1).max() < 1e-5
    deficit = 1.0 - (out.astype(np.float64) * _oracle_spans(rows, spans)).sum(1)
    n = np.array([hi - lo for _, lo, hi in spans])
    classes = {"1": deficit[n == 1].max(), "2-3": deficit[(n > 1) & (n < 4)].max(), ">=4": deficit[n >= 4].max()}
    return classes, folded


@pytest.mark.parametrize("wseed,bseed", SEEDS)
def test_bf16_mode_span_rows_match_the_oracle(wseed, bseed):
    classes, folded = bf16_span_deficits(wseed, bseed, LENGTHS, NO_SPAN)
    print(f"bf16 small-batch path, seeds ({wseed}, {bseed}): worst 1 - cos by span length: "
          + ", ".join(f"{k}: {v:.2e}" for k, v in classes.items()))
    assert not folded
    assert max(classes.values()) <= BF16_SPAN_DEFICIT_BOUND, classes
    assert classes[">=4"] < 1e-3           # spans of >= 4 tokens inside the whole-sequence bound of the project


# ---- 3. the LayerNorm-folded path

@pytest.mark.parametrize("wseed,bseed", SEEDS)
def test_folded_path_span_rows_match_the_oracle(wseed, bseed):
    classes, folded = bf16_span_deficits(wseed, bseed, FOLDED_LENGTHS, 7, extra=[(3, lo, hi) for lo, hi in TILING])
    print(f"bf16 folded path, seeds ({wseed}, {bseed}): worst 1 - cos by span length: "
          + ", ".join(f"{k}: {v:.2e}" for k, v in classes.items()))
    assert folded                           # T = 1040 >= 1024 takes forward_folded_bf16
    assert max(classes.values()) <= BF16_SPAN_DEFICIT_BOUND, classes
    assert classes[">=4"] < 1e-3


def test_folded_path_spans_that_tile_a_sequence_add_up_to_its_pooled_row():
    mo, cfg = _mpnet()
    batch = mo.synth_batch(cfg, FOLDED_LENGTHS, seed=11)
    tiled = [0, 3, 13, 25]                  # cu = 0, 120, 520, 1000: token classes 0, 8, 8, 8 at the sequence start
    spans = [(b, lo, hi) for b in reversed(tiled) for lo, hi in TILING]
    enc = MpnetEncoder(synthetic_seed=7, compute="bf16", cfg_overrides={"num_layers": 2})
    seq, out, _ = enc.encode_spans_ids(batch, spans, normalize=False)
    with pytest.raises(RuntimeError):
        enc.debug_read("x32", (sum(FOLDED_LENGTHS), 768))      # the folded path ran
    assert np.array_equal(seq, enc.encode_ids(batch, normalize=False))
    gamma = enc.export_weight("encoder.layer.1.output.LayerNorm.weight", (768,))
    beta = enc.export_weight("encoder.layer.1.output.LayerNorm.bias", (768,))
    enc.close()
    # A LayerNorm output is bounded by |gamma| sqrt(H) + |beta|; two fp32 sums of len terms are compared.  About 1e-4 at
    # len = 40, while a dropped or doubled token moves the sum by a whole row
    L = 40
    tol = 2 * L * U * (np.abs(gamma).max() * np.sqrt(768.0) + np.abs(beta).max())
    worst = 0.0
    for i, b in enumerate(reversed(tiled)):
        parts = out[i * len(TILING):(i + 1) * len(TILING)].astype(np.float64)
        total = sum((hi - lo) * parts[j] for j, (lo, hi) in enumerate(TILING))
        worst = max(worst, float(np.abs(total - L * seq[b].astype(np.float64)).max()))
    print(f"partition identity: worst |sum len_i span_i - len seq_out| = {worst:.2e}, tolerance {tol:.2e}")
    assert worst <= tol, (worst, tol)


# ---- 4. seq_out on a CLS-pooling encoder: the CLS row, while spans are means

@pytest.mark.parametrize("lengths", [LENGTHS, FOLDED_LENGTHS], ids=["small-batch", "folded"])
def test_cls_pooling_encoder_seq_out_is_the_cls_row_and_spans_are_means(lengths):
    import bert_reference as br

    cfg = br.BertCfg(num_layers=2, pooling="cls", **br.BASE)
    batch = br.synth_batch(cfg, lengths, 11)
    enc = MpnetEncoder(synthetic_seed=7, compute="bf16", cfg_overrides=cfg.encoder_overrides())
    spans = [(b, 0, 1) for b in range(len(lengths))] + [(b, 0, lengths[b]) for b in range(len(lengths))]
    seq, out, _ = enc.encode_spans_ids(batch, spans)
    assert np.array_equal(seq, enc.encode_ids(batch))
    enc.close()
    B = len(lengths)
    # the span [0, 1) is the CLS row as well (another kernel: equal up to the rounding of the norm) ...
    assert np.abs(out[:B] - seq).max() < 1e-6
    # ... and the whole-sequence span is the MEAN, not the CLS row
    assert all(float(out[B + b] @ seq[b]) < 0.999 for b in range(B) if lengths[b] > 1)


# ---- 5. call shapes and errors

def test_call_shapes_errors_and_the_captured_graph_survives():
    mo, cfg = _mpnet()
    batch = mo.synth_batch(cfg, LENGTHS, seed=11)
    spans = _spans(LENGTHS, NO_SPAN)
    enc = MpnetEncoder(synthetic_seed=7, compute="bf16", cfg_overrides={"num_layers": 2})
    one = [0, 17, 923, 4055, 12000, 2]
    first = enc.encode_ids([one])
    for _ in range(3):                                     # eager, capture, replay
        assert np.array_equal(first, enc.encode_ids([one]))
    q = np.random.default_rng(2).standard_normal(768).astype(np.float32)
    a = enc.encode_spans_ids(batch, spans, query=q)
    b = enc.encode_spans_ids(batch, spans, query=q)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                # the same call gives the same bits
    assert a[0].shape == (6, 768) and a[1].shape == (len(spans), 768) and a[2].shape == (len(spans),)
    assert np.array_equal(first, enc.encode_ids([one]))                    # the captured graph survived
    # S == 0
    seq, out, sc = enc.encode_spans_ids(batch, [])
    assert np.array_equal(seq, a[0]) and out.shape == (0, 768) and sc is None
    seq, out, sc = enc.encode_spans_ids(batch, [], query=q)
    assert sc.shape == (0,)
    # span_out NULL, scores only
    seq, out, sc = enc.encode_spans_ids(batch, spans, query=q, span_rows=False)
    assert out is None and np.array_equal(sc, a[2]) and np.array_equal(seq, a[0])
    # more spans than ever before: the span buffers grow, the graph stays
    many = spans * 40
    big = enc.encode_spans_ids(batch, many, query=q)
    assert np.array_equal(big[1][:len(spans)], a[1]) and np.array_equal(big[1][-len(spans):], a[1])
    assert np.array_equal(big[2], np.tile(a[2], 40))
    assert np.array_equal(first, enc.encode_ids([one]))
    # bad spans: named, nothing enqueued, the encoder stays usable
    ok = [(0, 0, 5), (1, 2, 9)]
    for bad, what in (((1, 4, 4), r"span 2 is \[4, 4\)"), ((1, 9, 3), r"span 2 is \[9, 3\)"), ((1, 3, 18), r"span 2 is \[3, 18\)"),
                      ((1, -1, 3), r"span 2 is \[-1, 3\)"), ((6, 0, 1), "span 2 names sequence 6"),
                      ((-1, 0, 1), "span 2 names sequence -1")):
        with pytest.raises(CssError, match=what):
            enc.encode_spans_ids(batch, ok + [bad] + ok)
    with pytest.raises(ValueError, match=r"\[S, 3\]"):
        enc.encode_spans_ids(batch, [(0, 1)])
    with pytest.raises(ValueError, match="hidden size"):
        enc.encode_spans_ids(batch, spans, query=np.ones(5, np.float32))
    with pytest.raises(RuntimeError):
        enc.encode_spans_ids([[0, 5, 1, 2]], [(0, 0, 1)])                  # the batch rules of encode_ids hold
    again = enc.encode_spans_ids(batch, spans, query=q)
    assert all(np.array_equal(x, y) for x, y in zip(a, again))
    assert np.array_equal(first, enc.encode_ids([one]))
    enc.close()


# ---- 6. end to end

def test_best_passages_ranks_like_encode_spans_ids_plus_numpy():
    """The synthetic encoder's vectors are not meaningful text embeddings, so the check is not "passage j wins":
    ``best_passages`` must return what ``encode_spans_ids`` over the same spans plus a numpy ranking gives."""
    from claude_semantic_search_amd.embeddings import EmbeddingConfig, EmbeddingGenerator
    from claude_semantic_search_amd.passages import pack_passages, split_passages
    from claude_semantic_search_amd.storage import SearchResult

    rng = np.random.default_rng(4)
    vocab = [f"w{i}" for i in range(500)]

    def sentence():
        return " ".join(rng.choice(vocab, size=int(rng.integers(5, 30)))) + rng.choice([".", "!", "?", ""])

    texts = ["\n".join(sentence() for _ in range(6)), " ".join(sentence() for _ in range(12)), "",
             " ".join(sentence() for _ in range(60))]                        # the last one spills over 384 tokens
    enc = MpnetEncoder(synthetic_seed=3, compute="bf16", cfg_overrides={"num_layers": 2})
    body = lambda s: [int(t) for t in enc.tokenize([s])[0]][1:-1]             # noqa: E731
    ranges = [split_passages(t, lambda s: len(body(s))) for t in texts]
    j = 2
    a, b = ranges[1][j]
    qv = enc.encode_ids([[0] + body(texts[1][a:b]) + [2]])[0]               # passage j of text 1, verbatim, as the query
    res = enc.best_passages(qv, texts, n=3)
    batch, spans, owner = [], [], []
    for ti, t in enumerate(texts):
        if not ranges[ti]:
            continue
        seqs, sp = pack_passages([body(t[x:y]) for x, y in ranges[ti]], enc.max_seq_length)
        spans += [(len(batch) + s, lo, hi) for s, lo, hi in sp]
        owner += [ti] * len(sp)
        batch += seqs
    assert len(batch) > 4 and max(map(len, batch)) <= 384                   # text 3 landed in more than one sequence
    _, rows, scores = enc.encode_spans_ids(batch, spans, query=qv)
    assert np.allclose(scores, rows @ qv, atol=1e-5)
    owner = np.array(owner)
    for ti, t in enumerate(texts):
        idx = np.flatnonzero(owner == ti)
        order = idx[np.argsort(-scores[idx], kind="stable")][:3]
        assert [(p.start, p.end) for p in res[ti]] == [ranges[ti][i - idx[0]] for i in order]
        assert [p.score for p in res[ti]] == [float(scores[i]) for i in order]
        assert all(p.text == t[p.start:p.end] for p in res[ti])
    assert res[2] == []
    # the generator on top: a query vector, search results carrying the chunk text
    gen = EmbeddingGenerator(EmbeddingConfig(show_progress=False))
    gen.model = enc
    assert gen.best_passages(qv, [SearchResult("c", 0.5, text=t) for t in texts], n=3) == res
    enc.close()
