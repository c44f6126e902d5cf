"""CPU side of the per-stage encoder tests (tests/test_encoder_stages_gpu.py): the float64 restatement in
tests/encoder_stage_reference.py is pinned against the oracles, and the inputs the GPU test uses are shown not to be
vacuous -- every mutant reference exceeds the derived bound, every tile edge carries probability, and the row sums of
the two weight sets lie where the fast pass / its fallback need them."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bert_reference as br  # noqa: E402
import encoder_stage_reference as sr  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden"
MODEL_NAMES = list(sr.MODELS)


# ------------------------------------------------------------------------------------------------ the helpers themselves
def test_bucket_function_equals_the_golden_table():
    table = np.load(GOLDEN / "rel_bucket_table.npy")          # rel = -511 .. 511
    assert table.shape == (1023,)
    assert [sr.rel_bucket(r) for r in range(-511, 512)] == table.astype(int).tolist()


@pytest.mark.parametrize("W", [768, 2304])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 1030])
def test_deblock_inverts_block(T, W):
    rows = np.arange(T * W, dtype=np.float64).reshape(T, W) + 1.0
    n = sr.blocked_numel(T, W)
    idx = sr.preblk_elem(np.arange(T)[:, None], np.arange(W)[None, :], W)
    assert idx.min() >= 0 and idx.max() < n and np.unique(idx).size == T * W      # injective, inside the block rows
    if T % 16 == 0:
        assert np.array_equal(np.sort(idx.ravel()), np.arange(n))                 # whole block rows: a permutation
    flat = np.zeros(n)
    flat[idx] = rows                                                              # "block": scatter by the same formula
    assert np.array_equal(sr.deblock(flat, T, W), rows)
    # the layout's defining property: the 16-byte piece (8 elements) of token t at piece (j, lg) holds columns
    # 32 j + 4 lg + {0..3} and 32 j + 16 + 4 lg + {0..3} of one 64-column block
    piece = sr.preblk_elem(0, np.array([4, 5, 6, 7, 20, 21, 22, 23]), W)
    assert np.array_equal(piece, piece[0] + np.arange(8)) and piece[0] % 8 == 0


def test_exact_roundings_match_the_ieee_conversions():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-20, 20, 200000))).astype(np.float32)
    ties = (np.arange(1, 4097, dtype=np.float32) * np.float32(2.0 ** -9) + np.float32(1.0)).astype(np.float32)  # 1 + k 2^-9: halfway cases
    for v in (x, ties, -ties, np.zeros(3, np.float32)):
        want = torch.from_numpy(v).to(torch.bfloat16).to(torch.float64).numpy()
        assert np.array_equal(sr.bf16_rne(v), want)
    d = rng.standard_normal(100000) * 1e-3
    assert np.array_equal(sr.f32(d), torch.from_numpy(d).to(torch.float32).to(torch.float64).numpy())
    assert np.array_equal(sr.bf16_ulp(np.array([1.0, 1.5, 2.0, 0.75])), np.array([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]))
    # a value just beside a boundary is ambiguous, one in the middle of a cell is not
    assert sr.bf16_ambiguous(np.array([1.0 + 2.0 ** -8 + 1e-9, 1.0 + 2.0 ** -7]), 1e-8).tolist() == [True, False]
    assert sr.qk_scale(64) == float(np.float32(0.125) * np.float32(sr.LOG2E))


# ------------------------------------------------------------------------------------------------ pinned to the oracles
def _torch_w(w):
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in w.items()}


def _exact_chain(name, lengths):
    """q / k / v and ctx of the restatement WITHOUT operand roundings (both GEMM paths), float64."""
    m = sr.MODELS[name]
    w = sr.model_weights(name)
    ids = sr.batch_ids(name, lengths)
    out = {}
    for folded in (False, True):
        y = sr.qkv64(w, m["arch"], m["heads"], m["ln_eps"], ids, folded, exact=True)["y"]
        ctx = sr.attention64(y, sr.offsets(lengths), m["heads"], m["hidden"] // m["heads"], sr.model_bias_table(name))[0]
        out[folded] = (y, ctx)
    return out


def test_restatement_agrees_with_the_mpnet_oracle():
    from oracle import mpnet_oracle as mo

    name, lengths = "mpnet768", [33, 2, 130]
    m = sr.MODELS[name]
    w = sr.model_weights(name)
    cfg = mo.MpnetCfg(num_layers=1, vocab=sr.VOCAB)
    tw = _torch_w(w)
    chain = _exact_chain(name, lengths)
    y, ctx = chain[False]
    # the two GEMM paths are the same algebra once nothing is rounded (k_fold_ln's centred weights, d and rs)
    assert np.abs(chain[True][0] - y).max() < 1e-9 * np.abs(y).max()
    cu = sr.offsets(lengths)
    H = m["hidden"]
    sc = sr.qk_scale(64)
    for b, ids in enumerate(sr.batch_ids(name, lengths)):
        probes = {}
        with torch.no_grad():
            mo.encode_tokens(tw, cfg, ids, dtype=torch.float64, probes=probes)
        x = probes["emb_ln"].numpy()
        rows = slice(int(cu[b]), int(cu[b + 1]))
        mine, _ = sr.layernorm64(sr.embedding_sum(w, "mpnet", [ids]), w["embeddings.LayerNorm.weight"].astype(np.float64),
                                 w["embeddings.LayerNorm.bias"].astype(np.float64), m["ln_eps"])
        # (the restatement adds word and position rows in fp32 as the kernels do, the oracle in float64: 2^-24 of a
        # 0.03 sum times rstd ~ 40)
        assert np.abs(mine - x).max() < 2e-7
        p = "encoder.layer.0.attention.attn."
        for j, nm in enumerate("qkv"):
            want = x @ w[p + nm + ".weight"].astype(np.float64).T + w[p + nm + ".bias"].astype(np.float64)
            got = y[rows, j * H:(j + 1) * H] / (sc if nm == "q" else 1.0)
            assert np.abs(got - want).max() < 1e-5 * np.abs(want).max(), nm
        a = ctx[rows] @ w[p + "o.weight"].astype(np.float64).T + w[p + "o.bias"].astype(np.float64) + x
        a = torch.nn.functional.layer_norm(torch.from_numpy(a), (H,), tw["encoder.layer.0.attention.LayerNorm.weight"],
                                           tw["encoder.layer.0.attention.LayerNorm.bias"], m["ln_eps"]).numpy()
        # attention output through the oracle's own O projection and LayerNorm (its next probe).  The restatement's q
        # carries the fp32 qk_scale (2^-25 relative to log2(e) / 8) on scores of up to ~45: 2e-6 on a probability.
        assert np.abs(a - probes["attn_out"].numpy()).max() < 2e-5, np.abs(a - probes["attn_out"].numpy()).max()


@pytest.mark.parametrize("name", ["bert768", "bert384"])
def test_restatement_agrees_with_the_bert_reference(name):
    lengths = [33, 2, 130]
    m = sr.MODELS[name]
    H = m["hidden"]
    w = sr.model_weights(name)
    tw = _torch_w(w)
    cfg = br.BertCfg(num_layers=1, hidden=H, heads=m["heads"], ffn=m["ffn"], vocab=sr.VOCAB)
    chain = _exact_chain(name, lengths)
    y, ctx = chain[False]
    assert np.abs(chain[True][0] - y).max() < 1e-9 * np.abs(y).max()
    cu = sr.offsets(lengths)
    F = torch.nn.functional
    p = "encoder.layer.0."
    for b, ids in enumerate(sr.batch_ids(name, lengths)):
        with torch.no_grad():
            want = br.encode_tokens(tw, cfg, ids).numpy()
            rows = slice(int(cu[b]), int(cu[b + 1]))
            x, _ = sr.layernorm64(sr.embedding_sum(w, "bert", [ids]), w["embeddings.LayerNorm.weight"].astype(np.float64),
                                  w["embeddings.LayerNorm.bias"].astype(np.float64), m["ln_eps"])
            lin = lambda t, nm: t @ tw[p + nm + ".weight"].T + tw[p + nm + ".bias"]  # noqa: E731
            a = F.layer_norm(lin(torch.from_numpy(ctx[rows]), "attention.output.dense") + torch.from_numpy(x), (H,),
                             tw[p + "attention.output.LayerNorm.weight"], tw[p + "attention.output.LayerNorm.bias"], m["ln_eps"])
            o = lin(F.gelu(lin(a, "intermediate.dense")), "output.dense")
            got = F.layer_norm(o + a, (H,), tw[p + "output.LayerNorm.weight"], tw[p + "output.LayerNorm.bias"], m["ln_eps"]).numpy()
        assert np.abs(got - want).max() < 2e-5, np.abs(got - want).max()


# ------------------------------------------------------------------------------------------------ the GPU test's inputs
def _all_batches(name):
    b = sr.BATCHES[name]
    return [tuple(x) for x in b["big"] + b["small"] + sr.SKINNY["skinny1"] + sr.SKINNY["skinny2"]]


@functools.lru_cache(maxsize=None)
def _chain(name, lengths, kind="fast"):
    """The reference chain of a batch: qkv as the device would store it (bf16 of qkv64), and attention64 on it."""
    m = sr.MODELS[name]
    qkv = sr.bf16_rne(sr.reference_qkv(name, lengths, kind)["y"])
    ref, tol, log2sum = sr.attention64(qkv, sr.offsets(lengths), m["heads"], m["hidden"] // m["heads"],
                                       sr.model_bias_table(name, kind), safe=True)
    return qkv, ref, tol, log2sum


def test_the_batches_are_what_the_issue_sets():
    base = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 383, 384}
    for name in MODEL_NAMES:
        want = base | ({511, 512} if sr.MODELS[name]["arch"] == "bert" else set())
        for part in ("big", "small"):
            lens = [L for b in sr.BATCHES[name][part] for L in b]
            assert sorted(lens) == sorted(want), (name, part)
        assert all(1024 <= sum(b) <= 2000 for b in sr.BATCHES[name]["big"]) and all(sum(b) < 1024 for b in sr.BATCHES[name]["small"])
        for b in sr.BATCHES[name]["big"] + sr.BATCHES[name]["small"]:
            assert any(o % 16 for o in sr.offsets(b)[1:-1]), "sequences must start off the 16-token grid"
    assert all(sum(b) <= 32 for b in sr.SKINNY["skinny1"]) and all(33 <= sum(b) <= 64 for b in sr.SKINNY["skinny2"])


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_scores_and_row_sums_lie_where_each_pass_needs_them(name):
    m = sr.MODELS[name]
    H, hd = m["hidden"], m["hidden"] // m["heads"]
    scores = []
    for lengths in [tuple(b) for b in sr.BATCHES[name]["small"]]:
        qkv, _, _, log2sum = _chain(name, lengths)
        assert log2sum.min() > -60 and log2sum.max() < 60, (log2sum.min(), log2sum.max())     # fast pass: inside 2^+-60
        cu = sr.offsets(lengths)
        for b in range(len(lengths)):
            for h in range(m["heads"]):
                rows = slice(int(cu[b]), int(cu[b + 1]))
                scores.append((qkv[rows, h * hd:(h + 1) * hd] @ qkv[rows, H + h * hd:H + (h + 1) * hd].T).ravel())
    scores = np.concatenate(scores)
    assert 6.0 <= scores.std() <= 10.0 and np.abs(scores).max() <= 60.0, (scores.std(), np.abs(scores).max())
    if m["arch"] == "mpnet":
        assert 1.0 <= sr.model_bias_table(name).std() / sr.LOG2E <= 2.0
    # fallback weights: a row sum outside the kernel's own 2^+-100 window, so the default setting has to fall back
    for part in ("small", "big"):
        lengths = tuple(sr.BATCHES[name][part][0])
        _, ref, tol, log2sum = _chain(name, lengths, "fallback")
        assert np.abs(log2sum).max() > 100 and np.isfinite(ref).all() and np.isfinite(tol).all()


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_every_edge_position_carries_probability(name):
    m = sr.MODELS[name]
    for lengths in [tuple(b) for b in sr.BATCHES[name]["big"] + sr.BATCHES[name]["small"]]:
        bad = sr.edge_coverage(_chain(name, lengths)[0], sr.offsets(lengths), m["heads"], m["hidden"] // m["heads"],
                               sr.model_bias_table(name))
        assert not bad, bad


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_every_attention_mutant_exceeds_the_bound(name):
    """On the reference chain of every batch, against the LARGER of the two bounds (the running-maximum pass's)."""
    m = sr.MODELS[name]
    bias = sr.model_bias_table(name)
    for lengths in [tuple(b) for b in sr.BATCHES[name]["big"] + sr.BATCHES[name]["small"]]:
        qkv, ref, tol, _ = _chain(name, lengths)
        cu = sr.offsets(lengths)
        for label, mut in sr.MUTANTS["attention"].items():
            hit = [b for b, L in enumerate(lengths) if mut["needs"](L, b == len(lengths) - 1, bias is not None)]
            if not hit:
                continue
            ratio = np.abs(mut["f"](qkv, cu, m["heads"], m["hidden"] // m["heads"], bias) - ref) / tol
            per_seq = [ratio[int(cu[b]):int(cu[b + 1])].max() for b in hit]
            assert min(per_seq) > 1.0, (label, lengths, [lengths[b] for b, r in zip(hit, per_seq) if r <= 1.0])
            assert max(per_seq) > 4.0, (label, lengths, max(per_seq))
            untouched = [b for b in range(len(lengths)) if b not in hit]
            assert all(ratio[int(cu[b]):int(cu[b + 1])].max() == 0.0 for b in untouched), label


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_every_qkv_mutant_exceeds_the_bound(name):
    for lengths in _all_batches(name):
        p = sr.reference_qkv(name, lengths)
        assert np.isfinite(p["tol"]).all() and (p["tol"] > 0).all()
        for label, mut in sr.MUTANTS["qkv"].items():
            if sum(lengths) < mut["needs"]:
                continue
            ratio = np.abs(mut["f"](p) - p["y"]) / p["tol"]
            assert ratio.max() > 4.0, (label, lengths, ratio.max())


def test_the_bound_is_of_the_order_of_one_bf16_rounding():
    """Nothing in the derived bounds is slack enough to hide a wrong operand: on the fast-pass inputs the attention
    bound stays below 4 bf16 roundings of the row's |v| average, the QKV bound below 4 roundings of |y| plus the fp32
    accumulation term."""
    name, lengths = "mpnet768", tuple(sr.BATCHES["mpnet768"]["small"][0])
    m = sr.MODELS[name]
    qkv, ref, tol, _ = _chain(name, lengths)
    vmax = np.abs(qkv[:, 2 * m["hidden"]:]).max()
    assert tol.max() <= 4 * sr.U_BF16 * vmax
    p = sr.reference_qkv(name, lengths)
    acc = (m["hidden"] + 2) * sr.U_F32 * (np.abs(p["A"]) @ np.abs(p["W"]).T + np.abs(p["bias"])) * p["sc"]
    assert (p["tol"] <= 4 * sr.U_BF16 * np.abs(p["y"]) + 4 * acc).mean() > 0.999
    # ambiguous LayerNorm outputs: 2 err / ulp with err ~ 40 fp32 roundings and ulp >= 2^-8 |o| -- a few per row of 768
    assert p["n_ambiguous"] < 5e-3 * p["A"].size
