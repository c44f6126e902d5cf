"""TEST SUPPORT, NOT PRODUCT CODE -- plain PyTorch fp32 learned sparse encoder (SPLADE).

What a ``BertForMaskedLM`` SPLADE checkpoint computes for one text: transformers' ``BertModel``
(``bert_reference.encode_tokens``), the masked-LM head (dense + exact erf GELU + LayerNorm, then the decoder with its
bias) over every token, and ``w[v] = max_t log(1 + relu(logit[t, v]))``.  Weights come from seeds through
``claude_semantic_search_amd.synth``: the body is ``bert_reference.synth_weights``, the head takes tensor ids 11-15, bit
for bit what ``sparse_encoder.synth_mlm_head`` builds, with the decoder tied to the word embeddings.
``tests/golden/make_splade_goldens.py`` checks this restatement against ``transformers.BertForMaskedLM``;
``tests/test_sparse_host.py`` pins it to the goldens.
"""
from __future__ import annotations

import math
import sys
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bert_reference as br  # noqa: E402

from claude_semantic_search_amd import sparse_encoder as se  # noqa: E402

GEOS = {"small": br.SMALL, "base": br.BASE}
P = "cls.predictions."


def synth_head(cfg: br.BertCfg, seed: int, bias_sigmas: float = se.SYNTH_BIAS_SIGMAS) -> Dict[str, torch.Tensor]:
    """The head tensors under their ``BertForMaskedLM`` names (no ``decoder.weight``: tied)."""
    h = se.synth_mlm_head(cfg.hidden, cfg.vocab, seed, bias_sigmas)
    return {P + "transform.dense.weight": torch.from_numpy(h["dense_w"]), P + "transform.dense.bias": torch.from_numpy(h["dense_b"]),
            P + "transform.LayerNorm.weight": torch.from_numpy(h["ln_g"]), P + "transform.LayerNorm.bias": torch.from_numpy(h["ln_b"]),
            P + "bias": torch.from_numpy(h["decoder_b"])}


def synth_weights(cfg: br.BertCfg, seed: int, bias_sigmas: float = se.SYNTH_BIAS_SIGMAS) -> Dict[str, torch.Tensor]:
    """``bert_reference.synth_weights`` plus the head (``synth_head``)."""
    w = br.synth_weights(cfg, seed)
    w.update(synth_head(cfg, seed, bias_sigmas))
    return w


def decoder(w: Dict[str, torch.Tensor]) -> torch.Tensor:
    return w.get(P + "decoder.weight", w["embeddings.word_embeddings.weight"])


def head_rows(w: Dict[str, torch.Tensor], cfg: br.BertCfg, hs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(g, u)`` [L, H] of the hidden states ``hs``: u = gelu(Wd h + bd), g = LayerNorm(u)."""
    u = F.gelu(hs @ w[P + "transform.dense.weight"].T + w[P + "transform.dense.bias"])
    g = F.layer_norm(u, (cfg.hidden,), w[P + "transform.LayerNorm.weight"], w[P + "transform.LayerNorm.bias"], cfg.ln_eps)
    return g, u


def sparse(w: Dict[str, torch.Tensor], cfg: br.BertCfg, ids: Sequence[int]) -> Dict[str, np.ndarray]:
    """ONE sequence: ``z`` [V] (max_t relu(logit)), ``logit_max`` [V] (max_t logit, sign kept), ``w`` [V] =
    float32(log1p(float64 z)), ``g`` [L, H] and ``umin``, the smallest per-token standard deviation of u."""
    with torch.no_grad():
        g, u = head_rows(w, cfg, br.encode_tokens(w, cfg, ids))
        lmax = (g @ decoder(w).T + w[P + "bias"]).max(dim=0).values.numpy().astype(np.float32)
        umin = float(u.double().std(dim=1, unbiased=False).min())
    z = np.maximum(lmax, np.float32(0))
    return {"z": z, "logit_max": lmax, "w": np.log1p(z.astype(np.float64)).astype(np.float32), "g": g.numpy(), "umin": umin}


def topm(z: np.ndarray, m: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """``(terms int32 [m], weights float32 [m], nnz)`` of one row of z: the m largest z > 0, best first, ties to the
    lower term id, padded with -1 / 0."""
    z = np.asarray(z, dtype=np.float32)
    order = np.lexsort((np.arange(z.size), -z.astype(np.float64)))
    nnz = int((z > 0).sum())
    k = min(m, nnz)
    terms = np.full(m, -1, dtype=np.int32)
    weights = np.zeros(m, dtype=np.float32)
    terms[:k] = order[:k]
    weights[:k] = np.log1p(z[order[:k]].astype(np.float64)).astype(np.float32)
    return terms, weights, nnz


def vector(z: np.ndarray, m: int) -> "se.SparseVector":
    t, wt, nnz = topm(z, m)
    k = min(m, nnz)
    return se.SparseVector(t[:k], wt[:k])


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------
#: weight seeds per geometry
WSEEDS = {"small": 157, "base": 8}
BSEED = 11
M = 256
#: document batches, each under 1024 tokens (lengths 1, 16, 17 and values that are no multiple of 16)
CASES = [[5], [1, 16, 17, 31], [128, 6, 64, 33], [383, 384, 5, 255]]
#: a batch of >= 1024 tokens (the LayerNorm-folded path at hidden 768, the wide GEMM tiles at hidden 384)
BIG_CASE = [384, 383, 255, 128, 31, 7, 5, 4, 200, 100]


# ---- bars ----------------------------------------------------------------------------------------------------------------
def fp32_z_bar(w: Dict[str, torch.Tensor], cfg: br.BertCfg, umin: float) -> float:
    """Bound on ``|z - z_ref|`` in fp32 mode, to first order: the project's 1e-4 bar on every component of a hidden
    state (``||dh||_2 <= 1e-4 sqrt(H)``) through the dense layer (``sigma_max(Wd)``), the GELU (slope at most 1.13), the
    LayerNorm (``||dg||_2 <= max|gamma| ||du||_2 / std(u)``, with ``umin`` the smallest per-token std of the case) and
    the decoder row (``|dz| <= max_v ||E_v||_2 ||dg||_2``); plus the fp32 accumulation of the decoder's dot product,
    2^-23 H max_v ||E_v||_2 ||g||_2 / sqrt(H) (c <= 1.5; ||g||_2 <= sqrt(H) (max|gamma| + max|beta|))."""
    H = cfg.hidden
    Wd = w[P + "transform.dense.weight"].numpy().astype(np.float64)
    gam = float(w[P + "transform.LayerNorm.weight"].abs().max())
    bet = float(w[P + "transform.LayerNorm.bias"].abs().max())
    emax = float(decoder(w).double().norm(dim=1).max())
    prop = emax * gam * 1.13 * float(np.linalg.norm(Wd, 2)) * 1e-4 * math.sqrt(H) / umin
    acc = 1.5 * 2.0 ** -23 * math.sqrt(H) * emax * math.sqrt(H) * (gam + bet)
    return prop + acc


def fp32_rows_bar(w: Dict[str, torch.Tensor], cfg: br.BertCfg, hs: np.ndarray, umin: float) -> float:
    """Bound on ``|g - g64|`` per component, g64 formed in float64 from the SAME hidden states: one fp32 GEMM of depth H
    (``|du| <= 1.5 * 2^-23 sum_k |Wd_k h_k| <= 1.5 * 2^-23 max_j ||Wd_j||_2 max_t ||h_t||_2 sqrt(H)`` by Cauchy-Schwarz
    on |.|, times the GELU slope 1.13 and its own few-ulp error on |u| <= umax), then the LayerNorm: every component of
    du moves g by at most max|gamma| |du| / std(u) directly and as much again through mean and variance, plus the
    LayerNorm's own fp32 arithmetic, 8 ulp of max|g|."""
    H = cfg.hidden
    Wd = w[P + "transform.dense.weight"].numpy().astype(np.float64)
    gam = float(w[P + "transform.LayerNorm.weight"].abs().max())
    bet = float(w[P + "transform.LayerNorm.bias"].abs().max())
    hmax = float(np.linalg.norm(hs.astype(np.float64), axis=1).max())
    wmax = float(np.linalg.norm(Wd, axis=1).max())
    du = 1.5 * 2.0 ** -23 * wmax * hmax * math.sqrt(H) * 1.13 + 4 * 2.0 ** -23 * wmax * hmax
    gmax = gam * math.sqrt(H) + bet      # |g_c| <= gamma |u_c - mean| / std + beta, and |u_c - mean| / std <= sqrt(H)
    return 2 * gam * du / umin + 8 * 2.0 ** -23 * gmax


def rows64(w: Dict[str, torch.Tensor], cfg: br.BertCfg, hs: np.ndarray) -> np.ndarray:
    """g in float64 from hidden states ``hs`` [T, H]."""
    h = torch.from_numpy(np.asarray(hs, dtype=np.float64))
    u = F.gelu(h @ w[P + "transform.dense.weight"].double().T + w[P + "transform.dense.bias"].double())
    return F.layer_norm(u, (cfg.hidden,), w[P + "transform.LayerNorm.weight"].double(),
                        w[P + "transform.LayerNorm.bias"].double(), cfg.ln_eps).numpy()


def binding_pairs(ref_scores: np.ndarray, bars) -> Tuple[np.ndarray, np.ndarray]:
    """Adjacent pairs (in the reference's order, best first) whose reference scores differ by more than twice the bar
    (``bars``: one per document, or one for all; a pair takes the larger of its two): ``(order, mask)``; the device's
    order must agree on every such pair."""
    order = np.argsort(-ref_scores.astype(np.float64), kind="stable")
    gaps = -np.diff(ref_scores.astype(np.float64)[order])
    b = np.broadcast_to(np.asarray(bars, dtype=np.float64), ref_scores.shape)[order]
    return order, gaps > 2 * np.maximum(b[:-1], b[1:])


def score_bar(rq: Dict[str, np.ndarray], rd: Dict[str, np.ndarray], mq: int, md: int, zbar: float) -> float:
    """Bound on the change of a pair's score when every logit maximum moves by at most ``zbar``, from the reference's
    dense results ``rq`` / ``rd`` (``sparse``) alone.  log1p o relu is 1-Lipschitz, so a weight moves by at most zbar and
    a product w_q w_d by at most (w_q + w_d) zbar + zbar^2; only terms whose logit maximum exceeds -zbar on BOTH sides
    can contribute on either machine.  A term within 2 zbar of a side's cut weight (the weight of rank m, when more than
    m are positive) may enter or leave that side's list, which moves the score by its whole product at most."""
    wq, wd = rq["w"].astype(np.float64), rd["w"].astype(np.float64)
    live = (rq["logit_max"] > -zbar) & (rd["logit_max"] > -zbar)
    bar = float(((wq + wd) * zbar + zbar * zbar)[live].sum())
    flips = np.zeros(wq.size, bool)
    for wv, m in ((wq, mq), (wd, md)):
        if int((wv > 0).sum()) > m:
            cut = np.sort(wv)[::-1][m - 1:m + 1].mean()
            flips |= np.abs(wv - cut) <= 2 * zbar + abs(np.sort(wv)[::-1][m - 1] - cut)
    return bar + float(((wq + zbar) * (wd + zbar))[flips & live].sum())


#: bf16 mode.  The propagated hidden-state bar of that mode (2e-2 per component) is far larger than the quantities, so
#: the bars on |z - z_ref| are MEASURED on the device against this fp32 reference over the batches of the GPU tests
#: (the tests print every figure; DESIGN.md 3.3e lists them) and then doubled: the margin is for other batch
#: compositions (another GEMM tile walk moves bf16 noise).  One bar per model depth: the 2-layer models of
#: test_sparse_tokens_gpu.py take twice the largest of their figures (hidden 384: 6.864e-3, the big batch with
#: set_attention_range(0) 7.541e-3; hidden 768: 1.268e-2 and 1.189e-2), the 6-layer model of test_sparse_encoder_gpu.py
#: twice the larger of its two (tied decoder 8.933e-3, untied 6.823e-3).
BF16_Z_MEASURED = {"2layer": 1.268e-2, "6layer": 8.933e-3}


# ---- the end-to-end case (tests/test_sparse_encoder_gpu.py, counted on the CPU by tests/test_sparse_host.py) --------------
#: a 6-layer hidden-384 checkpoint over a vocabulary of 1082 words (no multiple of the kernel's 128-term tile).  The
#: ranking check compares the order only where reference scores differ by more than twice the score bar, and the bf16 z
#: bar is some 4 % of a logit's spread, so the case is built for scores that are far apart and weights that are large
#: against the bar:
#:  - the decoder bias keeps one term in E2E_LIVE_STEP live (E2E_LIVE_SIGMAS) and the rest dead (E2E_DEAD_SIGMAS, never
#:    positive), as a trained model's sparsity regulariser does: a live term's weight is several times the bar, and with
#:    at most 68 live terms the cuts at 64 / 256 play next to no part (the cut itself is the business of
#:    test_sparse_tokens_gpu.py);
#:  - the documents are the first E2E_KS words of the 32-word query: a token's logits depend mostly on the token and its
#:    position, so a document shares about as many of the query's large terms as it shares words, and the reference
#:    score grows by half or more from each document to the next.
#: tests/test_sparse_host.py::test_ranking_check_binds counts the pairs that this binds, per decoder and compute mode.
E2E_VOCAB = 1082
E2E_SEED = 31
E2E_LIVE_STEP, E2E_LIVE_SIGMAS, E2E_DEAD_SIGMAS = 16, -1.0, -6.0
E2E_WORDS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + [f"w{i}" for i in range(E2E_VOCAB - 4)]
E2E_QUERY = " ".join(f"w{(131 * i + 7) % (E2E_VOCAB - 4)}" for i in range(32))      # 32 distinct words
#: document lengths in words, about tripling: with doubling lengths the bf16 leg would bind a majority of its pairs only
#: just, and not at all at a z bar a fifth larger
E2E_KS = [1, 3, 9, 32]


def e2e_cfg() -> br.BertCfg:
    return br.BertCfg(num_layers=6, pooling="cls", normalize=False, vocab=E2E_VOCAB, **br.SMALL)


def e2e_weights(tied: bool) -> Dict[str, torch.Tensor]:
    """The checkpoint's tensors: ``synth_weights`` with every term dead, every E2E_LIVE_STEP-th term raised to the live
    bias, and for the untied decoder a matrix of its own, N(0, 0.02^2)."""
    cfg = e2e_cfg()
    w = synth_weights(cfg, E2E_SEED, E2E_DEAD_SIGMAS)
    b = w[P + "bias"].clone()
    b[::E2E_LIVE_STEP] += float((E2E_LIVE_SIGMAS - E2E_DEAD_SIGMAS) * 0.02 * math.sqrt(cfg.hidden))
    w[P + "bias"] = b
    if not tied:
        w[P + "decoder.weight"] = br._t(E2E_SEED, 40, (cfg.vocab, cfg.hidden), 0.0, 0.02)
    return w


def e2e_documents() -> List[str]:
    """The first E2E_KS words of the query (the last document is the query itself)."""
    words = E2E_QUERY.split()
    return [" ".join(words[:k]) for k in E2E_KS]


def e2e_z_bar(w: Dict[str, torch.Tensor], compute: str, refs: Sequence[Dict[str, np.ndarray]]) -> float:
    """The bar on |z - z_ref| of the end-to-end case: bf16 twice the measured 6-layer figure, fp32 ``fp32_z_bar``."""
    if compute == "bf16":
        return 2 * BF16_Z_MEASURED["6layer"]
    return fp32_z_bar(w, e2e_cfg(), min(r["umin"] for r in refs))


def e2e_ranking(rq: Dict[str, np.ndarray], rd: Sequence[Dict[str, np.ndarray]], zbar: float):
    """``(ref_scores float32 [n], score_bars [n], order, bound)`` of the query against the documents at the z bar
    ``zbar``, from the reference's results alone: what the GPU test asserts and what the host test counts."""
    ref = np.array([se.sparse_dot_numpy(vector(rq["z"], 64), vector(r["z"], 256)) for r in rd], np.float32)
    bars = np.array([score_bar(rq, r, 64, 256, zbar) for r in rd])
    order, bound = binding_pairs(ref, bars)
    return ref, bars, order, bound


def e2e_ids(text: str) -> List[int]:
    """[CLS] words [SEP] with the ids of E2E_WORDS (what the WordPiece tokenizer gives for these texts)."""
    return [2] + [4 + int(t[1:]) for t in text.split()] + [3]
