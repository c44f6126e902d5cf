"""TEST SUPPORT, NOT PRODUCT CODE -- plain PyTorch fp32 late-interaction scorer (ColBERT).

What a colbert-ir checkpoint computes for one side: transformers' ``BertModel`` (``bert_reference.encode_tokens``), one
bias-free ``torch.nn.Linear(H, P)`` over every token, L2 normalisation per token; the score of a (query, doc) pair is
``sum_s max_{t kept} q_s . d_t``.  Weights come from seeds through ``claude_semantic_search_amd.synth``: the body is
``bert_reference.synth_weights``, the projection takes tensor id 10 (N(0, 0.05^2)), bit for bit what
``late_interaction.synth_projection`` builds.  ``tests/golden/make_li_goldens.py`` checks this restatement against
``transformers.BertModel`` + ``torch.nn.Linear``; ``tests/test_late_interaction_host.py`` pins it to the goldens.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bert_reference as br  # noqa: E402

PROJ_ID, PROJ_STD = 10, 0.05
GEOS = {"small": br.SMALL, "base": br.BASE}
#: projection width per geometry (answerai-colbert-small: 384 -> 96; colbertv2.0: 768 -> 128)
WIDTH = {"small": 96, "base": 128}


def synth_weights(cfg: br.BertCfg, seed: int, P: Optional[int]) -> Dict[str, torch.Tensor]:
    """``bert_reference.synth_weights`` plus ``linear.weight`` [P, H] (``P`` None: no projection)."""
    w = br.synth_weights(cfg, seed)
    if P:
        w["linear.weight"] = br._t(seed, PROJ_ID, (P, cfg.hidden), 0.0, PROJ_STD)
    return w


def token_vectors(w: Dict[str, torch.Tensor], cfg: br.BertCfg, ids: Sequence[int], normalize: bool = True) -> np.ndarray:
    """[L, P] float32 token vectors of ONE sequence."""
    with torch.no_grad():
        v = br.encode_tokens(w, cfg, ids)
        if "linear.weight" in w:
            v = v @ w["linear.weight"].T
        if normalize:
            v = F.normalize(v, p=2, dim=1, eps=1e-12)
        return v.numpy().astype(np.float32)


def score(q: np.ndarray, d: np.ndarray, keep=None) -> float:
    """MaxSim of float32 matrices in PyTorch fp32."""
    sim = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)) @ torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).T
    if keep is not None:
        sim = sim[:, torch.from_numpy(np.asarray(keep).reshape(-1) != 0)]
    return float(sim.max(dim=1).values.sum())


def scores(q_mats: List[np.ndarray], d_mats: List[np.ndarray], pairs, keep=None) -> np.ndarray:
    return np.array([score(q_mats[i], d_mats[j], None if keep is None else keep[j]) for i, j in pairs], dtype=np.float32)


def cosine_gap(got: np.ndarray, ref: np.ndarray) -> float:
    """Largest ``1 - cos`` between corresponding rows (float64)."""
    a, b = got.astype(np.float64), ref.astype(np.float64)
    cos = (a * b).sum(1) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)
    return float((1.0 - cos).max())


# ---- the cases of tests/test_late_interaction_gpu.py -----------------------------------------------------------------------
#: weight seeds per geometry, chosen so that the ranking check of RANK_CASE binds at least half of its adjacent pairs
#: in both compute modes (test_late_interaction_host.py::test_ranking_check_binds counts them)
WSEEDS = {"small": 157, "base": 8}
BSEED = 11
QSEED = 23
QUERY_LENS = [4, 17, 32]
#: test 4: document batches, each under 1024 tokens (lengths 1, 16, 17 and values that are no multiple of 16)
CASES = [[5], [1, 16, 17, 31], [128, 6, 64, 33], [383, 384, 5, 255]]
#: test 5: a batch of >= 1024 tokens (the LayerNorm-folded path at hidden 768, the wide GEMM tiles at hidden 384)
BIG_CASE = [384, 383, 255, 128, 31, 7, 5, 4, 200, 100]
#: the ranking check: the 32-token query against documents of these lengths (a MaxSim score grows with the number of
#: doc tokens to choose from until it saturates near 40 tokens of these random models, so short lengths in a rough
#: geometric progression keep the reference scores apart)
RANK_CASE = [2, 3, 4, 5, 6, 8, 10, 12, 15, 18, 22, 27, 33, 40]


def queries(cfg: br.BertCfg) -> List[List[int]]:
    return br.synth_batch(cfg, QUERY_LENS, QSEED)


# ---- bars ----------------------------------------------------------------------------------------------------------------
def fp32_token_eps(w: Dict[str, torch.Tensor], cfg: br.BertCfg, vmin: float) -> float:
    """Bound on ``||u - u_ref||_2`` of a unit token vector in fp32 mode: the project's 1e-4 bar on every component of a
    hidden state (``||dh||_2 <= 1e-4 sqrt(H)``) through the projection (``||dv||_2 <= sigma_max(W) ||dh||_2``; without
    one W = I), the normalisation (``||v / ||v|| - v' / ||v'|| ||_2 <= 2 ||dv||_2 / ||v||_2``, with ``vmin`` the
    smallest reference ``||v||_2`` of the case) and the one rounding to bf16 (relative 2^-9 per component, so 2^-9 in
    the norm of a unit vector)."""
    smax = float(np.linalg.norm(w["linear.weight"].numpy().astype(np.float64), 2)) if "linear.weight" in w else 1.0
    return 2.0 * smax * 1e-4 * np.sqrt(cfg.hidden) / vmin + 2.0 ** -9


def fp32_cos_bar(eps: float) -> float:
    """``1 - cos`` of two vectors, one of them a unit vector, at distance <= eps: 1 - cos <= eps^2 / 2 for unit vectors
    (``||a - b||^2 = 2 (1 - cos)``); the bf16 row is a unit vector only to 2^-9, which the eps already counts, so the
    bar is eps^2 (twice the unit-vector figure)."""
    return eps * eps


def fp32_score_bar(eps_q: float, eps_d: float, m: int, P: int) -> float:
    """A dot of two unit vectors moves by at most eps_q + eps_d + eps_q eps_d, a maximum by no more than its largest
    argument does, and the score adds m of them; plus the kernel's own fp32 rounding 2^-23 m (P + m) (c <= 1.01)."""
    return m * (eps_q + eps_d + eps_q * eps_d) + 2.0 ** -23 * m * (P + m) * 1.01


#: bf16 mode.  The propagated hidden-state bar of that mode (2e-2 per component) is far larger than the quantities, so
#: these bars are MEASURED on the device against this fp32 reference over the cases of GPU tests 4, 5 and 8
#: (test_late_interaction_gpu.py prints every figure; DESIGN.md 3.3d lists them per test) and then doubled: the margin
#: is for other batch compositions (another GEMM tile walk moves bf16 noise).  One pair of bars per model depth: the
#: 2-layer models of tests 4 and 5 take twice the larger of their own two figures, the 6-layer model of test 8 twice
#: its own, so the deeper model's noise does not loosen the bars of the shallow ones.
BF16_COS_MEASURED = {"test4": 1.612e-5, "test5": 1.766e-5, "test8": 4.146e-5}
BF16_SCORE_MEASURED = {"test4": 9.335e-3, "test5": 9.966e-3, "test8": 1.017e-2}
BF16_COS_BAR = 2 * max(BF16_COS_MEASURED["test4"], BF16_COS_MEASURED["test5"])
BF16_SCORE_BAR = 2 * max(BF16_SCORE_MEASURED["test4"], BF16_SCORE_MEASURED["test5"])
BF16_COS_BAR_6LAYER = 2 * BF16_COS_MEASURED["test8"]
BF16_SCORE_BAR_6LAYER = 2 * BF16_SCORE_MEASURED["test8"]


def binding_pairs(ref_scores: np.ndarray, bar: float):
    """Adjacent pairs (in the reference's order, best first) whose reference scores differ by more than twice the bar:
    ``(order, mask)``; the device's order must agree on every such pair."""
    order = np.argsort(-ref_scores.astype(np.float64), kind="stable")
    gaps = -np.diff(ref_scores.astype(np.float64)[order])
    return order, gaps > 2 * bar
