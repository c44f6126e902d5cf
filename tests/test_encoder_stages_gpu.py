"""bf16 attention and QKV GEMMs of the encoder against float64, PER ELEMENT (tests/encoder_stage_reference.py).

A one-layer model is run through the ordinary forward entry point; ``debug_read("qkv")`` / ``("ctx")`` give the layer's
QKV projection and attention output as the device stored them (blocked on the LayerNorm-folded path of >= 1024
tokens).  ctx is held against ``attention64`` of the device's OWN qkv, qkv against ``qkv64`` of the token ids, each
within a bound derived from the kernels' rounding points -- no fitted factor.  tests/test_encoder_stages_host.py shows
on the CPU that the one-line kernel mistakes these tests exist for (``MUTANTS``) exceed these bounds on these inputs.

Kernel instantiations: k_attention_bf16<64, false, true> / <64, true, true> (MPNet, row-major / blocked),
<64, false, false> / <64, true, false> (BERT 768), <32, false, false> (BERT 384); k_gemm_skinny<.., 1> / <.., 2>
(<= 32 / <= 64 tokens; UNR 6 at hidden 384), the 128 x 128 k_gemm, k_gemm8p<EPI_AFF_QKV>.
Each case prints its worst err / tol (pytest -s)."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder

sys.path.insert(0, str(Path(__file__).resolve().parent))
import encoder_stage_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

#: kernel instantiation -> (model, the batches that reach it)
ATTENTION = {
    "mpnet768 row-major <64,false,true>": ("mpnet768", ("small", "skinny1", "skinny2")),
    "mpnet768 blocked <64,true,true>": ("mpnet768", ("big",)),
    "bert768 row-major <64,false,false>": ("bert768", ("small", "skinny1", "skinny2")),
    "bert768 blocked <64,true,false>": ("bert768", ("big",)),
    "bert384 row-major <32,false,false>": ("bert384", ("small", "skinny1", "skinny2")),
}
#: GEMM regime -> batches; at hidden 768 `big` is k_gemm8p<EPI_AFF_QKV> (folded path), at 384 the 128 x 128 k_gemm again
GEMM_REGIMES = ("big", "small", "skinny1", "skinny2")


def _batches(name, part):
    return [tuple(b) for b in (sr.SKINNY[part] if part in sr.SKINNY else sr.BATCHES[name][part])]


@functools.lru_cache(maxsize=None)
def _encoder(name, kind="fast"):
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides=sr.model_cfg(name))
    enc.load_state_dict(sr.model_weights(name, kind))
    return enc


def _forward(enc, name, lengths):
    """One forward of the batch; (qkv [T, 3 H], ctx [T, H]) as the device stored them, row-major."""
    H, T = sr.MODELS[name]["hidden"], sum(lengths)
    out = enc.encode_ids(sr.batch_ids(name, lengths))
    assert np.isfinite(out).all()
    if sr.path_is_folded(name, lengths):
        qkv = sr.deblock(enc.debug_read("qkv", (sr.blocked_numel(T, 3 * H),)), T, 3 * H)
        ctx = sr.deblock(enc.debug_read("ctx", (sr.blocked_numel(T, H),)), T, H)
    else:
        qkv = enc.debug_read("qkv", (T, 3 * H))
        ctx = enc.debug_read("ctx", (T, H))
    return qkv.astype(np.float64), ctx.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _run(name, lengths, forced):
    """(qkv, ctx) of the fast-weights model; forced: set_attention_range(0), the running-maximum pass."""
    enc = _encoder(name)
    enc.set_attention_range(0.0 if forced else 2.0 ** 100)
    try:
        return _forward(enc, name, lengths)
    finally:
        enc.set_attention_range(2.0 ** 100)


@functools.lru_cache(maxsize=None)
def _attention_reference(name, lengths, safe):
    """attention64 of the device's own qkv (the two passes read the same qkv bits: checked by the caller)."""
    m = sr.MODELS[name]
    qkv = _run(name, lengths, False)[0]
    return sr.attention64(qkv, sr.offsets(lengths), m["heads"], m["hidden"] // m["heads"], sr.model_bias_table(name), safe=safe)


def _worst(err, tol):
    assert np.isfinite(err).all() and np.isfinite(tol).all()
    ratio = err / tol
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[i]), i


@pytest.mark.parametrize("forced", [False, True], ids=["default-range", "range-0"])
@pytest.mark.parametrize("inst", list(ATTENTION))
def test_attention_meets_its_bound_per_element(inst, forced):
    name, parts = ATTENTION[inst]
    m = sr.MODELS[name]
    worst = 0.0
    for part in parts:
        for lengths in _batches(name, part):
            qkv, ctx = _run(name, lengths, forced)
            assert np.array_equal(qkv, _run(name, lengths, False)[0])          # same GEMM, same bits: one reference
            ref, tol, log2sum = _attention_reference(name, lengths, forced)
            # the default setting really stays on the reference-free pass: every row sum far inside 2^+-100
            assert np.abs(log2sum).max() < 60, np.abs(log2sum).max()
            r, at = _worst(np.abs(ctx - ref), tol)
            worst = max(worst, r)
            assert r <= 1.0, f"{inst} {lengths}: |ctx - ref| = {r:.2f} tol at (token, column) {at}"
            if forced:     # the two passes agree within the sum of their bounds (<= 2 x the larger)
                fast = _run(name, lengths, False)[1]
                r2, at2 = _worst(np.abs(ctx - fast), tol + _attention_reference(name, lengths, False)[1])
                assert r2 <= 1.0, f"{inst} {lengths}: passes differ by {r2:.2f} of their bounds at {at2}"
            else:          # edge coverage on the device's own qkv
                bad = sr.edge_coverage(qkv, sr.offsets(lengths), m["heads"], m["hidden"] // m["heads"], sr.model_bias_table(name))
                assert not bad, bad
    print(f"\nSTAGE attention {inst} {'range 0' if forced else 'default'}: worst err / tol = {worst:.3f}")


@pytest.mark.parametrize("inst", list(ATTENTION))
def test_attention_falls_back_by_itself_and_still_meets_the_bound(inst):
    """Logits in the hundreds: exp2(score) leaves fp32, the DEFAULT range has to repeat such blocks with the
    running-maximum pass.  ctx still meets the bound computed from the device's qkv."""
    name, parts = ATTENTION[inst]
    m = sr.MODELS[name]
    lengths = _batches(name, parts[0])[0]
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides=sr.model_cfg(name))
    try:
        enc.load_state_dict(sr.model_weights(name, "fallback"))
        qkv, ctx = _forward(enc, name, lengths)
    finally:
        enc.close()
    ref, tol, log2sum = sr.attention64(qkv, sr.offsets(lengths), m["heads"], m["hidden"] // m["heads"],
                                       sr.model_bias_table(name, "fallback"), safe=True)
    assert np.abs(log2sum).max() > 100, "no row sum outside the fast pass's window: the fallback did not run"
    r, at = _worst(np.abs(ctx - ref), tol)
    print(f"\nSTAGE fallback {inst}: worst err / tol = {r:.3f}, |log2 row sum| up to {np.abs(log2sum).max():.0f}")
    assert r <= 1.0, f"{inst} {lengths}: |ctx - ref| = {r:.2f} tol at {at}"


@pytest.mark.parametrize("part", GEMM_REGIMES)
@pytest.mark.parametrize("name", list(sr.MODELS))
def test_qkv_projection_meets_its_bound_per_element(name, part):
    worst, n_amb = 0.0, 0
    for lengths in _batches(name, part):
        qkv = _run(name, lengths, False)[0]
        p = sr.reference_qkv(name, lengths)
        r, at = _worst(np.abs(qkv - p["y"]), p["tol"])
        worst, n_amb = max(worst, r), n_amb + p["n_ambiguous"]
        assert r <= 1.0, f"{name} {part} {lengths}: |qkv - y| = {r:.2f} tol at (token, column) {at}"
    path = "folded" if sr.path_is_folded(name, _batches(name, part)[0]) else "row-major"
    print(f"\nSTAGE qkv {name} {part} ({path}): worst err / tol = {worst:.3f}, ambiguous operands = {n_amb}")


@pytest.mark.parametrize("name", ["mpnet768", "bert768"])
def test_the_same_sequences_meet_their_bounds_on_both_paths(name):
    """Every sequence goes through the folded batch (blocked qkv / ctx) and through a small batch (row-major); each
    ctx row is held to ITS OWN bound, from the qkv of its own path -- there is no cross-path tolerance."""
    seen = {}
    for part in ("big", "small"):
        for lengths in _batches(name, part):
            ctx = _run(name, lengths, False)[1]
            ref, tol, _ = _attention_reference(name, lengths, False)
            cu = sr.offsets(lengths)
            for b, L in enumerate(lengths):
                rows = slice(int(cu[b]), int(cu[b + 1]))
                assert (np.abs(ctx[rows] - ref[rows]) <= tol[rows]).all(), (name, part, L)
                seen.setdefault(L, {})[part] = ctx[rows]
    assert all(set(v) == {"big", "small"} for v in seen.values()) and len(seen) >= 13
    gap = max(np.abs(v["big"] - v["small"]).max() for v in seen.values())
    print(f"\nSTAGE two paths {name}: largest |ctx folded - ctx row-major| = {gap:.4f} (reported, not asserted)")
