"""Every kind of candidate cascade launches what its plan says (csrc/css_knn_plan.h, restated in cascade_plan_rule.py):
the per-name launch counts of the library's own timing scopes, under the default environment, and the results of the
same calls against the CPU oracle."""
import numpy as np
import pytest

import cascade_plan_rule as rule
from claude_semantic_search_amd import synth
from knn_checks import assert_topk_matches

D = 128
SCOPES = ("knn_coarse_cascade", "knn_scan_coarse_stage", "knn_scan_coarse_main", "knn_sweep_cascade", "knn_sweep_fused",
          "knn_sweep_coarse_stage", "knn_sweep_coarse_main", "knn_sweep_mfma_stage", "knn_sweep_mfma_main")
STAGE_SCOPES = {rule.BATCH: "knn_scan_coarse", rule.SWEEP_VALU: "knn_sweep_coarse", rule.SWEEP_MFMA: "knn_sweep_mfma"}


def _expected(kind, i8, k, n, fused):
    want = dict.fromkeys(SCOPES, 0)
    want["knn_coarse_cascade" if kind == rule.BATCH else "knn_sweep_cascade"] = 1
    if fused:
        want["knn_sweep_fused"] = 1
        return want
    stages, _ = rule.plan_for(kind, i8, k, n)
    # the main stage: stride 1 behind a stage 0; every other stage with tiles counts as "stage"
    main = [si > 0 and stride == 1 for si, (stride, _, _) in enumerate(stages)]
    want[STAGE_SCOPES[kind] + "_main"] = sum(1 for m, (_, _, count) in zip(main, stages) if m and count > 0)
    want[STAGE_SCOPES[kind] + "_stage"] = sum(1 for m, (_, _, count) in zip(main, stages) if not m and count > 0)
    return want


# (n, nq, k, search mode, kind with int8 rows, kind without, one launch): with 128 columns a batch never reads the int8 rows
# (they serve rows of 256 / 512 / 768 / 1024 columns there), a sweep does where the index has them
CASES = {
    "a_batch_17_tiles": (4_097, 17, 10, "coarse", rule.BATCH, rule.BATCH, False),       # the smallest batch with two stages
    "b_batch_ragged_k100": (20_001, 17, 100, None, rule.BATCH, rule.BATCH, False),      # a ragged last tile, growth 4
    "c_one_query_one_launch": (100_000, 1, 10, None, rule.SWEEP_VALU, rule.SWEEP_VALU, True),
    "d_two_queries_per_stage": (100_000, 2, 10, None, rule.SWEEP_VALU, rule.SWEEP_VALU, False),
    "e_eight_queries_int8_mfma": (50_000, 8, 10, None, rule.SWEEP_MFMA, rule.BATCH, False),   # growth 8
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_cascade_launches_follow_the_plan(case):
    from oracle import knn_oracle as ko
    from claude_semantic_search_amd import _native as nat
    from claude_semantic_search_amd.flat_index import IndexFlatIP

    n, nq, k, mode, kind_i8, kind_bf16, fused = CASES[case]
    x = ko.normalize_rows(synth.rows(n, D, 51))
    q = synth.rows(nq, D, 52 + nq)
    ix = IndexFlatIP(D)
    ix.add(x)
    if mode:
        ix.set_search_mode(mode)
    has_i8 = bool(ix.shadow_info()["int8"])
    kind = kind_i8 if has_i8 else kind_bf16
    i8 = has_i8 and kind != rule.BATCH
    nat.prof_reset()
    nat.prof_enable(True)
    Dg, Ig = ix.search(q, k, normalize=True)
    nat.prof_enable(False)
    got = {name: nat.prof_read(name)[1] for name in SCOPES}
    nat.prof_reset()
    ix.close()
    print(case, "int8 rows" if has_i8 else "bf16 rows only", rule.plan_for(kind, i8, k, n), got)
    assert got == _expected(kind, i8, k, n, fused)
    ref = ko.FlatIndexOracle(D, 0)
    ref.add(x)
    qr = ko.normalize_rows(q)
    Dr, Ir = ref.search(qr, k)
    assert_topk_matches(Dg, Ig, Dr, Ir, ref.rescore64(qr, Ir), case)
