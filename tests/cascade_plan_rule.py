"""The rules of the candidate cascade (csrc/css_knn_plan.h), restated in Python for the tests that check the header
(test_cascade_plan_host.py) and the launches it leads to (test_cascade_launches_gpu.py)."""
import numpy as np

BATCH, SWEEP_VALU, SWEEP_MFMA = 0, 1, 2
TILE_ROWS = 256       # CZ_T: rows of a tile
FUSED_MAX_STAGES = 16  # CZ_FS_MAXST


def growth(kind, i8, k, nrows, env_growth=0, env_growth_sweep=0):
    if kind == BATCH:
        return env_growth or (8 if k <= 32 and not i8 else 4)
    return env_growth_sweep or (8 if kind == SWEEP_MFMA and k <= 32 and nrows < 4_000_000 else 4)


def eps_rel(kind, i8, dpad):
    """float32 arithmetic in the header's order"""
    f = np.float32
    acc = f(2.0 ** -11)
    if not i8:
        return (f(2.0 ** -8) if kind == SWEEP_VALU else f(2.0 ** -7)) + acc
    r = np.sqrt(f(dpad)) / f(254.0)
    return (r if kind == SWEEP_VALU else f(2.0) * r + r * r) + acc


def fills_stage0(kind):
    return kind != SWEEP_VALU


def splits_last(kind, i8):
    return bool(i8) and kind != SWEEP_VALU


def plan(ntiles, g, fill_stage0, split_last):
    """[(stride, ratio, count)]: stage 0 reads every tile at its stride, a later stage those at a stride `ratio` times
    smaller that no stage before it read"""
    s0 = 1
    while ntiles // (s0 * g) >= 2:
        s0 *= g
    if fill_stage0 and s0 >= g and -(-ntiles // (s0 // g)) <= 15:
        s0 //= g
    w0 = -(-ntiles // s0)
    g0 = (w0 + 14) // 15
    stages = [(s0 * g0, 0)] if g0 > 1 else []
    stages.append((s0, g0))
    s = s0 // g
    while s >= 1:
        stages.append((s, g))
        s //= g
    if split_last and g == 4 and len(stages) >= 2 and stages[-1][0] == 1 and ntiles >= 64:
        stages[-1:] = [(2, 2), (1, 2)]
    out = []
    for si, (stride, ratio) in enumerate(stages):
        w = -(-ntiles // stride)
        out.append((stride, ratio, w if si == 0 else (w - 1) - (w - 1) // ratio))
    return out


def tickets(stages, g):
    """(first, stride, gm1) of the one-launch sweep: quarter tiles in stage order"""
    first = [0]
    for _, _, count in stages:
        first.append(first[-1] + 4 * count)
    gm1 = [max(1, (g if si == 0 else ratio) - 1) for si, (_, ratio, _) in enumerate(stages)]
    return first, [s for s, _, _ in stages], gm1


def plan_for(kind, i8, k, nrows):
    """the plan of one search under the default environment, and its growth"""
    g = growth(kind, i8, k, nrows)
    return plan(-(-nrows // TILE_ROWS), g, fills_stage0(kind), splits_last(kind, i8)), g
