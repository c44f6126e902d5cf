"""The rules of the candidate cascade (csrc/css_knn_plan.h: schedule, growth, a-priori error bound, ticket table) need no
GPU: tests/native/cascade_plan.cc, a stand-alone program that includes nothing but that header, is built with the host
compiler and its answers are compared with the restatement of the rules in cascade_plan_rule.py."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cascade_plan_rule as rule

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "cascade_plan.cc"
INC = ROOT / "claude_semantic_search_amd" / "csrc"

NTILES = list(range(1, 3001)) + [3907, 4883, 39063, 65536, 312500, 2 ** 20]
GROWTHS = (4, 8, 16)


def _build(tmp, name, extra):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *extra, f"-I{INC}", str(SRC), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return out


def _ask(prog, lines):
    r = subprocess.run([str(prog)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _parse_plan(line):
    head, tail = line.split(" | tickets ")
    words = head.split()
    assert words[0] == "plan" and int(words[1]) == len(words) - 2
    stages = [tuple(int(v) for v in w.split(",")) for w in words[2:]]
    t = tail.split()
    if t[0] == "0":
        return stages, None
    n = len(stages)
    assert t[1] == "first" and t[n + 3] == "stride" and t[2 * n + 4] == "gm1" and len(t) == 3 * n + 5
    ints = lambda a, b: [int(v) for v in t[a:b]]
    return stages, (ints(2, n + 3), ints(n + 4, 2 * n + 4), ints(2 * n + 5, 3 * n + 5))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cascade_plan"), "cascade_plan", ["-O2"])


@pytest.fixture(scope="module")
def plans(prog):
    """every (ntiles, growth, fill_stage0, split_last) of the sweep -> (stages, tickets) as the header plans them"""
    keys = [(nt, g, fill, split) for nt in NTILES for g in GROWTHS for fill in (0, 1) for split in (0, 1)]
    out = _ask(prog, [f"plan {nt} {g} {fill} {split}" for nt, g, fill, split in keys])
    return dict(zip(keys, (_parse_plan(line) for line in out)))


def test_literal_plans(plans):
    assert plans[(16, 8, 1, 0)][0] == [(8, 1, 2), (1, 8, 14)]
    assert plans[(64, 4, 1, 1)][0] == [(16, 1, 4), (4, 4, 12), (2, 2, 16), (1, 2, 32)]
    assert plans[(79, 4, 0, 0)][0] == [(16, 1, 5), (4, 4, 15), (1, 4, 59)]
    assert plans[(391, 8, 1, 0)][0] == [(64, 1, 7), (8, 8, 42), (1, 8, 342)]
    assert plans[(3907, 4, 1, 1)][0] == [(1024, 1, 4), (256, 4, 12), (64, 4, 46), (16, 4, 183), (4, 4, 732), (2, 2, 977),
                                         (1, 2, 1953)]


def test_plans_and_tickets_match_the_rule(plans):
    for (nt, g, fill, split), (stages, tickets) in plans.items():
        want = rule.plan(nt, g, bool(fill), bool(split))
        assert stages == want, (nt, g, fill, split)
        # (at most 11 stages and 2^20 tiles here: the ticket table always holds the plan)
        assert tickets is not None and tuple(tickets) == rule.tickets(want, g), (nt, g, fill, split)


def test_every_tile_is_read_by_exactly_one_stage(plans):
    for (nt, g, fill, split), (stages, tickets) in plans.items():
        what = (nt, g, fill, split)
        seen = np.zeros(nt, dtype=np.int32)
        for si, (stride, ratio, count) in enumerate(stages):
            w = -(-nt // stride)
            j = np.arange(w, dtype=np.int64)
            if si > 0:
                j = j[j % ratio != 0]
            assert count == len(j) and count > 0, what          # no stage is empty, and count is what the stage reads
            assert (j * stride < nt).all(), what
            seen[j * stride] += 1
        assert (seen == 1).all(), what
        assert stages[0][2] <= 15, what                          # stage 0 keeps every score: 15 tiles fill its buffers
        assert stages[-1][0] == 1, what
        assert len(stages) <= 11, what
        first = tickets[0]
        assert first[0] == 0 and [b - a for a, b in zip(first, first[1:])] == [4 * c for _, _, c in stages], what


def test_growth_and_error_bound_match_the_rule(prog):
    asks, want = [], []
    for kind in (rule.BATCH, rule.SWEEP_VALU, rule.SWEEP_MFMA):
        for i8 in (0, 1):
            for k in (1, 10, 32, 33, 100):
                for nrows in (1000, 3_999_999, 4_000_000):
                    for eg, egs in ((0, 0), (16, 0), (0, 8), (4, 16)):
                        asks.append(f"growth {kind} {i8} {k} {nrows} {eg} {egs}")
                        want.append(f"growth {rule.growth(kind, i8, k, nrows, eg, egs)}")
            for dpad in (64, 128, 256, 768, 1024, 4096):
                asks.append(f"eps {kind} {i8} {dpad}")
                want.append(f"eps {np.float32(rule.eps_rel(kind, i8, dpad)).view(np.uint32):08x}")
    assert _ask(prog, asks) == want


def test_plan_program_under_address_and_undefined_sanitizers(tmp_path):
    """the same program, instrumented: every array write of cascade_plan / cascade_tickets checked, up to the longest plans
    (growth 2 over 2^60 tiles: the strides 2^59 .. 1, 60 stages, beyond the ticket table)"""
    san = _build(tmp_path, "cascade_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    asks = [f"plan {nt} {g} {fill} {split}" for nt in list(range(1, 400)) + NTILES[-6:] + [2 ** 28 - 1, 2 ** 28, 2 ** 40, 2 ** 60]
            for g in (2,) + GROWTHS for fill in (0, 1) for split in (0, 1)]
    out = _ask(san, asks + ["growth 2 1 10 50000 0 0", "eps 0 1 768"])
    stages, tickets = _parse_plan(out[asks.index("plan 1152921504606846976 2 0 1")])
    assert stages == rule.plan(2 ** 60, 2, False, True) and len(stages) == 60 and tickets is None
    assert _parse_plan(out[asks.index(f"plan {2 ** 28} 4 1 1")])[1] is None      # tickets beyond an int: one launch per stage
    assert _parse_plan(out[asks.index(f"plan {2 ** 28 - 1} 4 1 1")])[1] is not None
