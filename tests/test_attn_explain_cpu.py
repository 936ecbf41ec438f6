"""CPU tests of tests/attn_explain_ref.py: the builder's margins hold on every case the GPU test uses (so the expected lists are
exact), the fp32 emulator of attn_explain_kernel's walk passes the check the GPU test applies, and each of eight seeded defects
fails it."""
import itertools

import numpy as np
import pytest
import torch

import attn_explain_ref as XR
import attn_forms_ref as R
from test_gpu_basic import assert_close


def _close(got, ref, tag):
    assert_close(got, ref)


def test_gpu_cases_cover_every_combination():
    cs = XR.GPU_CASES
    assert {c[0] for c in cs} == {m for m, _ in XR.MODES} and {c[2] for c in cs} == {1, 130}
    for a, b, va, vb in ((3, 4, (1, 3, 4, 5), (1, 8, 64)), (3, 5, (1, 3, 4, 5), ("rule", "all", "none")), (4, 5, (1, 8, 64), ("rule", "all", "none"))):
        assert {(c[a], c[b]) for c in cs} == set(itertools.product(va, vb))


@pytest.mark.parametrize("c", XR.GPU_CASES, ids=XR.case_id)
def test_margins_hold_on_every_gpu_case(c):
    case = XR.explain_inputs(*c)              # the builder asserts the margins; once more on the finished case
    XR.check_margins(case)
    assert case["min_gap"] > XR.MARGIN
    exp = XR.expected(case)
    counts = np.array([[p[0] for p in row] for row in exp])
    if c[5] == "none":
        assert not counts.any()
    if c[5] == "all":                        # everything qualifies: the count is the number of valid entries, the list is cut at E
        assert counts.max() > 256 > c[4] and all(len(p[1]) == min(p[0], c[4]) for row in exp for p in row)
    if c[5] == "rule" and c[0] in (R.ATT_COS, R.ATT_LINEAR):     # the MLP cases' weights are near uniform: none reaches 1.5 / n
        assert counts.any() and counts.min() == 0
    u, s = case["empty_slot"]
    assert counts[u, s] == 0


@pytest.mark.parametrize("kind,E", [("rule", 8), ("all", 8), ("all", 64), ("none", 1), ("rule", 1)])
def test_the_right_walk_passes_the_gpu_check(kind, E):
    case = XR.explain_inputs(R.ATT_LINEAR, 1, 130, 5, E, kind, XR.SEED)
    XR.check(case, XR.emulate(case), _close, "emulator")


@pytest.mark.parametrize("defect", XR.DEFECTS)
def test_each_seeded_defect_fails_the_gpu_check(defect):
    case = XR.explain_inputs(R.ATT_LINEAR, 1, 130, 5, 8, XR.DEFECT_THR[defect], XR.SEED)
    with pytest.raises(AssertionError):
        XR.check(case, XR.emulate(case, defect), _close, defect)


def test_ties_are_present_where_the_tie_rule_is_tested():
    """Equal logits give equal weights: among the first E of some pair two float64 weights are equal, so the tie rule decides."""
    case = XR.explain_inputs(R.ATT_LINEAR, 1, 130, 5, 8, "all", XR.SEED)
    assert any(len(np.unique(p[2])) < len(p[2]) for row in XR.expected(case) for p in row)


def test_a_written_guard_word_fails_the_check():
    case = XR.explain_inputs(R.ATT_LINEAR, 1, 130, 5, 8, "rule", XR.SEED)
    bufs = XR.emulate(case)
    bufs[3][case["U"] * case["k"]] = 0
    with pytest.raises(AssertionError):
        XR.check(case, bufs, _close, "guard")
