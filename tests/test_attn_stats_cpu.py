"""CPU tests of tests/attn_stats_ref.py and of the host side of the attention statistics: the fp32 emulator of the two kernels' walk
passes the check the GPU test applies and each of eight seeded defects fails it; the float64 route reproduces the tables the
reference itself accumulated (tests/golden/g9_att_stats.npz, made by tests/golden/make_att_stats_golden.py); and
``attention_stat_ratios`` is the reference's formula as written."""
import numpy as np
import pytest
import torch

import attn_forms_ref as R
import attn_stats_ref as SR
from conftest import load_golden
from test_gpu_basic import assert_close


def _close(got, ref, tag):
    assert_close(got, ref)


def _case(Ic, Ir):
    return SR.stats_inputs(R.ATT_LINEAR, 1, Ic, Ir, SR.SEED)


def test_gpu_cases_cover_the_modes_the_sizes_and_the_slab_boundary():
    cs = SR.GPU_CASES
    assert {(c[0], c[2]) for c in cs if c[3] == R.N_ITEMS} == {(m, Ic) for m, _ in SR.XR.MODES for Ic in (1, 130)}
    assert [c for c in cs if c[3] != R.N_ITEMS] == [(R.ATT_MLP, 12, 2, SR.SLAB + 1, SR.SEED)]
    for c in cs:
        SR.stats_inputs(*c)                                            # the builder asserts what the case promises


@pytest.mark.parametrize("Ic,Ir", [(130, R.N_ITEMS), (1, R.N_ITEMS), (2, SR.SLAB + 1)])
@pytest.mark.parametrize("continued", [False, True])
def test_the_right_walk_passes_the_gpu_check(Ic, Ir, continued):
    case = _case(Ic, Ir)
    init = SR.initial_tables(case) if continued else None
    SR.check(case, SR.emulate(case, init=init), _close, "emulator", init=init)


@pytest.mark.parametrize("defect", SR.DEFECTS)
def test_each_seeded_defect_fails_the_gpu_check(defect):
    case = _case(*SR.DEFECT_SHAPE[defect])
    init = SR.initial_tables(case)
    with pytest.raises(AssertionError):
        SR.check(case, SR.emulate(case, defect, init=init), _close, defect, init=init)


def test_a_written_guard_word_fails_the_check():
    case = _case(130, R.N_ITEMS)
    for k, pos in ((0, case["Ir"]), (1, case["Ic"] * (case["Ir"] + SR.LD_EXTRA))):       # after a row; after the table
        bufs = SR.emulate(case)
        bufs[k][pos] = 0
        with pytest.raises(AssertionError, match="guard word"):
            SR.check(case, bufs, _close, "guard")


def test_two_halves_add_up_to_the_whole_file():
    case = _case(130, R.N_ITEMS)
    half = case["S"] // 2
    first = SR.expected(case, samples=range(half))
    both = SR.expected(case, init=first, samples=range(half, case["S"]))
    whole = SR.expected(case)
    assert torch.equal(both[0], whole[0]) and torch.equal(both[1], whole[1])      # float64 additions in the same order: the same bits


# ------------------------------------------------------------------------------------------------ the reference's own tables
def golden_case():
    """g9_att_stats as an attn_stats_ref case: the logit table in float64 from the stored weights through the oracle's layers."""
    from oracle import ncf_oracle as O
    state, a, kw = load_golden("g9_att_stats")
    assert kw["att_dense"] == 8 and not kw["use_cos_sim_instead"]
    st64 = {k: v.double() for k, v in state.items()}
    feats = torch.from_numpy(a["features"]).double()
    n = feats.shape[0]
    emb = torch.nn.functional.linear(feats, st64["ItemEmbeddings.0.weight"], st64["ItemEmbeddings.0.bias"])
    att_in = torch.cat((emb.repeat_interleave(n, dim=0), emb.repeat(n, 1)), dim=1)      # (candidate c, rated j) at row c * n + j
    logits = O.mlp_forward(att_in, O.mlp_weights(st64, "AttentionNet")).view(n, n)
    case = dict(Ic=n, Ir=n, n_rows=len(a["rowptr"]) - 1, rowptr=torch.from_numpy(a["rowptr"]), col=torch.from_numpy(a["col"]),
                user_rows=torch.from_numpy(a["users"]), cands=torch.from_numpy(a["cands"]), S=len(a["users"]), st64=logits.t().contiguous())
    return case, state, a, kw


def test_float64_route_reproduces_the_reference_tables():
    case, _, a, _ = golden_case()
    lens = np.diff(a["rowptr"])
    assert case["S"] == 160 and case["Ic"] == 48 and {0, 1}.issubset(lens.tolist()) and lens.max() > 32
    ref_sum, ref_count = torch.from_numpy(a["sum"]), torch.from_numpy(a["count"])
    assert ref_sum.dtype == torch.float64 and ref_count.dtype == torch.int64
    got_sum, got_count = SR.expected(case)
    assert torch.equal(got_count, ref_count)
    assert_close(got_sum, ref_sum)
    per = np.bincount(a["cands"], minlength=48)
    assert (per == 0).sum() >= 15 and per.max() >= 40                                   # silent candidates and a busy one
    # the reference's count is structural: the samples whose user rated j, per (candidate, j)
    dense = np.zeros((case["n_rows"], 48), dtype=np.int64)
    for u in range(case["n_rows"]):
        dense[u, a["col"][a["rowptr"][u]:a["rowptr"][u + 1]]] = 1
    structural = np.zeros((48, 48), dtype=np.int64)
    np.add.at(structural, a["cands"], dense[a["users"]])
    assert np.array_equal(structural, a["count"])


# ------------------------------------------------------------------------------------------------ attention_stat_ratios
def test_ratios_are_the_reference_formula_as_written():
    from deeprecommendation_amd import AttentionStats, attention_stat_ratios
    rng = np.random.default_rng(5)
    s = rng.random((12, 12)) * 3
    c = rng.integers(0, 9, (12, 12))
    c[4] = 0                                                           # a candidate that was never sampled: its row maximum is 0
    s[4] = 0.0
    pos = np.array([7, 4, 0, 11, 2])
    stats = AttentionStats(torch.from_numpy(s), torch.from_numpy(c))
    for positions in (pos, pos.tolist(), torch.from_numpy(pos)):
        sub_s, sub_c, ratio = attention_stat_ratios(stats, positions)
        ref_s, ref_c = s[pos, :][:, pos], c[pos, :][:, pos]            # plots.py:173-174
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = ref_s / np.max(ref_c, 1)                             # plots.py:181
        assert np.array_equal(sub_s, ref_s) and np.array_equal(sub_c, ref_c) and sub_c.dtype == np.int64
        assert np.array_equal(ratio, ref, equal_nan=True)
        assert np.isnan(ratio[1, 1]) and np.isinf(ratio[0, 1])         # 0 / 0 and x / 0, as numpy gives them
        # the vector of row maxima broadcasts over the LAST axis: cell (i, j) is divided by the maximum of row j
        assert ratio[0, 2] == ref_s[0, 2] / ref_c[2].max() and ref_c[2].max() != ref_c[0].max()
    e = attention_stat_ratios(stats, [])
    assert e[0].shape == e[1].shape == e[2].shape == (0, 0)
