"""The peaked-softmax fixtures (g3_att_peaked_e64, g3_att_peaked_none, g3_att_train_peaked: tests/golden/make_golden.py,
golden_g3_peaked) really are peaked, and their conditioning.  CPU only.

With trained weights AttentionNCF's softmax is peaked: one rated item takes almost all the weight, the logits of a row spread over tens
of units and most exp terms underflow.  These tests keep a later regeneration from drifting back to diffuse weights, check the float64
softmax of test_gpu_attention_softmax against the reference's own F.softmax / nan_to_num on the fixtures' logits, and hold the
condition estimate that the GPU route tests (test_gpu_attention.py) widen their bar by to the reference's own fp32 rounding.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import ncf_oracle as O
from test_gpu_attention_softmax import masked_softmax64

EVAL = ["g3_att_peaked_e64", "g3_att_peaked_none"]
ALL = EVAL + ["g3_att_train_peaked"]


def _dense_logits(a):
    """The reference's raw logits (attOut, attention_ncf.py:179) scattered into the (B, I) matrix of -inf (:182, :192)."""
    um = torch.from_numpy(a["user_matrix"])
    valid = um != 0
    s = torch.full(um.shape, -float("inf"), dtype=torch.float64)
    s[valid] = torch.from_numpy(a["logits"]).double()
    return s, valid


def _float64_forward(state, a, logits=None):
    """attention_ncf.py:136-224 in float64 on the fixture (eval mode): (out, weights, logits, d out / d logits).  ``logits`` replaces
    the computed ones (used to propagate a perturbation)."""
    st = {k: v.double() for k, v in state.items()}
    cand, rated, um = (torch.from_numpy(a[k]).double() for k in ("candidate_items", "rated_items", "user_matrix"))
    ce = F.linear(cand, st["ItemEmbeddings.0.weight"], st["ItemEmbeddings.0.bias"])
    re = F.linear(rated, st["ItemEmbeddings.0.weight"], st["ItemEmbeddings.0.bias"])
    B, I = um.shape
    x = torch.cat((ce[:, None, :].expand(B, I, -1), re[None].expand(B, I, -1)), 2)
    s = O.mlp_forward(x, O.mlp_weights(st, "AttentionNet")).squeeze(-1)
    valid = um != 0
    s = s.detach().requires_grad_(True)
    w = torch.softmax(torch.where(valid, s, torch.tensor(-float("inf"), dtype=torch.float64)), 1).nan_to_num(0.0)
    ue = F.linear((w * um) @ rated, st["UserEmbeddings.0.weight"], st["UserEmbeddings.0.bias"])
    out = O.mlp_forward(torch.cat((ce, ue), 1), O.mlp_weights(st))
    g, = torch.autograd.grad(out.sum(), s)          # row b of the logits only reaches out[b]
    return out.detach(), w.detach(), s.detach(), torch.where(valid, g, torch.zeros_like(g))


def peaked_condition(name):
    """(float64 out, float64 weights, extra out bar, extra weight bar) of an eval fixture.

    The logits of a peaked fixture are sums of terms much larger than themselves (AttentionNet's output weight is scaled by
    ``att_scale``): computed in fp32 they carry a rounding that no kernel avoids, and it moves the weights and the output by more than
    the default bar (1e-5 relative).  The fixture stores the reference's own fp32 logits; ``eps`` = their largest distance from the
    float64 logits is the measured size of that rounding.  Two fp32 evaluations (the reference's and the kernel's, in other summation
    orders) each carry up to ``eps`` on every logit, so to first order the output of pair b may differ by
    ``sum_e |d out_b / d s_e| * 2 eps`` and weight e by ``w_e (2 eps + sum_j w_j 2 eps)`` (softmax derivative): those are the extra
    bars.  They bound a logit rounding only: an error in the softmax, the merge or the weighted sum is pinned separately at the default
    bar with exact logits (test_gpu_attention_softmax)."""
    state, a, kw = load_golden(name)
    out, w, s, g = _float64_forward(state, a)
    s32, valid = _dense_logits(a)
    eps = float((s32 - s)[valid].abs().max())
    ds = torch.where(valid, torch.full_like(s, 2 * eps), torch.zeros_like(s))
    d_out = (g.abs() * ds).sum(1, keepdim=True)
    d_w = w * (ds + (w * ds).sum(1, keepdim=True))
    return out, w, d_out, d_w


def _row_stats(a):
    s, valid = _dense_logits(a)
    att = torch.from_numpy(a["att"]).double()
    rows = valid.sum(1) >= 2
    fin = torch.where(valid, s, torch.full_like(s, float("nan")))
    spread = (torch.nan_to_num(fin, nan=-1e30).max(1).values - torch.nan_to_num(fin, nan=1e30).min(1).values)[rows]
    return att.max(1).values[rows], spread, rows


@pytest.mark.parametrize("name", ALL)
def test_fixture_is_peaked(name):
    """Median row max weight >= 0.9 and per-row logit spread >= 60 (the e64 and the linear fixtures); the train fixture, scaled less
    (make_golden.py TRAIN_PEAK_SCALE: its reference gradients must stay well inside their bar), median >= 0.75 and spread >= 20 over
    rows of ~75 entries; the scale is recorded."""
    state, a, kw = load_golden(name)
    assert float(a["att_scale"]) >= 100.0
    maxw, spread, rows = _row_stats(a)
    med, low, sp = float(maxw.median()), float(maxw.min()), float(spread.min())
    print(f"{name}: c = {float(a['att_scale']):g}, median row max weight {med:.4f}, minimum {low:.3f}, minimum logit spread {sp:.1f}")
    train = name == "g3_att_train_peaked"
    assert med >= (0.75 if train else 0.9)
    assert sp >= (20.0 if train else 60.0)
    assert low > 0.2                                   # no row is diffuse either
    assert int(rows.sum()) >= 5


@pytest.mark.parametrize("name", EVAL)
def test_fixture_rows_are_the_designed_cases(name):
    """A user's row repeated per candidate; a single-entry row; an empty row (weights all 0: nan_to_num, attention_ncf.py:208-209);
    rows of >= 300 entries in e64 (several 64-entry tiles); ratings of both signs; for some users the row maximum lies beyond the
    first 64 entries of the row (the first tile), and for some the leader's rating is negative."""
    state, a, kw = load_golden(name)
    um = torch.from_numpy(a["user_matrix"])
    att = torch.from_numpy(a["att"])
    s, valid = _dense_logits(a)
    n = valid.sum(1)
    assert bool((n == 1).any()) and bool((n == 0).any())
    assert float(att[n == 0].abs().sum()) == 0.0
    assert bool((att[n == 1][valid[n == 1]] == 1.0).all())
    assert bool((um > 0).any()) and bool((um < 0).any())
    distinct = torch.unique(um, dim=0)
    assert distinct.shape[0] * 4 <= um.shape[0]       # rows shared by several candidates (the grouped kernels' call shape)
    if name == "g3_att_peaked_e64":
        assert int((n >= 300).sum()) >= um.shape[0] // 2
        assert kw["item_emb"] == kw["user_emb"] == 64 and kw["att_dense"] == 128 and kw["mlp_dense_layers"] == [256, 128]
    lead = torch.where(valid, s, torch.full_like(s, -float("inf"))).argmax(1)
    pos = torch.tensor([int(valid[b, :int(lead[b])].sum()) for b in range(um.shape[0])])    # position of the leader in its CSR row
    many = n >= 2
    assert bool((pos[many] >= 64).any()) or name == "g3_att_peaked_none"
    assert bool((um[torch.arange(um.shape[0]), lead][many] < 0).any())


@pytest.mark.parametrize("name", ALL)
def test_float64_softmax_matches_the_reference_softmax(name):
    """masked_softmax64 (the float64 reference of test_gpu_attention_softmax) == the reference's F.softmax over the (B, I) matrix of
    -inf + nan_to_num (attention_ncf.py:182-209) on the fixture's logits, and both round to the stored fp32 weights (eval fixtures;
    the train fixture's weights also carry the target mask)."""
    state, a, kw = load_golden(name)
    s, valid = _dense_logits(a)
    if name.startswith("g3_att_train"):
        cand, rated = torch.from_numpy(a["candidate_items"]), torch.from_numpy(a["rated_items"])
        ce = F.linear(cand, state["ItemEmbeddings.0.weight"], state["ItemEmbeddings.0.bias"])
        re = F.linear(rated, state["ItemEmbeddings.0.weight"], state["ItemEmbeddings.0.bias"])
        same = torch.isclose(ce[:, None, :], re[None], atol=1e-5).all(2)           # :195-205
        valid = valid & ~same
        s = torch.where(valid, s, torch.full_like(s, -float("inf")))
    ref = F.softmax(s, dim=1).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
    B = s.shape[0]
    rowptr = torch.zeros(B + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(valid.sum(1), 0)
    w = masked_softmax64(s[valid], rowptr)
    dense = torch.zeros_like(s)
    dense[valid] = w
    assert float((dense - ref).abs().max()) <= 1e-15
    assert float((dense - torch.from_numpy(a["att"]).double()).abs().max()) <= 1e-6      # fp32 softmax of the same fp32 logits


@pytest.mark.parametrize("name", EVAL)
def test_condition_estimate_covers_the_reference_rounding(name):
    """The reference's own fp32 output and weights lie within the default bar plus half the extra bar of peaked_condition from the
    float64 evaluation (half: one of the two fp32 evaluations the extra bar allows for), and the float64 evaluation reproduces the
    stored logits to that rounding."""
    state, a, kw = load_golden(name)
    out, w, d_out, d_w = peaked_condition(name)
    ref_out, ref_w = torch.from_numpy(a["out"]).double(), torch.from_numpy(a["att"]).double()
    bar_out = 1e-5 * out.abs() + 1e-6 * out.abs().max() + d_out / 2
    bar_w = 1e-5 * w.abs() + 1e-6 * w.abs().max() + d_w / 2
    assert bool(((ref_out - out).abs() <= bar_out).all())
    assert bool(((ref_w - w).abs() <= bar_w).all())
    extra = float((d_out / (1e-5 * out.abs() + 1e-6 * out.abs().max())).max())
    print(f"{name}: largest extra output bar {extra:.2f} x the default")
