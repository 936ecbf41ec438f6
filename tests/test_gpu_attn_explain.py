"""ncf_attn_explain (csrc/attn_explain.hip) and the layers above it: native.attn_explain against the exact expected lists of
tests/attn_explain_ref.py (tests/test_attn_explain_cpu.py shows that the check rejects eight seeded defects), a peaked softmax, the
sticky out-of-range flag, and ``explain_items`` against the dense route — the per-pair forward with
``return_attention_weights=True``, an independent kernel — and against ``recommend_for_user``.

The kernel gets the exact table (the cases' logits are exact in fp32) as a column slice of a wider poisoned buffer; every output is
the head of a buffer of sentinels with guard words behind it."""
import numpy as np
import pytest
import torch

import attn_explain_ref as XR
import attn_forms_ref as R
from test_gpu_attn_cross import _peaked_case
from test_gpu_basic import assert_close

pytestmark = pytest.mark.gpu

BAND = 1e-4                # relative: the dense route and the table route may disagree on what lies this close (10 x the project's bar)


def _close(got, ref, tag):
    assert_close(got, ref)


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def _run(native, case, gpu, st=None):
    Ic = case["Ic"]
    st = R.wide(case["st64"].float(), Ic + 4).to(gpu)[:, :Ic] if st is None else st
    bufs = tuple(b.to(gpu) for b in XR.fresh_outputs(case))
    out = XR.views(case, bufs)
    got = native.attn_explain(st, case["rowptr"].to(gpu), case["col"].to(gpu), case["val"].to(gpu), case["user_rows"].to(gpu),
                              case["items"].to(gpu), case["thr"].to(gpu), case["E"], out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    return tuple(b.cpu() for b in bufs)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("c", XR.GPU_CASES, ids=XR.case_id)
def test_explanations_against_the_exact_lists(native, gpu, c):
    case = XR.explain_inputs(*c)
    bufs = _run(native, case, gpu)
    native.check_oob(gpu)                                              # the -1 slot is no error
    XR.check(case, bufs, _close, "attn_explain")
    again = _run(native, case, gpu)
    assert all(torch.equal(a, b) for a, b in zip(bufs, again)), "two calls on the same inputs must give the same bits"


def test_fresh_outputs_are_allocated_when_none_are_given(native, gpu):
    case = XR.explain_inputs(R.ATT_LINEAR, 1, 130, 3, 8, "rule", XR.SEED)
    want = XR.views(case, _run(native, case, gpu))
    got = native.attn_explain(case["st64"].float().to(gpu), *(case[k].to(gpu) for k in ("rowptr", "col", "val", "user_rows", "items", "thr")), 8)
    assert [g.dtype for g in got] == [torch.int32, torch.float32, torch.float32, torch.int32]
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))     # a contiguous table and a column slice: the same bits


# ------------------------------------------------------------------------------------------------ a peaked softmax
def test_peaked_rows(native, gpu):
    """Logits in [82, 92] (exp overflows without the max subtraction), in [-200, -190] (0 / 0 without it) and leaders 60 above the
    rest: everything finite, the leader the single reason with weight >= 1 - 1e-6."""
    case = _peaked_case()
    Ic, user_rows, rp = case["Ic"], case["user_rows"], case["rowptr"]
    U = user_rows.numel()
    st = R.wide(case["st64"].float(), Ic + 4).to(gpu)[:, :Ic]
    items = torch.tensor([[0, 77, Ic - 1]] * U, dtype=torch.int64)
    args = [case[k].to(gpu) for k in ("rowptr", "col", "val", "user_rows")] + [items.to(gpu)]
    half = [t.cpu() for t in native.attn_explain(st, *args, torch.full((U,), 0.5).to(gpu), 8)]
    every = [t.cpu() for t in native.attn_explain(st, *args, torch.full((U,), -1.0).to(gpu), 64)]
    native.check_oob(gpu)
    leader = {2: 0, 3: 64, 4: 130}                                     # row -> the leader's offset in it
    for u, r in enumerate(user_rows.tolist()):
        n = int(rp[r + 1] - rp[r])
        assert bool(torch.isfinite(every[1][u]).all()) and bool(torch.isfinite(half[1][u]).all())
        assert every[3][u].tolist() == [n] * 3
        for s in range(3):
            w64 = torch.softmax(case["st64"][int(rp[r]):int(rp[r + 1]), int(items[u, s])], 0)
            top = torch.sort(w64, descending=True, stable=True).values[:64]
            assert_close(every[1][u, s], top)
            if r in leader:
                assert int(half[3][u, s]) == 1 and int(half[0][u, s, 0]) == int(rp[r]) + leader[r]
                assert float(half[1][u, s, 0]) >= 1 - 1e-6 and int(every[0][u, s, 0]) == int(rp[r]) + leader[r]
                assert float(half[2][u, s, 0]) == float(case["val"][int(rp[r]) + leader[r]])
                assert half[0][u, s, 1:].tolist() == [-1] * 7
            else:                                                      # 150 logits within 10 of each other: none takes half the weight
                assert int(half[3][u, s]) == 0


# ------------------------------------------------------------------------------------------------ the sticky flag
def test_out_of_range_rows_and_items_raise_at_check_oob(native, gpu):
    case = XR.explain_inputs(R.ATT_LINEAR, 1, 130, 3, 8, "all", XR.SEED)
    st = case["st64"].float().to(gpu)
    dev = {k: case[k].to(gpu) for k in ("rowptr", "col", "val", "user_rows", "items", "thr")}
    live = int(((case["rowptr"][1:] - case["rowptr"][:-1])[case["user_rows"]] == 200).nonzero()[0])
    call = lambda **kw: [t.cpu() for t in native.attn_explain(st, *({**dev, **kw}.values()), 8)]
    native.check_oob(gpu)
    good = call()
    native.check_oob(gpu)                                              # -1 does not raise
    assert int(good[3][live].min()) > 0
    for bad in (case["n_rows"], -1, -7):
        rows = case["user_rows"].clone()
        rows[live] = bad
        got = call(user_rows=rows.to(gpu))
        with pytest.raises(IndexError):
            native.check_oob(gpu)
        native.check_oob(gpu)                                          # the raise reset the flag
        assert got[3][live].tolist() == [0, 0, 0] and bool((got[0][live] == -1).all()) and bool((got[1][live] == 0).all())
        keep = torch.arange(case["U"]) != live
        assert all(torch.equal(g[keep], w[keep]) for g, w in zip(got, good))
    for bad in (case["Ic"], -2, 1 << 40):
        items = case["items"].clone()
        items[live, 1] = bad
        got = call(items=items.to(gpu))
        with pytest.raises(IndexError):
            native.check_oob(gpu)
        assert int(got[3][live, 1]) == 0 and bool((got[0][live, 1] == -1).all()) and bool((got[2][live, 1] == 0).all())
        assert int(got[3][live, 0]) == int(good[3][live, 0]) and torch.equal(got[0][live, 0], good[0][live, 0])


# ------------------------------------------------------------------------------------------------ the front end against the dense route
I_CAT, F_DIM, N_USERS, TOP = 130, 40, 40, 5
FORMS = {"mlp": dict(att_dense=32), "linear": dict(att_dense=None), "cos": dict(att_dense=None, use_cos_sim_instead=True)}
# random initialisation, then the attention's own weights scaled so that its softmax is not flat (a flat one explains nothing:
# no weight reaches 1.5 / n).  The cosine's logits stay within [-1, 1] whatever the weights, so that form is asked with a lower rule.
# Seeds, gains and rules were chosen so that the DENSE route alone keeps the share of ambiguous pairs under 2 %
GAIN = {"mlp": 24.0, "linear": 20.0, "cos": 30.0}
RULE = {"mlp": (1.5, 0.025), "linear": (1.5, 0.025), "cos": (1.3, 0.005)}       # (explain_factor, explain_constant)
WORLD_SEED = 2026


def build_world():
    """Catalogue features, the users' CSR (40 users with 0 .. 130 ratings — a row lists a catalogue position once, so the catalogue
    bounds it —, columns ascending as a provider builds them, ratings of both signs and never 0), on the CPU."""
    rng = np.random.default_rng(WORLD_SEED)
    feats = ((rng.random((I_CAT, F_DIM)) < 0.2) * rng.random((I_CAT, F_DIM))).astype(np.float32)
    lens = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 63, 64, 65, 89, 129, 130, 0]
    lens += rng.integers(0, I_CAT + 1, N_USERS - len(lens)).tolist()
    cols = [np.sort(rng.permutation(I_CAT)[:n]) for n in lens]
    rowptr = torch.zeros(N_USERS + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(lens), 0)
    col = torch.tensor(np.concatenate(cols), dtype=torch.int32)
    val = torch.tensor(rng.choice([-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0, 2.5], col.numel()), dtype=torch.float32)
    return torch.from_numpy(feats), rowptr, col, val


def build_model(form):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.manual_seed(300 + list(FORMS).index(form))
    m = AttentionNCF(item_dim=F_DIM, item_emb=64, user_emb=64, mlp_dense_layers=[256, 128], **FORMS[form]).eval()
    with torch.no_grad():
        if form == "cos":
            m.ItemEmbeddings[0].weight.mul_(GAIN[form])               # the cosine is scale free: make the directions differ instead
        else:
            m.AttentionNet[-1].weight.mul_(GAIN[form])
    return m


def compare_with_dense(ex, dense, rowptr, col, users, E):
    """``ex``: Explanations on the CPU; ``dense`` (B, k, I) the dense route's weights.  An entry within BAND (relative) of the
    threshold may be in or out, and two listable entries closer than BAND to each other may swap; outside those, sets, order and
    counts agree and the weights meet the project's bar.  Returns (pairs with an ambiguous entry, pairs, pairs with a reason)."""
    B, k = ex.counts.shape
    ambiguous = explained = 0
    got_w, ref_w = [], []
    for b in range(B):
        u = int(users[b])
        cols = col[int(rowptr[u]):int(rowptr[u + 1])].long()
        t = float(ex.threshold[b])
        for s in range(k):
            dw = dense[b, s][cols].double()
            sure, maybe = dw > t * (1 + BAND), (dw - t).abs() <= t * BAND
            listable = torch.sort(dw[sure | maybe], descending=True).values
            close = bool(((listable[:-1] - listable[1:]) <= BAND * listable[:-1]).any()) if listable.numel() > 1 else False
            ambiguous += bool(maybe.any()) or close
            cnt = int(ex.counts[b, s])
            assert int(sure.sum()) <= cnt <= int((sure | maybe).sum()), (b, s)
            m = min(cnt, E)
            pos = ex.positions[b, s]
            assert bool((pos[m:] == -1).all()) and bool((ex.weights[b, s, m:] == 0).all()) and bool((ex.ratings[b, s, m:] == 0).all())
            if m == 0:
                continue
            explained += 1
            where = torch.searchsorted(cols, pos[:m])
            assert torch.equal(cols[where.clamp_max(cols.numel() - 1)], pos[:m]), (b, s, "a listed position the user never rated")
            listed = dw[where]
            assert bool((sure | maybe)[where].all()), (b, s, "a listed entry is below the threshold")
            assert len(set(where.tolist())) == m
            assert bool((listed[1:] <= listed[:-1] * (1 + BAND)).all()), (b, s, "not in descending order")
            rest = sure.clone()
            rest[where] = False                                       # sure entries left out: only a cut at E explains them
            if bool(rest.any()):
                assert cnt > E and float(dw[rest].max()) <= float(listed.min()) * (1 + BAND), (b, s)
            got_w.append(ex.weights[b, s, :m])
            ref_w.append(listed)
    if got_w:
        assert_close(torch.cat(got_w), torch.cat(ref_w))
    return ambiguous, B * k, explained


@pytest.fixture(scope="module")
def world(gpu):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import SparseRatings
    feats, rowptr, col, val = build_world()
    ratings = SparseRatings(rowptr.to(gpu), col.to(gpu), val.to(gpu), I_CAT)
    return dict(feats=feats.to(gpu), ratings=ratings, rowptr=rowptr, col=col, val=val)


@pytest.mark.parametrize("form", list(FORMS))
def test_explain_items_against_the_dense_route(gpu, world, form):
    from deeprecommendation_amd import explain_items, native, top_k_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import RowsOf, SparseRatings
    m = build_model(form).to(gpu)
    feats, ratings = world["feats"], world["ratings"]
    users = torch.tensor(np.random.default_rng(7).permutation(N_USERS), dtype=torch.int64, device=gpu)
    _, winners, counts = top_k_items(m, users, TOP, profiles=(feats, ratings))
    assert counts.tolist() == [TOP] * N_USERS
    E = 8
    factor, constant = RULE[form]
    ex = explain_items(m, users, winners, (feats, ratings), max_reasons=E, explain_factor=factor, explain_constant=constant)
    native.check_oob(gpu)
    assert ex.positions.shape == ex.weights.shape == ex.ratings.shape == (N_USERS, TOP, E) and ex.counts.shape == (N_USERS, TOP)
    assert (ex.positions.dtype, ex.weights.dtype, ex.ratings.dtype, ex.counts.dtype, ex.threshold.dtype) == \
        (torch.int64, torch.float32, torch.float32, torch.int32, torch.float32)
    assert all(t.device == feats.device for t in ex)
    # the threshold rule, bit for bit
    n = (world["rowptr"][1:] - world["rowptr"][:-1])[users.cpu()]
    assert torch.equal(ex.threshold.cpu(), factor / n.clamp_min(1).to(torch.float32) + constant)
    if form == "mlp":                                                 # the defaults are the reference's 1.5 and 0.025
        assert torch.equal(explain_items(m, users, winners, (feats, ratings)).threshold, ex.threshold) and RULE[form] == (1.5, 0.025)
    # the dense route: the per-pair forward on the same pairs, weights as a dense (pairs, I) matrix
    pairs = SparseRatings(ratings.rowptr, ratings.col, ratings.val, I_CAT, pair_row=users.repeat_interleave(TOP))
    with torch.no_grad():
        _, dense = m(RowsOf(feats, winners.reshape(-1)), feats, pairs, return_attention_weights=True)
    exc = type(ex)(*(t.cpu() for t in ex))
    amb, total, explained = compare_with_dense(exc, dense.view(N_USERS, TOP, I_CAT).cpu(), world["rowptr"], world["col"], users.cpu(), E)
    print(f"{form}: {amb} of {total} pairs hold an ambiguous entry, {explained} pairs have a reason, max count {int(ex.counts.max())}")
    assert amb <= 0.02 * total
    assert explained >= total // 10                                   # the comparison is not vacuous
    # the ratings are the stored ones
    rp, col, val = world["rowptr"], world["col"], world["val"]
    for b, u in enumerate(users.tolist()):
        cols, vals = col[int(rp[u]):int(rp[u + 1])].long(), val[int(rp[u]):int(rp[u + 1])]
        for s in range(TOP):
            mm = min(int(exc.counts[b, s]), E)
            assert torch.equal(exc.ratings[b, s, :mm], vals[torch.searchsorted(cols, exc.positions[b, s, :mm])])
    # other arguments: another rule and E, winners with an empty slot
    w2 = winners.clone()
    w2[3, 2] = -1
    ex2 = explain_items(m, users, w2, (feats, ratings), max_reasons=3, explain_factor=1.25, explain_constant=0.0125)
    native.check_oob(gpu)
    assert torch.equal(ex2.threshold.cpu(), 1.25 / n.clamp_min(1).to(torch.float32) + 0.0125)
    assert int(ex2.counts[3, 2]) == 0 and ex2.positions[3, 2].tolist() == [-1] * 3 and ex2.positions.shape == (N_USERS, TOP, 3)


def test_explain_needs_the_table_only(gpu, world, monkeypatch):
    """user_emb = 48 has no cross kernel; the explanation reads the logit table alone.  Inside a stream capture with no table built it
    raises as logit_table does."""
    from deeprecommendation_amd import explain_items, native
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.manual_seed(9)
    m = AttentionNCF(item_dim=F_DIM, item_emb=64, user_emb=48, att_dense=32, mlp_dense_layers=[256, 128]).eval().to(gpu)
    assert not native.attn_cross_supported(48)
    users = torch.arange(N_USERS, dtype=torch.int64, device=gpu)
    items = torch.arange(N_USERS * 2, dtype=torch.int64, device=gpu).view(N_USERS, 2) % I_CAT
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="never built inside a stream capture"):
        explain_items(m, users, items, (world["feats"], world["ratings"]))
    monkeypatch.undo()
    ex = explain_items(m, users, items, (world["feats"], world["ratings"]), max_reasons=64)
    native.check_oob(gpu)
    thr = ex.threshold[:, None, None]
    listed = ex.positions >= 0
    assert bool((ex.weights[listed] > thr.expand_as(ex.weights)[listed]).all()) and bool((ex.counts.clamp_max(64) == listed.sum(2)).all())


# ------------------------------------------------------------------------------------------------ recommend_for_user
def test_consistent_with_recommend_for_user(gpu, world):
    """One user: explain_items on recommend_for_user's k winners gives the same ``because`` sets (an item whose weight lies within
    BAND of the threshold is exempt).  The comparison uses the reference's n_rated for both."""
    import pandas as pd
    from deeprecommendation_amd import explain_items, recommend_for_user
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import SparseRatings
    m = build_model("mlp").to(gpu)
    feats = world["feats"]
    ids = np.arange(1000, 1000 + I_CAT)
    rng = np.random.default_rng(11)
    rated = np.sort(rng.permutation(I_CAT)[:12])
    stars = rng.choice([0.5, 1.0, 2.0, 3.0, 4.0, 4.5, 5.0], 12)
    series = pd.Series(stars, index=ids[rated])
    k, factor, constant = 6, 1.5, 0.025
    frame = recommend_for_user(m, (feats, ids), series, k=k, explain_factor=factor, explain_constant=constant)
    centred = (stars - ((stars.mean() + 2.5) / 2)).astype(np.float32)
    keep = centred != 0
    n_rated = len(rated)                                               # the reference counts a rating of exactly the centre too
    ratings = SparseRatings(torch.tensor([0, int(keep.sum())], dtype=torch.int64, device=gpu),
                            torch.tensor(rated[keep], dtype=torch.int32, device=gpu), torch.tensor(centred[keep], device=gpu), I_CAT)
    winners = torch.tensor((frame["imdbID"].values - 1000)[None], dtype=torch.int64, device=gpu)
    # explain_items counts the stored entries: the same threshold needs factor' / n_stored = factor / n_rated
    ex = explain_items(m, torch.zeros(1, dtype=torch.int64, device=gpu), winners, (feats, ratings), max_reasons=64,
                       explain_factor=factor * int(keep.sum()) / n_rated, explain_constant=constant)
    thr = factor / n_rated + constant
    assert abs(float(ex.threshold[0]) - thr) <= 1e-6 * thr
    some = 0
    for s in range(len(frame)):
        cnt = int(ex.counts[0, s])
        got = set((ex.positions[0, s, :cnt].cpu().numpy() + 1000).tolist())
        ref = set(np.asarray(frame["because"].iloc[s]).tolist())
        att = np.asarray(frame["attention"].iloc[s])
        near = {int(i) for i, w in zip(np.asarray(frame["because"].iloc[s]), att) if abs(w - thr) <= BAND * thr}
        near |= {int(p) + 1000 for p, w in zip(ex.positions[0, s, :cnt].tolist(), ex.weights[0, s, :cnt].tolist()) if abs(w - thr) <= BAND * thr}
        assert got - near == ref - near, (s, got, ref)
        some += len(ref)
    assert some > 0
