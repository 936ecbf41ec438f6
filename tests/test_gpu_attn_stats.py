"""ncf_attn_stats (csrc/attn_stats.hip) and the layers above it: native.attn_stats against the float64 tables of
tests/attn_stats_ref.py (tests/test_attn_stats_cpu.py shows that the check rejects eight seeded defects), the order contract (equal
bits on a second run and from two half-file calls), the sticky out-of-range flag, ``attention_statistics`` against the dense route —
the per-pair forward with ``return_attention_weights=True`` and a float64 ``index_add_`` — and against the tables the reference
itself accumulated (tests/golden/g9_att_stats.npz), and ``eval_model(att_stats=True)``.

The kernel gets the exact table (the cases' logits are exact in fp32) as a column slice of a wider poisoned buffer; both tables are
strided views of buffers of sentinels with guard words after every row and after the last."""
import numpy as np
import pandas as pd
import pytest
import torch

import attn_forms_ref as R
import attn_stats_ref as SR
from conftest import load_golden
from test_gpu_attn_explain import F_DIM, FORMS, I_CAT, N_USERS, build_model, build_world
from test_gpu_basic import assert_close

pytestmark = pytest.mark.gpu


def _close(got, ref, tag):
    assert_close(got, ref)


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    assert n.ATTN_STATS_SLAB == SR.SLAB
    return n


def _device_case(case, gpu):
    Ic = case["Ic"]
    return dict(st=R.wide(case["st64"].float(), Ic + 4).to(gpu)[:, :Ic], rowptr=case["rowptr"].to(gpu), col=case["col"].to(gpu),
                user_rows=case["user_rows"].to(gpu), cands=case["cands"].to(gpu))


def _run(native, case, dev, bufs, lo=0, hi=None, **kw):
    """One call on samples [lo, hi) into the tables inside ``bufs`` (device buffers of SR.fresh_tables)."""
    tsum, tcnt = SR.views(case, bufs)
    a = {**dev, **kw}
    got = native.attn_stats(a["st"], a["rowptr"], a["col"], a["user_rows"][lo:hi].contiguous(), a["cands"][lo:hi].contiguous(), tsum, tcnt)
    assert got[0].data_ptr() == tsum.data_ptr() and got[1].data_ptr() == tcnt.data_ptr()


def _fresh(case, init, gpu):
    return tuple(b.to(gpu) for b in SR.fresh_tables(case, init))


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("c", SR.GPU_CASES, ids=SR.case_id)
def test_tables_against_the_float64_reference(native, gpu, c):
    case = SR.stats_inputs(*c)
    dev = _device_case(case, gpu)
    init = SR.initial_tables(case)                                     # the tables are continued, not overwritten
    bufs = _fresh(case, init, gpu)
    _run(native, case, dev, bufs)
    native.check_oob(gpu)
    whole = tuple(b.cpu() for b in bufs)
    SR.check(case, whole, _close, "attn_stats", init=init)
    again = _fresh(case, init, gpu)
    _run(native, case, dev, again)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(again, whole)), "two calls on the same inputs must give the same bits"
    halves = _fresh(case, init, gpu)
    half = case["S"] // 2
    _run(native, case, dev, halves, 0, half)
    _run(native, case, dev, halves, half, None)
    native.check_oob(gpu)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(halves, whole)), "two half-file calls must give the bits of one call"
    if c[2] == 130 and c[0] == R.ATT_LINEAR:                           # zeroed tables: what the model allocates
        zero = _fresh(case, None, gpu)
        _run(native, case, dev, zero)
        SR.check(case, tuple(b.cpu() for b in zero), _close, "attn_stats from zero")


def test_an_empty_sample_file_leaves_the_tables_untouched(native, gpu):
    case = SR.stats_inputs(R.ATT_LINEAR, 1, 130, R.N_ITEMS, SR.SEED)
    dev = _device_case(case, gpu)
    init = SR.initial_tables(case)
    bufs = _fresh(case, init, gpu)
    before = tuple(b.cpu() for b in bufs)
    _run(native, case, dev, bufs, 0, 0)
    native.check_oob(gpu)
    assert all(torch.equal(b.cpu(), a) for b, a in zip(bufs, before))


def test_out_of_range_rows_and_candidates_raise_at_check_oob(native, gpu):
    case = SR.stats_inputs(R.ATT_LINEAR, 1, 130, R.N_ITEMS, SR.SEED)
    dev = _device_case(case, gpu)
    init = SR.initial_tables(case)
    lens = (case["rowptr"][1:] - case["rowptr"][:-1])[case["user_rows"]]
    victim = int((lens == 200).nonzero()[0])                           # a sample with a live row
    rest = [s for s in range(case["S"]) if s != victim]
    native.check_oob(gpu)
    for name, bads in (("user_rows", (case["n_rows"], -1, 1 << 40)), ("cands", (case["Ic"], -2, 1 << 40))):
        for bad in bads:
            t = case[name].clone()
            t[victim] = bad
            bufs = _fresh(case, init, gpu)
            _run(native, case, dev, bufs, **{name: t.to(gpu)})
            with pytest.raises(IndexError):
                native.check_oob(gpu)
            native.check_oob(gpu)                                      # the raise reset the flag
            SR.check(case, tuple(b.cpu() for b in bufs), _close, f"{name} = {bad}", init=init, samples=rest)   # it added nothing


# ------------------------------------------------------------------------------------------------ the front end against the dense route
N_SAMPLES = 200


@pytest.fixture(scope="module")
def world(gpu):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import SparseRatings
    feats, rowptr, col, val = build_world()
    rng = np.random.default_rng(77)
    users = np.concatenate([np.arange(N_USERS), rng.integers(0, N_USERS, N_SAMPLES - N_USERS)])     # every user, many twice
    cands = rng.choice(np.arange(0, I_CAT, 2), N_SAMPLES)                                           # odd positions: never a candidate
    cands[rng.permutation(N_SAMPLES)[:70]] = 11                                                     # one busy candidate
    p = rng.permutation(N_SAMPLES)
    return dict(feats=feats.to(gpu), ratings=SparseRatings(rowptr.to(gpu), col.to(gpu), val.to(gpu), I_CAT), rowptr=rowptr, col=col, val=val,
                users=torch.tensor(users[p], dtype=torch.int64), cands=torch.tensor(cands[p], dtype=torch.int64))


def _structural_count(world, users, cands):
    rated = torch.zeros((N_USERS, I_CAT), dtype=torch.int64)
    rp = world["rowptr"]
    for u in range(N_USERS):
        rated[u, world["col"][int(rp[u]):int(rp[u + 1])].long()] = 1
    return torch.zeros((I_CAT, I_CAT), dtype=torch.int64).index_add_(0, cands, rated[users])


@pytest.mark.parametrize("form", list(FORMS))
def test_attention_statistics_against_the_dense_route(gpu, world, form):
    from deeprecommendation_amd import AttentionStats, attention_statistics, native
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import RowsOf, SparseRatings
    m = build_model(form).to(gpu)
    feats, ratings = world["feats"], world["ratings"]
    users, cands = world["users"].to(gpu), world["cands"].to(gpu)
    stats = attention_statistics(m, users, cands, (feats, ratings))
    native.check_oob(gpu)
    assert isinstance(stats, AttentionStats) and stats.sum.shape == stats.count.shape == (I_CAT, I_CAT)
    assert (stats.sum.dtype, stats.count.dtype) == (torch.float64, torch.int64) and stats.sum.device == stats.count.device == feats.device
    # the dense route, from existing functions only: the per-pair forward's (S, I_c) weights, added per candidate in float64
    pairs = SparseRatings(ratings.rowptr, ratings.col, ratings.val, I_CAT, pair_row=users)
    with torch.no_grad():
        _, dense = m(RowsOf(feats, cands), feats, pairs, return_attention_weights=True)
    ref_sum = torch.zeros((I_CAT, I_CAT), dtype=torch.float64).index_add_(0, world["cands"], dense.cpu().double())
    assert torch.equal(stats.count.cpu(), _structural_count(world, world["users"], world["cands"]))
    assert_close(stats.sum, ref_sum)
    assert float(ref_sum.max()) > 1.0 and int((stats.count.sum(1) == 0).sum()) >= I_CAT // 2        # not vacuous; silent candidates
    # out= continues: the file in two pieces gives the bits of one call
    half = N_SAMPLES // 2
    first = attention_statistics(m, users[:half], cands[:half], (feats, ratings))
    both = attention_statistics(m, users[half:], cands[half:], (feats, ratings), out=first)
    assert both.sum.data_ptr() == first.sum.data_ptr() and both.count.data_ptr() == first.count.data_ptr()
    assert torch.equal(both.sum, stats.sum) and torch.equal(both.count, stats.count)
    # with the table cached nothing reads the host: the sample lists are built on the device, no size comes back
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        quiet = attention_statistics(m, users, cands, (feats, ratings))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(quiet.sum, stats.sum) and torch.equal(quiet.count, stats.count)


def test_statistics_need_the_table_only(gpu, world, monkeypatch):
    """user_emb = 48 has no cross kernel; the statistics read the logit table alone.  Inside a stream capture with no table built it
    raises as logit_table does."""
    from deeprecommendation_amd import attention_statistics, native
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.manual_seed(9)
    m = AttentionNCF(item_dim=F_DIM, item_emb=64, user_emb=48, att_dense=32, mlp_dense_layers=[256, 128]).eval().to(gpu)
    assert not native.attn_cross_supported(48)
    users, cands = world["users"].to(gpu), world["cands"].to(gpu)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="never built inside a stream capture"):
        attention_statistics(m, users, cands, (world["feats"], world["ratings"]))
    monkeypatch.undo()
    stats = attention_statistics(m, users, cands, (world["feats"], world["ratings"]))
    native.check_oob(gpu)
    assert torch.equal(stats.count.cpu(), _structural_count(world, world["users"], world["cands"]))
    # a sample's weights sum to 1 (0 for a user without ratings): the row sums count the candidate's samples with a rated item
    n = (world["rowptr"][1:] - world["rowptr"][:-1])[world["users"]]
    live = torch.zeros(I_CAT, dtype=torch.float64).index_add_(0, world["cands"], (n > 0).double())
    assert_close(stats.sum.sum(1), live)


# ------------------------------------------------------------------------------------------------ the reference's own tables
def test_attention_statistics_against_the_reference_tables(gpu):
    from deeprecommendation_amd import attention_statistics, native
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF, SparseRatings
    state, a, kw = load_golden("g9_att_stats")
    m = AttentionNCF(**kw)
    m.load_state_dict(state)
    m = m.eval().to(gpu)
    n = a["features"].shape[0]
    ratings = SparseRatings(*(torch.from_numpy(a[k]).to(gpu) for k in ("rowptr", "col", "val")), n)
    stats = attention_statistics(m, torch.from_numpy(a["users"]).to(gpu), torch.from_numpy(a["cands"]).to(gpu),
                                 (torch.from_numpy(a["features"]).to(gpu), ratings))
    native.check_oob(gpu)
    assert torch.equal(stats.count.cpu(), torch.from_numpy(a["count"]))
    assert_close(stats.sum, torch.from_numpy(a["sum"]))


# ------------------------------------------------------------------------------------------------ eval_model
def test_eval_model_att_stats(gpu, monkeypatch):
    from deeprecommendation_amd import attention_statistics, native
    from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider
    from deeprecommendation_amd.neural_collaborative_filtering import eval as ev
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import SparseRatings
    feats, rowptr, col, _ = build_world()
    rng = np.random.default_rng(31)
    item_ids, user_ids = np.arange(1000, 1000 + I_CAT), np.arange(500, 500 + N_USERS)
    rated = [item_ids[col[int(rowptr[u]):int(rowptr[u + 1])].numpy()] for u in range(N_USERS)]
    stars = [rng.choice([0.5, 1.0, 2.0, 3.0, 4.5, 5.0], len(r)) for r in rated]
    means = np.array([s.mean() if len(s) else 0.0 for s in stars])
    prov = SparseDynamicProvider(item_ids, feats.numpy(), user_ids, rated, stars, means)
    S = 150
    frame = pd.DataFrame({"userId": rng.choice(user_ids, S), "movieId": rng.choice(item_ids[::3], S), "rating": rng.choice([1.0, 2.5, 4.0, 5.0], S)})
    ds = DynamicPointwiseDataset(frame, prov)
    m = build_model("mlp").to(gpu)
    plain = ev.eval_model(m, ds, 64, device=gpu)
    assert set(plain) == {"predictions", "mse", "rmse", "ndcg@5", "adj_ndcg@5", "ndcg@10", "adj_ndcg@10", "ndcg@20", "adj_ndcg@20"}
    monkeypatch.setattr(ev, "ATT_STATS_CHUNK", 64)                     # three chunks
    res = ev.eval_model(m, ds, 64, device=gpu, att_stats=True)
    assert set(res) == set(plain) | {"att_stats"}
    assert np.array_equal(res["predictions"], plain["predictions"]) and res["mse"] == plain["mse"]
    state = prov.device_state(gpu)
    rows, pos = state.train_positions(torch.from_numpy(frame["userId"].to_numpy()).to(gpu), torch.from_numpy(frame["movieId"].to_numpy()).to(gpu))
    ref = attention_statistics(m, rows, pos, (state.features, SparseRatings(state.rowptr, state.col, state.val, state.num_items)))
    native.check_oob(gpu)
    got = res["att_stats"]
    assert torch.equal(got.sum, ref.sum) and torch.equal(got.count, ref.count) and int(got.count.sum()) > 0
    # an id the provider does not know raises at the run's single check
    bad = DynamicPointwiseDataset(frame.assign(movieId=frame["movieId"].where(np.arange(S) != 7, 5000)), prov)
    with pytest.raises(IndexError):
        ev.eval_model(m, bad, 64, device=gpu, att_stats=True)
    native.check_oob(gpu)
