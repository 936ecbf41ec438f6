"""Pair-wise (BPR) training on the host against the REFERENCE's own numbers (g9_* fixtures, tests/golden/make_golden_bpr.py):
schedule_w, _negative_sampling_probs, the host __getitem__ draws, BPR_loss, the torch-op pair-wise step of BasicNCF / MF /
AttentionNCF; plus the ranking datasets' construction checks and the maximising EarlyStopping of train_model's ranking branch
(reference train.py:79-210)."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden, onehot

W_SCHEDULE = (0.0, 0.5, 1, 1.5, 3)


def _frame(neg_ids, neg_ratings, users=None, positives=None):
    n = len(neg_ids)
    return pd.DataFrame({"userId": np.arange(n) + 1 if users is None else users,
                         "positive_movieId": np.arange(n) + 9000 if positives is None else positives,
                         "negative_movieIds": list(neg_ids), "negative_ratings": list(neg_ratings)})


def _sampling_dataset():
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import RankingDataset
    _, a, _ = load_golden("g9_bpr_sampling")
    rp = a["rowptr"]
    ids = [a["neg_ids"][rp[k]:rp[k + 1]].tolist() for k in range(len(rp) - 1)]
    rts = [a["neg_ratings"][rp[k]:rp[k + 1]].tolist() for k in range(len(rp) - 1)]
    return RankingDataset(_frame(ids, rts)), a


def test_schedule_w_equals_the_reference():
    from deeprecommendation_amd.neural_collaborative_filtering.train import schedule_w
    _, a, _ = load_golden("g9_bpr_sampling")
    got = np.array([schedule_w(e) for e in range(1, 31)], dtype=np.float64)
    assert np.array_equal(got, a["schedule_w"])
    assert sorted(set(got.tolist())) == [0.0, 0.5, 1.0, 1.5, 3.0]


def test_negative_sampling_probs_equal_the_reference_for_every_type_and_w():
    ds, a = _sampling_dataset()
    rp = a["rowptr"]
    for k, w in enumerate(W_SCHEDULE):
        ds.w = w
        for t in ("sum", "sum_dynamic", "softmax"):
            got = np.concatenate([np.asarray(ds._negative_sampling_probs(np.array(ds._neg_r[rp[r]:rp[r + 1]]), type=t), dtype=np.float64)
                                  for r in range(len(rp) - 1)])
            assert np.array_equal(got, a[f"probs_{t}_{k}"]), (t, w)
        assert ds._negative_sampling_probs(np.array([1.0, 2.0]), type="uniform") is None


def test_host_draws_equal_the_reference_under_the_same_seed():
    ds, a = _sampling_dataset()
    rounds = int(a["draw_rounds"])
    for k, w in enumerate(W_SCHEDULE):
        ds.w = w
        np.random.seed(1234 + k)
        got = np.array([ds[i][2] for _ in range(rounds) for i in range(len(ds))], dtype=np.int64)
        assert np.array_equal(got, a[f"draws_{k}"]), w


def test_bpr_loss_equals_the_reference_including_the_underflow():
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import BPR_loss
    _, a, _ = load_golden("g9_bpr_sampling")
    got = BPR_loss(torch.from_numpy(a["bpr_pos"]), torch.from_numpy(a["bpr_neg"])).item()
    assert got == float(a["bpr_loss"])
    under = BPR_loss(torch.from_numpy(a["bpr_pos_under"]), torch.from_numpy(a["bpr_neg_under"])).item()
    assert np.isinf(under) and np.isinf(float(a["bpr_loss_under"]))


@pytest.mark.parametrize("ids,ratings,words,row", [
    ([[1, 2], [3], []], [[1.0, 2.0], [1.0], []], "empty", 2),
    ([[1, 2], [3]], [[1.0, 2.0], [1.0, 2.0]], "length", 1),
    ([[1, 2], [3, 4]], [[1.0, -0.5], [1.0, 2.0]], "negative", 0),
    ([[1, 2], [3, 4]], [[1.0, 2.0], [np.nan, 2.0]], "NaN", 1),
    ([[1, 2], [3, 4]], [[np.inf, 2.0], [1.0, 2.0]], "infinite", 0),
    ([[1, 2], [3, 4]], [[1.0, 2.0], [0.0, 0.0]], "is 0", 1),
])
def test_ranking_dataset_refuses_rows_it_cannot_sample(ids, ratings, words, row):
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import RankingDataset
    with pytest.raises(ValueError, match=words) as e:
        RankingDataset(_frame(ids, ratings))
    assert f"[{row}]" in str(e.value)


def test_ranking_dataset_flattens_the_lists_into_one_csr():
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import RankingDataset
    ds = RankingDataset(_frame([[5, 6, 7], [8], [9, 10]], [[1.0, 0.0, 3.0], [2.5], [4.0, 4.0]]))
    assert len(ds) == 3 and ds.w == 0.0
    assert ds._rowptr.tolist() == [0, 3, 4, 6]
    assert ds._neg_ids.tolist() == [5, 6, 7, 8, 9, 10]
    assert ds._neg_r.tolist() == [1.0, 0.0, 3.0, 2.5, 4.0, 4.0]
    ds.w = 1.5
    np.random.seed(3)
    draws = [ds[0][2] for _ in range(300)]
    assert 6 not in draws and {5, 7} <= set(draws)          # a zero rating is never drawn once w > 0


def test_graph_ranking_dataset_draws_like_the_base_dataset():
    """GraphRankingDataset draws positions with the same RNG calls as RankingDataset draws ids (gnn_datasets.py:37-44)."""
    from deeprecommendation_amd.content_providers.index_providers import IndexGraphProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import RankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.gnn_datasets import GraphRankingDataset
    rng = np.random.default_rng(2)
    users, items = np.arange(100, 120), np.arange(10, 50)
    gcp = IndexGraphProvider(users, items, rng.choice(users, 200), rng.choice(items, 200), rng.integers(1, 11, 200) * 0.5)
    ids = [rng.choice(items, int(rng.integers(1, 6)), replace=False) for _ in range(40)]
    frame = _frame(ids, [rng.integers(0, 11, len(x)) * 0.5 + 0.5 for x in ids], users=rng.choice(users, 40), positives=rng.choice(items, 40))
    base, graph = RankingDataset(frame), GraphRankingDataset(frame, gcp)
    base.w = graph.w = 1.5
    np.random.seed(8)
    want = [base[i] for i in range(40)]
    np.random.seed(8)
    got = [graph[i] for i in range(40)]
    for (u, p, n), (gu, gp, gn) in zip(want, got):
        assert (gu, gp, gn) == (gcp.get_user_nodeID(u), gcp.get_item_nodeID(p), gcp.get_item_nodeID(n))


def _replay_ranking_branch(ndcgs, patience, max_patience):
    """train.py:165-212 for a RankingDataset, literally (the `previous is not None and ... or ...` precedence included)."""
    verdicts, early_stop_times, best, previous, starting_max_patience = [], 0, None, None, max_patience
    for val_ndcg in ndcgs:
        if best is None or val_ndcg > best:
            best, early_stop_times, max_patience = val_ndcg, 0, starting_max_patience
            verdicts.append(("best", best, early_stop_times))
        else:
            if previous is not None and False or (val_ndcg < previous):
                early_stop_times += 1
            else:
                early_stop_times = max(0, early_stop_times - 1)
            max_patience -= 1
            stop = early_stop_times > patience or max_patience <= 0
            verdicts.append(("stop" if stop else "continue", best, early_stop_times))
            if stop:
                break
        previous = val_ndcg
    return verdicts


def test_early_stopping_maximising_mode_follows_the_reference_ranking_branch():
    from deeprecommendation_amd.neural_collaborative_filtering.train import EarlyStopping
    rng = np.random.default_rng(9)
    for trial in range(300):
        patience, max_patience = int(rng.integers(0, 4)), int(rng.integers(1, 7))
        ndcgs = np.round(rng.random(30) * 0.3 + np.linspace(0.5, 0.8, 30) * rng.random(), 2)   # rounding: exact ties occur
        if trial % 4 == 0:
            ndcgs[rng.integers(0, 30, 3)] = np.nan                                             # NaN NDCGs, the first epoch's too
        want = _replay_ranking_branch(list(ndcgs), patience, max_patience)
        es = EarlyStopping(patience, max_patience, maximize=True)
        for epoch, (verdict, best, strikes) in enumerate(want):
            assert es.update(float(ndcgs[epoch]), epoch) == verdict, (trial, epoch)
            assert (es.best == best or (np.isnan(es.best) and np.isnan(best))) and es.strikes == strikes, (trial, epoch)


def test_train_model_still_refuses_a_dataset_that_is_neither_pointwise_nor_ranking():
    from deeprecommendation_amd.neural_collaborative_filtering.train import train_model
    with pytest.raises(NotImplementedError):
        train_model(torch.nn.Linear(1, 1), object(), object(), 1e-3, 0, 8, 8, False, device="cpu")


# ------------------------------------------------------------------ the pair-wise step, torch ops, against the reference
def pairwise_step(name, device, indexed=False):
    """(model, out_pos, out_neg, loss) after one BPR step through the ranking datasets' do_forward."""
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import BPR_loss
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    state, a, kw = load_golden(name)
    m = {"g9_bpr_basic": BasicNCF, "g9_bpr_mf": MF, "g9_bpr_att": AttentionNCF}[name](**kw)
    m.load_state_dict(state)
    m = m.to(device).train()
    if name == "g9_bpr_att":
        batch = (None, None, *(torch.from_numpy(a[k]) for k in ("candidate_items1", "rated_items", "user_matrix", "candidate_items2")))
        out_pos, out_neg = DynamicRankingDataset.do_forward(m, batch, device)
    else:
        cols = (a["user_pos"], a["pos_pos"], a["neg_pos"])
        dims = (kw["user_dim"], kw["item_dim"], kw["item_dim"])
        batch = tuple(torch.as_tensor(c) if indexed else onehot(c, d) for c, d in zip(cols, dims))
        out_pos, out_neg = FixedRankingDataset.do_forward(m, batch, device)
    loss = BPR_loss(out_pos, out_neg)
    loss.backward()
    return m, out_pos, out_neg, loss, a


def compare_with_reference(m, out_pos, out_neg, loss, a, tag, rtol=1e-5):
    """Outputs and loss within 1e-5 relative.  Each gradient within 1e-5 of the largest magnitude of the two calls' shares of it
    (``s::``, make_golden_bpr.py): a BPR gradient is the positive call's share minus the negative call's, and where the two cancel
    the rounding of either is not small against the result — the reference's own fp32 gradient of the last Linear of g9_bpr_basic
    is 1.5e-5 of its largest element away from the float64 value, and the last bias's gradient is 0 by construction (rounding
    noise in the reference)."""
    from conftest import record_error
    for got, key in ((out_pos, "out_pos"), (out_neg, "out_neg")):
        ref = torch.from_numpy(a[key]).double()
        err = float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())
        record_error(f"{tag}:{key}", err, rtol)
        assert err <= rtol, f"{key}: {err:.3e}"
    el = abs(float(loss.detach()) - float(a["loss"])) / abs(float(a["loss"]))
    record_error(tag + ":loss", el, rtol)
    assert el <= rtol
    named = dict(m.named_parameters())
    assert set(named) == set(a["grads"])
    worst = 0.0
    noise = 1e-8 * abs(float(a["loss"]))
    for k, g in a["grads"].items():
        got = named[k].grad
        assert got is not None and got.shape == g.shape, k
        scale = float(np.abs(a["s::" + k]).max())
        e = float((got.detach().cpu().double() - g.double()).abs().max())
        if scale <= noise:
            # zero by construction even per call — AttentionNet's output bias: a shift of all scores cancels in the softmax — the
            # reference's autograd leaves rounding noise, the HIP backward an exact 0: both inside the noise floor, as in
            # test_reference_gradients._compare
            assert e <= noise and float(got.abs().max()) <= noise, k
            continue
        worst = max(worst, e / scale)
        assert e <= rtol * scale, f"{k}: max abs err {e:.3e} vs largest share {scale:.3e}"
    record_error(tag + ":grads", worst, rtol)


@pytest.mark.parametrize("name", ["g9_bpr_basic", "g9_bpr_mf", "g9_bpr_att"])
def test_pairwise_step_torch_path_vs_reference(name):
    m, out_pos, out_neg, loss, a = pairwise_step(name, torch.device("cpu"))
    compare_with_reference(m, out_pos, out_neg, loss, a, f"cpu:{name}")
