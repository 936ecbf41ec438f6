"""GPU tests of pair-wise (BPR) training: the pair-wise step on the HIP autograd blocks against the reference's own numbers
(g9_bpr_*), GraphNCF's pair-wise HIP step against its CPU torch-op path, and train_model's ranking branch (reference
train.py:79-210) with device-resident negative sampling."""
import copy

import numpy as np
import pandas as pd
import pytest
import torch

from test_ranking_cpu import compare_with_reference, pairwise_step

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,indexed", [("g9_bpr_basic", True), ("g9_bpr_basic", False), ("g9_bpr_mf", True), ("g9_bpr_mf", False),
                                          ("g9_bpr_att", False)])
def test_pairwise_step_hip_blocks_vs_reference(gpu, name, indexed):
    m, out_pos, out_neg, loss, a = pairwise_step(name, gpu, indexed)
    compare_with_reference(m, out_pos, out_neg, loss, a, f"hip:{name}:{'idx' if indexed else 'onehot'}")
    if name == "g9_bpr_att":
        assert (a["pos_col"] >= 0).sum() >= 8          # candidates that are rated rows: the target mask acted


def test_graph_pairwise_hip_step_equals_cpu_torch_path(gpu):
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import BPR_loss
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.gnn_datasets import GraphRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphData, GraphNCF
    from test_gpu_training import _grads_close, _train_graph
    n_items, n_users, B = 40, 300, 256
    u2i, i2u, a = _train_graph(n_items, n_users, 4000, seed=3)
    torch.manual_seed(5)
    m_cpu = GraphNCF(item_dim=n_items, user_dim=n_users, num_gnn_layers=2, hetero=False, node_emb=64, mlp_dense_layers=[128],
                     dropout_rate=0.0).train()
    m_gpu = copy.deepcopy(m_cpu).to(gpu).train()
    g = torch.Generator().manual_seed(6)
    pick = torch.randint(0, u2i.shape[1], (B,), generator=g)         # positives and negatives ARE edges: both calls mask theirs
    users, pos = u2i[0][pick], u2i[1][pick]
    neg = u2i[1][torch.randint(0, u2i.shape[1], (B,), generator=g)]

    def graph(dev):
        return GraphData(user2item_edge_index=u2i.to(dev), item2user_edge_index=i2u.to(dev), user2item_edge_attr=a.to(dev),
                         item2user_edge_attr=a.clone().to(dev), num_items=n_items, num_users=n_users)

    losses = []
    for m, dev in ((m_cpu, torch.device("cpu")), (m_gpu, gpu)):
        out_pos, out_neg = GraphRankingDataset.do_forward(m, (users, pos, neg), dev, graph(dev))
        loss = BPR_loss(out_pos, out_neg)
        loss.backward()
        losses.append(float(loss.detach()))
    assert abs(losses[1] - losses[0]) <= 2e-5 * abs(losses[0])
    _grads_close(m_gpu, m_cpu, rtol=5e-5)


# ------------------------------------------------------------------------------------------ train_model, ranking branch
def _toy_ranking(n_users=120, n_items=60, seed=0, one_negative=False):
    """Point-wise interactions with a learnable structure, and the ranking file the reference's notebook makes from them:
    per (user, positive) every item the user rated lower (one of them with ``one_negative``)."""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(1, n_users + 1):
        items = rng.choice(np.arange(1, n_items + 1), 12, replace=False)
        r = np.clip(np.round(((u % 5) + (items % 3)) * 0.5 + 1 + rng.normal(0, 0.3, len(items)), 0) / 1.0, 0.5, 5.0)
        rows += [(u, int(i), float(x)) for i, x in zip(items, r)]
    inter = pd.DataFrame(rows, columns=["userId", "movieId", "rating"])
    train_rows, val_rows = [], []
    for u, grp in inter.groupby("userId"):
        grp = grp.sample(frac=1.0, random_state=int(u))
        val_rows.append(grp.iloc[:4])
        tr = grp.iloc[4:]
        for _, p in tr.iterrows():
            lower = tr[tr.rating < p.rating]
            if len(lower):
                if one_negative:
                    lower = lower.iloc[:1]
                train_rows.append((u, int(p.movieId), lower.movieId.astype(np.int64).tolist(), lower.rating.tolist()))
    ranking = pd.DataFrame(train_rows, columns=["userId", "positive_movieId", "negative_movieIds", "negative_ratings"])
    return ranking, pd.concat(val_rows).reset_index(drop=True), inter


class _WandbStub:
    def __init__(self):
        self.logs = []

    def log(self, d):
        self.logs.append(dict(d))


def _basic_model(n_users, n_items, seed=0):
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    torch.manual_seed(seed)
    return BasicNCF(item_dim=n_items, user_dim=n_users, item_emb=64, user_emb=64, mlp_dense_layers=[128], dropout_rate=0.0)


def test_resident_and_dataloader_ranking_epochs_agree_with_one_negative_per_row(gpu, tmp_path):
    """Every row has one negative, shuffling off: the device-resident epoch (ids and negatives uploaded once, negatives drawn on
    the device) and the DataLoader epoch see the same batches: the same epoch losses and final weights (BasicNCF, GraphNCF)."""
    from deeprecommendation_amd.content_providers.index_providers import IndexGraphProvider, IndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset, FixedRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.gnn_datasets import GraphPointwiseDataset, GraphRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF
    from deeprecommendation_amd.neural_collaborative_filtering.train import train_model
    U, I = 120, 60
    ranking, val, inter = _toy_ranking(U, I, seed=1, one_negative=True)
    prov = IndexProvider(np.arange(1, U + 1), np.arange(1, I + 1))
    gcp = IndexGraphProvider(np.arange(1, U + 1), np.arange(1, I + 1), inter.userId, inter.movieId, inter.rating)
    cases = [(lambda: _basic_model(U, I), lambda: FixedRankingDataset(ranking, prov), lambda: FixedPointwiseDataset(val, prov)),
             (lambda: (torch.manual_seed(0), GraphNCF(item_dim=I, user_dim=U, num_gnn_layers=2, hetero=False, node_emb=64,
                                                      mlp_dense_layers=[128], dropout_rate=0.0))[1],
              lambda: GraphRankingDataset(ranking, gcp), lambda: GraphPointwiseDataset(val, gcp))]
    for make_model, make_train, make_val in cases:
        res = {}
        for resident in (True, False):
            m = make_model()
            mm = train_model(m, make_train(), make_val(), lr=2e-3, weight_decay=0.0, batch_size=128, val_batch_size=256, early_stop=False,
                             final_model_path=None, checkpoint_model_path=str(tmp_path / "c.pt"), max_epochs=3, device=gpu,
                             resident=resident, shuffle=False, verbose=False)
            res[resident] = (mm, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        (a, wa), (b, wb) = res[True], res[False]
        np.testing.assert_allclose(a["train_loss"], b["train_loss"], rtol=2e-4)
        assert a["val_loss"] == b["val_loss"] == []
        for k in wa:
            assert float((wa[k] - wb[k]).abs().max()) <= 1e-4 * (float(wb[k].abs().max()) + 1e-6), k


def _train_and_check(model, train_ds, val_ds, gpu, tmp_path, resident, model_cls, epochs=6):
    from deeprecommendation_amd.neural_collaborative_filtering.eval import eval_model
    from deeprecommendation_amd.neural_collaborative_filtering.train import schedule_w, train_model
    from deeprecommendation_amd.neural_collaborative_filtering.util import load_model
    model = model.to(gpu)
    ndcg0 = eval_model(model, val_ds, 256, ranking=True, device=gpu, cutoffs=(10,))["ndcg@10"]
    stub = _WandbStub()
    mm = train_model(model, train_ds, val_ds, lr=5e-3, weight_decay=0.0, batch_size=128, val_batch_size=256, early_stop=True,
                     final_model_path=str(tmp_path / "final.pt"), checkpoint_model_path=str(tmp_path / "ckpt.pt"), max_epochs=epochs,
                     patience=10, max_patience=10, wandb=stub, device=gpu, resident=resident, verbose=False)
    assert mm["val_loss"] == [] and len(mm["train_loss"]) == len(mm["val_ndcg"]) == epochs
    assert mm["train_loss"][-1] < mm["train_loss"][0]
    assert max(mm["val_ndcg"]) > ndcg0
    per_epoch = [d for d in stub.logs if "epoch" in d]
    assert [d["neg_sampling_w"] for d in per_epoch] == [schedule_w(e) for e in range(1, epochs + 1)]
    assert all("val_loss" not in d for d in stub.logs) and "best_val_loss" not in stub.logs[-1]
    reloaded = load_model(str(tmp_path / "final.pt"), model_cls).to(gpu)
    got = eval_model(reloaded, val_ds, 256, ranking=True, device=gpu, cutoffs=(10,))["ndcg@10"]
    assert abs(got - max(mm["val_ndcg"])) <= 1e-9


def test_train_model_ranking_fixed_resident_and_dataloader(gpu, tmp_path):
    from deeprecommendation_amd.content_providers.index_providers import IndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset, FixedRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    U, I = 120, 60
    ranking, val, _ = _toy_ranking(U, I, seed=2)
    prov = IndexProvider(np.arange(1, U + 1), np.arange(1, I + 1))
    for resident in (True, False):
        train_ds = FixedRankingDataset(ranking, prov)
        assert (train_ds.resident_pairs(gpu) is not None) == True   # noqa: E712  (index provider: the resident path exists)
        np.random.seed(0)
        _train_and_check(_basic_model(U, I, seed=3), train_ds, FixedPointwiseDataset(val, prov), gpu, tmp_path, resident, BasicNCF)


def test_train_model_ranking_graph(gpu, tmp_path):
    from deeprecommendation_amd.content_providers.index_providers import IndexGraphProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.gnn_datasets import GraphPointwiseDataset, GraphRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF
    U, I = 120, 60
    ranking, val, inter = _toy_ranking(U, I, seed=4)
    gcp = IndexGraphProvider(np.arange(1, U + 1), np.arange(1, I + 1), inter.userId, inter.movieId, inter.rating)
    torch.manual_seed(4)
    m = GraphNCF(item_dim=I, user_dim=U, num_gnn_layers=2, hetero=False, node_emb=64, mlp_dense_layers=[128], dropout_rate=0.0)
    _train_and_check(m, GraphRankingDataset(ranking, gcp), GraphPointwiseDataset(val, gcp), gpu, tmp_path, None, GraphNCF)


def test_train_model_ranking_dynamic(gpu, tmp_path):
    from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset, DynamicRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    U, I, F = 120, 60, 24
    ranking, val, inter = _toy_ranking(U, I, seed=5)
    rng = np.random.default_rng(6)
    feats = (rng.random((I, F)) < 0.2).astype(np.float32) + np.eye(I, F, dtype=np.float32)
    by_user = {u: g for u, g in inter.groupby("userId")}
    users = np.arange(1, U + 1)
    prov = SparseDynamicProvider(np.arange(1, I + 1), feats, users, [np.sort(by_user[u].movieId.to_numpy()) for u in users],
                                 [by_user[u].sort_values("movieId").rating.to_numpy() for u in users],
                                 [by_user[u].rating.mean() for u in users])
    torch.manual_seed(7)
    m = AttentionNCF(item_dim=F, item_emb=32, user_emb=32, att_dense=16, mlp_dense_layers=[64], dropout_rate=0.0)
    np.random.seed(1)
    _train_and_check(m, DynamicRankingDataset(ranking, prov), DynamicPointwiseDataset(val, prov), gpu, tmp_path, None, AttentionNCF)


def test_resident_ranking_steps_do_not_synchronise(gpu):
    """The resident epoch's steps — gather, sample_negatives (CDF rebuilt on a new w), two forwards, BPR, backward, FusedAdam —
    enqueue without a host read."""
    from deeprecommendation_amd.content_providers.index_providers import IndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedRankingDataset
    from deeprecommendation_amd.optim import FusedAdam
    U, I = 120, 60
    ranking, _, _ = _toy_ranking(U, I, seed=7)
    ds = FixedRankingDataset(ranking, IndexProvider(np.arange(1, U + 1), np.arange(1, I + 1)))
    pairs = ds.resident_pairs(gpu)
    m = _basic_model(U, I).to(gpu).train()
    opt = FusedAdam(m.parameters(), lr=1e-3)

    def step(pick, seed, slot0):
        batch = pairs.batch(pick, seed, slot0)
        opt.zero_grad()
        out_pos, out_neg = FixedRankingDataset.do_forward(m, batch, gpu)
        loss = ds.calculate_loss(out_pos, out_neg)
        loss.backward()
        opt.step()
        return loss.detach()

    order = torch.randperm(len(ds), device=gpu)
    step(order[:128], 1, 0)                                   # warm-up: allocator, optimiser state, library load
    torch.cuda.synchronize()
    ds.w = 1.5                                                # the next draw rebuilds the CDF, inside the checked window
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [step(order[s:s + 128], 2, s) for s in range(0, len(ds), 128)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert pairs.sampler.cdf_w == 1.5
    assert all(bool(torch.isfinite(l)) for l in losses)
    pairs.check()


def test_unknown_negative_id_raises_index_error_at_the_end_of_the_epoch(gpu, tmp_path):
    from deeprecommendation_amd.content_providers.index_providers import IndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset, FixedRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.train import train_model
    U, I = 120, 60
    ranking, val, _ = _toy_ranking(U, I, seed=8, one_negative=True)
    ranking.at[3, "negative_movieIds"] = [I + 500]            # an id the provider does not know
    prov = IndexProvider(np.arange(1, U + 1), np.arange(1, I + 1))
    with pytest.raises(IndexError):
        train_model(_basic_model(U, I), FixedRankingDataset(ranking, prov), FixedPointwiseDataset(val, prov), lr=1e-3, weight_decay=0.0,
                    batch_size=128, val_batch_size=256, early_stop=False, final_model_path=None,
                    checkpoint_model_path=str(tmp_path / "c.pt"), max_epochs=1, device=gpu, resident=True, verbose=False)
