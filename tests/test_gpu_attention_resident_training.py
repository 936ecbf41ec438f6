"""GPU: AttentionNCF training on device-built batches (train_model(..., resident=True) for DynamicPointwiseDataset and
DynamicRankingDataset): the resident batch against the host collate, the on-stream per-pair CSR + target mask (native.pair_rows)
against the reference's own training numbers (g3_att_train_*), one step and whole epochs against the DataLoader loop, no host read
inside a step, the defaults, the flag checks and the torch fallback.  Toy data as in test_train_model_ranking_dynamic."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden, record_error
from test_gpu_bpr_training import _toy_ranking
from test_reference_gradients import ATT_CASES, _compare

pytestmark = pytest.mark.gpu

U, I, F = 120, 60, 24


def _toy(seed=5, one_negative=True):
    """(provider, ranking frame, point-wise training frame, validation frame)."""
    from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider
    ranking, val, inter = _toy_ranking(U, I, seed=seed, one_negative=one_negative)
    rng = np.random.default_rng(6)
    feats = (rng.random((I, F)) < 0.2).astype(np.float32) + np.eye(I, F, dtype=np.float32)
    by_user = {u: g for u, g in inter.groupby("userId")}
    users = np.arange(1, U + 1)
    prov = SparseDynamicProvider(np.arange(1, I + 1), feats, users, [np.sort(by_user[u].movieId.to_numpy()) for u in users],
                                 [by_user[u].sort_values("movieId").rating.to_numpy() for u in users],
                                 [by_user[u].rating.mean() for u in users])
    merged = inter.merge(val[["userId", "movieId"]], on=["userId", "movieId"], how="left", indicator=True)
    point = merged[merged["_merge"] == "left_only"].drop(columns="_merge").reset_index(drop=True)
    return prov, ranking, point, val


def _model(seed=7, **kw):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.manual_seed(seed)
    return AttentionNCF(item_dim=F, item_emb=32, user_emb=32, att_dense=16, mlp_dense_layers=[64], dropout_rate=0.0, **kw)


def _datasets(prov, ranking, point):
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset, DynamicRankingDataset
    return DynamicPointwiseDataset(point, prov), DynamicRankingDataset(ranking, prov)


def _resident_point_batch(ds, gpu, s, e, bs=128):
    res = ds.resident_inputs(gpu, bs)
    dev = [t.to(gpu) for t in (*res.tensors, res.targets)]
    inputs = res.train_on_chunk(*dev[:-1])
    return res.train_on_batch(*[t[s:e] for t in inputs], dev[-1][s:e])


def _dense_over(ratings, positions):
    """The batch's CSR as the dense (B, len(positions)) matrix over the given catalogue positions, and what lies outside them."""
    dense = ratings.expanded().to_dense(ratings.expanded().val).cpu()
    keep = torch.zeros(dense.shape[1], dtype=torch.bool)
    keep[torch.as_tensor(positions)] = True
    return dense[:, torch.as_tensor(positions)], dense[:, ~keep]


# ------------------------------------------------------------------------------------------ 1. batches
def test_resident_batches_carry_the_host_collates_data(gpu):
    prov, ranking, point, _ = _toy()
    pds, rds = _datasets(prov, ranking, point)
    pairs = rds.resident_pairs(gpu)
    assert pairs is not None
    for s in (0, 128, len(pds) - 50):
        e = min(s + 128, len(pds))
        host = pds.use_collate()([pds[k] for k in range(s, e)])
        dev = _resident_point_batch(pds, gpu, s, e)
        pos = np.searchsorted(prov.item_ids, host[1])
        inside, outside = _dense_over(dev[4], pos)
        assert torch.equal(inside, host[4].to_dense(host[4].val)) and not bool(outside.any())
        assert torch.equal(dev[2].materialise().cpu(), host[2]) and torch.equal(dev[5].cpu(), host[5])
        assert dev[3] is prov.device_state(gpu).features and dev[4].max_row_len == prov.device_state(gpu).max_row_len
    for s in (0, 128):
        e = min(s + 128, len(rds))
        host = rds.use_collate()([rds[k] for k in range(s, e)])                 # one negative per row: the draw is forced
        dev = pairs.batch(torch.arange(s, e, device=gpu), 3, s)
        pos = np.searchsorted(prov.item_ids, host[1])
        inside, outside = _dense_over(dev[4], pos)
        assert torch.equal(inside, host[4].to_dense(host[4].val)) and not bool(outside.any())
        assert torch.equal(dev[2].materialise().cpu(), host[2]) and torch.equal(dev[5].materialise().cpu(), host[5])
    pairs.check()


# ------------------------------------------------------------------------------------------ 2. reference pin
@pytest.mark.parametrize("name", ATT_CASES)
def test_on_stream_route_vs_reference_training_numbers(gpu, name, monkeypatch):
    """g3_att_train_* with user_matrix as a shared-row CSR made by hand (rows from torch.unique(dim=0)), max_row_len set: the
    per-pair CSR and the target mask come from native.pair_rows; out, loss and every gradient against the reference's own, and the
    attention weights rebuilt from the returned columns — the masked entries are exactly self_cols."""
    from deeprecommendation_amd import native
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF, SparseRatings
    state, a, kw = load_golden(name)
    m = AttentionNCF(**kw)
    m.load_state_dict(state)
    m = m.to(gpu).train()
    um = torch.from_numpy(a["user_matrix"])
    rows, inv = torch.unique(um, dim=0, return_inverse=True)
    nz = [torch.nonzero(r).view(-1) for r in rows]
    rowptr = torch.zeros(len(nz) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(x) for x in nz]), 0)
    col = torch.cat(nz).to(torch.int32)
    val = torch.cat([r[x] for r, x in zip(rows, nz)]).float()
    ratings = SparseRatings(rowptr.to(gpu), col.to(gpu), val.to(gpu), um.shape[1], pair_row=inv.to(gpu),
                            max_row_len=max(len(x) for x in nz))
    seen = {}
    real_pair_rows, real_attn = native.pair_rows, native.attn_forward

    def spy_pair_rows(*args, **kwargs):
        seen["csr"] = real_pair_rows(*args, **kwargs)
        return seen["csr"]

    def spy_attn(*args, **kwargs):
        res = real_attn(*args, **kwargs)
        seen["wts"] = res[1]
        return res

    monkeypatch.setattr(native, "pair_rows", spy_pair_rows)
    monkeypatch.setattr(native, "attn_forward", spy_attn)
    cand, rated = (torch.from_numpy(a[k]).to(gpu) for k in ("candidate_items", "rated_items"))
    out = m(cand, rated, ratings)
    loss = torch.nn.MSELoss(reduction="sum")(out, torch.from_numpy(a["y"]).to(gpu).view(-1, 1).float())
    loss.backward()
    if name == "g3_att_train_ue50":                       # user_emb = 50: no attention backward kernel — the torch fallback, no pair_rows
        assert "csr" not in seen
        _compare(m, a, out, None, loss, f"stream:{name}")
        return
    r, c, v, _ = (t.cpu().numpy() for t in seen["csr"])
    wts = seen["wts"].cpu().numpy()
    rowptr_n, col_n, val_n, inv_n = rowptr.numpy(), col.numpy(), val.numpy(), inv.numpy()
    att = torch.zeros_like(um)
    masked = set()
    for b in range(um.shape[0]):
        src, n = rowptr_n[inv_n[b]], int(r[b + 1] - r[b])
        orig, got = col_n[src:src + n], c[r[b]:r[b] + n]
        assert n == rowptr_n[inv_n[b] + 1] - src and np.array_equal(v[r[b]:r[b] + n], val_n[src:src + n])
        assert np.array_equal(got[got != -1], orig[got != -1])
        att[b, torch.from_numpy(orig.astype(np.int64))] = torch.from_numpy(wts[r[b]:r[b] + n])
        masked |= {(b, int(x)) for x in orig[got == -1]}
    _compare(m, a, out, att, loss, f"stream:{name}")
    want = {(b, int(s)) for b, s in enumerate(a["self_cols"]) if um[b, int(s)] != 0}
    assert masked == want and len(want) > 0
    native.check_pair_rows(gpu)


# ------------------------------------------------------------------------------------------ 3. one step
def _grads_within(m_got, m_ref, loss_ref, tag, rtol=1e-5):
    """test_reference_gradients._compare's bars: 1e-5 of the largest element per tensor, the 1e-8-of-loss noise floor."""
    noise = 1e-8 * abs(float(loss_ref.detach()))
    worst = 0.0
    for (k, p), (_, q) in zip(m_got.named_parameters(), m_ref.named_parameters()):
        g, ref = p.grad.detach().cpu().double(), q.grad.detach().cpu().double()
        scale, e = float(ref.abs().max()), float((g - ref).abs().max())
        if scale <= noise:
            assert e <= noise, k
            continue
        worst = max(worst, e / scale)
        assert e <= rtol * scale, f"{k}: max abs err {e:.3e} vs largest reference element {scale:.3e}"
    record_error(tag + ":grads", worst, rtol)


def _close(got, ref, tag, rtol=1e-5):
    err = float((got.detach().double() - ref.detach().double()).abs().max() / ref.detach().double().abs().max())
    record_error(tag, err, rtol)
    assert err <= rtol, f"{tag}: {err:.3e}"


def test_one_pointwise_step_resident_batch_vs_host_collate(gpu):
    from deeprecommendation_amd import native
    prov, ranking, point, _ = _toy()
    pds, _ = _datasets(prov, ranking, point)
    assert native.attn_backward_supported(native.ATT_MLP, 16, 32)
    m_host = _model().to(gpu).train()
    m_dev = copy.deepcopy(m_host)
    host = pds.use_collate()([pds[k] for k in range(128)])
    out_h, y_h = type(pds).do_forward(m_host, host, gpu)
    loss_h = pds.calculate_loss(out_h, y_h.to(gpu))
    loss_h.backward()
    out_d, y_d = type(pds).do_forward(m_dev, _resident_point_batch(pds, gpu, 0, 128), gpu)
    loss_d = pds.calculate_loss(out_d, y_d)
    loss_d.backward()
    _close(out_d, out_h, "point:out")
    _close(loss_d, loss_h, "point:loss")
    _grads_within(m_dev, m_host, loss_h, "point")
    native.check_pair_rows(gpu)


def test_one_pairwise_step_resident_batch_vs_host_collate_and_one_forward_vs_two(gpu):
    from deeprecommendation_amd import native
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import _dev
    prov, ranking, point, _ = _toy()
    _, rds = _datasets(prov, ranking, point)
    m_host = _model().to(gpu).train()
    m_dev, m_two = copy.deepcopy(m_host), copy.deepcopy(m_host)
    host = rds.use_collate()([rds[k] for k in range(128)])
    pos_h, neg_h = type(rds).do_forward(m_host, host, gpu)                     # the host tuple keeps its two calls
    loss_h = rds.calculate_loss(pos_h, neg_h)
    loss_h.backward()
    batch = rds.resident_pairs(gpu).batch(torch.arange(128, device=gpu), 3, 0)
    pos_d, neg_d = type(rds).do_forward(m_dev, batch, gpu)                     # one forward of 2B pairs
    loss_d = rds.calculate_loss(pos_d, neg_d)
    loss_d.backward()
    assert pos_d.shape == neg_d.shape == (128, 1)
    for tag, got, ref in (("pair:pos", pos_d, pos_h), ("pair:neg", neg_d, neg_h), ("pair:loss", loss_d, loss_h)):
        _close(got, ref, tag)
    _grads_within(m_dev, m_host, loss_h, "pair")
    # the same device-built batch through two forwards
    pos_t = m_two(batch[2].float().to(gpu), batch[3], _dev(batch[4], gpu))
    neg_t = m_two(batch[5].float().to(gpu), batch[3], _dev(batch[4], gpu))
    loss_t = rds.calculate_loss(pos_t, neg_t)
    loss_t.backward()
    for tag, got, ref in (("2B:pos", pos_d, pos_t), ("2B:neg", neg_d, neg_t), ("2B:loss", loss_d, loss_t)):
        _close(got, ref, tag)
    _grads_within(m_dev, m_two, loss_t, "2B")
    native.check_pair_rows(gpu)


# ------------------------------------------------------------------------------------------ 4. epochs
def _train(make_ds, val_ds, gpu, tmp_path, resident, epochs=2, model=None, lr=2e-3):
    from deeprecommendation_amd.neural_collaborative_filtering.train import train_model
    m = model if model is not None else _model()
    np.random.seed(1)
    torch.manual_seed(11)
    mm = train_model(m, make_ds(), val_ds, lr=lr, weight_decay=0.0, batch_size=128, val_batch_size=256, early_stop=False,
                     final_model_path=None, checkpoint_model_path=str(tmp_path / "c.pt"), max_epochs=epochs, device=gpu, resident=resident,
                     shuffle=False, verbose=False)
    return mm, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("pairwise", [False, True])
def test_resident_and_dataloader_epochs_agree(gpu, tmp_path, pairwise):
    """2 epochs, shuffling off, one negative per row: train_model(resident=True) against the DataLoader loop.  The attention backward
    adds with float atomics, so the DataLoader loop does not reproduce itself bit for bit: it is run twice with equal seeds first and
    the bar is the larger of the index-dataset test's bars (rtol 2e-4 on epoch losses, 1e-4 of max|w| on final weights) and 4x that
    spread (4x: the extra summation-order differences the whole-catalogue rated list brings to the Linear weight gradients).
    Measured on an MI355X — DataLoader self-spread: epoch losses 0 (equal to the last bit) point- and pair-wise, final weights
    2.9e-7 (point-wise) and 2.1e-7 (pair-wise) of the largest element; resident against DataLoader: losses 0, weights 2.9e-7 and
    2.1e-7.  4x the spread is 1.2e-6 at most, so the bars in force are the index-dataset test's 2e-4 and 1e-4."""
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset
    prov, ranking, point, val = _toy()
    make = (lambda: _datasets(prov, ranking, point)[1]) if pairwise else (lambda: _datasets(prov, ranking, point)[0])
    val_ds = DynamicPointwiseDataset(val, prov)
    (la, wa), (lb, wb) = _train(make, val_ds, gpu, tmp_path, False), _train(make, val_ds, gpu, tmp_path, False)
    loss_spread = max(abs(x - y) / abs(y) for x, y in zip(la["train_loss"], lb["train_loss"]))
    w_spread = max(float((wa[k] - wb[k]).abs().max()) / (float(wb[k].abs().max()) + 1e-6) for k in wa)
    loss_bar, w_bar = max(2e-4, 4 * loss_spread), max(1e-4, 4 * w_spread)
    lr_, wr = _train(make, val_ds, gpu, tmp_path, True)
    loss_err = max(abs(x - y) / abs(y) for x, y in zip(lr_["train_loss"], lb["train_loss"]))
    per_key = {k: float((wr[k] - wb[k]).abs().max()) / (float(wb[k].abs().max()) + 1e-6) for k in wb}
    worst = max(per_key, key=per_key.get)
    w_err = per_key[worst]
    print(f"\n[epochs pairwise={pairwise}] DataLoader self-spread: loss {loss_spread:.3e}, weights {w_spread:.3e}; "
          f"resident vs DataLoader: loss {loss_err:.3e} (bar {loss_bar:.3e}), weights {w_err:.3e} in {worst} (bar {w_bar:.3e})")
    record_error(f"epochs:{'pair' if pairwise else 'point'}:loss", loss_err, loss_bar)
    record_error(f"epochs:{'pair' if pairwise else 'point'}:weights", w_err, w_bar)
    assert len(lr_["train_loss"]) == 2 and lr_["val_ndcg"] and all(np.isfinite(lr_["train_loss"]))
    assert loss_err <= loss_bar
    assert w_err <= w_bar, worst


# ------------------------------------------------------------------------------------------ 5. no host read
@pytest.mark.parametrize("pairwise", [False, True])
def test_resident_attention_steps_do_not_synchronise(gpu, pairwise):
    from deeprecommendation_amd import native
    from deeprecommendation_amd.optim import FusedAdam
    prov, ranking, point, _ = _toy(one_negative=False)
    pds, rds = _datasets(prov, ranking, point)
    ds = rds if pairwise else pds
    m = _model().to(gpu).train()
    opt = FusedAdam(m.parameters(), lr=1e-3)
    if pairwise:
        pairs = ds.resident_pairs(gpu)
        make = lambda pick, s: pairs.batch(pick, 2, s)
    else:
        res = ds.resident_inputs(gpu, 128)
        dev = [t.to(gpu) for t in (*res.tensors, res.targets)]
        inputs = res.train_on_chunk(*dev[:-1])
        make = lambda pick, s: res.train_on_batch(*[t[pick] for t in inputs], dev[-1][pick])

    def step(pick, s):
        opt.zero_grad()
        a, b = type(ds).do_forward(m, make(pick, s), gpu)
        loss = ds.calculate_loss(a, b)
        loss.backward()
        opt.step()
        return loss.detach()

    order = torch.randperm(len(ds), device=gpu)
    step(order[:128], 0)                                      # warm-up: allocator, optimiser state, library load, the sticky flags
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [step(order[s:s + 128], s) for s in range(0, len(ds), 128)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(losses) >= 3 and all(bool(torch.isfinite(l)) for l in losses)
    native.check_oob(gpu)
    native.check_pair_rows(gpu)


# ------------------------------------------------------------------------------------------ 6. defaults
@pytest.mark.parametrize("pairwise", [False, True])
def test_resident_none_keeps_the_collate_and_resident_true_never_calls_it(gpu, tmp_path, pairwise, monkeypatch):
    from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset
    prov, ranking, point, val = _toy()
    calls = []
    real = SparseDynamicProvider.collate_interacted_items

    def counting(self, batch, for_ranking, **kw):
        calls.append(for_ranking)
        return real(self, batch, for_ranking, **kw)

    monkeypatch.setattr(SparseDynamicProvider, "collate_interacted_items", counting)
    make = (lambda: _datasets(prov, ranking, point)[1]) if pairwise else (lambda: _datasets(prov, ranking, point)[0])
    n = len(make())
    val_ds = DynamicPointwiseDataset(val, prov)
    _train(make, val_ds, gpu, tmp_path, None, epochs=1)
    assert calls.count(pairwise) >= -(-n // 128) and (pairwise or True not in calls)
    calls.clear()
    _train(make, val_ds, gpu, tmp_path, True, epochs=1)
    assert calls == []                                         # neither the training epoch nor the validation pass
    with pytest.raises(ValueError, match="resident training"):
        _train(make, val_ds, torch.device("cpu"), tmp_path, True, epochs=1)


# ------------------------------------------------------------------------------------------ 7. unknown id, overflow
def test_unknown_negative_id_raises_index_error_at_the_end_of_the_epoch(gpu, tmp_path):
    from deeprecommendation_amd import native
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset
    prov, ranking, point, val = _toy()
    ranking.at[3, "negative_movieIds"] = [I + 500]            # an id the provider does not know
    try:
        with pytest.raises(IndexError):
            _train(lambda: _datasets(prov, ranking, point)[1], DynamicPointwiseDataset(val, prov), gpu, tmp_path, True, epochs=1)
    finally:
        native._oob_flag(gpu).zero_()


def test_a_row_longer_than_max_row_len_raises_overflow_error_at_the_end_of_the_epoch(gpu, tmp_path):
    from deeprecommendation_amd import native
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset
    prov, ranking, point, val = _toy()
    prov.device_state(gpu).max_row_len = 3                    # every user rated 12 items
    try:
        with pytest.raises(OverflowError):
            _train(lambda: _datasets(prov, ranking, point)[0], DynamicPointwiseDataset(val, prov), gpu, tmp_path, True, epochs=1)
    finally:
        native._pair_rows_flag(gpu).zero_()


# ------------------------------------------------------------------------------------------ 8. torch fallback
def test_message_dropout_model_trains_resident_through_the_torch_fallback(gpu, tmp_path, monkeypatch):
    from deeprecommendation_amd import native
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset
    prov, ranking, point, val = _toy()
    called = []
    real = native.pair_rows
    monkeypatch.setattr(native, "pair_rows", lambda *a, **k: (called.append(1), real(*a, **k))[1])
    for make in ((lambda: _datasets(prov, ranking, point)[0]), (lambda: _datasets(prov, ranking, point)[1])):
        mm, _ = _train(make, DynamicPointwiseDataset(val, prov), gpu, tmp_path, True, epochs=3, model=_model(message_dropout=0.1), lr=5e-3)
        assert all(np.isfinite(mm["train_loss"])) and mm["train_loss"][-1] < mm["train_loss"][0]
    assert called == []                                        # message dropout: the torch ops of _forward_train, as before
