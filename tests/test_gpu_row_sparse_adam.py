"""GPU tests of row-sparse Adam: the ncf_adam_rows kernels (grouping, run sums, the 16-byte and the scalar path, long runs, ids out
of range) against the float64 oracle row_adam_ref, bit for bit against the dense ncf_adam_step where every row is touched once,
and optim.RowSparseAdam on BasicNCF / MF / a pair-wise (BPR) epoch.

The "Adam bar" is the one of test_fused_adam_matches_torch_adam: |x - ref| <= 2e-6 * max|ref| + 1e-7, here for p, m and v.  Both
sides get float32-representable hyper-parameters (row_adam_ref.f32), the kernel's argument type."""
import numpy as np
import pytest
import torch

from row_adam_ref import f32, row_adam_ref

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = f32(3e-3), f32(0.9), f32(0.999), f32(1e-8)
ROWS = 300


def _adam_bar(got, ref, what):
    got = got.detach().cpu().double().numpy()
    err, bar = float(np.abs(got - ref).max()), 2e-6 * float(np.abs(ref).max()) + 1e-7
    assert err <= bar, f"{what}: max error {err:.3e} > {bar:.3e}"


def _guarded(rows, E, gpu, gen):
    """(p, m, v) as [rows, E] views 64 floats into three flat buffers, with the buffers themselves: the 64 floats on either side
    are guards (NaN-free random values that no kernel may change)."""
    bufs = [torch.randn(64 + rows * E + 64, generator=gen) for _ in range(3)]
    bufs[1].mul_(0.1)
    bufs[2].abs_().mul_(0.01)
    bufs = [b.to(gpu) for b in bufs]
    return [b[64:64 + rows * E].view(rows, E) for b in bufs], bufs


def _guards(bufs):
    return [torch.cat((b[:64], b[-64:])).clone() for b in bufs]


def _quantised(n, E, gen):
    """Multiples of 2^-10 in [-4, 4]: a sum of up to 2^11 of them is exact in fp32 in any order."""
    return torch.randint(-4096, 4097, (n, E), generator=gen).float() / 1024.0


def _batch_ids(n, gen, rows=ROWS, hot=True):
    pool = torch.randperm(rows, generator=gen)[:41]
    ids = pool[torch.randint(0, 40, (n,), generator=gen)]
    if hot and n >= 64:
        ids[torch.randperm(n, generator=gen)[:n // 2]] = pool[40]       # one id fills half the batch
    return ids


def _step_and_check(native, state, ids, g_dev, g_host, wd, step, what):
    """One native.adam_rows_ call on the device state against the oracle on its host copy; untouched rows bit for bit."""
    before = [x.clone() for x in state]
    host = [x.cpu().double().numpy() for x in state]
    native.adam_rows_(*state, ids.to(g_dev.device), g_dev, LR, B1, B2, EPS, wd, step)
    ref = row_adam_ref(*host, ids.numpy(), g_host.double().numpy(), LR, B1, B2, EPS, wd, step)
    touched = torch.zeros(state[0].shape[0], dtype=torch.bool)
    inside = ids[(ids >= 0) & (ids < state[0].shape[0])]
    touched[inside] = True
    for x, x0, r, name in zip(state, before, ref, "pmv"):
        _adam_bar(x, r, f"{what} {name} step {step}")
        assert torch.equal(x[~touched.to(x.device)], x0[~touched.to(x.device)]), f"{what}: an untouched row of {name} changed"
    if inside.numel():
        assert not torch.equal(state[0][touched.to(g_dev.device)], before[0][touched.to(g_dev.device)])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
@pytest.mark.parametrize("E", [64, 128, 7, 4])
def test_grouping_with_exact_sums(gpu, E, n):
    """Three consecutive steps with fresh batches (40 distinct ids and one id on half the batch): every run sum is exact, so p, m, v
    meet the Adam bar whatever order the kernel adds in, and rows outside the batch keep their bits.  E = 64 / 128 / 4 take the
    16-byte path (one and two chunks per lane, a partly idle group), E = 7 the scalar path; n = 4096 holds runs beyond 64 rows."""
    from deeprecommendation_amd import native
    gen = torch.Generator().manual_seed(1000 * E + n)
    state, bufs = _guarded(ROWS, E, gpu, gen)
    guards = _guards(bufs)
    for step in (1, 2, 3):
        ids, g = _batch_ids(n, gen), _quantised(n, E, gen)
        _step_and_check(native, state, ids, g.to(gpu), g, f32(1e-2), step, f"E={E} n={n}")
    assert all(torch.equal(a, b) for a, b in zip(_guards(bufs), guards))
    native.check_oob(gpu)


def test_strided_gradient_rows_and_the_empty_batch(gpu):
    """g as the right column half of a wider matrix (row stride 2E, as GatherColumnsConcatFn hands it over); n = 0 changes nothing."""
    from deeprecommendation_amd import native
    gen = torch.Generator().manual_seed(7)
    E, n = 64, 4096
    state, _ = _guarded(ROWS, E, gpu, gen)
    wide = _quantised(n, 2 * E, gen)
    ids = _batch_ids(n, gen)
    wide_dev = wide.to(gpu)
    assert wide_dev[:, E:].stride() == (2 * E, 1)
    _step_and_check(native, state, ids, wide_dev[:, E:], wide[:, E:], 0.0, 1, "strided g")
    before = [x.clone() for x in state]
    native.adam_rows_(*state, torch.empty(0, dtype=torch.int64, device=gpu), torch.empty((0, E), device=gpu), LR, B1, B2, EPS, 0.0, 2)
    assert all(torch.equal(a, b) for a, b in zip(state, before))
    # an odd row stride sends a 4-divisible width down the scalar path
    odd = _quantised(n, E + 1, gen)
    _step_and_check(native, state, ids, odd.to(gpu)[:, :E], odd[:, :E], 0.0, 2, "odd stride")


@pytest.mark.parametrize("E", [64, 7])
def test_run_lengths_around_the_long_run_threshold(gpu, E):
    """Runs of 1, 2, 16, 17, 63, 64, 65, 66, 128, 129, 513 and 1100 rows in one shuffled batch: both sides of the 64-row threshold
    between the per-group kernel and the workgroup kernel, whole and partial rounds of both, a long run at either end of the
    sorted order (first and last id) and long runs next to each other."""
    from deeprecommendation_amd import native
    gen = torch.Generator().manual_seed(3 + E)
    lengths = [65, 1, 2, 16, 17, 63, 64, 129, 66, 128, 513, 1100]
    ids = torch.cat([torch.full((r,), 7 * k, dtype=torch.int64) for k, r in enumerate(lengths)])      # ascending ids 0, 7, 14, ...
    ids = ids[torch.randperm(ids.numel(), generator=gen)]
    state, _ = _guarded(ROWS, E, gpu, gen)
    for step in (1, 2):
        g = _quantised(ids.numel(), E, gen)
        _step_and_check(native, state, ids, g.to(gpu), g, f32(1e-2), step, f"run lengths E={E}")


@pytest.mark.parametrize("E", [64, 7])
def test_arbitrary_floats_meet_the_summation_bound_and_repeat_bit_for_bit(gpu, E):
    """randn gradients, beta1 = 0, wd = 0, zero moments: exp_avg of a touched row IS the kernel's run sum.  Per element
    |exp_avg - sum_64 g| <= (r - 1) 2^-24 sum|g_k| (1 + 2^-20) for a run of r rows — the bound of any summation order — and a
    second call from the same start state gives the same bits (no atomics)."""
    from deeprecommendation_amd import native
    gen = torch.Generator().manual_seed(11 + E)
    n = 4096
    ids = _batch_ids(n, gen)
    g = torch.randn(n, E, generator=gen)
    p0 = torch.randn(ROWS, E, generator=gen).to(gpu)
    outs = []
    for _ in range(2):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        native.adam_rows_(p, m, v, ids.to(gpu), g.to(gpu), LR, 0.0, B2, EPS, 0.0, 1)
        outs.append((p, m, v))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    m = outs[0][1].cpu().double().numpy()
    g64, idn = g.double().numpy(), ids.numpy()
    longest = 0
    for r in np.unique(idn):
        rows_of = g64[idn == r]
        k = len(rows_of)
        longest = max(longest, k)
        bound = (k - 1) * 2.0 ** -24 * np.abs(rows_of).sum(axis=0) * (1 + 2.0 ** -20)
        assert np.all(np.abs(m[r] - rows_of.sum(axis=0)) <= bound), f"row {r} (run of {k})"
    assert longest >= n // 2
    untouched = np.setdiff1d(np.arange(ROWS), idn)
    assert len(untouched) and not m[untouched].any()


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_all_rows_touched_once_is_the_dense_kernel_bit_for_bit(gpu, wd):
    from deeprecommendation_amd import native
    gen = torch.Generator().manual_seed(21)
    rows, E = 257, 64
    p0 = torch.randn(rows, E, generator=gen).to(gpu)
    sparse = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    dense = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    for step in range(1, 5):
        ids = torch.randperm(rows, generator=gen).to(gpu)
        g = torch.randn(rows, E, generator=gen).to(gpu)
        scattered = torch.zeros_like(p0)
        scattered[ids] = g
        native.adam_rows_(*sparse, ids, g, LR, B1, B2, EPS, wd, step)
        native.adam_step_(dense[0], scattered, dense[1], dense[2], LR, B1, B2, EPS, wd, step)
        for a, b, name in zip(sparse, dense, "pmv"):
            assert torch.equal(a, b), f"{name} differs from ncf_adam_step at step {step}"
    assert not torch.equal(sparse[0], p0)


@pytest.mark.parametrize("E", [64, 7])
def test_out_of_range_ids_are_skipped_and_flagged(gpu, E):
    """-1 and `rows` in the batch (once each, and -1 as a run beyond 64): check_oob raises, every in-range row is updated as usual
    and nothing outside the three buffers is written (64 guard floats on either side of each)."""
    from deeprecommendation_amd import native
    gen = torch.Generator().manual_seed(31 + E)
    native.check_oob(gpu)                                             # start from a clear flag
    for n_bad in (1, 80):
        n = 600
        state, bufs = _guarded(ROWS, E, gpu, gen)
        guards = _guards(bufs)
        ids = _batch_ids(n, gen)
        where = 2 + torch.randperm(n - 2, generator=gen)[:2 * n_bad]
        ids[where[:n_bad]] = -1
        ids[where[n_bad:]] = ROWS
        ids[0], ids[1] = 0, ROWS - 1                                  # the table's first and last row take part
        g = _quantised(n, E, gen)
        _step_and_check(native, state, ids, g.to(gpu), g, 0.0, 1, f"oob x{n_bad}")
        with pytest.raises(IndexError):
            native.check_oob(gpu)
        native.check_oob(gpu)                                         # raising cleared it
        assert all(torch.equal(a, b) for a, b in zip(_guards(bufs), guards)), "a guard float changed"


# ------------------------------------------------------------------------------------------------ the optimiser on a model
def _ncf(gpu, seed=0):
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    torch.manual_seed(seed)
    return BasicNCF(item_dim=30, user_dim=50, item_emb=8, user_emb=8, mlp_dense_layers=[16], dropout_rate=None).to(gpu).train()


def _loss(model, u, i, y):
    return torch.nn.functional.mse_loss(model(u, i), y, reduction="sum")


def test_row_sparse_adam_tracks_fused_adam_when_every_row_is_in_every_batch(gpu):
    from deeprecommendation_amd.optim import FusedAdam, RowSparseAdam
    gen = torch.Generator().manual_seed(41)
    batches = []
    for _ in range(5):
        u = (torch.arange(150) % 50)[torch.randperm(150, generator=gen)]
        i = (torch.arange(150) % 30)[torch.randperm(150, generator=gen)]
        batches.append((u.to(gpu), i.to(gpu), (torch.rand(150, 1, generator=gen) * 5).to(gpu)))
    losses = {}
    for kind in (FusedAdam, RowSparseAdam):
        m = _ncf(gpu)
        opt = kind(m.parameters(), lr=1e-3, weight_decay=1e-4)
        out = []
        for u, i, y in batches:
            opt.zero_grad(set_to_none=True)
            loss = _loss(m, u, i, y)
            loss.backward()
            opt.step()
            out.append(float(loss.detach()))
        losses[kind] = out
        if kind is RowSparseAdam:
            assert m.user_embeddings[0].weight.grad is None and opt.state[m.user_embeddings[0].weight]["step"] == 5
            opt.close()
    for a, b in zip(losses[RowSparseAdam], losses[FusedAdam]):
        assert abs(a - b) <= 1e-5 * abs(b), (losses[RowSparseAdam], losses[FusedAdam])


def test_row_sparse_adam_moves_only_touched_rows_and_keeps_the_rest_of_the_contract(gpu):
    """A batch over 10 users and 5 items: no dense embedding gradient, untouched rows of the weights and of both moments keep their
    bits, touched rows move, biases and MLP parameters take dense updates; eval-mode scores follow the new weights; the state
    moves to FusedAdam and back; nothing synchronises with the host; close() brings the dense gradients back."""
    from deeprecommendation_amd.optim import FusedAdam, RowSparseAdam
    from oracle import ncf_oracle as O
    gen = torch.Generator().manual_seed(43)
    m = _ncf(gpu, seed=1)
    ue, ie = m.user_embeddings[0], m.item_embeddings[0]
    opt = RowSparseAdam(m.parameters(), lr=1e-2, weight_decay=1e-3)
    assert isinstance(ue.weight._ncf_row_grads, list) and isinstance(ie.weight._ncf_row_grads, list)
    assert not hasattr(ue.bias, "_ncf_row_grads") and not hasattr(m.MLP[0].weight, "_ncf_row_grads")
    users, items = torch.randperm(50, generator=gen)[:10], torch.randperm(30, generator=gen)[:5]
    B = 96
    u = users[torch.arange(B) % 10].to(gpu)
    i = items[torch.randint(0, 5, (B,), generator=gen)].to(gpu)
    i[:5] = items.to(gpu)
    y = (torch.rand(B, 1, generator=gen) * 5).to(gpu)

    def scores():
        m.eval()
        with torch.no_grad():
            s = m(u, i)
        state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        ref = O.basic_ncf_forward_indexed(state, u.cpu(), i.cpu())
        assert float((s.cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        m.train()
        return s.clone()

    prev = scores()
    # step 1 creates the state; step 2 is compared against it
    for step in (1, 2):
        before = {k: v.detach().clone() for k, v in m.named_parameters()}
        moments = {k: {s: opt.state[p][s].clone() for s in ("exp_avg", "exp_avg_sq")} for k, p in m.named_parameters() if opt.state[p]}
        opt.zero_grad(set_to_none=True)
        _loss(m, u, i, y).backward()
        assert ue.weight.grad is None and ie.weight.grad is None
        assert len(ue.weight._ncf_row_grads) == 1 and len(ie.weight._ncf_row_grads) == 1
        assert all(p.grad is not None for k, p in m.named_parameters() if "embeddings.0.weight" not in k)
        opt.step()
        assert ue.weight._ncf_row_grads == [] and ie.weight._ncf_row_grads == []
        for lin, name, ids, count in ((ue, "user_embeddings.0.weight", users, 50), (ie, "item_embeddings.0.weight", items, 30)):
            touched = torch.zeros(count, dtype=torch.bool)
            touched[ids] = True
            touched = touched.to(gpu)
            now, was = lin.weight.detach().t(), before[name].t()
            assert torch.equal(now[~touched], was[~touched]), f"{name}: an untouched row moved"
            assert bool((now[touched] != was[touched]).any(dim=1).all()), f"{name}: a touched row did not move"
            st = opt.state[lin.weight]
            assert st["step"] == step and st["exp_avg"].stride() == lin.weight.stride()
            for s in ("exp_avg", "exp_avg_sq"):
                old = moments[name][s].t() if name in moments else torch.zeros_like(now)
                assert torch.equal(st[s].t()[~touched], old[~touched]), f"{name}: {s} of an untouched row changed"
                assert bool((st[s].t()[touched] != old[touched]).any(dim=1).all())
        for k, p in m.named_parameters():
            if "embeddings.0.weight" not in k:
                assert not torch.equal(p.detach(), before[k]), f"{k} took no dense update"
        now_scores = scores()                                         # (c): the scoring caches saw the raw-pointer writes
        assert not torch.equal(now_scores, prev)
        prev = now_scores

    # no host synchronisation in zero_grad / forward / backward / step (the state and the library are warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.zero_grad(set_to_none=True)
        loss = _loss(m, u, i, y)
        loss.backward()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss))

    # a marked weight with nothing pending is skipped but counted; a dense .grad next to pending rows is refused
    opt.zero_grad(set_to_none=True)
    w = ue.weight.detach().clone()
    opt.step()
    assert torch.equal(ue.weight.detach(), w) and opt.state[ue.weight]["step"] == 4
    _loss(m, u, i, y).backward()
    ue.weight.grad = torch.zeros_like(ue.weight)
    with pytest.raises(RuntimeError, match="both"):
        opt.step()
    opt.zero_grad(set_to_none=True)
    assert ue.weight._ncf_row_grads == [] and ie.weight._ncf_row_grads == []

    # (d) the state moves to FusedAdam and back
    sd = opt.state_dict()
    dense = FusedAdam(m.parameters(), lr=1e-2)
    dense.load_state_dict(sd)
    assert dense.state[ue.weight]["step"] == 4 and torch.equal(dense.state[ue.weight]["exp_avg"], opt.state[ue.weight]["exp_avg"])
    assert dense.state[ue.weight]["exp_avg"].stride() == ue.weight.stride()
    back = RowSparseAdam(m.parameters(), lr=1e-2)
    back.load_state_dict(dense.state_dict())
    back.zero_grad(set_to_none=True)
    _loss(m, u, i, y).backward()
    back.step()
    assert back.state[ue.weight]["step"] == 5 and ue.weight.grad is None

    # (e) close(): dense gradients again, and the inherited dense step takes them
    back.close()
    assert not hasattr(ue.weight, "_ncf_row_grads") and not hasattr(ie.weight, "_ncf_row_grads")
    back.zero_grad(set_to_none=True)
    _loss(m, u, i, y).backward()
    assert ue.weight.grad is not None and ue.weight.grad.shape == ue.weight.shape and ie.weight.grad is not None
    back.step()
    assert back.state[ue.weight]["step"] == 6


def test_row_sparse_list_marks_exactly_those_parameters(gpu):
    from deeprecommendation_amd.optim import RowSparseAdam
    m = _ncf(gpu, seed=2)
    ue, ie = m.user_embeddings[0], m.item_embeddings[0]
    with pytest.raises(ValueError):
        RowSparseAdam(m.parameters(), row_sparse=[m.MLP[0].weight])
    assert not hasattr(m.MLP[0].weight, "_ncf_row_grads")
    opt = RowSparseAdam(m.parameters(), lr=1e-2, row_sparse=[ue.weight])
    assert hasattr(ue.weight, "_ncf_row_grads") and not hasattr(ie.weight, "_ncf_row_grads")
    u, i = torch.arange(20, device=gpu), torch.arange(20, device=gpu)
    _loss(m, u, i, torch.ones(20, 1, device=gpu)).backward()
    assert ue.weight.grad is None and ie.weight.grad is not None          # the unmarked table keeps its dense gradient
    w_u, w_i = ue.weight.detach().clone(), ie.weight.detach().clone()
    opt.step()
    assert torch.equal(ue.weight.detach().t()[20:], w_u.t()[20:]) and not torch.equal(ue.weight.detach().t()[:20], w_u.t()[:20])
    assert not torch.equal(ie.weight.detach().t()[:20], w_i.t()[:20])     # the dense route of the unmarked table
    opt.close()


def test_mf_with_marked_weights_takes_one_row_sparse_step(gpu):
    """MF, both weights marked: the training forward takes the HIP gather, one step moves only the touched rows and meets the Adam
    bar against the oracle fed the model's own dX."""
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    from deeprecommendation_amd.optim import RowSparseAdam
    torch.manual_seed(51)
    m = MF(item_dim=30, user_dim=50, item_emb=8, user_emb=8).to(gpu).train()
    ue, ie = m.user_embeddings[0], m.item_embeddings[0]
    lr, wd = f32(1e-2), f32(1e-3)
    opt = RowSparseAdam(m.parameters(), lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd)
    gen = torch.Generator().manual_seed(52)
    u = torch.randint(0, 12, (64,), generator=gen).to(gpu)
    i = torch.randint(20, 27, (64,), generator=gen).to(gpu)
    y = (torch.rand(64, 1, generator=gen) * 5).to(gpu)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    _loss(m, u, i, y).backward()
    assert ue.weight.grad is None and ie.weight.grad is None and ue.bias.grad is not None
    pending = {"u": ue.weight._ncf_row_grads[0], "i": ie.weight._ncf_row_grads[0]}
    refs = {}
    for key, lin in (("u", ue), ("i", ie)):
        ids, dX = pending[key]
        p0 = lin.weight.detach().t().cpu().double().numpy()
        refs[key] = (row_adam_ref(p0, np.zeros_like(p0), np.zeros_like(p0), ids.cpu().numpy(), dX.cpu().double().numpy(), lr, B1, B2, EPS,
                                  wd, 1), ids.cpu())
    opt.step()
    for key, lin, name in (("u", ue, "user_embeddings.0.weight"), ("i", ie, "item_embeddings.0.weight")):
        (rp, rm, rv), ids = refs[key]
        st = opt.state[lin.weight]
        _adam_bar(lin.weight.t(), rp, f"MF {key} p")
        _adam_bar(st["exp_avg"].t(), rm, f"MF {key} m")
        _adam_bar(st["exp_avg_sq"].t(), rv, f"MF {key} v")
        touched = torch.zeros(lin.weight.shape[1], dtype=torch.bool)
        touched[ids] = True
        touched = touched.to(gpu)
        assert torch.equal(lin.weight.detach().t()[~touched], before[name].t()[~touched])
        assert bool((lin.weight.detach().t()[touched] != before[name].t()[touched]).any(dim=1).all())
    assert not torch.equal(ue.bias.detach(), before["user_embeddings.0.bias"])
    opt.close()
    # unmarked again: the torch-op path and its dense gradients
    opt.zero_grad(set_to_none=True)
    _loss(m, u, i, y).backward()
    assert ue.weight.grad is not None


def test_resident_bpr_epoch_with_row_sparse_adam(gpu, tmp_path):
    """One device-resident pair-wise epoch of train_model with RowSparseAdam: two forwards per step give two pending entries per
    table; the loss is finite, item rows that are reached only as negatives have moved, and the epoch's flags are clear."""
    from deeprecommendation_amd.content_providers.index_providers import IndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset, FixedRankingDataset
    from deeprecommendation_amd.neural_collaborative_filtering.train import train_model
    from deeprecommendation_amd.optim import RowSparseAdam
    from test_gpu_bpr_training import _basic_model, _toy_ranking
    U, I, extra = 120, 60, 5
    ranking, val, _ = _toy_ranking(U, I, seed=9)
    for k in range(10):                                               # rows whose only negative is an item nobody rated
        ranking.at[3 * k, "negative_movieIds"] = [I + 1 + k % extra]
        ranking.at[3 * k, "negative_ratings"] = [1.0]
    assert not set(ranking.positive_movieId) & set(range(I + 1, I + extra + 1))
    prov = IndexProvider(np.arange(1, U + 1), np.arange(1, I + extra + 1))
    model = _basic_model(U, I + extra, seed=9).to(gpu)
    w0 = model.item_embeddings[0].weight.detach().clone()
    opt = RowSparseAdam(model.parameters(), lr=5e-3)
    mm = train_model(model, FixedRankingDataset(ranking, prov), FixedPointwiseDataset(val, prov), lr=5e-3, weight_decay=0.0, batch_size=128,
                     val_batch_size=256, early_stop=False, final_model_path=None, checkpoint_model_path=str(tmp_path / "c.pt"),
                     max_epochs=1, device=gpu, resident=True, verbose=False, optimizer=opt)     # pairs.check() runs at the epoch's end
    assert len(mm["train_loss"]) == 1 and np.isfinite(mm["train_loss"][0])
    w1 = model.item_embeddings[0].weight.detach()
    assert model.item_embeddings[0].weight.grad is None
    moved = (w1.t() != w0.t()).any(dim=1)
    assert bool(moved[I:I + extra].all()), "an item reached only as a negative did not move"
    assert bool(torch.isfinite(w1).all())
    opt.close()
