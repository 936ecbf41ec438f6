"""GPU: the full-catalogue softmax loss of a dot-product readout (csrc/dot_softmax.hip) against the float64 reference and the
cases of tests/dot_softmax_ref.py, on every form the host can pick: ncf_dot_lse, both roles of ncf_dot_softmax_grad,
DotSoftmaxLossFn under MF and GraphNCF, fit_implicit(loss="softmax"), the refusals, the out-of-range guard and the memory bound."""
import functools

import numpy as np
import pytest
import torch

import dot_softmax_ref as R
from deeprecommendation_amd import implicit, native
from deeprecommendation_amd.autograd import DotSoftmaxLossFn
from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF
from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
from deeprecommendation_amd.optim import RowSparseAdam

pytestmark = pytest.mark.gpu
KINDS = ("lse", "grad_rows", "grad_items")


@pytest.mark.parametrize("name", list(R.CASES))
def test_lse_and_both_gradients_against_float64_on_the_form_the_case_must_take(gpu, name):
    c = R.case(name)
    forms = tuple(("one" if tiles == 1 else "multi") + ("+chunked" if chunk < resident else "")
                  for (_, tiles, chunk), resident in ((native.dot_softmax_plan(k, c.B, c.N, c.D), c.N if k == "grad_items" else c.B)
                                                      for k in KINDS))
    assert forms == R.FORMS[name]                              # no form is silently skipped
    A, Q, idxA, idxB, t, g = c.tables(gpu)
    assert A.stride(0) == c.A.shape[1] and Q.stride(0) == c.Q.shape[1]
    lse, mx = native.dot_lse(A, idxA, Q, idxB, c.scale, return_max=True)
    dA, dQ = native.dot_softmax_grad(A, idxA, Q, idxB, t, lse, g, c.scale)
    lse2 = native.dot_lse(A, idxA, Q, idxB, c.scale)
    dA2, dQ2 = native.dot_softmax_grad(A, idxA, Q, idxB, t, lse, g, c.scale)
    native.check_oob(gpu)
    print(name, forms)
    assert torch.equal(mx.cpu().double(), c.ref["z"].max(1).values)               # the maximum is exact
    R.lse_close(lse, c.ref["lse"])
    conf = name == "confident"
    R.grad_close(dA, c.ref["dA"], c.ref["absA"], "dA", confident=c.ref["confA"] if conf else None)
    R.grad_close(dQ, c.ref["dQ"], c.ref["absQ"], "dQ", confident=c.ref["confQ"] if conf else None)
    assert torch.equal(lse, lse2) and torch.equal(dA, dA2) and torch.equal(dQ, dQ2)      # run to run, bit for bit
    # the target logit the loss uses is gather_dot's bits (and, the scores being exact integers, the reference's)
    zt = native.gather_dot(A, idxA, Q, t if idxB is None else idxB[t], B=c.B).view(-1) * c.scale
    assert torch.equal(zt.cpu().double(), c.ref["z"][torch.arange(c.B), c.t])
    if name == "zero":
        assert float((lse.cpu().double() - np.log(c.N)).abs().max()) <= 1e-6 * np.log(c.N)
        assert not bool(dA.any()) and not bool(dQ.any())
    if name == "peaked":
        assert bool(torch.isfinite(lse).all())
        assert torch.equal(lse[c.peaked_rows].cpu(), torch.full((len(c.peaked_rows),), 120.0))


def test_the_scores_inside_the_kernels_are_gather_dots_bits_on_inexact_tables(gpu):
    """Random fp32 tables, where the order of summation shows: with one column per row (N = 1) lse IS the logit, so the kernel's
    chain must be gather_dot's; and the maximum over a catalogue is the maximum of gather_dot's scores, bit for bit."""
    gen = torch.Generator().manual_seed(3)
    for D in (1, 17, 64, 65, 200, 256):
        A = torch.randn(37, D, generator=gen).to(gpu)
        Q = torch.randn(150, D, generator=gen).to(gpu)
        ia = torch.arange(37, device=gpu).repeat_interleave(150)
        ib = torch.arange(150, device=gpu).repeat(37)
        s = native.gather_dot(A, ia, Q, ib).view(37, 150)
        _, mx = native.dot_lse(A, None, Q, None, 0.5, return_max=True)
        assert torch.equal(mx, (s * 0.5).max(1).values)
        one = native.dot_lse(A, None, Q, torch.full((1,), 149, dtype=torch.int64, device=gpu), 2.0)
        assert torch.equal(one, s[:, 149] * 2.0)
    native.check_oob(gpu)


# ------------------------------------------------------------------ refusals and the out-of-range guard
def test_refusals_raise_with_their_code_and_name_the_entry_point(gpu):
    A, Q = torch.zeros(8, 16, device=gpu), torch.zeros(9, 16, device=gpu)
    t, lse, g = torch.zeros(8, dtype=torch.int64, device=gpu), torch.zeros(8, device=gpu), torch.ones(8, device=gpu)
    wide = torch.zeros(4, 257, device=gpu)
    for scale in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(native.NativeError, match="ncf_dot_lse: scale") as e:
            native.dot_lse(A, None, Q, None, scale)
        assert e.value.code == native.NCF_EINVAL
        with pytest.raises(native.NativeError, match="ncf_dot_softmax_grad: scale") as e:
            native.dot_softmax_grad(A, None, Q, None, t, lse, g, scale)
        assert e.value.code == native.NCF_EINVAL
    with pytest.raises(native.NativeError, match="ncf_dot_lse: width D = 257") as e:
        native.dot_lse(wide, None, wide, None)
    assert e.value.code == native.NCF_EUNSUPPORTED
    with pytest.raises(native.NativeError, match="ncf_dot_softmax_grad: width D = 257") as e:
        native.dot_softmax_grad(wide, None, wide, None, t[:4], lse[:4], g[:4])
    assert e.value.code == native.NCF_EUNSUPPORTED
    with pytest.raises(ValueError, match="targets"):
        native.dot_softmax_grad(A, None, Q, None, t[:3], lse, g)
    # rows == 0: OK, empty results, nothing launched
    none = torch.zeros(0, dtype=torch.int64, device=gpu)
    assert native.dot_lse(A, none, Q, None).shape == (0,)
    dA, dQ = native.dot_softmax_grad(A, none, Q, None, none, lse[:0], g[:0], need=(True, False))
    assert dA.shape == (0, 16) and dQ is None
    native.check_oob(gpu)


@pytest.mark.parametrize("what", ["idxA", "idxB", "target"])
def test_an_id_out_of_range_raises_index_error_and_leaves_the_other_rows_right(gpu, what):
    """The guard: the id is never used as an address.  A listed row with a bad id or a bad target gets a zero gradient row and adds
    nothing to the columns; a bad column is in no denominator and gets a zero gradient row: the other rows' results are those of
    the problem without it."""
    gen = np.random.default_rng(11)
    B, N, D, scale = 70, 300, 40, 0.5
    A = torch.from_numpy(gen.integers(-2, 3, size=(B, D))).float()
    Q = torch.from_numpy(gen.integers(-2, 3, size=(N + 3, D))).float()
    idxA, idxB = np.arange(B)[::-1].copy(), gen.permutation(N + 3)[:N]
    t = gen.integers(0, N, size=B)
    g = torch.from_numpy(gen.integers(1, 4, size=B)).float()
    p_t = torch.softmax(A[idxA].double() @ Q[idxB].double().t() * scale, 1)[torch.arange(B), torch.from_numpy(t)]
    g[p_t > 0.25] = 0.0                   # dot_softmax_ref's rule on a target's own probability (with room for the dropped column)
    bad_row, bad_col = 33, 257
    keep_rows, keep_cols = np.arange(B), np.arange(N)
    if what == "idxA":
        idxA[bad_row] = B + 5
    elif what == "idxB":
        idxB[bad_col] = -1
        g[torch.from_numpy(t == bad_col)] = 0.0
        t[t == bad_col] = 0
        keep_cols = np.delete(keep_cols, bad_col)
    else:
        t[bad_row] = N
    on = lambda x: torch.from_numpy(x).to(gpu)
    a, q = A.to(gpu), Q.to(gpu)
    lse = native.dot_lse(a, on(idxA), q, on(idxB), scale)
    if what != "target":
        with pytest.raises(IndexError):
            native.check_oob(gpu)
    dA, dQ = native.dot_softmax_grad(a, on(idxA), q, on(idxB), on(t), lse, g.to(gpu), scale)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.check_oob(gpu)                                        # raised once, then cleared
    # the reference over what remains: a bad listed row is a zero user row with g = 0
    U = A[np.clip(idxA, 0, B - 1)].double()
    gg = g.double().clone()
    tt = t.copy()
    if what != "idxB":
        gg[bad_row] = 0.0
        tt[bad_row] = 0
        if what == "idxA":
            U[bad_row] = 0.0
    V = Q[idxB[keep_cols]].double()
    col_of = np.full(N, -1)
    col_of[keep_cols] = np.arange(len(keep_cols))
    ref = R.reference(U, V, torch.from_numpy(col_of[tt]), gg, scale)
    R.lse_close(lse, ref["lse"])
    R.grad_close(dA, ref["dA"], ref["absA"], "dA")
    R.grad_close(dQ[keep_cols], ref["dQ"], ref["absQ"], "dQ")
    if what == "idxB":
        assert not bool(dQ[bad_col].any())
    else:
        assert not bool(dA[bad_row].any())


# ------------------------------------------------------------------ autograd
def _mf_case(gpu, D=32, seed=0):
    """An MF whose tables hold small integers (exact scores), a batch with a repeated user, and the float64 truth of its loss."""
    gen = np.random.default_rng(seed)
    U, I, B = 23, 75, 40
    torch.manual_seed(seed)
    model = MF(item_dim=I, user_dim=U, item_emb=D, user_emb=D).to(gpu)
    with torch.no_grad():
        for lin in (model.user_embeddings[0], model.item_embeddings[0]):
            lin.weight.copy_(torch.from_numpy(gen.integers(-2, 3, size=tuple(lin.weight.shape))).float())
            lin.bias.copy_(torch.from_numpy(gen.integers(-1, 2, size=tuple(lin.bias.shape))).float())
    users = gen.integers(0, U, size=B)
    users[5] = users[4]
    items = gen.integers(0, I, size=B)
    g = torch.from_numpy(np.array([1.0, -2.0, 0.0, 0.5])[np.arange(B) % 4])
    return model, users, items, g


def _mf_truth(model, users, items, g, scale):
    ue, ie = model.user_embeddings[0], model.item_embeddings[0]
    Ut = (ue.weight.detach().t() + ue.bias.detach()).cpu().double()
    Qt = (ie.weight.detach().t() + ie.bias.detach()).cpu().double()
    ref = R.reference(Ut[users], Qt, torch.from_numpy(items), g, scale)
    nU = Ut.shape[0]
    scat = torch.zeros(nU, len(users), dtype=torch.float64)
    scat[torch.from_numpy(users), torch.arange(len(users))] = 1.0
    dUt, absUt = scat @ ref["dA"], scat @ ref["absA"]              # the same tolerance carried through the scatter
    return ref, dUt, absUt


@pytest.mark.parametrize("row_sparse", [False, True])
def test_mf_softmax_loss_backward_is_the_float64_gradient(gpu, row_sparse):
    scale = 0.25
    model, users, items, g = _mf_case(gpu)
    model.train()
    opt = RowSparseAdam(model.parameters(), lr=0.0) if row_sparse else None
    ref, dUt, absUt = _mf_truth(model, users, items, g, scale)
    u, i = torch.from_numpy(users).to(gpu), torch.from_numpy(items).to(gpu)
    loss = model.softmax_loss(u, i, scale)
    assert loss.shape == (len(users),)
    tol = 1e-5 * ref["loss"].abs() + 1e-6 * ref["lse"].abs().max()
    assert bool(((loss.detach().cpu().double() - ref["loss"]).abs() <= tol).all())
    (loss * g.float().to(gpu)).sum().backward()
    native.check_oob(gpu)
    ue, ie = model.user_embeddings[0], model.item_embeddings[0]
    R.grad_close(ie.weight.grad.t(), ref["dQ"], ref["absQ"], "item weight")
    R.grad_close(ie.bias.grad, ref["dQ"].sum(0), ref["absQ"].sum(0), "item bias")
    if row_sparse:
        assert ue.weight.grad is None and len(ue.weight._ncf_row_grads) == 1 and not ie.weight._ncf_row_grads
        ids, rows = ue.weight._ncf_row_grads[0]
        assert torch.equal(ids, u)
        R.grad_close(rows, ref["dA"], ref["absA"], "user rows handed to RowSparseAdam")
        opt.step()                                                # the dense item gradient and the user rows, one step, no error
        opt.close()
    else:
        R.grad_close(ue.weight.grad.t(), dUt, absUt, "user weight")
    R.grad_close(ue.bias.grad, ref["dA"].sum(0), ref["absA"].sum(0), "user bias")


U_, I_ = 40, 50


@functools.lru_cache(None)
def _pairs():
    rng = np.random.default_rng(23)
    u = np.repeat(np.arange(U_), 9)
    i = np.concatenate([rng.choice(I_, 9, replace=False) for _ in range(U_)])
    return u, i


def _graph():
    from deeprecommendation_amd.content_providers.index_providers import IndexGraphProvider
    u, i = _pairs()
    return IndexGraphProvider(np.arange(U_), np.arange(I_), u, i, np.full(len(u), 5.0), binary=True).get_graph()


def test_graph_ncf_softmax_loss_backward_is_the_float64_gradient_of_its_node_table(gpu):
    """GraphNCF(use_dot_product=True): the loss and the gradient DotSoftmaxLossFn sends into the propagated node table against
    float64 on that table's own fp32 values, through the Function's two outputs summed by autograd (user rows scattered with a
    repeated user, item rows dense); then the parameters' gradients equal the table gradient pushed through the same graph."""
    torch.manual_seed(1)
    graph = _graph().to(gpu)
    model = GraphNCF(item_dim=I_, user_dim=U_, num_gnn_layers=2, hetero=False, node_emb=32, use_dot_product=True, dropout_rate=0.0).to(gpu)
    model.train()
    gen = np.random.default_rng(2)
    B, scale = 30, 2.0
    users, items = gen.integers(0, U_, size=B), gen.integers(0, I_, size=B)
    users[7] = users[3]
    un, it = torch.from_numpy(users + I_).to(gpu), torch.from_numpy(items).to(gpu)
    combined = model._combined_train_hip(graph, un, it, False)
    assert combined.shape == (I_ + U_, 32)
    table = combined.detach().clone().requires_grad_(True)
    g = torch.from_numpy(np.array([1.0, -1.0, 0.5])[np.arange(B) % 3])
    loss = DotSoftmaxLossFn.apply(table, table[:I_], un, it, scale)
    (loss * g.float().to(gpu)).sum().backward()
    T = table.detach().cpu().double()
    ref = R.reference(T[users + I_], T[:I_], torch.from_numpy(items), g, scale)
    assert bool(((loss.detach().cpu().double() - ref["loss"]).abs() <= 1e-5 * ref["loss"].abs() + 1e-6 * ref["lse"].abs().max()).all())
    scat = torch.zeros(I_ + U_, B, dtype=torch.float64)
    scat[torch.from_numpy(users + I_), torch.arange(B)] = 1.0
    want, bar = scat @ ref["dA"], scat @ ref["absA"]
    want[:I_] += ref["dQ"]
    bar[:I_] += ref["absQ"]
    R.grad_close(table.grad, want, bar, "node table")
    # the model's method is that Function over its own table: the same loss bits, and parameter gradients equal to the table
    # gradient pushed back through the propagation
    torch.manual_seed(4)
    loss2 = model.softmax_loss(graph, un, it, scale, mask_targets=False)
    assert torch.equal(loss2.detach(), loss.detach())
    (loss2 * g.float().to(gpu)).sum().backward()
    got = [p.grad.clone() for p in model.parameters() if p.grad is not None]
    model.zero_grad()
    torch.manual_seed(4)
    model._combined_train_hip(graph, un, it, False).backward(table.grad)
    want_p = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(got) == len(want_p) > 0
    for a, b in zip(got, want_p):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))
    native.check_oob(gpu)
    mlp = GraphNCF(item_dim=I_, user_dim=U_, num_gnn_layers=1, hetero=False, node_emb=32, mlp_dense_layers=[16]).to(gpu)
    with pytest.raises(TypeError, match="use_dot_product"):
        mlp.softmax_loss(graph, un, it)


# ------------------------------------------------------------------ fit_implicit
def _fit(gpu, lr, epochs, seed=9, model_seed=0, batch_size=128, **kw):
    u, i = _pairs()
    data = implicit.ImplicitFeedback(u, i, U_, I_, gpu)
    torch.manual_seed(model_seed)
    model = MF(item_dim=I_, user_dim=U_, item_emb=16, user_emb=16)
    start = [p.detach().clone() for p in model.parameters()]
    hist = implicit.fit_implicit(model, data, loss="softmax", epochs=epochs, batch_size=batch_size, lr=lr, seed=seed, **kw)
    return model, data, hist, start


def test_fit_implicit_softmax_reports_the_mean_negative_log_likelihood(gpu):
    model, data, hist, start = _fit(gpu, lr=0.0, epochs=1, scale=0.5, negatives="ignored")
    for p, q in zip(model.parameters(), start):
        assert torch.equal(p.detach().cpu(), q)                   # lr = 0: the model the loss is reported for is the initial one
    ue, ie = model.user_embeddings[0], model.item_embeddings[0]
    Ut = (ue.weight.detach().t() + ue.bias.detach()).cpu().double()
    Qt = (ie.weight.detach().t() + ie.bias.detach()).cpu().double()
    u, i = data.users.cpu(), data.items.cpu()
    ref = R.reference(Ut[u], Qt, i, torch.ones(len(u), dtype=torch.float64), 0.5)
    want = float(ref["loss"].mean())
    got = hist["train_loss"][0]
    print(f"train_loss {got!r} reference {want!r}")
    # each row's loss within the lse bar plus the fp32 chain's rounding of its two logits (D = 16, |z| < 1: < 2^-20 each); a batch's
    # 128 losses are summed in fp32 (<= 128 * 2^-24 relative in any order), the batches in float64
    assert abs(got - want) <= (1e-5 + 128 * 2.0 ** -24) * want + 2.0 ** -19


def test_fit_implicit_softmax_learns_and_repeats_bit_for_bit(gpu):
    model, _, hist, _ = _fit(gpu, lr=0.05, epochs=5)
    print(hist["train_loss"])
    assert hist["train_loss"][-1] < hist["train_loss"][0]
    model2, _, hist2, _ = _fit(gpu, lr=0.05, epochs=5)
    assert hist2["train_loss"] == hist["train_loss"]
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p.detach(), q.detach())


# ------------------------------------------------------------------ memory
def test_forward_and_backward_never_hold_a_b_by_n_matrix(gpu):
    B, N, D = 4096, 8192, 64
    gen = torch.Generator().manual_seed(0)
    U = (torch.randn(5000, D, generator=gen) * 0.3).to(gpu).requires_grad_(True)
    Q = (torch.randn(N, D, generator=gen) * 0.3).to(gpu).requires_grad_(True)
    users = torch.randint(0, 5000, (B,), generator=gen).to(gpu)
    t = torch.randint(0, N, (B,), generator=gen).to(gpu)
    DotSoftmaxLossFn.apply(U, Q, users[:64], t[:64], 1.0).sum().backward()      # the library is loaded and warm
    U.grad = Q.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = DotSoftmaxLossFn.apply(U, Q, users, t, 1.0)
    loss.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = (U.numel() + Q.numel() + loss.numel()) * 4                          # both table gradients and the loss
    print(f"peak {peak / 2 ** 20:.1f} MiB over the inputs, outputs {outputs / 2 ** 20:.1f} MiB, B x N matrix {4 * B * N / 2 ** 20:.1f} MiB")
    assert peak - outputs < 4 * B * N / 4
    native.check_oob(gpu)
    assert bool(torch.isfinite(U.grad).all()) and bool(torch.isfinite(Q.grad).all())
