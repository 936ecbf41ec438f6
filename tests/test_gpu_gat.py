"""GPU: the LightGAT training kernels (csrc/gat.hip, csrc/edge_softmax.hip) against tests/gat_ref.py — the softmax over kept entries (bit-identical to the
scoring softmax without a keep mask, exact cases bitwise, random and peaked scores against float64), the per-edge gradient (exact
cases bitwise on every launch form, random data under the rounding-count bound), the ordered reduce per source, the refusals —
and GraphNCF(convType='LightGAT') training steps on the HIP blocks against a CPU copy of the model on the graph of kept edges."""
import copy

import numpy as np
import pytest
import torch

import gat_ref as G
import graph_forms_ref as R
from dropout_mask_ref import mask_factor64, spmm_dropout64
from edge_keep_ref import edge_keep_ref, keep_lists, node_keep

pytestmark = pytest.mark.gpu


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _segments(rowptr, seg_len):
    """(segptr, row_of, seg_first) of native.SegmentedCSR's level 0 at ``seg_len`` (None: the rows; row_of None when nothing splits)."""
    from deeprecommendation_amd import native
    if seg_len is None:
        return rowptr, None, None
    col = torch.zeros(int(rowptr[-1]), dtype=torch.int32, device=rowptr.device)
    segptr, row_of, _ = native.SegmentedCSR(rowptr, col, None, seg_len=seg_len).levels[0]
    return segptr, row_of, (None if row_of is None else R.seg_first_of(row_of, rowptr.numel() - 1))


def _softmax(case, seg_len, keep="case"):
    from deeprecommendation_amd import native
    segptr, row_of, seg_first = _segments(case["rowptr"], seg_len)
    return native.gat_edge_softmax(segptr, row_of, seg_first, case["rowptr"].numel() - 1, case["col"], case["attr"],
                                   case["keep"] if keep == "case" else keep, case["s"])


def _grad(case, alpha, seg_len, p, seed):
    from deeprecommendation_amd import native
    segptr, row_of, seg_first = _segments(case["rowptr"], seg_len)
    return native.gat_edge_grad(segptr, row_of, seg_first, case["rowptr"].numel() - 1, case["col"], case["attr"], alpha, case["dY"], case["z"], p, seed)


def _cpu(case):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


# ------------------------------------------------------------------------------------------------------------ 1. softmax
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("lengths,seg_len", [(R.TREE_LENGTHS, 4), (R.TREE_LENGTHS, 64), (R.PLAIN_LENGTHS, None)], ids=["tree-seg4", "tree-seg64", "plain-rows"])
def test_softmax_without_keep_has_the_bits_of_the_scoring_softmax(gpu, lengths, seg_len, weighted):
    from deeprecommendation_amd import native
    gen = _gen(gpu, 3)
    rowptr = R.rowptr_of(lengths, gpu)
    E, Ns = int(rowptr[-1]), 300
    col = R.draw_cols(E, Ns, gen)
    attr = torch.randn(E, generator=gen, device=gpu) if weighted else None
    s = (torch.randn(Ns, generator=gen, device=gpu) * 4).contiguous()
    segptr, row_of, seg_first = _segments(rowptr, seg_len)
    assert (row_of is None) == (seg_len is None)
    want = native.edge_softmax_csr(rowptr, col, attr, s, segments=None if row_of is None else (segptr, row_of, seg_first))
    alpha, coef = native.gat_edge_softmax(segptr, row_of, seg_first, len(lengths), col, attr, None, s)
    assert torch.equal(coef.view(torch.int32), want.view(torch.int32))
    if weighted:
        assert torch.equal((attr * alpha).view(torch.int32), want.view(torch.int32))
    alpha2, coef2 = native.gat_edge_softmax(segptr, row_of, seg_first, len(lengths), col, attr, None, s)
    assert torch.equal(alpha.view(torch.int32), alpha2.view(torch.int32)) and torch.equal(coef.view(torch.int32), coef2.view(torch.int32))
    # "kept" taken by every entry: an all-ones keep is no keep at all
    alpha1, coef1 = native.gat_edge_softmax(segptr, row_of, seg_first, len(lengths), col, attr, torch.ones(E, device=gpu), s)
    assert torch.equal(alpha1.view(torch.int32), alpha.view(torch.int32)) and torch.equal(coef1.view(torch.int32), coef.view(torch.int32))


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("seg_len", [None, 4, 64])
def test_softmax_with_keep_exact_cases(gpu, seg_len, weighted):
    case = G.exact_case(_gen(gpu, 1), 8, weighted)
    want = G.exact_alpha(_cpu(case))
    alpha, coef = _softmax(case, seg_len)
    assert R.same_bits(alpha, want)
    assert R.same_bits(coef, want if not weighted else (case["attr"].cpu().numpy() * want).astype(np.float32))
    again = _softmax(case, seg_len)
    assert R.same_bits(again[0], alpha) and R.same_bits(again[1], coef)


def _random_softmax_case(gpu, peaked):
    gen = _gen(gpu, 17)
    lengths = [3000, 0, 1, 64, 65, 700, 5, 129, 2999]
    rowptr = R.rowptr_of(lengths, gpu)
    E, Ns = int(rowptr[-1]), 400
    col = R.draw_cols(E, Ns, gen)
    keep = (torch.rand(E, generator=gen, device=gpu) > 0.3).float()
    keep[int(rowptr[6]):int(rowptr[7])] = 0                                   # a row with every entry removed
    s = torch.rand(Ns, generator=gen, device=gpu) * 24.0                       # spread <= 24
    if peaked:
        # every removed in-range entry reads a node whose score is 60 .. 100 above all kept ones: had it stayed in its group it
        # would hold the row maximum, and every kept weight would be exp(-60) or an overflowed ratio
        s = torch.rand(Ns, generator=gen, device=gpu) * 5.0
        hot = torch.arange(Ns, device=gpu) % 4 == 0
        s = torch.where(hot, s + 60.0 + 40.0 * torch.rand(Ns, generator=gen, device=gpu), s)
        inr = (col >= 0) & (col < Ns)
        is_hot = torch.zeros(E, dtype=torch.bool, device=gpu)
        is_hot[inr] = hot[col[inr].long()]
        keep = torch.where(is_hot, torch.zeros_like(keep), torch.ones_like(keep))
        assert float(s.max() - s[~hot].max()) >= 55.0
    attr = torch.randn(E, generator=gen, device=gpu)
    return dict(rowptr=rowptr, col=col, attr=attr, keep=keep.contiguous(), s=s.contiguous())


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("seg_len", [None, 64])
def test_softmax_with_keep_against_float64(gpu, seg_len, peaked):
    case = _random_softmax_case(gpu, peaked)
    alpha, coef = _softmax(case, seg_len)
    a64, c64 = G.masked_softmax64(case["rowptr"], case["col"], case["attr"], case["keep"], case["s"])
    assert bool(torch.isfinite(alpha).all()) and bool(torch.isfinite(coef).all())
    for got, ref, what in ((alpha, a64, "alpha"), (coef, c64, "coef")):
        bar = R.softmax_bar(case["rowptr"], ref)
        err = (got.double() - ref).abs()
        used = float((err / bar.clamp_min(1e-300)).max()) if bool((bar > 0).any()) else 0.0
        print(f"{what} seg_len {seg_len} peaked {peaked}: worst fraction of the bar {used:.3f}")
        assert bool((err <= bar).all()), what
    dead = (case["keep"] == 0) | (case["col"] < 0) | (case["col"] >= case["s"].numel())
    assert bool((alpha[dead] == 0).all())
    dst = R.rows_of(case["rowptr"])
    sums = torch.zeros(case["rowptr"].numel() - 1, dtype=torch.float64, device=gpu).index_add_(0, dst, alpha.double())
    has_kept = torch.zeros_like(sums).index_add_(0, dst, (~dead).double()) > 0
    assert bool(((sums[has_kept] - 1).abs() < 1e-4).all()) and bool((sums[~has_kept] == 0).all())
    if peaked:
        assert float(alpha.max()) > 1e-4                                       # the kept weights are not exp(-60) of a shifted maximum


# ---------------------------------------------------------------------------------------------------------- 2. edge_grad
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("seg_len", [None, 4, 64])
@pytest.mark.parametrize("D", [4, 36, 64])
def test_edge_grad_exact_cases(gpu, D, seg_len, p):
    case = G.exact_case(_gen(gpu, 2 + D), D)
    seed = 1234 + D
    want, _ = G.exact_dlogit(_cpu(case), p, seed)
    alpha, _ = _softmax(case, seg_len)
    assert R.same_bits(alpha, G.exact_alpha(_cpu(case)))
    got = _grad(case, alpha, seg_len, p, seed)
    assert R.same_bits(got, want)
    assert R.same_bits(_grad(case, alpha, seg_len, p, seed), got)
    if p > 0:                                                                  # the mask is a function of the seed
        assert not R.same_bits(_grad(case, alpha, seg_len, p, seed + 1), want)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("seg_len", [None, 64])
@pytest.mark.parametrize("D", [64, 132])
def test_edge_grad_random_under_the_rounding_bound(gpu, D, seg_len, p):
    gen = _gen(gpu, 23 + D)
    lengths = R.TREE_LENGTHS + [3000, 2]
    rowptr = R.rowptr_of(lengths, gpu)
    E, Nz = int(rowptr[-1]), 500
    case = dict(rowptr=rowptr, col=R.draw_cols(E, Nz, gen), attr=torch.randn(E, generator=gen, device=gpu),
                keep=(torch.rand(E, generator=gen, device=gpu) > 0.2).float().contiguous(), s=torch.randn(Nz, generator=gen, device=gpu) * 2,
                z=torch.randn(Nz, D, generator=gen, device=gpu), dY=torch.randn(len(lengths), D, generator=gen, device=gpu))
    alpha, _ = _softmax(case, seg_len)
    got = _grad(case, alpha, seg_len, p, 99)
    c = _cpu(case)
    ref, _ = G.edge_grad64(c["rowptr"], c["col"], c["attr"], alpha.cpu(), c["dY"], c["z"], p, 99)
    bound = G.edge_grad_bound(c["rowptr"], c["col"], c["attr"], alpha.cpu(), c["dY"], c["z"], p, 99, seg_len)
    ok, used, err, b, rel = R.bound_check(got.cpu(), ref, bound)
    print(f"edge_grad D {D} seg_len {seg_len} p {p}: worst fraction of the bound {used:.3f} (err {err:.3e}, bound {b:.3e}), max err / max |ref| {rel:.2e}")
    assert ok
    assert R.same_bits(_grad(case, alpha, seg_len, p, 99), got)


# ------------------------------------------------------------------------------------------------------ 3. source_reduce
@pytest.mark.parametrize("seg_len,fan", [(4, 2), (64, 4), (512, 64), (2000, 64)])
def test_source_reduce_exact(gpu, seg_len, fan):
    from deeprecommendation_amd import native
    rowptr_t, eid, dlogit = G.reduce_case(_gen(gpu, 5))
    csr_t = native.SegmentedCSR(rowptr_t, torch.zeros(eid.numel(), dtype=torch.int32, device=gpu), None, seg_len=seg_len, fan=fan)
    assert (len(csr_t.levels) > 2) == (seg_len < 512) and (len(csr_t.levels) == 1) == (seg_len == 2000)
    want = G.as_exact32(G.source_reduce64(rowptr_t, eid, dlogit))
    got = native.gat_source_reduce(csr_t, eid, dlogit)
    assert R.same_bits(got, want) and want[1] == 0 and want[6] == 0
    assert R.same_bits(native.gat_source_reduce(csr_t, eid, dlogit), got)


def test_edgeless_graph(gpu):
    from deeprecommendation_amd import native
    rowptr = torch.zeros(6, dtype=torch.int64, device=gpu)
    empty_i, empty_f = torch.zeros(0, dtype=torch.int32, device=gpu), torch.zeros(0, device=gpu)
    csr_t = native.SegmentedCSR(rowptr, empty_i, None)
    ds = native.gat_source_reduce(csr_t, empty_i, empty_f)
    assert ds.shape == (5,) and bool((ds == 0).all())
    alpha, coef = native.gat_edge_softmax(rowptr, None, None, 5, empty_i, None, None, torch.zeros(5, device=gpu))
    assert alpha.numel() == 0 and coef.numel() == 0
    assert native.gat_edge_grad(rowptr, None, None, 5, empty_i, None, empty_f, torch.zeros(5, 8, device=gpu), torch.zeros(5, 8, device=gpu)).numel() == 0


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing(gpu):
    from deeprecommendation_amd import native
    lib = native.load_library()
    case = G.exact_case(_gen(gpu, 1), 8)
    n_rows, E = case["rowptr"].numel() - 1, case["col"].numel()
    segptr, row_of, seg_first = _segments(case["rowptr"], 64)
    n_seg = segptr.numel() - 1
    alpha, coef, dl = (torch.full((E,), 7.0, device=gpu) for _ in range(3))
    ds = torch.full((n_rows,), 7.0, device=gpu)
    ws = torch.full((2 * n_seg + 2 * n_rows,), 7.0, device=gpu)
    P = lambda t: None if t is None else t.data_ptr()

    def softmax(segptr=segptr, row_of=row_of, n_seg=n_seg, seg_first=seg_first, n_rows=n_rows, s=case["s"], Ns=case["s"].numel(), alpha=alpha,
                ws=ws, ws_bytes=ws.numel() * 4):
        return lib.ncf_gat_edge_softmax(P(segptr), P(row_of), n_seg, P(seg_first), n_rows, P(case["col"]), P(case["attr"]), P(case["keep"]), P(s), Ns,
                                        P(alpha), P(coef), P(ws), ws_bytes, None)

    def grad(D=8, p=0.0, n_seg=n_seg, z=case["z"], dY=case["dY"], ws=ws, ws_bytes=ws.numel() * 4, ldz=8, seg_first=seg_first):
        return lib.ncf_gat_edge_grad(P(segptr), P(row_of), n_seg, P(seg_first), n_rows, P(case["col"]), P(case["attr"]), P(alpha), P(dY), 8, P(z),
                                     case["z"].shape[0], ldz, D, p, 1, P(dl), P(ws), ws_bytes, None)

    def reduce(n_seg=n_rows, val=dl, out=ds, n_val=E):
        return lib.ncf_gat_source_reduce(P(case["rowptr"]), None, n_seg, P(case["col"]), P(val), n_val, P(out), n_rows, None, None)

    bad = [softmax(s=None), softmax(alpha=None), softmax(n_seg=-1), softmax(n_rows=-2), softmax(Ns=-1), softmax(seg_first=None), softmax(ws=None),
           softmax(segptr=None), softmax(row_of=None),
           grad(D=6), grad(D=0), grad(p=1.0), grad(p=-0.1), grad(p=float("nan")), grad(p=float("inf")), grad(z=None), grad(dY=None), grad(ws=None),
           grad(n_seg=-1), grad(ldz=6), grad(seg_first=None),
           reduce(n_seg=-1), reduce(val=None), reduce(out=None), reduce(n_val=-1), reduce(n_seg=n_rows + 1)]
    assert all(rc == native.NCF_EINVAL for rc in bad), bad
    assert b"ncf_gat_source_reduce" in lib.ncf_last_error()
    assert softmax(ws_bytes=8) == native.NCF_EWORKSPACE and grad(ws_bytes=8) == native.NCF_EWORKSPACE
    assert b"ncf_gat_edge_grad" in lib.ncf_last_error() and b"workspace" in lib.ncf_last_error()
    assert grad(D=260) == native.NCF_EUNSUPPORTED
    torch.cuda.synchronize()
    for t in (alpha, coef, dl, ds, ws):
        assert bool((t == 7.0).all())
    with pytest.raises(TypeError):
        native.gat_edge_softmax(segptr, row_of, seg_first, n_rows, case["col"], case["attr"], case["keep"].double(), case["s"])
    with pytest.raises(TypeError):
        native.gat_edge_softmax(segptr, row_of, None, n_rows, case["col"], case["attr"], case["keep"], case["s"])
    with pytest.raises(native.NativeError):
        native.gat_edge_grad(segptr, row_of, seg_first, n_rows, case["col"], case["attr"], case["keep"], case["dY"], case["z"], 1.5, 1)
    assert softmax() == native.NCF_OK                                          # the same arguments, accepted
    torch.cuda.synchronize()
    assert R.same_bits(alpha, G.exact_alpha(_cpu(case)))


# ------------------------------------------------------------------------------------------------------ 5. training step
def _train_graph(n_items, n_users, n_inter, seed, binary=False):
    """The recipe of tests/test_gpu_training.py::_train_graph (restated: test modules do not import each other's helpers)."""
    g = torch.Generator().manual_seed(seed)
    key = torch.unique(torch.randint(0, n_users, (n_inter,), generator=g) * n_items + (torch.rand(n_inter, generator=g) ** 2 * n_items).long())
    u, i = key // n_items + n_items, key % n_items
    a = None if binary else torch.randn(u.numel(), generator=g)
    return torch.stack([u, i]), torch.stack([i, u]), a


def _graph_data(u2i, i2u, a, n_items, n_users, dev, dt=torch.float32):
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphData
    return GraphData(user2item_edge_index=u2i.to(dev), item2user_edge_index=i2u.to(dev), user2item_edge_attr=None if a is None else a.to(dev).to(dt),
                     item2user_edge_attr=None if a is None else a.clone().to(dev).to(dt), num_items=n_items, num_users=n_users)


def _np(t):
    return None if t is None else t.numpy()


def _draw():
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


def _att_params(model, hetero):
    conv = model.gnn_convs[0]
    return [conv.item2user_AttNet[0], conv.user2item_AttNet[0]] if hetero else [conv.AttNet[0]]


def _compare_step(m_gpu, m_cpu, loss_g, loss_c, hetero, D, rtol=5e-5):
    """Loss within 2e-5 relative, every parameter gradient within rtol of its scale; AttNet's bias and destination half get a
    gradient that is exactly zero on the HIP model (on the CPU model they are rounding noise, held to the weight's bar)."""
    lc, lg = float(loss_c.detach()), float(loss_g.detach())
    print(f"loss hip {lg:.9g} cpu {lc:.9g} rel {abs(lg - lc) / abs(lc):.3e}")
    assert abs(lg - lc) <= 2e-5 * abs(lc)
    att_bias = {id(a.bias) for a in _att_params(m_gpu, hetero)}
    scales = {}
    for (n, q), (_, r) in zip(m_gpu.named_parameters(), m_cpu.named_parameters()):
        assert q.grad is not None, n
        x, ref = q.grad.cpu().double(), r.grad.double()
        scale = float(ref.abs().max()) + 1e-30
        scales[n] = scale
        err = float((x - ref).abs().max())
        print(f"  grad {n}: max abs err {err:.3e} scale {scale:.3e}")
        if id(q) in att_bias:
            assert bool((q.grad == 0).all()), n
            assert float(ref.abs().max()) <= rtol * scales[n.replace("bias", "weight")], n
        else:
            assert err <= rtol * scale, f"{n}: max abs err {err:.3e} vs scale {scale:.3e}"
    for a in _att_params(m_gpu, hetero):
        assert a.weight.grad.shape == (1, 2 * D)
        assert bool((a.weight.grad[:, D:] == 0).all()) and float(a.weight.grad[:, :D].abs().max()) > 0


def _spies(monkeypatch, B):
    from deeprecommendation_amd import native
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF
    calls = {"hip": [], "edge_keep": [], "big_dropout": 0, "choice": 0}
    real_hip, real_keep, real_dropout, real_choice = GraphNCF._forward_train_hip, native.edge_keep, torch.nn.functional.dropout, np.random.choice

    def spy_hip(self, *args, **kw):
        out = real_hip(self, *args, **kw)
        calls["hip"].append(out)
        return out

    def spy_keep(*args, **kw):
        out = real_keep(*args, **kw)
        calls["edge_keep"].append(out)
        return out

    def spy_dropout(x, *args, **kw):
        if x.dim() == 1 and x.numel() > B:                           # an edge mask (the layers' own dropouts see 2-D tensors)
            calls["big_dropout"] += 1
        return real_dropout(x, *args, **kw)

    def spy_choice(*args, **kw):
        calls["choice"] += 1
        return real_choice(*args, **kw)

    monkeypatch.setattr(GraphNCF, "_forward_train_hip", spy_hip)
    monkeypatch.setattr(native, "edge_keep", spy_keep)
    monkeypatch.setattr(torch.nn.functional, "dropout", spy_dropout)
    monkeypatch.setattr(np.random, "choice", spy_choice)
    return calls


def _run_step(gpu, monkeypatch, hetero, binary, concat, dot, message_dropout, node_dropout, graph_shape=(40, 300, 4000, 3), seg_len=None):
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF, PreparedGraph
    n_items, n_users, draws, gseed = graph_shape
    D, B = 64, 256
    N = n_items + n_users
    u2i, i2u, a = _train_graph(n_items, n_users, draws, seed=gseed, binary=binary)
    E1 = u2i.shape[1]
    torch.manual_seed(5)
    m = GraphNCF(item_dim=n_items, user_dim=n_users, num_gnn_layers=2, hetero=hetero, node_emb=D, mlp_dense_layers=[128], dropout_rate=0.0,
                 concat=concat, use_dot_product=dot, message_dropout=message_dropout, node_dropout=node_dropout, convType="LightGAT").train()
    with torch.no_grad():                                            # scores of spread ~ 1: a softmax that is not uniform
        for att in _att_params(m, hetero):
            att.weight.mul_(8.0)
    m_gpu = copy.deepcopy(m).to(gpu).train()
    m_cpu = copy.deepcopy(m).train()
    m_cpu.message_dropout = m_cpu.node_dropout = None
    g = torch.Generator().manual_seed(6)
    pick = torch.randint(0, E1, (B,), generator=g)                   # batch pairs that ARE edges: the target masking has work to do
    users, items = u2i[0][pick], u2i[1][pick]
    y = torch.rand(B, 1, generator=g) * 5

    torch.manual_seed(91)                                            # dropout_rate = 0: no seed0; then node_seed, then seed
    node_seed = _draw() if node_dropout else None
    seed = _draw() if message_dropout else 0
    nmask = node_keep(node_seed, N, torch.cat([items, users]).numpy(), node_dropout) if node_dropout else None
    na = _np(a)
    k1, k2 = keep_lists(_np(u2i), _np(i2u), na, na, N, None, None, message_dropout or 0.0, seed, nmask)
    k1, k2 = torch.from_numpy(k1), torch.from_numpy(k2)
    kept_graph = _graph_data(u2i[:, k1], i2u[:, k2], None, n_items, n_users, "cpu")
    if a is not None:
        kept_graph.user2item_edge_attr, kept_graph.item2user_edge_attr = a[k1], a[k2]
    loss_c = torch.nn.functional.mse_loss(m_cpu(kept_graph, users, items, "cpu", True), y, reduction="sum")
    loss_c.backward()

    calls = _spies(monkeypatch, B)
    graph_gpu = _graph_data(u2i, i2u, a, n_items, n_users, gpu)
    if seg_len is not None:
        prep = PreparedGraph(graph_gpu, hetero, seg_len=seg_len)
        assert prep.row_of is not None and int(prep.counts.max()) > 10 * seg_len
        graph_gpu._prepared[("prep", hetero)] = prep
    torch.manual_seed(91)
    out_g = m_gpu(graph_gpu, users.to(gpu), items.to(gpu), gpu, True)
    assert out_g.requires_grad
    loss_g = torch.nn.functional.mse_loss(out_g, y.to(gpu), reduction="sum")
    loss_g.backward()
    assert len(calls["hip"]) == 1 and isinstance(calls["hip"][0], torch.Tensor)
    assert len(calls["edge_keep"]) == 1 and calls["big_dropout"] == 0 and calls["choice"] == 0
    keep_g, deg_g = calls["edge_keep"][0]
    # the indicator: attr = None to the kernel, the slots those of the graph's own lists (symmetric when weighted)
    kk1, kk2 = keep_lists(_np(u2i), _np(i2u), na, na, N, _np(users), _np(items), message_dropout or 0.0, seed, nmask)
    order = np.argsort(np.concatenate([_np(u2i)[1], _np(i2u)[1]]), kind="stable")
    w_ref = np.concatenate([kk1, kk2]).astype(np.float32)[order]
    if a is None:
        assert np.array_equal(w_ref, edge_keep_ref(_np(u2i), _np(i2u), None, None, N, _np(users), _np(items), message_dropout or 0.0, seed, nmask)[0])
    assert np.array_equal(keep_g.cpu().numpy().view(np.uint32), w_ref.view(np.uint32))
    assert set(np.unique(keep_g.cpu().numpy())) <= {0.0, 1.0} and int((keep_g == 0).sum()) > 0
    _compare_step(m_gpu, m_cpu, loss_g, loss_c, hetero, D)
    return m_gpu, graph_gpu, users, items, calls


@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("message_dropout,node_dropout", [(None, None), (0.2, None), (None, 0.3), (0.2, 0.3)])
@pytest.mark.parametrize("binary,concat,dot", [(False, False, False), (True, True, False), (False, False, True)])
def test_lightgat_training_step_on_the_hip_blocks(gpu, monkeypatch, hetero, message_dropout, node_dropout, binary, concat, dot):
    """GraphNCF / LightGAT, 2 layers, in .train() on CUDA, with and without node / message dropout: the step runs on the HIP blocks
    (spies: _forward_train_hip returned a tensor, native.edge_keep ran once, no E-sized F.dropout, no np.random.choice).  The drawn
    seeds and the kept edge lists are restated with edge_keep_ref, and a CPU copy of the model WITHOUT dropout runs on the graph of
    kept edges with the same target masking: loss within 2e-5 relative, every parameter gradient within 5e-5 of its scale, AttNet's
    bias and destination half exactly zero."""
    m_gpu, graph_gpu, users, items, calls = _run_step(gpu, monkeypatch, hetero, binary, concat, dot, message_dropout, node_dropout)
    m_gpu.train_with_torch_ops = True                                # keeps selecting the torch path
    m_gpu(graph_gpu, users.to(gpu), items.to(gpu), gpu, True)
    assert len(calls["hip"]) == 1 and len(calls["edge_keep"]) == 1
    assert calls["big_dropout"] == (0 if not message_dropout else (2 if binary else 1)) and calls["choice"] == (1 if node_dropout else 0)


def test_lightgat_training_step_with_split_rows(gpu, monkeypatch):
    """The hub graph (50 items, 2000 users, 60 000 draws) prepared with seg_len = 64: split rows pass through the whole step."""
    _run_step(gpu, monkeypatch, False, False, False, False, 0.2, 0.3, graph_shape=(50, 2000, 60000, 8), seg_len=64)


class _MaskDropout(torch.nn.Module):
    """Stands where the conv's nn.Dropout stood in the float64 CPU module: row k of call c is multiplied by the restated mask of
    entry ids[k] under seed0 + 7919 c."""

    def __init__(self, p, seed0, ids):
        super().__init__()
        self.p, self.seed0, self.ids, self.calls = p, seed0, ids, 0

    def forward(self, x):
        assert x.shape[0] == len(self.ids)
        f = mask_factor64(self.seed0 + 7919 * self.calls, self.ids, x.shape[1], self.p)
        self.calls += 1
        return x * f


def test_lightgat_training_step_with_feature_dropout(gpu):
    """dropout_rate = 0.2: the per-(edge, feature) dropout inside the per-edge Linear (p = 0.1) is regenerated in the forward SpMM,
    its transpose and the per-edge gradient.  Forward of one aggregation against spmm_dropout64 fed with the kernel's own
    coefficients; loss and gradients of the step against the float64 CPU module whose W[1] is the restated mask (row k of a call is
    the k-th kept edge of cat(u2i, i2u); its entry id is the edge's position in the CSR by destination)."""
    from deeprecommendation_amd import native
    from deeprecommendation_amd.autograd import GatSpmmFn
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF, PreparedGraph
    n_items, n_users, D, B = 40, 300, 64, 256
    u2i, i2u, a = _train_graph(n_items, n_users, 4000, seed=3)
    N, E1 = n_items + n_users, u2i.shape[1]
    torch.manual_seed(5)
    m = GraphNCF(item_dim=n_items, user_dim=n_users, num_gnn_layers=2, hetero=False, node_emb=D, mlp_dense_layers=[128], dropout_rate=0.2,
                 convType="LightGAT").train()
    for mod in m.MLP:                                                # the MLP's dropouts draw from torch's Philox stream: not tested here
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    with torch.no_grad():
        m.gnn_convs[0].AttNet[0].weight.mul_(8.0)
    p = float(m.gnn_convs[0].W[1].p)
    assert p == 0.1
    m_gpu = copy.deepcopy(m).to(gpu).train()
    m_cpu = copy.deepcopy(m).double().train()
    g = torch.Generator().manual_seed(6)
    pick = torch.randint(0, E1, (B,), generator=g)
    users, items = u2i[0][pick], u2i[1][pick]
    y = torch.rand(B, 1, generator=g) * 5
    order = torch.argsort(torch.cat([u2i[1], i2u[1]]), stable=True)
    pos = torch.empty_like(order)
    pos[order] = torch.arange(order.numel())
    key = users * N + items
    keep1, keep2 = ~torch.isin(u2i[0] * N + u2i[1], key), ~torch.isin(i2u[1] * N + i2u[0], key)
    ids = np.concatenate([pos[:E1][keep1].numpy(), pos[E1:][keep2].numpy()])
    torch.manual_seed(91)
    seed0 = _draw()
    m_cpu.gnn_convs[0].W[1] = _MaskDropout(p, seed0, ids)
    loss_c = torch.nn.functional.mse_loss(m_cpu(_graph_data(u2i, i2u, a, n_items, n_users, "cpu", torch.float64), users, items, "cpu", True),
                                          y.double(), reduction="sum")
    assert m_cpu.gnn_convs[0].W[1].calls == 2
    loss_c.backward()
    graph_gpu = _graph_data(u2i, i2u, a, n_items, n_users, gpu)
    torch.manual_seed(91)
    loss_g = torch.nn.functional.mse_loss(m_gpu(graph_gpu, users.to(gpu), items.to(gpu), gpu, True), y.to(gpu), reduction="sum")
    loss_g.backward()
    _compare_step(m_gpu, m_cpu, loss_g, loss_c, False, D)
    # forward of one aggregation with the mask, against float64 on the kernel's own coefficients
    prep = graph_gpu._prepared[("prep", False)]
    gen = _gen(gpu, 8)
    z, s = torch.randn(N, D, generator=gen, device=gpu), torch.randn(N, 1, generator=gen, device=gpu)
    keep = prep.batch_keep(users.to(gpu), items.to(gpu))
    yk = GatSpmmFn.apply(z, s, prep, keep, (p, 4242))
    seg = prep.softmax_segments()
    _, coef = native.gat_edge_softmax(prep.segptr, prep.row_of, None if seg is None else seg[2], N, prep.col, prep.attr, keep, s.view(-1).contiguous())
    ref, mag = spmm_dropout64(prep.rowptr.cpu(), prep.col.cpu(), coef.cpu(), z.cpu(), N, None, 4242, p)
    n_r = (prep.rowptr[1:] - prep.rowptr[:-1]).cpu().double()[:, None]
    ok, used, *_ = R.bound_check(yk.cpu(), ref, (n_r + 9) * R.U24 * mag)       # the SpMM's (n_r + 8) bound and the mask's scale product
    print(f"forward with the mask: worst fraction of the bound {used:.3f}")
    assert ok


@pytest.mark.parametrize("width", [8, 192, 320, 6])
def test_ordered_readout_gather(gpu, width):
    """GatherPairOrderedFn: forward = the two row gathers side by side; backward = each table row's gradient rows summed, against
    float64 index_add_ at (count + 8) 2^-24 of the magnitudes, with heavy duplicates, an id out of range and untouched rows.  Widths
    that are a multiple of 4 (320: two column blocks) repeat bit for bit; 6 takes the scatter kernel and is only held to the bound."""
    from deeprecommendation_amd import native
    from deeprecommendation_amd.autograd import GatherPairOrderedFn
    gen = _gen(gpu, 40 + width)
    rows, B = 500, 2000
    table = torch.randn(rows, width, generator=gen, device=gpu).requires_grad_()
    ia = torch.randint(0, 40, (B,), generator=gen, device=gpu)                  # 40 hot rows: ~50 duplicates each
    ib = torch.randint(100, rows, (B,), generator=gen, device=gpu)
    dX = torch.randn(B, 2 * width, generator=gen, device=gpu)
    out = GatherPairOrderedFn.apply(table, ia, ib)
    assert torch.equal(out, torch.cat((table[ia], table[ib]), dim=1))
    (g1,) = torch.autograd.grad(out, table, dX, retain_graph=True)
    (g2,) = torch.autograd.grad(out, table, dX)
    ref = torch.zeros(rows, width, dtype=torch.float64, device=gpu).index_add_(0, ia, dX[:, :width].double()).index_add_(0, ib, dX[:, width:].double())
    mag = torch.zeros(rows, width, dtype=torch.float64, device=gpu).index_add_(0, ia, dX[:, :width].double().abs()).index_add_(0, ib, dX[:, width:].double().abs())
    cnt = (torch.bincount(ia, minlength=rows) + torch.bincount(ib, minlength=rows)).double()[:, None]
    ok, used, *_ = R.bound_check(g1, ref, (cnt + 8) * R.U24 * mag)
    print(f"ordered gather width {width}: worst fraction of the bound {used:.3f}")
    assert ok and bool((g1[40:100] == 0).all())
    if width % 4 == 0:
        assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
        bad = ia.clone()
        bad[0] = rows + 3                                                      # reported by the gather, no gradient row
        (g3,) = torch.autograd.grad(GatherPairOrderedFn.apply(table, bad, ib), table, dX)
        ref3 = ref.clone()
        ref3[ia[0]] -= dX[0, :width].double()
        assert R.bound_check(g3, ref3, (cnt + 8) * R.U24 * mag)[0]
        with pytest.raises(IndexError):
            native.check_oob(gpu)


# ---------------------------------------------------------------------------------------------------- 6. train_model
def _toy_files(n=6000, U=300, I=120, seed=0):
    """The toy interaction files of tests/test_gpu_training.py (recipe restated)."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    u, i = rng.integers(1, U + 1, n), rng.integers(1, I + 1, n)
    r = np.clip(np.round(((u % 5) + (i % 3)) * 0.5 + 1 + rng.normal(0, 0.2, n), 1), 0.5, 5.0)
    frame = pd.DataFrame({"userId": u, "movieId": i, "rating": r})
    cut = n * 4 // 5
    return frame.iloc[:cut].reset_index(drop=True), frame.iloc[cut:].reset_index(drop=True), U, I


@pytest.mark.parametrize("resident", [True, False])
def test_train_model_lightgat_with_message_dropout(gpu, tmp_path, monkeypatch, resident):
    """One epoch of train_model with convType='LightGAT' and message_dropout = 0.2: every step takes the HIP path (spy), the losses
    are finite and a second run under the same seed gives exactly the same losses."""
    from deeprecommendation_amd.content_providers.index_providers import IndexGraphProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.gnn_datasets import GraphPointwiseDataset
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF
    from deeprecommendation_amd.neural_collaborative_filtering.train import train_model
    tr, va, U, I = _toy_files()
    gcp = IndexGraphProvider(np.arange(1, U + 1), np.arange(1, I + 1), tr.userId.values, tr.movieId.values, tr.rating.values)
    real_hip = GraphNCF._forward_train_hip
    steps = []

    def spy_hip(self, *args, **kw):
        out = real_hip(self, *args, **kw)
        steps.append(isinstance(out, torch.Tensor))
        return out

    monkeypatch.setattr(GraphNCF, "_forward_train_hip", spy_hip)
    losses = []
    for run in range(2):
        torch.manual_seed(0)
        np.random.seed(0)
        m = GraphNCF(item_dim=I, user_dim=U, num_gnn_layers=2, hetero=True, node_emb=64, mlp_dense_layers=[128], message_dropout=0.2,
                     convType="LightGAT")
        mm = train_model(m, GraphPointwiseDataset(tr, gcp), GraphPointwiseDataset(va, gcp), lr=2e-3, weight_decay=1e-5, batch_size=512,
                         val_batch_size=1024, early_stop=False, final_model_path=str(tmp_path / f"f{run}.pt"),
                         checkpoint_model_path=str(tmp_path / f"c{run}.pt"), max_epochs=1, device=gpu, resident=resident, verbose=False)
        assert len(mm["train_loss"]) == 1 and np.isfinite(mm["train_loss"]).all() and np.isfinite(mm["val_loss"]).all()
        losses.append((list(mm["train_loss"]), list(mm["val_loss"])))
    assert len(steps) == 2 * -(-len(tr) // 512) and all(steps)
    assert losses[0] == losses[1]
