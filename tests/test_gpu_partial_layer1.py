"""GPU tests (MI355X) of the partial first layer: native.layer1_partial + native.score_fused_partial, and its automatic use
by BasicNCF.  The contract is bit-identity with native.score_fused (and so with the kernel-order C oracle): every comparison
below is torch.equal, on int32 views where a NaN can occur."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def _mlp(g, dims):
    ws = [torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    bs = [torch.randn(dims[i + 1], generator=g) * 0.1 for i in range(len(dims) - 1)]
    return ws, bs


def _case(native, gpu, EA, EB, hidden, rowsA=900, rowsB=400, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * EA + EB + len(hidden))
    ta = torch.randn(rowsA, EA, generator=g) * 0.5
    tb = torch.randn(rowsB, EB, generator=g) * 0.5
    ws, bs = _mlp(g, [EA + EB] + hidden + [1])
    packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
    return g, ta, tb, ws, bs, packed


SHAPES = [(E, E, h) for E in (32, 64, 128) for h in ([256, 128], [256], [128, 64])
          if (2 * E, h[-1]) != (256, 64)] + [(32, 96, [256, 128]), (96, 32, [256, 128])]   # 256-128-64-1 has no fused instance


@pytest.mark.parametrize("EA,EB,hidden", SHAPES)
def test_partial_equals_fused_and_c_oracle(native, gpu, EA, EB, hidden):
    """Every shape at every dispatch of ncf_score_fused_partial: 1 and 999 pairs go to ncf_score_fused's small kernel, 40 000
    pairs (1250 tiles) to the partial kernel plus a ragged tail on the small kernel, 65 536 pairs to the partial kernel alone, so
    the partial kernel instance of every shape runs (a round is 4 x CUs = 1024 tiles on an MI355X).  The kernel-order C oracle
    checks the first 2048 pairs."""
    from oracle import c_oracle
    g, ta, tb, ws, bs, packed = _case(native, gpu, EA, EB, hidden)
    assert native.partial_supported(EA, EB, packed)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    assert P.shape == (ta.shape[0] + 1, hidden[0])
    for B in (1, 999, 40000, 65536):
        ia = torch.randint(0, ta.shape[0], (B,), generator=g)
        ib = torch.randint(0, tb.shape[0], (B,), generator=g)
        out = native.score_fused_partial(P, tag, ia.to(gpu), tbg, ib.to(gpu), packed)
        assert torch.equal(out, native.score_fused(tag, ia.to(gpu), tbg, ib.to(gpu), packed)), B
        n = min(B, 2048)
        assert torch.equal(out[:n].cpu(), c_oracle.score_fused_f32(ta, tb, ia[:n], ib[:n], ws, bs)), B


@pytest.mark.parametrize("EA,EB,hidden", [(64, 64, [256, 128]), (32, 96, [256, 128]), (64, 64, [128, 64]), (128, 128, [256])])
@pytest.mark.parametrize("B", [1, 999, 30000, 40000, 65536, 98304])
def test_partial_equals_fused_at_every_dispatch(native, gpu, EA, EB, hidden, B):
    """Small batches, the ragged-round split and full rounds all return score_fused's bits."""
    g, ta, tb, ws, bs, packed = _case(native, gpu, EA, EB, hidden, rowsA=20000, rowsB=5000, seed=B)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = torch.randint(0, ta.shape[0], (B,), generator=g).to(gpu)
    ib = torch.randint(0, tb.shape[0], (B,), generator=g).to(gpu)
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed)
    assert torch.equal(out, native.score_fused(tag, ia, tbg, ib, packed))


def test_partial_table_close_to_float64(native, gpu):
    """Sanity check of P itself: tabA . W1[:, :EA]^T + b1 in float64 (1e-5 with an absolute floor, like test_gpu_basic)."""
    g, ta, tb, ws, bs, packed = _case(native, gpu, 64, 64, [256, 128], rowsA=3000)
    P = native.layer1_partial(ta.to(gpu), packed).cpu().double()
    ref = ta.double() @ ws[0][:, :64].double().t() + bs[0].double()
    ref_bad = bs[0].double().unsqueeze(0)   # the out-of-range row: row 0 times zero
    ref = torch.cat([ref, ref_bad])
    tol = 1e-5 * ref.abs() + 1e-6 * ref.abs().max()
    assert bool(((P - ref).abs() <= tol).all()), f"max abs err {(P - ref).abs().max().item():.3e}"


@pytest.mark.parametrize("B", [999, 40000])
def test_out_of_range_ids_match_fused_and_set_flag(native, gpu, B):
    g, ta, tb, ws, bs, packed = _case(native, gpu, 64, 64, [256, 128], rowsA=5000, rowsB=3000, seed=5)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = torch.randint(0, 5000, (B,), generator=g)
    ib = torch.randint(0, 3000, (B,), generator=g)
    ia[::97] = 5000 + torch.arange(ia[::97].numel())
    ia[5::89] = -3
    ib[3::71] = 3000
    ib[7::83] = -1
    ia, ib = ia.to(gpu), ib.to(gpu)
    native._oob_flag(gpu).zero_()
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    ref = native.score_fused(tag, ia, tbg, ib, packed)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize("B", [999, 65536])
def test_nonfinite_row0_and_negative_zero_bias(native, gpu, B):
    """Row 0 of A holding inf / NaN (read, times zero, for an out-of-range id) and a -0.0 entry of b1: same bits as score_fused."""
    g = torch.Generator().manual_seed(11)
    ta = torch.randn(4000, 64, generator=g) * 0.5
    tb = torch.randn(2000, 64, generator=g) * 0.5
    ta[0, 3] = float("inf")
    ta[0, 17] = float("nan")
    ta[0, 40] = -float("inf")
    ws, bs = _mlp(g, [128, 256, 128, 1])
    bs[0][5] = -0.0
    bs[0][6] = 0.0
    packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = torch.randint(0, 4000, (B,), generator=g)
    ib = torch.randint(0, 2000, (B,), generator=g)
    ia[::50] = 0
    ia[1::61] = 4000      # out of range: row 0 times zero
    ia, ib = ia.to(gpu), ib.to(gpu)
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed)
    ref = native.score_fused(tag, ia, tbg, ib, packed)
    native._oob_flag(gpu).zero_()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(P[-1].view(torch.int32), native.layer1_partial(tag, packed)[-1].view(torch.int32))


# ----------------------------------------------------------------------------------------------------------- model selection
def _basic(gpu, U=40000, I=3000, E=64, hidden=(256, 128), seed=0):
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    torch.manual_seed(seed)
    return BasicNCF(item_dim=I, user_dim=U, item_emb=E, user_emb=E, mlp_dense_layers=list(hidden)).eval().to(gpu)


def _partials(model):
    return [v for k, v in model._native_cache.items() if isinstance(k, tuple) and k[0] == "partial"]


def _built(model):
    return any(e["P"] is not None for e in _partials(model))


def test_basic_ncf_builds_on_second_forward_and_matches(gpu):
    model = _basic(gpu)
    g = torch.Generator().manual_seed(3)
    B = 65536
    batches = [(torch.randint(0, 40000, (B,), generator=g).to(gpu), torch.randint(0, 3000, (B,), generator=g).to(gpu)) for _ in range(4)]
    with torch.no_grad():
        outs = [model(*batches[0])]
        assert not _built(model)
        for u, i in batches[1:]:
            outs.append(model(u, i))
        assert _built(model)
        model.set_partial_first_layer(False)
        refs = [model(u, i) for u, i in batches]
        assert not _partials(model) or not _built(model)
    for o, r in zip(outs, refs):
        assert torch.equal(o, r)


def test_basic_ncf_small_batches_never_build(gpu):
    model = _basic(gpu)
    u = torch.randint(0, 40000, (1000,), device=gpu)
    i = torch.randint(0, 3000, (1000,), device=gpu)
    with torch.no_grad():
        for _ in range(3):
            model(u, i)
    assert not _built(model)


def test_forced_mode_and_in_place_update_rebuild(gpu):
    model = _basic(gpu).set_partial_first_layer(True)
    u = torch.randint(0, 40000, (40000,), device=gpu)
    i = torch.randint(0, 3000, (40000,), device=gpu)
    with torch.no_grad():
        a = model(u, i)
        assert _built(model)
        P0 = _partials(model)[0]["P"]
        model.MLP[0].weight.mul_(1.25)               # in-place weight update: new version, P rebuilt
        b = model(u, i)
        assert _built(model) and _partials(model)[0]["P"] is not P0
        model.set_partial_first_layer(False)
        assert torch.equal(b, model(u, i))
    assert not torch.equal(a, b)


def test_cap_of_zero_falls_back(gpu):
    model = _basic(gpu).set_partial_first_layer(True, max_bytes=0)
    u = torch.randint(0, 40000, (40000,), device=gpu)
    i = torch.randint(0, 3000, (40000,), device=gpu)
    with torch.no_grad():
        out = model(u, i)
        out2 = model(u, i)
        assert not _built(model)
        model.set_partial_first_layer(False)
        assert torch.equal(out, model(u, i)) and torch.equal(out2, out)


def test_dense_profile_path_never_takes_partial(gpu):
    model = _basic(gpu, U=300, I=200).set_partial_first_layer(True)
    xu = torch.rand(40000, 300, device=gpu)
    xi = torch.rand(40000, 200, device=gpu)
    with torch.no_grad():
        model(xu, xi)
        model(xu, xi)
    assert not _built(model)


def test_attention_ncf_never_takes_partial(gpu):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.manual_seed(1)
    F, I, Ba = 40, 90, 96
    att = AttentionNCF(item_dim=F, item_emb=64, user_emb=64, att_dense=128, mlp_dense_layers=[256, 128]).eval().to(gpu)
    att.set_partial_first_layer(True)
    rated, cand = torch.rand(I, F, device=gpu), torch.rand(Ba, F, device=gpu)
    rows = torch.zeros(8, I)
    m = torch.rand(8, I) < 0.4
    rows[m] = 1.0
    user_matrix = rows.repeat_interleave(Ba // 8, dim=0).to(gpu)
    with torch.no_grad():
        a = att(cand, rated, user_matrix)
        b = att(cand, rated, user_matrix)
    assert torch.equal(a, b)
    assert not _built(att)


def test_captured_graph_replays_identical_outputs(gpu):
    model = _basic(gpu)
    g = torch.Generator().manual_seed(9)
    B = 65536
    u = torch.randint(0, 40000, (B,), generator=g).to(gpu)
    i = torch.randint(0, 3000, (B,), generator=g).to(gpu)
    with torch.no_grad():
        model(u, i)
        eager = model(u, i)                          # second forward: P built
        assert _built(model)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(u, i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            cap = model(u, i)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, eager)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, eager)


def test_capture_before_build_never_builds(gpu):
    model = _basic(gpu).set_partial_first_layer(True)
    u = torch.randint(0, 40000, (40000,), device=gpu)
    i = torch.randint(0, 3000, (40000,), device=gpu)
    with torch.no_grad():
        model._refresh()
        model._table("user", model.user_embeddings[0])
        model._table("item", model.item_embeddings[0])
        model._packed_mlp()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            cap = model(u, i)
        assert not _built(model)
        gr.replay()
        torch.cuda.synchronize()
        model.set_partial_first_layer(False)
        assert torch.equal(cap, model(u, i))


def test_graph_ncf_mlp_partial_matches(gpu):
    """GraphNCF-MLP scores cat(item, user) from ONE cached table (`combined`): tabA and tabB are the same table and P covers
    item and user rows alike.  The automatic path builds P on the second forward; every output equals the plain path's."""
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF, GraphData
    from test_gpu_graph import _bipartite
    n_items, n_users = 3000, 2000
    u2i, i2u, a1, a2 = _bipartite(n_items, n_users, 40000, seed=6)
    torch.manual_seed(6)
    m = GraphNCF(item_dim=n_items, user_dim=n_users, num_gnn_layers=2, hetero=True, node_emb=64,
                 mlp_dense_layers=[256, 128]).eval().to(gpu)
    graph = GraphData(user2item_edge_index=u2i, item2user_edge_index=i2u, user2item_edge_attr=a1, item2user_edge_attr=a2,
                      num_items=n_items, num_users=n_users)
    g = torch.Generator().manual_seed(6)
    B = 65536
    batches = [(torch.randint(n_items, n_items + n_users, (B,), generator=g).to(gpu),
                torch.randint(0, n_items, (B,), generator=g).to(gpu)) for _ in range(3)]
    with torch.no_grad():
        outs = [m(graph, *batches[0])]
        assert not _built(m)
        outs += [m(graph, u, i) for u, i in batches[1:]]
        assert _built(m)
        m.set_partial_first_layer(False)
        refs = [m(graph, u, i) for u, i in batches]
    for o, r in zip(outs, refs):
        assert torch.equal(o, r)
