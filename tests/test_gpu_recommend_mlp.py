"""GPU: top_k_items on an MLP readout (BasicNCF, GraphNCF with use_dot_product=False) ranks through the fused MLP score-and-select
kernel (native.mlp_topk) by default, bit-equal to score-then-select (fused=False) and in agreement with the CPU oracle; models
outside the kernel's limits (folded first layer, bf16 scoring, k > 128, an MLP without a fused instance) fall back to
score-then-select with the same result."""
import numpy as np
import pytest
import torch

from oracle import ncf_oracle as O
from test_gpu_graph import _bipartite
from test_gpu_recommend import _check_ranked
from test_topk_cpu import topk_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture
def mlp_calls(monkeypatch):
    """Counts native.mlp_topk calls (the fused route) while the test runs."""
    from deeprecommendation_amd import native
    calls = []
    real = native.mlp_topk

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(native, "mlp_topk", counted)
    return calls


def _equal(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)


def _basic(gpu, U, I, eu, ei, layers, seed):
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    torch.manual_seed(seed)
    m = BasicNCF(item_dim=I, user_dim=U, item_emb=ei, user_emb=eu, mlp_dense_layers=layers).eval()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to(gpu), state


def _exclude(rng, B, I, gpu):
    lists = [rng.integers(0, I, int(rng.integers(0, I // 3))).tolist() for _ in range(B)]
    lists[0] = list(range(I))                                      # a user who has rated everything: count 0
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64, device=gpu)
    col = torch.tensor(np.concatenate([np.asarray(x, np.int64) for x in lists]), dtype=torch.int32, device=gpu)
    return lists, (rowptr, col)


@pytest.mark.parametrize("with_exclude", [False, True])
@pytest.mark.parametrize("with_items", [False, True])
def test_basic_ncf_default_route_is_fused_and_bit_equal(gpu, mlp_calls, with_exclude, with_items):
    """cfg-2 widths (E = 64 + 64, MLP 128 -> 256 -> 128 -> 1)."""
    from deeprecommendation_amd import top_k_items
    U, I, k = 3000, 5000, 100
    m, state = _basic(gpu, U, I, 64, 64, [256, 128], 1)
    rng = np.random.default_rng(int(with_exclude) + 2 * int(with_items))
    users = torch.as_tensor(rng.integers(0, U, 300), device=gpu)
    items = torch.as_tensor(rng.integers(0, I, 2500), device=gpu) if with_items else None
    n_cols = 2500 if with_items else I
    lists, exclude = _exclude(rng, 300, n_cols, gpu) if with_exclude else (None, None)
    got = top_k_items(m, users, k, item_ids=items, exclude=exclude)
    assert len(mlp_calls) == 1
    ref = top_k_items(m, users, k, item_ids=items, exclude=exclude, fused=False)
    assert len(mlp_calls) == 1
    _equal(got, ref)
    # and the CPU oracle
    ids = items.cpu() if with_items else torch.arange(I)
    u = users.cpu().repeat_interleave(n_cols)
    scores = O.basic_ncf_forward_indexed(state, u, ids.repeat(300)).view(300, n_cols)
    rs, ri, rn = topk_oracle(scores, k, lists)
    s, pos, n = (t.cpu().numpy() for t in got)
    scale = float(scores.abs().max())
    for r in range(300):
        rid = ri[r].numpy()
        if with_items:
            rid = np.where(rid >= 0, ids.numpy()[np.clip(rid, 0, None)], rid)
        _check_ranked(s[r], pos[r], int(n[r]), rs[r].numpy(), rid, int(rn[r]), scale)
        assert np.all(pos[r, n[r]:] == -1) and np.all(np.isneginf(s[r, n[r]:]))


@pytest.mark.parametrize("eu,ei,layers", [(32, 96, [256, 128]), (96, 32, [128]), (128, 128, [256])])
def test_basic_ncf_unequal_widths(gpu, mlp_calls, eu, ei, layers):
    from deeprecommendation_amd import top_k_items
    m, _ = _basic(gpu, 500, 4000, eu, ei, layers, 2)
    users = torch.randint(0, 500, (64,), device=gpu)
    got = top_k_items(m, users, 20)
    assert len(mlp_calls) == 1
    _equal(got, top_k_items(m, users, 20, fused=False))


N_ITEMS, N_USERS = 300, 90


@pytest.mark.parametrize("hetero", [True, False])
@pytest.mark.parametrize("concat", [False, True])
def test_graph_ncf_mlp_route(gpu, mlp_calls, hetero, concat):
    """GraphNCF-MLP with an instance: mean over D = 64 (K0 = 128) or concat of D = 32 over one layer (K0 = 128); items first."""
    from deeprecommendation_amd import seen_items, top_k_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF, GraphData
    D, L = (32, 1) if concat else (64, 2)
    u2i, i2u, a1, a2 = _bipartite(N_ITEMS, N_USERS, 3000, seed=5)
    torch.manual_seed(5)
    m = GraphNCF(item_dim=N_ITEMS, user_dim=N_USERS, num_gnn_layers=L, hetero=hetero, node_emb=D, mlp_dense_layers=[256, 128],
                 use_dot_product=False, concat=concat).eval()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(gpu)
    graph = GraphData(user2item_edge_index=u2i, item2user_edge_index=i2u, user2item_edge_attr=a1, item2user_edge_attr=a2,
                      num_items=N_ITEMS, num_users=N_USERS)
    rng = np.random.default_rng(int(hetero) + 2 * int(concat))
    users = rng.choice(N_USERS, 70, replace=False) + N_ITEMS
    ug = torch.as_tensor(users, device=gpu)
    exclude = seen_items(graph, ug)
    k = 25
    got = top_k_items(m, ug, k, graph=graph, exclude=exclude)
    assert len(mlp_calls) == 1
    _equal(got, top_k_items(m, ug, k, graph=graph, exclude=exclude, fused=False))
    items = torch.as_tensor(rng.integers(0, N_ITEMS, 200), device=gpu)        # an item subset: the id-list form
    _equal(top_k_items(m, ug, k, item_ids=items, graph=graph), top_k_items(m, ug, k, item_ids=items, graph=graph, fused=False))
    assert len(mlp_calls) == 2
    u = torch.as_tensor(users).repeat_interleave(N_ITEMS)
    i = torch.arange(N_ITEMS).repeat(len(users))
    ref = O.graph_ncf_forward(state, hetero, L, concat, False, torch.eye(N_ITEMS), torch.eye(N_USERS), u2i, i2u, a1, a2,
                              u, i).view(len(users), N_ITEMS)
    lists = [u2i[1, u2i[0] == x].tolist() for x in users]
    rs, ri, rn = topk_oracle(ref, k, lists)
    s, pos, n = (t.cpu().numpy() for t in got)
    scale = float(ref.abs().max())
    for r in range(len(users)):
        _check_ranked(s[r], pos[r], int(n[r]), rs[r].numpy(), ri[r].numpy(), int(rn[r]), scale)


def test_fallbacks_give_the_same_result(gpu, mlp_calls):
    from deeprecommendation_amd import top_k_items
    m, _ = _basic(gpu, 400, 3000, 64, 64, [256, 128], 3)
    users = torch.randint(0, 400, (50,), device=gpu)
    _equal(top_k_items(m, users, 300), top_k_items(m, users, 300, fused=False))        # k above the fused limit
    assert len(mlp_calls) == 0
    m.set_fold_first_layer(True)                                                      # folded first layer
    _equal(top_k_items(m, users, 20), top_k_items(m, users, 20, fused=False))
    assert len(mlp_calls) == 0
    m.set_fold_first_layer(False)
    m.set_scoring_dtype(torch.bfloat16)                                               # bf16 scoring
    _equal(top_k_items(m, users, 20), top_k_items(m, users, 20, fused=False))
    assert len(mlp_calls) == 0
    m.set_scoring_dtype(torch.float32)
    _equal(top_k_items(m, users, 20), top_k_items(m, users, 20, fused=False))
    assert len(mlp_calls) == 1
    m2, _ = _basic(gpu, 400, 3000, 64, 64, [64], 4)                                    # N1 = 64: no fused instance
    _equal(top_k_items(m2, users, 20), top_k_items(m2, users, 20, fused=False))
    assert len(mlp_calls) == 1
