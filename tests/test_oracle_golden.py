"""Pins oracle/ncf_oracle.py to golden vectors produced by the reference itself (tests/golden/make_golden.py).

CPU only.  Tolerances: the oracle issues the same ATen ops as the reference on the same inputs, so outputs
are compared bit-exact (torch.equal) wherever the op sequence is identical and the CPU sums in the goldens' order
(conftest.golden_path_blas: a stored fingerprint of that order; other CPUs take other BLAS / vector kernels, and there the
same results are held to 1e-6 of the largest reference element); the table formulation (W.T[idx] + b) is bit-exact to the
dense one on any CPU because a one-hot GEMM adds exact zeros.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_path_blas, load_golden, onehot
from oracle import ncf_oracle as O

GOLDEN_ORDER = golden_path_blas()


def assert_golden(x, ref, what="", rel=1e-6, floor=0.0):
    """Bit-exact where this CPU sums in the goldens' order; elsewhere within fp32 reordering: ``rel`` of the largest reference
    element, at least ``floor`` (outputs: 1e-6, the bar of test_attention_checkpoint_dims; gradients, which cancel terms larger
    than the result: 1e-5 with a floor of 1e-8 of the loss for gradients that are zero by construction, the bars of
    test_reference_gradients)."""
    ref = torch.as_tensor(ref)
    if GOLDEN_ORDER:
        assert torch.equal(x, ref), what
    else:
        assert x.shape == ref.shape and x.dtype == ref.dtype, what
        assert float((x.double() - ref.double()).abs().max()) <= max(rel * float(ref.abs().max()), floor), what


def assert_golden_scalar(v, ref):
    if GOLDEN_ORDER:
        assert float(v) == float(ref)
    else:
        assert abs(float(v) - float(ref)) <= 1e-6 * abs(float(ref))


@pytest.fixture(autouse=True)
def _single_thread():
    """The goldens were produced with one CPU thread; MKL's GEMM blocking (hence the fp32 summation order) depends on
    the thread count, so bit-exact comparisons pin it."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("name", ["g1_basic_onehot_small", "g1_basic_onehot_e32", "g1_basic_onehot_nodrop",
                                  "g1_basic_onehot_e64", "g1_basic_onehot_e128", "g1_basic_onehot_e64_h256"])
def test_basic_onehot_dense_and_table(name):
    state, a, kw = load_golden(name)
    up, ip = a["user_pos"], a["item_pos"]
    ref = torch.from_numpy(a["out"])
    dense = O.basic_ncf_forward(state, onehot(up, kw["user_dim"]), onehot(ip, kw["item_dim"]))
    assert_golden(dense, ref)
    table = O.basic_ncf_forward_indexed(state, torch.as_tensor(up), torch.as_tensor(ip))
    assert torch.equal(table, dense)  # Linear(onehot(i)) == W[:, i] + b, bit-exact
    assert_golden(table, ref)


def test_basic_dense_profiles():
    state, a, kw = load_golden("g1_basic_dense_profiles")
    out = O.basic_ncf_forward(state, torch.from_numpy(a["X_user"]), torch.from_numpy(a["X_item"]))
    assert_golden(out, torch.from_numpy(a["out"]))


def test_mf():
    state, a, kw = load_golden("g2_mf_onehot")
    ref = torch.from_numpy(a["out"])
    out = O.mf_forward(state, onehot(a["user_pos"], kw["user_dim"]), onehot(a["item_pos"], kw["item_dim"]))
    assert_golden(out, ref)
    out2 = O.mf_forward_indexed(state, torch.as_tensor(a["user_pos"]), torch.as_tensor(a["item_pos"]))
    assert_golden(out2, ref)


@pytest.mark.parametrize("name", ["g3_att_dense8", "g3_att_none", "g3_att_cos", "g3_att_vec64", "g3_att_vec128",
                                  "g3_att_peaked_e64", "g3_att_peaked_none"])
def test_attention(name):
    state, a, kw = load_golden(name)
    out, att = O.attention_ncf_forward(state, torch.from_numpy(a["candidate_items"]),
                                       torch.from_numpy(a["rated_items"]), torch.from_numpy(a["user_matrix"]),
                                       use_cos_sim_instead=kw["use_cos_sim_instead"], return_attention_weights=True)
    assert_golden(out, torch.from_numpy(a["out"]))
    assert_golden(att, torch.from_numpy(a["att"]))
    if name.startswith("g3_att_peaked"):             # peaked softmax; its designed rows: test_attention_peaked_fixtures.py
        return
    if name.startswith("g3_att_vec"):
        assert float(att[0].abs().sum()) == 0.0
        return
    # quirks the fixture was built to exercise (attention_ncf.py:158, :208-209)
    assert float(att[1].abs().sum()) == 0.0          # user with no ratings -> all zeros, not NaN
    assert float(att[2, 3]) == 0.0                   # exact-0 entry is treated as unrated


def test_attention_checkpoint_dims():
    """G4: AttentionNCF at the dims of the reference's shipped checkpoint (2094 input features, embeddings and attention
    net 128, MLP [256, 128]), with hashed weights at the trained checkpoint's scale and the reference's outputs."""
    state, a, kw = load_golden("g4_att_ckpt_dims")
    assert kw == {"item_dim": 2094, "item_emb": 128, "user_emb": 128, "att_dense": 128, "mlp_dense_layers": [256, 128],
                  "dropout_rate": 0.2, "use_cos_sim_instead": False, "message_dropout": 0.0}
    assert tuple(state["ItemEmbeddings.0.weight"].shape) == (128, 2094)
    out, att = O.attention_ncf_forward(state, torch.from_numpy(a["candidate_items"]),
                                       torch.from_numpy(a["rated_items"]), torch.from_numpy(a["user_matrix"]),
                                       return_attention_weights=True)
    # K = 2094 GEMMs: MKL's blocking depends on the thread count (golden was made with 1 thread), so the
    # summation order may differ in the last bit -> 1e-6 relative instead of bit-exact.
    assert torch.allclose(out, torch.from_numpy(a["out"]), rtol=1e-6, atol=1e-7)
    assert torch.allclose(att, torch.from_numpy(a["att"]), rtol=1e-6, atol=1e-8)


def test_mlp_key_names():
    keys = json.load(open(os.path.join(GOLDEN, "g6_mlp_keys.json")))
    for name, dr in (("with_dropout", 0.2), ("no_dropout", None)):
        idx = O.mlp_linear_indices(2, dr)
        want = [f"{i}.{p}" for i in idx for p in ("weight", "bias")]
        assert keys[name] == want


def test_eval_ranking():
    _, a, _ = load_golden("g5_eval_ranking")
    for k, key in ((5, "ndcg5"), (10, "ndcg10")):
        nd, adj = O.eval_ranking(a["userId"], a["rating"], a["prediction"], cutoff=k)
        assert abs(nd - a[key][0]) < 1e-12 and abs(adj - a[key][1]) < 1e-12


def test_cfg1_ml1m_scale():
    """BASELINE configs[0]: U=6040, I=3706, emb 32, MLP [256], 20k pairs, batch 512 — per-pair predictions
    bit-exact (assert_golden); MSE and NDCG/adj-NDCG @5/10/20 of the golden predictions to 1e-12."""
    state, a, kw = load_golden("cfg1_basic_ml1m")
    up = torch.as_tensor(a["user_pos"].astype(np.int64))
    ip = torch.as_tensor(a["item_pos"].astype(np.int64))
    outs = [O.basic_ncf_forward_indexed(state, up[s:s + 512], ip[s:s + 512]) for s in range(0, len(up), 512)]
    out = torch.cat(outs)
    assert_golden(out, torch.from_numpy(a["out"]))
    pred = a["out"].reshape(-1).astype(np.float64)   # == out where the CPU sums in the goldens' order
    mse = float(((pred - a["rating"]) ** 2).sum() / len(pred))
    assert abs(mse - float(a["mse"])) < 1e-12
    for k in (5, 10, 20):
        nd, adj = O.eval_ranking(a["user_pos"] + 1, a["rating"], pred, cutoff=k)
        assert abs(nd - a[f"ndcg{k}"][0]) < 1e-12 and abs(adj - a[f"ndcg{k}"][1]) < 1e-12


# ---------------- GraphNCF / LightGCN: PARITY UNPINNED (PyG absent) — self-consistency only ----------------
def _tiny_graph(seed, n_items=5, n_users=7, n_inter=20, binary=False):
    g = torch.Generator().manual_seed(seed)
    pairs = set()
    while len(pairs) < n_inter:
        pairs.add((int(torch.randint(0, n_users, (1,), generator=g)), int(torch.randint(0, n_items, (1,), generator=g))))
    pairs = sorted(pairs)
    u = torch.tensor([p[0] + n_items for p in pairs])
    i = torch.tensor([p[1] for p in pairs])
    u2i = torch.stack([u, i])
    i2u = torch.stack([i, u])
    if binary:
        return u2i, i2u, None, None
    return u2i, i2u, torch.randn(len(pairs), generator=g), torch.randn(len(pairs), generator=g)


@pytest.mark.parametrize("hetero", [True, False])
@pytest.mark.parametrize("binary", [True, False])
def test_lightgcn_edge_list_vs_dense_adjacency(hetero, binary):
    torch.manual_seed(5)
    D, N = 8, 12
    x = torch.randn(N, D)
    names = ["user2item_W", "item2user_W"] if hetero else ["W"]
    cs = {}
    for n in names:
        cs[f"{n}.0.weight"] = torch.randn(D, D) * 0.3
        cs[f"{n}.0.bias"] = torch.randn(D) * 0.1
    u2i, i2u, a1, a2 = _tiny_graph(3, binary=binary)
    y = O.lightgcn_conv(x, cs, hetero, u2i, i2u, a1, a2)
    yd = O.lightgcn_conv_dense(x, cs, hetero, u2i, i2u, a1, a2)
    assert torch.allclose(y.double(), yd, rtol=1e-5, atol=1e-6)


def test_c_kernel_order_oracle_agrees_with_reference_level_oracle():
    """oracle/ncf_oracle_c.c restates the fused kernel's fp32 operation ORDER; it must still be the same function as the
    reference-level oracle (to fp32 rounding) and reproduce the reference's golden outputs to 1e-5."""
    from oracle import c_oracle
    state, a, kw = load_golden("g1_basic_onehot_e32")  # E = 32, MLP [256, 128]: tileable like the kernel
    tu = O.embedding_table(state["user_embeddings.0.weight"], state["user_embeddings.0.bias"])
    ti = O.embedding_table(state["item_embeddings.0.weight"], state["item_embeddings.0.bias"])
    layers = O.mlp_weights(state)
    out = c_oracle.score_fused_f32(tu, ti, torch.as_tensor(a["user_pos"]), torch.as_tensor(a["item_pos"]),
                                   [w for w, _ in layers], [b for _, b in layers])
    ref = torch.from_numpy(a["out"])
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-6)
    state, a, kw = load_golden("cfg1_basic_ml1m")       # E = 32, MLP [256]
    tu = O.embedding_table(state["user_embeddings.0.weight"], state["user_embeddings.0.bias"])
    ti = O.embedding_table(state["item_embeddings.0.weight"], state["item_embeddings.0.bias"])
    layers = O.mlp_weights(state)
    sub = slice(0, 4096)
    out = c_oracle.score_fused_f32(tu, ti, torch.as_tensor(a["user_pos"][sub].astype(np.int64)),
                                   torch.as_tensor(a["item_pos"][sub].astype(np.int64)), [w for w, _ in layers], [b for _, b in layers])
    assert torch.allclose(out, torch.from_numpy(a["out"][sub]), rtol=1e-5, atol=1e-6)


# ---------------- round 3: deterministic train-mode pins (target mask, gradients) ----------------
@pytest.mark.parametrize("name", ["g3_att_train_dense8", "g3_att_train_cos", "g3_att_train_vec64", "g3_att_train_ue50",
                                  "g3_att_train_peaked"])
def test_attention_train_mode_target_mask_and_gradients(name):
    """attention_ncf.py:195-205 (train-only target mask) and the gradients of MSELoss(sum) (datasets/base.py:31-32)."""
    state, a, kw = load_golden(name)
    cand, rated, um = (torch.from_numpy(a[k]) for k in ("candidate_items", "rated_items", "user_matrix"))
    out, att = O.attention_ncf_forward(state, cand, rated, um, use_cos_sim_instead=kw["use_cos_sim_instead"],
                                       return_attention_weights=True, training=True)
    assert_golden(out, torch.from_numpy(a["out"]))
    assert_golden(att, torch.from_numpy(a["att"]))
    for b, c in enumerate(a["self_cols"]):           # the fixture's self-rated candidates are masked ...
        assert float(att[b, c]) == 0.0 and float(um[b, c]) != 0.0
    ev = O.attention_ncf_forward(state, cand, rated, um, use_cos_sim_instead=kw["use_cos_sim_instead"], return_attention_weights=True)[1]
    assert float(ev[0, a["self_cols"][0]]) > 0.0     # ... and are not in eval mode
    assert float(att[1].abs().sum()) == 0.0          # row whose only entry is the candidate itself: all -inf -> 0
    _, loss, grads = O.loss_and_grads(
        lambda st: O.attention_ncf_forward(st, cand, rated, um, use_cos_sim_instead=kw["use_cos_sim_instead"], training=True),
        state, torch.from_numpy(a["y"]))
    assert_golden_scalar(loss, a["loss"])
    assert set(grads) == set(a["grads"])
    for k, g in a["grads"].items():
        assert_golden(grads[k], g, k, rel=1e-5, floor=1e-8 * abs(float(a["loss"])))


@pytest.mark.parametrize("name", ["g7_grads_basic_small", "g7_grads_basic_e64", "g7_grads_basic_h256", "g7_grads_mf"])
def test_basic_and_mf_gradients(name):
    state, a, kw = load_golden(name)
    fwd = O.mf_forward if name.endswith("_mf") else O.basic_ncf_forward
    Xu, Xi = onehot(a["user_pos"], kw["user_dim"]), onehot(a["item_pos"], kw["item_dim"])
    out, loss, grads = O.loss_and_grads(lambda st: fwd(st, Xu, Xi), state, torch.from_numpy(a["y"]))
    assert_golden(out, torch.from_numpy(a["out"]))
    assert_golden_scalar(loss, a["loss"])
    for k, g in a["grads"].items():
        assert_golden(grads[k], g, k, rel=1e-5, floor=1e-8 * abs(float(a["loss"])))
    if not name.endswith("_mf"):
        # table formulation: same loss; embedding gradients are the scatter-add the dense one-hot GEMM performs
        _, loss2, g2 = O.loss_and_grads(lambda st: O.basic_ncf_forward_indexed(st, torch.as_tensor(a["user_pos"]), torch.as_tensor(a["item_pos"])),
                                        state, torch.from_numpy(a["y"]))
        assert_golden_scalar(loss2, a["loss"])
        for k, g in a["grads"].items():
            assert torch.allclose(g2[k], g, rtol=1e-5, atol=1e-6 * float(g.abs().max())), k
