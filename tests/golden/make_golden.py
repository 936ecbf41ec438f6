"""Generate the golden vectors under tests/golden/ by running the REFERENCE itself on CPU.

Needs a checkout of the reference project (its path as the argument, or NCF_REFERENCE_DIR):

    python tests/golden/make_golden.py <reference checkout>
    python tests/golden/make_golden.py <reference checkout> --only g4     # the G4 fixture alone (or: --only g3_peaked, blas_probe)

Each .npz holds weights (every state_dict entry, prefixed ``w::``), inputs and the reference's
outputs, so nothing depends on RNG-stream equality between torch versions.  Only *data* is stored:
no reference source, no checkpoint bytes (G4 runs the reference model at the shipped checkpoint's dims with
hashed weights: the fixture stores their recipe, the inputs and the outputs).

The reference imports ``torch_geometric.data.Data`` (content_providers.py:1, annotation only) and
``seaborn`` (plots.py:3); neither is installed, so two empty in-memory stub modules are registered
before the import.  GraphNCF cannot be imported (needs torch_geometric.nn) -> no golden for it
(parity unpinned; see oracle/ncf_oracle.py header).

Round 3 adds the deterministic train-mode pins:
  g3_att_train_*   AttentionNCF in .train() with dropout_rate=0.0 / message_dropout=None: target masking (:195-205)
  g7_grads_*       loss = MSELoss(reduction='sum') (datasets/base.py:19-20,31-32), .backward(): every parameter gradient
  g8_create_graph_*  content_providers/graph_providers.py:10-66 create_graph, binary and weighted

and the peaked-softmax pins (golden_g3_peaked): g3_att_peaked_e64, g3_att_peaked_none, g3_att_train_peaked.
"""
import hashlib
import json
import os
import sys
import types

import numpy as np

REF = os.environ.get("NCF_REFERENCE_DIR", "")   # checkout of the reference project (first argument overrides)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
from conftest import blas_probe_arrays, hashed_weight  # noqa: E402  (tests/conftest.py)

# G4: the dims of the reference's shipped AttentionNCF checkpoint (models/runs/AttentionNCF_with_features_attNet128_3mil.pt).
# Its trained weights are reference content and stay out of this repository; the fixture uses hashed weights of the same shapes.
G4_KWARGS = {"item_dim": 2094, "item_emb": 128, "user_emb": 128, "att_dense": 128, "mlp_dense_layers": [256, 128],
             "dropout_rate": 0.2, "use_cos_sim_instead": False, "message_dropout": 0.0}
# per-tensor bounds of the hashed weights at the trained checkpoint's scale (about sqrt(3) x its standard deviation per tensor;
# the single-element biases at its magnitude), so that the attention weights spread as they do with trained weights
G4_BOUNDS = {"ItemEmbeddings.0.weight": 0.3, "ItemEmbeddings.0.bias": 0.22, "UserEmbeddings.0.weight": 0.36,
             "UserEmbeddings.0.bias": 0.4, "AttentionNet.0.weight": 0.26, "AttentionNet.0.bias": 0.13,
             "AttentionNet.3.weight": 0.04, "AttentionNet.3.bias": 0.03, "MLP.0.weight": 0.19, "MLP.0.bias": 0.3,
             "MLP.3.weight": 0.17, "MLP.3.bias": 0.68, "MLP.6.weight": 0.025, "MLP.6.bias": 3.3}


def _import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REF, "src"))
    tg = types.ModuleType("torch_geometric")
    tgd = types.ModuleType("torch_geometric.data")

    class Data:  # attribute bag: the reference uses it as an annotation (content_providers.py:61) and, in create_graph
        # (graph_providers.py:58-66), as a keyword container — no PyG behaviour is involved in either
        def __init__(self, **kw):
            self.__dict__.update(kw)

    tgd.Data = Data
    tg.data = tgd
    sys.modules["torch_geometric"] = tg
    sys.modules["torch_geometric.data"] = tgd
    sys.modules["seaborn"] = types.ModuleType("seaborn")


def _state_arrays(model):
    return {"w::" + k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def _save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


# attention_ncf.py:195-205: in training a candidate that equals one of the rated rows (isclose on the embeddings) is
# masked out of its own softmax row.  Candidates 0..n_self-1 ARE rated rows of the batch; the loss is the reference's
# MSELoss(reduction='sum') against y (datasets/base.py:19-20,31-32) and every parameter gradient is stored.
def _att_train_case(torch, AttentionNCF, tag, Fdim, IE, UE, B, I, n_self, seed, mlp, density=0.5, att_scale=None, **kw):
    torch.manual_seed(seed)
    m = AttentionNCF(item_dim=Fdim, item_emb=IE, user_emb=UE, mlp_dense_layers=mlp, dropout_rate=0.0,
                     message_dropout=None, **kw).train()
    extra = {}
    if att_scale is not None:                             # peaked softmax: AttentionNet's last Linear scaled (see golden_g3_peaked)
        with torch.no_grad():
            m.AttentionNet[-1].weight.mul_(att_scale)
        extra["att_scale"] = np.array(float(att_scale))
        hook = _logit_hook(m, extra)
    g = torch.Generator().manual_seed(seed + 1)
    rated = torch.rand(I, Fdim, generator=g)
    cand = torch.rand(B, Fdim, generator=g)
    self_cols = torch.randperm(I, generator=g)[:n_self]
    cand[:n_self] = rated[self_cols]                      # these candidates are rated items of the batch
    um = torch.zeros(B, I)
    mask = torch.rand(B, I, generator=g) < density
    um[mask] = (torch.randint(1, 11, (B, I), generator=g).float() * 0.5 - 2.9)[mask]
    for b in range(n_self):                               # the user HAS rated the candidate (that is what gets masked)
        um[b, self_cols[b]] = 1.35 if b % 2 == 0 else -0.65
    um[B - 1] = 0.0                                       # all-unrated row in train mode
    if n_self > 1:                                        # a row whose ONLY rated entry is the candidate itself -> all -inf -> 0
        um[1] = 0.0
        um[1, self_cols[1]] = 0.85
    y = torch.randint(1, 11, (B,), generator=g).float() * 0.5
    out, att = m(cand, rated, um, return_attention_weights=True)
    if att_scale is not None:
        hook.remove()
    loss = torch.nn.MSELoss(reduction='sum')(out, y.view(-1, 1).float())
    loss.backward()
    grads = {"g::" + k: p.grad.detach().numpy().copy() for k, p in m.named_parameters()}
    assert all(np.isfinite(v).all() for v in grads.values())
    _save(tag, candidate_items=cand.numpy(), rated_items=rated.numpy(), user_matrix=um.numpy(), y=y.numpy(),
          self_cols=self_cols.numpy(), out=out.detach().numpy(), att=att.numpy(), loss=np.array(loss.item()),
          kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m), **grads, **extra)


def _logit_hook(m, store):
    """Forward hook on AttentionNet: its output is the reference's raw logits attOut (attention_ncf.py:179), one per valid pair of
    the batch in row-major (pair, rated item) order; stored as ``logits``."""
    return m.AttentionNet.register_forward_hook(lambda mod, inp, out: store.__setitem__("logits", out.detach().reshape(-1).numpy().copy()))


# G3 peaked: AttentionNet's last Linear (the one that produces the logit) multiplied by PEAK_SCALE, so that the softmax is as peaked
# as with trained weights: one rated item takes almost all the weight, the logits of a row spread over tens of units and most exp
# terms underflow.  PEAK_SCALE is the smallest round value with a median row max weight >= 0.9 and a per-row logit spread >= 60 in
# g3_att_peaked_e64 (tests/test_attention_peaked_fixtures.py checks both).
PEAK_SCALE = 500.0
# the train fixture's scale: its rows are shorter (~75 entries) and its gradients go through the softmax derivative, whose fp32 rounding
# grows with the logits: at 500 the reference's own gradients lie 0.5-0.8 of the 1e-5 bar from their float64 values, at 300 the median
# row max weight is still 0.8
TRAIN_PEAK_SCALE = 300.0


def golden_g3_peaked(torch, AttentionNCF):
    """g3_att_peaked_e64: the dims where the grouped / entry-split / tail kernels all apply (F = 50, IE = UE = 64, A = 128, MLP
    [256, 128]), 8 users x 32 candidates in the reference's call shape (a user's row repeated per candidate), 400 rated items: six
    users rate 300-360 of them (rows of 5-6 tiles of 64), one rates a single item, one none; ratings of both signs.
    g3_att_peaked_none: the linear AttentionNet (att_dense=None) scaled the same way.  g3_att_train_peaked: the train-mode recipe
    (target mask, gradients of MSELoss(sum)) with the scaled AttentionNet.  Every fixture stores the reference's raw logits."""
    def eval_case(tag, Fdim, IE, A, mlp, users, per_user, I, counts, seed):
        # hashed weights at PyTorch's default Linear scale (bound 1 / sqrt(fan_in)) stored as their recipe, except AttentionNet's scaled
        # output weight, stored as values
        m = AttentionNCF(item_dim=Fdim, item_emb=IE, user_emb=IE, att_dense=A, mlp_dense_layers=mlp).eval()
        recipe, state, peaked = [], {}, "AttentionNet.%d.weight" % (len(m.AttentionNet) - 1)
        for salt, (k, v) in enumerate(m.state_dict().items()):
            fan_in = int(m.state_dict()[k.replace(".bias", ".weight")].shape[1])
            state[k] = torch.from_numpy(hashed_weight(tuple(v.shape), seed * 100 + salt, fan_in ** -0.5))
            if k == peaked:
                state[k] = state[k] * PEAK_SCALE
            else:
                recipe.append([k, list(v.shape), seed * 100 + salt, fan_in ** -0.5])
        m.load_state_dict(state)
        g = torch.Generator().manual_seed(seed + 1)
        rated = torch.rand(I, Fdim, generator=g)
        cand = torch.rand(users * per_user, Fdim, generator=g)
        rows = torch.zeros(users, I)
        for u, n in enumerate(counts):
            cols = torch.randperm(I, generator=g)[:n]
            rows[u, cols] = torch.randint(1, 11, (n,), generator=g).float() * 0.5 - 2.9     # -2.4 .. 2.1, never 0
        um = rows[torch.arange(users * per_user) // per_user].contiguous()                # the user's row once per candidate
        extra = {}
        hook = _logit_hook(m, extra)
        with torch.no_grad():
            out, att = m(cand, rated, um, return_attention_weights=True)
        hook.remove()
        _save(tag, candidate_items=cand.numpy(), rated_items=rated.numpy(), user_matrix=um.numpy(), out=out.numpy(), att=att.numpy(),
              att_scale=np.array(PEAK_SCALE), kwargs=np.array(json.dumps(m.kwargs)), hashed_weights=np.array(json.dumps(recipe)),
              **{"w::" + peaked: state[peaked].numpy()}, **extra)

    eval_case("g3_att_peaked_e64", 50, 64, 128, [256, 128], 8, 32, 400, [340, 300, 360, 1, 320, 0, 350, 310], 107)
    eval_case("g3_att_peaked_none", 20, 16, None, [32, 16], 6, 4, 120, [100, 90, 1, 0, 110, 70], 108)
    _att_train_case(torch, AttentionNCF, "g3_att_train_peaked", 48, 64, 64, 40, 150, 9, 205, [64], density=0.5,
                    att_scale=TRAIN_PEAK_SCALE, att_dense=128)


def golden_g4(torch, AttentionNCF):
    """G4: AttentionNCF at the shipped checkpoint's dims (K = 2094 input features), weights from hashed_weight within
    G4_BOUNDS; the fixture stores the recipe, the inputs and the reference's outputs."""
    m = AttentionNCF(**G4_KWARGS).eval()
    recipe, state = [], {}
    for salt, (k, v) in enumerate(m.state_dict().items()):
        recipe.append([k, list(v.shape), 1000 + salt, G4_BOUNDS[k]])
        state[k] = torch.from_numpy(hashed_weight(tuple(v.shape), 1000 + salt, G4_BOUNDS[k]))
    m.load_state_dict(state)
    g = torch.Generator().manual_seed(10)
    Fdim = G4_KWARGS["item_dim"]
    rated = (torch.rand(16, Fdim, generator=g) < 0.02).float() + torch.rand(16, Fdim, generator=g) * 0.1
    cand = (torch.rand(4, Fdim, generator=g) < 0.02).float() + torch.rand(4, Fdim, generator=g) * 0.1
    um = torch.zeros(4, 16)
    mask = torch.rand(4, 16, generator=g) < 0.6
    um[mask] = (torch.randint(1, 11, (4, 16), generator=g).float() * 0.5 - 3.1)[mask]
    with torch.no_grad():
        out, att = m(cand, rated, um, return_attention_weights=True)
    _save("g4_att_ckpt_dims", candidate_items=cand.numpy(), rated_items=rated.numpy(), user_matrix=um.numpy(),
          out=out.numpy(), att=att.numpy(), kwargs=np.array(json.dumps(G4_KWARGS)), hashed_weights=np.array(json.dumps(recipe)))


def golden_blas_probe(torch):
    # SHA-256 of each product's bytes: the test only asks whether the bits are the same
    _save("blas_probe", **{k: np.array(hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
                           for k, v in blas_probe_arrays(torch).items()})


def main():
    _import_reference()
    import torch
    from neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from neural_collaborative_filtering.models.mf import MF
    from neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    from neural_collaborative_filtering.util import build_MLP_layers

    import pandas as pd
    torch.set_num_threads(1)

    def onehot(pos, n):
        x = torch.zeros((len(pos), n), dtype=torch.float32)
        x[torch.arange(len(pos)), torch.as_tensor(pos)] = 1.0
        return x

    # ---------------- G1: BasicNCF, one-hot and dense-profile inputs ----------------
    for tag, U, I, E, mlp, dr in (("g1_basic_onehot_small", 60, 40, 8, [16], 0.2),
                                  ("g1_basic_onehot_e32", 60, 40, 32, [256, 128], 0.2),
                                  ("g1_basic_onehot_nodrop", 60, 40, 8, [16, 8], None)):
        torch.manual_seed(101)
        m = BasicNCF(item_dim=I, user_dim=U, item_emb=E, user_emb=E, mlp_dense_layers=mlp, dropout_rate=dr).eval()
        rng = np.random.default_rng(7)
        up = rng.integers(0, U, 64)
        ip = rng.integers(0, I, 64)
        with torch.no_grad():
            out = m(onehot(up, U), onehot(ip, I))
        _save(tag, user_pos=up, item_pos=ip, out=out.numpy(),
              kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m))

    # kernel-shaped cases: these dims hit the fused / small-batch / folded HIP instances directly
    for tag, E, mlp in (("g1_basic_onehot_e64", 64, [256, 128]), ("g1_basic_onehot_e128", 128, [256, 128]),
                        ("g1_basic_onehot_e64_h256", 64, [256])):
        torch.manual_seed(105)
        U, I = 600, 400
        m = BasicNCF(item_dim=I, user_dim=U, item_emb=E, user_emb=E, mlp_dense_layers=mlp).eval()
        rng = np.random.default_rng(12)
        up = rng.integers(0, U, 700)
        ip = rng.integers(0, I, 700)
        with torch.no_grad():
            out = m(onehot(up, U), onehot(ip, I))
        _save(tag, user_pos=up, item_pos=ip, out=out.numpy(), kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m))

    torch.manual_seed(102)
    m = BasicNCF(item_dim=24, user_dim=24, item_emb=16, user_emb=8, mlp_dense_layers=[32, 16]).eval()
    Xu = torch.rand(48, 24)
    Xi = torch.rand(48, 24)
    with torch.no_grad():
        out = m(Xu, Xi)
    _save("g1_basic_dense_profiles", X_user=Xu.numpy(), X_item=Xi.numpy(), out=out.numpy(),
          kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m))

    # ---------------- G2: MF ----------------
    torch.manual_seed(103)
    m = MF(item_dim=40, user_dim=60, item_emb=16, user_emb=16).eval()
    rng = np.random.default_rng(8)
    up = rng.integers(0, 60, 64)
    ip = rng.integers(0, 40, 64)
    with torch.no_grad():
        out = m(onehot(up, 60), onehot(ip, 40))
    _save("g2_mf_onehot", user_pos=up, item_pos=ip, out=out.numpy(),
          kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m))

    # ---------------- G3: AttentionNCF variants ----------------
    def att_inputs(B, I, Fdim, seed):
        g = torch.Generator().manual_seed(seed)
        rated = torch.rand(I, Fdim, generator=g)
        cand = torch.rand(B, Fdim, generator=g)
        um = torch.zeros(B, I)
        mask = torch.rand(B, I, generator=g) < 0.5
        ratings = torch.randint(1, 11, (B, I), generator=g).float() * 0.5  # 0.5 .. 5.0
        mean = torch.rand(B, 1, generator=g) * 2 + 2.5
        um[mask] = (ratings - (mean + 2.5) / 2)[mask]
        um[1, :] = 0.0  # a user with no rated items: softmax over all -inf -> NaN -> 0 (:208-209)
        # a rated position whose normalised value is exactly 0.0 is dropped by `!= 0` (:158)
        um[2, 3] = 0.0
        um[0, 0] = 1.25
        return cand, rated, um

    for tag, kw in (("g3_att_dense8", dict(att_dense=8)),
                    ("g3_att_none", dict(att_dense=None)),
                    ("g3_att_cos", dict(use_cos_sim_instead=True))):
        torch.manual_seed(104)
        m = AttentionNCF(item_dim=20, item_emb=16, user_emb=16, mlp_dense_layers=[32, 16], **kw).eval()
        cand, rated, um = att_inputs(8, 12, 20, 9)
        with torch.no_grad():
            out, att = m(cand, rated, um, return_attention_weights=True)
        _save(tag, candidate_items=cand.numpy(), rated_items=rated.numpy(), user_matrix=um.numpy(),
              out=out.numpy(), att=att.numpy(), kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m))

    # kernel-shaped attention cases (vector paths of the HIP kernel: A = 128, IE = UE = 64 / 128)
    for tag, Fdim, IE, A, B, I in (("g3_att_vec64", 50, 64, 128, 64, 200), ("g3_att_vec128", 40, 128, 128, 33, 129)):
        torch.manual_seed(106)
        m = AttentionNCF(item_dim=Fdim, item_emb=IE, user_emb=IE, att_dense=A, mlp_dense_layers=[256, 128]).eval()
        g = torch.Generator().manual_seed(13)
        rated = torch.rand(I, Fdim, generator=g)
        cand = torch.rand(B, Fdim, generator=g)
        um = torch.zeros(B, I)
        mask = torch.rand(B, I, generator=g) < 0.3
        um[mask] = (torch.randint(1, 11, (B, I), generator=g).float() * 0.5 - 2.9)[mask]
        um[0] = 0.0
        with torch.no_grad():
            out, att = m(cand, rated, um, return_attention_weights=True)
        _save(tag, candidate_items=cand.numpy(), rated_items=rated.numpy(), user_matrix=um.numpy(),
              out=out.numpy(), att=att.numpy(), kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m))

    # ---------------- G3-train: AttentionNCF.train(), deterministic (dropout 0, no message dropout) ----------------
    def att_train_case(*args, **kw):
        _att_train_case(torch, AttentionNCF, *args, **kw)

    att_train_case("g3_att_train_dense8", 20, 16, 16, 8, 12, 3, 201, [32, 16], att_dense=8)
    att_train_case("g3_att_train_cos", 20, 16, 16, 8, 12, 3, 202, [32, 16], use_cos_sim_instead=True)
    att_train_case("g3_att_train_vec64", 48, 64, 64, 40, 150, 9, 203, [256, 128], density=0.3, att_dense=128)
    att_train_case("g3_att_train_ue50", 24, 16, 50, 8, 12, 2, 204, [32], att_dense=8)   # user_emb not a multiple of 4

    # ---------------- G7: gradients of BasicNCF / MF under the reference's loss ----------------
    def grads_case(tag, m, up, ip, U, I, seed):
        g = torch.Generator().manual_seed(seed)
        y = torch.randint(1, 11, (len(up),), generator=g).float() * 0.5
        out = m(onehot(up, U), onehot(ip, I))
        loss = torch.nn.MSELoss(reduction='sum')(out, y.view(-1, 1).float())
        loss.backward()
        grads = {"g::" + k: p.grad.detach().numpy().copy() for k, p in m.named_parameters()}
        _save(tag, user_pos=up, item_pos=ip, y=y.numpy(), out=out.detach().numpy(), loss=np.array(loss.item()),
              kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m), **grads)

    rng = np.random.default_rng(21)
    torch.manual_seed(301)
    U, I = 60, 40
    m = BasicNCF(item_dim=I, user_dim=U, item_emb=8, user_emb=8, mlp_dense_layers=[16, 8], dropout_rate=None).train()
    grads_case("g7_grads_basic_small", m, rng.integers(0, U, 96), rng.integers(0, I, 96), U, I, 31)   # duplicates in the batch
    torch.manual_seed(302)
    U, I = 300, 200
    m = BasicNCF(item_dim=I, user_dim=U, item_emb=64, user_emb=64, mlp_dense_layers=[256, 128], dropout_rate=None).train()
    grads_case("g7_grads_basic_e64", m, rng.integers(0, U, 500), rng.integers(0, I, 500), U, I, 32)
    torch.manual_seed(303)
    m = BasicNCF(item_dim=I, user_dim=U, item_emb=32, user_emb=32, mlp_dense_layers=[256], dropout_rate=None).train()
    grads_case("g7_grads_basic_h256", m, rng.integers(0, U, 130), rng.integers(0, I, 130), U, I, 33)
    torch.manual_seed(304)
    m = MF(item_dim=40, user_dim=60, item_emb=16, user_emb=16).train()
    grads_case("g7_grads_mf", m, rng.integers(0, 60, 96), rng.integers(0, 40, 96), 60, 40, 34)

    # ---------------- G8: create_graph (content_providers/graph_providers.py:10-66) ----------------
    from content_providers.graph_providers import create_graph
    rng = np.random.default_rng(41)
    all_users = np.arange(100, 145)
    all_items = np.arange(0, 100)
    n = 300
    users = rng.integers(100, 140, n)
    items = rng.integers(7, 30, n) * 3
    ratings = rng.integers(1, 11, n) * 0.5
    inter = pd.DataFrame({"userId": users, "movieId": items, "rating": ratings})
    item_to_node = {int(i): k for k, i in enumerate(sorted(all_items))}                     # graph_providers.py:77-80
    user_to_node = {int(u): len(all_items) + k for k, u in enumerate(sorted(all_users))}
    for binary in (False, True):
        gr = create_graph(inter, None, None, item_to_node, user_to_node, binary=binary)
        pos = gr.pos_df.reset_index()[["Id1", "Id2", "pos"]].to_numpy().astype(np.int64)
        extra = {}
        if not binary:
            extra = dict(user2item_edge_attr=gr.user2item_edge_attr.numpy(), item2user_edge_attr=gr.item2user_edge_attr.numpy())
        _save("g8_create_graph_" + ("binary" if binary else "weighted"), all_users=all_users, all_items=all_items,
              userId=users, movieId=items, rating=ratings,
              user2item_edge_index=gr.user2item_edge_index.numpy(), item2user_edge_index=gr.item2user_edge_index.numpy(),
              pos=pos, **extra)

    golden_g3_peaked(torch, AttentionNCF)

    golden_g4(torch, AttentionNCF)

    golden_blas_probe(torch)

    # ---------------- G5: eval_ranking (eval.py:25-75) ----------------
    import pandas as pd
    from neural_collaborative_filtering.eval import eval_ranking
    rng = np.random.default_rng(11)
    uid = np.repeat(np.arange(1, 7), 5)
    uid = np.concatenate([uid, [99]])  # a user with a single row (skipped, :38)
    mid = rng.integers(1, 100, len(uid))
    rating = rng.integers(1, 11, len(uid)) * 0.5
    rating[5:10] = 3.0  # one user whose ratings are all ties (ideal == worst, :57)
    pred = rating + rng.normal(0, 1.0, len(uid))
    pred[2] = pred[3]  # a tie in the predictions (sklearn tie-averaged DCG)
    df = pd.DataFrame({"userId": uid, "movieId": mid, "rating": rating, "prediction": pred})
    res = {}
    for k in (5, 10):
        nd, adj = eval_ranking(df, cutoff=k)
        res[k] = (nd, adj)
    _save("g5_eval_ranking", userId=uid, movieId=mid, rating=rating, prediction=pred,
          ndcg5=np.array(res[5]), ndcg10=np.array(res[10]))

    # ---------------- G6: build_MLP_layers key names ----------------
    keys = {}
    for name, dr in (("with_dropout", 0.2), ("no_dropout", None)):
        seq = build_MLP_layers(10, [8, 4], dropout_rate=dr)
        keys[name] = list(seq.state_dict().keys())
    with open(os.path.join(OUT, "g6_mlp_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)

    # ---------------- cfg 1 (BASELINE.json configs[0]): ML-1M-scale BasicNCF ----------------
    U, I = 6040, 3706
    torch.manual_seed(0)
    m = BasicNCF(item_dim=I, user_dim=U, item_emb=32, user_emb=32, mlp_dense_layers=[256], dropout_rate=0.2).eval()
    rng = np.random.default_rng(42)
    n = 20000
    up = rng.integers(0, U, n)
    ip = rng.integers(0, I, n)
    rating = rng.integers(1, 11, n) * 0.5
    outs = []
    with torch.no_grad():
        for s in range(0, n, 512):  # val_batch_size = 512 (globals.py:36)
            outs.append(m(onehot(up[s:s + 512], U), onehot(ip[s:s + 512], I)))
    out = torch.cat(outs).numpy()
    mse = float(((out.reshape(-1).astype(np.float64) - rating) ** 2).sum() / n)
    df = pd.DataFrame({"userId": up + 1, "movieId": ip + 1, "rating": rating,
                       "prediction": out.reshape(-1).astype(np.float64)})
    nd = {k: eval_ranking(df, cutoff=k) for k in (5, 10, 20)}
    _save("cfg1_basic_ml1m", user_pos=up.astype(np.int32), item_pos=ip.astype(np.int32), rating=rating, out=out,
          mse=np.array(mse), ndcg5=np.array(nd[5]), ndcg10=np.array(nd[10]), ndcg20=np.array(nd[20]),
          kwargs=np.array(json.dumps(m.kwargs)), **_state_arrays(m))


if __name__ == "__main__":
    # python tests/golden/make_golden.py <reference checkout> [--only g4|g3_peaked|blas_probe]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        REF = args[0]
    if not REF or not os.path.isdir(os.path.join(REF, "src")):
        raise SystemExit("usage: make_golden.py <reference checkout> [--only g4|g3_peaked|blas_probe]  (or set NCF_REFERENCE_DIR)")
    if "--only" in sys.argv:
        _import_reference()
        import torch
        from neural_collaborative_filtering.models.attention_ncf import AttentionNCF
        torch.set_num_threads(1)
        only = sys.argv[sys.argv.index("--only") + 1]
        if only == "g4":
            golden_g4(torch, AttentionNCF)
        elif only == "g3_peaked":
            golden_g3_peaked(torch, AttentionNCF)
        else:
            golden_blas_probe(torch)
    else:
        main()
