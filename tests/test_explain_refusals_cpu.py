"""CPU: what the explanation path refuses before anything touches a device — ``explain_items`` (the front end),
``AttentionNCF.explain`` (the model), ``native.attn_explain`` (the binding) and ``ncf_attn_explain`` (the entry point, on stand-in
pointers).  Every row is raised on CPU tensors, in the order the checks are made; the last refusal of each layer is the device's."""
import os

import pytest
import torch

from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF, SparseRatings
from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF

I_CAT, F_DIM = 30, 12


@pytest.fixture(scope="module")
def world():
    feats = torch.rand(I_CAT, F_DIM)
    rowptr = torch.tensor([0, 2, 2, 5], dtype=torch.int64)
    ratings = SparseRatings(rowptr, torch.tensor([1, 7, 0, 3, 29], dtype=torch.int32), torch.tensor([0.5, -1.0, 2.0, 1.5, -0.5]), I_CAT)
    model = AttentionNCF(item_dim=F_DIM, item_emb=32, user_emb=40, att_dense=16, mlp_dense_layers=[16]).eval()   # 40: no cross kernel needed
    users = torch.arange(3, dtype=torch.int64)
    items = torch.tensor([[4, 9], [0, -1], [29, 3]], dtype=torch.int64)
    return dict(feats=feats, ratings=ratings, model=model, users=users, items=items, profiles=(feats, ratings),
                thr=torch.full((3,), 0.1))


@pytest.fixture(scope="module")
def native():
    from deeprecommendation_amd import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    n.load_library()
    return n


# ------------------------------------------------------------------------------------------------ explain_items
def test_explain_items_is_exported_lazily():
    import deeprecommendation_amd
    import deeprecommendation_amd.recommend as rec
    assert "explain_items" in deeprecommendation_amd._RECOMMEND
    assert deeprecommendation_amd.explain_items is rec.explain_items
    assert rec.Explanations._fields == ("positions", "weights", "ratings", "counts", "threshold")


def test_explain_items_refuses_before_the_device(world):
    from deeprecommendation_amd import explain_items
    w, m = world, world["model"]
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            explain_items(m, w["users"], w["items"], w["profiles"])
    finally:
        m.eval()
    basic = BasicNCF(item_dim=I_CAT, user_dim=3, item_emb=8, user_emb=8, mlp_dense_layers=[16]).eval()
    with pytest.raises(ValueError, match="takes an AttentionNCF, not BasicNCF"):
        explain_items(basic, w["users"], w["items"], w["profiles"])
    with pytest.raises(ValueError, match="pass profiles="):
        explain_items(m, w["users"], w["items"], None)
    for bad in ((w["feats"], "ratings"), (w["feats"],), (w["feats"][0], w["ratings"]), "profiles"):
        with pytest.raises(ValueError, match="profiles = "):
            explain_items(m, w["users"], w["items"], bad)
    for users in (torch.arange(3, dtype=torch.int32), torch.zeros((3, 1), dtype=torch.int64), torch.zeros(3)):
        with pytest.raises(ValueError, match="user_ids must be a 1-D int64 tensor"):
            explain_items(m, users, w["items"], w["profiles"])
    for items in (w["items"].to(torch.int32), w["items"][0], w["items"][:, :, None], w["items"].float(), [[1, 2]] * 3):
        with pytest.raises(ValueError, match=r"item_positions must be a \(B, k\) int64 tensor"):
            explain_items(m, w["users"], items, w["profiles"])
    with pytest.raises(ValueError, match="item_positions has 2 rows for 3 users"):
        explain_items(m, w["users"], w["items"][:2], w["profiles"])
    for E in (0, 65, -1):
        with pytest.raises(ValueError, match=rf"max_reasons = {E} is outside 1 \.\. 64"):
            explain_items(m, w["users"], w["items"], w["profiles"], max_reasons=E)
    short = SparseRatings(w["ratings"].rowptr, w["ratings"].col, w["ratings"].val, I_CAT - 1)
    with pytest.raises(ValueError, match="29 columns"):
        explain_items(m, w["users"], w["items"], (w["feats"], short))
    # everything above passed: the next refusal is the device's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        explain_items(m, w["users"], w["items"], w["profiles"])


# ------------------------------------------------------------------------------------------------ AttentionNCF.explain
def test_model_explain_refuses_before_the_device(world, monkeypatch):
    w, m = world, world["model"]
    call = lambda **kw: m.explain(*{**dict(f=w["feats"], r=w["ratings"], u=w["users"], i=w["items"], t=w["thr"], E=8), **kw}.values())
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            call()
    finally:
        m.eval()
    with pytest.raises(TypeError, match="SparseRatings"):
        call(r=(w["ratings"].rowptr, w["ratings"].col))
    with pytest.raises(ValueError, match="30 columns"):
        call(f=w["feats"][:29])
    for users in (w["users"].to(torch.int32), w["users"][:, None]):
        with pytest.raises(ValueError, match="user_rows must be a 1-D int64 tensor"):
            call(u=users)
    for items in (w["items"].to(torch.int32), w["items"][0], w["items"][:2]):
        with pytest.raises(ValueError, match=r"items must be a \(3, k\) int64 tensor"):
            call(i=items)
    for thr in (w["thr"].double(), w["thr"][:2], w["thr"][:, None]):
        with pytest.raises(ValueError, match=r"thr must be a \(3,\) fp32 tensor"):
            call(t=thr)
    for E in (0, 65):
        with pytest.raises(ValueError, match=rf"max_reasons = {E} is outside 1 \.\. 64"):
            call(E=E)
    nbytes = 4 * I_CAT * I_CAT
    monkeypatch.setattr(AttentionNCF, "cross_table_max_bytes", nbytes - 1)
    with pytest.raises(ValueError, match=rf"{nbytes} bytes.*AttentionNCF\.cross_table_max_bytes = {nbytes - 1}"):
        call()
    monkeypatch.setattr(AttentionNCF, "cross_table_max_bytes", nbytes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # the table fits; user_emb = 40 is no obstacle: the device is next
        call()


# ------------------------------------------------------------------------------------------------ native.attn_explain
def test_binding_refuses_before_the_device(native):
    ST = torch.zeros(10, 12)[:, :10]
    rowptr, col, val = torch.tensor([0, 2, 3]), torch.tensor([1, 4, 9], dtype=torch.int32), torch.ones(3)
    users, items, thr = torch.tensor([1, 0, 1]), torch.tensor([[3, -1], [0, 9], [2, 2]]), torch.full((3,), 0.25)
    base = dict(ST=ST, rowptr=rowptr, col=col, val=val, user_rows=users, items=items, thr=thr, max_reasons=4)
    call = lambda **kw: native.attn_explain(**{**base, **kw})
    assert native.ATTN_EXPLAIN_MAX_REASONS == 64
    for E in (0, 65):
        with pytest.raises(ValueError, match="max_reasons"):
            call(max_reasons=E)
    with pytest.raises(ValueError, match="ST must be 2-D with unit inner stride"):
        call(ST=ST.t())
    with pytest.raises(ValueError, match="ST must be 2-D"):
        call(ST=ST[0])
    with pytest.raises(TypeError, match="ST must be fp32"):
        call(ST=ST.double())
    for kw in (dict(rowptr=rowptr.to(torch.int32)), dict(col=col.long()), dict(val=val.double())):
        with pytest.raises(TypeError, match="CSR must be"):
            call(**kw)
    for kw in (dict(val=val[:2]), dict(rowptr=rowptr[:0]), dict(col=col[:, None], val=val[:, None])):
        with pytest.raises(ValueError, match="CSR must be 1-D"):
            call(**kw)
    for u in (users.to(torch.int32), users[:, None], torch.arange(6)[::2]):
        with pytest.raises(ValueError, match="index tensors must be contiguous 1-D int64"):
            call(user_rows=u)
    for it in (items.to(torch.int32), items[:2], items[0], items.t().contiguous().t()):
        with pytest.raises(ValueError, match=r"items must be a contiguous \(3, k\) int64 tensor"):
            call(items=it)
    for t in (thr.double(), thr[:2], thr[:, None]):
        with pytest.raises(ValueError, match=r"thr must be a contiguous \(3,\) fp32 tensor"):
            call(thr=t)
    good = (torch.zeros(3, 2, 4, dtype=torch.int32), torch.zeros(3, 2, 4), torch.zeros(3, 2, 4), torch.zeros(3, 2, dtype=torch.int32))
    for k, wrong in ((0, torch.zeros(3, 2, 4, dtype=torch.int64)), (1, torch.zeros(3, 2, 5)), (2, torch.zeros(3, 4, 2).transpose(1, 2)),
                     (3, torch.zeros(3, 2))):
        out = list(good)
        out[k] = wrong
        with pytest.raises(ValueError, match="out must be contiguous"):
            call(out=tuple(out))
    with pytest.raises(ValueError, match="out must be contiguous"):
        call(out=good[:3])
    with pytest.raises(RuntimeError, match="must live on the GPU"):    # every host check passed
        call()
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        call(out=good)


# ------------------------------------------------------------------------------------------------ ncf_attn_explain
def test_entry_point_refuses_before_launching(native):
    """Stand-in pointers: every row is refused (or accepted as empty) before anything is launched."""
    lib, P = native.load_library(), 16
    EINVAL, EUNSUP, OK = native.NCF_EINVAL, native.NCF_EUNSUPPORTED, native.NCF_OK
    assert lib.ncf_attn_explain_max_reasons() == 64
    assert len(native.SIGNATURES["ncf_attn_explain"][1]) == 20 and native.SIGNATURES["ncf_attn_explain_max_reasons"][1] == []
    ex = lambda **kw: lib.ncf_attn_explain(*{**dict(st=P, ldst=100, Ir=100, Ic=100, rowptr=P, col=P, val=P, n_rows=4, user_rows=P, U=4,
                                                    items=P, k=3, thr=P, E=8, rcol=P, rw=P, rval=P, rcnt=P, oob=None, stream=None),
                                             **kw}.values())
    for E in (0, -1, 65, 1 << 20):
        assert ex(E=E) == EUNSUP and b"max_reasons" in lib.ncf_last_error()
    assert ex(E=0, U=0) == EUNSUP                                      # the shape refusal comes first, also for an empty call
    assert ex(U=0, st=None, items=None) == OK and ex(k=0, rcol=None) == OK
    for name in ("st", "rowptr", "user_rows", "items", "thr", "rcol", "rw", "rval", "rcnt"):
        assert ex(**{name: None}) == EINVAL and b"null" in lib.ncf_last_error(), name
    for kw in (dict(Ir=-1), dict(Ic=-1), dict(n_rows=-1), dict(U=-1), dict(k=-1)):
        assert ex(**kw) == EINVAL and b"bad sizes" in lib.ncf_last_error(), kw
    assert ex(ldst=99) == EINVAL and b"leading dimension" in lib.ncf_last_error()
    assert ex(U=1 << 40, k=1 << 10) == EUNSUP and b"workgroups" in lib.ncf_last_error()
    from deeprecommendation_amd.csrc import build
    assert "attn_explain.hip" in build.SOURCES
