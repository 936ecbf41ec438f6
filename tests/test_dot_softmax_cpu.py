"""CPU: what tests/dot_softmax_ref.py states is right before the GPU tests lean on it (its float64 reference against torch.autograd
through float64 F.cross_entropy; its restated launch plans against ncf_dot_softmax_plan; the forms its cases must reach), the
entry points are declared, bound and exported, and the host-side refusals of fit_implicit(loss="softmax")."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dot_softmax_ref as R
from deeprecommendation_amd import implicit, native

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ncf_abi.h")
SYMBOLS = ("ncf_dot_lse", "ncf_dot_lse_workspace_bytes", "ncf_dot_softmax_grad", "ncf_dot_softmax_grad_workspace_bytes")


def test_the_reference_is_torch_autograd_through_float64_cross_entropy():
    gen = torch.Generator().manual_seed(5)
    B, N, D, scale = 9, 23, 7, 0.5
    U = torch.randn(B, D, dtype=torch.float64, generator=gen, requires_grad=True)
    V = torch.randn(N, D, dtype=torch.float64, generator=gen, requires_grad=True)
    t = torch.randint(0, N, (B,), generator=gen)
    g = torch.randn(B, dtype=torch.float64, generator=gen)
    ref = R.reference(U.detach(), V.detach(), t, g, scale)
    loss = F.cross_entropy(U @ V.t() * scale, t, reduction="none")
    (loss * g).sum().backward()
    assert float((ref["loss"] - loss.detach()).abs().max()) <= 1e-12
    assert float((ref["dA"] - U.grad).abs().max()) <= 1e-12
    assert float((ref["dQ"] - V.grad).abs().max()) <= 1e-12
    # the sums of absolute terms bound the gradients they are the tolerance of
    assert bool((ref["absA"] >= ref["dA"].abs() - 1e-12).all()) and bool((ref["absQ"] >= ref["dQ"].abs() - 1e-12).all())


def test_the_header_declares_the_symbols_and_the_library_exports_them():
    text = open(HEADER).read()
    lib = native.load_library()
    for sym in SYMBOLS + ("ncf_dot_softmax_plan",):
        assert re.search(r"\b(int|size_t) %s\(" % sym, text), sym
        assert sym in native.SIGNATURES
        assert getattr(lib, sym) is not None
    assert callable(native.dot_lse) and callable(native.dot_softmax_grad)


def test_the_restated_plans_are_the_librarys_and_the_cases_reach_every_form():
    kinds = ("lse", "grad_rows", "grad_items")
    shapes = [(c[0], c[1], c[2]) for c in R.CASES.values()] + [(65536, 20000, 64), (65536, 3706, 128), (4096, 8192, 64), (1, 1 << 24, 256),
                                                               (65536, 1, 1), (700, 513, 33)]
    for rows, cols, D in shapes:
        for kind in kinds:
            assert native.dot_softmax_plan(kind, rows, cols, D) == R.plan(kind, rows, cols, D), (kind, rows, cols, D)
    reached = [set(), set(), set()]
    for name, (B, N, D, *_rest) in R.CASES.items():
        forms = tuple(R.form(kind, B, N, D) for kind in kinds)
        assert forms == R.FORMS[name], (name, forms)
        for k in range(3):
            reached[k].add(forms[k])
    assert reached[0] == {"one", "multi"}
    assert reached[1] == reached[2] == {"one", "multi", "multi+chunked"}
    # the partial outputs never scale with rows x cols: at most 8 Mi floats, or one 64-row block of tiles
    for rows, cols, D in shapes:
        for kind, items in (("grad_rows", 0), ("grad_items", 1)):
            tile, tiles, chunk = R.plan(kind, rows, cols, D)
            nbytes = native.load_library().ncf_dot_softmax_grad_workspace_bytes(rows, cols, D, items)
            assert nbytes == (tiles * chunk * D * 4 if tiles > 1 else 0)
            assert nbytes <= max(R.PARTIAL_FLOATS, tiles * R.BLOCK * D) * 4
        tile, tiles, _ = R.plan("lse", rows, cols, D)
        assert native.load_library().ncf_dot_lse_workspace_bytes(rows, cols, D) == tiles * rows * 8


def test_the_cases_keep_what_the_tolerances_assume():
    for name in R.CASES:
        c = R.case(name)
        B, N = c.B, c.N
        assert max(B, N) <= 4224                              # the fp32 sums' length behind the 64 eps32 of the gradient bar
        p_t = torch.softmax(c.ref["z"], 1)[torch.arange(B), c.t]
        if name == "confident":                               # every target is the row's largest logit, many of them near 1
            assert bool((c.ref["z"].max(1).values == c.ref["z"][torch.arange(B), c.t]).all())
            assert int(((p_t > 0.9) & (c.g != 0)).sum()) >= 10
            assert float(c.ref["confA"].max()) <= 2.0 ** -10 * float((c.g.abs().max() * c.scale) * c.Q.abs().max())
        else:
            assert bool(((p_t <= 0.5) | (c.g == 0)).all()), name
        if c.idxA is not None:
            assert len(np.unique(c.idxA)) < B                 # a repeated user
    c = R.case("peaked")
    assert float(c.ref["z"].abs().max()) == 120.0
    z = c.ref["z"][c.peaked_rows]
    top2 = torch.topk(z, 2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) >= 100.0
    assert torch.equal(c.ref["lse"][c.peaked_rows].float(), torch.full((len(c.peaked_rows),), 120.0))
    z0 = R.case("zero")
    assert torch.allclose(z0.ref["lse"], torch.full((z0.B,), float(np.log(z0.N)), dtype=torch.float64), rtol=0, atol=1e-12)
    u = R.case("unit")
    # the indicator case: out[r][d] is the sum of w over the walked rows c with c mod D == d
    w = u.ref["w"]
    want = torch.stack([w[:, d::u.D].sum(1) for d in range(u.D)], 1)
    assert float((want - u.ref["dA"]).abs().max()) <= 1e-12


class _NoData:
    """Raises on any attribute: fit_implicit must refuse before it looks at ``data``."""

    def __getattr__(self, name):
        raise AssertionError(f"data.{name} was examined")


def test_fit_implicit_refuses_a_model_without_a_dot_product_readout_before_the_data():
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    assert "softmax" in implicit.LOSSES
    ncf = BasicNCF(item_dim=5, user_dim=4, item_emb=8, user_emb=8, mlp_dense_layers=[8])
    with pytest.raises(TypeError, match="MF.*GraphNCF\\(use_dot_product=True\\)"):
        implicit.fit_implicit(ncf, _NoData(), loss="softmax", epochs=1, batch_size=4, lr=0.1)
    mf = MF(item_dim=5, user_dim=4, item_emb=8, user_emb=8)
    with pytest.raises(ValueError, match="mse"):
        implicit.fit_implicit(mf, _NoData(), loss="mse", epochs=1, batch_size=4, lr=0.1)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            implicit.fit_implicit(mf, _NoData(), loss="softmax", scale=bad, epochs=1, batch_size=4, lr=0.1)
    with pytest.raises(ValueError, match="batch_size"):                       # the rows one ncf_dot_lse call takes
        implicit.fit_implicit(mf, _NoData(), loss="softmax", epochs=1, batch_size=native.DOT_SOFTMAX_MAX_ROWS + 1, lr=0.1)
    with pytest.raises(TypeError, match="ImplicitFeedback"):                  # a dot-product model passes the check; the data is next
        implicit.fit_implicit(mf, object(), loss="softmax", epochs=1, batch_size=4, lr=0.1)


def test_the_host_refusals_of_the_entry_points():
    """Made before any pointer is read, so stand-in pointers do: each with its code and a message naming the entry point."""
    lib = native.load_library()
    p = 4096                                                   # an aligned stand-in address that is never dereferenced

    def lse(rows=4, cols=4, D=8, ldA=8, ldB=8, rowsA=4, rowsB=4, tabA=p, idxA=None, scale=1.0, out=p, ws=p, nbytes=1 << 20):
        return lib.ncf_dot_lse(tabA, rowsA, ldA, p, rowsB, ldB, idxA, None, rows, cols, D, scale, out, None, ws, nbytes, None, None)

    def grad(rows=4, cols=4, D=8, ldA=8, ldB=8, rowsA=4, rowsB=4, tabA=p, idxA=None, scale=1.0, out=p, ws=p, nbytes=1 << 20, t=p, items=0):
        return lib.ncf_dot_softmax_grad(tabA, rowsA, ldA, p, rowsB, ldB, idxA, None, rows, cols, D, t, p, p, scale, items, out, ws, nbytes,
                                        None, None)

    for fn, name in ((lse, b"ncf_dot_lse"), (grad, b"ncf_dot_softmax_grad")):
        for kw, code, word in ((dict(D=0), native.NCF_EUNSUPPORTED, b"width"), (dict(D=257), native.NCF_EUNSUPPORTED, b"width"),
                               (dict(tabA=None), native.NCF_EINVAL, b"null"), (dict(out=None), native.NCF_EINVAL, b"null"),
                               (dict(ldA=7), native.NCF_EINVAL, b"leading dimension"), (dict(ldB=7), native.NCF_EINVAL, b"leading dimension"),
                               (dict(rows=5), native.NCF_EINVAL, b"rowsA"), (dict(cols=5), native.NCF_EINVAL, b"rowsB"),
                               (dict(scale=0.0), native.NCF_EINVAL, b"scale"), (dict(scale=-1.0), native.NCF_EINVAL, b"scale"),
                               (dict(scale=float("inf")), native.NCF_EINVAL, b"scale"), (dict(scale=float("nan")), native.NCF_EINVAL, b"scale")):
            assert fn(**kw) == code, (name, kw)
            err = lib.ncf_last_error()
            assert name in err and word in err, (name, kw, err)
        assert fn(rows=0, tabA=None, out=None) == native.NCF_OK          # nothing to do: nothing is looked at
    assert grad(t=None) == native.NCF_EINVAL and b"ncf_dot_softmax_grad: null" in lib.ncf_last_error()
    # a short workspace: the multi-tile forms need one (rows = 64, cols = 2047: 32 column tiles)
    assert lse(rows=64, cols=2047, rowsA=64, rowsB=2047, nbytes=16) == native.NCF_EWORKSPACE
    assert b"ncf_dot_lse_workspace_bytes" in lib.ncf_last_error()
    assert grad(rows=64, cols=2047, rowsA=64, rowsB=2047, nbytes=16) == native.NCF_EWORKSPACE
    assert b"ncf_dot_softmax_grad_workspace_bytes" in lib.ncf_last_error()
    assert lib.ncf_dot_softmax_plan(3, 4, 4, 8, None, None, None) == native.NCF_EINVAL and b"kind" in lib.ncf_last_error()
