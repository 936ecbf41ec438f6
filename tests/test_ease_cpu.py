"""CPU tests of the EASE baseline: the numpy restatements of tests/ease_ref.py against the float64 closed form on the four shared
cases, the KKT identity of the closed form, and the refusals of ``baselines.EASE`` that need no device."""
import numpy as np
import pytest
import torch

import ease_ref as E

CASE_IDS = range(len(E.CASES))


def test_the_panel_width_of_the_restatement_is_the_headers_and_the_bindings():
    from deeprecommendation_amd import native
    assert E.NB == native.EASE_BLOCK


@pytest.mark.parametrize("c", CASE_IDS)
def test_gram_restatement_is_the_dense_product_and_symmetric_bit_for_bit(c):
    s = E.solved(c)
    G = s["G"]
    assert G.dtype == np.float32 and np.array_equal(G.view(np.int32), G.T.copy().view(np.int32))
    X = E.dense64(*s["csr"], s["I"])
    assert np.array_equal(G.astype(np.float64), X.T @ X)                # small integers: every partial sum is exact in fp32


@pytest.mark.parametrize("c", CASE_IDS)
def test_blocked_fp32_inverse_and_weights_against_float64(c):
    """The yardstick's own figures (printed: they are what DESIGN quotes).  fp32 has 2^-24 = 6e-8 of relative rounding per
    operation and the condition numbers are in the hundreds, so 1e-5 of the largest entry is a loose ceiling that a broken
    restatement (a wrong sign, a missed panel) misses by orders of magnitude."""
    s = E.solved(c)
    A = s["G"].astype(np.float64) + s["lam"] * np.eye(s["I"])
    print(f"case {E.CASES[c]}: cond {np.linalg.cond(A):.0f}, blocked fp32 |P - P64| / max|P64| = {s['err_P']:.3e}, "
          f"|W - W64| / max|W64| = {s['err_W']:.3e}, residual {s['res']:.3e}, kkt {s['kkt']:.3e} of max|G| {s['G'].max():.0f}")
    assert s["err_P"] < 1e-5 and s["err_W"] < 1e-5
    assert s["res"] < 1e-4
    assert np.array_equal(np.diag(s["Wb"]), np.zeros(s["I"], np.float32)) and not np.signbit(np.diag(s["Wb"])).any()


@pytest.mark.parametrize("c", CASE_IDS)
def test_kkt_identity_of_the_float64_closed_form(c):
    s = E.solved(c)
    assert E.kkt(s["G"], s["lam"], s["W64"]) <= 1e-9 * float(s["G"].max())


def test_a_single_panel_is_the_scalar_elimination_and_a_bad_pivot_gives_zeros():
    s = E.solved(0)
    G, lam = s["G"], s["lam"]
    one = E.blocked_inverse_ref(G, lam, nb=len(G))
    A = G.copy()
    A[np.arange(len(G)), np.arange(len(G))] += np.float32(lam)
    assert np.array_equal(one, E.diag_inverse_ref(A))
    for nb in (7, 32, 50):                                             # any panel width inverts, partial last panel included
        assert E.rel_err(E.blocked_inverse_ref(G, lam, nb=nb), s["P64"]) < 1e-5
    bad = G.copy()
    bad[3, 3] = -1.0
    assert not E.blocked_inverse_ref(bad, 1e-3, nb=32).any()
    bad = G.copy()
    bad[5, 40] = np.nan
    assert not E.blocked_inverse_ref(bad, lam, nb=32).any()


def test_scores_and_predict_restatements_against_the_dense_product():
    s = E.solved(1)
    rowptr, col, val = s["csr"]
    W = s["Wb"]
    users = [0, 7, 1499, 7]
    got = E.scores_ref(rowptr, col, val, users, W)
    want = E.dense64(rowptr, col, val, s["I"])[users] @ W.astype(np.float64)
    assert np.abs(got - want).max() <= 64 * 2.0 ** -24 * np.abs(want).max() + 1e-12
    part = E.scores_ref(rowptr, col, val, users, W, (60, 131))
    assert np.array_equal(part.view(np.int32), got[:, 60:131].view(np.int32))
    pred = E.predict_ref(rowptr, col, val, [0, 7, 1499], [3, 200, 256], W)
    assert np.array_equal(pred.view(np.int32), got[[0, 1, 2], [3, 200, 256]].view(np.int32))
    assert not E.scores_ref(rowptr, col, val, [-1, 1500], W).any()


def test_planted_case_holds_all_but_one_item_of_a_block():
    (rowptr, col, val), held = E.planted_case()
    assert len(rowptr) == 41 and (np.diff(rowptr) == 7).all() and len(held) == 40
    W = E.weights_ref(E.inverse64(E.gram_ref(rowptr, col, val, 24), 1.0))
    s = E.dense64(rowptr, col, val, 24) @ W
    s[np.repeat(np.arange(40), 7), col] = -np.inf
    assert np.array_equal(s.argmax(1), held)


# ------------------------------------------------------------------ refusals that need no device
@pytest.mark.parametrize("reg", [0.0, -1.0, float("nan"), float("inf"), True, "500", None])
def test_constructor_refuses_a_reg_that_is_not_a_positive_finite_number(reg):
    from deeprecommendation_amd import baselines
    with pytest.raises(ValueError, match="^EASE: "):
        baselines.EASE(reg=reg)


def test_constructor_takes_numpy_scalars_and_refuses_a_binary_that_is_no_bool():
    import deeprecommendation_amd as pkg
    m = pkg.EASE(reg=np.float32(250.0), binary=np.bool_(True))
    assert m.reg == 250.0 and m.binary is True and pkg.EASE().reg == 500.0 and pkg.EASE().binary is False
    with pytest.raises(ValueError, match="^EASE: binary"):
        pkg.EASE(binary=1)


def test_fit_refuses_cpu_tensors_and_wrong_dtypes_and_an_unfitted_model_says_so():
    from deeprecommendation_amd import baselines
    m = baselines.EASE()
    u, i, r = torch.tensor([0, 1, 2]), torch.tensor([1, 0, 1]), torch.ones(3)
    with pytest.raises(RuntimeError, match=r"EASE\.fit runs on the GPU: the samples must live on one GPU .*no CPU path"):
        m.fit(u, i, r, 3, 2)
    for bad in ((u.to(torch.int32), i, r), (u, i.to(torch.int32), r), (u, i, r.double()), (u, i[:2], r)):
        with pytest.raises(ValueError, match="^EASE: "):
            m.fit(*bad, 3, 2)
    rowptr, col = torch.tensor([0, 1, 2, 3]), torch.tensor([1, 0, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"EASE\.fit_csr runs on the GPU: the CSR must live on one GPU .*no CPU path"):
        m.fit_csr(rowptr, col, r, 2)
    with pytest.raises(ValueError, match="^EASE"):
        m.fit_csr(rowptr, col, r.double(), 2)
    with pytest.raises(ValueError, match="^EASE: "):
        m.fit_csr(rowptr, col, r, 2, at_regs=[10.0, -1.0])
    for call in (m._fitted, m.check, lambda: m.scores((rowptr, col, r), u), lambda: m.predict((rowptr, col, r), u, i),
                 lambda: m.similar_items(i, 2)):
        with pytest.raises(RuntimeError, match="EASE: not fitted"):
            call()
    import deeprecommendation_amd as pkg
    for front in (lambda: pkg.ease_top_k(m, (rowptr, col, r), u, 2), lambda: pkg.ease_ranks(m, (rowptr, col, r), u, (rowptr, col))):
        with pytest.raises(RuntimeError, match="EASE: not fitted"):
            front()


def test_wrappers_check_before_the_device_is_touched():
    from deeprecommendation_amd import native
    A = torch.zeros((4, 4))
    with pytest.raises(ValueError, match="ease_invert: lam"):
        native.ease_invert(A, 0.0)
    with pytest.raises(ValueError, match="ease_invert: A must be square"):
        native.ease_invert(torch.zeros((4, 5)), 1.0)
    with pytest.raises(ValueError, match="ease_invert: A must be a 2-D float32"):
        native.ease_invert(A.double(), 1.0)
    with pytest.raises(RuntimeError, match="A must live on the GPU"):
        native.ease_invert(A, 1.0)
    with pytest.raises(RuntimeError, match="P must live on the GPU"):
        native.ease_weights(A)
    flag = torch.zeros(1, dtype=torch.int32)
    native.check_ease(torch.device("cpu"), flag=flag)
    for word, text in ((native.EASE_FLAG_ORDER, "ascending"), (native.EASE_FLAG_PIVOT, "pivot"), (3, "pivot")):
        flag.fill_(word)
        with pytest.raises(ValueError, match="^EASE: .*" + text):
            native.check_ease(torch.device("cpu"), flag=flag)
        assert int(flag) == 0
