"""CPU tests of the SLIM baseline: the two numpy restatements of tests/slim_ref.py against each other (screening is exact), the
restatement against scikit-learn's ElasticNet and against its own float64 optimality conditions, and the refusals of
``baselines.SLIM`` and ``native.slim_solve`` that need no device."""
import re

import numpy as np
import pytest
import torch

import ease_ref as E
import slim_ref as S


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def test_the_header_the_binding_and_the_shared_cases_agree():
    from conftest import ROOT
    from deeprecommendation_amd import native
    import os
    txt = open(os.path.join(ROOT, "include", "ncf_abi.h")).read()
    assert int(re.search(r"#define\s+NCF_SLIM_MAX_ITEMS\s+(\d+)", txt).group(1)) == native.SLIM_MAX_ITEMS == 32768
    assert "ncf_slim_solve" in native.SIGNATURES
    assert [S.CASES[n][0][:2] for n in "ABCSW"] == [(400, 96), (1500, 257), (3000, 600), (400, 96), (3000, 2100)]
    assert S.CASES["C"][2] == tuple(range(0, 600, 6)) and len(S.CASES["W"][2]) == 48 and S.CASES["W"][2][:32] == tuple(range(32))


# ------------------------------------------------------------------ 1. screening is exact
@pytest.mark.parametrize("T", [1, 64, 100, 1024])
def test_the_screened_loop_is_the_serial_loop_bit_for_bit(T):
    _, _, G = S.gram("B")
    cols = tuple(range(0, 257, 16))
    l1, l2 = S.CASES["B"][1]
    want = _serial_B(cols)
    assert want[1].max() > 20 and (want[3] <= S.TOL).all()              # a real descent, and every column converged under the cap
    assert _same(S.solve(G, cols, l1, l2, T=T), want)


_serial = {}


def _serial_B(cols):
    if cols not in _serial:
        _serial[cols] = S.solve(S.gram("B")[2], cols, *S.CASES["B"][1], serial=True)
    return _serial[cols]


def test_the_screened_loop_is_the_serial_loop_signed_warm_and_capped():
    _, _, G = S.gram("S")
    cols = tuple(range(0, 96, 7))
    l1, l2 = S.CASES["S"][1]
    want = S.solve(G, cols, l1, l2, positive=False, max_sweeps=500, serial=True)
    assert (want[0] < 0).any() and (want[3] <= S.TOL).all()
    assert _same(S.solve(G, cols, l1, l2, positive=False, max_sweeps=500, T=64), want)
    capped = S.solve(G, cols, l1, l2, positive=False, max_sweeps=3, serial=True)
    assert (capped[1] == 3).all() and (capped[3] > S.TOL).any()
    assert _same(S.solve(G, cols, l1, l2, positive=False, max_sweeps=3, T=100), capped)
    Wt0 = np.zeros((96, 96), np.float32)
    Wt0[list(cols)] = S.solve(G, cols, 2 * l1, l2, positive=False, max_sweeps=500)[0]
    Wt0[7, 7] = 3.0                                                     # a warm row's own coordinate is read as +0.0
    warm = S.solve(G, cols, l1, l2, positive=False, Wt0=Wt0, max_sweeps=500, serial=True)
    assert _same(S.solve(G, cols, l1, l2, positive=False, Wt0=Wt0, max_sweeps=500, T=64), warm)
    assert warm[1].sum() < want[1].sum() and not warm[0][1, 7]           # the warm path needs fewer sweeps
    assert _same(S.solve(G, cols, l1, l2, positive=False, Wt0=np.zeros((96, 96), np.float32), max_sweeps=500), want)


@pytest.mark.parametrize("name", ["A", "B", "C", "S"])
def test_every_listed_column_of_the_shared_cases_converges_under_its_cap(name):
    """The condition the GPU tests rest on: no cap hides a column.  Sweeps measured: A 56, B 92, C 78, S 114 (W: 94)."""
    s = S.solved(name)
    print(f"case {name}: sweeps <= {s['sweeps'].max()}, steps {s['steps'].sum()}, last <= {s['last'].max():.3e}")
    assert (s["last"] <= S.TOL).all() and s["sweeps"].max() < s["cap"]
    assert s["sweeps"].max() <= {"A": 56, "B": 92, "C": 83, "S": 114}[name]
    assert (s["W"] < 0).any() == (name == "S")
    assert not s["W"][np.arange(len(s["cols"])), s["cols"]].any()        # diag(W) = 0


# ------------------------------------------------------------------ 2. scikit-learn
def test_the_restatement_is_scikit_learns_elastic_net():
    """Measured: supports identical, max |dw| = 4.7e-6 with max |w| = 0.27; the bound is ten times that, because the fp32 drift of q
    differs by column."""
    lm = pytest.importorskip("sklearn.linear_model")
    csr, I, G = S.gram("A")
    U = len(csr[0]) - 1
    l1, l2 = S.CASES["A"][1]
    cols = tuple(range(0, 96, 5))
    W, sweeps, _, last = S.solve(G, cols, l1, l2, max_sweeps=500, tol=1e-6)
    assert (last <= 1e-6).all() and sweeps.max() < 500
    X = E.dense64(*csr, I)
    worst = 0.0
    for c, j in enumerate(cols):
        Xj = X.copy()
        Xj[:, j] = 0.0
        m = lm.ElasticNet(alpha=(l1 + l2) / U, l1_ratio=l1 / (l1 + l2), positive=True, fit_intercept=False, tol=1e-12,
                          max_iter=100000).fit(Xj, X[:, j])
        assert np.array_equal(m.coef_ != 0, W[c] != 0), j
        worst = max(worst, float(np.abs(m.coef_ - W[c]).max()))
    print(f"max |w - ElasticNet| = {worst:.3e}, max |w| = {np.abs(W).max():.3f}")
    assert worst <= 5e-5


# ------------------------------------------------------------------ 3. optimality
@pytest.mark.parametrize("name,measured", [("A", 1.172e-4), ("B", 1.607e-4)])
def test_the_restatement_meets_its_float64_optimality_conditions(name, measured):
    """The largest KKT violation over the columns, relative to max G, held to 4 x the measured figure (A 1.172e-4, B 1.607e-4).
    The figure is the stopping rule's: a weight may still be tol = 1e-4 from its coordinate-wise optimum, times d + l2 of about
    max G."""
    s = S.solved(name)
    worst = max(S.kkt(s["G"], int(j), s["W"][c], s["l1"], s["l2"], s["positive"]) for c, j in enumerate(s["cols"]))
    print(f"case {name}: KKT {worst:.3e} of max G = {s['G'].max()}")
    assert worst <= 4 * measured


# ------------------------------------------------------------------ 4. host refusals
@pytest.mark.parametrize("kw", [dict(l1_reg=-1.0, l2_reg=1.0), dict(l1_reg=1.0, l2_reg=float("inf")), dict(l1_reg=float("nan"), l2_reg=1.0),
                                dict(l1_reg=True, l2_reg=1.0), dict(l1_reg="1", l2_reg=1.0), dict(l1_reg=1.0, l2_reg=1.0, tol=-1e-3),
                                dict(l1_reg=1.0, l2_reg=1.0, tol=float("nan")), dict(l1_reg=1.0, l2_reg=1.0, max_sweeps=0),
                                dict(l1_reg=1.0, l2_reg=1.0, max_sweeps=10.0), dict(l1_reg=1.0, l2_reg=1.0, max_sweeps=True),
                                dict(l1_reg=1.0, l2_reg=1.0, binary=1), dict(l1_reg=1.0, l2_reg=1.0, positive="yes")])
def test_slim_refuses_bad_hyper_parameters(kw):
    from deeprecommendation_amd import baselines
    with pytest.raises(ValueError, match="^SLIM: "):
        baselines.SLIM(**kw)


def test_slim_takes_numpy_scalars_and_scikit_learns_parameters():
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd import baselines, recommend
    assert "SLIM" in pkg._BASELINES and pkg.SLIM is baselines.SLIM
    for name in ("slim_top_k", "slim_ranks"):
        assert name in pkg._RECOMMEND and getattr(pkg, name) is getattr(recommend, name)
    m = pkg.SLIM(np.float32(2.0), np.int64(3), positive=np.bool_(False), max_sweeps=np.int32(7), tol=0.0, binary=np.bool_(True))
    assert (m.l1_reg, m.l2_reg, m.positive, m.max_sweeps, m.tol, m.binary) == (2.0, 3.0, False, 7, 0.0, True)
    d = pkg.SLIM(1.0, 2.0)
    assert (d.positive, d.max_sweeps, d.tol, d.binary) == (True, 100, 1e-4, False)
    e = pkg.SLIM.elastic_net(0.015, 1.0 / 6.0, 400, max_sweeps=50)
    assert e.l1_reg == 0.015 * (1.0 / 6.0) * 400 and e.l2_reg == 0.015 * (1.0 - 1.0 / 6.0) * 400 and e.max_sweeps == 50
    for bad in (dict(alpha=-1.0, l1_ratio=0.5, num_users=10), dict(alpha=1.0, l1_ratio=1.5, num_users=10),
                dict(alpha=1.0, l1_ratio=0.5, num_users=0)):
        with pytest.raises(ValueError, match=r"^SLIM\.elastic_net: "):
            pkg.SLIM.elastic_net(**bad)


def test_slim_has_no_cpu_path_and_refuses_before_it_allocates():
    from deeprecommendation_amd import baselines, native, recommend
    m = baselines.SLIM(1.0, 2.0)
    u, i, r = torch.tensor([0, 1]), torch.tensor([1, 0]), torch.tensor([1.0, 2.0])
    with pytest.raises(RuntimeError, match=r"SLIM\.fit runs on the GPU: the samples must live on one GPU .*no CPU path"):
        m.fit(u, i, r, 2, 2)
    rowptr, col, val = torch.tensor([0, 1, 2]), torch.tensor([1, 0], dtype=torch.int32), torch.tensor([1.0, 2.0])
    with pytest.raises(RuntimeError, match=r"SLIM\.fit_csr runs on the GPU: the CSR must live on one GPU .*no CPU path"):
        m.fit_csr(rowptr, col, val, 2)
    with pytest.raises(ValueError, match=f"^SLIM: {native.SLIM_MAX_ITEMS + 1} items"):
        m.fit_csr(rowptr, col, val, native.SLIM_MAX_ITEMS + 1)
    with pytest.raises(ValueError, match="^SLIM: nothing to fit"):
        m.fit_csr(rowptr, col[:0], val[:0], 2)
    for bad in ([1.0, 2.0], [(1.0, 2.0, 3.0)], [(1.0, -2.0)]):
        with pytest.raises(ValueError, match="^SLIM: "):
            m.fit_csr(rowptr, col, val, 2, at_regs=bad)
    with pytest.raises(ValueError, match="^SLIM: warm_path"):
        m.fit_csr(rowptr, col, val, 2, warm_path=1)
    for call in (lambda: m.check(), lambda: m.scores((rowptr, col, val), u), lambda: m.predict((rowptr, col, val), u, i),
                 lambda: m.similar_items(i, 1), lambda: recommend.slim_top_k(m, (rowptr, col, val), u, 1),
                 lambda: recommend.slim_ranks(m, (rowptr, col, val), u, (rowptr, col))):
        with pytest.raises(RuntimeError, match="SLIM: not fitted"):
            call()


def test_slim_solve_checks_its_arguments_before_the_device():
    from deeprecommendation_amd import native
    G = torch.eye(4)
    for kw, text in ((dict(l1=-1.0, l2=1.0), "l1"), (dict(l1=1.0, l2=float("nan")), "l2"), (dict(l1=1.0, l2=1.0, tol=-1.0), "tol"),
                     (dict(l1=1.0, l2=1.0, max_sweeps=0), "max_sweeps"), (dict(l1=1.0, l2=1.0, max_sweeps=2.5), "max_sweeps"),
                     (dict(l1=1.0, l2=1.0, positive=1), "positive"), (dict(l1=1.0, l2=1.0, warm=True), "warm start"),
                     (dict(l1=1.0, l2=1.0, cols=torch.tensor([0, 1])), "cols"), (dict(l1=1.0, l2=1.0, out=torch.zeros(4, 5)), "out"),
                     (dict(l1=1.0, l2=1.0, out=torch.zeros(4, 4, dtype=torch.float64)), "out")):
        with pytest.raises(ValueError, match="^slim_solve: .*" + text):
            native.slim_solve(G, **kw)
    with pytest.raises(ValueError, match="^slim_solve: G must be square"):
        native.slim_solve(torch.zeros(3, 4), 1.0, 1.0)
    with pytest.raises(ValueError, match="^slim_solve: G must be a 2-D float32"):
        native.slim_solve(G.double(), 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        native.slim_solve(G, 1.0, 1.0)
