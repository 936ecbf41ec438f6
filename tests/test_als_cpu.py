"""CPU tests of the ImplicitALS baseline: the fp32 restatement of tests/als_ref.py tracks its float64 twin, which is the dense closed
form through numpy.linalg.solve; the float64 objective never rises over the half-sweeps; planted blocks come back; the three entry
points are declared, exported, bound and built with THE CONTRACT in the header; their refusals, the binding's and ImplicitALS's come
before the device; the hoisted CSR builders are numpy's stable sorts."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import als_ref as A


def _lib():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load_library()


def test_fp32_restatement_tracks_its_float64_twin_and_the_closed_form():
    rowptr, col, val = A.base_case()
    worst = 0.0
    for F in A.F_LIST:
        T = A.table(A.I, F, 100 + F)
        (x32, f32), (x64, f64) = A.base_sweep(F), A.base_sweep(F, np.float64)
        dense = A.solve_rows_dense64(rowptr, col, val, np.arange(A.U), T, A.ALPHA, A.REG, F)
        dev, dd = np.abs(x32.astype(np.float64) - x64).max(), np.abs(x64 - dense).max()
        print(f"F={F}: max |fp32 - float64 twin| = {dev:.3e}, |twin - closed form| = {dd:.3e}, max |x| = {np.abs(x64).max():.3f}")
        assert f32 == f64 == 0 and x32.dtype == np.float32 and x64.dtype == np.float64
        # the twin IS the closed form up to float64 rounding: condition numbers near 1e3 (reg = 0.1 under eigenvalues of tens) times
        # F <= 128 roundings of 1.1e-16 on solutions below 4 stay under 1e-12
        assert dd <= 1e-12
        assert not x64[A.U - 1].any() and np.abs(x64).max() > 0.1
        worst = max(worst, dev)
    print(f"worst {worst:.3e}; recorded {A.F32_VS_F64_MEASURED:.3e}")
    assert worst <= 8 * A.F32_VS_F64_MEASURED


def test_gram_restatement_is_the_matrix_product():
    for rows in A.GRAM_ROWS_LIST:
        T, G = A.gram_case(rows, 33)
        T64 = T[:, :33].astype(np.float64)
        assert np.array_equal(G, G.T) and G.dtype == np.float32
        assert np.abs(G - T64.T @ T64).max() <= rows * 2.0 ** -23 * np.abs(T64).max() ** 2 * 2
        assert np.array_equal(A.gram_ref(T, 33, np.float64), np.tril(A.gram_ref(T, 33, np.float64)) + np.tril(A.gram_ref(T, 33, np.float64), -1).T)


def test_base_and_long_cases_hold_what_the_gpu_tests_rely_on():
    rowptr, col, val = A.base_case()
    lens = np.diff(rowptr)
    assert len(col) == A.NNZ and lens[-1] == 0 and not (col == A.I - 1).any() and lens.max() >= 4
    for u in range(A.U):
        assert (np.diff(col[rowptr[u]:rowptr[u + 1]]) > 0).all()
    assert set(np.unique(val * 2)) <= set(range(1, 11))
    lrow, lcol, lval = A.long_case()
    assert tuple(np.diff(lrow)) == A.LONG_LENS and -(-A.LONG_LENS[0] // A.SEG) == 3 and A.LONG_LENS[0] % A.SEG
    for u in range(len(A.LONG_LENS)):
        assert (np.diff(lcol[lrow[u]:lrow[u + 1]]) > 0).all()
    assert (lval == 0).any() and lcol.max() < A.LONG_I


@pytest.mark.parametrize("F", A.F_LIST)
def test_float64_objective_does_not_rise_over_six_half_sweeps(F):
    rowptr, col, val = A.base_case()
    X0, Y0 = A.initial_tables(A.U, A.I, F, A.FIT_SD, A.FIT_SEED, rowptr, col)
    start = A.objective64(rowptr, col, val, X0, Y0, A.ALPHA, A.REG)
    _, _, losses = A.fit_ref(rowptr, col, val, A.I, X0, Y0, 3, A.REG, A.ALPHA, np.float64, loss=True)
    print(f"F={F}: {start:.6f} -> " + ", ".join(f"{v:.6f}" for v in losses))
    assert len(losses) == 6 and all(b <= a for a, b in zip([start] + losses, losses))


def test_planted_blocks_come_back_with_hit_rate_one():
    (rowptr, col, val), held = A.planted_case()
    X, Y = A.planted_fit()
    S = X.astype(np.float64) @ Y.astype(np.float64).T
    S[np.repeat(np.arange(len(held)), np.diff(rowptr)), col] = -np.inf
    assert (S.argmax(1) == held).all()


def test_flags_of_the_restatement():
    rowptr, col, val = (a.copy() for a in A.base_case())
    F, T = 3, A.table(A.I, 3, 103)
    G = A.gram_ref(T, F)
    clean = A.base_sweep(F)[0]
    c = col.copy()
    c[0] = -1
    out, bits = A.solve_rows_ref(rowptr, c, val, np.arange(A.U), T, G, A.ALPHA, A.REG, F)
    assert bits == A.FLAG_COL and out[0].any() and np.array_equal(out[1:], clean[1:])
    c = col.copy()
    c[1] = c[0]
    out, bits = A.solve_rows_ref(rowptr, c, val, np.arange(A.U), T, G, A.ALPHA, A.REG, F)
    assert bits == A.FLAG_ORDER and not out[0].any() and np.array_equal(out[1:], clean[1:])
    v = val.copy()
    v[0] = np.nan
    out, bits = A.solve_rows_ref(rowptr, col, v, np.arange(A.U), T, G, A.ALPHA, A.REG, F)
    assert bits == A.FLAG_VAL and np.isfinite(out).all()
    out, bits = A.solve_rows_ref(rowptr, col, val, np.array([A.U]), T, G, A.ALPHA, A.REG, F)
    assert bits == A.FLAG_PTR and not out.any()
    out, bits = A.solve_rows_ref(rowptr, col, val, np.arange(A.U), T, G - np.float32(1e4) * np.eye(F, dtype=np.float32), A.ALPHA, A.REG, F)
    assert bits == A.FLAG_PIVOT and not out.any()


def test_entry_points_are_declared_exported_bound_and_built():
    from deeprecommendation_amd import native
    from deeprecommendation_amd.csrc import build
    hdr = open(os.path.join(ROOT, "include", "ncf_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("ncf_als_gram", "ncf_als_solve_rows"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    assert re.search(r"\bsize_t\s+ncf_als_gram_workspace_bytes\s*\(", code)
    for define, value in (("NCF_ALS_MAX_FACTORS", A.MAX_FACTORS), ("NCF_ALS_GRAM_ROWS", A.GRAM_ROWS), ("NCF_ALS_SEG", A.SEG)):
        assert re.search(r"#define\s+" + define + r"\s+" + str(value) + r"\b", code), define
    for line in ("P_c[a][b] = +0.0f;  for the chunk's rows t in ascending order, for a >= b:  P_c[a][b] = P_c[a][b] + t[a] * t[b]",
                 "G[a][b] = +0.0f;  for c = 0, 1, ... in that order:  G[a][b] = G[a][b] + P_c[a][b];      G[b][a] = G[a][b]",
                 "w_e = alpha * val_e",
                 "for the entries e of segment s in stored order, for a >= b:  S_s[a][b] = S_s[a][b] + (w_e * t_e[a]) * t_e[b]",
                 "A[a][b] = G[a][b];  for s = 0, 1, ... in that order:  A[a][b] = A[a][b] + S_s[a][b];  then  A[a][a] = A[a][a] + reg",
                 "b[a] = +0.0f;  for ALL the row's entries e in stored order:  b[a] = b[a] + (1.0f + w_e) * t_e[a]",
                 "s = A[j][j];  for k = 0 .. j - 1 in ascending order:  s = s - L[j][k] * L[j][k];      L[j][j] = sqrtf(s)",
                 "for i > j:  v = A[i][j];  for k = 0 .. j - 1 in ascending order:  v = v - L[i][k] * L[j][k];      L[i][j] = v / L[j][j]",
                 "v = b[i];  for k = 0 .. i - 1 in ascending order:  v = v - L[i][k] * z[k];      z[i] = v / L[i][i]",
                 "v = z[i];  for k = F - 1 .. i + 1 in descending order:  v = v - L[k][i] * x[k];      x[i] = v / L[i][i]",
                 "A row without entries is written as zeros, without a solve.",
                 "correctly rounded IEEE operations, hipcc's default for fp32",
                 "same inputs give the same bits for any grid, CU count or blocking of the rows"):
        assert line in hdr, line                                       # the contract is part of the ABI
    lib = _lib()
    for name, nargs in (("ncf_als_gram_workspace_bytes", 2), ("ncf_als_gram", 8), ("ncf_als_solve_rows", 23)):
        assert hasattr(lib, name) and len(native.SIGNATURES[name][1]) == nargs
    for name in ("als_gram", "als_plan", "als_solve_rows", "als_flag", "check_als"):
        assert callable(getattr(native, name))
    assert (native.ALS_MAX_FACTORS, native.ALS_GRAM_ROWS, native.ALS_SEG) == (A.MAX_FACTORS, A.GRAM_ROWS, A.SEG) == (128, 256, 512)
    assert (native.ALS_FLAG_COL, native.ALS_FLAG_PTR, native.ALS_FLAG_ORDER, native.ALS_FLAG_VAL, native.ALS_FLAG_PIVOT) == (1, 2, 4, 8, 16)
    assert "als.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["als.hip"]
    assert not any("fast" in f for f in build.EXTRA_FLAGS["als.hip"] + build.BASE_FLAGS)
    src = open(os.path.join(os.path.dirname(build.__file__), "als.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd" not in src and "fmaf" not in src
    assert lib.ncf_als_gram_workspace_bytes(0, 8) == 0 and lib.ncf_als_gram_workspace_bytes(257, 128) == 2 * 128 * 128 * 4
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd import baselines
    assert "ImplicitALS" in pkg._BASELINES and pkg.ImplicitALS is baselines.ImplicitALS
    assert pkg.ItemKNN.build_csr is baselines.build_csr and pkg.ItemKNN.build_transpose is baselines.build_transpose


P = 16                                           # a non-null, 16-byte aligned stand-in: every refusal comes before any launch
INF, NAN = float("inf"), float("nan")


def test_gram_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()

    def call(T=P, rows=10, ld=8, F=8, G=P, ws=P, nbytes=1 << 20):
        return lib.ncf_als_gram(T, rows, ld, F, G, ws, nbytes, None)

    for bad in (dict(rows=-1), dict(F=0), dict(F=-3), dict(F=129), dict(ld=7), dict(T=None), dict(G=None), dict(ws=None), dict(nbytes=255),
                dict(T=P + 2), dict(G=P + 1), dict(ws=P + 3), dict(rows=0, G=None), dict(rows=0, F=200), dict(rows=257, nbytes=2 * 8 * 8 * 4 - 1)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_als_gram" in lib.ncf_last_error(), bad


def test_solve_rows_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()

    def call(rowptr=P, col=P, val=P, nnz=10, R=3, rows=P, B=2, T=P, n_t=5, ldt=8, F=8, G=P, alpha=4.0, reg=0.1, out=P, ldo=8, by_row=0,
             seg_base=None, seg_row=None, n_slots=0, scratch=None, flag=P):
        return lib.ncf_als_solve_rows(rowptr, col, val, nnz, R, rows, B, T, n_t, ldt, F, G, alpha, reg, out, ldo, by_row, seg_base, seg_row,
                                      n_slots, scratch, flag, None)

    assert call(B=0) == native.NCF_OK
    assert call(B=0, rowptr=None, col=None, val=None, rows=None, T=None, G=None, out=None, flag=None) == native.NCF_OK
    for bad in (dict(nnz=-1), dict(R=-1), dict(B=-1), dict(n_t=-1), dict(n_slots=-1), dict(F=0), dict(F=129), dict(ldt=7), dict(ldo=7),
                dict(reg=0.0), dict(reg=-0.1), dict(reg=INF), dict(reg=NAN), dict(alpha=-1.0), dict(alpha=INF), dict(alpha=NAN), dict(by_row=2),
                dict(by_row=-1), dict(rowptr=None), dict(rows=None), dict(G=None), dict(out=None), dict(col=None), dict(val=None), dict(T=None),
                dict(n_slots=3), dict(n_slots=3, seg_base=P, seg_row=P), dict(n_slots=3, seg_base=P, scratch=P), dict(val=P + 2), dict(T=P + 1),
                dict(G=P + 3), dict(out=P + 2), dict(flag=P + 2), dict(col=P + 2), dict(rowptr=P + 4), dict(rows=P + 4),
                dict(n_slots=3, seg_base=P + 4, seg_row=P, scratch=P), dict(n_slots=3, seg_base=P, seg_row=P + 4, scratch=P),
                dict(n_slots=3, seg_base=P, seg_row=P, scratch=P + 2), dict(B=0, F=0), dict(B=0, reg=NAN), dict(B=0, alpha=-2.0), dict(B=0, ldt=3)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_als_solve_rows" in lib.ncf_last_error(), bad


def _host_case(F=8):
    rowptr, col, val = (torch.from_numpy(a.copy()) for a in A.base_case())
    T = torch.from_numpy(A.table(A.I, F, 100 + F).copy())
    G = torch.from_numpy(A.gram_ref(T.numpy(), F))
    return dict(rowptr=rowptr, col=col, val=val, rows=torch.arange(A.U), T=T, G=G, alpha=A.ALPHA, reg=A.REG)


def test_binding_refuses_mistyped_and_strided_tensors_before_the_device():
    from deeprecommendation_amd import native
    _lib()
    good = _host_case()
    T, G = good["T"], good["G"]
    for key, bad in (("rowptr", good["rowptr"].to(torch.int32)), ("rowptr", good["rowptr"][:0]), ("col", good["col"].long()),
                     ("val", good["val"].double()), ("val", good["val"][:-1]), ("rows", good["rows"].to(torch.int32)), ("rows", good["rows"][None]),
                     ("T", T.double()), ("T", T.t()), ("T", T[:, :7]), ("T", T[0]), ("G", G.double()), ("G", G[:, :7]), ("G", G.t()[::2]),
                     ("G", torch.zeros(129, 129)), ("alpha", -1.0), ("alpha", NAN), ("alpha", "4"), ("reg", 0.0), ("reg", -1.0), ("reg", INF),
                     ("reg", None), ("out_by_row", 1), ("out", torch.zeros(A.U, 7)), ("out", torch.zeros(A.U + 1, 8)),
                     ("out", torch.zeros(A.U, 8, dtype=torch.float64)), ("out", torch.zeros(8, A.U).t()), ("flag", torch.zeros(1)),
                     ("flag", torch.zeros(2, dtype=torch.int32)), ("block_bytes", 0), ("block_bytes", 1.5)):
        with pytest.raises(ValueError):
            native.als_solve_rows(**dict(good, **{key: bad}))
    with pytest.raises(ValueError):
        native.als_solve_rows(**dict(good, out_by_row=True))           # writes into the caller's table: out is required
    with pytest.raises(RuntimeError, match="GPU"):                     # well-formed host tensors: only now the device is asked for
        native.als_solve_rows(**good)
    with pytest.raises(RuntimeError, match="GPU"):
        native.als_solve_rows(**dict(good, out=torch.zeros(A.U, 9), out_by_row=True))
    for kw in (dict(T=T.double()), dict(T=T.t()), dict(T=T, F=9), dict(T=T, F=0), dict(T=T, F=2.0), dict(T=T, out=torch.zeros(8, 7)),
               dict(T=T, out=torch.zeros(8, 8, dtype=torch.float64)), dict(T=torch.zeros(4, 129))):
        with pytest.raises(ValueError):
            native.als_gram(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        native.als_gram(T)
    with pytest.raises(RuntimeError, match="GPU"):
        native.als_gram(T, 3)
    for kw in (dict(rowptr=good["rowptr"].float()), dict(rows=good["rows"].float()), dict(F=0), dict(F=129), dict(block_bytes=0)):
        with pytest.raises(ValueError):
            native.als_plan(**dict(dict(rowptr=good["rowptr"], rows=good["rows"], F=8), **kw))


def test_plan_cuts_batches_that_fit_the_scratch_buffer():
    from deeprecommendation_amd import native
    rowptr = torch.from_numpy(A.long_case()[0].copy())
    rows = torch.tensor([0, 1, 0, 5, 0, 7, -1, 3])                     # the long row three times; 7 and -1 lie outside the CSR
    F = 4
    assert native.als_plan(rowptr, torch.tensor([1, 2, 3, 4, 5]), F) == [(0, 5, None, None, 0)]
    assert native.als_plan(rowptr, rows[:0], F) == []
    one = native.als_plan(rowptr, rows, F)
    assert len(one) == 1 and one[0][:2] == (0, 8) and one[0][4] == 9
    assert one[0][2].tolist() == [0, -1, 3, -1, 6, -1, -1, -1] and one[0][3].tolist() == [0, 0, 0, 2, 2, 2, 4, 4, 4]
    two = native.als_plan(rowptr, rows, F, block_bytes=7 * F * F * 4)  # two rows' segments at a time
    assert [(p[0], p[1], p[4]) for p in two] == [(0, 4, 6), (4, 8, 3)]
    assert two[0][2].tolist() == [0, -1, 3, -1] and two[1][2].tolist() == [0, -1, -1, -1] and two[1][3].tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="block_bytes"):
        native.als_plan(rowptr, rows, F, block_bytes=2 * F * F * 4)


def test_implicit_als_refuses_bad_arguments_before_the_device():
    import deeprecommendation_amd as pkg
    for bad in (dict(n_factors=0), dict(n_factors=129), dict(n_factors=8.0), dict(n_factors=True), dict(n_iters=-1), dict(n_iters=2.0),
                dict(reg=0.0), dict(reg=-1.0), dict(reg=NAN), dict(reg="0.1"), dict(alpha=-1.0), dict(alpha=INF), dict(alpha=None),
                dict(init_sd=-0.1), dict(init_sd=NAN), dict(reg=True)):
        with pytest.raises(ValueError):
            pkg.ImplicitALS(**bad)
    m = pkg.ImplicitALS(n_factors=8, n_iters=2, reg=0.1, alpha=4.0)
    assert (m.n_factors, m.n_iters, m.reg, m.alpha, m.init_sd) == (8, 2, 0.1, 4.0, 0.01)
    d = pkg.ImplicitALS()
    assert (d.n_factors, d.n_iters, d.reg, d.alpha, d.init_sd) == (64, 15, 0.01, 40.0, 0.01)
    u, i, r = torch.tensor([0, 1, 2]), torch.tensor([1, 0, 1]), torch.ones(3)
    for args in ((u.to(torch.int32), i, r, 3, 2), (u, i[:2], r, 3, 2), (u, i, r.double(), 3, 2), (u, i, torch.ones(4), 3, 2), (u[:0], i[:0], r[:0], 3, 2),
                 (u, i, r, 0, 2), (u, i, r, 3, 0), (u[None], i, r, 3, 2), (u.numpy(), i, r, 3, 2)):
        with pytest.raises(ValueError):
            m.fit(*args)
    rowptr, col, val = (torch.from_numpy(a.copy()) for a in A.base_case())
    for args in ((rowptr.float(), col, val, A.I), (rowptr, col, val.double(), A.I), (rowptr, col[:-1], val, A.I), (rowptr, col, val, 0),
                 (rowptr[:1], col[:0], val[:0], A.I), (rowptr[None], col, val, A.I)):
        with pytest.raises(ValueError):
            m.fit_csr(*args)
    with pytest.raises(RuntimeError, match="GPU"):                     # well-formed host tensors: only now the device is asked for
        m.fit(u, i, r, 3, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        m.fit_csr(rowptr, col, val, A.I)
    ratings = (rowptr, col, val)
    for call in (m.check, m.as_mf, lambda: m.predict(u, i), lambda: m.fold_in_users(ratings, u), lambda: m.recommend_new_users(ratings, u, 3)):
        with pytest.raises(RuntimeError, match="not fitted"):
            call()


def test_hoisted_csr_builders_equal_numpys_stable_sorts():
    from deeprecommendation_amd import baselines
    for case, n_items in ((A.base_case(), A.I), (A.long_case(), A.LONG_I)):
        rowptr, col, val = case
        want = A.transpose_ref(rowptr, col, val, n_items)
        got = baselines.build_transpose(torch.from_numpy(rowptr.copy()), torch.from_numpy(col.copy()), torch.from_numpy(val.copy()), n_items)
        for g, w in zip(got, want):
            assert g.dtype == torch.from_numpy(np.array(w)).dtype and np.array_equal(g.numpy(), w)
        us, it = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), col.astype(np.int64)
        order = np.argsort(it, kind="stable")                          # numpy's stable sort on the column, spelt out
        assert np.array_equal(want[1], us[order].astype(np.int32)) and np.array_equal(want[2], val[order])
        perm = np.random.default_rng(0).permutation(len(us))
        got = baselines.build_csr(torch.from_numpy(us[perm]), torch.from_numpy(it[perm]), torch.from_numpy(val[perm]), len(rowptr) - 1, n_items)
        order = np.argsort(us[perm] * n_items + it[perm], kind="stable")
        for g, w in zip(got, (rowptr, it[perm][order].astype(np.int32), val[perm][order])):
            assert g.dtype == torch.from_numpy(np.array(w)).dtype and np.array_equal(g.numpy(), w)
        assert np.array_equal(got[1].numpy(), col) and np.array_equal(got[2].numpy(), val)
