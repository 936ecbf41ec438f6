"""CPU tests of the ItemKNN baseline: the fp32 restatement of tests/knn_ref.py tracks its float64 twin, which is the brute-force dense
computation; planted clusters come back exactly; full-table unweighted scores are S @ x_u; the transpose builder is numpy's stable
argsort; the four entry points are declared, exported, bound and built with THE CONTRACT in the header; their refusals, the
binding's and ItemKNN's come before the device."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import knn_ref as K


def _lib():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load_library()


def test_fp32_restatement_tracks_its_float64_twin_and_the_dense_computation():
    rowptr, col, val = K.base_case()
    worst = 0.0
    for shrink, ms in K.SIM_PARAMS:
        S32, S64 = K.base_sim(shrink, ms), K.base_sim(shrink, ms, np.float64)
        dense = K.sim_dense64(rowptr, col, val, K.I, shrink, ms)
        dev, dd = np.abs(S32.astype(np.float64) - S64).max(), np.abs(S64 - dense).max()
        print(f"shrink={shrink} min_support={ms}: max |fp32 - float64 twin| = {dev:.3e}, |twin - dense| = {dd:.3e}, "
              f"{int((S64 > 0).sum())} positive similarities, max {S64.max():.3f}")
        assert dd <= 1e-13                                             # the twin IS the dense computation, up to float64 summation order
        assert (S64 > 0).sum() > 1000 and S64.max() <= 1.0 + 1e-12
        worst = max(worst, dev)
    print(f"worst {worst:.3e} = {worst * 2 ** 24:.2f} * 2^-24; recorded {K.F32_VS_F64_MEASURED:.3e}")
    assert worst <= 8 * K.F32_VS_F64_MEASURED


def test_base_case_holds_what_the_gpu_tests_rely_on():
    rowptr, col, val = K.base_case()
    lens = np.diff(rowptr)
    assert lens[K.LONG_USER] == 130 and lens[K.EMPTY_USER] == 0 and lens[K.ONE_USER] == 1
    assert not (col == K.UNRATED_ITEM).any() and (col == K.COMMON_ITEM).sum() == K.U - 1
    for u in range(K.U):
        assert (np.diff(col[rowptr[u]:rowptr[u + 1]]) > 0).all()
    dot, co, sq = K.base_gram()
    off = ~np.eye(K.I, dtype=bool)
    assert ((co == 1) & off).sum() > 100                               # pairs that min_support = 2 removes
    assert ((dot < 0) & (co > 0) & off).sum() > 100                    # negative similarities, which are no neighbours
    assert sq[K.UNRATED_ITEM] == 0 and K.base_table(7, 0.0, 1)[2][K.UNRATED_ITEM] == 0
    cnt = K.base_table(200, 0.0, 1)[2]
    assert cnt.max() < 149 and (K.base_table(7, 0.0, 1)[2] == 7).any() and (K.base_table(200, 10.0, 2)[2] < cnt).any()


def test_integer_case_ties_exactly():
    rowptr, col, val = K.integer_case()
    S = K.sim_ref(rowptr, col, val, 70, 0.0, 1)
    assert set(np.unique(val)) <= {-2.0, -1.0, 1.0, 2.0}
    ties = 0
    for a, b in [(2 * k, 2 * k + 1) for k in range(10)] + [(60, 61), (60, 63), (64, 67)]:
        rest = np.setdiff1d(np.arange(70), [a, b])
        assert np.array_equal(S[rest, a], S[rest, b])
        ties += int((S[rest, a] > 0).sum())
    assert ties > 100
    pos, sim, cnt = K.table_ref(S, 7)
    for i in range(70):                                                # equal similarities sit in ascending position order
        for t in range(cnt[i] - 1):
            assert sim[i, t] > sim[i, t + 1] or (sim[i, t] == sim[i, t + 1] and pos[i, t] < pos[i, t + 1])


def test_planted_clusters_come_back_exactly():
    (rowptr, col, val), cluster = K.cluster_case()
    S = K.sim_ref(rowptr, col, val, len(cluster), 0.0, 1)
    pos, sim, cnt = K.table_ref(S, 50)
    for i in range(len(cluster)):
        assert (cluster[pos[i, :cnt[i]]] == cluster[i]).all()
        if (cluster == cluster[i]).sum() == 1:
            assert cnt[i] == 0
    assert cnt.max() >= 9


def test_full_table_unweighted_scores_are_the_matrix_product():
    rowptr, col, val = K.score_case()
    S64 = K.base_sim(0.0, 1, np.float64)
    X = np.zeros((len(rowptr) - 1, K.I))
    X[np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), col] = val.astype(np.float64)
    want = X @ S64.T                                                   # score(u, i) = sum_j s_ij x_uj
    got32 = K.base_scores(200, 0.0, 1, False, 0.0)
    twin = K.scores_ref(rowptr, col, val, np.arange(len(rowptr) - 1), K.table_ref(S64, 200), False, 0.0, np.float64)
    dev = np.abs(got32.astype(np.float64) - twin).max()
    print(f"max |fp32 scores - float64 twin| = {dev:.3e} (max |score| {np.abs(twin).max():.3f}); recorded {K.SCORE_F32_VS_F64_MEASURED:.3e}")
    assert np.abs(twin - want).max() <= 1e-12
    assert dev <= 8 * K.SCORE_F32_VS_F64_MEASURED
    assert np.abs(got32.astype(np.float64) - want).max() <= 8 * K.SCORE_F32_VS_F64_MEASURED + 1e-12


def test_weighted_scores_fill_where_no_neighbour_was_rated():
    got = K.base_scores(7, 10.0, 2, True, -3.5)
    assert (got[1] == -3.5).all() and (got[3] == -3.5).all() and (got[:, K.UNRATED_ITEM] == -3.5).all()
    assert (got[0] != -3.5).sum() > 100
    un = K.base_scores(7, 10.0, 2, False, -3.5)
    assert not un[1].any() and not un[3].any()


def test_transpose_builder_equals_numpys_stable_argsort():
    import deeprecommendation_amd as pkg
    for case, n_items in ((K.base_case(), K.I), (K.integer_case(), 70), (K.score_case(), K.I)):
        rowptr, col, val = case
        want = K.transpose_ref(rowptr, col, val, n_items)
        got = pkg.ItemKNN.build_transpose(torch.from_numpy(rowptr.copy()), torch.from_numpy(col.copy()), torch.from_numpy(val.copy()), n_items)
        for g, w in zip(got, want):
            assert g.dtype == torch.from_numpy(w).dtype and np.array_equal(g.numpy(), w)
        for i in range(n_items):                                       # users ascend inside a column
            assert (np.diff(want[1][want[0][i]:want[0][i + 1]]) > 0).all()
    us, it = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), col.astype(np.int64)
    perm = np.random.default_rng(0).permutation(len(us))
    got = pkg.ItemKNN.build_csr(torch.from_numpy(us[perm]), torch.from_numpy(it[perm]), torch.from_numpy(val[perm]), len(rowptr) - 1, K.I)
    for g, w in zip(got, (rowptr, col, val)):
        assert g.dtype == torch.from_numpy(w).dtype and np.array_equal(g.numpy(), w)


def test_entry_points_are_declared_exported_bound_and_built():
    from deeprecommendation_amd import native
    from deeprecommendation_amd.csrc import build
    hdr = open(os.path.join(ROOT, "include", "ncf_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("ncf_knn_item_sq", "ncf_knn_sim_rows", "ncf_knn_scores", "ncf_knn_predict"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    for line in ("part_l = +0.0f;  for e = l, l + 64, l + 128, ... in that order:  part_l = part_l + tval[e] * tval[e]",
                 "sq[i]  = balanced tree over lanes 0..63 in lane order: adjacent pairs first, then pairs of pairs, ... (6 levels)",
                 "for the users u of column i in ascending order, for every entry (j, v_uj) of row u:",
                 "dot[j] = dot[j] + v_ui * v_uj;   co[j] = co[j] + 1",
                 "n = sqrtf(sq[i]) * sqrtf(sq[j])",
                 "s_ij = 0.0f  if j == i, or co[j] < min_support, or n == 0",
                 "s_ij = (dot[j] / n) * ((float)co[j] / ((float)co[j] + shrink))  otherwise, and 0.0f unless that is > 0",
                 "ties to the lower j (ncf_topk_rows' order)",
                 "if row u holds j with value v:  num = num + s * v;   den = den + s",
                 "weighted_average = 1:  num / den if den > 0, else fill;      weighted_average = 0:  num",
                 "correctly rounded IEEE operations, hipcc's default for fp32"):
        assert line in hdr, line                                       # the contract is part of the ABI
    lib = _lib()
    for name, nargs in (("ncf_knn_item_sq", 7), ("ncf_knn_sim_rows", 21), ("ncf_knn_scores", 21), ("ncf_knn_predict", 18)):
        assert hasattr(lib, name) and len(native.SIGNATURES[name][1]) == nargs
    for name in ("knn_item_sq", "knn_sim_rows", "knn_scores", "knn_predict", "check_knn"):
        assert callable(getattr(native, name))
    assert "knn.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["knn.hip"]
    assert not any("fast" in f for f in build.EXTRA_FLAGS["knn.hip"] + build.BASE_FLAGS)
    src = open(os.path.join(os.path.dirname(build.__file__), "knn.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd" not in src
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd import baselines, recommend
    assert "ItemKNN" in pkg._BASELINES and pkg.ItemKNN is baselines.ItemKNN
    for name in ("item_knn_top_k", "item_knn_ranks"):
        assert name in pkg._RECOMMEND and getattr(pkg, name) is getattr(recommend, name)


A = 16                                           # a non-null, 16-byte aligned stand-in: every refusal comes before any launch
INF, NAN = float("inf"), float("nan")


def test_item_sq_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()

    def call(colptr=A, tval=A, nnz=10, I=4, sq=A, oob=A):
        return lib.ncf_knn_item_sq(colptr, tval, nnz, I, sq, oob, None)

    assert call(I=0) == native.NCF_OK and call(I=0, nnz=0, colptr=None, tval=None, sq=None, oob=None) == native.NCF_OK
    for bad in (dict(I=-1), dict(nnz=-1), dict(colptr=None), dict(sq=None), dict(tval=None), dict(I=0, nnz=-1)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_knn_item_sq" in lib.ncf_last_error(), bad


def test_sim_rows_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()

    def call(rowptr=A, col=A, val=A, nnz=10, U=3, colptr=A, row=A, tval=A, nnzT=10, I=100, sq=A, i0=0, i1=100, ms=1, shrink=0.0, tile=0,
             out=A, ldo=100, oob=A, order=A):
        return lib.ncf_knn_sim_rows(rowptr, col, val, nnz, U, colptr, row, tval, nnzT, I, sq, i0, i1, ms, shrink, tile, out, ldo, oob, order, None)

    assert call(i0=5, i1=5) == native.NCF_OK and call(I=0, i1=0, ldo=0) == native.NCF_OK
    assert call(i0=7, i1=7, rowptr=None, col=None, val=None, colptr=None, row=None, tval=None, sq=None, out=None, oob=None, order=None,
                nnz=0, nnzT=0) == native.NCF_OK
    for bad in (dict(U=-1), dict(I=-1), dict(nnz=-1), dict(nnzT=-1), dict(i0=-1), dict(i0=3, i1=2), dict(i1=101), dict(ms=0), dict(ms=-3),
                dict(shrink=-1.0), dict(shrink=INF), dict(shrink=NAN), dict(tile=-64), dict(tile=63), dict(tile=100), dict(tile=8256),
                dict(ldo=99), dict(rowptr=None), dict(colptr=None), dict(sq=None), dict(out=None), dict(col=None), dict(val=None),
                dict(row=None), dict(tval=None), dict(i0=5, i1=5, ms=0), dict(i0=5, i1=5, tile=65), dict(i0=5, i1=5, shrink=NAN)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_knn_sim_rows" in lib.ncf_last_error(), bad
    assert call(I=70000, i1=70000, ldo=70000) == native.NCF_EUNSUPPORTED and b"ncf_knn_sim_rows" in lib.ncf_last_error()
    assert call(i0=5, i1=5, tile=64) == native.NCF_OK and call(i0=5, i1=5, tile=8192) == native.NCF_OK


def test_scores_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()

    def call(rowptr=A, col=A, val=A, nnz=10, R=3, users=A, B=2, pos=A, sim=A, cnt=A, I=100, N=7, i0=0, i1=100, w=1, fill=0.0, cap=0, out=A,
             ldo=100, oob=A):
        return lib.ncf_knn_scores(rowptr, col, val, nnz, R, users, B, pos, sim, cnt, I, N, i0, i1, w, fill, cap, out, ldo, oob, None)

    assert call(B=0) == native.NCF_OK and call(i0=4, i1=4) == native.NCF_OK
    assert call(B=0, rowptr=None, col=None, val=None, users=None, pos=None, sim=None, cnt=None, out=None, oob=None) == native.NCF_OK
    for bad in (dict(R=-1), dict(B=-1), dict(nnz=-1), dict(I=-1), dict(N=0), dict(N=257), dict(N=-1), dict(i0=-1), dict(i0=3, i1=2),
                dict(i1=101), dict(w=2), dict(w=-1), dict(fill=INF), dict(fill=NAN), dict(cap=-1), dict(cap=8193), dict(ldo=99),
                dict(rowptr=None), dict(users=None), dict(pos=None), dict(sim=None), dict(cnt=None), dict(out=None), dict(col=None),
                dict(val=None), dict(B=0, N=0), dict(B=0, fill=NAN), dict(i0=4, i1=4, N=300)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_knn_scores" in lib.ncf_last_error(), bad
    assert call(B=65536) == native.NCF_EUNSUPPORTED and b"ncf_knn_scores" in lib.ncf_last_error()
    assert call(B=0, N=1) == native.NCF_OK and call(B=0, N=256, cap=8192) == native.NCF_OK


def test_predict_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()

    def call(rowptr=A, col=A, val=A, nnz=10, R=3, users=A, items=A, n=5, pos=A, sim=A, cnt=A, I=100, N=7, w=1, fill=0.0, out=A, oob=A):
        return lib.ncf_knn_predict(rowptr, col, val, nnz, R, users, items, n, pos, sim, cnt, I, N, w, fill, out, oob, None)

    assert call(n=0) == native.NCF_OK
    assert call(n=0, rowptr=None, col=None, val=None, users=None, items=None, pos=None, sim=None, cnt=None, out=None, oob=None) == native.NCF_OK
    for bad in (dict(R=-1), dict(n=-1), dict(nnz=-1), dict(I=-1), dict(N=0), dict(N=257), dict(w=2), dict(fill=-INF), dict(fill=NAN),
                dict(rowptr=None), dict(users=None), dict(items=None), dict(pos=None), dict(sim=None), dict(cnt=None), dict(out=None),
                dict(col=None), dict(val=None), dict(n=0, N=0), dict(n=0, fill=NAN)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_knn_predict" in lib.ncf_last_error(), bad


def _host_case():
    rowptr, col, val = (torch.from_numpy(a.copy()) for a in K.base_case())
    colptr, row, tval = (torch.from_numpy(a.copy()) for a in K.transpose_ref(*K.base_case(), K.I))
    pos, sim, cnt = (torch.from_numpy(a.copy()) for a in K.base_table(7, 0.0, 1))
    return dict(rowptr=rowptr, col=col, val=val), dict(colptr=colptr, row=row, tval=tval), dict(nb_pos=pos, nb_sim=sim, nb_cnt=cnt)


def test_binding_refuses_mistyped_and_strided_tensors_before_the_device():
    from deeprecommendation_amd import native
    _lib()
    csr, csc, tab = _host_case()
    sq = torch.zeros(K.I)
    good = dict(csr, **csc, sq=sq)
    for key, bad in (("rowptr", csr["rowptr"].to(torch.int32)), ("rowptr", csr["rowptr"][:0]), ("col", csr["col"].long()), ("val", csr["val"].double()),
                     ("val", csr["val"][:-1]), ("col", torch.zeros(2 * csr["col"].numel(), dtype=torch.int32)[::2]), ("colptr", csc["colptr"][None]),
                     ("row", csc["row"].long()), ("tval", csc["tval"][:-1]), ("sq", sq[:-1]), ("sq", sq.double()), ("item_range", (-1, 5)),
                     ("item_range", (5, 4)), ("item_range", (0, K.I + 1)), ("min_support", 0), ("min_support", 1.5), ("shrink", -0.5),
                     ("shrink", NAN), ("shrink", "1"), ("col_tile", 63), ("col_tile", -64), ("col_tile", 8256), ("out", torch.zeros(K.I, K.I + 1)),
                     ("out", torch.zeros(K.I, K.I, dtype=torch.float64)), ("flag", torch.zeros(1)), ("flag", torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            native.knn_sim_rows(**dict(good, **{key: bad}))
    with pytest.raises(RuntimeError, match="GPU"):        # well-formed host tensors: only now the device is asked for
        native.knn_sim_rows(**good)
    for kw in (dict(colptr=csc["colptr"].to(torch.int32), tval=csc["tval"]), dict(colptr=csc["colptr"], tval=csc["tval"].double()),
               dict(colptr=csc["colptr"][:0], tval=csc["tval"]), dict(colptr=csc["colptr"], tval=csc["tval"], out=torch.zeros(K.I + 1))):
        with pytest.raises(ValueError):
            native.knn_item_sq(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        native.knn_item_sq(csc["colptr"], csc["tval"])
    users = torch.tensor([0, 5, 6])
    good = dict(csr, users=users, **tab)
    for key, bad in (("users", users.to(torch.int32)), ("users", users[None]), ("nb_pos", tab["nb_pos"].long()), ("nb_pos", tab["nb_pos"].t()),
                     ("nb_sim", tab["nb_sim"][:, :6]), ("nb_sim", tab["nb_sim"].double()), ("nb_cnt", tab["nb_cnt"][:-1]), ("nb_cnt", tab["nb_cnt"].long()),
                     ("item_range", (3, 2)), ("fill", INF), ("fill", None), ("stage_cap", -1), ("stage_cap", 8193), ("stage_cap", 2.0),
                     ("out", torch.zeros(3, K.I + 1)), ("col", csr["col"].long())):
        with pytest.raises(ValueError):
            native.knn_scores(**dict(good, **{key: bad}))
    wide = torch.zeros((K.I, 257))
    with pytest.raises(ValueError):
        native.knn_scores(**dict(good, nb_pos=wide.to(torch.int32), nb_sim=wide))
    with pytest.raises(RuntimeError, match="GPU"):
        native.knn_scores(**good)
    good = dict(csr, users=users, items=torch.tensor([1, 2, 3]), **tab)
    for key, bad in (("items", torch.tensor([1, 2])), ("items", good["items"].to(torch.int32)), ("users", users.float()), ("fill", NAN),
                     ("nb_cnt", tab["nb_cnt"][:5]), ("rowptr", csr["rowptr"].float())):
        with pytest.raises(ValueError):
            native.knn_predict(**dict(good, **{key: bad}))
    with pytest.raises(RuntimeError, match="GPU"):
        native.knn_predict(**good)


def test_item_knn_refuses_bad_arguments_before_the_device():
    import deeprecommendation_amd as pkg
    for bad in (dict(k=0), dict(k=257), dict(k=2.0), dict(k=True), dict(shrink=-1.0), dict(shrink=NAN), dict(shrink="0"), dict(min_support=0),
                dict(min_support=1.0), dict(fill=INF), dict(fill=None), dict(weighted_average=1)):
        with pytest.raises(ValueError):
            pkg.ItemKNN(**bad)
    m = pkg.ItemKNN(k=7, shrink=10.0, min_support=2)
    u, i, r = torch.tensor([0, 1, 2]), torch.tensor([1, 0, 1]), torch.ones(3)
    for args in ((u.to(torch.int32), i, r, 3, 2), (u, i[:2], r, 3, 2), (u, i, r.double(), 3, 2), (u, i, torch.ones(4), 3, 2), (u[:0], i[:0], r[:0], 3, 2),
                 (u, i, r, 0, 2), (u, i, r, 3, 0), (u[None], i, r, 3, 2), (u.numpy(), i, r, 3, 2)):
        with pytest.raises(ValueError):
            m.fit(*args)
    csr, _, _ = _host_case()
    for args in ((csr["rowptr"].float(), csr["col"], csr["val"], K.I), (csr["rowptr"], csr["col"], csr["val"].double(), K.I),
                 (csr["rowptr"], csr["col"][:-1], csr["val"], K.I), (csr["rowptr"], csr["col"], csr["val"], 0),
                 (csr["rowptr"][:1], csr["col"][:0], csr["val"][:0], K.I), (csr["rowptr"][None], csr["col"], csr["val"], K.I)):
        with pytest.raises(ValueError):
            m.fit_csr(*args)
    with pytest.raises(RuntimeError, match="GPU"):        # well-formed host tensors: only now the device is asked for
        m.fit(u, i, r, 3, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        m.fit_csr(csr["rowptr"], csr["col"], csr["val"], K.I)
    ratings = (csr["rowptr"], csr["col"], csr["val"])
    for call in (m.check, lambda: m.neighbours, lambda: m.similar_items(u, 3), lambda: m.scores(ratings, u), lambda: m.predict(ratings, u, i),
                 lambda: pkg.item_knn_top_k(m, ratings, u, 3), lambda: pkg.item_knn_ranks(m, ratings, u, (torch.tensor([0, 1, 2, 3]), i.int()))):
        with pytest.raises(RuntimeError, match="not fitted"):
            call()
