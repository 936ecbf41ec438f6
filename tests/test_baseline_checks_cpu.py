"""CPU: the argument-check vocabulary of native.py's "who: ..." wrappers and the fit front end the three baselines share
(baselines._Baseline).  Each helper takes one good value and refuses each bad one with its exception type and the ``who:`` prefix; a
sticky flag word raises the type its table lists, names every set bit and is zero afterwards; and KernelMF, ItemKNN and ImplicitALS
refuse the same malformed samples with the same type, through fit and through fit_dataset, before any of them asks for the device."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deeprecommendation_amd import baselines, native

WHO = "some_call"
CPU = torch.device("cpu")


def _refused(exc, fn, *args, **kwargs):
    with pytest.raises(exc) as e:
        fn(WHO, *args, **kwargs)
    assert type(e.value) is exc and str(e.value).startswith(WHO + ": "), str(e.value)
    return str(e.value)


# ------------------------------------------------------------------ scalars
def test_integer_check_takes_both_ends_and_numpy_integers_and_refuses_bools_and_floats():
    assert native._int_in(WHO, 1, "k", 1, 8) == 1 and native._int_in(WHO, 8, "k", 1, 8) == 8
    got = native._int_in(WHO, np.int64(5), "k", 1, 8)
    assert got == 5 and type(got) is int
    for bad in (0, 9, True, False, 2.0, np.float32(2.0), "2", None):
        message = _refused(ValueError, native._int_in, bad, "k", 1, 8)
        assert "k = " in message and "1 .. 8" in message


def test_float_check_takes_its_lower_bound_and_refuses_nan_inf_and_bools():
    assert native._finite(WHO, 0.0, "reg", 0.0) == 0.0 and native._finite(WHO, -3, "fill") == -3.0
    got = native._finite(WHO, np.float32(0.5), "reg", 0.0)
    assert got == 0.5 and type(got) is float
    for bad in (math.nan, math.inf, -math.inf, True, "0.5", None):
        assert "reg = " in _refused(ValueError, native._finite, bad, "reg")
    assert ">= 0.0" in _refused(ValueError, native._finite, -1e-9, "reg", 0.0)


# ------------------------------------------------------------------ tensors
def test_vector_checks_refuse_dtype_rank_stride_and_length():
    v = torch.zeros(4, dtype=torch.int32)
    native._vec1d(WHO, v, "col", torch.int32)
    native._vec1d(WHO, v, "col", torch.int32, 4)
    for bad in (v.long(), v[None], torch.zeros(8, dtype=torch.int32)[::2], [0, 1, 2, 3]):
        assert "col" in _refused(ValueError, native._vec1d, bad, "col", torch.int32)
    assert "expected 5" in _refused(ValueError, native._vec1d, v, "col", torch.int32, 5)
    native._out1d(WHO, None, "sse", torch.float64, 6)
    native._out1d(WHO, torch.zeros(2, 3, dtype=torch.float64), "sse", torch.float64, 6)
    for bad in (torch.zeros(6), torch.zeros(5, dtype=torch.float64), torch.zeros(12, dtype=torch.float64)[::2]):
        assert "sse" in _refused(ValueError, native._out1d, bad, "sse", torch.float64, 6)


def test_csr_check_returns_rows_and_entries_and_refuses_each_array():
    ptr, idx, val = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1], dtype=torch.int32), torch.ones(3)
    names = ("rowptr", "col", "val")
    assert native._csr(WHO, ptr, idx, val, names) == (2, 3) and native._csr(WHO, ptr, idx, val, names, 2) == (2, 3)
    for bad, named in (((ptr.to(torch.int32), idx, val), "rowptr"), ((ptr[:0], idx, val), "rowptr"), ((ptr, idx.long(), val), "col"),
                       ((ptr, idx, val.double()), "val"), ((ptr, idx, val[:2]), "val")):
        assert named in _refused(ValueError, native._csr, *bad, names)
    assert "rowptr" in _refused(ValueError, native._csr, ptr, idx, val, names, 3)


def test_table_check_refuses_dtype_rank_inner_stride_and_too_few_columns():
    native._table_f32(WHO, torch.zeros(5, 8), "T")
    native._table_f32(WHO, torch.zeros(5, 16)[:, :8], "T", 8)             # a column slice: the row stride is free
    native._table_f32(WHO, torch.zeros(5, 4)[:, ::4], "T")                # one column wide: its inner stride is never used
    native._table_f32(WHO, torch.zeros(5, 0), "T", 0)
    for bad in (torch.zeros(5, 8, dtype=torch.float64), torch.zeros(40), torch.zeros(5, 16)[:, ::2], [[0.0]]):
        assert "T must be a 2-D float32 tensor with unit inner stride" in _refused(ValueError, native._table_f32, bad, "T")
    message = _refused(ValueError, native._table_f32, torch.zeros(5, 8), "T", 9)
    assert "T" in message and "8" in message and "9" in message


def test_out_check_refuses_shape_and_dtype_and_a_row_stride_only_where_the_caller_says():
    like, swept = torch.zeros(3), ((torch.zeros(3), "rowptr"),)
    accepted = (dict(out=torch.zeros(4, 6)), dict(out=torch.zeros(4, 12)[:, :6]), dict(out=torch.zeros(4, 6), contiguous=True),
                dict(out=torch.zeros(4, 9), wider=True), dict(out=torch.zeros(4, 3)[:, ::3], rows=4, cols=1), dict(out=None))
    for kw in accepted:                                                    # well-formed: the device sweep is what stops a host tensor
        with pytest.raises(RuntimeError, match="rowptr must live on the GPU"):
            native._out2d(WHO, **dict(dict(rows=4, cols=6, like=like, swept=swept), **kw))
    with pytest.raises(RuntimeError, match="out must live on the GPU"):
        native._out2d(WHO, torch.zeros(4, 6), 4, 6, like, ())
    for kw in (dict(out=torch.zeros(4, 5)), dict(out=torch.zeros(5, 6)), dict(out=torch.zeros(24)), dict(out=torch.zeros(4, 6, dtype=torch.float64)),
               dict(out=torch.zeros(4, 12)[:, ::2]), dict(out=torch.zeros(4, 12)[:, :6], contiguous=True), dict(out=torch.zeros(4, 7)),
               dict(out=torch.zeros(4, 5), wider=True), dict(out=[[0.0] * 6] * 4)):
        message = _refused(ValueError, native._out2d, **dict(dict(rows=4, cols=6, like=like, swept=swept), **kw))
        assert "out must be a (4, " in message and "6) float32 tensor" in message
    assert ">= 6" in _refused(ValueError, native._out2d, torch.zeros(4, 5), 4, 6, like, swept, wider=True)


def test_device_sweep_names_the_first_host_tensor_and_skips_none():
    native._dev_all()
    native._dev_all((None, "out"), (None, "flag"))
    with pytest.raises(RuntimeError, match="col must live on the GPU"):
        native._dev_all((None, "out"), (torch.zeros(1), "col"), (torch.zeros(1), "val"))


# ------------------------------------------------------------------ flag words
FLAG_CHECKS = {"kmf": (native.check_kmf, native.kmf_flag), "knn": (native.check_knn, native.knn_flag), "als": (native.check_als, native.als_flag)}


@pytest.mark.parametrize("kind", sorted(FLAG_CHECKS))
def test_flag_check_raises_the_listed_type_names_every_set_bit_and_clears_the_word(kind):
    check, _ = FLAG_CHECKS[kind]
    model, table = native._FLAG_BITS[kind]
    flag = torch.zeros(1, dtype=torch.int32)
    check(CPU, flag=flag)                                                  # a zero word raises nothing
    words = [(bit & 0x7fffffff, [text], exc) for bit, text, exc in table]
    words += [(a | b, [ta, tb], IndexError if IndexError in (ea, eb) else ea)
              for i, (a, ta, ea) in enumerate(table) for b, tb, eb in table[i + 1:]]
    for word, texts, exc in words:
        flag.fill_(word)
        with pytest.raises(exc) as e:
            check(CPU, flag=flag)
        assert type(e.value) is exc and str(e.value).startswith(model + ": ")
        assert all(t in str(e.value) for t in texts) and int(flag) == 0
        if len(table) > 1:
            assert str(e.value).endswith(f"(flag {word})") and sum(t in str(e.value) for _, t, _ in table) == len(texts)
        check(CPU, flag=flag)


def test_flag_tables_list_the_documented_types():
    types = {kind: [exc for _, _, exc in table] for kind, (_, table) in native._FLAG_BITS.items()}
    assert types == {"kmf": [IndexError] * 3, "knn": [ValueError], "als": [IndexError, IndexError, ValueError, ValueError, ValueError]}
    assert [bit for bit, _, _ in native._FLAG_BITS["als"][1]] == [native.ALS_FLAG_COL, native.ALS_FLAG_PTR, native.ALS_FLAG_ORDER,
                                                                  native.ALS_FLAG_VAL, native.ALS_FLAG_PIVOT]
    flag = torch.full((1,), native.ALS_FLAG_ORDER | native.ALS_FLAG_PTR, dtype=torch.int32)
    with pytest.raises(IndexError, match="a row or a row pointer outside the ratings, a row whose columns do not strictly ascend"):
        native.check_als(CPU, flag=flag)


def test_flag_check_without_an_override_reads_the_device_word():
    for kind, (check, word) in FLAG_CHECKS.items():
        try:
            word(CPU).fill_(1)
            with pytest.raises((IndexError, ValueError)):
                check(CPU)
            assert int(word(CPU)) == 0
        finally:
            word(CPU).zero_()


# ------------------------------------------------------------------ the fit front end
MODELS = [lambda: baselines.KernelMF(n_factors=4, n_epochs=2, n_blocks=2), lambda: baselines.ItemKNN(k=3),
          lambda: baselines.ImplicitALS(n_factors=4, n_iters=2)]
U, I, R = torch.tensor([0, 1, 2]), torch.tensor([1, 0, 1]), torch.ones(3)
MALFORMED = [(U.to(torch.int32), I, R, 3, 2), (U, I.to(torch.int32), R, 3, 2), (U, I[:2], R, 3, 2), (U, I, R.double(), 3, 2), (U, I, torch.ones(4), 3, 2),
             (U[None], I, R, 3, 2), (U, I, R[None], 3, 2), (U.numpy(), I, R, 3, 2), (U[:0], I[:0], R[:0], 3, 2), (U, I, R, 0, 2), (U, I, R, 3, 0)]


def _dataset(u, i, r, num_users, num_items, on_chunk=None):
    """What fit_dataset reads of a FixedPointwiseDataset over an index provider."""
    cp = SimpleNamespace(get_num_users=lambda: num_users, get_num_items=lambda: num_items)
    return SimpleNamespace(resident_inputs=lambda dev: SimpleNamespace(tensors=(u, i), targets=r, on_chunk=on_chunk), content_provider=cp)


@pytest.mark.parametrize("make", MODELS, ids=["KernelMF", "ItemKNN", "ImplicitALS"])
def test_every_baseline_refuses_the_same_samples_the_same_way(make):
    m, name = make(), type(make()).__name__
    for args in MALFORMED:
        with pytest.raises(ValueError) as e:
            m.fit(*args)
        assert str(e.value).startswith(name + ": "), str(e.value)
        if torch.is_tensor(args[0]):
            with pytest.raises(ValueError, match="^" + name + ": "):
                m.fit_dataset(_dataset(*args), device="cpu")
    for fit in (lambda: m.fit(U, I, R, 3, 2), lambda: m.fit_dataset(_dataset(U, I, R, 3, 2), device="cpu"),
                lambda: m.fit_dataset(_dataset(I, U, R, 3, 2, on_chunk=lambda a, b: (b, a)), device="cpu")):
        with pytest.raises(RuntimeError, match=name + r"\.fit runs on the GPU: the samples must live on one GPU .*no CPU path"):
            fit()
    with pytest.raises(ValueError, match=name + r"\.fit_dataset: the dataset's provider hands out dense rows"):
        m.fit_dataset(SimpleNamespace(resident_inputs=lambda dev: None), device="cpu")
    assert type(m).fit_dataset is baselines._Baseline.fit_dataset


@pytest.mark.parametrize("make", MODELS[1:], ids=["ItemKNN", "ImplicitALS"])
def test_both_csr_fits_refuse_the_same_csr_the_same_way(make):
    m, name = make(), type(make()).__name__
    rowptr, col, val = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1], dtype=torch.int32), torch.ones(3)
    for args in ((rowptr.float(), col, val, 2), (rowptr, col, val.double(), 2), (rowptr, col[:2], val, 2), (rowptr[None], col, val, 2),
                 (rowptr, col, val, 0), (rowptr[:1], col[:0], val[:0], 2), (torch.tensor([0, 0, 0]), col[:0], val[:0], 2)):
        with pytest.raises(ValueError, match="^" + name):
            m.fit_csr(*args)
    with pytest.raises(RuntimeError, match=name + r"\.fit_csr runs on the GPU: the CSR must live on one GPU .*no CPU path"):
        m.fit_csr(rowptr, col, val, 2)


def test_constructor_scalars_go_through_the_shared_checks():
    for bad in (dict(n_factors=True), dict(n_epochs=True), dict(n_blocks=True), dict(n_factors=2.0), dict(lr=True), dict(reg=math.nan)):
        with pytest.raises(ValueError, match="^KernelMF: "):
            baselines.KernelMF(**bad)
    for bad in (dict(k=True), dict(min_support=True), dict(shrink=True), dict(shrink=-1.0), dict(fill=math.inf)):
        with pytest.raises(ValueError, match="^ItemKNN: "):
            baselines.ItemKNN(**bad)
    for bad in (dict(n_factors=True), dict(n_iters=True), dict(reg=True), dict(reg=0.0), dict(alpha=-1.0)):
        with pytest.raises(ValueError, match="^ImplicitALS: "):
            baselines.ImplicitALS(**bad)
    m = baselines.KernelMF(n_factors=np.int64(8), n_epochs=np.int32(3), n_blocks=np.int64(2), lr=np.float32(0.5))
    assert (m.n_factors, m.n_epochs, m.n_blocks, m.lr) == (8, 3, 2, 0.5) and type(m.n_factors) is int and type(m.lr) is float
