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
    model, table, _ = native._FLAG_WORDS[kind]
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
    types = {kind: [exc for _, _, exc in table] for kind, (_, table, _) in native._FLAG_WORDS.items()}
    assert types == {"kmf": [IndexError] * 3, "knn": [ValueError], "als": [IndexError, IndexError, ValueError, ValueError, ValueError],
                     "ease": [ValueError] * 2, "unseen": [IndexError, ValueError], "oob": [IndexError], "pair_rows": [OverflowError],
                     "rank_overflow": [OverflowError]}
    assert [bit for bit, _, _ in native._FLAG_WORDS["als"][1]] == [native.ALS_FLAG_COL, native.ALS_FLAG_PTR, native.ALS_FLAG_ORDER,
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


# kind -> (its public check, its public accessor, whether the check takes flag=)
WORD_CHECKS = {"oob": (native.check_oob, native._oob_flag, False), "pair_rows": (native.check_pair_rows, native._pair_rows_flag, False),
               "rank_overflow": (native.check_rank_overflow, native._rank_overflow_flag, False),
               "kmf": (native.check_kmf, native.kmf_flag, True), "knn": (native.check_knn, native.knn_flag, True),
               "als": (native.check_als, native.als_flag, True), "ease": (native.check_ease, native.ease_flag, True),
               "unseen": (native.check_unseen, native.unseen_flag, True)}
# (kind, word, exception, message) as the checks raised them before they shared one table: every single bit, every pair of bits of
# a word with several meanings (an IndexError bit beside a ValueError bit raises IndexError), and all of them
RECORDED = [
    ("oob", 1, IndexError, "index out of range in an embedding gather"),
    ("oob", 7, IndexError, "index out of range in an embedding gather"),
    ("oob", -1, IndexError, "index out of range in an embedding gather"),
    ("pair_rows", 1, OverflowError, "a pair's rated entries did not fit the capacity pair_rows was given (max_row_len too small)"),
    ("pair_rows", 3, OverflowError, "a pair's rated entries did not fit the capacity pair_rows was given (max_row_len too small)"),
    ("rank_overflow", 1, OverflowError, "a row has more targets than the max_targets the rank call was given"),
    ("rank_overflow", 5, OverflowError, "a row has more targets than the max_targets the rank call was given"),
    ("kmf", 1, IndexError, "KernelMF: an id outside its table (flag 1)"),
    ("kmf", 2, IndexError, "KernelMF: a sample filed in the wrong block (flag 2)"),
    ("kmf", 4, IndexError, "KernelMF: a block / row pointer outside the samples (flag 4)"),
    ("kmf", 3, IndexError, "KernelMF: an id outside its table, a sample filed in the wrong block (flag 3)"),
    ("kmf", 5, IndexError, "KernelMF: an id outside its table, a block / row pointer outside the samples (flag 5)"),
    ("kmf", 6, IndexError, "KernelMF: a sample filed in the wrong block, a block / row pointer outside the samples (flag 6)"),
    ("kmf", 7, IndexError, "KernelMF: an id outside its table, a sample filed in the wrong block, a block / row pointer outside the samples (flag 7)"),
    ("knn", 1, ValueError, "ItemKNN: a row of the ratings CSR does not hold strictly ascending columns"),
    ("knn", 6, ValueError, "ItemKNN: a row of the ratings CSR does not hold strictly ascending columns"),
    ("knn", 2147483647, ValueError, "ItemKNN: a row of the ratings CSR does not hold strictly ascending columns"),
    ("knn", -1, ValueError, "ItemKNN: a row of the ratings CSR does not hold strictly ascending columns"),
    ("als", 1, IndexError, "ImplicitALS: a column outside the fixed table (flag 1)"),
    ("als", 2, IndexError, "ImplicitALS: a row or a row pointer outside the ratings (flag 2)"),
    ("als", 4, ValueError, "ImplicitALS: a row whose columns do not strictly ascend (flag 4)"),
    ("als", 8, ValueError, "ImplicitALS: a value that is negative or not finite (flag 8)"),
    ("als", 16, ValueError, "ImplicitALS: a pivot that is not positive and finite (flag 16)"),
    ("als", 3, IndexError, "ImplicitALS: a column outside the fixed table, a row or a row pointer outside the ratings (flag 3)"),
    ("als", 5, IndexError, "ImplicitALS: a column outside the fixed table, a row whose columns do not strictly ascend (flag 5)"),
    ("als", 9, IndexError, "ImplicitALS: a column outside the fixed table, a value that is negative or not finite (flag 9)"),
    ("als", 17, IndexError, "ImplicitALS: a column outside the fixed table, a pivot that is not positive and finite (flag 17)"),
    ("als", 6, IndexError, "ImplicitALS: a row or a row pointer outside the ratings, a row whose columns do not strictly ascend (flag 6)"),
    ("als", 10, IndexError, "ImplicitALS: a row or a row pointer outside the ratings, a value that is negative or not finite (flag 10)"),
    ("als", 18, IndexError, "ImplicitALS: a row or a row pointer outside the ratings, a pivot that is not positive and finite (flag 18)"),
    ("als", 12, ValueError, "ImplicitALS: a row whose columns do not strictly ascend, a value that is negative or not finite (flag 12)"),
    ("als", 20, ValueError, "ImplicitALS: a row whose columns do not strictly ascend, a pivot that is not positive and finite (flag 20)"),
    ("als", 24, ValueError, "ImplicitALS: a value that is negative or not finite, a pivot that is not positive and finite (flag 24)"),
    ("als", 31, IndexError, "ImplicitALS: a column outside the fixed table, a row or a row pointer outside the ratings, a row whose columns do not "
                            "strictly ascend, a value that is negative or not finite, a pivot that is not positive and finite (flag 31)"),
    ("ease", 1, ValueError, "EASE: a row of the ratings CSR does not hold strictly ascending columns (flag 1)"),
    ("ease", 2, ValueError, "EASE: a pivot of the inversion that is not positive and finite (flag 2)"),
    ("ease", 3, ValueError, "EASE: a row of the ratings CSR does not hold strictly ascending columns, a pivot of the inversion that is not positive "
                            "and finite (flag 3)"),
    ("unseen", 1, IndexError, "sample_unseen: a pick outside the users (flag 1)"),
    ("unseen", 256, ValueError, "sample_unseen: a user has fewer unseen items than the draws asked for (flag 256)"),
    ("unseen", 257, IndexError, "sample_unseen: a pick outside the users, a user has fewer unseen items than the draws asked for (flag 257)"),
]


def test_the_recorded_rows_cover_every_kind_every_bit_and_a_mixed_pair():
    assert {kind for kind, *_ in RECORDED} == set(WORD_CHECKS) == set(native._FLAG_WORDS)
    for kind, (_, rows, _) in native._FLAG_WORDS.items():
        words = {word for k, word, _, _ in RECORDED if k == kind}
        assert all((1 if bit == ~0 else bit) in words for bit, _, _ in rows), kind
        if len(rows) > 1:
            assert any(bin(w).count("1") == 2 for w in words), kind
    mixed = [("als", native.ALS_FLAG_PTR | native.ALS_FLAG_ORDER, IndexError), ("unseen", native.UNSEEN_FLAG_PICK | native.UNSEEN_FLAG_FEW, IndexError)]
    assert all(m in [r[:3] for r in RECORDED] for m in mixed)


@pytest.mark.parametrize("kind,word,exc,message", RECORDED, ids=[f"{r[0]}-{r[1]}" for r in RECORDED])
def test_every_flag_word_raises_what_it_raised_before_the_checks_shared_a_table(kind, word, exc, message):
    check, accessor, takes_flag = WORD_CHECKS[kind]
    device_word = accessor(CPU)
    assert device_word is accessor(CPU) and device_word.dtype == torch.int32 and device_word.numel() == 1
    try:
        check(CPU)                                                         # a zero word raises nothing
        device_word.fill_(word)
        with pytest.raises(exc) as e:
            check(CPU)
        assert type(e.value) is exc and str(e.value) == message
        assert int(device_word) == 0
        check(CPU)
        if takes_flag:                                                     # another word: the same message, the device's word untouched
            other = torch.full((1,), word, dtype=torch.int32)
            with pytest.raises(exc) as e:
                check(CPU, flag=other)
            assert type(e.value) is exc and str(e.value) == message
            assert int(other) == 0 and int(device_word) == 0
            check(CPU, flag=other)
            device_word.fill_(word)                                        # and with the override the device's word is not read
            check(CPU, flag=other)
            assert int(device_word) == word
    finally:
        device_word.zero_()


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
