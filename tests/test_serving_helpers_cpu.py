"""CPU: the helpers the ranking and serving front ends share — the CSR row-take (recommend._csr_take, ranking_eval._take_rows)
against a plain Python loop, and the sticky flag words of native.py (one tensor per (kind, device), each check_* raising its own
message, clearing its own word and nothing else)."""
import pytest
import torch

from deeprecommendation_amd import native, ranking_eval, recommend

ROWPTR = [0, 3, 3, 4, 9, 11]                   # row 1 is empty, row 4 is the last
COL = [5, 1, 7, 2, 9, 8, 6, 4, 3, 0, 10]


def _loop(rowptr, rows):
    new, entry = [0], []
    for r in rows:
        entry += list(range(rowptr[r], rowptr[r + 1]))
        new.append(len(entry))
    return new, entry


@pytest.mark.parametrize("rows", [[1], [2, 2], [4, 3, 1, 0], [4], [], [0, 1, 1, 3, 3, 4, 2]],
                         ids=["empty_row", "same_row_twice", "descending", "last_row", "no_rows", "mixed"])
def test_row_take_matches_a_python_loop(rows):
    rowptr, col = torch.tensor(ROWPTR, dtype=torch.int64), torch.tensor(COL, dtype=torch.int32)
    want_ptr, want_entry = _loop(ROWPTR, rows)
    new, cols, entry = ranking_eval._take_rows(rowptr, col, torch.tensor(rows, dtype=torch.int64))
    assert new.dtype == torch.int64 and cols.dtype == torch.int32
    assert new.tolist() == want_ptr and entry.tolist() == want_entry and cols.tolist() == [COL[e] for e in want_entry]
    # the spans given directly, as seen_items gives them (starts and counts from a search, not from a rowptr)
    start = torch.tensor([ROWPTR[r] for r in rows], dtype=torch.int64)
    count = torch.tensor([ROWPTR[r + 1] - ROWPTR[r] for r in rows], dtype=torch.int64)
    new2, entry2 = recommend._csr_take(start, count)
    assert new2.tolist() == want_ptr and entry2.tolist() == want_entry


def test_row_take_of_a_csr_without_entries():
    rowptr, col = torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    new, cols, entry = ranking_eval._take_rows(rowptr, col, torch.tensor([2, 0, 2]))
    assert new.tolist() == [0, 0, 0, 0] and cols.numel() == 0 and cols.dtype == torch.int32 and entry.numel() == 0


CPU = torch.device("cpu")
# getter, check, exception, message, the word that sets it
FLAGS = [
    (native._oob_flag, native.check_oob, IndexError, "index out of range in an embedding gather", 1),
    (native._pair_rows_flag, native.check_pair_rows, OverflowError,
     "a pair's rated entries did not fit the capacity pair_rows was given (max_row_len too small)", 1),
    (native.kmf_flag, native.check_kmf, IndexError,
     "KernelMF: an id outside its table, a block / row pointer outside the samples (flag 5)", native.KMF_FLAG_ID | native.KMF_FLAG_PTR),
    (native.knn_flag, native.check_knn, ValueError, "ItemKNN: a row of the ratings CSR does not hold strictly ascending columns", 1),
    (native._rank_overflow_flag, native.check_rank_overflow, OverflowError,
     "a row has more targets than the max_targets the rank call was given", 1),
]


def test_one_flag_word_per_kind_and_device():
    words = [get(CPU) for get, *_ in FLAGS]
    for (get, *_), w in zip(FLAGS, words):
        assert get(CPU) is w and w.dtype == torch.int32 and w.shape == (1,)
    assert len({w.data_ptr() for w in words}) == len(words)


@pytest.mark.parametrize("which", range(len(FLAGS)), ids=["oob", "pair_rows", "kmf", "knn", "rank_overflow"])
def test_a_check_raises_its_message_and_clears_only_its_word(which):
    for get, *_ in FLAGS:
        get(CPU).zero_()
    try:
        for get, _, _, _, word in FLAGS:
            get(CPU).fill_(word)
        get, check, exc, message, _ = FLAGS[which]
        with pytest.raises(exc) as e:
            check(CPU)
        assert type(e.value) is exc and str(e.value) == message
        for j, (other, _, _, _, word) in enumerate(FLAGS):
            assert int(other(CPU)) == (0 if j == which else word)
        check(CPU)                                         # cleared: silent now
    finally:
        for get, *_ in FLAGS:
            get(CPU).zero_()


@pytest.mark.parametrize("bits, named", [(native.KMF_FLAG_ID, ["an id outside its table"]),
                                         (native.KMF_FLAG_BLOCK, ["a sample filed in the wrong block"]),
                                         (native.KMF_FLAG_BLOCK | native.KMF_FLAG_PTR,
                                          ["a sample filed in the wrong block", "a block / row pointer outside the samples"]),
                                         (7, ["an id outside its table", "a sample filed in the wrong block",
                                              "a block / row pointer outside the samples"])])
def test_check_kmf_names_exactly_the_bits_that_were_set(bits, named):
    native.kmf_flag(CPU).fill_(bits)
    with pytest.raises(IndexError) as e:
        native.check_kmf(CPU)
    assert str(e.value) == "KernelMF: " + ", ".join(named) + f" (flag {bits})"
    native.check_kmf(CPU)
