"""GPU: ncf_pair_rows_count / ncf_pair_rows_fill (csrc/pair_rows.hip) against their numpy restatement (tests/pair_rows_ref.py), exact
equality.  R = 8 shared rows of lengths {0, 1, 3, 63, 64, 65, 130, 257}; B = 37 pairs (unsorted, repeats, an unused row), 1 and 0; the
vector path at E in {4, 32, 64, 128, 256} and E = 64 inside a wider buffer, the generic path at E in {1, 50} and at leading dimension
66; the mask cases of pair_rows_ref.mask_tables; capacity at and one below the total; pair rows outside the CSR."""
import numpy as np
import pytest
import torch

from pair_rows_ref import F32, N_ITEMS, check_plan, mask_tables, pair_rows_count_ref, pair_rows_ref, pairs, shared_csr

pytestmark = pytest.mark.gpu

# (E, leading dimension of both embedding tables)
VECTOR = [(4, 4), (32, 32), (64, 64), (128, 128), (256, 256), (64, 72)]
GENERIC = [(1, 1), (50, 50), (50, 66), (64, 66)]


def _wide(a, ld, gpu):
    """``a`` (n, E) as a view of a (n, ld) device buffer whose padding is NaN (a kernel that reads it cannot compare equal)."""
    buf = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float32, device=gpu)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(gpu)
    return buf[:, :a.shape[1]]


def _csr(gpu):
    rowptr, col, val = shared_csr()
    return (rowptr, col, val), tuple(torch.from_numpy(x).to(gpu) for x in (rowptr, col, val))


def _total(rowptr, pr):
    return int(pair_rows_count_ref(rowptr, pr)[0].sum())


@pytest.mark.parametrize("B", [37, 1])
@pytest.mark.parametrize("E,ld", VECTOR + GENERIC)
def test_fill_with_mask_equals_reference(gpu, E, ld, B):
    from deeprecommendation_amd import native
    (rowptr, col, val), dev = _csr(gpu)
    pr = pairs(B)
    cand, rated, plan, twins = mask_tables(rowptr, col, pr, E)
    total = _total(rowptr, pr)
    want = pair_rows_ref(rowptr, col, val, pr, total, (cand, rated))
    mask = (_wide(cand, ld, gpu), _wide(rated, ld, gpu))
    got = native.pair_rows(*dev, torch.from_numpy(pr).to(gpu), total, mask)
    again = native.pair_rows(*dev, torch.from_numpy(pr).to(gpu), total, mask)
    r, c, v, flag = (t.cpu().numpy() for t in got)
    assert np.array_equal(r, want[0])
    assert np.array_equal(c[:total], want[1]) and np.array_equal(v[:total].view(np.uint32), want[2].view(np.uint32))
    assert int(flag[0]) == 0 == want[3]
    assert torch.equal(got[0], again[0])                              # the same inputs give the same bits
    assert torch.equal(got[1][:total], again[1][:total]) and torch.equal(got[2][:total].view(torch.int32), again[2][:total].view(torch.int32))
    if B == 37:
        assert check_plan(plan, twins, rowptr, col, pr, r, c) == {"self", "twins", "twins-both", "half", "over", "nan", "inf"}
    native.check_oob(gpu)                                             # no row was out of range


@pytest.mark.parametrize("B", [37, 1, 0])
def test_fill_without_mask_equals_reference(gpu, B):
    from deeprecommendation_amd import native
    (rowptr, col, val), dev = _csr(gpu)
    pr = pairs(B) if B else np.zeros(0, dtype=np.int64)
    total = _total(rowptr, pr)
    want = pair_rows_ref(rowptr, col, val, pr, total)
    r, c, v, flag = (t.cpu().numpy() for t in native.pair_rows(*dev, torch.from_numpy(pr).to(gpu), total))
    assert np.array_equal(r, want[0]) and r.dtype == np.int64 and len(r) == B + 1
    assert np.array_equal(c[:total], want[1]) and np.array_equal(v[:total], want[2])
    assert int(flag[0]) == 0
    if B == 0:                                                        # with a mask too: nothing is launched
        m = (torch.zeros((0, 32), device=gpu), torch.zeros((N_ITEMS, 32), device=gpu))
        r2 = native.pair_rows(*dev, torch.from_numpy(pr).to(gpu), 0, m)
        assert r2[0].tolist() == [0] and int(r2[3].item()) == 0


@pytest.mark.parametrize("E,ld", [(64, 64), (50, 66), (None, None)])
def test_capacity_one_short_sets_the_flag_and_leaves_the_tail_alone(gpu, E, ld):
    """The raw entry points over buffers of capacity + 64 sentinel entries: with capacity == total the flag stays 0; with total - 1 it
    is set, the first ``capacity`` entries are right and nothing beyond them is written."""
    from deeprecommendation_amd import native
    lib = native.load_library()
    (rowptr, col, val), (d_rowptr, d_col, d_val) = _csr(gpu)
    pr = pairs(37)
    d_pr = torch.from_numpy(pr).to(gpu)
    total = _total(rowptr, pr)
    mask, cand, rated = None, None, None
    if E is not None:
        c_np, r_np, _, _ = mask_tables(rowptr, col, pr, E)
        mask, cand, rated = (c_np, r_np), _wide(c_np, ld, gpu), _wide(r_np, ld, gpu)
    st = native._stream(d_rowptr)
    for capacity, want_flag in ((total, 0), (total - 1, 1)):
        want = pair_rows_ref(rowptr, col, val, pr, capacity, mask)
        out_rowptr = torch.empty(len(pr) + 1, dtype=torch.int64, device=gpu)
        out_col = torch.full((capacity + 64,), -77, dtype=torch.int32, device=gpu)
        out_val = torch.full((capacity + 64,), -77.0, dtype=torch.float32, device=gpu)
        flag = torch.zeros(1, dtype=torch.int32, device=gpu)
        oob = torch.zeros(1, dtype=torch.int32, device=gpu)
        native._check(lib.ncf_pair_rows_count(d_rowptr.data_ptr(), 8, d_pr.data_ptr(), len(pr), out_rowptr.data_ptr(), oob.data_ptr(), st))
        torch.cumsum(out_rowptr, 0, out=out_rowptr)
        native._check(lib.ncf_pair_rows_fill(d_rowptr.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), 8, d_pr.data_ptr(), len(pr),
                                             out_rowptr.data_ptr(), out_col.data_ptr(), out_val.data_ptr(), capacity,
                                             None if cand is None else cand.data_ptr(), ld or 0, None if rated is None else rated.data_ptr(),
                                             ld or 0, N_ITEMS if E else 0, E or 0, 1e-5, 1e-5, flag.data_ptr(), st))
        assert int(flag.item()) == want_flag == want[3] and int(oob.item()) == 0
        assert np.array_equal(out_rowptr.cpu().numpy(), want[0])
        c, v = out_col.cpu().numpy(), out_val.cpu().numpy()
        assert np.array_equal(c[:capacity], want[1]) and np.array_equal(v[:capacity], want[2])
        assert (c[capacity:] == -77).all() and (v[capacity:] == -77.0).all() and len(c) == capacity + 64


def test_pair_rows_outside_the_csr_are_empty_and_raise_the_sticky_flag(gpu):
    from deeprecommendation_amd import native
    (rowptr, col, val), dev = _csr(gpu)
    native._oob_flag(gpu).zero_()
    pr = pairs(37)
    pr[2], pr[9] = -1, 8
    total = _total(rowptr, pr)
    cand, rated, _, _ = mask_tables(rowptr, col, np.clip(pr, 0, 7), 32)
    want = pair_rows_ref(rowptr, col, val, pr, total, (cand, rated))
    assert want[4] == 1 and want[0][3] == want[0][2] and want[0][10] == want[0][9]
    try:
        r, c, v, flag = native.pair_rows(*dev, torch.from_numpy(pr).to(gpu), total, (torch.from_numpy(cand).to(gpu), torch.from_numpy(rated).to(gpu)))
        assert np.array_equal(r.cpu().numpy(), want[0])
        assert np.array_equal(c.cpu().numpy()[:total], want[1]) and np.array_equal(v.cpu().numpy()[:total], want[2])
        assert int(flag.item()) == 0
        with pytest.raises(IndexError):
            native.check_oob(gpu)
    finally:
        native._oob_flag(gpu).zero_()
    native.check_oob(gpu)


def test_binding_refuses_what_the_kernels_cannot_take(gpu):
    from deeprecommendation_amd import native
    _, (rowptr, col, val) = _csr(gpu)
    pr = torch.from_numpy(pairs(37)).to(gpu)
    with pytest.raises(ValueError):
        native.pair_rows(rowptr, col, val, pr, 10, (torch.zeros((36, 8), device=gpu), torch.zeros((N_ITEMS, 8), device=gpu)))
    with pytest.raises(TypeError):
        native.pair_rows(rowptr, col.long(), val, pr, 10)
    with pytest.raises(ValueError):
        native.pair_rows(rowptr, col, val, pr.to(torch.int32), 10)
    with pytest.raises(ValueError):
        native.pair_rows(rowptr, col, val, pr, -1)
