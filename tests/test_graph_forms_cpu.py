"""CPU tests of the graph propagation case tables and references (tests/graph_forms_ref.py): the references agree with
independent definitions, the case table reaches the forms it claims, and the checks the GPU tests hold the kernels to
(tests/test_gpu_graph_forms.py) are run here against numpy emulators of the segment walk and of the segmented softmax.  The
right emulator passes; every listed defect is rejected by the exact check, and the earlier bar (assert_close at its defaults)
lets two of them pass.  That is what shows the GPU tests fail for a subtly wrong kernel, and that the gap was real."""
import numpy as np
import pytest
import torch

import graph_forms_ref as R
from deeprecommendation_amd.native import SegmentedCSR

D = 8


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _csr(c, rowptr, col, coef=None):
    return SegmentedCSR(rowptr, col, coef, seg_len=c.seg_len, fan=c.fan)


def _entries_per_row(levels):
    """Per level, the number of entries (level 0) or partial sums (deeper levels) of every row the level walks."""
    out = []
    for segptr, row_of, _ in R.levels_to_numpy(levels):
        seglen = np.diff(segptr)
        if row_of is None:
            out.append(seglen)
        else:
            out.append(np.bincount(np.unique(row_of, return_inverse=True)[1], weights=seglen).astype(np.int64))
    return out


# ------------------------------------------------------------------------------------------------------ references
def test_exact_spmm_reference_is_an_int64_index_add():
    rowptr, col, coef, z, _, _ = R.int_problem(R.TREE_LENGTHS, 40, D, _gen(1), all_bad_row=3)
    assert int((col < 0).sum()) > 4 and int((col >= 40).sum()) > 4
    ok = (col >= 0) & (col < 40)
    for cf in (coef, None):
        msg = z.long()[col.long().clamp(0, 39)] * (1 if cf is None else cf.long()[:, None])
        want = torch.zeros((len(R.TREE_LENGTHS), D), dtype=torch.int64).index_add_(0, R.rows_of(rowptr)[ok], msg[ok])
        assert torch.equal(R.exact_spmm_reference(rowptr, col, cf, z), want)
        assert float(R.spmm_bound(rowptr, col, cf, z)[1].abs().max()) == 0.0      # an empty row has bound 0
    assert int(want[3].abs().max()) == 0 and int(want[0].abs().max()) > 0


@pytest.mark.parametrize("kind", ["a", "b"])
def test_exact_softmax_expectation_is_the_float64_definition(kind):
    lengths = [700, 0, 1, 2, 9, 130, 64, 7, 65, 300, 3, 0, 128, 40, 641]
    case = R.softmax_case(kind, lengths, _gen(2))
    rowptr, col, attr, s = case["rowptr"], case["col"], case["attr"], case["s"]
    if kind == "a":
        assert {float(v) for v in s.tolist()} >= {3e4, -3e4}
    plain = R.exact_softmax_expected(rowptr, col, None, s)
    ref = R.softmax_reference64(rowptr, col, None, s)
    assert R.same_bits(plain, ref.float())                                  # 1 / (k + 1e-16) rounds to fl32(1 / k)
    with_attr = R.exact_softmax_expected(rowptr, col, attr, s)
    ref_a = R.softmax_reference64(rowptr, col, attr, s)
    # float64 keeps exp(-200) = 1.4e-87 on the low entries: below half the smallest fp32 denormal, 0 in fp32
    assert bool(((torch.from_numpy(with_attr).double() - ref_a).abs() <= 2.0 ** -23 * ref_a.abs() + 2.0 ** -150).all())
    bad = ((col < 0) | (col >= s.numel())).numpy()
    assert bad.sum() > 20 and not plain[bad].any() and np.isfinite(plain).all()
    dst = R.rows_of(rowptr).numpy()
    assert not plain[dst == 7].any() and (dst == 7).sum() == 7              # a row whose entries are all out of range
    sums = np.bincount(dst, weights=plain.astype(np.float64), minlength=len(lengths))
    live = np.bincount(dst[~bad], minlength=len(lengths)) > 0
    assert np.allclose(sums[live], 1.0, rtol=1e-6) and not sums[~live].any()
    # both emulated forms give the expectation bit for bit
    for seg_len in (None, 64, 512):
        seg = None
        if seg_len is not None:
            segptr, row_of, _ = SegmentedCSR(rowptr, col, None, seg_len=seg_len).levels[0]
            assert row_of is not None
            seg = (segptr, row_of)
        for a in (None, attr):
            assert R.same_bits(R.emulate_softmax(rowptr, col, a, s, seg), R.exact_softmax_expected(rowptr, col, a, s)), seg_len


def test_case_b_has_low_only_segments_and_rows_of_equal_segment_maxima():
    lengths = [700, 0, 1, 2, 9, 130, 64, 7, 65, 300, 3, 0, 128, 40, 641]
    for seg_len in (64, 512):
        case = R.softmax_case("b", [v * (seg_len // 64) for v in lengths], _gen(3), block=seg_len)
        rowptr, col, s = case["rowptr"], case["col"], case["s"].numpy()
        segptr, row_of, _ = R.levels_to_numpy(SegmentedCSR(rowptr, col, None, seg_len=seg_len).levels)[0]
        c = col.numpy().astype(np.int64)
        ok = (c >= 0) & (c < len(s))
        sc = np.where(ok, s[np.clip(c, 0, len(s) - 1)], -np.inf)
        segm = np.array([sc[segptr[g]:segptr[g + 1]].max(initial=-np.inf) for g in range(len(segptr) - 1)])
        rowm = np.full(len(lengths), -np.inf)
        np.maximum.at(rowm, row_of, segm)
        n_seg_row = np.bincount(row_of, minlength=len(lengths))
        low_only = segm == rowm[row_of] - 200
        assert low_only.sum() >= 3                                           # exp(m_seg - M) is exactly 0 there
        shared = [r for r in range(len(lengths)) if n_seg_row[r] >= 2 and np.all(segm[row_of == r] == rowm[r])]
        assert len(shared) >= 1                                              # every factor exactly 1


def test_softmax_model_keeps_the_bounded_cases_under_the_bar():
    for spread, n_row, seg_len in [(24, 3000, None), (24, 3000, 64), (24, 3000, 512), (8, 3000, 64)]:
        assert R.softmax_model_ulps(spread, n_row, seg_len) * R.U24 < R.RTOL, (spread, n_row, seg_len)
    assert R.softmax_model_ulps(40, 9000) * R.U24 > R.RTOL             # the model does bind: a wider case would not fit


# ------------------------------------------------------------------------------------------------------ case table
@pytest.mark.parametrize("c", R.TREE_CASES, ids=R.tree_id)
def test_levels_of_every_row_of_the_table(c):
    rowptr, col, coef, _, _, _ = R.int_problem(c.lengths, 40, D, _gen(4))
    csr = _csr(c, rowptr, col, coef)
    assert len(csr.levels) == c.levels
    row_of = csr.levels[0][1]
    split = [n > c.seg_len for n in c.lengths]
    if not any(split):
        assert row_of is None
    else:
        nseg = np.bincount(row_of.numpy(), minlength=len(c.lengths))
        assert [bool(n > 1) for n in nseg] == split
        assert all(lv[1] is not None for lv in csr.levels)


def test_table_reaches_the_forms_it_claims():
    by_key = {(c.seg_len, c.fan, len(c.lengths)): c for c in R.TREE_CASES}
    for (seg_len, fan) in [(4, 2), (4, 4)]:
        c = by_key[(seg_len, fan, len(R.TREE_LENGTHS))]
        rowptr, col, _, _, _, _ = R.int_problem(c.lengths, 40, D, _gen(5))
        per_level = _entries_per_row(_csr(c, rowptr, col).levels)
        deeper = np.concatenate(per_level[1:])
        assert fan in deeper and fan + 1 in deeper, (seg_len, fan)           # exactly fan and fan + 1 partial sums in a row
        assert c.lengths[0] > seg_len                                         # first row split
    for (seg_len, fan) in [(64, 4), (512, 64)]:                              # first and last row whole beside a split row
        c = by_key[(seg_len, fan, len(R.TREE_LENGTHS))]
        assert c.lengths[0] <= seg_len and c.lengths[-1] <= seg_len and max(c.lengths) > seg_len
    c = by_key[(4, 2, 2)]
    assert all(n > c.seg_len for n in c.lengths)                             # first and last row both split, every row split
    # a row that becomes single-segment at a middle level: 5 entries at (4, 2) are 2 partial sums, one segment at level 1 of 10
    c = by_key[(4, 2, len(R.TREE_LENGTHS))]
    rowptr, col, _, _, _, _ = R.int_problem(c.lengths, 40, D, _gen(5))
    segptr, row_of, _ = R.levels_to_numpy(_csr(c, rowptr, col).levels)[1]
    assert list(np.diff(segptr)[row_of == 4]) == [2]
    assert set(R.PLAIN_LENGTHS) >= {0, 1, 15, 16, 17, 63, 64, 65}
    assert {R.lanes_per_row(d) for d in R.PLAIN_WIDTHS} == {8, 16, 32, 64}
    assert [d for d in R.PLAIN_WIDTHS if R.lanes_per_row(d) != R.lanes_per_row(d - 4)] == [36, 68, 132]


def test_a_matrix_without_rows_is_accepted_with_null_operands():
    """SegmentedCSR.spmm on no rows passes a (0, D) y, whose pointer is null: nothing to do, not a bad argument (host-side check
    only: no launch either way).  With segments to walk a null y stays refused."""
    import os
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = native.load_library()
    rp = torch.zeros(3, dtype=torch.int64)
    assert torch.empty((0, 36)).data_ptr() == 0
    assert lib.ncf_spmm_csr(native.NCF_F32, rp.data_ptr(), None, 0, None, None, None, 0, 36, 36, None, 36, None, 0, None, 1, None) == native.NCF_OK
    assert lib.ncf_spmm_csr(native.NCF_F32, rp.data_ptr(), None, 2, None, None, None, 0, 36, 36, None, 36, None, 0, None, 1, None) == native.NCF_EINVAL
    assert lib.ncf_spmm_csr(native.NCF_F32, None, None, 0, None, None, None, 0, 36, 36, None, 36, None, 0, None, 1, None) == native.NCF_EINVAL
    assert lib.ncf_spmm_csr(native.NCF_F32, rp.data_ptr(), None, 0, None, None, None, 0, 36, 38, None, 36, None, 0, None, 1, None) == native.NCF_EUNSUPPORTED


# ------------------------------------------------------------------------------------- emulators against the checks
def _run_tree(c, defect=None, seed=6):
    """(y exact, acc exact) of the emulated SegmentedCSR.spmm on the case's integer problem."""
    rowptr, col, coef, z, y0, acc0 = R.int_problem(c.lengths, 40, D, _gen(seed), all_bad_row=2 if len(c.lengths) > 3 else None)
    levels = R.levels_to_numpy(_csr(c, rowptr, col, coef).levels)
    y, acc = y0.double().numpy().copy(), acc0.double().numpy().copy()
    R.emulate_tree(levels, col.numpy(), coef.numpy(), z.double().numpy(), y, acc, defect)
    ref = R.exact_spmm_reference(rowptr, col, coef, z)
    return (R.exact_equal(torch.from_numpy(y).float(), ref),
            R.exact_equal(torch.from_numpy(acc).float(), acc0.long() + ref))


def _run_fixup(lengths, seg_len, defect=None, seed=7):
    rowptr, col, coef, z, y0, acc0 = R.int_problem(lengths, 40, D, _gen(seed))
    segptr, row_of, _ = R.levels_to_numpy(SegmentedCSR(rowptr, col, coef, seg_len=seg_len).levels)[0]
    y, acc = y0.double().numpy().copy(), acc0.double().numpy().copy()
    partial = R.emulate_fixup(segptr, row_of, col.numpy(), coef.numpy(), z.double().numpy(), y, acc, defect)
    ref = R.exact_spmm_reference(rowptr, col, coef, z)
    whole = np.bincount(row_of, minlength=len(lengths))[row_of] == 1
    return (R.exact_equal(torch.from_numpy(y).float(), ref), R.exact_equal(torch.from_numpy(acc).float(), acc0.long() + ref),
            bool(np.isnan(partial[whole]).all()) and not bool(np.isnan(partial[~whole]).any()))


@pytest.mark.parametrize("c", R.TREE_CASES, ids=R.tree_id)
def test_right_emulator_is_exact_on_every_row_of_the_table(c):
    assert _run_tree(c) == (True, True)


@pytest.mark.parametrize("lengths,seg_len", [(R.TREE_LENGTHS, 4), (R.TREE_LENGTHS, 64), ([9, 9], 4)])
def test_right_fixup_emulator_is_exact_and_leaves_whole_rows_partials_alone(lengths, seg_len):
    assert _run_fixup(lengths, seg_len) == (True, True, True)


def _tree_case(seg_len, fan, n_rows=len(R.TREE_LENGTHS)):
    return next(c for c in R.TREE_CASES if (c.seg_len, c.fan, len(c.lengths)) == (seg_len, fan, n_rows))


# defect -> where the exact check must reject it: ("tree", seg_len, fan, rows) or ("fixup", lengths, seg_len)
REJECTED_BY = {
    "drop_last_entry": [("tree", 4, 2, 14), ("tree", 512, 64, 14), ("fixup", R.TREE_LENGTHS, 64)],
    "tail_overread": [("tree", 4, 2, 14), ("tree", 512, 64, 14), ("fixup", R.TREE_LENGTHS, 4)],
    "partial_twice": [("tree", 4, 2, 14), ("tree", 64, 4, 14), ("tree", 4, 2, 2), ("fixup", R.TREE_LENGTHS, 64)],
    "middle_row_unwritten": [("tree", 4, 2, 14), ("tree", 4, 4, 14), ("tree", 8, 3, 14)],
    "acc_on_two_levels": [("tree", 4, 2, 14), ("tree", 512, 64, 14), ("tree", 4, 2, 2)],
    "no_edge_guards": [("tree", 64, 4, 14), ("tree", 512, 64, 14), ("fixup", [9, 9], 4), ("fixup", R.TREE_LENGTHS, 4)],
}


@pytest.mark.parametrize("defect", R.SPMM_DEFECTS)
def test_exact_check_rejects_each_spmm_defect(defect):
    assert set(REJECTED_BY) == set(R.SPMM_DEFECTS)
    for where in REJECTED_BY[defect]:
        if where[0] == "tree":
            y_ok, acc_ok = _run_tree(_tree_case(*where[1:]), defect)
        else:
            y_ok, acc_ok, _ = _run_fixup(where[1], where[2], defect)
        assert not (y_ok and acc_ok), where
        if defect == "acc_on_two_levels":
            assert y_ok and not acc_ok                                       # only acc_sum == acc0 + y sees this one


def test_exact_check_rejects_each_softmax_defect():
    lengths = [700, 0, 1, 2, 9, 130, 64, 7, 65, 300, 3, 0, 128, 40, 641]
    assert R.SOFTMAX_DEFECTS == ["segment_max_no_rescale", "oob_counted"]
    for kind in ("a", "b"):
        case = R.softmax_case(kind, lengths, _gen(8))
        rowptr, col, attr, s = case["rowptr"], case["col"], case["attr"], case["s"]
        segptr, row_of, _ = SegmentedCSR(rowptr, col, None, seg_len=64).levels[0]
        want = R.exact_softmax_expected(rowptr, col, attr, s)
        assert not R.same_bits(R.emulate_softmax(rowptr, col, attr, s, None, "oob_counted"), want)
        assert not R.same_bits(R.emulate_softmax(rowptr, col, attr, s, (segptr, row_of), "oob_counted"), want)
        got = R.emulate_softmax(rowptr, col, attr, s, (segptr, row_of), "segment_max_no_rescale")
        assert R.same_bits(got, want) == (kind == "a")                       # (a) has no low segment; (b) is what pins the rescale


# --------------------------------------------------------------------------------------- what the earlier bar let through
def test_earlier_bar_passes_a_dropped_entry_in_a_long_row():
    """A hub destination with degree-normalised coefficients and embeddings of one sign (what a LightGCN layer sums): one entry
    is 1 / n of the row, below 1e-5 for n = 300 000.  The exact check sees the same defect on integer data."""
    n, Nz = R.MAX_ROW, 500
    lengths = [3, n, 0, 40]
    gen = _gen(9)
    rowptr = R.rowptr_of(lengths)
    col = R.draw_cols(sum(lengths), Nz, gen, bad=False)
    z = torch.rand(Nz, 4, generator=gen) + 0.5
    coef = torch.full((sum(lengths),), float(n) ** -0.5)
    csr = SegmentedCSR(rowptr, col, coef, seg_len=512)
    levels = R.levels_to_numpy(csr.levels)
    assert len(levels) == 3
    ref = R.spmm_reference64(rowptr, col, coef, z)
    # only the hub row's last segment loses its last entry: the defect as a wrong tail would show it
    short = col.clone()
    short[int(rowptr[2]) - 1] = -1
    y = np.zeros((4, 4))
    R.emulate_tree(levels, short.numpy(), coef.numpy(), z.double().numpy(), y, None)
    assert not np.array_equal(y, ref.numpy()) and R.passes_assert_close(y, ref)
    zi, ci = R.int_tensor((Nz, 4), gen), R.int_tensor((sum(lengths),), gen)
    ci[int(rowptr[2]) - 1], zi[int(col[int(rowptr[2]) - 1])] = 3.0, torch.tensor([1.0, -2.0, 5.0, 7.0])
    yi = np.zeros((4, 4))
    R.emulate_tree(levels, short.numpy(), ci.numpy(), zi.double().numpy(), yi, None)
    assert not R.exact_equal(torch.from_numpy(yi).float(), R.exact_spmm_reference(rowptr, col, ci, zi))
    yi = np.zeros((4, 4))
    R.emulate_tree(levels, col.numpy(), ci.numpy(), zi.double().numpy(), yi, None)
    assert R.exact_equal(torch.from_numpy(yi).float(), R.exact_spmm_reference(rowptr, col, ci, zi))


def test_earlier_bar_passes_an_unrescaled_low_segment():
    """A hub row of 17 full segments and a one-entry tail whose score is far below: without exp(m_seg - M) the tail counts 1 in
    the denominator, 1.1e-4 of weights of 1.1e-4, under a floor that the one-entry rows (weight 1) set at 1e-6.  Case (b)
    rejects the same defect bit for bit."""
    N, hub = 300, 17 * 512 + 1
    lengths = [hub] + [1] * 20 + [0] + [5] * 30
    gen = _gen(10)
    rowptr = R.rowptr_of(lengths)
    col = torch.randint(0, N - 1, (sum(lengths),), generator=gen).to(torch.int32)
    col[hub - 1] = N - 1
    s = torch.randn(N, generator=gen) * 0.01
    s[N - 1] = -30.0
    segptr, row_of, _ = SegmentedCSR(rowptr, col, None, seg_len=512).levels[0]
    ref = R.softmax_reference64(rowptr, col, None, s)
    good = R.emulate_softmax(rowptr, col, None, s, (segptr, row_of))
    bad = R.emulate_softmax(rowptr, col, None, s, (segptr, row_of), "segment_max_no_rescale")
    bar = R.softmax_bar(rowptr, ref)
    assert bool(((torch.from_numpy(good).double() - ref).abs() <= bar).all())
    assert R.passes_assert_close(bad, ref)                                   # the earlier bar: passes
    assert not bool(((torch.from_numpy(bad).double() - ref).abs() <= bar).all())   # the per-row bar: rejects
