"""GPU: the graph propagation kernels (csrc/spmm.hip), native.SegmentedCSR and PreparedGraph on every launch form, against the
exact and bounded references of tests/graph_forms_ref.py (case tables, references and their derivations are described there;
the CPU tests show that the checks reject subtly wrong kernels).

Integer operands make every order of summation, every split into segments and every tree shape exact, so the SpMM is compared
with ``torch.equal``: a dropped entry, a tail read past its end, a partial sum added twice, a row never written or a layer
accumulator added on two levels cannot hide below a tolerance.  The softmax is compared bitwise where the construction is
exact (constant rows, two levels 200 apart) and held to the per-row 1e-5 bar on random scores; edge_coef and scale_rows are
compared bitwise with their numpy float32 recipes.  The grid-stride cases sit just above the launch caps (65 536 waves,
2 097 152 threads) and check the elements that only the second pass of the loop reaches."""
import copy

import numpy as np
import pytest
import torch

import graph_forms_ref as R
from conftest import record_error

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
NZ = 50


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def _gen(gpu, seed):
    return torch.Generator(device=gpu).manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel_window(rows, cols, top, left, right, gpu):
    """(int32 buffer full of SENTINEL, its float32 window [top:top+rows, left:left+cols], mask of the window)."""
    buf = torch.full((rows + top + 1, left + cols + right), SENTINEL, dtype=torch.int32, device=gpu)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[top:top + rows, left:left + cols] = True
    return buf, buf.view(torch.float32)[top:top + rows, left:left + cols], inside


# ================================================================================================ exact SpMM
@pytest.mark.parametrize("D", R.PLAIN_WIDTHS)
def test_exact_plain_spmm(native, gpu, D):
    rowptr, col, coef, z, y0, acc0 = R.int_problem(R.PLAIN_LENGTHS, NZ, D, _gen(gpu, D), all_bad_row=5)
    N = len(R.PLAIN_LENGTHS)
    assert int((col < 0).sum()) > 10 and int((col >= NZ).sum()) > 10
    for cf in (coef, None):
        ref = R.exact_spmm_reference(rowptr, col, cf, z)
        assert int(ref[5].abs().max()) == 0 and int(ref[0].abs().max()) == 0       # all out of range; empty
        y, acc = y0.clone(), acc0.clone()
        out = native.spmm_csr(rowptr, None, col, cf, z, N, y=y, acc_sum=acc)
        assert out.data_ptr() == y.data_ptr()
        assert R.exact_equal(y, ref), f"coef {cf is not None}"
        assert R.exact_equal(acc, acc0.long() + ref), f"coef {cf is not None}"
        fresh = native.spmm_csr(rowptr, None, col, cf, z, N)                        # y allocated by the call, no acc_sum
        assert torch.equal(_bits(fresh), _bits(y))


@pytest.mark.parametrize("D", [36, 100, 132])
def test_exact_strided_spmm(native, gpu, D):
    """z a column window of a wider buffer, y and acc_sum windows of sentinel buffers: exact inside, nothing written outside."""
    gen = _gen(gpu, 100 + D)
    rowptr, col, coef, _, _, acc0 = R.int_problem(R.PLAIN_LENGTHS, NZ, D, gen)
    N = len(R.PLAIN_LENGTHS)
    zbuf = R.int_tensor((NZ, D + 12), gen)
    z = zbuf[:, 4:4 + D]
    ybuf, y, y_in = _sentinel_window(N, D, 1, 4, 4, gpu)
    abuf, acc, a_in = _sentinel_window(N, D, 2, 8, 4, gpu)
    acc.copy_(acc0)
    assert z.stride(0) == D + 12 and y.stride(0) == D + 8 and acc.stride(0) == D + 12
    assert all(t.data_ptr() % 16 == 0 and not t.is_contiguous() for t in (z, y, acc))
    native.spmm_csr(rowptr, None, col, coef, z, N, y=y, acc_sum=acc)
    ref = R.exact_spmm_reference(rowptr, col, coef, z.contiguous())
    assert R.exact_equal(y.contiguous(), ref)
    assert R.exact_equal(acc.contiguous(), acc0.long() + ref)
    assert bool((ybuf[~y_in] == SENTINEL).all()) and bool((abuf[~a_in] == SENTINEL).all())


@pytest.mark.parametrize("seg_len", [4, 64])
@pytest.mark.parametrize("D", [4, 68, 132])
def test_exact_serial_fixup(native, gpu, seg_len, D):
    """ncf_spmm_csr with row_of and fixup = 1: spmm_fix_kernel adds a split row's partial sums in segment order; a whole row is
    finished by the segment kernel and its slot of ``partial`` is never written."""
    for lengths in (R.TREE_LENGTHS, [9, 9] if seg_len == 4 else [130, 65]):
        rowptr, col, coef, z, y0, acc0 = R.int_problem(lengths, NZ, D, _gen(gpu, 200 + D + seg_len),
                                                          all_bad_row=3 if lengths is R.TREE_LENGTHS else None)
        segptr, row_of, _ = native.SegmentedCSR(rowptr, col, coef, seg_len=seg_len).levels[0]
        assert row_of is not None
        n_seg = row_of.numel()
        pbuf = torch.full((n_seg, D), SENTINEL, dtype=torch.int32, device=gpu)
        y, acc = y0.clone(), acc0.clone()
        native.spmm_csr(segptr, row_of, col, coef, z, len(lengths), y=y, acc_sum=acc, partial=pbuf.view(torch.float32), fixup=True)
        ref = R.exact_spmm_reference(rowptr, col, coef, z)
        assert R.exact_equal(y, ref) and R.exact_equal(acc, acc0.long() + ref)
        whole = torch.bincount(row_of.long(), minlength=len(lengths))[row_of.long()] == 1
        assert bool((pbuf[whole] == SENTINEL).all()) and not bool((pbuf[~whole] == SENTINEL).any())
        assert bool(whole.any()) == (lengths is R.TREE_LENGTHS)


def test_spmm_refusals_launch_nothing(native, gpu):
    lib = native.load_library()
    rowptr, col, coef, _, _, _ = R.int_problem([9, 9], NZ, 8, _gen(gpu, 3))
    segptr, row_of, _ = native.SegmentedCSR(rowptr, col, coef, seg_len=4).levels[0]
    n_seg = row_of.numel()
    zbuf = torch.ones((NZ, 272), device=gpu)
    ybuf = torch.full((2, 272), SENTINEL, dtype=torch.int32, device=gpu)
    pbuf = torch.full((n_seg, 272), SENTINEL, dtype=torch.int32, device=gpu)

    def call(D, ldz=272, ldy=272, z_off=0, y_off=0, rows=True, partial=True, fixup=1):
        return lib.ncf_spmm_csr(native.NCF_F32, segptr.data_ptr(), row_of.data_ptr() if rows else None, n_seg, col.data_ptr(), coef.data_ptr(),
                                zbuf.data_ptr() + 4 * z_off, NZ, ldz, D, ybuf.data_ptr() + 4 * y_off, ldy, None, 0,
                                pbuf.data_ptr() if partial else None, fixup, None)

    assert call(8, partial=False) == native.NCF_EINVAL                        # split rows, fix-up asked for, no partial buffer
    assert "partial" in lib.ncf_last_error().decode()
    assert call(6) == native.NCF_EUNSUPPORTED and call(260) == native.NCF_EUNSUPPORTED
    assert call(8, ldz=270) == native.NCF_EINVAL and call(8, ldy=270) == native.NCF_EINVAL
    assert call(8, z_off=1) == native.NCF_EINVAL and call(8, y_off=2) == native.NCF_EINVAL
    torch.cuda.synchronize()
    assert bool((ybuf == SENTINEL).all()) and bool((pbuf == SENTINEL).all())
    assert call(8) == native.NCF_OK                                           # the same call, well formed, does write
    torch.cuda.synchronize()
    assert not bool((ybuf[:, :8] == SENTINEL).any()) and bool((ybuf[:, 8:] == SENTINEL).all())


@pytest.mark.parametrize("c", R.TREE_CASES, ids=R.tree_id)
def test_exact_segmented_csr(native, gpu, c):
    gen = _gen(gpu, 300 + c.seg_len + c.fan + len(c.lengths))
    N = len(c.lengths)
    rowptr, col, coef, z, y0, acc0 = R.int_problem(c.lengths, NZ, 36, gen, all_bad_row=2 if N > 3 else None)
    z8, coef2 = R.int_tensor((NZ, 8), gen), R.int_tensor((col.numel(),), gen)
    csr = native.SegmentedCSR(rowptr, col, coef, seg_len=c.seg_len, fan=c.fan)
    assert len(csr.levels) == c.levels
    ref = R.exact_spmm_reference(rowptr, col, coef, z)
    ref8 = R.exact_spmm_reference(rowptr, col, coef, z8)
    y, acc = y0.clone(), acc0.clone()
    assert csr.spmm(z, y=y, acc_sum=acc).data_ptr() == y.data_ptr()
    assert R.exact_equal(y, ref) and R.exact_equal(acc, acc0.long() + ref)    # acc_sum added exactly once over the levels
    y8 = csr.spmm(z8)                                                         # another width on the same object ...
    assert R.exact_equal(y8, ref8)
    again = csr.spmm(z)                                                       # ... and back: the cached partial buffers per width
    assert torch.equal(_bits(again), _bits(y)) and R.exact_equal(csr.spmm(z8), ref8)
    assert sorted(csr._partials) == ([8, 36] if c.levels > 1 else [])
    over = csr.spmm(z, coef=coef2)                                            # coef= override
    assert R.exact_equal(over, R.exact_spmm_reference(rowptr, col, coef2, z))
    binary = native.SegmentedCSR(rowptr, col, None, seg_len=c.seg_len, fan=c.fan).spmm(z)
    assert R.exact_equal(binary, R.exact_spmm_reference(rowptr, col, None, z))


def _stride_lengths(head, tail, n_seg, seg_len, gen):
    """Row lengths with ``head`` first and ``tail`` last and short rows (0 .. seg_len entries) between, n_seg segments in all."""
    nseg = lambda n: max(1, -(-n // seg_len))
    middle = n_seg - sum(map(nseg, head + tail))
    mid = torch.randint(0, seg_len + 1, (middle,), generator=gen, device=gen.device).tolist()
    return head + mid + tail


@pytest.mark.parametrize("split", [False, True])
def test_exact_grid_stride_of_the_segment_kernel(native, gpu, split):
    """65 541 segments at D = 4: five more than the 65 536 waves of the capped grid."""
    gen, n_seg = _gen(gpu, 41 + split), R.WAVE_CAP + 5
    lengths = _stride_lengths([9], [9, 9, 9], n_seg, 4, gen) if split else _stride_lengths([3], [2, 4, 1], n_seg, 4, gen)
    rowptr, col, coef, z, y0, acc0 = R.int_problem(lengths, NZ, 4, gen)
    csr = native.SegmentedCSR(rowptr, col, coef, seg_len=4, fan=2)
    assert csr.levels[0][0].numel() - 1 == n_seg and (csr.levels[0][1] is not None) == split and len(csr.levels) == (3 if split else 1)
    y, acc = y0.clone(), acc0.clone()
    csr.spmm(z, y=y, acc_sum=acc)
    ref = R.exact_spmm_reference(rowptr, col, coef, z)
    assert R.exact_equal(y[-3:], ref[-3:]) and int(ref[-3:].abs().max()) > 0  # the rows only the second pass reaches
    assert R.exact_equal(y, ref) and R.exact_equal(acc, acc0.long() + ref)


def test_exact_grid_stride_of_the_fixup_kernel(native, gpu):
    """65 541 segments at D = 132 (LPR 64): five more than the 65 536 lane groups of spmm_fix_kernel's capped grid; the last split
    row starts at segment 65 538."""
    gen, n_seg, D = _gen(gpu, 43), R.WAVE_CAP + 5, 132
    lengths = _stride_lengths([9], [9, 9, 9], n_seg, 4, gen)
    rowptr, col, coef, z, y0, acc0 = R.int_problem(lengths, NZ, D, gen)
    segptr, row_of, _ = native.SegmentedCSR(rowptr, col, coef, seg_len=4).levels[0]
    assert row_of.numel() == n_seg and int(row_of[R.WAVE_CAP + 2]) == len(lengths) - 1 and int(row_of[R.WAVE_CAP + 1]) == len(lengths) - 2
    partial = torch.empty((n_seg, D), device=gpu)
    y, acc = y0.clone(), acc0.clone()
    native.spmm_csr(segptr, row_of, col, coef, z, len(lengths), y=y, acc_sum=acc, partial=partial, fixup=True)
    ref = R.exact_spmm_reference(rowptr, col, coef, z)
    assert R.exact_equal(y[-1:], ref[-1:]) and int(ref[-1].abs().max()) > 0
    assert R.exact_equal(y, ref) and R.exact_equal(acc, acc0.long() + ref)


# ================================================================================================ bounded SpMM
@pytest.mark.parametrize("form", ["plain", (4, 2), (64, 4), (512, 64), "fixup64"], ids=str)
def test_random_spmm_inside_the_bound(native, gpu, form):
    gen, D = _gen(gpu, 51), 68
    lengths = R.PLAIN_LENGTHS if form == "plain" else R.TREE_LENGTHS
    rowptr = R.rowptr_of(lengths, gpu)
    E, N = int(rowptr[-1]), len(lengths)
    col = R.draw_cols(E, NZ, gen)
    coef, z, acc0 = torch.randn(E, generator=gen, device=gpu), torch.randn(NZ, D, generator=gen, device=gpu), torch.randn(N, D, generator=gen, device=gpu)
    acc = acc0.clone()
    if form == "plain":
        y = native.spmm_csr(rowptr, None, col, coef, z, N, acc_sum=acc)
    elif form == "fixup64":
        segptr, row_of, _ = native.SegmentedCSR(rowptr, col, coef, seg_len=64).levels[0]
        y = native.spmm_csr(segptr, row_of, col, coef, z, N, acc_sum=acc, fixup=True)
    else:
        y = native.SegmentedCSR(rowptr, col, coef, seg_len=form[0], fan=form[1]).spmm(z, acc_sum=acc)
    ref = R.spmm_reference64(rowptr, col, coef, z)
    for name, got, want, bound in (("y", y, ref, R.spmm_bound(rowptr, col, coef, z)),
                                   ("acc", acc, ref + acc0.double(), R.spmm_bound(rowptr, col, coef, z, acc0))):
        ok, frac, err, bnd, rel = R.bound_check(got, want, bound)
        print(f"spmm {form} {name}: {frac:.4f} of the bound (err {err:.3e}, bound {bnd:.3e})")
        record_error(f"{form}-{name}", err, bnd, scale_rel=rel)
        assert ok, f"{form} {name}: {frac:.3f} of the bound"


# ================================================================================================ edge softmax
SOFTMAX_LENGTHS = [3000, 0, 1, 2, 9, 130, 64, 7, 65, 300, 3, 0, 128, 40, 641, 5, 513, 2500]   # hub rows first and last


def _softmax_forms(native, case, seg_len):
    """{'row': weights, 'seg': weights} of one case through both entries."""
    rowptr, col, attr, s = case["rowptr"], case["col"], case["attr"], case["s"]
    segptr, row_of, _ = native.SegmentedCSR(rowptr, col, None, seg_len=seg_len).levels[0]
    assert row_of is not None
    seg = (segptr, row_of, R.seg_first_of(row_of, rowptr.numel() - 1))
    E = col.numel()
    out_row = torch.full((E,), float("nan"), device=col.device)
    out_seg = torch.full((E,), float("nan"), device=col.device)
    native.edge_softmax_csr(rowptr, col, attr, s, out=out_row)
    native.edge_softmax_csr(rowptr, col, attr, s, out=out_seg, segments=seg)
    return {"row": out_row, "seg": out_seg}


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("seg_len", [64, 512])
@pytest.mark.parametrize("kind", ["a", "b"])
def test_exact_softmax(native, gpu, kind, seg_len, weighted):
    """Constant rows (a) and two levels 200 apart (b), hub rows first and last, empty rows, rows all out of range: both forms
    give fl32(1 / k) (times attr) bit for bit, and a shift of all scores by an integer changes no bit."""
    case = R.softmax_case(kind, SOFTMAX_LENGTHS, _gen(gpu, 61 + seg_len), block=seg_len, weighted=weighted)
    want = R.exact_softmax_expected(case["rowptr"].cpu(), case["col"].cpu(), None if not weighted else case["attr"].cpu(), case["s"].cpu())
    assert np.isfinite(want).all()
    got = _softmax_forms(native, case, seg_len)
    for form in ("row", "seg"):
        assert R.same_bits(got[form], want), f"{form} form"
    assert torch.equal(_bits(got["row"]), _bits(got["seg"]))
    shifted = _softmax_forms(native, dict(case, s=case["s"] + 5.0), seg_len)
    for form in ("row", "seg"):
        assert torch.equal(_bits(shifted[form]), _bits(got[form])), f"{form} form, shifted"


@pytest.mark.parametrize("kind", ["a", "b"])
def test_exact_softmax_grid_stride(native, gpu, kind):
    """66 000 destinations of 0 - 2 entries between two hub rows: more rows than the 65 536 waves of the row form and of the row
    statistics, more 64-entry segments than the waves of the segment statistics and the apply pass."""
    lengths = [3000] + [r % 3 for r in range(66_000)] + [2500]
    case = R.softmax_case(kind, lengths, _gen(gpu, 71), block=64, weighted=(kind == "b"))
    rowptr = case["rowptr"].cpu()
    want = R.exact_softmax_expected(rowptr, case["col"].cpu(), None if case["attr"] is None else case["attr"].cpu(), case["s"].cpu())
    got = _softmax_forms(native, case, 64)
    tail = int(rowptr[R.WAVE_CAP])                                            # first entry of the rows the second pass walks
    assert len(want) - tail > 2500 and np.count_nonzero(want[tail:]) > 500
    for form in ("row", "seg"):
        assert R.same_bits(got[form][tail:], want[tail:]), f"{form} form, second pass"
        assert R.same_bits(got[form], want), f"{form} form"


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("seg_len", [64, 512])
@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_random_softmax_inside_the_per_row_bar(native, gpu, sigma, seg_len, weighted):
    """N(0, sigma) scores cut at 4 sigma (spread <= 24, rows <= 3000: under the bar by the model of graph_forms_ref)."""
    gen, Ns = _gen(gpu, 81), 400
    assert R.softmax_model_ulps(8 * sigma, max(SOFTMAX_LENGTHS), seg_len) * R.U24 < R.RTOL
    rowptr = R.rowptr_of(SOFTMAX_LENGTHS, gpu)
    E = int(rowptr[-1])
    col = R.draw_cols(E, Ns, gen)
    s = (torch.randn(Ns, generator=gen, device=gpu) * sigma).clamp(-4 * sigma, 4 * sigma)
    attr = torch.randn(E, generator=gen, device=gpu) if weighted else None
    got = _softmax_forms(native, dict(rowptr=rowptr, col=col, attr=attr, s=s), seg_len)
    ref = R.softmax_reference64(rowptr, col, attr, s)
    bar = R.softmax_bar(rowptr, ref)
    for form in ("row", "seg"):
        ok, frac, err, bnd, rel = R.bound_check(got[form], ref, bar)
        print(f"softmax sigma {sigma} seg_len {seg_len} {form}: {frac:.4f} of the bar (err {err:.3e}, bar {bnd:.3e})")
        record_error(form, err, bnd, scale_rel=rel)
        assert ok, f"{form}: {frac:.3f} of the bar"


def test_peaked_softmax_in_a_split_row(native, gpu):
    """One entry 100 above the rest of a split row: its weight is exactly 1, the rest are within the bar."""
    gen, Ns = _gen(gpu, 91), 400
    lengths = [5, 3000, 0, 40]
    rowptr = R.rowptr_of(lengths, gpu)
    col = R.draw_cols(sum(lengths), Ns - 1, gen, bad=False)
    peak = int(rowptr[1]) + 1777
    col[peak], col[peak + 5], col[peak - 9] = Ns - 1, -1, Ns + 2
    s = torch.randn(Ns, generator=gen, device=gpu)
    s[Ns - 1] = 100.0
    got = _softmax_forms(native, dict(rowptr=rowptr, col=col, attr=None, s=s), 64)
    ref = R.softmax_reference64(rowptr, col, None, s)
    bar = R.softmax_bar(rowptr, ref)
    for form in ("row", "seg"):
        assert float(got[form][peak]) == 1.0, form
        ok, frac, err, bnd, rel = R.bound_check(got[form], ref, bar)
        record_error(form, err, bnd, scale_rel=rel)
        assert ok, f"{form}: {frac:.3f} of the bar"


# ================================================================================================ degree, edge_coef, scale_rows
def test_degree_counts_are_exact_and_bad_ids_raise(native, gpu):
    gen, N, E = _gen(gpu, 101), 50, R.THREAD_CAP + 1000
    dst = torch.randint(0, N, (E,), generator=gen, device=gpu)
    dst[: E // 3] = 7                                                         # a hub destination
    dst[-5:] = 11                                                             # elements past the capped grid
    deg = torch.zeros(N, device=gpu)
    native.degree_accumulate(dst, N, deg)
    native.check_oob(gpu)                                                     # clean ids: no flag
    assert torch.equal(deg, torch.bincount(dst, minlength=N).float()) and float(deg[7]) > E // 3
    bad = dst.clone()
    bad[5], bad[E - 2], bad[1000] = -1, N, N + 3
    deg2 = torch.zeros(N, device=gpu)
    native.degree_accumulate(bad, N, deg2)
    ok = (bad >= 0) & (bad < N)
    assert torch.equal(deg2, torch.bincount(bad[ok], minlength=N).float())    # skipped, the rest counted
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.check_oob(gpu)                                                     # the flag is cleared by the raise


@pytest.mark.parametrize("weighted", [True, False])
def test_edge_coef_bitwise(native, gpu, weighted):
    gen, N, E = _gen(gpu, 111), 1000, R.THREAD_CAP + 77
    deg = torch.randint(0, 60, (N,), generator=gen, device=gpu).float()
    deg[3] = 0.0
    deg[4] = 4_000_000.0
    src = torch.randint(0, N, (E,), generator=gen, device=gpu)
    dst = torch.randint(0, N, (E,), generator=gen, device=gpu)
    src[10], dst[11], src[12], dst[12], dst[13], src[E - 1], dst[E - 2] = 3, 3, 4, 4, 4, 3, 4     # an endpoint of degree 0, also past the cap
    src[20], dst[21], src[22], dst[23], src[E - 3] = -1, -1, N, N + 4, N              # out of range: 0
    attr = torch.randn(E, generator=gen, device=gpu) if weighted else None
    coef = native.edge_coef(src, dst, attr, deg)
    want = R.edge_coef_expected(src.cpu(), dst.cpu(), None if attr is None else attr.cpu(), deg.cpu())
    assert R.same_bits(coef[-100:], want[-100:]) and R.same_bits(coef, want)
    c = coef.cpu()
    assert all(float(c[i]) == 0.0 for i in (10, 11, 20, 21, 22, 23, E - 1, E - 3)) and float(c[12].abs()) > 0.0
    assert bool(torch.isfinite(coef).all())


@pytest.mark.parametrize("divisor", [2.0, 3.0, 4.0])
def test_scale_rows_bitwise(native, gpu, divisor):
    """Strided in and out, N * D just above the capped grid, a sentinel border around the output."""
    gen, D = _gen(gpu, 121), 132
    N = R.THREAD_CAP // D + 3
    assert N * D > R.THREAD_CAP
    xbuf = torch.randn((N, D + 3), generator=gen, device=gpu) * 100.0
    x = xbuf[:, 1:1 + D]
    obuf, out, inside = _sentinel_window(N, D, 1, 2, 3, gpu)
    assert native.scale_rows(x, divisor, out=out).data_ptr() == out.data_ptr()
    want = R.scale_rows_expected(x.cpu().numpy(), divisor)
    assert R.same_bits(out.contiguous()[-2:], want[-2:]) and R.same_bits(out.contiguous(), want)
    assert bool((obuf[~inside] == SENTINEL).all())
    fresh = native.scale_rows(x[:7].contiguous(), divisor)
    assert R.same_bits(fresh, want[:7])


def test_scale_rows_and_edge_coef_keep_denormals(native, gpu):
    tiny = torch.tensor([[1e-38, 3e-39, -2e-38, 1.4e-45], [5e-39, 1.2e-38, -7e-42, 0.0]], device=gpu)
    for divisor in (2.0, 3.0, 4.0):
        want = R.scale_rows_expected(tiny.cpu().numpy(), divisor)
        assert np.count_nonzero(want) >= 5
        assert R.same_bits(native.scale_rows(tiny, divisor), want)
    deg = torch.tensor([1.0, 4.0], device=gpu)
    src, dst = torch.tensor([0, 1], device=gpu), torch.tensor([1, 1], device=gpu)
    attr = torch.tensor([3e-39, 1e-38], device=gpu)
    assert R.same_bits(native.edge_coef(src, dst, attr, deg), R.edge_coef_expected(src.cpu(), dst.cpu(), attr.cpu(), deg.cpu()))


# ================================================================================================ PreparedGraph and the models
N_ITEMS, N_USERS, EMB, LAYERS = 40, 70, 64, 3


def _edges(n_inter, seed, binary=False, mixed=False):
    """A bipartite interaction graph in reference numbering (items first); ``mixed`` appends u2i edges whose source is an item node
    and i2u edges whose source is a user node: still a valid hetero graph, but no longer one hoisted table per node range."""
    g = torch.Generator().manual_seed(seed)
    key = torch.unique(torch.randint(0, N_USERS, (n_inter,), generator=g) * N_ITEMS + torch.randint(0, N_ITEMS, (n_inter,), generator=g))
    u, i = key // N_ITEMS + N_ITEMS, key % N_ITEMS
    u2i, i2u = torch.stack([u, i]), torch.stack([i, u])
    if mixed:
        N = N_ITEMS + N_USERS
        extra1 = torch.stack([torch.randint(0, N_ITEMS, (6,), generator=g), torch.randint(0, N, (6,), generator=g)])
        extra2 = torch.stack([torch.randint(N_ITEMS, N, (5,), generator=g), torch.randint(0, N, (5,), generator=g)])
        u2i, i2u = torch.cat([u2i, extra1], dim=1), torch.cat([i2u, extra2], dim=1)
    if binary:
        return u2i, i2u, None, None
    return u2i, i2u, torch.randn(u2i.shape[1], generator=g), torch.randn(i2u.shape[1], generator=g)


def _graph(edges, dev):
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphData
    u2i, i2u, a1, a2 = edges
    return GraphData(user2item_edge_index=u2i.to(dev), item2user_edge_index=i2u.to(dev), user2item_edge_attr=None if a1 is None else a1.to(dev),
                     item2user_edge_attr=None if a2 is None else a2.to(dev), num_items=N_ITEMS, num_users=N_USERS)


def _model(hetero, conv="LightGCN", **kw):
    from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphNCF
    torch.manual_seed(11)
    return GraphNCF(item_dim=N_ITEMS, user_dim=N_USERS, num_gnn_layers=LAYERS, hetero=hetero, node_emb=EMB, mlp_dense_layers=[128],
                    convType=conv, **kw)


def _oracle(m, hetero, edges, users, items, concat=False):
    from oracle import ncf_oracle as O
    state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return O.graph_ncf_forward(state, hetero, LAYERS, concat, False, torch.eye(N_ITEMS), torch.eye(N_USERS), *edges, users, items)


def _batch(seed, B=200):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, N_USERS, (B,), generator=g) + N_ITEMS, torch.randint(0, N_ITEMS, (B,), generator=g)


@pytest.mark.parametrize("binary", [True, False])
def test_hetero_graph_that_is_not_bipartite(native, gpu, binary):
    """Sources of both edge types on both sides: two stacked hoisted tables (z_rows = 2 N), i2u sources offset by N."""
    from test_gpu_basic import assert_close
    edges = _edges(900, 3, binary=binary, mixed=True)
    m = _model(True).eval()
    users, items = _batch(5)
    ref = _oracle(m, True, edges, users, items)
    graph = _graph(edges, gpu)
    m.to(gpu)
    with torch.no_grad():
        out = m(graph, users.to(gpu), items.to(gpu), gpu)
    prep = graph._prepared[("prep", True)]
    N = N_ITEMS + N_USERS
    assert prep.split is None and prep.z_rows == 2 * N and not prep.type_pure
    assert int(prep.col.max()) >= N
    assert_close(out, ref)
    # the CSR by source has a row per stacked table row, and is the exact adjoint of the CSR by destination
    csr_t, eid = prep.transposed()
    assert csr_t.n_rows == 2 * N
    gen = _gen(gpu, 131)
    z, gy, ci = R.int_tensor((2 * N, 8), gen), R.int_tensor((N, 8), gen), R.int_tensor((prep.col.numel(),), gen)
    y = prep.csr.spmm(z, coef=ci)
    dz = csr_t.spmm(gy, coef=ci[eid.long()].contiguous())
    assert R.exact_equal(y, R.exact_spmm_reference(prep.rowptr, prep.col, ci, z))
    assert int((y.double() * gy.double()).sum()) == int((z.double() * dz.double()).sum())
    # LightGAT's softmax groups would mix edge types here
    gat = _model(True, conv="LightGAT").eval().to(gpu)
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            gat(graph, users.to(gpu), items.to(gpu), gpu)


@pytest.mark.parametrize("mask_targets", [True, False])
def test_training_step_on_a_non_bipartite_hetero_graph_takes_the_torch_path(native, gpu, mask_targets):
    from test_gpu_training import _grads_close
    edges = _edges(900, 4, mixed=True)
    m_cpu = _model(True, dropout_rate=0.0).train()
    m_gpu = copy.deepcopy(m_cpu).to(gpu).train()
    g = torch.Generator().manual_seed(6)
    pick = torch.randint(0, 600, (128,), generator=g)                         # batch pairs that are edges
    users, items = edges[0][0][pick], edges[0][1][pick]
    y = torch.rand(128, 1, generator=g) * 5
    graph = _graph(edges, gpu)
    assert m_gpu._hip_training_possible(graph, users.to(gpu))
    assert m_gpu._forward_train_hip(graph, users.to(gpu), items.to(gpu), mask_targets) is None
    out_c = m_cpu(_graph(edges, "cpu"), users, items, "cpu", mask_targets)
    loss_c = torch.nn.functional.mse_loss(out_c, y, reduction="sum")
    loss_c.backward()
    out_g = m_gpu(graph, users.to(gpu), items.to(gpu), gpu, mask_targets)
    assert out_g.requires_grad
    loss_g = torch.nn.functional.mse_loss(out_g, y.to(gpu), reduction="sum")
    loss_g.backward()
    assert abs(float(loss_g) - float(loss_c)) <= 2e-5 * abs(float(loss_c))
    _grads_close(m_gpu, m_cpu, rtol=5e-5)


@pytest.mark.parametrize("hetero", [True, False])
@pytest.mark.parametrize("concat", [True, False])
def test_edgeless_graph(native, gpu, hetero, concat):
    """No edges: every layer's output is 0, so the combined table is the input table (its mean with L zeros: x0 / (L + 1),
    correctly rounded; or x0 beside zero blocks)."""
    from test_gpu_basic import assert_close
    empty = torch.zeros((2, 0), dtype=torch.int64)
    edges = (empty, empty.clone(), None, None)
    m = _model(hetero, concat=concat).eval()
    users, items = _batch(7)
    ref = _oracle(m, hetero, edges, users, items, concat=concat)
    graph = _graph(edges, gpu)
    m.to(gpu)
    with torch.no_grad():
        out = m(graph, users.to(gpu), items.to(gpu), gpu)
        x0 = m._node_table0(graph)
        combined = m.propagate_all(graph)
    assert_close(out, ref)
    if concat:
        assert torch.equal(_bits(combined[:, :EMB]), _bits(x0)) and float(combined[:, EMB:].abs().max()) == 0.0
    else:
        assert R.same_bits(combined, R.scale_rows_expected(x0.cpu().numpy(), LAYERS + 1))


@pytest.mark.parametrize("hetero", [True, False])
def test_graph_with_isolated_nodes(native, gpu, hetero):
    from test_gpu_basic import assert_close
    edges = _edges(60, 9)
    touched = torch.unique(torch.cat([edges[0][0], edges[0][1]]))
    assert touched.numel() < N_ITEMS + N_USERS - 20                           # many nodes of degree 0 on both sides
    m = _model(hetero).eval()
    users, items = _batch(8)
    ref = _oracle(m, hetero, edges, users, items)
    graph = _graph(edges, gpu)
    m.to(gpu)
    with torch.no_grad():
        out = m(graph, users.to(gpu), items.to(gpu), gpu)
    prep = graph._prepared[("prep", hetero)]
    assert int((prep.deg == 0).sum()) > 20 and bool(torch.isfinite(prep.coef).all())
    assert_close(out, ref)
