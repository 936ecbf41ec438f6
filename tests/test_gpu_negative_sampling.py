"""GPU tests of the negative-sampling kernels (csrc/negsample.hip) against tests/negsample_ref.py, the header's contract in numpy.
ncf_negative_cdf: bit for bit against cdf_exact where the weights are specified to the bit (w = 0 and w = 1), within 1e-6 of the
float64 CDF elsewhere (the device's powf is not), with more rows than the launch has waves so that every wave walks rows of
changing form, flagged rows among good ones, the clamp and the register / streamed boundary.  ncf_sample_negatives: against
draw_ref (numpy's searchsorted over the kernel's CDF, u restated from the header's hash) past the grid cap, at u equal to a CDF
entry, on CDFs that do not end in 1, on empty rows and bad picks; against the reference's probabilities; both calls captured
into a graph; and their refusals and flags."""
import math

import numpy as np
import pytest
import torch

import negsample_ref as R
from negsample_ref import slot_uniform

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 300, 4097, 20000]
W_SCHEDULE = [0.0, 0.5, 1.0, 1.5, 3.0]
# one or several 64-entry chunks, both sides of the 512-entry boundary between the register and the streamed form, and a
# streamed row of more than one pass-1 round; 11 lengths, coprime to the number of waves
CYCLE = [1, 2, 63, 64, 65, 511, 512, 513, 576, 577, 1025]


def _csr(lengths, seed):
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rating = (rng.integers(0, 11, int(rowptr[-1])) * 0.5).astype(np.float32)      # zeros inside rows
    for r, n in enumerate(lengths):
        s = rowptr[r]
        if n >= 3:
            rating[s] = rating[s + n - 1] = 0.0                                      # and at both ends
        rating[s + n // 2] = 3.5                                                     # every row keeps a positive weight
    neg = rng.integers(0, 1 << 20, int(rowptr[-1])).astype(np.int32)
    return rowptr, rating, neg


def _ref_cdf(rating, rowptr, w):
    out = np.empty(len(rating), dtype=np.float64)
    for r in range(len(rowptr) - 1):
        s, e = rowptr[r], rowptr[r + 1]
        wt = np.ones(e - s) if w == 0 else rating[s:e].astype(np.float64) ** w
        out[s:e] = np.cumsum(wt) / wt.sum()
    return out


def _dev(gpu, *arrays):
    return [torch.from_numpy(a).to(gpu) for a in arrays]


@pytest.mark.parametrize("w", W_SCHEDULE)
def test_negative_cdf_matches_float64_is_monotone_and_ends_in_one(gpu, w):
    from deeprecommendation_amd import native
    rowptr, rating, _ = _csr(LENGTHS, 1)
    rp, rt = _dev(gpu, rowptr, rating)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    cdf = native.negative_cdf(rp, rt, w, flag=flag).cpu().numpy()
    assert int(flag.item()) == 0
    ref = _ref_cdf(rating, rowptr, w)
    assert float(np.abs(cdf - ref).max()) <= 1e-6
    for r in range(len(LENGTHS)):
        s, e = rowptr[r], rowptr[r + 1]
        row = cdf[s:e]
        assert row[-1] == np.float32(1.0)
        assert (np.diff(row) >= 0).all()
        if w > 0:
            zero = np.flatnonzero(rating[s:e] == 0)
            for k in zero:                                  # a zero weight repeats its predecessor (0.0 at the row's start)
                assert row[k] == (row[k - 1] if k > 0 else 0.0)


def test_draws_equal_searchsorted_over_the_kernel_cdf(gpu):
    from deeprecommendation_amd import native
    lengths = [1, 2, 5, 63, 64, 65, 300, 1000, 4097] * 7
    rowptr, rating, neg = _csr(lengths, 2)
    rp, rt, ng = _dev(gpu, rowptr, rating, neg)
    cdf = native.negative_cdf(rp, rt, 1.5)
    n, seed, slot0 = 1 << 20, 987654321, (1 << 32) - 5000          # slots cross the 32-bit boundary
    pick = torch.from_numpy(np.random.default_rng(3).integers(0, len(lengths), n)).to(gpu)
    out = native.sample_negatives(rp, cdf, ng, pick, seed, slot0).cpu()
    native.check_oob(gpu)
    cdf_h, pick_h = cdf.cpu().numpy(), pick.cpu().numpy()
    u = slot_uniform(seed, slot0 + np.arange(n, dtype=np.uint64))
    want = np.empty(n, dtype=np.int64)
    for r in range(len(lengths)):
        sel = np.flatnonzero(pick_h == r)
        s, e = rowptr[r], rowptr[r + 1]
        j = np.searchsorted(cdf_h[s:e], u[sel], side="right")
        want[sel] = neg[s + np.minimum(j, e - s - 1)]
    assert torch.equal(out, torch.from_numpy(want))
    ref, bad = R.draw_ref(rowptr, cdf_h, neg, pick_h, seed, slot0)
    assert not bad and np.array_equal(ref, want)
    again = native.sample_negatives(rp, cdf, ng, pick, seed, slot0).cpu()
    assert torch.equal(again, out)                                  # same seed and slots: same draws
    assert not torch.equal(native.sample_negatives(rp, cdf, ng, pick, seed + 1, slot0).cpu(), out)


@pytest.mark.parametrize("w", [0.0, 1.5, 3.0])
def test_draw_frequencies_follow_the_reference_probabilities(gpu, w):
    """2^22 draws per row; every entry's count within 6 sigma of N p with p from the reference's formula (r ** w / sum r ** w,
    datasets/base.py:62-64); zero-weight entries never drawn; w = 0 uniform."""
    from deeprecommendation_amd import native
    lengths = [5, 64, 300]
    rowptr, rating, _ = _csr(lengths, 4)
    neg = np.arange(int(rowptr[-1]), dtype=np.int32)                  # the draw's own CSR position
    rp, rt, ng = _dev(gpu, rowptr, rating, neg)
    cdf = native.negative_cdf(rp, rt, w)
    N = 1 << 22
    for r in range(len(lengths)):
        pick = torch.full((N,), r, dtype=torch.int64, device=gpu)
        got = native.sample_negatives(rp, cdf, ng, pick, 77 + r, r * N).cpu().numpy()
        s, e = rowptr[r], rowptr[r + 1]
        counts = np.bincount(got - s, minlength=e - s).astype(np.float64)
        wt = np.ones(e - s) if w == 0 else rating[s:e].astype(np.float64) ** w
        p = wt / wt.sum()
        assert counts.sum() == N and len(counts) == e - s
        sigma = np.sqrt(N * p * (1 - p))
        assert (np.abs(counts - N * p) <= 6 * sigma + 1e-9).all(), (w, r)
        assert (counts[p == 0] == 0).all()
    native.check_oob(gpu)


def test_refusals_launch_nothing(gpu):
    from deeprecommendation_amd import native
    lib = native.load_library()
    rowptr, rating, neg = _csr([3, 4], 5)
    rp, rt, ng = _dev(gpu, rowptr, rating, neg)
    cdf = torch.full_like(rt, -7.0)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    pick = torch.zeros(4, dtype=torch.int64, device=gpu)
    out = torch.full((4,), -9, dtype=torch.int64, device=gpu)
    p = lambda t: t.data_ptr()   # noqa: E731
    EINVAL = native.NCF_EINVAL
    assert lib.ncf_negative_cdf(p(rp), 2, p(rt), -0.5, p(cdf), p(flag), None) == EINVAL
    assert lib.ncf_negative_cdf(p(rp), 2, p(rt), float("nan"), p(cdf), p(flag), None) == EINVAL
    assert lib.ncf_negative_cdf(p(rp), -1, p(rt), 1.0, p(cdf), p(flag), None) == EINVAL
    assert lib.ncf_negative_cdf(None, 2, p(rt), 1.0, p(cdf), p(flag), None) == EINVAL
    assert lib.ncf_negative_cdf(p(rp), 2, p(rt), 1.0, p(cdf), None, None) == EINVAL
    assert b"ncf_negative_cdf" in lib.ncf_last_error()
    assert lib.ncf_sample_negatives(p(rp), p(cdf), p(ng), 2, p(pick), -1, 1, 0, p(out), None, None) == EINVAL
    assert lib.ncf_sample_negatives(p(rp), p(cdf), p(ng), -2, p(pick), 4, 1, 0, p(out), None, None) == EINVAL
    assert lib.ncf_sample_negatives(p(rp), p(cdf), p(ng), 2, p(pick), 4, 1, -3, p(out), None, None) == EINVAL
    assert lib.ncf_sample_negatives(p(rp), None, p(ng), 2, p(pick), 4, 1, 0, p(out), None, None) == EINVAL
    assert lib.ncf_sample_negatives(p(rp), p(cdf), p(ng), 2, p(pick), 4, 1, 0, None, None, None) == EINVAL
    assert b"ncf_sample_negatives" in lib.ncf_last_error()
    assert lib.ncf_sample_negatives(p(rp), p(cdf), p(ng), 2, None, 0, 1, 0, None, None, None) == native.NCF_OK   # n == 0
    torch.cuda.synchronize()
    assert bool((cdf == -7.0).all()) and bool((out == -9).all()) and int(flag.item()) == 0


def test_overflowing_total_and_out_of_range_picks_raise(gpu):
    from deeprecommendation_amd import native
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import NegativeSampler
    rowptr = np.array([0, 3, 5], dtype=np.int64)
    rating = np.array([1e20, 2e20, 3e20, 1.0, 2.0], dtype=np.float32)      # finite ratings; (1e20) ** 3 overflows fp32
    neg = np.arange(5, dtype=np.int32)
    rp, rt, ng = _dev(gpu, rowptr, rating, neg)
    sampler = NegativeSampler(rp, ng, rt)
    pick = torch.tensor([0, 1, 1, 0], dtype=torch.int64, device=gpu)
    d = sampler.draw(pick, 1.0, 5, 0)                                        # w = 1: the total is finite
    sampler.check()
    assert set(d.cpu().tolist()) <= {0, 1, 2, 3, 4}
    d = sampler.draw(pick, 3.0, 5, 0)                                        # rebuilt for w = 3: row 0 overflows
    with pytest.raises(ValueError, match="w = 3"):
        sampler.check()
    assert set(d.cpu().tolist()) <= {0, 1, 2, 3, 4}                          # still inside the rows, no fault
    sampler.check()                                                          # the flag was cleared
    bad = torch.tensor([0, 2, -1, 1], dtype=torch.int64, device=gpu)
    out = native.sample_negatives(rp, sampler.cdf, ng, bad, 5, 0).cpu().tolist()
    assert out[1] == -1 and out[2] == -1 and out[0] in (0, 1, 2) and out[3] in (3, 4)
    with pytest.raises(IndexError):
        native.check_oob(gpu)


# ================================================================================================ every launch form, exactly
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _cdf(gpu, rowptr, rating, w, expect_flag):
    """The kernel's CDF (numpy) through a flag of the test's own, which must end as ``expect_flag``."""
    from deeprecommendation_amd import native
    rp, rt = _dev(gpu, rowptr, rating)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    cdf = native.negative_cdf(rp, rt, w, flag=flag).cpu().numpy()
    assert int(flag.item()) == expect_flag
    return cdf


def _assert_same_bits(got, want, rowptr):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    if len(bad):
        k = int(bad[0])
        r = int(np.searchsorted(rowptr, k, side="right") - 1)
        raise AssertionError(f"{len(bad)} of {len(got)} entries differ; first at entry {k - rowptr[r]} of row {r} (length "
                             f"{rowptr[r + 1] - rowptr[r]}): kernel {got[k]!r} ({_bits(got[k:k + 1])[0]:#010x}), "
                             f"contract {want[k]!r} ({_bits(want[k:k + 1])[0]:#010x})")


def _assert_structure(cdf, rowptr, wt):
    """Every (non-empty) row ends in exactly 1.0f and is non-decreasing; a zero weight repeats its predecessor's bits, 0.0f at a
    row's start."""
    assert (np.diff(rowptr) > 0).all()
    assert (_bits(cdf[rowptr[1:] - 1]) == 0x3F800000).all()
    first = np.zeros(len(cdf), dtype=bool)
    first[rowptr[:-1]] = True
    step = np.diff(cdf)
    assert (step[~first[1:]] >= 0).all()
    zero = np.asarray(wt) == 0
    bits = _bits(cdf)
    assert (bits[zero & first] == 0).all()
    inner = np.flatnonzero(zero & ~first)
    assert (bits[inner] == bits[inner - 1]).all()
    return int(zero.sum())


def _waves(gpu):
    """The waves of ncf_negative_cdf's largest launch: num_cus() * 8 workgroups of 4."""
    return 32 * torch.cuda.get_device_properties(gpu).multi_processor_count


@pytest.fixture(scope="module")
def walked(gpu):
    """More than twice as many rows as the launch has waves, so that every wave takes three rows (some two) in turn; their
    lengths cycle through CYCLE, whose 11 entries are coprime to the number of waves: rows r, r + waves and r + 2 waves of one
    wave differ in length, and among the waves every change of form occurs (register to streamed and back, one chunk to several
    and back).  State that a wave keeps from one row to the next shows in the next row's bits.  Read-only."""
    waves = _waves(gpu)
    rows = 2 * waves + 37
    assert rows > waves and math.gcd(len(CYCLE), waves) == 1
    rowptr, rating, neg, groups = R.rows_cycle(rows, CYCLE, 21)
    lens = np.diff(rowptr)
    a, b, c = lens[:waves], lens[waves:2 * waves], lens[2 * waves:]
    assert (a != b).all() and (b[:37] != c).all() and (a[:37] != c).all()      # no wave meets one length twice
    for first, then in ((a, b), (b[:37], c)):                                  # register form -> streamed and back, 1 chunk <-> many
        assert ((first <= 512) & (then > 512)).any() and ((first > 512) & (then <= 512)).any()
        assert ((first <= 64) & (then > 64)).any() and ((first > 64) & (then <= 64)).any()
    return waves, rowptr, rating, neg, groups


@pytest.mark.parametrize("w", [0.0, 1.0])
def test_cdf_is_the_contract_bit_for_bit_when_every_wave_walks_rows_of_changing_form(gpu, walked, w):
    waves, rowptr, rating, _, groups = walked
    assert len(rowptr) - 1 > waves and math.gcd(len(CYCLE), waves) == 1
    cdf = _cdf(gpu, rowptr, rating, w, expect_flag=0)
    want, flagged = R.cdf_exact(R.weights(rating, w), rowptr, groups)
    assert not flagged
    _assert_same_bits(cdf, want, rowptr)
    _assert_structure(cdf, rowptr, R.weights(rating, w))


@pytest.mark.parametrize("w", [0.5, 1.5, 3.0])
def test_cdf_stays_within_1e_6_of_float64_when_every_wave_walks_rows_of_changing_form(gpu, walked, w):
    waves, rowptr, rating, _, _ = walked
    assert len(rowptr) - 1 > waves and math.gcd(len(CYCLE), waves) == 1
    cdf = _cdf(gpu, rowptr, rating, w, expect_flag=0)
    ref = R.cdf_float64(R.weights(rating, w), rowptr)
    err = float(np.abs(cdf - ref).max())
    print(f"w = {w}: max |cdf - float64| = {err:.3e}")
    assert err <= 1e-6
    assert _assert_structure(cdf, rowptr, rating) > len(rowptr)               # zero ratings are zero weights for any w > 0


def test_flagged_rows_leak_nothing_into_the_rows_their_wave_takes_next(gpu):
    waves = _waves(gpu)
    rows = 2 * waves + 37
    assert rows > waves
    rowptr, rating, _, kind = R.rows_cycle_flagged(rows, CYCLE, 22)
    assert all((kind == k).sum() > 100 for k in range(len(R.FLAGGED_KINDS)))
    cdf = _cdf(gpu, rowptr, rating, 1.0, expect_flag=1)
    for r in np.flatnonzero(kind >= 0):                                       # a flagged row: the uniform prefix, bit for bit
        row = cdf[rowptr[r]:rowptr[r + 1]]
        assert np.array_equal(_bits(row), _bits(R.uniform_prefix(len(row)))), (r, R.FLAGGED_KINDS[kind[r]])
    want, flagged = R.cdf_exact(rating, rowptr)
    assert flagged
    _assert_same_bits(cdf, want, rowptr)                                      # and every other row as if the flagged were not there


def test_a_csr_of_one_empty_row_sets_the_flag_and_writes_nothing(gpu):
    from deeprecommendation_amd import native
    rp = torch.zeros(2, dtype=torch.int64, device=gpu)
    rt = torch.full((1,), 3.5, device=gpu)                                    # one entry past the CSR's none
    out = torch.full((1,), -7.0, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    native.negative_cdf(rp, rt, 1.0, out=out, flag=flag)
    assert int(flag.item()) == 1 and out.item() == -7.0


ZERO_U = (2024, 2623356)   # slot_uniform(seed, slot) == 0.0 (tests/test_negsample_cpu.py checks it)


def test_clamp_magnitudes_and_the_513th_entry_are_the_contract_bit_for_bit(gpu):
    """The rows whose bits depend on S and on the clamp.  Where nothing is clamped, another S scales every q and the total by
    the same power of two and the quotient keeps its bits (ratings of the data set's domain cannot tell 62 from 63); a clamped
    weight is one unit whatever S is, so its prefix 1 / total halves when S grows by one."""
    from deeprecommendation_amd import native
    tiny = np.array([1e-20, 5.0, 1e-20, 0.0, 2.5], dtype=np.float32)
    mixed = np.array([1e-30, 1.0, 1e19], dtype=np.float32)
    _, r512, _, _ = R.rows_cycle(1, [512], 5)
    r513 = np.concatenate([r512, np.zeros(1, dtype=np.float32)])             # the same bit length: the same S
    rows = [tiny, mixed, r512, r513]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    rating = np.concatenate(rows)
    cdf = _cdf(gpu, rowptr, rating, 1.0, expect_flag=0)
    want, _ = R.cdf_exact(rating, rowptr)
    _assert_same_bits(cdf, want, rowptr)
    t, m, a, b = (cdf[rowptr[r]:rowptr[r + 1]] for r in range(4))
    assert 0 < t[0] < 2e-18 and _bits(t[1]) == _bits(t[2]) == _bits(t[3]) and t[4] == 1.0     # one unit of 2^59 + 2^58 + 2
    assert 0 < m[0] < m[1] < 1e-17 and m[2] == 1.0
    assert np.array_equal(_bits(b[:512]), _bits(a)) and _bits(b[512:])[0] == 0x3F800000       # streamed and register form
    # u == 0 draws the clamped entry 0 of the tiny row, whose prefix is positive, but entry 1 of [0, 3.5]: a leading zero weight
    seed, slot = ZERO_U
    assert slot_uniform(seed, [slot])[0] == 0.0
    rp2, rt2 = _dev(gpu, np.array([0, 5, 7], dtype=np.int64), np.concatenate([tiny, np.array([0.0, 3.5], dtype=np.float32)]))
    ng2 = torch.arange(7, dtype=torch.int32, device=gpu)
    cdf2 = native.negative_cdf(rp2, rt2, 1.0)
    got = native.sample_negatives(rp2, cdf2, ng2, torch.tensor([0, 1], device=gpu), seed, slot).cpu().tolist()
    got += native.sample_negatives(rp2, cdf2, ng2, torch.tensor([1, 1], device=gpu), seed, slot - 1).cpu().tolist()
    native.check_oob(gpu)
    assert got[0] == 0 and got[3] == 6                                        # got[3]: row 1 at the slot of u == 0


def test_draws_past_the_grid_cap_equal_the_reference_on_every_pick(gpu):
    """2^24 + 1000 picks: the launch is capped at 65 536 blocks of 256, so the first 1000 lanes take a second pick."""
    from deeprecommendation_amd import native
    rowptr, rating, neg, _ = R.rows_cycle(9, [1, 2, 3, 5, 8, 13, 21, 34, 55], 23)
    rowptr = np.concatenate([rowptr[:5], rowptr[4:]])                         # an empty row 4 among the nine
    assert len(rowptr) == 11 and rowptr[4] == rowptr[5]
    n, seed, slot0 = (1 << 24) + 1000, 31337, (1 << 32) - (1 << 23)           # the slots cross 2^32 in the middle
    assert n > 65536 * 256
    rp, rt, ng = _dev(gpu, rowptr, rating, neg)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    cdf = native.negative_cdf(rp, rt, 1.0, flag=flag)
    pick_h = np.random.default_rng(24).integers(0, 10, n)
    pick = torch.from_numpy(pick_h).to(gpu)
    out = torch.full((n,), -5, dtype=torch.int64, device=gpu)
    native.sample_negatives(rp, cdf, ng, pick, seed, slot0, out=out)
    with pytest.raises(IndexError):                                           # the picks of the empty row; clears the flag
        native.check_oob(gpu)
    want, bad = R.draw_ref(rowptr, cdf.cpu().numpy(), neg, pick_h, seed, slot0)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    assert bad and int(flag.item()) == 1 and (want != -5).all()


def test_a_draw_at_equality_lands_one_past_the_entry_and_a_short_cdf_clamps(gpu):
    """ncf_sample_negatives takes any CDF buffer.  Row 0: a sorted subset of the very u values of slots 0 .. 63, then 1.0.  Row 1
    ends at 0.5.  Row 2 is [0.0, 1.0], a leading zero weight."""
    from deeprecommendation_amd import native
    seed = ZERO_U[0]
    u = slot_uniform(seed, np.arange(64, dtype=np.uint64))
    row0 = R.equality_cdf(seed)
    row1 = np.array([0.125, 0.25, 0.5], dtype=np.float32)
    row2 = np.array([0.0, 1.0], dtype=np.float32)
    cdf = np.concatenate([row0, row1, row2])
    n0 = len(row0)
    rowptr = np.array([0, n0, n0 + 3, n0 + 5], dtype=np.int64)
    neg = np.arange(1000, 1000 + len(cdf), dtype=np.int32)
    pick_h = np.concatenate([np.zeros(64, dtype=np.int64), np.tile(np.array([1, 2], dtype=np.int64), 4096)])
    rp, cd, ng, pick = _dev(gpu, rowptr, cdf, neg, pick_h)
    out = native.sample_negatives(rp, cd, ng, pick, seed, 0).cpu().numpy()
    native.check_oob(gpu)                                                     # the clamp of row 1 leaves the flag clear
    want, bad = R.draw_ref(rowptr, cdf, neg, pick_h, seed, 0)
    assert not bad and np.array_equal(out, want)
    hits = 0
    for b in range(64):
        at = np.flatnonzero(row0 == u[b])
        if len(at):
            assert out[b] == 1000 + at[0] + 1
            hits += 1
    assert hits >= 16
    ub = slot_uniform(seed, np.arange(len(pick_h), dtype=np.uint64))
    on1, on2 = pick_h == 1, pick_h == 2
    assert (ub[on1] >= 0.5).sum() > 1000 and (out[on1 & (ub >= 0.5)] == 1000 + n0 + 2).all()
    assert (out[on2] == 1000 + n0 + 4).all()                                  # never entry 0 of [0.0, 1.0] ...
    seed0, slot = ZERO_U                                                      # ... not even at u == 0
    z = native.sample_negatives(rp, cd, ng, torch.tensor([2], device=gpu), seed0, slot).cpu().tolist()
    assert z == [1000 + n0 + 4]


def test_empty_rows_and_bad_picks_write_minus_one_beside_correct_neighbours(gpu):
    from deeprecommendation_amd import native
    rowptr, rating, neg, _ = R.rows_cycle(4, [3, 64, 5, 1], 25)
    rowptr = np.concatenate([rowptr[:2], rowptr[1:4], rowptr[3:]])            # rows 1 and 4 are empty
    rows = len(rowptr) - 1
    assert rows == 6 and np.diff(rowptr).tolist() == [3, 0, 64, 5, 0, 1]
    rp, rt, ng = _dev(gpu, rowptr, rating, neg)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    cdf = native.negative_cdf(rp, rt, 1.0, flag=flag)
    assert int(flag.item()) == 1                                              # the empty rows
    want_cdf, _ = R.cdf_exact(rating, rowptr)
    _assert_same_bits(cdf.cpu().numpy(), want_cdf, rowptr)
    pick_h = np.tile(np.array([0, 1, 2, -1, 3, rows, 5, 4, 2, 1 << 40, 0, -(1 << 40), 3], dtype=np.int64), 50)
    native.check_oob(gpu)
    out = native.sample_negatives(rp, cdf, ng, torch.from_numpy(pick_h).to(gpu), 7, 11).cpu().numpy()
    with pytest.raises(IndexError):                                           # clears the flag
        native.check_oob(gpu)
    want, bad = R.draw_ref(rowptr, cdf.cpu().numpy(), neg, pick_h, 7, 11)
    assert bad and np.array_equal(out, want)
    refused = np.isin(pick_h, [1, 4, -1, rows, 1 << 40, -(1 << 40)])
    assert (out[refused] == -1).all() and (out[~refused] >= 0).all()
    good = np.flatnonzero(~refused)                                           # the same picks alone leave the flag clear
    native.sample_negatives(rp, cdf, ng, torch.from_numpy(pick_h[good]).to(gpu), 7, 11)
    native.check_oob(gpu)


def test_cdf_and_draw_capture_into_one_graph(gpu):
    """No host synchronisation inside either call: one linear capture, replayed twice over poisoned buffers."""
    from deeprecommendation_amd import native
    rowptr, rating, neg, groups = R.rows_cycle(2000, CYCLE, 26)
    rp, rt, ng = _dev(gpu, rowptr, rating, neg)
    pick_h = np.random.default_rng(27).integers(0, 2000, 4096)
    pick = torch.from_numpy(pick_h).to(gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    seed, slot0 = 4242, 1 << 33

    def run():
        cdf = native.negative_cdf(rp, rt, 1.0, flag=flag)
        return cdf, native.sample_negatives(rp, cdf, ng, pick, seed, slot0)

    eager_cdf, eager_out = (t.cpu() for t in run())
    want_cdf, _ = R.cdf_exact(rating, rowptr, groups)
    _assert_same_bits(eager_cdf.numpy(), want_cdf, rowptr)
    want, bad = R.draw_ref(rowptr, want_cdf, neg, pick_h, seed, slot0)
    assert not bad and np.array_equal(eager_out.numpy(), want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                 # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cdf, out = run()
    for _ in range(2):
        cdf.fill_(-3.0)
        out.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cdf.cpu().view(torch.int32), eager_cdf.view(torch.int32))
        assert torch.equal(out.cpu(), eager_out)
    assert int(flag.item()) == 0
    native.check_oob(gpu)
