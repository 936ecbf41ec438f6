"""GPU tests of the negative-sampling kernels (csrc/negsample.hip): ncf_negative_cdf against a float64 numpy CDF, and
ncf_sample_negatives against numpy's searchsorted over the kernel's CDF with u restated from include/ncf_abi.h's hash,
against the reference's probabilities, and on its refusals and flags."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 300, 4097, 20000]
W_SCHEDULE = [0.0, 0.5, 1.0, 1.5, 3.0]


def _lowbias32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def slot_uniform(seed, slots):
    """u of include/ncf_abi.h (ncf_sample_negatives), in numpy."""
    s = np.asarray(slots, dtype=np.uint64)
    lo, hi = (s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = _lowbias32((lo * np.uint32(0x9E3779B1)) ^ np.uint32(seed))
        x = _lowbias32(x ^ (hi * np.uint32(0x85EBCA77)) ^ np.uint32(0x68E31DA4))
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


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
