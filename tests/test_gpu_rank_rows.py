"""GPU: ncf_rank_rows (native.rank_rows) equals the numpy statement of the rank contract (rank_ref.rank_oracle), integer for
integer: one and many column tiles, one and many rows, a strided score matrix, every kind of target row (none, one, a full chunk,
the chunked forms, duplicates, excluded and out-of-range targets, the last column), every kind of exclusion list and of score row
(random, heavy ties, all zero, NaN / inf, all NaN)."""
import numpy as np
import pytest
import torch

from rank_ref import csr, rank_oracle, seen_rows, target_rows

pytestmark = pytest.mark.gpu


def _scores(R, C, pad, rng):
    """(R, C) view of an (R, C + pad) matrix; the kind of row r goes round: random, small integers, zeros, NaN / inf, all NaN."""
    s = rng.standard_normal((R, C + pad)).astype(np.float32)
    for r in range(R):
        kind = r % 5
        if kind == 1:
            s[r] = rng.integers(-3, 4, C + pad)
        elif kind == 2:
            s[r] = 0.0
            s[r, ::7] = -0.0
        elif kind == 3:
            s[r, rng.random(C + pad) < 0.2] = np.nan
            s[r, rng.random(C + pad) < 0.1] = np.inf
            s[r, rng.random(C + pad) < 0.1] = -np.inf
        elif kind == 4:
            s[r] = np.nan
    return s


@pytest.mark.parametrize("C", [1, 100, 8191, 8192, 8193, 20000])
@pytest.mark.parametrize("R", [1, 3, 70])
def test_rank_rows_equals_the_oracle(gpu, C, R):
    from deeprecommendation_amd import native
    cap = native.RANK_MAX_TARGETS
    rng = np.random.default_rng(C * 131 + R)
    shifts = range(10) if R == 1 else range(0, 9, 3) if R == 3 else (0,)      # few rows: go round the row kinds call by call
    for shift in shifts:
        pad = (0, 3, 4)[(C + shift) % 3]                                      # leading dimension: C, unaligned rows, aligned rows
        host = np.roll(_scores(max(R, 5), C, pad, rng), -shift, axis=0)[:R]
        seen = seen_rows(R, C, rng, shift)
        targets = target_rows(R, C, cap, rng, seen, shift)
        scores = torch.from_numpy(host).to(gpu)[:, :C]
        assert scores.stride(0) == C + pad
        for sl in (seen, None):
            rank, ranked = native.rank_rows(scores, csr(targets, gpu), None if sl is None else csr(sl, gpu))
            ref_rank, ref_ranked = rank_oracle(host[:, :C], sl, targets)
            assert rank.dtype == torch.int32 and ranked.dtype == torch.int32
            assert torch.equal(ranked.cpu(), ref_ranked)
            assert torch.equal(rank.cpu(), ref_rank)


def test_rank_rows_blocks_share_one_rank_array(gpu):
    """A slice of the row pointer ranks a block of rows against the whole col / rank arrays and leaves the other rows' entries alone."""
    from deeprecommendation_amd import native
    rng = np.random.default_rng(1)
    R, C = 9, 9000
    host = _scores(R, C, 0, rng)
    seen = seen_rows(R, C, rng)
    targets = target_rows(R, C, native.RANK_MAX_TARGETS, rng, seen)
    scores = torch.from_numpy(host).to(gpu)
    (trow, tcol), (srow, scol) = csr(targets, gpu), csr(seen, gpu)
    rank = torch.full((tcol.numel(),), 77, dtype=torch.int32, device=gpu)
    ref_rank, ref_ranked = rank_oracle(host, seen, targets)
    rk, ranked = native.rank_rows(scores[3:7], (trow[3:8], tcol), (srow[3:8], scol), rank=rank)
    assert rk is rank and torch.equal(ranked.cpu(), ref_ranked[3:7])
    lo, hi = int(trow[3]), int(trow[7])
    assert torch.equal(rank[lo:hi].cpu(), ref_rank[lo:hi]) and bool((rank[:lo] == 77).all()) and bool((rank[hi:] == 77).all())
    native.rank_rows(scores[:3], (trow[:4], tcol), (srow[:4], scol), rank=rank)
    native.rank_rows(scores[7:], (trow[7:], tcol), (srow[7:], scol), rank=rank)
    assert torch.equal(rank.cpu(), ref_rank)


def test_rank_rows_refuses_without_launching(gpu):
    from deeprecommendation_amd import native
    s = torch.zeros(2, 10, device=gpu)
    with pytest.raises(TypeError):
        native.rank_rows(s.double(), csr([[0], [1]], gpu))
    with pytest.raises(ValueError):
        native.rank_rows(s, csr([[0]], gpu))                                  # one row of targets for two score rows
    with pytest.raises(RuntimeError, match="GPU"):
        native.rank_rows(s.cpu(), csr([[0], [1]], "cpu"))
    rank, ranked = native.rank_rows(s, csr([[], []], gpu))                    # no targets at all: ranked alone
    assert rank.numel() == 0 and ranked.tolist() == [10, 10]
