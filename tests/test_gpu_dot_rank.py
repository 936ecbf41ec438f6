"""GPU: ncf_dot_rank (native.dot_rank) equals native.rank_rows over native.gather_dot's all-pairs score matrix, integer for integer:
every width class (every MFMA step count, the scalar load path, a strided table with ld % 4 != 0), one and many user blocks and
column tiles, with and without an item id list, max_targets 1 / 2 / 16 / the cap with every kind of target row, exclusion lists;
exact ties, zero rows, NaN / inf; the overflow flag; bad ids set the out-of-range flag; a captured call replays to the same
answer."""
import numpy as np
import pytest
import torch

from rank_ref import csr, seen_rows, target_rows

pytestmark = pytest.mark.gpu

DS = [1, 15, 16, 64, 100, 256]
BS = [1, 16, 17, 65, 130]
IS = [1, 15, 2047, 2049, 8193, 20000]
CAP = 128
MTS = [1, 2, 16, CAP]


def _rand(rows, D, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(rows, D, device=dev, generator=g)


def _reference(A, ia, B, ib, targets, seen):
    from deeprecommendation_amd import native
    rows = ia if ia is not None else torch.arange(A.shape[0], device=A.device)
    cols = ib if ib is not None else torch.arange(B.shape[0], device=A.device)
    nu, ni = rows.numel(), cols.numel()
    s = native.gather_dot(A, rows.repeat_interleave(ni), B, cols.repeat(nu)).view(nu, ni)
    return native.rank_rows(s, targets, seen)


def _check(A, ia, B, ib, targets, max_targets, seen=None):
    from deeprecommendation_amd import native
    got = native.dot_rank(A, ia, B, ib, targets, max_targets, seen)
    ref = _reference(A, ia, B, ib, targets, seen)
    torch.cuda.synchronize()
    assert torch.equal(got[1], ref[1])
    assert torch.equal(got[0], ref[0])
    return got


def _case(gpu, D, nB, I, mt, seed):
    """nB users (an id list into a larger table) x I columns, with and without an item id list (with repeats), with and without
    exclusion lists, target rows of every kind that fits max_targets = mt; the user table is a strided view when D % 4 != 0."""
    from deeprecommendation_amd import native
    rng = np.random.default_rng(seed)
    A = _rand(nB + 20, D + 3, seed, gpu)[:, :D] if D % 4 else _rand(nB + 20, D, seed, gpu)
    T = _rand(I + 10, D, seed + 1, gpu)
    g = torch.Generator(device=gpu).manual_seed(seed)
    ia = torch.randint(0, nB + 20, (nB,), device=gpu, generator=g)
    for ib in (None, torch.randint(0, I + 10, (I,), device=gpu, generator=g)):
        C = I if ib is not None else I + 10
        for with_seen in (True, False):
            seen = seen_rows(nB, C, rng, seed) if with_seen else None
            targets = target_rows(nB, C, mt, rng, seen, seed, big=False)
            _check(A, ia, T, ib, csr(targets, gpu), mt, None if seen is None else csr(seen, gpu))
    native.check_rank_overflow(gpu)                              # no row above max_targets: the flag stays clear
    native.check_oob(gpu)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mt", MTS)
def test_dot_rank_widths_and_max_targets(gpu, D, mt):
    n = DS.index(D) * len(MTS) + MTS.index(mt)
    _case(gpu, D, BS[n % len(BS)], IS[(n * 5 + 1) % len(IS)], mt, 1000 + n)


@pytest.mark.parametrize("nB", BS)
@pytest.mark.parametrize("I", IS)
def test_dot_rank_user_blocks_and_column_tiles(gpu, nB, I):
    n = BS.index(nB) * len(IS) + IS.index(I)
    _case(gpu, DS[n % len(DS)], nB, I, MTS[(n // 2) % len(MTS)], 2000 + n)


def test_dot_rank_overflow_flag(gpu):
    from deeprecommendation_amd import native
    A, T = _rand(5, 64, 1, gpu), _rand(3000, 64, 2, gpu)
    native.check_rank_overflow(gpu)                              # start clean
    rng = np.random.default_rng(0)
    for mt in (1, 16, CAP):
        lists = [rng.integers(0, 3000, n).tolist() for n in (mt, 0, mt + 1, 1, mt)]
        targets = csr(lists, gpu)
        rank, ranked = native.dot_rank(A, None, T, None, targets, mt)
        ref, ref_ranked = _reference(A, None, T, None, targets, None)
        with pytest.raises(OverflowError):
            native.check_rank_overflow(gpu)
        native.check_rank_overflow(gpu)                          # reading it cleared it
        # the row above max_targets has its first max_targets entries ranked, the one beyond is -1; every other row is exact
        lo = int(targets[0][2])
        keep = torch.ones_like(rank, dtype=torch.bool)
        keep[lo + mt] = False
        assert int(rank[lo + mt]) == -1 and torch.equal(rank[keep], ref[keep]) and torch.equal(ranked, ref_ranked)


def test_dot_rank_ties_zero_rows_and_specials(gpu):
    D, I = 64, 10000
    rng = np.random.default_rng(3)
    base = _rand(40, D, 7, gpu)
    T = base[torch.randint(0, 40, (I,), device=gpu)].contiguous()            # duplicated rows: exact ties, lower column first
    A = _rand(20, D, 8, gpu)
    A[3] = 0.0                                                                # every score +0: ranked by column
    seen = seen_rows(20, I, rng)
    for mt in (1, 16):
        targets = target_rows(20, I, mt, rng, seen, big=False)
        targets[3] = [4321][:mt]
        rank, _ = _check(A, None, T, None, csr(targets, gpu), mt)
        assert int(rank[int(csr(targets, "cpu")[0][3])]) == 4321
        _check(A, None, T, None, csr(targets, gpu), mt, csr(seen, gpu))
        Ti = torch.randint(-3, 4, (I, D), device=gpu).float()                 # small integers: exact sums, heavy ties
        Ai = torch.randint(-3, 4, (20, D), device=gpu).float()
        _check(Ai, None, Ti, None, csr(targets, gpu), mt, csr(seen, gpu))
        # NaN / inf in either table, as a short list and as the whole table; an all-NaN row
        Ts = T.clone()
        Ts[5, 3] = float("nan")
        Ts[17, 0] = float("inf")
        Ts[18, :] = float("-inf")
        Ts[19, 0], Ts[19, 1] = float("inf"), float("-inf")
        As = A.clone()
        As[4, 0] = float("inf")
        As[0, 0] = float("nan")
        ib = torch.tensor([5, 17, 18, 19, 0, 1, 2, 3, 4, 6], device=gpu)
        short = [[int(x) for x in rng.integers(0, 10, mt)] for _ in range(20)]
        _check(As, None, Ts, ib, csr(short, gpu), mt)
        _check(As, None, Ts, None, csr(targets, gpu), mt, csr(seen, gpu))
        rank, ranked = _check(As[:1], None, T, None, csr([[I - 1][:mt]], gpu), mt)
        assert rank.tolist() == [I - 1] and ranked.tolist() == [I]            # all NaN: by column


def test_dot_rank_bad_ids_set_the_flag(gpu):
    from deeprecommendation_amd import native
    A, T = _rand(10, 64, 0, gpu), _rand(500, 64, 1, gpu)
    native.check_oob(gpu)                                       # start clean
    native.dot_rank(A, torch.tensor([0, 10], device=gpu), T, None, csr([[1], [2]], gpu), 1)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.dot_rank(A, None, T, torch.tensor([3, -1, 2], device=gpu), csr([[0]] * 10, gpu), 1)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.dot_rank(A, None, T, None, csr([[499]] * 10, gpu), 1)
    native.check_oob(gpu)                                       # good ids leave it clear


def test_dot_rank_refusals_launch_nothing(gpu):
    from deeprecommendation_amd import native
    A, T, Tw = _rand(4, 64, 0, gpu), _rand(100, 64, 1, gpu), _rand(100, 300, 1, gpu)
    targets = csr([[1], [2], [3], [4]], gpu)
    rank = torch.full((4,), 7, dtype=torch.int32, device=gpu)
    for args, code in (((A, None, T, None, targets, 0), native.NCF_EINVAL), ((A, None, T, None, targets, CAP + 1), native.NCF_EUNSUPPORTED),
                       ((Tw[:4], None, Tw, None, targets, 1), native.NCF_EUNSUPPORTED)):
        with pytest.raises(native.NativeError) as e:
            native.dot_rank(*args, rank=rank)
        assert e.value.code == code
    torch.cuda.synchronize()
    assert bool((rank == 7).all())
    with pytest.raises(RuntimeError, match="GPU"):
        native.dot_rank(A.cpu(), None, T.cpu(), None, csr([[1]] * 4, "cpu"), 1)


@pytest.mark.parametrize("mt", [1, 16])
def test_dot_rank_captures_into_a_graph(gpu, mt):
    """One capture on a single stream (no parallel branches), replayed twice: the outputs are initialised inside the captured
    sequence, so every replay gives the eager call's answer."""
    from deeprecommendation_amd import native
    A, T = _rand(100, 64, 11, gpu), _rand(30000, 64, 12, gpu)
    rng = np.random.default_rng(mt)
    seen = csr([list(range(r, 30000, 97)) for r in range(100)], gpu)
    targets = csr([rng.integers(0, 30000, int(rng.integers(0, mt + 1))).tolist() for _ in range(100)], gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = native.dot_rank(A, None, T, None, targets, mt, seen)      # warm-up outside the capture (library load, allocator)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = native.dot_rank(A, None, T, None, targets, mt, seen)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    ref = _reference(A, None, T, None, targets, seen)
    assert torch.equal(eager[0], ref[0]) and torch.equal(eager[1], ref[1])
