"""CPU tests of tests/negsample_ref.py, the numpy statement of include/ncf_abi.h's negative-sampling contract: the properties the
header promises for every row, the derived distance from the float64 probabilities, the clamp, the 512 / 513 boundary, the
flagged kinds, the draw at equality and the uniform's grid.  The GPU tests (tests/test_gpu_negative_sampling.py) hold the
kernels to these references bit for bit."""
import numpy as np
import pytest

import negsample_ref as R

LENGTHS = [1, 2, 63, 64, 65, 511, 512, 513, 576, 577, 1025, 4097, 70000]
ONE = np.float32(1.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def cycle():
    """Three rows of every length, and the exact CDF at w = 0 and w = 1, computed once."""
    rowptr, rating, neg, groups = R.rows_cycle(3 * len(LENGTHS), LENGTHS, 11)
    cdf = {w: R.cdf_exact(R.weights(rating, w), rowptr, groups) for w in (0, 1)}
    return rowptr, rating, cdf


def test_rows_cycle_has_the_lengths_the_domain_and_its_groups():
    rowptr, rating, neg, groups = R.rows_cycle(3 * len(LENGTHS) + 2, LENGTHS, 11)
    lens = np.diff(rowptr)
    assert lens.tolist() == [LENGTHS[r % len(LENGTHS)] for r in range(len(lens))]
    assert rating.dtype == np.float32 and neg.dtype == np.int32 and len(rating) == len(neg) == rowptr[-1]
    assert set(np.unique(rating).tolist()) <= set((np.arange(11) * 0.5).tolist())
    assert sorted(groups) == sorted(LENGTHS)
    for n, rows in groups.items():
        assert (lens[rows] == n).all() and len(rows) == (lens == n).sum()
    for r in range(len(lens)):
        row = rating[rowptr[r]:rowptr[r + 1]]
        assert row.max() > 0
        if len(row) >= 3:
            assert row[0] == 0 and row[-1] == 0


@pytest.mark.parametrize("w", [0, 1])
def test_every_row_ends_in_one_is_monotone_and_a_zero_weight_repeats_its_predecessor(cycle, w):
    rowptr, rating, cdf = cycle
    got, flag = cdf[w]
    assert got.dtype == np.float32 and not flag
    wt = R.weights(rating, w)
    for r in range(len(rowptr) - 1):
        s, e = rowptr[r], rowptr[r + 1]
        row = got[s:e]
        assert row[-1] == ONE and _bits(row[-1:])[0] == 0x3F800000
        assert (np.diff(row) >= 0).all()
        zero = np.flatnonzero(wt[s:e] == 0)
        assert w == 0 or len(row) < 3 or len(zero) >= 2                       # the property below is not vacuous
        lead, inner = zero[zero == 0], zero[zero > 0]
        assert (_bits(row[lead]) == 0).all()                                  # a leading zero weight: 0.0f
        assert (_bits(row[inner]) == _bits(row[inner - 1])).all()


@pytest.mark.parametrize("w", [0, 1])
def test_distance_from_the_float64_cumsum_is_at_most_2_to_the_minus_24(cycle, w):
    """Derived, not measured: rounding a value <= 1 to fp32 costs at most 2^-25; the fixed point errs by at most len * 2^-S of the
    largest weight (2^-29 at 70000 entries, S = 45); the float64 cumsum itself by about len * 2^-53."""
    rowptr, rating, cdf = cycle
    ref = R.cdf_float64(R.weights(rating, w), rowptr)
    err = float(np.abs(cdf[w][0].astype(np.float64) - ref).max())
    print(f"w = {w}: max |cdf_exact - float64| = {err:.3e}")
    assert err <= 2.0 ** -24


def test_cdf_float64_is_the_plain_cumsum_over_the_sum():
    rowptr, rating, _, _ = R.rows_cycle(7, [1, 5, 64], 3)
    ref = R.cdf_float64(R.weights(rating, 1.5), rowptr)
    for r in range(7):
        wt = rating[rowptr[r]:rowptr[r + 1]].astype(np.float64) ** 1.5
        assert np.array_equal(ref[rowptr[r]:rowptr[r + 1]], np.cumsum(wt) / np.cumsum(wt)[-1])
        assert np.abs(ref[rowptr[r]:rowptr[r + 1]] - np.cumsum(wt) / wt.sum()).max() <= 1e-15


def test_weights_are_ones_the_ratings_themselves_or_a_float64_power():
    r = np.array([0.0, 0.5, 3.5, 5.0, 1e-20], dtype=np.float32)
    assert R.weights(r, 0).dtype == np.float32 and (R.weights(r, 0) == 1).all()
    assert R.weights(r, 1).dtype == np.float32 and np.array_equal(_bits(R.weights(r, 1)), _bits(r))
    assert np.array_equal(_bits(r ** np.float32(1.0)), _bits(r))              # numpy's r ** 1.0 is r
    assert R.weights(r, 1.5).dtype == np.float64 and np.array_equal(R.weights(r, 1.5), r.astype(np.float64) ** 1.5)


def test_a_positive_weight_never_quantises_below_one_unit():
    """[1e-20, 5, 1e-20, 0, 2.5]: len 5 has bit length 3, S = 59, scale = 2^59 / 5; 1e-20 * scale = 1.15e-3 rounds to 0 and is
    raised to 1.  total = 2^59 + 2^58 + 2, first prefix = 1 / total = 1.16e-18, and entries 1 to 3 share (2^59 + 1 | 2 | 2) /
    total, which differ far below fp32's resolution."""
    wt = np.array([1e-20, 5.0, 1e-20, 0.0, 2.5], dtype=np.float32)
    cdf, flag = R.cdf_exact(wt, [0, 5])
    total = 2 ** 59 + 2 ** 58 + 2
    assert not flag
    assert cdf[0] > 0 and cdf[0] == np.float32(1.0 / total) and abs(float(cdf[0]) - 1.16e-18) < 1e-20
    assert _bits(cdf[1]) == _bits(cdf[2]) == _bits(cdf[3]) == _bits(np.float32((2 ** 59 + 1) / total))
    assert cdf[4] == ONE
    # without the clamp the first prefix would be 0.0f and entry 0 could never be drawn at u == 0
    assert np.searchsorted(cdf, np.float32(0.0), side="right") == 0


def test_a_row_mixing_magnitudes_keeps_every_positive_weight_drawable():
    """[1e-30, 1, 1e19]: S = 60, 1 * 2^60 / 1e19 = 0.115 and 1e-30's share both clamp to one unit against 2^60."""
    wt = np.array([1e-30, 1.0, 1e19], dtype=np.float32)
    cdf, flag = R.cdf_exact(wt, [0, 3])
    total = 2 ** 60 + 2
    assert not flag and cdf[2] == ONE
    assert cdf[0] == np.float32(1.0 / total) and cdf[1] == np.float32(2.0 / total) and 0 < cdf[0] < cdf[1]


def test_a_zero_weight_appended_to_512_entries_keeps_the_first_512_prefixes():
    """512 and 513 share the bit length 10, so S, the scale, every q and the total are the same; the 513th prefix is total / total."""
    rowptr, rating, _, _ = R.rows_cycle(1, [512], 5)
    twin = np.concatenate([rating, np.zeros(1, dtype=np.float32)])
    assert (512).bit_length() == (513).bit_length()
    a, fa = R.cdf_exact(rating, rowptr)
    b, fb = R.cdf_exact(twin, [0, 513])
    assert not fa and not fb
    assert np.array_equal(_bits(b[:512]), _bits(a))
    assert _bits(b[512:])[0] == 0x3F800000


@pytest.mark.parametrize("kind", R.FLAGGED_KINDS)
@pytest.mark.parametrize("n", [1, 2, 65, 513])
def test_the_flagged_kinds_give_the_exact_uniform_prefix_and_the_flag(kind, n):
    """Beside a good row, which stays what it is alone."""
    good = np.array([0.0, 3.5, 1.0], dtype=np.float32)
    bad = R.flagged_row(kind, n)
    assert len(bad) == (0 if kind == "empty" else n)
    rowptr = np.array([0, 3, 3 + len(bad), 6 + len(bad)], dtype=np.int64)
    cdf, flag = R.cdf_exact(np.concatenate([good, bad, good]), rowptr)
    assert flag is True
    want = (np.arange(1, len(bad) + 1, dtype=np.float64) / max(len(bad), 1)).astype(np.float32)
    assert np.array_equal(_bits(cdf[3:3 + len(bad)]), _bits(want))
    assert np.array_equal(_bits(R.uniform_prefix(len(bad))), _bits(want))
    alone, f = R.cdf_exact(good, [0, 3])
    assert not f and np.array_equal(_bits(cdf[:3]), _bits(alone)) and np.array_equal(_bits(cdf[3 + len(bad):]), _bits(alone))
    with np.errstate(over="ignore", invalid="ignore"):                       # flagged in any order of summation
        for order in (bad, bad[::-1], np.sort(bad), np.roll(bad, 1)):
            s = np.float32(0)
            for v in order:
                s = np.float32(s + v)
            assert not (np.isfinite(s) and s > 0)


def test_rows_cycle_flagged_swaps_every_seventh_row_through_the_four_kinds():
    lengths = [1, 2, 63, 64, 65, 511, 512, 513, 576, 577, 1025]
    rowptr, rating, neg, kind = R.rows_cycle_flagged(700, lengths, 9)
    lens = np.diff(rowptr)
    assert (np.flatnonzero(kind >= 0) == np.arange(0, 700, 7)).all()
    assert kind[::7].tolist() == [k % 4 for k in range(100)]
    assert (lens[kind == 3] == 0).all() and (lens[kind != 3] == np.asarray(lengths)[np.flatnonzero(kind != 3) % 11]).all()
    for k in range(3):                                                        # every kind meets every length
        assert set(lens[kind == k].tolist()) == set(lengths)
    assert np.isnan(rating).sum() == (kind == 1).sum()
    cdf, flag = R.cdf_exact(rating, rowptr)
    assert flag
    for r in range(700):
        row = cdf[rowptr[r]:rowptr[r + 1]]
        if kind[r] >= 0:
            assert np.array_equal(_bits(row), _bits(R.uniform_prefix(len(row))))
        else:
            assert row[-1] == ONE and (np.diff(row) >= 0).all()


def test_a_draw_at_equality_takes_the_entry_after_it():
    seed = 2024
    u = R.slot_uniform(seed, np.arange(64, dtype=np.uint64))
    cdf = R.equality_cdf(seed)
    n = len(cdf)
    assert n >= 16 and cdf[-1] == ONE and (np.diff(cdf) > 0).all()
    rowptr = np.array([0, n], dtype=np.int64)
    neg = np.arange(100, 100 + n, dtype=np.int32)
    out, flag = R.draw_ref(rowptr, cdf, neg, np.zeros(64, dtype=np.int64), seed, 0)
    assert not flag
    hits = 0
    for b in range(64):
        at = np.flatnonzero(cdf == u[b])
        if len(at):                                                           # u is entry at[0], bit for bit: one past it
            assert out[b] == 100 + at[0] + 1
            hits += 1
        assert out[b] == 100 + int((cdf <= u[b]).sum())                       # the number of entries <= u
    assert hits >= 16


def test_draw_ref_clamps_to_the_last_entry_refuses_bad_picks_and_offsets_slots():
    rowptr = np.array([0, 2, 2, 5], dtype=np.int64)                           # row 1 is empty
    cdf = np.array([0.25, 0.5, 0.0, 0.5, 1.0], dtype=np.float32)              # row 0 ends at 0.5: the clamp
    neg = np.array([10, 11, 20, 21, 22], dtype=np.int32)
    pick = np.array([0, 1, 2, -1, 3, 0, 2] * 40, dtype=np.int64)
    seed, slot0 = 5, (1 << 32) - 100                                          # slots cross 2^32
    out, flag = R.draw_ref(rowptr, cdf, neg, pick, seed, slot0)
    u = R.slot_uniform(seed, slot0 + np.arange(len(pick), dtype=np.uint64))
    assert flag and out.dtype == np.int64
    seen = set()
    for b, r in enumerate(pick):
        if r == 0:
            assert out[b] == (10 if u[b] < 0.25 else 11)                      # u >= 0.5 stays on the last entry
            seen.add(("row0", u[b] >= 0.5))
        elif r == 2:
            assert out[b] == (21 if u[b] < 0.5 else 22)                       # the leading zero weight is never drawn
        else:
            assert out[b] == -1
    assert seen == {("row0", True), ("row0", False)}
    good, flag = R.draw_ref(rowptr, cdf, neg, np.array([0, 2, 2], dtype=np.int64), seed, 0)
    assert not flag and (good >= 0).all()
    assert not np.array_equal(u[:64], R.slot_uniform(seed, np.arange(64, dtype=np.uint64)))   # the high word enters the hash


@pytest.mark.parametrize("n_rows", [40, 200])                                   # draw_ref's two ways of grouping picks by row
def test_draw_ref_equals_one_searchsorted_per_pick(n_rows):
    rowptr, rating, neg, kind = R.rows_cycle_flagged(n_rows, [1, 2, 5, 63, 64, 65], 4)          # empty rows among them
    cdf, _ = R.cdf_exact(rating, rowptr)
    pick = np.random.default_rng(6).integers(-2, n_rows + 2, 3000)
    seed, slot0 = 99, 12345
    out, flag = R.draw_ref(rowptr, cdf, neg, pick, seed, slot0)
    u = R.slot_uniform(seed, slot0 + np.arange(len(pick), dtype=np.uint64))
    bad = 0
    for b, r in enumerate(pick):
        s, e = (rowptr[r], rowptr[r + 1]) if 0 <= r < n_rows else (0, 0)
        if e == s:
            assert out[b] == -1
            bad += 1
        else:
            assert out[b] == neg[s + min(np.searchsorted(cdf[s:e], u[b], side="right"), e - s - 1)]
    assert flag and 0 < bad < len(pick) / 2


def test_slot_uniform_is_a_24_bit_multiple_of_2_to_the_minus_24_in_the_unit_interval():
    slots = np.concatenate([np.arange(1 << 16, dtype=np.uint64), (1 << 32) - 500 + np.arange(1000, dtype=np.uint64),
                            np.array([2 ** 63 - 1], dtype=np.uint64)])
    for seed in (0, 1, 0xFFFFFFFF, 987654321):
        u = R.slot_uniform(seed, slots)
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
        k = u.astype(np.float64) * 2.0 ** 24
        assert (k == np.rint(k)).all() and (k < 2 ** 24).all()
        assert len(np.unique(u)) > 0.99 * len(u)


def test_the_known_slot_of_u_equal_to_zero():
    """tests/test_gpu_negative_sampling.py draws at it: u == 0 is below every positive prefix and equal to a leading 0.0f."""
    assert R.slot_uniform(2024, [2623355, 2623356, 2623357]).tolist()[1] == 0.0
    assert (R.slot_uniform(2024, [2623355, 2623357]) > 0).all()


def test_slot_uniform_equals_the_header_formula_in_python_integers():
    M = 0xFFFFFFFF

    def mix(x):
        x ^= x >> 16
        x = x * 0x7feb352d & M
        x ^= x >> 15
        x = x * 0x846ca68b & M
        return x ^ x >> 16

    seed = 987654321
    slots = [0, 1, 63, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 12345]
    want = []
    for s in slots:
        x = mix(((s & M) * 0x9E3779B1 & M) ^ seed)
        x = mix(x ^ ((s >> 32) * 0x85EBCA77 & M) ^ 0x68E31DA4)
        want.append((x >> 8) / 2.0 ** 24)
    assert R.slot_uniform(seed, np.array(slots, dtype=np.uint64)).tolist() == want
