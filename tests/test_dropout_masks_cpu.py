"""CPU tests of the restated dropout mask (tests/dropout_mask_ref.py; the contract is include/ncf_abi.h, "THE MASK"): before a kernel
is held to the restatement element by element (tests/test_gpu_dropout_masks.py), the restatement itself is shown to be a sound
Bernoulli(1 - p') mask — frequencies and pair frequencies on a FIXED grid, each within 6 standard deviations of its binomial
expectation (the bar tests/test_gpu_negative_sampling.py uses for frequencies) — and to quantise p the way the library does."""
import numpy as np
import pytest

from dropout_mask_ref import keep_mask, mask_factor64, p_quantised, scale32, threshold

N_ENTRIES = 120_000
SEEDS = [0, 1, 1234, 2 ** 31 - 2, 2 ** 32 - 1]
PS = [0.1, 0.2, 0.5, 0.9]
CHUNKS = [1, 8, 32, 64]
SIGMAS = 6.0


def _z(count, n, q):
    """Standard score(s) of ``count`` successes in ``n`` Bernoulli(q) trials."""
    return np.abs(np.asarray(count, dtype=np.float64) - n * q) / np.sqrt(n * q * (1.0 - q))


@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("p", PS)
def test_kept_fractions_and_neighbour_pairs_are_binomial(p, chunks):
    """Kept fraction overall and per feature column, and the joint keep rate of neighbouring features and of neighbouring entries, under
    q = 1 - p'.  Pairs are taken DISJOINT (features (2j, 2j+1) and, separately, (2j+1, 2j+2); entries (2k, 2k+1) and (2k+1, 2k+2)), so
    that each count is a sum of independent Bernoulli(q^2) trials under the null and the binomial sigma is the right one; the odd
    tilings cover the pairs that straddle the two 16-bit halves of a hash word, the two words h0 / h1 and two chunks."""
    F = 4 * chunks
    q = 1.0 - p_quantised(p)
    worst = 0.0
    for seed in SEEDS:
        m = keep_mask(seed, np.arange(N_ENTRIES), F, p)
        stats = [_z(m.sum(), m.size, q), _z(m.sum(axis=0), N_ENTRIES, q).max()]
        for off in (0, 1):                                             # neighbouring features of one entry
            a, b = m[:, off:F - 1:2], m[:, off + 1:F:2]
            both = a & b
            stats.append(_z(both.sum(), both.size, q * q))
            stats.append(_z(both.sum(axis=0), N_ENTRIES, q * q).max())
        for off in (0, 1):                                             # the same feature of neighbouring entries
            a, b = m[off:N_ENTRIES - 1:2], m[off + 1:N_ENTRIES:2]
            both = a & b
            stats.append(_z(both.sum(), both.size, q * q))
            stats.append(_z(both.sum(axis=0), both.shape[0], q * q).max())
        worst = max(worst, max(float(s) for s in stats))
        assert max(float(s) for s in stats) <= SIGMAS, (seed, p, chunks, [round(float(s), 2) for s in stats])
    print(f"p={p} chunks={chunks}: worst statistic {worst:.2f} sigma")


def test_threshold_quantisation_follows_the_fp32_arithmetic_of_the_library():
    assert {p: threshold(p) for p in (0.1, 0.2, 0.3, 0.5)} == {0.1: 6554, 0.2: 13107, 0.3: 19661, 0.5: 32768}
    assert scale32(0.5) == np.float32(2.0) and scale32(0.5).dtype == np.float32
    assert scale32(0.1) == np.float32(65536.0) / np.float32(58982.0)
    # a half rounds UP (x + 0.5 truncated), where Python's round goes to the even neighbour
    assert threshold(2.5 / 65536) == 3 and round(2.5) == 2
    assert threshold(0.5 / 65536) == 1 and round(0.5) == 0
    # p so small that thr = 0: the mask is all ones and the scale exactly 1 (the library then runs the plain kernel)
    for p in (0.0, 1e-6, 7.6e-6):
        assert threshold(p) == 0 and float(scale32(p)) == 1.0
        assert keep_mask(99, np.arange(1000), 256, p).all()
        assert float(mask_factor64(99, np.arange(10), 8, p).min()) == 1.0
    assert threshold(2.0 ** -17) == 1
    # p just below 1: p * 65536 + 0.5 rounds to 65536 in fp32, the clamp gives 65535, and the scale is finite
    top = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert threshold(top) == 65535 and float(scale32(top)) == 65536.0 and np.isfinite(scale32(top))
    assert threshold(0.99999) == 65535
    m = keep_mask(5, np.arange(200_000), 4, top)                       # keep probability 2^-16: a handful survive, scaled by 65536
    assert 0 <= int(m.sum()) < 60
    f = mask_factor64(5, np.arange(200_000), 4, top)
    assert set(np.unique(f.numpy()).tolist()) <= {0.0, 65536.0}


def test_mask_factor_is_scale_where_kept_and_zero_elsewhere():
    for p in (0.1, 0.3, 0.5):
        k = keep_mask(7, np.arange(5000), 36, p)
        f = mask_factor64(7, np.arange(5000), 36, p).numpy()
        assert f.shape == (5000, 36) and f.dtype == np.float64
        assert np.array_equal(f != 0, k) and np.all(f[k] == float(scale32(p)))
        # 1 / (1 - p') in fp32, which is not 1 / (1 - p)
        assert abs(float(scale32(p)) - 1.0 / (1.0 - p_quantised(p))) <= 2.0 ** -23 * float(scale32(p))
    assert float(scale32(0.1)) != float(np.float32(1.0) / np.float32(0.9))


def test_features_beyond_a_chunk_boundary_are_a_prefix_of_the_wider_mask():
    """Feature f depends on (entry, f // 4, f % 4) alone: a narrower call sees a prefix of a wider one's mask (D = 36 vs 256)."""
    wide = keep_mask(1234, np.arange(3000), 256, 0.3)
    for F in (4, 36, 100, 132):
        assert np.array_equal(keep_mask(1234, np.arange(3000), F, 0.3), wide[:, :F])


def test_entries_2_pow_32_apart_share_their_mask():
    e = np.array([0, 1, 77, 2 ** 31 - 1, 2 ** 32 - 1], dtype=np.int64)
    for seed in (0, 4242):
        a = keep_mask(seed, e, 64, 0.3)
        assert np.array_equal(a, keep_mask(seed, e + 2 ** 32, 64, 0.3))
        assert np.array_equal(a, keep_mask(seed, e + 5 * 2 ** 32, 64, 0.3))
    assert np.array_equal(keep_mask(3, np.array([-1]), 64, 0.3), keep_mask(3, np.array([2 ** 32 - 1]), 64, 0.3))
    assert not np.array_equal(keep_mask(3, e, 64, 0.3), keep_mask(3, e + 1, 64, 0.3))
    assert np.array_equal(keep_mask(3 + 2 ** 32, e, 64, 0.3), keep_mask(3, e, 64, 0.3))        # the seed is a uint32 too


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_layer_seeds_of_graph_ncf_give_independent_masks(p):
    """GraphNCF draws seed0 per step and uses seed0 + 7919 * layer: the masks of two layers must differ, and agree as often as
    two independent Bernoulli(q) masks do, q^2 + (1 - q)^2, within 6 sigma — overall and per feature column."""
    q = 1.0 - p_quantised(p)
    agree_p = q * q + (1.0 - q) * (1.0 - q)
    for seed0 in (0, 1234, 2 ** 31 - 2):
        for D in (32, 128):
            a = keep_mask(seed0, np.arange(N_ENTRIES), D, p)
            for layer in (1, 2):
                b = keep_mask(seed0 + 7919 * layer, np.arange(N_ENTRIES), D, p)
                assert not np.array_equal(a, b)
                same = a == b
                assert float(_z(same.sum(), same.size, agree_p)) <= SIGMAS, (seed0, D, layer)
                assert float(_z(same.sum(axis=0), N_ENTRIES, agree_p).max()) <= SIGMAS, (seed0, D, layer)
