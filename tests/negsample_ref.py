"""The contract of the negative-sampling kernels (csrc/negsample.hip, stated in include/ncf_abi.h) in numpy, exact.  No GPU
needed.  The CPU tests (tests/test_negsample_cpu.py) pin these references; the GPU tests (tests/test_gpu_negative_sampling.py)
hold the kernels to them.

cdf_exact restates ncf_negative_cdf step by step: integers summed exactly, one divide in double, one rounding to fp32.  None of
that depends on an order of summation, so the kernel's CDF equals it bit for bit whenever the weights themselves are specified
bit for bit (w == 0 and w == 1).  The one step that does depend on an order is the fp32 row sum that decides whether a row is
flagged; tests use only rows that are flagged, or not, in any order (see cdf_exact).
"""
import numpy as np


# ================================================================================================ the draw's uniform
def lowbias32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def slot_uniform(seed, slots):
    """u of include/ncf_abi.h (ncf_sample_negatives), in numpy: fp32, a multiple of 2^-24 in [0, 1)."""
    s = np.asarray(slots, dtype=np.uint64)
    lo, hi = (s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = lowbias32((lo * np.uint32(0x9E3779B1)) ^ np.uint32(seed))
        x = lowbias32(x ^ (hi * np.uint32(0x85EBCA77)) ^ np.uint32(0x68E31DA4))
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


# ================================================================================================ weights and the CDF
def weights(rating32, w):
    """The weight of every entry.  w == 0: ones (numpy's 0 ** 0 == 1).  w == 1: the ratings themselves, fp32 (numpy's r ** 1.0
    is r) — these two are specified bit for bit.  Any other w: float64 rating ** w, for the tolerance tests only (the device's
    powf is not specified to the bit)."""
    rating32 = np.asarray(rating32, dtype=np.float32)
    if w == 0:
        return np.ones_like(rating32)
    if w == 1:
        return rating32
    return rating32.astype(np.float64) ** w


def uniform_prefix(n):
    """The CDF of a flagged row of n entries: float32(float64(k + 1) / float64(n))."""
    return (np.arange(1, n + 1, dtype=np.float64) / np.float64(n)).astype(np.float32)


def length_groups(rowptr):
    """{length: the rows of that length (int64, ascending)} — the 2-D blocks cdf_exact works on."""
    lens = np.diff(np.asarray(rowptr, dtype=np.int64))
    order = np.argsort(lens, kind="stable")
    uniq, start = np.unique(lens[order], return_index=True)
    return {int(n): order[a:b] for n, a, b in zip(uniq, start, list(start[1:]) + [len(order)])}


def cdf_exact(weights32, rowptr, groups=None):
    """(cdf fp32, flag bool) of ncf_negative_cdf for fp32 weights, by the header's steps:

      1. s = the row's fp32 sum.  Not finite and positive (an empty row included): the row is flagged and holds
         float32(float64(k + 1) / float64(len)); an empty row writes nothing.
      2. S = 62 - len.bit_length(); scale = ldexp(1.0, S) / float64(max weight).
      3. q = rint(float64(wt) * scale) as int64, every weight > 0 raised to at least 1, everything else 0.
      4. prefix = the inclusive int64 cumsum of q; total = its last entry.
      5. cdf = float32(float64(prefix) / float64(total)).

    Step 1 sums in numpy's order and the kernel in its own, so a caller uses flagged rows that are flagged in any order (all
    weights zero, a NaN, an overflow of two 3e38s, an empty row) and good rows whose sum is finite and positive in any order.
    Rows of one length are handled together as 2-D arrays (``groups``: length_groups(rowptr), when the caller already has it)."""
    wt = np.asarray(weights32)
    assert wt.dtype == np.float32 and wt.ndim == 1
    rowptr = np.asarray(rowptr, dtype=np.int64)
    cdf = np.zeros(len(wt), dtype=np.float32)
    flag = False
    for n, rows in (length_groups(rowptr) if groups is None else groups).items():
        if n == 0:
            flag = flag or len(rows) > 0
            continue
        idx = rowptr[rows][:, None] + np.arange(n, dtype=np.int64)[None, :]
        W = wt[idx]                                                               # (rows of this length, n) fp32
        with np.errstate(over="ignore", invalid="ignore"):
            s = W.sum(axis=1, dtype=np.float32)
        bad = ~(np.isfinite(s) & (s > 0))
        if bad.any():
            flag = True
            cdf[idx[bad]] = uniform_prefix(n)[None, :]
        if bad.all():
            continue
        idx, W = idx[~bad], W[~bad]
        S = 62 - int(n).bit_length()
        scale = np.ldexp(np.float64(1.0), S) / W.max(axis=1).astype(np.float64)
        q = np.rint(W.astype(np.float64) * scale[:, None])
        q = np.where(W > 0, np.maximum(q, 1.0), 0.0).astype(np.int64)            # below 2^62: exact
        prefix = np.cumsum(q, axis=1, dtype=np.int64)
        cdf[idx] = (prefix.astype(np.float64) / prefix[:, -1:].astype(np.float64)).astype(np.float32)
    return cdf, flag


def cdf_float64(weights_any, rowptr):
    """cumsum(wt) / sum(wt) per row in float64: the reference's probabilities, for the tolerance comparisons."""
    wt = np.asarray(weights_any, dtype=np.float64)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    out = np.zeros(len(wt), dtype=np.float64)
    for n, rows in length_groups(rowptr).items():
        if n:
            idx = rowptr[rows][:, None] + np.arange(n, dtype=np.int64)[None, :]
            c = np.cumsum(wt[idx], axis=1)
            out[idx] = c / c[:, -1:]
    return out


# ================================================================================================ the draw
def draw_ref(rowptr, cdf, neg, pick, seed, slot0):
    """(out int64, flag bool) of ncf_sample_negatives: pick b draws with u = slot_uniform(seed, slot0 + b) the entry
    j = searchsorted(cdf_row, u, side='right'), clamped to len - 1, of row pick[b]; a pick outside [0, rows) or of an empty row
    gives -1 and sets the flag."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    cdf, neg, pick = np.asarray(cdf, dtype=np.float32), np.asarray(neg), np.asarray(pick, dtype=np.int64)
    rows, n = len(rowptr) - 1, len(pick)
    u = slot_uniform(seed, np.uint64(slot0) + np.arange(n, dtype=np.uint64))
    out = np.full(n, -1, dtype=np.int64)
    inside = (pick >= 0) & (pick < rows)
    lens = np.zeros(n, dtype=np.int64)
    lens[inside] = rowptr[pick[inside] + 1] - rowptr[pick[inside]]
    ok = lens > 0
    if rows <= 64:                                                               # a few rows, perhaps many picks: one mask per row
        per_row = ((r, np.flatnonzero(ok & (pick == r))) for r in range(rows))
    else:                                                                        # many rows: the picks of one row side by side
        where = np.flatnonzero(ok)
        where = where[np.argsort(pick[where], kind="stable")]
        picked, start = np.unique(pick[where], return_index=True)
        per_row = ((r, where[a:b]) for r, a, b in zip(picked, start, list(start[1:]) + [len(where)]))
    for r, sel in per_row:
        s, e = rowptr[r], rowptr[r + 1]
        if e == s:
            continue
        j = np.searchsorted(cdf[s:e], u[sel], side="right")
        out[sel] = neg[s + np.minimum(j, e - s - 1)]
    return out, bool((~ok).any())


# ================================================================================================ inputs
def _fill(lens, rng):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rowptr[-1])
    rating = (rng.integers(0, 11, nnz) * 0.5).astype(np.float32)
    beg, end = rowptr[:-1], rowptr[1:]
    ends = lens >= 3
    rating[beg[ends]] = 0.0
    rating[end[ends] - 1] = 0.0
    some = lens >= 1
    rating[(beg + lens // 2)[some]] = 3.5
    neg = rng.integers(0, 1 << 20, nnz).astype(np.int32)
    return rowptr, rating, neg


def rows_cycle(n_rows, lengths, seed):
    """(rowptr int64, rating fp32, neg int32, groups) of a CSR whose row r has lengths[r % len(lengths)] entries.  Ratings are
    the data set's: multiples of 0.5 in 0 .. 5 with zeros inside the rows, at both ends of every row of 3 or more entries, and
    one 3.5 in the middle so that every row keeps a positive weight.  All sums of such a row are exact in fp32, so no order of
    summation flags it.  ``groups`` is length_groups(rowptr)."""
    lens = np.asarray(lengths, dtype=np.int64)[np.arange(n_rows) % len(lengths)]
    assert (lens > 0).all()
    rowptr, rating, neg = _fill(lens, np.random.default_rng(seed))
    return rowptr, rating, neg, length_groups(rowptr)


FLAGGED_KINDS = ("zeros", "nan", "overflow", "empty")


def flagged_row(kind, n):
    """fp32 ratings of a row of n entries that has no distribution at w == 1, whatever the order its weights are summed in: all
    zeros; a NaN among ratings; two 3e38s (their sum alone overflows fp32) among ratings; no entries.  One entry cannot hold two
    3e38s: that row is all zeros."""
    if kind == "empty":
        return np.zeros(0, dtype=np.float32)
    row = np.zeros(n, dtype=np.float32)
    if kind == "zeros" or (kind == "overflow" and n < 2):
        return row
    row[:] = (np.arange(n) % 11) * 0.5
    if kind == "nan":
        row[n // 2] = np.nan
    else:
        assert kind == "overflow"
        row[0] = row[n - 1] = 3e38
    return row


def rows_cycle_flagged(n_rows, lengths, seed, every=7):
    """rows_cycle with every ``every``-th row replaced, in turn, by each of FLAGGED_KINDS.  Returns (rowptr, rating, neg, kind) with
    kind[r] = -1 for a good row, else the index into FLAGGED_KINDS."""
    lens = np.asarray(lengths, dtype=np.int64)[np.arange(n_rows) % len(lengths)]
    kind = np.full(n_rows, -1, dtype=np.int64)
    swapped = np.arange(0, n_rows, every)
    kind[swapped] = np.arange(len(swapped)) % len(FLAGGED_KINDS)
    lens[kind == FLAGGED_KINDS.index("empty")] = 0
    rowptr, rating, neg = _fill(lens, np.random.default_rng(seed))
    for r in swapped:
        rating[rowptr[r]:rowptr[r + 1]] = flagged_row(FLAGGED_KINDS[kind[r]], int(lens[r]))
    return rowptr, rating, neg, kind


def equality_cdf(seed, n_slots=64, step=3):
    """A hand-written CDF row: every ``step``-th of the distinct u values of slots 0 .. n_slots - 1, ascending, then 1.0.  A pick
    whose u is one of those entries, bit for bit, must land on the entry after it ('right')."""
    u = np.unique(slot_uniform(seed, np.arange(n_slots, dtype=np.uint64)))[::step]
    return np.concatenate([u, [1.0]]).astype(np.float32)
