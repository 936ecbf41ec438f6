"""numpy restatement of csrc/pair_rows.hip (include/ncf_abi.h: ncf_pair_rows_count / ncf_pair_rows_fill), the reference the GPU tests hold
the kernels to bit for bit, and the shared test data of test_pair_rows_cpu.py / test_gpu_pair_rows.py."""
import numpy as np

F32 = np.float32


def isclose_f32(a, b, atol=1e-5, rtol=1e-5):
    """torch.isclose(a, b, rtol, atol) in fp32, every operation rounded on its own:
    a == b || (isfinite(a) && isfinite(b) && |a - b| <= atol + |rtol * b|)."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.abs(a - b)                                    # fp32 - fp32 -> fp32
        bound = F32(atol) + np.abs(F32(rtol) * b)               # the product rounds to fp32 before the add
        return (a == b) | (np.isfinite(a) & np.isfinite(b) & (diff <= bound))


def pair_rows_count_ref(rowptr, pair_row):
    """(out_rowptr before the cumulative sum (B + 1), out-of-range flag)."""
    R = len(rowptr) - 1
    out = np.zeros(len(pair_row) + 1, dtype=np.int64)
    oob = 0
    for b, r in enumerate(pair_row):
        if 0 <= r < R:
            out[b + 1] = rowptr[r + 1] - rowptr[r]
        else:
            oob = 1
    return out, oob


def pair_rows_ref(rowptr, col, val, pair_row, capacity, mask=None, atol=1e-5, rtol=1e-5, fill_col=None, fill_val=None):
    """(out_rowptr (B + 1), out_col (capacity), out_val (capacity), overflow flag, out-of-range flag).  ``fill_col`` / ``fill_val``: what
    the output buffers hold before the call (entries the kernel does not write keep it)."""
    rowptr, col, val, pair_row = np.asarray(rowptr), np.asarray(col), np.asarray(val), np.asarray(pair_row)
    R = len(rowptr) - 1
    cnt, oob = pair_rows_count_ref(rowptr, pair_row)
    out_rowptr = np.cumsum(cnt)
    out_col = np.full(capacity, 0 if fill_col is None else fill_col, dtype=np.int32)
    out_val = np.full(capacity, 0 if fill_val is None else fill_val, dtype=F32)
    flag = 0
    for b, r in enumerate(pair_row):
        if not 0 <= r < R:
            continue
        for k in range(int(rowptr[r + 1] - rowptr[r])):
            c, v = int(col[rowptr[r] + k]), val[rowptr[r] + k]
            if mask is not None and 0 <= c < mask[1].shape[0] and bool(isclose_f32(mask[0][b], mask[1][c], atol, rtol).all()):
                c = -1
            o = out_rowptr[b] + k
            if o < capacity:
                out_col[o], out_val[o] = c, v
            else:
                flag = 1
    return out_rowptr, out_col, out_val, flag, oob


# ------------------------------------------------------------------------------------------ the shared case of the GPU test
ROW_LENS = (0, 1, 3, 63, 64, 65, 130, 257)     # around the wave (64) and every lane-group step of the vector path
N_ITEMS = 300


def shared_csr(seed=0):
    """R = 8 shared rows of ROW_LENS over a catalogue of N_ITEMS; a few entries carry col = -1 and col = N_ITEMS (outside the
    catalogue: copied unchanged, never compared)."""
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(len(ROW_LENS) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(ROW_LENS)
    col = np.concatenate([np.sort(rng.choice(N_ITEMS, n, replace=False)) for n in ROW_LENS]).astype(np.int32)
    val = rng.uniform(-2, 2, len(col)).astype(F32)
    for r, k, c in ((3, 5, -1), (5, 64, N_ITEMS), (7, 0, -1), (7, 256, N_ITEMS), (6, 129, N_ITEMS + 7)):
        col[rowptr[r] + k] = c
    return rowptr, col, val


def pairs(B, seed=1):
    """pair_row (B,): unsorted, with repeats; row 4 is never used."""
    rng = np.random.default_rng(seed)
    if B == 1:
        return np.array([7], dtype=np.int64)
    pr = rng.choice([0, 1, 2, 3, 5, 6, 7], B).astype(np.int64)
    pr[:8] = [7, 7, 6, 6, 3, 1, 5, 0]
    return pr


KINDS = ("self", "twins", "half", "over", "nan", "inf")


def mask_tables(rowptr, col, pair_row, E, seed=2):
    """(cand (B, E), rated (N_ITEMS, E), plan) with every mask case the kernel can meet.  ``rated`` rows are random; the first two
    catalogue rows that shared row 7 rates (the twins) are made identical.  Pair b with a usable rated entry c0 of ITS OWN row gets
    a candidate built from rated[c0], by kind KINDS[b % 6]:
      self   an exact copy (the self entry: masked)
      twins  a copy of the twins' row: a pair that rates both has both masked
      half   one element off by 0.5x the allowed error atol + |rtol * rated| (still masked)
      over   one element off by 1.5x the allowed error (not masked)
      nan    one element NaN on both sides (not masked: NaN is close to nothing)
      inf    one element +inf on both sides (masked); another rated entry c1 of the pair holds the same row with -inf there (not masked)
    ``plan``: [(b, kind, c0, c1 or None)] for the pairs that got their case, for the tests to check the reference against."""
    rng = np.random.default_rng(seed)
    rated = rng.uniform(-1, 1, (N_ITEMS, E)).astype(F32)
    row7 = [int(c) for c in col[rowptr[7]:rowptr[8]] if 0 <= c < N_ITEMS]
    twins = (row7[0], row7[1])
    rated[twins[1]] = rated[twins[0]]
    B = len(pair_row)
    cand = rng.uniform(-1, 1, (B, E)).astype(F32)

    def usable(b):
        r = pair_row[b]
        return [int(c) for c in col[rowptr[r]:rowptr[r + 1]] if 0 <= c < N_ITEMS and c not in twins and np.isfinite(rated[c]).all()]

    plan = []
    for b in range(B):                              # first the cases that put specials INTO the rated table
        kind, e = KINDS[b % 6], (5 * b) % E
        if kind not in ("nan", "inf"):
            continue
        ent = usable(b)
        if kind == "nan" and ent:
            c0 = ent[(3 * b) % len(ent)]
            rated[c0, e] = np.nan
            plan.append((b, kind, c0, None))
        elif kind == "inf" and len(ent) > 1:
            c0, c1 = ent[(3 * b) % len(ent)], ent[(3 * b + 1) % len(ent)]
            rated[c0, e] = np.inf
            rated[c1] = rated[c0]
            rated[c1, e] = -np.inf
            plan.append((b, kind, c0, c1))
    for b in range(B):                              # then the others, over rows that stayed finite
        kind, e = KINDS[b % 6], (5 * b) % E
        ent = usable(b)
        if kind in ("nan", "inf") or not ent:
            continue
        c0 = ent[(3 * b) % len(ent)]
        plan.append((b, kind, c0, None))
    for b, kind, c0, _ in plan:                     # candidates last: the rated table no longer changes
        e = (5 * b) % E
        cand[b] = rated[twins[0]] if kind == "twins" else rated[c0]
        allowed = F32(1e-5) + np.abs(F32(1e-5) * rated[c0, e])
        if kind == "half":
            cand[b, e] = rated[c0, e] + F32(0.5) * allowed
        elif kind == "over":
            cand[b, e] = rated[c0, e] + F32(1.5) * allowed
    return cand, rated, sorted(plan), twins


def check_plan(plan, twins, rowptr, col, pair_row, out_rowptr, out_col):
    """The reference's (or the kernel's) columns against what ``mask_tables`` built: which entry of which pair is masked."""
    seen = set()
    for b, kind, c0, c1 in plan:
        r = pair_row[b]
        orig = col[rowptr[r]:rowptr[r + 1]]
        got = out_col[out_rowptr[b]:out_rowptr[b + 1]]
        masked = set(int(c) for c, g in zip(orig, got) if g == -1 and c != -1)
        assert all(g == c for c, g in zip(orig, got) if g != -1)
        if kind == "self":
            assert masked == {c0}, (b, kind, masked)
        elif kind == "twins":
            assert masked == set(twins) & set(int(c) for c in orig), (b, kind, masked)
            if len(masked) == 2:
                seen.add("twins-both")
        elif kind == "half":
            assert masked == {c0}, (b, kind, masked)
        elif kind in ("over", "nan"):
            assert masked == set(), (b, kind, masked)
        else:
            assert c0 in masked and c1 not in masked, (b, kind, masked)    # (at E = 1 another pair's +inf row is this row too)
        seen.add(kind)
    return seen
