"""Inputs and references for the three families that prepare inputs for the scoring kernels: the dense matrix -> shared-row CSR
conversion (csrc/dense_csr.hip), the row L2 normalisation (l2_normalize_rows_kernel in csrc/attn.hip) and the bounded exchange
(csrc/exchange.hip: ncf_bucket_ids, ncf_bucket_ids_dedup, ncf_gather_buckets).  No GPU needed: everything here is plain torch /
Python on whatever device its arguments live on.  The CPU tests (tests/test_prep_forms_cpu.py) pin these references; the GPU
tests hold the kernels to them.

Every expected result is an integer or a moved bit pattern and is compared with torch.equal, except the norm, whose bar is
derived from the kernel's operation order (L2_BAR below).
"""
import math

import torch

# ================================================================================================ dense matrix -> shared-row CSR
DENSE_SENTINEL = 77.25          # the columns beside the slice: a kernel that reads past I counts or lists it
DENORMAL = 1e-40                # an fp32 denormal: a rated entry, listed with its bits


def dense_csr_reference(um, share_rows):
    """The definition.  um: CPU fp32 (B, I), any row stride.  Returns (rowptr int64 (B+1), col int32 (n), val bits int32 (n),
    pair_row int64 (B)): row b lists the columns where um[b] != 0 in column order with the values' bits; with sharing, pair_row[b]
    is the smallest b' <= b whose row equals row b element by element under float == (-0 equals +0; a row holding a NaN equals
    nothing, itself included, and so represents itself); rows that are not their own representative are empty.

    Equality under == is decided through a canonical form: for rows without a NaN, x == y element by element exactly when the two
    rows have the same bits once every -0 is written as +0.  dense_pair_row_by_definition is the quadratic statement of the same
    rule; the CPU tests hold this function to it."""
    um = um.detach().cpu()
    B, I = um.shape
    pair_row = torch.arange(B, dtype=torch.int64)
    if share_rows and B:
        canon = torch.where(um == 0, torch.zeros_like(um), um).contiguous()
        has_nan = torch.isnan(um).any(dim=1).tolist()
        raw = canon.view(torch.int32).numpy() if I else None
        first = {}
        for b in range(B):
            if has_nan[b]:
                continue
            key = raw[b].tobytes() if I else b""
            pair_row[b] = first.setdefault(key, b)
    keep = pair_row == torch.arange(B, dtype=torch.int64)
    mask = (um != 0) & keep[:, None]
    col = mask.nonzero()[:, 1].to(torch.int32) if B and I else torch.zeros(0, dtype=torch.int32)
    val = um[mask].contiguous().view(torch.int32) if B and I else torch.zeros(0, dtype=torch.int32)
    rowptr = torch.zeros(B + 1, dtype=torch.int64)
    if B:
        rowptr[1:] = torch.cumsum(mask.sum(dim=1), 0)
    return rowptr, col, val, pair_row


def dense_pair_row_by_definition(um):
    """pair_row with sharing on, by the quadratic definition (small B only)."""
    um = um.detach().cpu()
    B = um.shape[0]
    out = torch.arange(B, dtype=torch.int64)
    for b in range(B):
        for a in range(b):
            if bool((um[a] == um[b]).all()):
                out[b] = a
                break
    return out


def dense_csr_mismatch(got, ref):
    """None when (rowptr, col, val, pair_row) from a conversion equals the reference; else the name of the first part that differs.
    got's col / val may be longer than rowptr[B]: only that prefix is compared; val is compared through its int32 view."""
    rowptr, col, val, pair_row = (t.detach().cpu() for t in got)
    r_rowptr, r_col, r_val, r_pair = ref
    if not torch.equal(rowptr, r_rowptr):
        return "rowptr"
    if not torch.equal(pair_row, r_pair):
        return "pair_row"
    n = int(r_rowptr[-1])
    if not torch.equal(col[:n], r_col):
        return "col"
    bits = val[:n].contiguous()
    bits = bits if bits.dtype == torch.int32 else bits.view(torch.int32)
    if not torch.equal(bits, r_val):
        return "val"
    return None


def dense_window_columns(I):
    """First column of the last unroll window of the scan / compact loops (8 x 64 columns) and of the verify loop (4 x 64)."""
    return sorted({((I - 1) // 512) * 512, ((I - 1) // 256) * 256}) if I > 0 else []


def dense_planted_rows(I, g):
    """Rows built from one template row t (list of (name, row)), in order of priority when only the first few fit:
    t; three bitwise-identical rows that hold a NaN; t again (the NaN rows' non-NaN twin: it must still share with t); rows that
    differ from t only in column 0, only in column I-1, only in the first column of the last window (twice each: the pair must not
    share with t, and must share with each other); +0 / -0 in one column of otherwise equal rows; denormals of both signs; +-inf;
    one ulp; the same values in permuted columns."""
    t = torch.randint(1, 11, (I,), generator=g).float() * 0.5
    t[torch.rand(I, generator=g) < 0.5] = 0.0
    cz, cd, ci, cu, cn, cp, cq = (c % I for c in (3, 5, 9, 11, 17, 20, 21))
    for c in (0, I - 1, cz, cd, ci, cu, cn, *dense_window_columns(I)):
        t[c] = 1.5
    t[cp], t[cq] = 2.5, (4.0 if cp != cq else 2.5)

    def edit(*pairs):
        r = t.clone()
        for c, v in pairs:
            r[c] = v
        return r

    nan = edit((cn, float("nan")))
    rows = [("t", t.clone()), ("nan0", nan.clone()), ("nan1", nan.clone()), ("t_again", t.clone()), ("nan2", nan.clone()),
            ("col0", edit((0, 2.0))), ("col0_again", edit((0, 2.0))),
            ("last", edit((I - 1, 2.0))), ("last_again", edit((I - 1, 2.0)))]
    for c in dense_window_columns(I):
        rows += [(f"win{c}", edit((c, 3.0))), (f"win{c}_again", edit((c, 3.0)))]
    rows += [("pos_zero", edit((cz, 0.0))), ("neg_zero", edit((cz, -0.0))),
             ("pos_denormal", edit((cd, DENORMAL))), ("neg_denormal", edit((cd, -DENORMAL))), ("pos_denormal_again", edit((cd, DENORMAL))),
             ("pos_inf", edit((ci, float("inf")))), ("neg_inf", edit((ci, float("-inf")))),
             ("one_ulp", edit((cu, float(torch.nextafter(torch.tensor(1.5), torch.tensor(2.0)))))),
             ("permuted", edit((cp, float(t[cq])), (cq, float(t[cp])))),
             ("t_last", t.clone())]
    return rows


def dense_case(B, I, population="repeated", seed=0, plant=True, pad=3):
    """(wide, um): um = wide[:, pad:pad + I] is the (B, I) matrix under test, a column slice of a matrix whose other columns hold
    DENSE_SENTINEL.  population: "identical" (one user), "distinct" (every row drawn on its own), "repeated" (about 40 users, or
    B / 3 for a small batch, each row one of them).  With ``plant`` the rows of dense_planted_rows overwrite rows spread over the
    batch (the first B of them when B is smaller than their number)."""
    g = torch.Generator().manual_seed(seed * 1_000_003 + B * 1031 + I)
    wide = torch.full((B, I + 2 * pad), DENSE_SENTINEL, dtype=torch.float32)
    um = wide[:, pad:pad + I]
    if B == 0 or I == 0:
        return wide, um
    users = {"identical": 1, "distinct": B, "repeated": max(1, min(40, B // 3))}[population]
    rows = torch.randint(1, 11, (users, I), generator=g).float() * 0.5 - 2.75          # half-step ratings, never 0
    rows[torch.rand(users, I, generator=g) >= 0.3] = 0.0
    who = torch.arange(B) if population == "distinct" else torch.randint(0, users, (B,), generator=g)
    um.copy_(rows[who])
    if plant:
        planted = dense_planted_rows(I, g)
        for b, (_, r) in zip(_planted_positions(B, len(planted)), planted):
            um[b] = r
    return wide, um


def _planted_positions(B, n):
    """Rows of the first min(n, B) planted rows: spread over the workgroups (4 rows each), or the first rows of a small batch."""
    return [j if B < 2 * n else (j * B) // n + (j % 3) for j in range(min(n, B))]


def dense_planted_map(B, I):
    """{name: row} of the rows dense_case(B, I, plant=True) plants (the names of dense_planted_rows)."""
    names = [name for name, _ in dense_planted_rows(I, torch.Generator().manual_seed(0))]
    return dict(zip(names, _planted_positions(B, len(names))))


# ================================================================================================ row L2 normalisation
L2_CLAMP = float(torch.tensor(1e-12, dtype=torch.float32))         # the kernel's clamp as the fp32 number it is


def l2_bar(E):
    """Relative bar per element: ceil(E/16) fused multiply-adds per lane and four shuffle adds give at most (ceil(E/16) + 4) 2^-24
    in the sum of squares; the square root halves that and adds one rounding, the division one more; doubled for the second-order
    terms: (ceil(E/16) + 8) 2^-24."""
    return (math.ceil(E / 16) + 8) * 2.0 ** -24


def l2_reference(x):
    """float64: x / max(sqrt(sum x^2), float(float32(1e-12))); the maximum propagates a NaN norm."""
    x64 = x.detach().double()
    n = torch.sqrt((x64 * x64).sum(dim=1, keepdim=True))
    return x64 / torch.maximum(n, torch.full_like(n, L2_CLAMP))


L2_ROW_KINDS = ("unit", "small", "large", "zero", "single", "tiny", "nan", "inf")


def l2_case(R, E, seed=0):
    """CPU fp32 (R, E); row r is of kind L2_ROW_KINDS[r % 8]: random at scale 1, 1e-6, 1e12; all zeros; a single non-zero element;
    values around 1e-20 (norm below the clamp); a NaN among random values; one +inf among random values."""
    g = torch.Generator().manual_seed(seed * 7919 + R * 131 + E)
    x = torch.randn(R, E, generator=g)
    r = torch.arange(R)
    kind = r % 8
    x[kind == 1] *= 1e-6
    x[kind == 2] *= 1e12
    x[kind == 3] = 0.0
    x[kind == 5] *= 1e-20
    pos = (r * 7 + 3) % E
    single = kind == 4
    keep = x[r, pos].clone()
    x[single] = 0.0
    x[r[single], pos[single]] = torch.where(keep[single] == 0, torch.ones(()), keep[single]) * 3.7
    x[r[kind == 6], pos[kind == 6]] = float("nan")
    x[r[kind == 7], pos[kind == 7]] = float("inf")
    return x


def l2_ratio(out, ref, E):
    """Largest |out - ref| / (l2_bar(E) |ref|) over the elements with a finite non-zero reference, after asserting what has no
    tolerance: NaN exactly where the reference has one, and exact zeros where the reference is zero."""
    out64, ref = out.detach().double().cpu(), ref.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(out64), nan), "NaN positions differ from the float64 formula's"
    zero = ref == 0
    assert bool((out64[zero] == 0).all()), "a zero of the reference is not an exact zero"
    sel = ~nan & ~zero
    if not bool(sel.any()):
        return 0.0
    return float(((out64[sel] - ref[sel]).abs() / (l2_bar(E) * ref[sel].abs())).max())


def l2_kernel_order_model(x, drop_lane=None, clamp=L2_CLAMP, squared=False):
    """CPU emulation of the kernel's order in fp32: lane s of 16 accumulates x[s], x[s + 16], ... with fused multiply-adds (the
    product is exact in float64, one rounding to fp32 per step), four butterfly adds, sqrt, clamp, division.  The keyword
    arguments make the three wrong kernels the bar must reject."""
    R, E = x.shape
    steps = math.ceil(E / 16)
    xp = torch.zeros(R, steps * 16, dtype=torch.float32)
    xp[:, :E] = x
    xp = xp.view(R, steps, 16)
    ss = torch.zeros(R, 16, dtype=torch.float32)
    for k in range(steps):
        ss = (xp[:, k].double() * xp[:, k].double() + ss.double()).float()
    if drop_lane is not None:
        ss[:, drop_lane] = 0.0
    for off in (8, 4, 2, 1):
        ss = ss + ss[:, torch.arange(16) ^ off]
    n = torch.sqrt(ss[:, :1])
    if squared:
        n = n * n
    c = torch.tensor(clamp, dtype=torch.float32)
    d = torch.where(n < c, c, n)
    return x / d


# ================================================================================================ exchange: bucketing
def bucket_ids_model(idx, rpr, total, world, cap, dedup=False, sentinel=-7):
    """A sequential model of ncf_bucket_ids / ncf_bucket_ids_dedup (one of the many orders the definition allows).  Returns
    (send, slot, counts, oob, overflow); send is (world * cap) with unused slots 0, or, de-duplicating, world buckets of
    [count, ids...] whose padding keeps ``sentinel`` (never initialised)."""
    B = idx.numel()
    counts = [0] * world
    slot = torch.full((B,), -1, dtype=torch.int64)
    send = torch.full((world * (cap + 1),), sentinel, dtype=torch.int64) if dedup else torch.zeros(world * cap, dtype=torch.int64)
    oob = overflow = 0
    seen = {}
    for p, i in enumerate(idx.tolist()):
        if not 0 <= i < total:
            oob = 1
            continue
        if dedup and i in seen:
            slot[p] = seen[i]
            continue
        o = i // rpr
        k = counts[o]
        counts[o] += 1
        s = -1
        if k < cap:
            s = o * cap + k
            send[o * (cap + 1) + 1 + k if dedup else s] = i - o * rpr
        else:
            overflow = 1
        slot[p] = s
        if dedup:
            seen[i] = s
    if dedup:
        send.view(world, cap + 1)[:, 0] = torch.tensor(counts).clamp(max=cap)
    return send, slot, torch.tensor(counts, dtype=torch.int32), oob, overflow


def _owners(idx, rpr, total):
    ok = (idx >= 0) & (idx < total)
    return ok, torch.where(ok, idx // rpr, torch.zeros_like(idx))


def check_bucket_ids(idx, rpr, total, world, cap, send, slot, counts, overflow):
    """ncf_bucket_ids against its definition (include/ncf_abi.h), CPU tensors: every kept id sits in its owner's bucket as a local
    row, slot[p] points at it, counts are exact, unused slots are 0, buckets are filled from their start, ids over capacity / out
    of range are dropped (slot -1), the overflow flag is set exactly when a bucket overflows.  Returns the kept mask."""
    B = idx.numel()
    slot = slot[:B]
    ok, owner = _owners(idx, rpr, total)
    expect = torch.bincount(owner[ok], minlength=world)
    assert torch.equal(counts.long(), expect)
    assert int(overflow) == int(bool((expect > cap).any()))
    assert bool(((slot >= -1) & (slot < world * cap)).all())
    kept = slot >= 0
    assert not bool(kept[~ok].any())
    assert torch.equal(slot[kept] // cap, owner[kept])                       # the right bucket
    assert torch.equal(send[slot[kept]], (idx - owner * rpr)[kept])          # holding the right local row
    assert torch.unique(slot[kept]).numel() == int(kept.sum())               # one pair per slot
    assert torch.equal(torch.bincount(owner[kept], minlength=world), expect.clamp(max=cap))
    used = torch.zeros(world * cap, dtype=torch.bool)
    used[slot[kept]] = True
    assert bool((send[:world * cap][~used] == 0).all())                      # padding names local row 0
    filled = torch.arange(cap)[None, :] < expect.clamp(max=cap)[:, None]     # a bucket is filled from its start
    assert torch.equal(used.view(world, cap), filled)
    return kept


def check_bucket_ids_dedup(idx, rpr, total, world, cap, send, slot, counts, overflow):
    """ncf_bucket_ids_dedup against its definition, CPU tensors: every DISTINCT valid id is listed once in its owner's bucket (as a
    local row, inside the filled prefix, header = min(count, cap)), every pair of that id points at that slot, pairs of a dropped id
    all get -1, counts are the distinct counts, ids over capacity / out of range are dropped and flagged.  Returns the kept mask."""
    B = idx.numel()
    send_c, slot = send[:world * (cap + 1)].view(world, cap + 1), slot[:B]
    ok, owner = _owners(idx, rpr, total)
    uniq, inv = torch.unique(idx[ok], return_inverse=True)
    expect = torch.bincount(uniq // rpr, minlength=world)
    assert torch.equal(counts.long(), expect)
    assert int(overflow) == int(bool((expect > cap).any()))
    assert torch.equal(send_c[:, 0], expect.clamp(max=cap))                                # bucket headers
    assert bool(((slot >= -1) & (slot < world * cap)).all())
    kept = slot >= 0
    assert not bool(kept[~ok].any())
    assert torch.equal(slot[kept] // cap, owner[kept])                                     # the right bucket
    k = slot[kept] % cap
    assert bool((k < send_c[owner[kept], 0]).all())                                        # inside the bucket's filled prefix
    assert torch.equal(send_c[owner[kept], 1 + k], (idx - owner * rpr)[kept])              # holding the right local row
    # one slot per distinct id: pairs with equal ids share it (a dropped id is dropped for all its pairs), distinct ids never do
    assert torch.unique(slot[kept]).numel() == torch.unique(idx[kept]).numel()
    assert torch.unique(torch.stack([slot[kept], idx[kept]]), dim=1).shape[1] == torch.unique(slot[kept]).numel()
    if uniq.numel():
        lo = torch.full((uniq.numel(),), 1 << 62, dtype=torch.int64).scatter_reduce(0, inv, slot[ok], "amin")
        hi = torch.full((uniq.numel(),), -(1 << 62), dtype=torch.int64).scatter_reduce(0, inv, slot[ok], "amax")
        assert torch.equal(lo, hi)
        assert torch.equal(torch.bincount(uniq[lo >= 0] // rpr, minlength=world), expect.clamp(max=cap))   # exactly the overflow is dropped
    if not bool((expect > cap).any()):
        assert bool(kept[ok].all())
    return kept


# ================================================================================================ exchange: bucket gather
GATHER_CHUNKS = {1: (1, 2, 3), 4: (4, 5, 7), 8: (8, 12, 15), 16: (16, 17, 33)}      # lanes per row -> row sizes in 16-byte chunks


def gather_lanes_per_row(chunks):
    return 16 if chunks >= 16 else 8 if chunks >= 8 else 4 if chunks >= 4 else 1


def bit_table(rows, E, dtype, g, device="cpu"):
    """A table of random bit patterns (every exponent, NaNs included: rows are moved, never computed with)."""
    if dtype == torch.float32:
        return torch.randint(-2 ** 31, 2 ** 31, (rows, E), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32).to(device)
    return torch.randint(-2 ** 15, 2 ** 15, (rows, E), generator=g, dtype=torch.int64).to(torch.int16).view(torch.bfloat16).to(device)


def bits(t):
    """The integer view of an fp32 / bf16 tensor (contiguous copy)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def gather_buckets_expected(table, recv, world, cap, out_before):
    """(expected out, flag) of ncf_gather_buckets by its definition, on the arguments' device: row r * cap + k of out is
    table[recv[r][1 + k]] for k < recv[r][0], a zero row (and the flag) where that id is outside [0, rows); every other row of
    ``out_before`` (padding inside the buckets, rows past world * cap) is left as it was.  One indexed read."""
    rows = table.shape[0]
    rc = recv[:world * (cap + 1)].view(world, cap + 1)
    ids = rc[:, 1:]
    filled = torch.arange(cap, device=recv.device)[None, :] < rc[:, :1]
    ok = (ids >= 0) & (ids < rows)
    exp = out_before.clone()
    body = exp[:world * cap]
    good = (filled & ok).reshape(-1)
    body[good] = table[ids.reshape(-1)[good]]
    body[(filled & ~ok).reshape(-1)] = 0
    return exp, bool((filled & ~ok).any())
