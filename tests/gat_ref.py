"""References for the LightGAT training kernels (csrc/gat.hip: ncf_gat_edge_softmax, ncf_gat_edge_grad, ncf_gat_source_reduce),
restated in numpy / float64 from include/ncf_abi.h ("LightGAT TRAINING STEP").  Nothing here imports the package or needs a GPU.

    alpha_e  = exp(s[col_e] - M_r) / (sum_kept exp(s[col_.] - M_r) + 1e-16)          kept: keep[e] != 0 and col[e] in range
    g_e      = (attr ? attr_e : 1) * < dY[row_e], drop_e(z[col_e]) >                  drop_e: THE MASK on (CSR position e, feature)
    S_r      = sum_{e in r} alpha_e g_e,     dlogit_e = alpha_e (g_e - S_r),     ds[n] = sum_{e: col_e = n} dlogit_e

THE EXACT CASES (``exact_case``).  Rows whose kept, in-range entry counts are 1, 2, 4, .., 1024 (not in that order: the 1024-entry
row sits in the middle), an empty row, a row with every entry removed and a row with every entry out of range; removed and
out-of-range entries are mixed into the other rows too, and the removed ones point at nodes of ANOTHER class whose score is 3e4
higher or lower, so a removed entry that still counted would move the maximum.  Scores are constant within a row (the class
construction of graph_forms_ref.softmax_case("a"): node n has class n % 8 and score A_LEVELS[n % 8], a row reads its own class),
so every kept difference is 0, exp(0) = 1, the denominator is the integer count k = 2^j (1e-16 vanishes against it) and
alpha = 2^-j exactly.  z and dY are integers in [-3, 3], attr is a non-zero integer in [-3, 3], p is 0 or 0.5 (thr = 32768, scale
exactly 2).  Then, for D <= 64:
    |g_e| <= 3 * 2 * 9 * 64 = 3456 < 2^12, an integer;   alpha_e g_e is a multiple of 2^-10 below 2^12;
    every partial sum of S_r is a multiple of 2^-10 of magnitude <= 1024 * 2^-10 * 3456 < 2^12: 22 bits;
    g_e - S_r is a multiple of 2^-10 below 2^13 (23 bits) and the product with alpha_e = 2^-j only moves the exponent,
so every operation is exact in fp32 whatever the order of summation or the split into segments, and the float64 value IS the
expected fp32 output, bit for bit.  tests/test_gat_cpu.py proves it with float32 emulations of different orders and splits.
For ncf_gat_source_reduce: dlogit integers in [-7, 7], source degrees up to 1500: partial sums below 2^14, exact likewise.

THE BOUND of ncf_gat_edge_grad on random data (``edge_grad_bound``), of the gamma form used for the SpMM
(graph_forms_ref.spmm_bound): (roundings on the longest path + 8) 2^-24 x (the magnitudes that enter).  With the kernel's own alpha
taken as exact input and G_e = |attr_e| sum_f |dY[r, f] drop_e(z[col_e])_f|, counted from the summation order written in the
header comment of csrc/gat.hip (u = 2^-24, LPR = lanes per row, EPI = 64 / LPR entries per wave-instruction):
    g_e       the mask's scale product (p > 0)                                          1
              the lane's 4 products: one multiplication and three fma                   4
              the butterfly over the row's LPR lanes                                    log2 LPR
              the attr product                                                          1            = k_g
    S_r       alpha_e g_e enters its entry group's serial fma chain; the chain has
              ceil(min(n_r, seg_len) / EPI) links                                       ceil(min(n_r, seg_len) / EPI)
              the butterfly over the EPI groups                                         log2 EPI
              split rows: lane-strided sum of the segment sums, 6-step butterfly        ceil(n_seg / 64) + 6      = k_S - k_g
    dlogit_e  the difference and the product with alpha_e                               2
    |dlogit_e - ref_e| <= (k_S + 2 + 8) u alpha_e (G_e + sum_{j in r} alpha_j G_j)
(g_e's own error is <= gamma_{k_g} G_e and S_r's <= gamma_{k_S} sum_j alpha_j G_j; k_g <= k_S).  A zero bound asks for exactness.
"""
import numpy as np
import torch

import graph_forms_ref as R
from dropout_mask_ref import keep_mask, mask_factor64, scale32

U24 = 2.0 ** -24
EXACT_COUNTS = [1, 2, 4, 8, 16, 1024, 32, 64, 128, 256, 512]
SOFTMAX_DEFECTS = ["removed_counted"]
GRAD_DEFECTS = ["mask_not_regenerated", "sum_per_segment", "last_segment_dropped"]


# ------------------------------------------------------------------------------------------------------- float64 references
def masked_col(col, keep):
    """``col`` with the removed entries mapped out of range: a removed entry is not in its group."""
    return col if keep is None else torch.where(keep != 0, col, torch.full_like(col, -1))


def masked_softmax64(rowptr, col, attr, keep, s):
    """(alpha, coef) float64: graph_forms_ref.softmax_reference64 over the kept entries."""
    c = masked_col(col, keep)
    return R.softmax_reference64(rowptr, c, None, s), R.softmax_reference64(rowptr, c, attr, s)


def _masked_z64(col, z, p, seed):
    """(E, D) float64: drop_e(z[col_e]) with e the CSR position; rows of out-of-range entries are 0."""
    E, (Nz, D) = col.numel(), z.shape
    ok = (col >= 0) & (col < Nz)
    zz = z.double().cpu()[col.long().cpu().clamp(0, max(Nz - 1, 0))]
    if p > 0:
        zz = zz * mask_factor64(seed, np.arange(E), D, p)
    return torch.where(ok.cpu()[:, None], zz, torch.zeros_like(zz))


def edge_g64(rowptr, col, attr, dY, z, p=0.0, seed=0):
    """(g, G) float64 on the CPU: g_e and the magnitude sum_f |attr_e dY[r, f] drop_e(z)_f| that enters it."""
    dst = R.rows_of(rowptr.cpu())
    prod = dY.double().cpu()[dst] * _masked_z64(col, z, p, seed)
    w = torch.ones(col.numel(), dtype=torch.float64) if attr is None else attr.double().cpu()
    return w * prod.sum(1), w.abs() * prod.abs().sum(1)


def edge_grad64(rowptr, col, attr, alpha, dY, z, p=0.0, seed=0):
    """dlogit (E,) float64 on the CPU for the given alpha (0 on removed / out-of-range entries); also returns (g, S per row)."""
    rowptr = rowptr.cpu()
    dst = R.rows_of(rowptr)
    g, _ = edge_g64(rowptr, col, attr, dY, z, p, seed)
    a = alpha.double().cpu()
    S = torch.zeros(rowptr.numel() - 1, dtype=torch.float64).index_add_(0, dst, a * g)
    return torch.where(a != 0, a * (g - S[dst]), torch.zeros_like(a)), (g, S)        # outside its group: +0, as the kernel writes it


def source_reduce64(rowptr_t, eid, dlogit):
    """ds (n,) float64: the sum of dlogit[eid[k]] over each row of the CSR by source."""
    rowptr_t = rowptr_t.cpu()
    return torch.zeros(rowptr_t.numel() - 1, dtype=torch.float64).index_add_(0, R.rows_of(rowptr_t), dlogit.double().cpu()[eid.long().cpu()])


def edge_grad_bound(rowptr, col, attr, alpha, dY, z, p, seed, seg_len=None):
    """(E,) float64, the module docstring's bound for the kernel launched over segments of ``seg_len`` (None: rows unsplit)."""
    rowptr = rowptr.cpu()
    D = z.shape[1]
    lpr = R.lanes_per_row(D)
    epi = 64 // lpr
    dst = R.rows_of(rowptr)
    n_r = (rowptr[1:] - rowptr[:-1]).double()
    _, G = edge_g64(rowptr, col, attr, dY, z, p, seed)
    a = alpha.double().cpu().abs()
    k_g = (1 if p > 0 else 0) + 4 + int(np.log2(lpr)) + 1
    in_seg = n_r if seg_len is None else n_r.clamp(max=seg_len)
    k_S = k_g + torch.ceil(in_seg / epi) + int(np.log2(epi))
    if seg_len is not None:
        n_seg = torch.ceil(n_r / seg_len)
        k_S = k_S + torch.where(n_seg > 1, torch.ceil(n_seg / 64) + 6, torch.zeros_like(n_seg))
    mag_S = torch.zeros(rowptr.numel() - 1, dtype=torch.float64).index_add_(0, dst, a * G)
    return (k_S[dst] + 2 + 8) * U24 * a * (G + mag_S[dst])


# ------------------------------------------------------------------------------------------------------------- exact cases
def exact_case(gen, D, weighted=True, n_per_class=50):
    """dict(rowptr, col, attr, keep, s, z, dY, counts) on the generator's device (module docstring).  ``counts``: kept in-range
    entries per row."""
    dev = gen.device
    P = len(R.A_LEVELS)
    Ns = P * n_per_class
    s = torch.tensor(R.A_LEVELS, device=dev)[torch.arange(Ns, device=dev) % P].float().contiguous()
    rows = []                                                        # (kept, removed, out of range) entries per row
    for j, k in enumerate(EXACT_COUNTS):
        rows.append((k, (3 * j + 1) % 7, (2 * j) % 5))
    rows.insert(3, (0, 0, 0))                                        # an empty row
    rows.insert(8, (0, 5, 0))                                        # every entry removed
    rows.append((0, 0, 7))                                           # every entry out of range
    lengths = [a + b + c for a, b, c in rows]
    rowptr = R.rowptr_of(lengths, dev)
    E = int(rowptr[-1])
    col = torch.empty(E, dtype=torch.int64, device=dev)
    keep = torch.ones(E, dtype=torch.float32, device=dev)
    for r, (k, rem, oob) in enumerate(rows):
        n = k + rem + oob
        if n == 0:
            continue
        kind = torch.cat([torch.zeros(k), torch.ones(rem), torch.full((oob,), 2.0)]).to(dev)
        kind = kind[torch.randperm(n, generator=gen, device=dev)]
        pick = torch.randint(0, n_per_class, (n,), generator=gen, device=dev)
        own = r % P + P * pick                                       # a node of the row's own class
        other = (r + 1 + 2 * (r % 3)) % P + P * pick                 # removed entries: another class, a score far from the row's
        oor = torch.where(torch.arange(n, device=dev) % 2 == 0, torch.full((n,), -1, device=dev), Ns + pick)
        c = torch.where(kind == 0, own, torch.where(kind == 1, other, oor))
        beg = int(rowptr[r])
        col[beg:beg + n] = c
        keep[beg:beg + n] = (kind != 1).float()
    attr = None
    if weighted:
        attr = torch.randint(1, 4, (E,), generator=gen, device=dev).float() * (torch.randint(0, 2, (E,), generator=gen, device=dev) * 2 - 1).float()
    z = torch.randint(-3, 4, (Ns, D), generator=gen, device=dev).float()
    dY = torch.randint(-3, 4, (len(rows), D), generator=gen, device=dev).float()
    return dict(rowptr=rowptr, col=col.to(torch.int32).contiguous(), attr=attr, keep=keep.contiguous(), s=s, z=z, dY=dY,
                counts=[k for k, _, _ in rows])


def exact_alpha(case):
    """numpy float32 (E,): 2^-j on the kept in-range entries of a row with 2^j of them, 0 elsewhere."""
    rowptr, col, keep = case["rowptr"].cpu().numpy(), case["col"].cpu().numpy(), case["keep"].cpu().numpy()
    Ns = case["s"].numel()
    dst = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    ok = (col >= 0) & (col < Ns) & (keep != 0)
    k = np.bincount(dst[ok], minlength=len(rowptr) - 1)
    assert list(k) == list(case["counts"])
    with np.errstate(divide="ignore"):
        return np.where(ok, np.float32(1) / k.astype(np.float32)[dst], np.float32(0)).astype(np.float32)


def as_exact32(x64):
    """float32 numpy array of a float64 tensor whose every element is a float32 number (asserted)."""
    x = x64.numpy() if isinstance(x64, torch.Tensor) else np.asarray(x64)
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x), "the exact case left the float32 grid"
    return y


def exact_dlogit(case, p, seed):
    """(dlogit, g) as float32 numpy arrays: the float64 results, which are float32 numbers (module docstring)."""
    alpha = torch.from_numpy(exact_alpha(case))
    dl, (g, _) = edge_grad64(case["rowptr"], case["col"], case["attr"], alpha, case["dY"], case["z"], p, seed)
    return as_exact32(dl), as_exact32(g)


def reduce_case(gen, degrees=(1500, 0, 1, 64, 65, 300, 0, 4, 700, 3)):
    """(rowptr_t, eid, dlogit): a CSR by source with a hub, empty sources and integer dlogit in [-7, 7]; eid is a permutation."""
    dev = gen.device
    rowptr_t = R.rowptr_of(list(degrees), dev)
    E = int(rowptr_t[-1])
    eid = torch.randperm(E, generator=gen, device=dev).to(torch.int32).contiguous()
    return rowptr_t, eid, torch.randint(-7, 8, (E,), generator=gen, device=dev).float()


# --------------------------------------------------------------------------------------------------------------- emulators
def split_segments(rowptr, seg_len):
    """(segptr, row_of) numpy: rows cut into segments of at most seg_len entries, an empty row keeps one empty segment
    (native.SegmentedCSR._split); seg_len None: the rows themselves."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    if seg_len is None:
        return rowptr, np.arange(n)
    segptr, row_of = [], []
    for r in range(n):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        starts = list(range(b, e, seg_len)) or [b]
        segptr += starts
        row_of += [r] * len(starts)
    return np.array(segptr + [int(rowptr[-1])], dtype=np.int64), np.array(row_of, dtype=np.int64)


def sum32(v, order):
    """float32 sum of a 1-D float32 array in one of two orders: 'serial' (left to right) or 'tree' (pairwise halves)."""
    f = np.float32
    v = np.asarray(v, dtype=f)
    if len(v) == 0:
        return f(0)
    if order == "serial":
        acc = f(0)
        for x in v:
            acc = f(acc + x)
        return acc
    while len(v) > 1:
        if len(v) % 2:
            v = np.concatenate([v, np.zeros(1, dtype=f)])
        v = (v[0::2] + v[1::2]).astype(f)
    return v[0]


def emulate_masked_softmax(rowptr, col, attr, keep, s, segments=None, defect=None):
    """float32: graph_forms_ref.emulate_softmax over the kept entries (the three passes of the kernel); defect
    'removed_counted' leaves the removed entries in their groups."""
    col = np.asarray(col, dtype=np.int64)
    if keep is not None and defect != "removed_counted":
        col = np.where(np.asarray(keep) != 0, col, -1)
    alpha = R.emulate_softmax(rowptr, col, None, s, segments=segments)
    if keep is not None:
        alpha = np.where(np.asarray(keep) != 0, alpha, np.float32(0)).astype(np.float32)
    return alpha, alpha if attr is None else (np.asarray(attr, dtype=np.float32) * alpha).astype(np.float32)


def emulate_edge_grad(rowptr, col, attr, alpha, dY, z, p, seed, seg_len=None, order="serial", defect=None):
    """float32 numpy restatement of the three passes of ncf_gat_edge_grad over segments of ``seg_len``: every product, sum and
    difference rounded to float32, the sums taken in ``order`` (see sum32) over features, over a segment's entries and over a row's
    segments."""
    f = np.float32
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    alpha, dY, z = np.asarray(alpha, dtype=f), np.asarray(dY, dtype=f), np.asarray(z, dtype=f)
    E, (Nz, D) = len(col), z.shape
    segptr, row_of = split_segments(rowptr, seg_len)
    n_seg, n_rows = len(segptr) - 1, len(rowptr) - 1
    zz = z[np.clip(col, 0, Nz - 1)]
    if p > 0:
        mseed = seed + 1 if defect == "mask_not_regenerated" else seed
        zz = np.where(keep_mask(mseed, np.arange(E), D, p), (zz * scale32(p)).astype(f), f(0)).astype(f)
    live = (alpha != 0) & (col >= 0) & (col < Nz)
    g = np.zeros(E, dtype=f)
    segsum = np.zeros(n_seg, dtype=f)
    for sg in range(n_seg):
        r = row_of[sg]
        terms = []
        for e in range(segptr[sg], segptr[sg + 1]):
            if live[e]:
                d = sum32((dY[r] * zz[e]).astype(f), order)
                g[e] = d if attr is None else f(f(attr[e]) * d)
            terms.append(f(alpha[e] * g[e]))
        segsum[sg] = sum32(np.array(terms, dtype=f), order)
    S = np.zeros(n_rows, dtype=f)
    for r in range(n_rows):
        mine = np.nonzero(row_of == r)[0]
        if defect == "last_segment_dropped" and len(mine) > 1:
            mine = mine[:-1]
        S[r] = sum32(segsum[mine], order)
    out = np.zeros(E, dtype=f)
    for sg in range(n_seg):
        Sr = segsum[sg] if defect == "sum_per_segment" else S[row_of[sg]]
        sl = slice(segptr[sg], segptr[sg + 1])
        out[sl] = np.where(alpha[sl] != 0, (alpha[sl] * (g[sl] - Sr).astype(f)).astype(f), f(0))
    return out


def emulate_source_reduce(rowptr_t, eid, dlogit, seg_len=None, order="serial", defect=None):
    """float32: per segment of the CSR by source the sum of dlogit[eid[k]], then the segment sums per row, both in ``order``."""
    f = np.float32
    segptr, row_of = split_segments(rowptr_t, seg_len)
    vals = np.asarray(dlogit, dtype=f)[np.asarray(eid, dtype=np.int64)]
    part = np.array([sum32(vals[segptr[s]:segptr[s + 1]], order) for s in range(len(segptr) - 1)], dtype=f)
    out = np.zeros(len(rowptr_t) - 1, dtype=f)
    for r in range(len(out)):
        mine = np.nonzero(row_of == r)[0]
        if defect == "last_segment_dropped" and len(mine) > 1:
            mine = mine[:-1]
        out[r] = sum32(part[mine], order)
    return out
