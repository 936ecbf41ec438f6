"""Case tables and references for the graph propagation kernels (csrc/spmm.hip: ncf_spmm_csr, ncf_edge_softmax_csr,
ncf_edge_softmax_segmented, ncf_degree_accumulate, ncf_edge_coef, ncf_scale_rows), native.SegmentedCSR and PreparedGraph.
No GPU needed: the torch functions take tensors on any device, the float32 recipes and the emulators are numpy.

THE CASE TABLE (TREE_CASES).  SegmentedCSR splits rows longer than ``seg_len`` entries into segments and finishes split rows by
re-applying the segment kernel to the partial sums with ``fan``-wide segments, level after level.  Each row of the table names
row lengths, (seg_len, fan) and the number of levels the split rule must give, so that a later change of the rule cannot
silently move a case.  TREE_LENGTHS = [9, 0, 1, 4, 5, 8, 16, 17, 0, 64, 65, 1500, 3, 33] has empty rows, rows of exactly
seg_len, seg_len + 1, fan and fan + 1 segments, and one hub row:

    (seg_len, fan)   segments of the hub row, level by level                      levels
    (4, 2)           375 188 94 47 24 12 6 3 2 1                                   10
    (4, 4)           375 94 24 6 2 1                                               6
    (8, 3)           188 63 21 7 3 1                                               6
    (64, 4)          24 6 2 1                                                      4
    (512, 64)        3 1                                                           2

At (4, 2) and (4, 4) the first row is split; at (64, 4) and (512, 64) the first and the last row are whole while another row is
split (the ``s == 0`` / ``s == n_seg - 1`` guards decide).  [9, 9] at (4, 2): three levels, first and last row both split, every
row split.  [1, 2, 3, 0]: one level, ``row_of is None``.  [0, 0, 0] and a matrix without rows: nothing to add.

THE SpMM REFERENCES.
* Exact.  z, coef and the initial y / acc_sum are integers in [-7, 7] stored as fp32.  Every partial sum of a row with n
  entries is an integer of magnitude <= 49 n + 7 < 2^24 for every row here (n <= 300 000), so every order of summation, every
  split into segments and every tree shape gives the same fp32 value: the int64 result is the expected output bit for bit.  The
  messages are formed in float64 (exact far beyond these magnitudes) and returned as int64; the CPU tests hold that route to
  an int64 ``index_add_``.  Entries whose ``col`` is outside [0, Nz) are skipped; an empty row is 0.
* Bound.  Random N(0,1) data against float64: |y - ref| <= (n_r + 8) 2^-24 sum_e |coef_e z_e| per element of a row with n_r
  entries.  Every accumulation is one fma (the product is not rounded), so on the path from a product to the output there is
  one rounding when the product enters its lane's accumulator and one per later add of two non-zero partial sums: lane by
  lane, in the cross-lane butterfly, in every level of the tree or in the serial fix-up.  A binary summation tree with n_r
  leaves has n_r - 1 such adds, adds of an exact 0 (idle lanes, skipped entries) do not round, and the fused layer
  accumulator adds once more: at most n_r + 1 roundings to nearest (u = 2^-24) on any path, and the standard bound
  gamma_n = n u / (1 - n u) <= (n + 8) u holds for every order of summation at these n.  For acc_sum the magnitude gains
  |acc_sum_0|.  An empty row has bound 0 and must be exactly 0.

THE SOFTMAX REFERENCES.  out[e] = attr[e] * exp(s[col[e]] - M_r) / (sum_r exp(s[col[.]] - M_r) + 1e-16), M_r the row maximum.
* Exact.  (a) scores constant within a row (different from row to row, +-3e4 among them): every difference is 0, exp(0) = 1,
  the sums are integer counts and the weight is fl32(1 / k), k the number of in-range entries; 1e-16 vanishes against k >= 1.
  (b) two levels {c, c - 200} with c a small integer: the low entries are exp(-200) = 0 exactly (far below the smallest
  denormal), the high ones fl32(1 / k_high).  In the segmented form a segment that holds low entries only has local maximum
  c - 200 and its factor exp(m_seg - M) = exp(-200) is exactly 0; a row whose segments all hold a high entry has factors
  exactly 1.  With ``attr`` the result is one more correctly rounded product.  Out-of-range ``col`` entries (-1, >= Ns) are 0
  and do not count in k; a row whose entries are all out of range is all 0 (and finite); an empty row has nothing to write.
  The expectation is numpy float32 and compared bitwise, for the row form and the segmented form alike.
  ASSUMPTIONS, read from the compiled code (no fast-math: full divide and square-root sequences, denormals kept) and first
  measured by the GPU tests: expf(0) == 1 and expf(-200) == 0 on the device, a / b and sqrtf(x) correctly rounded.
* Bound.  Random scores against the float64 definition, per element: |out - ref| <= RTOL (|ref| + FLOOR max_row |ref|), the
  project's 1e-5 bar with its floor taken from the element's own row.  fp32 model of the relative error of one weight, in
  units of u = 2^-24, with S the score spread (max - min) of the row, n its length and expf within 1 ulp = 2 u:
    numerator     exp(fl(s - M)): the rounded difference moves the exponent by <= u |s - M|      S + 2
    denominator   the same per term (a weighted mean of the terms' errors, <= the worst),
                  the lane-serial sum of ceil(n / 64) terms and a 6-step butterfly                S + 2 + ceil(n / 64) + 6
    segmented     one more expf(m_seg - M) and product per segment, the row-level sum             S + 3 + ceil(n_seg / 64) + 6
    quotient, attr product (correctly rounded)                                                    2
  ``softmax_model_ulps`` adds these up; the bounded cases are sized (S <= 24, n <= 3000) so that the model's worst case stays
  under RTOL = 167 u.  The model is a sizing aid only: the observed fraction of the bar is what the tests record.

edge_coef AND scale_rows.  numpy float32, operation by operation: inv(d) = 1 / sqrt(d) or 0 for d <= 0, inv(deg[src]) *
inv(deg[dst]) (0 when either id is outside [0, N)), times attr, and x / divisor; compared bitwise under the assumptions above.

THE EMULATORS (tests only).  ``emulate_tree`` / ``emulate_fixup`` restate the segment walk of spmm_seg_kernel (a segment that
is the first AND the last of its row stores y and adds acc_sum, any other stores its partial sum), SegmentedCSR.spmm's level
loop and the ordered serial fix-up, from the kernel's header comment; ``emulate_softmax`` restates the three passes of the
segmented softmax (and, with segments == rows, the row form) in float32.  Each takes a ``defect``; the CPU tests show that the
exact checks reject every one of them, and that the earlier bar (assert_close at its defaults) let some of them pass.
"""
from collections import namedtuple

import numpy as np
import torch

U24 = 2.0 ** -24
INT_RANGE = 7
RTOL = 1e-5              # the project's fp32 bar (tests/test_gpu_basic.py, assert_close at its defaults) ...
FLOOR = 0.1              # ... with its absolute part: a tenth of the relative bar on the largest weight of the row
WAVE_CAP = 16384 * 4     # spmm_seg_kernel, the softmax kernels: 16 384 blocks of 4 waves, one segment / row per wave
THREAD_CAP = 8192 * 256  # degree, edge_coef, scale_rows: 8 192 blocks of 256 threads, one element per thread
MAX_ROW = 300_000        # longest row of any exact case: 49 * MAX_ROW + 7 < 2^24

TREE_LENGTHS = [9, 0, 1, 4, 5, 8, 16, 17, 0, 64, 65, 1500, 3, 33]
TreeCase = namedtuple("TreeCase", "lengths seg_len fan levels")
TREE_CASES = [
    TreeCase(TREE_LENGTHS, 4, 2, 10),
    TreeCase(TREE_LENGTHS, 4, 4, 6),
    TreeCase(TREE_LENGTHS, 8, 3, 6),
    TreeCase(TREE_LENGTHS, 64, 4, 4),
    TreeCase(TREE_LENGTHS, 512, 64, 2),
    TreeCase([9, 9], 4, 2, 3),
    TreeCase([1, 2, 3, 0], 4, 2, 1),
    TreeCase([0, 0, 0], 4, 2, 1),
    TreeCase([], 4, 2, 1),
]
# row lengths around EPI * UNROLL = 32 / 16 / 8 / 4 entries per wave step of LPR 8 / 16 / 32 / 64
PLAIN_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 3, 4, 5, 0, 7, 8, 9, 31, 32, 33, 127, 128, 129, 300, 2]
PLAIN_WIDTHS = [4, 32, 36, 64, 68, 100, 128, 132, 256]


def tree_id(c):
    name = "table" if c.lengths is TREE_LENGTHS else "x".join(map(str, c.lengths)) or "norows"
    return f"{name}-seg{c.seg_len}-fan{c.fan}"


def lanes_per_row(D):
    """LPR of the instantiation spmm_impl picks for width D."""
    chunks = D // 4
    return 8 if chunks <= 8 else 16 if chunks <= 16 else 32 if chunks <= 32 else 64


# ------------------------------------------------------------------------------------------------------------- graphs
def rowptr_of(lengths, device="cpu"):
    rp = torch.zeros(len(lengths) + 1, dtype=torch.int64, device=device)
    if len(lengths):
        rp[1:] = torch.cumsum(torch.as_tensor(lengths, dtype=torch.int64, device=device), 0)
    return rp


def rows_of(rowptr):
    """Destination row of every CSR entry."""
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def draw_cols(E, Nz, gen, bad=True):
    """int32 source ids in [0, Nz); with ``bad`` every 37th entry is -1 and every 41st is Nz or Nz + 5 (skipped by the kernels)."""
    col = torch.randint(0, Nz, (E,), generator=gen, device=gen.device).to(torch.int32)
    if bad and E:
        pos = torch.arange(E, device=gen.device)
        col[pos % 37 == 36] = -1
        col[pos % 41 == 40] = Nz
        col[pos % 82 == 81] = Nz + 5
    return col


def int_tensor(shape, gen):
    return torch.randint(-INT_RANGE, INT_RANGE + 1, shape, generator=gen, device=gen.device).float()


def int_problem(lengths, Nz, D, gen, bad=True, all_bad_row=None):
    """(rowptr, col, coef, z, y0, acc0) of integer-valued operands; ``all_bad_row``: a row whose entries are all out of range."""
    rowptr = rowptr_of(lengths, gen.device)
    E, N = int(rowptr[-1]), len(lengths)
    col = draw_cols(E, Nz, gen, bad)
    if all_bad_row is not None:
        col[int(rowptr[all_bad_row]):int(rowptr[all_bad_row + 1])] = -1
    return rowptr, col, int_tensor((E,), gen), int_tensor((Nz, D), gen), int_tensor((N, D), gen), int_tensor((N, D), gen)


# ---------------------------------------------------------------------------------------------------- SpMM references
def _messages64(rowptr, col, coef, z):
    Nz = z.shape[0]
    ok = (col >= 0) & (col < Nz)
    msg = z.double()[col.long().clamp(0, max(Nz - 1, 0))]
    if coef is not None:
        msg = msg * coef.double()[:, None]
    return torch.where(ok[:, None], msg, torch.zeros_like(msg))


def spmm_reference64(rowptr, col, coef, z):
    """(N, D) float64: y[r] = sum over the entries e of row r with col[e] in [0, Nz) of coef[e] * z[col[e]]."""
    N = rowptr.numel() - 1
    return torch.zeros((N, z.shape[1]), dtype=torch.float64, device=z.device).index_add_(0, rows_of(rowptr), _messages64(rowptr, col, coef, z))


def exact_spmm_reference(rowptr, col, coef, z):
    """int64 (N, D) for integer-valued operands (module docstring)."""
    lengths = rowptr[1:] - rowptr[:-1]
    assert lengths.numel() == 0 or int(lengths.max()) <= MAX_ROW
    assert INT_RANGE * INT_RANGE * MAX_ROW + INT_RANGE < 2 ** 24
    return spmm_reference64(rowptr, col, coef, z).round().long()


def exact_equal(out, ref_int):
    """The fp32 tensor holds the integer reference, element for element."""
    return out.shape == ref_int.shape and out.dtype == torch.float32 and torch.equal(out.double(), ref_int.double().to(out.device))


def spmm_bound(rowptr, col, coef, z, acc0=None):
    """(N, D) float64: (n_r + 8) 2^-24 (sum_e |coef_e z_e| [+ |acc0|])."""
    N = rowptr.numel() - 1
    mag = torch.zeros((N, z.shape[1]), dtype=torch.float64, device=z.device).index_add_(0, rows_of(rowptr), _messages64(rowptr, col, coef, z).abs())
    if acc0 is not None:
        mag = mag + acc0.double().abs()
    n_r = (rowptr[1:] - rowptr[:-1]).double()[:, None]
    return (n_r + 8) * U24 * mag


def bound_check(out, ref, bound):
    """(ok, worst fraction of the bound used, error there, bound there, max error / max |ref|); a zero bound asks for exactness."""
    err = (out.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if err.numel() == 0:
        return True, 0.0, 0.0, 0.0, 0.0
    used = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    k = int(used.argmax())
    return (bool((err <= bound).all()), float(used.flatten()[k]), float(err.flatten()[k]), float(bound.flatten()[k]),
            float(err.max()) / max(float(ref.abs().max()), 1e-300))


# ------------------------------------------------------------------------------------------------- softmax references
def softmax_reference64(rowptr, col, attr, s):
    """(E,) float64 on the tensors' device: the PyG definition per destination row; out-of-range entries are 0."""
    N, Ns, E = rowptr.numel() - 1, s.numel(), col.numel()
    dev = s.device
    dst = rows_of(rowptr)
    ok = (col >= 0) & (col < Ns)
    sc = torch.where(ok, s.double()[col.long().clamp(0, max(Ns - 1, 0))], torch.full((E,), -float("inf"), dtype=torch.float64, device=dev))
    mx = torch.full((N,), -float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, dst, sc, reduce="amax", include_self=True)
    ex = torch.where(ok, torch.exp(sc - mx[dst]), torch.zeros(E, dtype=torch.float64, device=dev))
    den = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, dst, ex)
    ref = ex / (den[dst] + 1e-16)
    return ref if attr is None else ref * attr.double()


def softmax_bar(rowptr, ref):
    """Per element RTOL (|ref| + FLOOR * the largest |ref| of the element's own row)."""
    N = rowptr.numel() - 1
    dst = rows_of(rowptr)
    row_max = torch.zeros(N, dtype=torch.float64, device=ref.device).scatter_reduce(0, dst, ref.abs(), reduce="amax", include_self=True)
    return RTOL * (ref.abs() + FLOOR * row_max[dst])


def softmax_model_ulps(spread, n_row, seg_len=None):
    """Worst relative error of one weight in units of 2^-24 under the module docstring's model."""
    num = spread + 2
    if seg_len is None:
        den = spread + 2 + -(-n_row // 64) + 6
    else:
        n_seg = -(-n_row // seg_len)
        den = spread + 2 + -(-min(n_row, seg_len) // 64) + 6 + spread + 3 + -(-n_seg // 64) + 6
    return num + den + 2


def exact_softmax_expected(rowptr, col, attr, s):
    """numpy float32 (E,): fl32(1 / k) on the in-range entries at the row maximum, 0 elsewhere, times attr.  Every other in-range
    entry must sit exactly 200 below its row's maximum (cases (a) and (b) of the module docstring)."""
    rowptr, col, s = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(s, dtype=np.float32)
    N, Ns = len(rowptr) - 1, len(s)
    dst = np.repeat(np.arange(N), np.diff(rowptr))
    ok = (col >= 0) & (col < Ns)
    sc = np.where(ok, s[np.clip(col, 0, max(Ns - 1, 0))], -np.inf).astype(np.float32)
    M = np.full(N, -np.inf, dtype=np.float32)
    np.maximum.at(M, dst[ok], sc[ok])
    high = ok & (sc == M[dst])
    low = ok & ~high
    assert np.all(sc[low] == M[dst][low] - np.float32(200))
    k = np.bincount(dst[high], minlength=N).astype(np.float32)
    assert k.max(initial=0) < 2 ** 24
    with np.errstate(divide="ignore"):
        w = np.float32(1) / k
    out = np.where(high, w[dst], np.float32(0)).astype(np.float32)
    return out if attr is None else (np.asarray(attr, dtype=np.float32) * out).astype(np.float32)


A_LEVELS = [3.0, -3e4, 0.0, 3e4, -1.5, 17.0, 1e4, -1e4]      # case (a): one score per row, row r takes level r % 8
B_CENTRES = [0.0, 3.0, -2.0, 5.0]                             # case (b): row r has high level c = B_CENTRES[r % 4], low c - 200


def softmax_case(kind, lengths, gen, block=64, n_per_class=50, weighted=True):
    """Exact softmax case on the generator's device: dict(rowptr, col, attr, s).  Source node n belongs to class n % P; a row
    reads nodes of its own class(es) only, so its scores are constant ("a") or on two levels 200 apart ("b").
    In "b" the entries of a row go in blocks of ``block`` (the segment length of the segmented form): block g of row r is all
    low when (g + r) % 3 == 1 and the row has another block, otherwise it alternates high / low starting high; rows with
    r % 5 == 4 are all high (every segment shares the maximum).  Entries -1 and >= Ns are mixed in; rows with r % 11 == 7 are
    all out of range."""
    dev = gen.device
    rowptr = rowptr_of(lengths, dev)
    E, N = int(rowptr[-1]), len(lengths)
    dst = rows_of(rowptr)
    local = torch.arange(E, device=dev) - rowptr[dst]
    pick = torch.randint(0, n_per_class, (E,), generator=gen, device=dev)
    if kind == "a":
        P = len(A_LEVELS)
        Ns = P * n_per_class
        s = torch.tensor(A_LEVELS, device=dev)[torch.arange(Ns, device=dev) % P]
        col = dst % P + P * pick
    else:
        P = 2 * len(B_CENTRES)
        Ns = P * n_per_class
        cls = torch.arange(Ns, device=dev) % P
        s = torch.tensor(B_CENTRES, device=dev)[cls // 2] - 200.0 * (cls % 2).float()
        g = local // block
        n_blocks = (rowptr[1:] - rowptr[:-1] + block - 1) // block
        low = torch.where(((g + dst) % 3 == 1) & (n_blocks[dst] > 1), torch.ones_like(local), local % 2)
        low = torch.where(dst % 5 == 4, torch.zeros_like(low), low)
        col = 2 * (dst % len(B_CENTRES)) + low + P * pick
    col = col.to(torch.int32)
    pos = torch.arange(E, device=dev)
    col[pos % 29 == 28] = -1
    col[pos % 31 == 30] = Ns
    col[pos % 62 == 61] = Ns + 9
    col[dst % 11 == 7] = -1
    attr = (torch.randn(E, generator=gen, device=dev) if weighted else None)
    return dict(rowptr=rowptr, col=col, attr=attr, s=s.float().contiguous())


def seg_first_of(row_of, n_rows):
    return torch.searchsorted(row_of.to(torch.int64), torch.arange(n_rows + 1, device=row_of.device)).contiguous()


# ------------------------------------------------------------------------------------------- edge_coef and scale_rows
def edge_coef_expected(src, dst, attr, deg):
    """numpy float32 (E,), operation by operation as edge_coef_kernel."""
    src, dst, deg = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), np.asarray(deg, dtype=np.float32)
    N = len(deg)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(deg > 0, np.float32(1) / np.sqrt(deg), np.float32(0)).astype(np.float32)
    ok = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    norm = np.where(ok, inv[np.clip(src, 0, N - 1)] * inv[np.clip(dst, 0, N - 1)], np.float32(0)).astype(np.float32)
    return norm if attr is None else (np.asarray(attr, dtype=np.float32) * norm).astype(np.float32)


def scale_rows_expected(x, divisor):
    return (np.asarray(x, dtype=np.float32) / np.float32(divisor)).astype(np.float32)


def passes_assert_close(a, ref):
    """The earlier bar: test_gpu_basic.assert_close at its defaults, |a - ref| <= 1e-5 |ref| + 1e-6 max |ref|."""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return bool(((a - ref).abs() <= RTOL * ref.abs() + FLOOR * RTOL * ref.abs().max()).all())


def same_bits(a, b):
    """Two float32 arrays / tensors hold the same bits."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# --------------------------------------------------------------------------------------------------------- emulators
SPMM_DEFECTS = ["drop_last_entry", "tail_overread", "partial_twice", "middle_row_unwritten", "acc_on_two_levels", "no_edge_guards"]
SOFTMAX_DEFECTS = ["segment_max_no_rescale", "oob_counted"]


def levels_to_numpy(levels):
    return [tuple(None if t is None else t.cpu().numpy() for t in lv) for lv in levels]


def _edge_flags(row_of, s, n_seg, defect):
    """first / last of spmm_seg_kernel.  Without the guards the kernel would read row_of[-1] / row_of[n_seg]; the emulated bad read
    returns the segment's own row (what memory holds there is anyone's guess; this is the value that does harm)."""
    if row_of is None:
        return s, True, True
    row = int(row_of[s])
    guards = defect != "no_edge_guards"
    prev = int(row_of[s - 1]) if s > 0 else (None if guards else row)
    nxt = int(row_of[s + 1]) if s < n_seg - 1 else (None if guards else row)
    return row, prev != row, nxt != row


def emulate_seg_pass(segptr, row_of, col, coef, z, y, acc, partial, level=0, last_level=0, defect=None):
    """One launch of spmm_seg_kernel over float64 numpy arrays (exact for the integer cases); y, acc and partial are updated in
    place.  ``level`` / ``last_level``: where this launch sits in SegmentedCSR.spmm's loop (only the defects look at them)."""
    n_seg, Nz = len(segptr) - 1, z.shape[0]
    for s in range(n_seg):
        beg, end = int(segptr[s]), int(segptr[s + 1])
        idx = np.arange(beg, end)
        if level == 0 and defect == "drop_last_entry" and end > beg:
            idx = idx[:-1]
        if level == 0 and defect == "tail_overread" and (end - beg) % 16 and end < len(col):
            idx = np.arange(beg, end + 1)
        if level > 0 and defect == "partial_twice" and end - beg >= 2:
            idx = np.concatenate([idx[:1], idx])
        c = col[idx].astype(np.int64)
        ok = (c >= 0) & (c < Nz)
        w = np.ones(len(idx)) if coef is None else coef[idx].astype(np.float64)
        val = (w[ok, None] * z[c[ok]]).sum(0)
        row, first, last = _edge_flags(row_of, s, n_seg, defect)
        if first and last:
            if defect == "middle_row_unwritten" and 0 < level < last_level:
                continue
            y[row] = val
            if acc is not None:
                acc[row] += val
        elif partial is not None:
            partial[s] = val
            if defect == "acc_on_two_levels" and first and acc is not None:
                acc[row] += val


def emulate_tree(levels, col, coef, z, y, acc, defect=None):
    """SegmentedCSR.spmm over ``levels`` (numpy, see levels_to_numpy).  Partial buffers start as NaN: a read of a slot that no
    launch wrote poisons the row."""
    D = z.shape[1]
    segptr, row_of, _ = levels[0]
    last = len(levels) - 1
    if last == 0:
        emulate_seg_pass(segptr, row_of, col, coef, z, y, acc, None, 0, 0, defect)
        return y
    bufs = [np.full((len(lv[0]) - 1, D), np.nan) for lv in levels[:-1]]
    emulate_seg_pass(segptr, row_of, col, coef, z, y, acc, bufs[0], 0, last, defect)
    for li in range(1, len(levels)):
        segptr, row_of, edge_ids = levels[li]
        emulate_seg_pass(segptr, row_of, edge_ids, None, bufs[li - 1], y, acc, None if li == last else bufs[li], li, last, defect)
    return y


def emulate_fixup(segptr, row_of, col, coef, z, y, acc, defect=None):
    """ncf_spmm_csr with row_of and fixup = 1: the segment kernel, then spmm_fix_kernel (the lane group of a split row's first
    segment adds the row's partial sums in segment order).  Returns the partial buffer."""
    n_seg = len(segptr) - 1
    partial = np.full((n_seg, z.shape[1]), np.nan)
    emulate_seg_pass(segptr, row_of, col, coef, z, y, acc, partial, 0, 0, defect)
    for s in range(n_seg):
        row, first, last = _edge_flags(row_of, s, n_seg, defect)
        if not first or last:
            continue
        tot = np.zeros(z.shape[1])
        t = s
        while t < n_seg and row_of[t] == row:
            tot = tot + partial[t]
            t += 1
        if defect == "partial_twice":
            tot = tot + partial[s]
        y[row] = tot
        if acc is not None:
            acc[row] += tot
    return partial


def emulate_softmax(rowptr, col, attr, s, segments=None, defect=None):
    """float32 numpy restatement of the three passes (segment statistics, row statistics, apply); ``segments`` = (segptr, row_of)
    or None for the row form (every row one segment).  Entries of the output that no pass writes stay NaN (there are none: every
    entry belongs to a segment)."""
    f = np.float32
    rowptr, col, s = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(s, dtype=f)
    n_rows, Ns, E = len(rowptr) - 1, len(s), len(col)
    segptr, row_of = (rowptr, np.arange(n_rows)) if segments is None else (np.asarray(segments[0], dtype=np.int64), np.asarray(segments[1], dtype=np.int64))
    n_seg = len(segptr) - 1
    ok = (col >= 0) & (col < Ns)
    sc = np.where(ok, s[np.clip(col, 0, max(Ns - 1, 0))], -np.inf).astype(f)
    segm, segl = np.full(n_seg, -np.inf, dtype=f), np.zeros(n_seg, dtype=f)
    for g in range(n_seg):
        v = sc[segptr[g]:segptr[g + 1]][ok[segptr[g]:segptr[g + 1]]]
        if len(v):
            segm[g] = v.max()
            segl[g] = np.exp(v - segm[g]).astype(f).sum(dtype=f)
        if defect == "oob_counted":
            segl[g] += f(np.count_nonzero(~ok[segptr[g]:segptr[g + 1]]))
    rowm, rowl = np.full(n_rows, -np.inf, dtype=f), np.zeros(n_rows, dtype=f)
    np.maximum.at(rowm, row_of, segm)
    for g in range(n_seg):
        if segm[g] != -np.inf:
            factor = f(1) if defect == "segment_max_no_rescale" else np.exp(segm[g] - rowm[row_of[g]]).astype(f)
            rowl[row_of[g]] += segl[g] * factor
    den = rowl + f(1e-16)
    out = np.full(E, np.nan, dtype=f)
    for g in range(n_seg):
        sl = slice(segptr[g], segptr[g + 1])
        with np.errstate(invalid="ignore", over="ignore"):
            a = np.where(ok[sl], np.exp(sc[sl] - rowm[row_of[g]]).astype(f) / den[row_of[g]], f(0)).astype(f)
        out[sl] = a if attr is None else np.asarray(attr, dtype=f)[sl] * a
    return out
