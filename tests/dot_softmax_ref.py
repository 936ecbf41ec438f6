"""The contract of the full-catalogue softmax loss of a dot-product readout (csrc/dot_softmax.hip, include/ncf_abi.h) stated in
float64 torch on the host, the cases its GPU tests run, the tolerances, and the launch plans restated.

Exact scores.  The tables hold integer-valued fp32 numbers (entries in -4 .. 4) and the scale is a power of two, so every logit
z = scale * <a, q> is the same number in any order of summation: float64 logsumexp and float64 GEMMs over those z are the truth.
How many entries of a row are non-zero depends on (D, scale): the logits of a random case stay around |z| <= 40, where the ulp of
an fp32 log-sum-exp (<= 3.8e-6) stays inside the gradient tolerance below; the peaked case reaches |z| = 120 on purpose.

Tolerances.
  lse        |a - ref| <= 1e-5 |ref| + 1e-6 max|ref|              (tests/test_gpu_basic.py's assert_close, restated)
  gradients  |out - ref| <= (1e-5 + 2^-17) * sum_c |w64_rc * C_cd|  per entry: the lse bar carried into exp(z - lse), plus
             64 eps32 for the fp32 sum of n <= 4224 terms.  An entry whose terms are all zero must be zero.
The gradient bar is relative to the entry's own terms.  A softmax row whose probabilities are ALL far below fp32's normal range
but one (a peaked row whose target is the peak: every w is ~e^-100) has no fp32 answer inside it, so the peaked rows here keep
their target OFF the peak (their w at the peak and at the target are ~ +-g scale), and they sit among ordinary rows so that
every column's gradient keeps ordinary terms (a sum whose terms all lie below fp32's smallest number cannot be held to a bar
relative to those terms, so the builder gives every entry one term in the normal range); one peaked row keeps its target ON the peak with g = 0 (its lse and loss are checked,
its w is exactly zero).  The same holds in small for any target whose own probability is near 1: the builder keeps p_t <= 1/2,
except in the case "confident", where every target is its row's largest logit (p_t up to 1 - 1e-9) and the bar gains the absolute
term that the fp32 lse leaves on w_t, 2^-23 |lse| |g scale| |C_td| (reference()): three orders of magnitude below the |g scale C_td|
that a wrong sign or a dropped one-hot would show there.
"""
import functools

import numpy as np
import torch

GRAD_RTOL = 1e-5 + 2.0 ** -17
BLOCK = 64              # resident rows per workgroup (kDtBlockUsers)
MIN_TILE, TARGET_BLOCKS, PARTIAL_FLOATS = 64, 512, 8 << 20


# ------------------------------------------------------------------ the launch plans (csrc/dot_softmax.hip ds_plan), restated
def plan(kind, rows, cols, D):
    """(tile, tiles, chunk_rows) as native.dot_softmax_plan answers: the walk (the columns for "lse" / "grad_rows", the rows for
    "grad_items") starts as one power-of-two tile and is halved, down to 64, until resident blocks x tiles reaches 512; a split
    gradient walk takes its resident rows in chunks whose tiles x chunk x D partial floats stay within 8 Mi."""
    resident, walk = (cols, rows) if kind == "grad_items" else (rows, cols)
    rblocks = -(-resident // BLOCK)
    tile = MIN_TILE
    while tile < walk:
        tile *= 2
    while tile > MIN_TILE and rblocks * -(-walk // tile) < TARGET_BLOCKS:
        tile //= 2
    tiles = -(-walk // tile)
    chunk = resident
    if kind != "lse" and tiles > 1:
        chunk = min(resident, max(BLOCK, PARTIAL_FLOATS // (tiles * D) // BLOCK * BLOCK))
    return tile, tiles, chunk


def form(kind, rows, cols, D):
    """"one" / "multi" (tiles) and, for a gradient role, "+chunked" when the resident rows take more than one pass."""
    _, tiles, chunk = plan(kind, rows, cols, D)
    resident = cols if kind == "grad_items" else rows
    return ("one" if tiles == 1 else "multi") + ("+chunked" if chunk < resident else "")


# ------------------------------------------------------------------ the cases
# name: (B, N, D, ld pad, scale, idxA, idxB, targets, g, tables)
#   idxA   "rep": B picks of the user table with repeats, in permuted order; None: B = the table's rows
#   idxB   True: the catalogue is a permuted list of a larger item table
#   targets "rand" | "same" (every row one column) | "edges" (columns 0 and N - 1 alternate) | "argmax" (every row's largest
#          logit: the confident targets of a trained model, held to the bar with the absolute term below)
#   g      "mixed" (zeros, negatives, magnitudes 2^-6 .. 2^3) | "ones"
#   tables "rand" | "zero" | "peaked" | "unit" (both tables' rows are unit vectors e_{r mod D}: the indicator case, in both roles)
CASES = {
    "b1_n1_d1":           (1, 1, 1, 0, 1.0, None, False, "rand", "mixed", "rand"),
    "b15_n15_d17_ld":     (15, 15, 17, 1, 0.25, "rep", True, "rand", "mixed", "rand"),
    "b16_n16_d64":        (16, 16, 64, 0, 4.0, None, False, "edges", "mixed", "rand"),
    "b17_n17_d65_ld":     (17, 17, 65, 1, 1.0, "rep", False, "rand", "mixed", "rand"),
    "b64_n2047_d200":     (64, 2047, 200, 0, 0.25, None, True, "rand", "mixed", "rand"),
    "b65_n2048_d256_ld":  (65, 2048, 256, 1, 0.25, None, False, "rand", "ones", "rand"),
    "b130_n2049_d64":     (130, 2049, 64, 0, 1.0, "rep", False, "edges", "mixed", "rand"),
    "b130_n4100_d17":     (130, 4100, 17, 0, 4.0, "rep", True, "same", "mixed", "rand"),
    "b64_n16_d128":       (64, 16, 128, 0, 1.0, None, False, "rand", "mixed", "rand"),
    "peaked":             (65, 2049, 64, 0, 1.0, None, False, "rand", "mixed", "peaked"),
    "confident":          (65, 2049, 64, 0, 1.0, None, False, "argmax", "mixed", "rand"),
    "zero":               (17, 2047, 65, 1, 4.0, None, False, "rand", "mixed", "zero"),
    "unit":               (130, 4100, 17, 0, 1.0, None, False, "rand", "mixed", "unit"),
    "unit_d64":           (130, 2049, 64, 1, 0.25, "rep", True, "same", "mixed", "unit"),
    "chunked_d256":       (1100, 4100, 256, 0, 0.25, "rep", False, "rand", "mixed", "rand"),
}
# the form each case must take: (lse, grad_rows, grad_items); the CPU test holds the restated plan to the library's
FORMS = {
    "b1_n1_d1": ("one", "one", "one"), "b15_n15_d17_ld": ("one", "one", "one"), "b16_n16_d64": ("one", "one", "one"),
    "b17_n17_d65_ld": ("one", "one", "one"), "b64_n2047_d200": ("multi", "multi", "one"),
    "b65_n2048_d256_ld": ("multi", "multi", "multi"), "b130_n2049_d64": ("multi", "multi", "multi"),
    "b130_n4100_d17": ("multi", "multi", "multi"), "b64_n16_d128": ("one", "one", "one"), "peaked": ("multi", "multi", "multi"),
    "confident": ("multi", "multi", "multi"),
    "zero": ("multi", "multi", "one"), "unit": ("multi", "multi", "multi"), "unit_d64": ("multi", "multi", "multi"),
    "chunked_d256": ("multi", "multi+chunked", "multi+chunked"),
}


def _ints(shape, mag, density, rng):
    v = rng.integers(1, mag + 1, size=shape) * rng.choice([-1, 1], size=shape)
    return v * (rng.random(shape) < density)


class Case:
    """One case on the host: fp32 tables with their leading dimension, the index lists, targets, g, scale, and the float64 truth."""

    def __init__(self, name):
        B, N, D, pad, scale, idxA, idxB, targets, g, tables = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        self.name, self.B, self.N, self.D, self.scale = name, B, N, D, scale
        rowsA = B + 7 if idxA else B
        rowsB = N + 5 if idxB else N
        if tables == "zero":
            A, Q = np.zeros((rowsA, D), np.int64), np.zeros((rowsB, D), np.int64)
        elif tables == "unit":
            A, Q = np.zeros((rowsA, D), np.int64), np.zeros((rowsB, D), np.int64)
            A[np.arange(rowsA), np.arange(rowsA) % D] = 1
            Q[np.arange(rowsB), np.arange(rowsB) % D] = 1
        else:
            mag = 4 if scale <= 1 else 2                                  # entries in -mag .. mag: one shared coordinate moves z by <= 16
            ea2 = sum(k * k for k in range(1, mag + 1)) / mag             # E a^2 of a non-zero entry
            density = min(1.0, 6.0 / (scale * ea2 * np.sqrt(D)))          # std of z about 6
            A, Q = _ints((rowsA, D), mag, density, rng), _ints((rowsB, D), mag, density, rng)
        self.idxA = rng.integers(0, rowsA, size=B) if idxA else None
        if idxA:
            self.idxA[-1] = self.idxA[0]                                  # at least one repeat
        self.idxB = rng.permutation(rowsB)[:N] if idxB else None
        ia = self.idxA if idxA else np.arange(B)
        ib = self.idxB if idxB else np.arange(N)
        if targets == "rand":
            t = rng.integers(0, N, size=B)
        elif targets == "same":
            t = np.full(B, N // 3)
        elif targets == "argmax":
            t = (A[ia] @ Q[ib].T).argmax(1)
        else:
            t = np.where(np.arange(B) % 2 == 0, 0, N - 1)
        self.peaked_rows = np.zeros(0, np.int64)
        if tables == "peaked":
            # every third listed row is peaked: the k-th of them is the user row 4 e_k, and column (7 b) mod N is the item row
            # 30 e_k: z = 120 there and |z| <= 16 at every other column, so the largest logit leads by >= 104.  The other user
            # rows keep coordinates 0 .. K - 1 within -1 .. 1 (|z| <= 30 + the rest at a peak column).
            self.peaked_rows = np.arange(0, B, 3)
            K = len(self.peaked_rows)
            assert K <= D
            peaks = (7 * self.peaked_rows) % N
            A[:, :K] = np.clip(A[:, :K], -1, 1)
            A[self.peaked_rows], Q[peaks] = 0, 0
            A[self.peaked_rows, np.arange(K)] = 4
            Q[peaks, np.arange(K)] = 30
            t[self.peaked_rows] = (peaks + 1) % N                         # the target OFF the peak (see the module docstring)
            # every checked entry keeps a term in fp32's normal range: a peaked row's w is ~e^-100 (below fp32's smallest
            # number) except at its peak and its target, so its target's item row has no zero entry, and one ordinary user row
            # (row 1, g = -1) has none either, which gives every entry of dQ an ordinary term
            Q[t[self.peaked_rows]] = rng.choice([-2, -1, 1, 2], size=(K, D))
            A[1] = rng.choice([-1, 1], size=D)
            t[self.peaked_rows[-1]] = peaks[-1]                           # ... but one, for the lse alone
            self.peak_target_row = int(self.peaked_rows[-1])
        if g == "ones":
            gv = np.ones(B)
        else:
            gv = np.array([0.0, -1.0, 1.0, 2.0 ** -6, -8.0, 0.5, 3.0])[np.arange(B) % 7]
            if B == 1:
                gv = np.array([-1.5])
        # A target's own probability stays <= 1/2 (the module docstring): w_t = g scale (p_t - 1) is a difference of fp32 numbers
        # near 1 otherwise, with an absolute error of eps32 * lse that the entry's own terms, ~ (1 - p_t), no longer cover.  A
        # random target on such a column moves to the next one; a row that cannot move (one column; a fixed target; the peaked
        # row kept on its peak for the lse's sake) gets g = 0, where every w is exactly 0 on both sides.
        z0 = (torch.from_numpy(A[ia]).double() @ torch.from_numpy(Q[ib]).double().t()) * scale
        p0 = torch.softmax(z0, 1).numpy()
        for b in range(B):
            if targets == "argmax":
                continue                                                   # the confident case: its bar carries the absolute term
            fixed = targets != "rand" or N == 1 or (tables == "peaked" and b == self.peaked_rows[-1])
            while p0[b, t[b]] > 0.5 and not fixed:
                t[b] = (t[b] + 1) % N
            if p0[b, t[b]] > 0.5:
                gv[b] = 0.0
        self.A = torch.zeros((rowsA, D + pad), dtype=torch.float32)
        self.A[:, :D] = torch.from_numpy(A).float()
        self.Q = torch.zeros((rowsB, D + pad), dtype=torch.float32)
        self.Q[:, :D] = torch.from_numpy(Q).float()
        if pad:
            self.A[:, D:], self.Q[:, D:] = 1e30, -1e30                    # what lies past D is never read as data
        self.t = torch.from_numpy(t.astype(np.int64))
        self.g = torch.from_numpy(gv).float()
        # ---- the truth
        U, V = torch.from_numpy(A[ia]).double(), torch.from_numpy(Q[ib]).double()
        self.ref = reference(U, V, self.t, self.g.double(), scale)
        z = self.ref["z"]
        assert float(z.abs().max()) <= 120.0, float(z.abs().max())
        if tables == "peaked":
            assert gv[1] != 0
            top2 = torch.topk(z[self.peaked_rows], 2, dim=1).values
            assert float((top2[:, 0] - top2[:, 1]).min()) >= 100.0 and float(top2[:, 0].max()) == 120.0

    def tables(self, dev):
        """(A view (rowsA, D) with its leading dimension, Q view, idxA, idxB, targets, g) on ``dev``."""
        on = lambda x: None if x is None else (x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, dtype=np.int64))).to(dev)
        return on(self.A)[:, :self.D], on(self.Q)[:, :self.D], on(self.idxA), on(self.idxB), on(self.t), on(self.g)


def reference(U, V, t, g, scale):
    """float64: the logits z (B, N) of user rows U against item rows V, lse, the per-row loss, w, both gradients and the sums of
    absolute terms their tolerances are stated in."""
    B = U.shape[0]
    z = (U @ V.t()) * scale
    lse = torch.logsumexp(z, 1)
    onehot = torch.zeros_like(z)
    onehot[torch.arange(B), t] = 1.0
    w = (g * scale)[:, None] * (torch.exp(z - lse[:, None]) - onehot)
    # the absolute term of a confident target: w_t = g scale (p_t - 1) is computed from p_t = exp(z_t - lse) in fp32, and lse's own
    # rounding (<= 2^-24 |lse|) plus that of the difference z_t - lse (<= 2^-24 |lse|, as |z_t - lse| <= |lse| there) move p_t, and
    # so w_t, by up to 2^-23 |lse| |g scale| whatever 1 - p_t is; entry d of the row's (the target column's) gradient moves by that
    # times |C_td|
    dev_t = 2.0 ** -23 * lse.abs() * (g * scale).abs()
    return {"z": z, "lse": lse, "loss": lse - z[torch.arange(B), t], "w": w, "dA": w @ V, "dQ": w.t() @ U,
            "absA": w.abs() @ V.abs(), "absQ": w.abs().t() @ U.abs(),
            "confA": dev_t[:, None] * V[t].abs(), "confQ": (onehot * dev_t[:, None]).t() @ U.abs()}


@functools.lru_cache(None)
def case(name):
    return Case(name)


def lse_close(a, ref):
    a, ref = a.detach().cpu().double(), ref.double()
    tol = 1e-5 * ref.abs() + 1e-6 * ref.abs().max()
    diff = (a - ref).abs()
    k = int((diff / tol.clamp_min(1e-300)).argmax())
    print(f"  lse: worst |diff| {float(diff.flatten()[k]):.3e} of tol {float(tol.flatten()[k]):.3e}")
    assert bool((diff <= tol).all()), (float(diff.flatten()[k]), float(tol.flatten()[k]))


def grad_close(out, ref, abs_terms, what, rtol=GRAD_RTOL, confident=None):
    """``confident``: the absolute term of the confident case (reference()'s confA / confQ), added to the bar."""
    out, ref = out.detach().cpu().double(), ref.double()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    tol = rtol * abs_terms + (0.0 if confident is None else confident)
    diff = (out - ref).abs()
    used = diff / tol.clamp_min(1e-300)
    k = int(used.argmax())
    print(f"  {what}: worst |diff| {float(diff.flatten()[k]):.3e} of tol {float(tol.flatten()[k]):.3e} (ref {float(ref.flatten()[k]):.3e})")
    assert bool((diff <= tol).all()), (what, float(diff.flatten()[k]), float(tol.flatten()[k]))
