"""numpy restatement of ncf_slim_solve (csrc/slim.hip; THE CONTRACT in include/ncf_abi.h): the serial cyclic coordinate descent of one
column as explicit fp32 scalar operations (``solve_col``), the screened form of the same loop with any width T, which is what the
kernel runs and what the tests use where the scalar loop is too slow (``solve_col_screened``; tests/test_slim_cpu.py holds the two
to each other bit for bit), float64 KKT residuals, and the cases the CPU and the GPU tests share, built with ease_ref's generator
and Gram restatement.  numpy rounds every elementwise product, sum and quotient on its own, as the contract asks."""
import functools

import numpy as np

import ease_ref as E

F = np.float32
TOL, CAP = 1e-4, 200


def _target(rho, den, l1, positive):
    """wn of one coordinate: fp32 scalars in, fp32 scalar out."""
    if positive:
        a = rho - l1
        return a / den if a > 0 and den > 0 else F(0.0)
    if rho > l1 and den > 0:
        return (rho - l1) / den
    if rho < -l1 and den > 0:
        return (rho + l1) / den
    return F(0.0)


def _start(G, j, w0):
    """(w, q) before the first sweep: zeros, or the warm start of the contract."""
    I = len(G)
    q = np.zeros(I, F)
    if w0 is None:
        return np.zeros(I, F), q
    w = np.array(w0, F)
    w[j] = F(0.0)
    for k in np.flatnonzero(w != 0):
        q = q + w[k] * G[k]
    return w, q


def solve_col(G, j, l1, l2, positive=True, w0=None, max_sweeps=CAP, tol=TOL):
    """The contract's loop, coordinate by coordinate.  Returns (w (I,) fp32, sweeps, steps, last fp32)."""
    assert G.dtype == F
    I = len(G)
    l1, l2, tol = F(l1), F(l2), F(tol)
    d = np.diag(G).copy()
    w, q = _start(G, j, w0)
    sweeps = steps = 0
    while True:
        maxd = F(0.0)
        for k in range(I):
            if k == j:
                continue
            t = d[k] * w[k]
            r = q[k] - t
            rho = G[j, k] - r
            den = d[k] + l2
            wn = _target(rho, den, l1, positive)
            delta = wn - w[k]
            if delta != 0:
                q = q + delta * G[k]
                w[k] = wn
                steps += 1
                if abs(delta) > maxd:
                    maxd = abs(delta)
        sweeps += 1
        if maxd <= tol or sweeps >= max_sweeps:
            return w, sweeps, steps, F(maxd)


def solve_col_screened(G, j, l1, l2, positive=True, w0=None, max_sweeps=CAP, tol=TOL, T=1024):
    """The same loop as the kernel runs it: the candidates of the block [k0, k0 + T) that lie behind the last update are evaluated
    side by side against the unchanged q, and the first one with delta != 0 is applied."""
    assert G.dtype == F
    I = len(G)
    l1, l2, tol = F(l1), F(l2), F(tol)
    d = np.diag(G).copy()
    den_all = d + l2
    gj = G[j]
    w, q = _start(G, j, w0)
    sweeps = steps = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while True:
            maxd = F(0.0)
            for k0 in range(0, I, T):
                k1 = min(I, k0 + T)
                lo = k0
                while lo < k1:
                    s = slice(lo, k1)
                    den = den_all[s]
                    rho = gj[s] - (q[s] - d[s] * w[s])
                    if positive:
                        a = rho - l1
                        wn = np.where((a > 0) & (den > 0), a / den, F(0.0))
                    else:
                        wn = np.where((rho > l1) & (den > 0), (rho - l1) / den,
                                      np.where((rho < -l1) & (den > 0), (rho + l1) / den, F(0.0)))
                    delta = (wn - w[s]).astype(F)
                    move = delta != 0
                    if lo <= j < k1:
                        move[j - lo] = False
                    hit = np.flatnonzero(move)
                    if len(hit) == 0:
                        break
                    k = lo + int(hit[0])
                    dk = delta[hit[0]]
                    q = q + dk * G[k]
                    w[k] = wn[hit[0]]
                    steps += 1
                    if abs(dk) > maxd:
                        maxd = abs(dk)
                    lo = k + 1
            sweeps += 1
            if maxd <= tol or sweeps >= max_sweeps:
                return w, sweeps, steps, F(maxd)


def solve(G, cols, l1, l2, positive=True, Wt0=None, max_sweeps=CAP, tol=TOL, T=1024, serial=False):
    """The listed columns: (W (len(cols), I) fp32 — row c is column cols[c] of the weights —, sweeps int32, steps int32, last fp32).
    ``Wt0``: the (I, I) rows a warm start reads."""
    fn = solve_col if serial else functools.partial(solve_col_screened, T=T)
    out = [fn(G, int(j), l1, l2, positive, None if Wt0 is None else Wt0[int(j)], max_sweeps, tol) for j in cols]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], F))


def kkt(G, j, w, l1, l2, positive=True):
    """The largest violation of column j's optimality conditions, in float64, relative to max G.  With g = (G + l2 1) w - G[j]:
    a coordinate with w[k] > 0 needs g[k] = -l1, one with w[k] < 0 needs g[k] = +l1, one at zero needs g[k] >= -l1 (and g[k] <= l1
    when signed).  Coordinate j is fixed at zero and has no condition."""
    G64, w64 = G.astype(np.float64), w.astype(np.float64)
    l1, l2 = float(F(l1)), float(F(l2))
    g = G64 @ w64 + l2 * w64 - G64[j]
    v = np.where(w64 > 0, np.abs(g + l1), np.where(w64 < 0, np.abs(g - l1), np.maximum(0.0, -l1 - g)))
    if not positive:
        v = np.where(w64 == 0, np.maximum(v, np.maximum(0.0, g - l1)), v)
    v[j] = 0.0
    return float(v.max() / np.abs(G64).max())


# name -> (ease_ref.case arguments, (l1, l2), listed columns, positive, cap)
_W_COLS = tuple(range(32)) + tuple(range(100, 2100, 125))
CASES = {
    "A": (E.CASES[0][:4] + (None, E.CASES[0][5]), (1.0, 5.0), tuple(range(96)), True, CAP),
    "B": (E.CASES[1][:4] + (None, E.CASES[1][5]), (2.0, 20.0), tuple(range(257)), True, CAP),
    "C": (E.CASES[2][:4] + (None, E.CASES[2][5]), (20.0, 50.0), tuple(range(0, 600, 6)), True, CAP),
    "S": ((400, 96, 12, 7, None, False), (5.0, 20.0), tuple(range(96)), False, 500),
    "W": ((3000, 2100, 60, 9, None, False), (20.0, 50.0), _W_COLS, True, CAP),
}
assert len(_W_COLS) == 48 and len(set(_W_COLS)) == 48


@functools.lru_cache(maxsize=None)
def gram(name):
    """(csr, I, G fp32) of a case; A, B and C are ease_ref's cases 0, 1 and 2 and share its cache."""
    args = CASES[name][0]
    for c, known in enumerate(E.CASES[:3]):
        if known[:4] == args[:4] and known[5] == args[5]:
            s = E.solved(c)
            return s["csr"], s["I"], s["G"]
    csr = E.case(*args)
    return csr, args[1], E.gram_ref(*csr, args[1])


@functools.lru_cache(maxsize=None)
def solved(name, max_sweeps=None, regs=None):
    """The screened restatement of a case's listed columns, computed once: dict(G, I, cols, l1, l2, positive, cap, W, sweeps, steps,
    last)."""
    _, (l1, l2), cols, positive, cap = CASES[name]
    if regs is not None:
        l1, l2 = regs
    cap = cap if max_sweeps is None else max_sweeps
    csr, I, G = gram(name)
    W, sweeps, steps, last = solve(G, cols, l1, l2, positive, max_sweeps=cap)
    return dict(csr=csr, G=G, I=I, cols=np.array(cols, np.int32), l1=l1, l2=l2, positive=positive, cap=cap, W=W, sweeps=sweeps,
                steps=steps, last=last)
