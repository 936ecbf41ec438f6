"""The contract of ncf_adam_rows / optim.RowSparseAdam restated in numpy float64 — the oracle of the row-sparse Adam tests.

Rows are grouped by id, each group's gradient rows are summed in float64, and every touched row takes ONE Adam update

    g += wd * p;  m += (1 - b1) * (g - m);  v = b2 * v + (1 - b2) * g * g;
    p -= (lr / (1 - b1^step)) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)

with the bias corrections of the tensor-wide ``step``.  Untouched rows, and ids outside ``[0, rows)``, change nothing.

The kernel's ABI takes its hyper-parameters as C floats, so the tests hand BOTH sides float32-representable values (``f32``
below): with b2 = 0.999 as a double here and as a float there, ``1 - b2`` alone would differ by 1.3e-5 relative, which is a
property of the argument type and not of the arithmetic under test."""
import numpy as np


def f32(x) -> float:
    """The float32 value nearest to x, as a Python float."""
    return float(np.float32(x))


def row_adam_ref(p, m, v, ids, g, lr, b1, b2, eps, wd, step):
    """(p, m, v) after one row-sparse Adam step, as new float64 arrays.  p, m, v: [rows, E]; ids: [n]; g: [n, E]."""
    p, m, v = (np.array(x, dtype=np.float64) for x in (p, m, v))
    ids = np.asarray(ids, dtype=np.int64)
    g = np.asarray(g, dtype=np.float64).reshape(len(ids), p.shape[1])
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    for r in np.unique(ids):
        if r < 0 or r >= p.shape[0]:
            continue
        gg = g[ids == r].sum(axis=0) + wd * p[r]
        m[r] += (1.0 - b1) * (gg - m[r])
        v[r] = b2 * v[r] + (1.0 - b2) * gg * gg
        p[r] -= (lr / bc1) * m[r] / (np.sqrt(v[r]) / np.sqrt(bc2) + eps)
    return p, m, v
