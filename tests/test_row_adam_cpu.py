"""CPU: the row-sparse Adam oracle (row_adam_ref) against torch.optim.Adam in float64; the ncf_adam_rows entry point is declared,
exported and bound; RowSparseAdam refuses what it cannot run."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from row_adam_ref import row_adam_ref

HYPER = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8)


def _torch_adam(p0, wd):
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    return p, torch.optim.Adam([p], lr=HYPER["lr"], betas=(HYPER["b1"], HYPER["b2"]), eps=HYPER["eps"], weight_decay=wd)


def _close(a, b):
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_every_row_touched_once_is_torch_adam(wd):
    rng = np.random.default_rng(0)
    rows, E = 37, 5
    p0 = rng.standard_normal((rows, E))
    p, opt = _torch_adam(p0, wd)
    rp, rm, rv = p0, np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 5):
        ids = rng.permutation(rows)
        g = rng.standard_normal((rows, E))
        dense = np.zeros_like(p0)
        dense[ids] = g
        p.grad = torch.tensor(dense)
        opt.step()
        rp, rm, rv = row_adam_ref(rp, rm, rv, ids, g, wd=wd, step=step, **HYPER)
        st = opt.state[p]
        _close(rp, p.detach().numpy())
        _close(rm, st["exp_avg"].numpy())
        _close(rv, st["exp_avg_sq"].numpy())


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_duplicates_are_summed_and_untouched_rows_stay(wd):
    rng = np.random.default_rng(1)
    rows, E, n = 41, 6, 90
    p0 = rng.standard_normal((rows, E))
    m0, v0 = rng.standard_normal((rows, E)) * 0.1, rng.random((rows, E)) * 0.01
    ids = rng.choice(np.arange(0, rows, 3), n)                       # a third of the rows at most, with duplicates
    ids[:20] = ids[0]                                                # and one id many times
    g = rng.standard_normal((n, E))
    rp, rm, rv = row_adam_ref(p0, m0, v0, ids, g, wd=wd, step=3, **HYPER)
    touched = np.zeros(rows, dtype=bool)
    touched[ids] = True
    assert 1 < touched.sum() < rows and len(np.unique(ids)) < n
    for got, before in ((rp, p0), (rm, m0), (rv, v0)):
        assert np.array_equal(got[~touched], before[~touched])
    # dense Adam at step 3 from the same state, fed the summed gradient: its touched rows
    p, opt = _torch_adam(p0, wd)
    opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": torch.tensor(m0), "exp_avg_sq": torch.tensor(v0)}
    dense = np.zeros_like(p0)
    np.add.at(dense, ids, g)
    p.grad = torch.tensor(dense)
    opt.step()
    _close(rp[touched], p.detach().numpy()[touched])
    _close(rm[touched], opt.state[p]["exp_avg"].numpy()[touched])
    _close(rv[touched], opt.state[p]["exp_avg_sq"].numpy()[touched])
    assert not np.array_equal(rp[touched], p0[touched])
    # ids outside the table change nothing
    op, om, ov = row_adam_ref(p0, m0, v0, np.array([-1, rows, rows + 5]), rng.standard_normal((3, E)), wd=wd, step=1, **HYPER)
    assert np.array_equal(op, p0) and np.array_equal(om, m0) and np.array_equal(ov, v0)


def _lib():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load_library()


def test_adam_rows_entry_point_is_declared_bound_and_refuses_bad_arguments():
    from deeprecommendation_amd import native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ncf_abi.h")).read(), flags=re.S)
    lib = _lib()
    assert re.search(r"\bncf_adam_rows\s*\(", txt)
    assert hasattr(lib, "ncf_adam_rows") and "ncf_adam_rows" in native.SIGNATURES
    assert len(native.SIGNATURES["ncf_adam_rows"][1]) == 19 and callable(native.adam_rows_)
    a = 16                                       # a non-null, 16-byte aligned stand-in: every refusal comes before any launch

    def call(p=a, ld=8, E=8, ids=a, n=4, g=a, ld_g=8, step=1):
        return lib.ncf_adam_rows(p, a, a, ld, 10, E, ids, None, n, g, ld_g, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, None, None)

    assert call(n=0) == native.NCF_OK and call(n=0, step=0, p=None) == native.NCF_OK          # an empty batch launches nothing
    for bad in (dict(step=0), dict(E=0), dict(ld=7), dict(ld_g=7), dict(p=None), dict(ids=None), dict(g=None), dict(n=-1)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_adam_rows" in lib.ncf_last_error(), bad


def test_row_sparse_adam_refuses_cpu_parameters_and_plain_weights():
    from deeprecommendation_amd.neural_collaborative_filtering.util import is_row_major_embedding, row_major_embedding_
    from deeprecommendation_amd.optim import FusedAdam, RowSparseAdam
    assert issubclass(RowSparseAdam, FusedAdam)
    emb = row_major_embedding_(torch.nn.Linear(12, 4))
    plain = torch.nn.Linear(12, 4)
    assert is_row_major_embedding(emb.weight) and not is_row_major_embedding(plain.weight)
    with pytest.raises(RuntimeError, match="GPU"):
        RowSparseAdam(emb.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="id-major"):
        RowSparseAdam(list(emb.parameters()) + list(plain.parameters()), lr=1e-3, row_sparse=[plain.weight])
    assert not hasattr(emb.weight, "_ncf_row_grads") and not hasattr(plain.weight, "_ncf_row_grads")    # a refusal leaves no mark
