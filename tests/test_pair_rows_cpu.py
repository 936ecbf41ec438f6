"""CPU tests of the per-pair CSR entry points (csrc/pair_rows.hip): the symbols are declared, exported and bound; the refusals come
before any launch (the library loads and refuses without a GPU); the numpy restatement the GPU tests compare with
(tests/pair_rows_ref.py) equals the torch code it replaces — SparseRatings.expanded() and the target mask of _forward_train_hip —
and torch.isclose itself on boundary-dense data and on specials."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from pair_rows_ref import (F32, N_ITEMS, check_plan, isclose_f32, mask_tables, pair_rows_count_ref, pair_rows_ref, pairs, shared_csr)


def _lib():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load_library()


def test_pair_rows_entry_points_are_declared_exported_and_bound():
    from deeprecommendation_amd import native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ncf_abi.h")).read(), flags=re.S)
    lib = _lib()
    for name, nargs in (("ncf_pair_rows_count", 7), ("ncf_pair_rows_fill", 20)):
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert hasattr(lib, name) and name in native.SIGNATURES, name
        assert len(native.SIGNATURES[name][1]) == nargs
    assert callable(native.pair_rows) and callable(native.check_pair_rows)
    from deeprecommendation_amd.csrc import build
    assert "pair_rows.hip" in build.SOURCES
    # the formula is part of the ABI
    hdr = open(os.path.join(ROOT, "include", "ncf_abi.h")).read()
    assert "a == b || (isfinite(a) && isfinite(b) && fabsf(a - b) <= atol + fabsf(rtol * b))" in hdr


def test_pair_rows_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()
    a = 16                                       # a non-null, 16-byte aligned stand-in: every refusal comes before any launch

    def count(rowptr=a, R=8, pair_row=a, B=4, out=a):
        return lib.ncf_pair_rows_count(rowptr, R, pair_row, B, out, None, None)

    def fill(rowptr=a, col=a, val=a, R=8, pair_row=a, B=4, out_rowptr=a, out_col=a, out_val=a, capacity=100, cand=a, ldcand=32, rated=a,
             ldrated=32, I=10, E=32, atol=1e-5, rtol=1e-5, flag=a):
        return lib.ncf_pair_rows_fill(rowptr, col, val, R, pair_row, B, out_rowptr, out_col, out_val, capacity, cand, ldcand, rated, ldrated,
                                      I, E, atol, rtol, flag, None)

    assert count(B=0) == native.NCF_OK and count(B=0, rowptr=None, pair_row=None) == native.NCF_OK      # an empty batch launches nothing
    for bad in (dict(R=-1), dict(B=-1), dict(rowptr=None), dict(pair_row=None), dict(out=None), dict(B=0, out=None)):
        assert count(**bad) == native.NCF_EINVAL and b"ncf_pair_rows_count" in lib.ncf_last_error(), bad
    assert count(B=1 << 31) == native.NCF_EUNSUPPORTED
    assert fill(B=0) == native.NCF_OK and fill(B=0, out_col=None, out_val=None, col=None) == native.NCF_OK
    for bad in (dict(R=-1), dict(B=-1), dict(capacity=-1), dict(rowptr=None), dict(col=None), dict(val=None), dict(pair_row=None),
                dict(out_rowptr=None), dict(out_col=None), dict(out_val=None), dict(flag=None), dict(rated=None), dict(I=-1), dict(E=0),
                dict(ldcand=31), dict(ldrated=31), dict(atol=-1.0), dict(rtol=float("nan")), dict(B=0, E=0)):
        assert fill(**bad) == native.NCF_EINVAL and b"ncf_pair_rows_fill" in lib.ncf_last_error(), bad
    assert fill(B=1 << 31) == native.NCF_EUNSUPPORTED


def _torch_expand_and_mask(rowptr, col, val, pair_row, mask):
    """What _forward_train_hip does with torch ops: SparseRatings.expanded(), then the isclose mask per entry."""
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import SparseRatings
    ex = SparseRatings(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), N_ITEMS,
                       pair_row=torch.from_numpy(pair_row)).expanded()
    r, c, v = ex.rowptr, ex.col, ex.val
    if mask is not None and c.numel():
        cand_emb, rated_emb = torch.from_numpy(mask[0]), torch.from_numpy(mask[1])
        b_of = torch.repeat_interleave(torch.arange(r.numel() - 1), r[1:] - r[:-1])
        same = torch.isclose(cand_emb[b_of], rated_emb[c.long()], atol=1e-5).all(dim=1)
        c = torch.where(same, torch.full_like(c, -1), c)
    return r.numpy(), c.numpy(), v.numpy()


@pytest.mark.parametrize("E", [None, 1, 4, 50, 64])
def test_reference_equals_expanded_plus_the_torch_mask(E):
    rowptr, col, val = shared_csr()
    col = np.where((col < 0) | (col >= N_ITEMS), 5, col).astype(np.int32)      # the torch code indexes with every column: keep them inside
    pr = pairs(37)
    mask = None
    if E is not None:
        cand, rated, plan, twins = mask_tables(rowptr, col, pr, E)
        mask = (cand, rated)
    total = int(pair_rows_count_ref(rowptr, pr)[0].sum())
    out_rowptr, out_col, out_val, flag, oob = pair_rows_ref(rowptr, col, val, pr, total, mask)
    r, c, v = _torch_expand_and_mask(rowptr, col, val, pr, mask)
    assert flag == 0 and oob == 0
    assert np.array_equal(out_rowptr, r) and np.array_equal(out_col, c) and np.array_equal(out_val, v)
    if E is not None:
        assert (out_col == -1).sum() > 0


@pytest.mark.parametrize("E", [1, 4, 32, 50, 64, 128, 256])
def test_mask_data_reaches_every_case(E):
    """The shared GPU-test data: on the reference's output every planned case holds (self, twins with both masked, 0.5x / 1.5x the
    allowed error, NaN, +inf / -inf), and columns outside the catalogue pass through."""
    rowptr, col, val = shared_csr()
    pr = pairs(37)
    cand, rated, plan, twins = mask_tables(rowptr, col, pr, E)
    total = int(pair_rows_count_ref(rowptr, pr)[0].sum())
    out_rowptr, out_col, out_val, flag, oob = pair_rows_ref(rowptr, col, val, pr, total, (cand, rated))
    seen = check_plan(plan, twins, rowptr, col, pr, out_rowptr, out_col)
    assert seen == {"self", "twins", "twins-both", "half", "over", "nan", "inf"}
    b = 0                                         # pair 0 uses row 7: entries at col = -1 and col = N_ITEMS, unchanged
    got = out_col[out_rowptr[b]:out_rowptr[b + 1]]
    assert got[0] == -1 and got[256] == N_ITEMS


def test_reference_capacity_and_out_of_range_rows():
    rowptr, col, val = shared_csr()
    pr = pairs(37)
    total = int(pair_rows_count_ref(rowptr, pr)[0].sum())
    full = pair_rows_ref(rowptr, col, val, pr, total)
    short = pair_rows_ref(rowptr, col, val, pr, total - 1)
    assert full[3] == 0 and short[3] == 1
    assert np.array_equal(short[1], full[1][:-1]) and np.array_equal(short[2], full[2][:-1])
    bad = pr.copy()
    bad[2], bad[5] = -1, 8
    r, c, v, flag, oob = pair_rows_ref(rowptr, col, val, bad, total)
    assert oob == 1 and r[3] == r[2] and r[6] == r[5]


def test_isclose_restatement_equals_torch_isclose():
    """Boundary-dense: |a - b| spread over 0 .. 1.2x of atol + rtol * |b| across magnitudes, plus +-inf, NaN and +-0."""
    rng = np.random.default_rng(3)
    n = 1 << 20
    b = (rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-6, 4, n)).astype(F32)
    allowed = F32(1e-5) + np.abs(F32(1e-5) * b)
    a = (b + rng.choice([-1.0, 1.0], n).astype(F32) * rng.uniform(0, 1.2, n).astype(F32) * allowed).astype(F32)
    # right at the bound: the neighbouring floats of b +- allowed
    edge = (b[:4096] + allowed[:4096]).astype(F32)
    a = np.concatenate([a, edge, np.nextafter(edge, F32(np.inf)), np.nextafter(edge, F32(-np.inf))])
    b = np.concatenate([b, b[:4096], b[:4096], b[:4096]])
    sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, 1e-5, -1e-5, 3.4e38, -3.4e38, 1e-45], dtype=F32)
    a = np.concatenate([a, np.repeat(sp, len(sp))])
    b = np.concatenate([b, np.tile(sp, len(sp))])
    want = torch.isclose(torch.from_numpy(a), torch.from_numpy(b), atol=1e-5).numpy()
    got = isclose_f32(a, b)
    assert int((got != want).sum()) == 0
    assert 0.1 < got[:n].mean() < 0.95            # both sides of the bound are populated


def test_dynamic_ranking_resident_pairs_is_none_on_cpu_and_opt_in():
    import pandas as pd
    from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset, DynamicRankingDataset
    prov = SparseDynamicProvider(np.arange(1, 6), np.eye(5, 4, dtype=np.float32), [1, 2], [np.array([1, 2]), np.array([3])],
                                 [np.array([4.0, 2.0]), np.array([5.0])], [3.0, 4.0])
    frame = pd.DataFrame({"userId": [1, 2], "positive_movieId": [1, 3], "negative_movieIds": [[2], [1]], "negative_ratings": [[2.0], [1.0]]})
    ds = DynamicRankingDataset(frame, prov)
    assert ds.resident_pairs(torch.device("cpu")) is None and ds.resident_pairs(None) is None
    assert DynamicRankingDataset.resident_opt_in and DynamicPointwiseDataset.resident_opt_in
