"""CPU tests of the content form of BasicNCF: the contract of ncf_user_profiles as a float64 loop equals numpy's mean expression bit
for bit (tests/user_profiles_ref.py); the entry point is declared, exported, bound and built; its refusals, the binding's and
BasicNCF.set_content's come before the device; ContentIndexProvider hands out IndexProvider's positions and so gives the fixed
datasets their resident form."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from user_profiles_ref import F_LIST, cases, make_case, profiles_loop, profiles_numpy


def _lib():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load_library()


@pytest.mark.parametrize("F", F_LIST)
def test_loop_equals_the_numpy_mean_expression_bit_for_bit(F):
    for name, c in cases(F):
        a, b = profiles_loop(**c), profiles_numpy(**c)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), name
        empty = np.nonzero(np.diff(c["rowptr"]) == 0)[0]
        assert not a[empty].any(), name


def test_loop_skips_a_column_out_of_range_and_still_divides_by_the_row_length():
    c = make_case(5, [4, 3], seed=3)
    want = profiles_loop(**c)
    c["col"][1] = c["features"].shape[0]
    got = profiles_loop(**c)
    assert np.array_equal(got[1], want[1]) and not np.array_equal(got[0], want[0])
    d = c["rating"][:4].astype(np.float64) - c["avg"][0]
    rows = c["features"][c["col"][[0, 2, 3]]].astype(np.float64)
    acc = (0.0 + d[0] * rows[0]) + d[2] * rows[1]
    acc = acc + d[3] * rows[2]
    assert np.array_equal(got[0], (acc / 4.0).astype(np.float32))


def test_entry_point_is_declared_exported_bound_and_built():
    from deeprecommendation_amd import native
    from deeprecommendation_amd.csrc import build
    hdr = open(os.path.join(ROOT, "include", "ncf_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+ncf_user_profiles\s*\(", code)
    assert "product rounded, THEN sum rounded" in hdr                  # the contract is part of the ABI
    lib = _lib()
    assert hasattr(lib, "ncf_user_profiles") and "ncf_user_profiles" in native.SIGNATURES
    assert len(native.SIGNATURES["ncf_user_profiles"][1]) == 14
    assert callable(native.user_profiles)
    assert "user_profiles.hip" in build.SOURCES
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["user_profiles.hip"]
    import deeprecommendation_amd as pkg
    assert "content_cosine_top_k" in pkg._RECOMMEND and callable(pkg.content_cosine_top_k)


def test_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()
    a = 16                                       # a non-null, 16-byte aligned stand-in: every refusal comes before any launch

    def call(rowptr=a, col=a, rating=a, nnz=10, avg=a, U=3, feat=a, I=20, ldf=8, F=8, out=a, ldout=8, flag=a):
        return lib.ncf_user_profiles(rowptr, col, rating, nnz, avg, U, feat, I, ldf, F, out, ldout, flag, None)

    assert call(U=0) == native.NCF_OK and call(U=0, rowptr=None, avg=None, out=None, col=None, rating=None, feat=None) == native.NCF_OK
    for bad in (dict(U=-1), dict(I=-1), dict(nnz=-1), dict(F=0), dict(F=-3), dict(ldf=7), dict(ldout=7), dict(rowptr=None), dict(avg=None),
                dict(out=None), dict(col=None), dict(rating=None), dict(feat=None), dict(U=0, F=0)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_user_profiles" in lib.ncf_last_error(), bad


def test_binding_refuses_mistyped_and_strided_tensors_before_the_device():
    from deeprecommendation_amd import native
    _lib()
    good = dict(rowptr=torch.tensor([0, 2, 3]), col=torch.tensor([0, 1, 1], dtype=torch.int32), rating=torch.ones(3),
                avg=torch.zeros(2, dtype=torch.float64), features=torch.ones(4, 6))
    for key, bad in (("rowptr", good["rowptr"].to(torch.int32)), ("col", good["col"].to(torch.int64)), ("rating", good["rating"].double()),
                     ("avg", good["avg"].float()), ("features", good["features"].double()), ("features", torch.ones(6, 4).t()),
                     ("features", torch.ones(4)), ("col", torch.zeros(6, dtype=torch.int32)[::2]), ("rowptr", torch.tensor([0, 2])),
                     ("rating", torch.ones(4))):
        with pytest.raises(ValueError):
            native.user_profiles(**dict(good, **{key: bad}))
    with pytest.raises(ValueError):
        native.user_profiles(**good, out=torch.zeros(2, 6, dtype=torch.float64))
    with pytest.raises(ValueError):
        native.user_profiles(**good, out=torch.zeros(3, 6))
    with pytest.raises(RuntimeError, match="GPU"):        # well-formed host tensors: only now the device is asked for
        native.user_profiles(**good)


def test_set_content_refuses_before_the_device():
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    m = BasicNCF(item_dim=6, user_dim=6, item_emb=8, user_emb=8, mlp_dense_layers=[16]).eval()
    assert m.num_users == 6 and m.num_items == 6
    up, it = torch.zeros(5, 6), torch.zeros(9, 6)
    for bad_u, bad_i in ((up.double(), it), (up, it.to(torch.int64)), (up[0], it), (up, it[None]), (torch.zeros(5, 7), it), (up, torch.zeros(9, 5)),
                         (torch.zeros(6, 5).t(), it), (up, torch.zeros(9, 12)[:, ::2]), (None, it), (up, None), (up.numpy(), it),
                         (up, it)):                      # the last pair is well formed and on the host: refused for its device
        with pytest.raises(ValueError):
            m.set_content(bad_u, bad_i)
        assert m._content is None
    assert m.set_content(None, None) is m and m.num_items == 6


def test_cosine_case_leaves_out_at_most_five_percent_for_near_ties():
    """The data of the GPU test of the cosine baseline: what its seed leaves undecided (float64 neighbours within twice the tolerance),
    from the float64 scores alone; the zero profile scores 0 everywhere."""
    from content_cosine_ref import K, TOL, ZERO_USER, cosine_case, decided, undecided_share
    prof, feat, cos, order = cosine_case()
    assert undecided_share(cos, order) <= 0.05
    assert not cos[ZERO_USER].any() and not decided(cos, order)[ZERO_USER].any()
    assert decided(cos, order).shape == (len(prof), K) and TOL == 75 * 2.0 ** -24


def _toy_provider():
    from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider
    rng = np.random.default_rng(5)
    item_ids = np.arange(1, 30) * 7
    user_ids = (np.arange(10, 60) * 3)[rng.permutation(50)]          # the provider's user order is not the sorted order
    rated = [np.sort(rng.choice(item_ids, int(rng.integers(0, 9)), replace=False)) for _ in user_ids]
    ratings = [rng.integers(1, 11, len(r)) * 0.5 for r in rated]
    means = [float(r.mean()) if len(r) else 0.0 for r in ratings]
    feats = rng.standard_normal((len(item_ids), 6)).astype(np.float32)
    return SparseDynamicProvider(item_ids[::-1], feats[::-1], user_ids, rated, ratings, means), item_ids, user_ids, feats


def test_profile_csr_keeps_every_rating_in_order():
    prov, item_ids, user_ids, feats = _toy_provider()
    rowptr, col, rating, avg = prov.profile_csr()
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and rating.dtype == np.float32 and avg.dtype == np.float64
    assert np.array_equal(np.diff(rowptr), [len(r) for r in prov.user_rated_items])
    assert np.array_equal(item_ids[col], np.concatenate(prov.user_rated_items))
    assert np.array_equal(avg, (prov.user_mean + 2.5) / 2)
    assert all((np.diff(col[rowptr[u]:rowptr[u + 1]]) > 0).all() for u in range(len(user_ids)))
    assert np.array_equal(prov.features.numpy(), feats)            # the provider sorts its items by id


def test_content_index_provider_hands_out_index_provider_positions():
    from deeprecommendation_amd.content_providers.index_providers import ContentIndexProvider, IndexProvider
    rng = np.random.default_rng(1)
    users, items = np.arange(10, 60) * 3, np.arange(1, 30) * 7
    prof, feats = rng.standard_normal((50, 6)).astype(np.float32), rng.standard_normal((29, 6)).astype(np.float32)
    cp, ip = ContentIndexProvider(users[::-1], items, prof, feats), IndexProvider(users, items)
    q_u, q_i = rng.choice(users, 5000), rng.choice(items, 5000)
    assert np.array_equal(cp.get_user_profile(q_u), ip.get_user_profile(q_u)) and np.array_equal(cp.get_item_profile(q_i), ip.get_item_profile(q_i))
    assert np.array_equal(cp.get_user_profile(q_u[:7]), ip.get_user_profile(q_u[:7]))
    assert cp.get_num_users() == 50 and cp.get_num_items() == 29 and cp.get_item_feature_dim() == 6
    u, i = cp.content(torch.device("cpu"))
    assert u.dtype == i.dtype == torch.float32 and torch.equal(u, torch.from_numpy(prof)) and torch.equal(i, torch.from_numpy(feats))
    assert cp.content(torch.device("cpu"))[0] is u
    f, g = cp.device_lookup(torch.device("cpu")), ip.device_lookup(torch.device("cpu"))
    raw = torch.from_numpy(q_u), torch.from_numpy(q_i)
    assert all(torch.equal(a, b) for a, b in zip(f(*raw), g(*raw)))
    with pytest.raises(KeyError):
        cp.get_user_profile([31])
    for bad in ((prof[:49], feats), (prof, feats[:28]), (prof[:, :5], feats)):
        with pytest.raises(ValueError):
            ContentIndexProvider(users, items, *bad)


def test_resident_inputs_over_content_index_provider_match_the_dataloader_batches():
    import pandas as pd
    from torch.utils.data import DataLoader
    from deeprecommendation_amd.content_providers.index_providers import ContentIndexProvider, OneHotProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset
    rng = np.random.default_rng(0)
    n = 257
    frame = pd.DataFrame({"userId": rng.integers(10, 60, n) * 3, "movieId": rng.integers(1, 30, n) * 7, "rating": rng.integers(1, 11, n) * 0.5})
    users, items = np.arange(10, 60) * 3, np.arange(1, 30) * 7
    cp = ContentIndexProvider(users, items, np.zeros((50, 4), np.float32), np.zeros((29, 4), np.float32))
    ds = FixedPointwiseDataset(frame, cp)
    res = ds.resident_inputs()
    assert res is not None and res.on_chunk is None
    (u, i), y = res.tensors, res.targets
    batches = list(DataLoader(ds, batch_size=50, collate_fn=ds.use_collate()))
    assert torch.equal(u, torch.cat([b[0] for b in batches])) and torch.equal(i, torch.cat([b[1] for b in batches]))
    assert torch.equal(y, torch.cat([b[2] for b in batches])) and u.dtype == torch.int64
    raw = ds.resident_inputs(torch.device("cpu"))
    assert raw.on_chunk is not None
    up, ip = raw.on_chunk(*raw.tensors)
    assert torch.equal(up, u) and torch.equal(ip, i)
    assert FixedPointwiseDataset(frame, OneHotProvider(users, items)).resident_inputs() is None
