"""CPU tests of the diversified top-K: the three restatements of THE CONTRACT in tests/mmr_ref.py agree with each other and with brute
force; defects seeded into the reference are caught by the case sets of tests/test_gpu_mmr.py; the two entry points are declared,
exported, bound and built without contraction; their refusals, the binding's and the front end's come before the device; the two
beyond-accuracy metrics equal a float64 loop."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import mmr_ref as R


def _lib():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load_library()


def _same(x, y):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x[:3], y[:3]))


def _user(vec, score, pos, K, lam, normalize, kind="f32", n=None):
    return R.rerank_user(vec, score, pos, len(score) if n is None else n, K, lam, normalize, kind)[:2]


def _random_pool(N=24, D=8, n_items=40, seed=0):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n_items, D))
    vec = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    return vec, rng.uniform(size=N).astype(np.float32), rng.permutation(n_items)[:N].astype(np.int64)


def test_lam_one_returns_the_live_slots_in_relevance_order():
    vec, score, pos = _random_pool()
    score[[3, 7]] = score[5]                       # ties go to the lower slot
    score[11], pos[13] = np.nan, -1                # dead slots
    for normalize in (0, 1):
        slots, _ = _user(vec, score, pos, 24, 1.0, normalize)
        live = [j for j in range(24) if j not in (11, 13)]
        assert slots == sorted(live, key=lambda j: (-score[j], j))


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7])
def test_two_picks_equal_brute_force_over_all_pairs(lam):
    vec, score, pos = _random_pool(seed=1)
    slots, values = _user(vec, score, pos, 2, lam, 0, "f64")
    first = int(np.argmax(score))
    rows = vec[pos].astype(np.float64)
    lam64 = float(np.float32(lam))                 # the kernel is handed lambda in fp32
    value = lambda j: lam64 * float(score[j]) - (1 - lam64) * float(rows[j] @ rows[first])
    best = max((j for j in range(24) if j != first), key=lambda j: (value(j), -j))
    assert slots == [first, best]
    assert values[1] == pytest.approx(value(best), abs=1e-12)


def test_low_lambda_leaves_the_favoured_cluster_where_pure_relevance_does_not():
    """Two tight clusters, relevance favouring cluster 0: lam = 1 never leaves it; lam = 0.3 goes to the other cluster with its second
    pick.  (With the contract's m_j = MAXIMUM similarity every remaining item then has a near-duplicate in the list, so from the third
    pick on relevance decides again: greedy max-MMR switches clusters once per cluster, it does not alternate for ever.)  With four
    clusters the first four picks are one of each."""
    vec, score, pos, cluster = R.cluster_fixture(n_clusters=2, per_cluster=8)
    relevant, _ = _user(vec, score[0], pos[0], 6, 1.0, 1)
    diverse, _ = _user(vec, score[0], pos[0], 6, 0.3, 1)
    assert [int(cluster[s]) for s in relevant] == [0] * 6
    assert [int(cluster[s]) for s in diverse[:2]] == [0, 1] and diverse[0] == relevant[0]
    vec, score, pos, cluster = R.cluster_fixture()
    relevant, _ = _user(vec, score[0], pos[0], 8, 1.0, 1)
    diverse, _ = _user(vec, score[0], pos[0], 8, 0.3, 1)
    assert {int(cluster[s]) for s in relevant} == {0} and sorted(int(cluster[s]) for s in diverse[:4]) == [0, 1, 2, 3]
    ild = lambda slots: R.ild_ref(pos[:, slots], np.array([len(slots)]), vec)[0]
    assert ild(diverse) > ild(relevant) + 0.1


def test_minmax_of_a_flat_pool_is_zero_relevance():
    vec, score, pos = _random_pool(seed=2)
    score[:] = 0.75
    for kind in ("f32", "f64"):
        slots, values = _user(vec, score, pos, 5, 0.5, 1, kind)
        assert slots[0] == 0 and values[0] == 0.0                     # every rel is 0: the lowest slot, then pure diversity
        rows = vec[pos].astype(np.float64)
        assert slots[1] == int(np.argmin(rows @ rows[0]))
        assert values[1] == pytest.approx(-0.5 * float((rows @ rows[0]).min()), abs=1e-6)


def test_accumulate_is_the_sequential_loop_bit_for_bit():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((37, 100)).astype(np.float32)
    rows[5, 0] = -0.0
    for p in (0, 5, 36):
        assert np.array_equal(R.seq_dot_f32(rows, p).view(np.int32), R.seq_dot_loop(rows, p).view(np.int32))
    assert np.any(R.seq_dot_f32(rows, 0) != (rows.astype(np.float64) @ rows[0].astype(np.float64)).astype(np.float32))   # order matters


def test_exact_cases_do_not_depend_on_the_summation_order():
    """On the exact case set the fp32 emulator (sequential sums) and the order-free Gram loop give the same bits."""
    for case in R.exact_cases():
        a, c = R.rerank(case, "f32"), R.rerank(case, "exact")
        assert _same(a, c) and not a[3], case["name"]
    names = " ".join(c["name"] for c in R.exact_cases())
    for N, D in itertools.product(R.EXACT_N, R.EXACT_D):
        assert f"N{N}-D{D}-" in names
    for lam in R.EXACT_LAM:
        assert f"N256-D256-K128-lam{lam}-" in names and f"N256-D128-K128-lam{lam}-" in names
    assert "-B0-" in names and "-B1-" in names and "-B300-" in names and "nullcount" in names


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defect_is_caught_by_the_gpu_case_set(defect):
    """A reference with one defect seeded differs from the clean one on a case of the set tests/test_gpu_mmr.py holds the kernel to."""
    for cases, kind in ((R.exact_cases(), "exact"), (R.float_cases(), "f32")):
        for case in cases:
            if case["score"].shape[0] > 8:
                case = dict(case, score=case["score"][:8], pos=case["pos"][:8], count=None if case["count"] is None else case["count"][:8])
            if not _same(R.rerank(case, kind), R.rerank(case, kind, defect=defect)):
                return
    pytest.fail(f"no case notices the defect {defect!r}")


def test_sequential_fp32_stays_with_its_float64_twin_within_the_cap():
    """The kernel's own summation order, on the CPU: per twin case the users whose fp32 pick sequence leaves the float64 twin's do so
    at a near-tie (margin below TWIN_MARGIN), and they are at most TWIN_CAP of the users."""
    for i, case in enumerate(R.twin_cases()):
        slots = R.rerank(case, "f32")[0]
        left_out, wrong = R.twin_verdict(i, slots)
        print(f"{case['name']}: {len(left_out)} of {slots.shape[0]} users left out, {len(wrong)} beyond the margin")
        assert not wrong and len(left_out) <= R.TWIN_CAP * slots.shape[0], case["name"]


def test_entry_points_are_declared_exported_bound_and_built():
    from deeprecommendation_amd import native
    from deeprecommendation_amd.csrc import build
    hdr = open(os.path.join(ROOT, "include", "ncf_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+ncf_mmr_supported\s*\(", code) and re.search(r"\bint\s+ncf_mmr_rerank\s*\(", code)
    for line in ("acc = +0.0f;  for d = 0 .. D-1:  acc = acc + vec[pos_j, d] * vec[pos_p, d]",
                 "v_j = (lambda * rel_j) - ((1 - lambda) * m_j)",
                 "m_j starts at -inf, and after each pick  if sim > m_j: m_j = sim",
                 "slot j < n is LIVE iff 0 <= pos[j] < n_items and score[j] is finite",
                 "rel_j = (score_j - lo) / (hi - lo)"):
        assert line in hdr, line                                       # the contract is part of the ABI
    lib = _lib()
    for name, nargs in (("ncf_mmr_supported", 3), ("ncf_mmr_rerank", 17)):
        assert hasattr(lib, name) and len(native.SIGNATURES[name][1]) == nargs
    assert callable(native.mmr_rerank) and callable(native.mmr_supported)
    assert (native.MMR_MAX_N, native.MMR_MAX_D, native.MMR_MAX_K) == (R.MAX_N, R.MAX_D, R.MAX_K)
    assert "mmr.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["mmr.hip"]
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd import ranking_eval, recommend
    assert pkg.diversify_top_k is recommend.diversify_top_k and pkg.item_vectors is recommend.item_vectors
    assert pkg.intra_list_diversity is ranking_eval.intra_list_diversity and pkg.catalogue_coverage is ranking_eval.catalogue_coverage


def test_supported_over_the_edges_of_the_envelope():
    from deeprecommendation_amd import native
    _lib()
    yes = [(1, 4, 1), (256, 256, 128), (256, 4, 1), (128, 128, 128), (2, 60, 2), (200, 252, 128)]
    no = [(0, 4, 1), (257, 4, 1), (1, 0, 1), (1, 3, 1), (8, 6, 1), (8, 260, 1), (8, 257, 1), (8, 8, 0), (8, 8, 9), (256, 8, 129), (-1, 8, 1),
          (8, -4, 1), (8, 8, -1), (1, 4, 2)]
    for N, D, K in yes:
        assert native.mmr_supported(N, D, K), (N, D, K)
    for N, D, K in no:
        assert not native.mmr_supported(N, D, K), (N, D, K)


def test_rerank_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()
    a = 16                                       # a non-null, 16-byte aligned stand-in: every refusal comes before any launch

    def call(vec=a, n_items=10, D=8, ldv=8, score=a, pos=a, count=a, B=3, N=16, K=4, lam=0.5, normalize=1, slot=a, value=a, out_count=a,
             oob=a):
        return lib.ncf_mmr_rerank(vec, n_items, D, ldv, score, pos, count, B, N, K, lam, normalize, slot, value, out_count, oob, None)

    assert call(B=0) == native.NCF_OK
    assert call(B=0, vec=None, score=None, pos=None, count=None, slot=None, value=None, out_count=None, oob=None) == native.NCF_OK
    for bad in (dict(B=-1), dict(n_items=-1), dict(N=-1), dict(D=-4), dict(K=-1), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")),
                dict(lam=float("inf")), dict(normalize=2), dict(normalize=-1), dict(ldv=7), dict(score=None), dict(pos=None), dict(slot=None),
                dict(value=None), dict(out_count=None), dict(vec=None), dict(B=0, lam=2.0), dict(B=0, ldv=4), dict(B=0, normalize=3)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_mmr_rerank" in lib.ncf_last_error(), bad
    assert b"lambda" in (call(lam=1.5), lib.ncf_last_error())[1] and b"normalize" in (call(normalize=5), lib.ncf_last_error())[1]
    for bad in (dict(N=0, K=0), dict(N=257), dict(D=0, ldv=0), dict(D=6), dict(D=260, ldv=260), dict(K=0), dict(K=17), dict(N=256, K=129)):
        assert call(**bad) == native.NCF_EUNSUPPORTED and b"ncf_mmr_rerank" in lib.ncf_last_error() and b"256" in lib.ncf_last_error(), bad


def test_binding_and_front_end_refuse_before_the_device():
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd import native
    _lib()
    good = dict(scores=torch.zeros(3, 16), positions=torch.zeros(3, 16, dtype=torch.int64), counts=torch.full((3,), 16, dtype=torch.int32),
                item_vectors=torch.zeros(10, 8), k=4, lam=0.5, normalize="minmax")
    for key, bad, limit in (("scores", torch.zeros(3, 16, dtype=torch.float64), None), ("scores", torch.zeros(48), None),
                            ("scores", torch.zeros(3, 15), None), ("positions", torch.zeros(3, 16, dtype=torch.int32), None),
                            ("positions", torch.zeros(2, 16, dtype=torch.int64), None), ("counts", torch.zeros(3, dtype=torch.int64), None),
                            ("counts", torch.zeros(4, dtype=torch.int32), None), ("item_vectors", torch.zeros(10, 8, dtype=torch.float16), None),
                            ("item_vectors", torch.zeros(80), None), ("item_vectors", torch.zeros(10, 6), "multiple of 4"),
                            ("item_vectors", torch.zeros(10, 260), "256"), ("k", 0, "1 .."), ("k", 17, "min(N = 16"), ("k", 2.0, None),
                            ("lam", -0.1, "[0, 1]"), ("lam", 1.5, "[0, 1]"), ("lam", float("nan"), "[0, 1]"), ("lam", "0.5", None),
                            ("normalize", "zscore", "minmax"), ("normalize", True, "minmax")):
        with pytest.raises(ValueError, match=None if limit is None else re.escape(limit)):
            pkg.diversify_top_k(**dict(good, **{key: bad}))
    wide = dict(good, scores=torch.zeros(1, 257), positions=torch.zeros(1, 257, dtype=torch.int64), counts=None)
    with pytest.raises(ValueError, match="1 .. 256"):
        pkg.diversify_top_k(**wide)
    with pytest.raises(ValueError, match="128"):
        pkg.diversify_top_k(**dict(good, scores=torch.zeros(1, 200), positions=torch.zeros(1, 200, dtype=torch.int64), counts=None, k=129))
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # well-formed host tensors: only now the device is asked for
        pkg.diversify_top_k(**good)
    args = dict(vectors=good["item_vectors"], scores=good["scores"], positions=good["positions"], counts=good["counts"], k=4, lam=0.5)
    for key, bad in (("vectors", torch.zeros(10, 16)[:, ::2]), ("vectors", torch.zeros(10, 6)), ("scores", torch.zeros(3, 32)[:, ::2]),
                     ("positions", torch.zeros(3, 16, dtype=torch.int32)), ("counts", torch.zeros(3, dtype=torch.int64)), ("k", 17), ("k", 0),
                     ("k", True), ("lam", 1.5), ("lam", float("nan"))):
        with pytest.raises(ValueError, match="mmr_rerank"):
            native.mmr_rerank(**dict(args, **{key: bad}))
    with pytest.raises(RuntimeError, match="GPU"):
        native.mmr_rerank(**args)


def test_item_vectors_refuses_before_the_device():
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    m = BasicNCF(item_dim=10, user_dim=12, item_emb=8, user_emb=8, mlp_dense_layers=[16])
    with pytest.raises(RuntimeError, match="eval"):
        pkg.item_vectors(m)
    m.eval()
    with pytest.raises(ValueError, match="AttentionNCF"):
        pkg.item_vectors(m, item_features=torch.zeros(10, 4))
    with pytest.raises(ValueError, match="GraphNCF"):
        pkg.item_vectors(m, graph=object())
    a = AttentionNCF(item_dim=6, item_emb=512, user_emb=32, att_dense=8, mlp_dense_layers=[16]).eval()
    with pytest.raises(ValueError, match="item_features"):
        pkg.item_vectors(a)
    with pytest.raises(ValueError, match="wider than the 256"):
        pkg.item_vectors(a, item_features=torch.zeros(5, 6))


def test_diversity_and_coverage_equal_a_float64_loop():
    import deeprecommendation_amd as pkg
    vec, _, _, _ = R.cluster_fixture()
    rng = np.random.default_rng(11)
    pos = rng.integers(0, vec.shape[0], size=(9, 7)).astype(np.int64)
    pos[2, 3] = -1                                                   # a padded slot inside the count
    pos[4] = pos[4, 0]                                               # one item seven times: diversity 0 up to rounding
    counts = np.array([7, 2, 7, 1, 7, 0, 5, 3, 7], dtype=np.int32)
    got = pkg.intra_list_diversity(torch.from_numpy(pos), torch.from_numpy(counts), torch.from_numpy(vec)).numpy()
    want = R.ild_ref(pos, counts, vec)
    assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[[3, 5]]).all()
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= 1e-5 * np.abs(want[ok]) + 1e-6).all()
    cov = pkg.catalogue_coverage(torch.from_numpy(pos), torch.from_numpy(counts), vec.shape[0])
    want_cov = R.coverage_ref(pos, counts, vec.shape[0])
    assert cov.dim() == 0 and 0 < want_cov < 1 and abs(float(cov) - want_cov) <= 1e-5 * want_cov + 1e-6
    assert float(pkg.catalogue_coverage(torch.from_numpy(pos), None, 10 ** 6)) == pytest.approx(len(set(pos[pos >= 0].tolist())) / 10 ** 6)
    for bad in (dict(positions=torch.zeros(3, 2)), dict(counts=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            pkg.catalogue_coverage(**dict(dict(positions=torch.zeros(3, 2, dtype=torch.int64), counts=None, n_items=5), **bad))
    with pytest.raises(ValueError):
        pkg.catalogue_coverage(torch.zeros(3, 2, dtype=torch.int64), None, 0)
