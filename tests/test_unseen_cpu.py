"""CPU tests of the implicit-feedback protocol: the numpy contract of ncf_sample_unseen (tests/unseen_ref.py) against itself — unrank
against the explicit complement, the properties of a draw, a split call — and its uniformity figures; leave_one_out on a hand-written
frame; and the refusals of ImplicitFeedback, fit_implicit and eval_sampled, none of which touches a device."""
import numpy as np
import pytest
import torch

import unseen_ref as R
from deeprecommendation_amd import implicit

SEEDS = (0, 1, 12345, 0xFFFFFFFF)
SLOT0S = (0, 2 ** 33 + 7)


def _rows(n_items, rng):
    lengths = sorted({0, 1, n_items // 2, n_items - 1} & set(range(n_items)))
    return [np.sort(rng.choice(n_items, a, replace=False)) for a in lengths]


@pytest.mark.parametrize("n_items", [1, 5, 70, 1000])
def test_unrank_equals_the_explicit_complement(n_items):
    rng = np.random.default_rng(n_items)
    for A in _rows(n_items, rng):
        left = np.setdiff1d(np.arange(n_items), A)
        assert [R.unrank(n_items, A, r) for r in range(len(left))] == left.tolist()
        with pytest.raises(IndexError):
            R.unrank(n_items, A, len(left))


@pytest.mark.parametrize("n_items", [1, 5, 70, 1000])
def test_draws_are_distinct_unseen_and_in_range_and_a_split_call_equals_one_call(n_items):
    rng = np.random.default_rng(100 + n_items)
    rows = _rows(n_items, rng)
    rowptr = np.concatenate([[0], np.cumsum([len(A) for A in rows])])
    col = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    pick = rng.integers(0, len(rows), 23)
    for K in (1, 4, 9):
        out = R.draw_ref(rowptr, col, n_items, pick, K, 7, slot0=2 ** 33 + 7)
        for b, u in enumerate(pick):
            M = n_items - len(rows[u])
            if K > M:
                assert (out[b] == -1).all()
                continue
            assert len(set(out[b])) == K and out[b].min() >= 0 and out[b].max() < n_items and not set(out[b]) & set(rows[u])
            if K == M:
                assert sorted(out[b]) == np.setdiff1d(np.arange(n_items), rows[u]).tolist()
        parts = [R.draw_ref(rowptr, col, n_items, pick[a:b], K, 7, slot0=2 ** 33 + 7 + a) for a, b in ((0, 5), (5, 6), (6, 23))]
        assert np.array_equal(np.concatenate(parts), out)
    bad = R.draw_ref(rowptr, col, n_items, [-1, len(rows)], 1, 0)
    assert (bad == -1).all()


def test_the_formula_is_uniform_to_the_figures_of_its_issue():
    """200 000 consecutive slots, M = 20, j = 0 .. 3, over the 8 (seed, slot0) cases.  Every cell of the four marginal histograms lies
    within 5 binomial standard deviations of n / (M - j) — the bound: about 600 cells, whose worst measured 3.35 — and the chi-square of
    the (r_0, r_1) table against its 20 * 19 equally likely cells stays below 379 + 5 * sqrt(2 * 379) (379 degrees of freedom)."""
    n, M, K = 200_000, 20, 4
    worst = 0.0
    for seed in SEEDS:
        for slot0 in SLOT0S:
            r = R.ranks(seed, slot0 + np.arange(n, dtype=np.uint64), K, M)
            for j in range(K):
                m = M - j
                assert r[:, j].min() >= 0 and r[:, j].max() < m
                counts = np.bincount(r[:, j], minlength=m)
                p = 1.0 / m
                z = np.abs(counts - n * p) / np.sqrt(n * p * (1 - p))
                worst = max(worst, float(z.max()))
                assert z.max() <= 5.0, (seed, slot0, j, float(z.max()))
            table = np.bincount(r[:, 0] * (M - 1) + r[:, 1], minlength=M * (M - 1))
            e = n / (M * (M - 1))
            chi2 = float(((table - e) ** 2 / e).sum())
            assert chi2 < 379 + 5 * np.sqrt(2 * 379), (seed, slot0, chi2)
    print(f"worst cell: {worst:.2f} binomial standard deviations")


# ------------------------------------------------------------------ leave_one_out
def test_leave_one_out_by_time_with_a_tie_a_duplicate_and_a_one_item_user():
    #        user 0: items 3 (t 5), 7 (t 9), 2 (t 9): the tie at t = 9 goes to the larger item, 7
    #        user 1: item 4 twice (t 1 and t 8) and item 6 (t 5): the pair counts once, at its latest time, so 4 is held out
    #        user 2: one item only: kept, nothing held out;  user 4: item 1 twice: one distinct item, kept
    u = np.array([0, 1, 0, 2, 1, 0, 1, 4, 4])
    i = np.array([3, 4, 7, 9, 6, 2, 4, 1, 1])
    t = np.array([5, 1, 9, 3, 5, 9, 8, 2, 6])
    tu, ti, hu, hi = implicit.leave_one_out(u, i, t)
    assert list(zip(hu, hi)) == [(0, 7), (1, 4)]
    assert list(zip(tu, ti)) == [(0, 2), (0, 3), (1, 6), (2, 9), (4, 1)]
    assert all(a.dtype == np.int64 for a in (tu, ti, hu, hi))
    # torch tensors are taken too, and the order of the input does not matter
    perm = np.random.default_rng(0).permutation(len(u))
    again = implicit.leave_one_out(torch.from_numpy(u[perm]), torch.from_numpy(i[perm]), torch.from_numpy(t[perm]))
    assert all(np.array_equal(a, b) for a, b in zip(again, (tu, ti, hu, hi)))


def test_leave_one_out_by_hash_repeats_for_a_seed_and_follows_the_stated_pick():
    rng = np.random.default_rng(3)
    u, i = rng.integers(0, 30, 400), rng.integers(0, 50, 400)
    u, i = np.append(u, [40, 41, 41]), np.append(i, [5, 6, 6])          # users 40 and 41 have one distinct item
    a, b = implicit.leave_one_out(u, i, seed=11), implicit.leave_one_out(u, i, seed=11)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    tu, ti, hu, hi = a
    pairs = {(int(x), int(y)) for x, y in zip(u, i)}
    assert {(int(x), int(y)) for x, y in zip(tu, ti)} | {(int(x), int(y)) for x, y in zip(hu, hi)} == pairs
    assert len(tu) + len(hu) == len(pairs) and 40 not in hu and 41 not in hu and len(set(hu.tolist())) == len(hu)
    for user, item in zip(hu, hi):
        items = sorted(y for x, y in pairs if x == user)
        # the pick uses the two-round hash of (seed, user), restated here
        x = R.lowbias32(np.uint64((int(user) * 0x9E3779B1) & R.M32) ^ np.uint64(11))
        x = int(R.lowbias32(x ^ np.uint64(0x68E31DA4)))                # the user's high word is 0
        assert item == items[(x * len(items)) >> 32]
    other = implicit.leave_one_out(u, i, seed=12)
    assert not np.array_equal(other[3], hi)


# ------------------------------------------------------------------ refusals, before any device
def test_implicit_feedback_refuses_bad_positions_and_a_cpu_device():
    ok_u, ok_i = np.array([0, 1, 2]), np.array([0, 1, 4])
    for u, i in (([0, 1, 3], ok_i), ([-1, 1, 2], ok_i), (ok_u, [0, 1, 5]), (ok_u, [0, -2, 4])):
        with pytest.raises(ValueError, match="outside"):
            implicit.ImplicitFeedback(np.array(u), np.array(i), 3, 5, "cuda")
    with pytest.raises(ValueError):
        implicit.ImplicitFeedback(ok_u, ok_i[:2], 3, 5, "cuda")
    with pytest.raises(ValueError):
        implicit.ImplicitFeedback(ok_u.astype(np.float32), ok_i, 3, 5, "cuda")
    with pytest.raises(ValueError):
        implicit.ImplicitFeedback(ok_u, ok_i, 0, 5, "cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        implicit.ImplicitFeedback(ok_u, ok_i, 3, 5, "cpu")


def _mf():
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    return MF(item_dim=5, user_dim=3, item_emb=4, user_emb=4)


def test_fit_implicit_refuses_an_unsupported_model_a_bad_loss_and_bad_counts():
    fit = dict(epochs=1, batch_size=4, lr=0.1)
    with pytest.raises(TypeError, match="BasicNCF.*MF.*GraphNCF"):
        implicit.fit_implicit(torch.nn.Linear(2, 1), None, **fit)
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    with pytest.raises(TypeError, match="BasicNCF.*MF.*GraphNCF"):
        implicit.fit_implicit(AttentionNCF(item_dim=4, item_emb=8, user_emb=8, att_dense=8, mlp_dense_layers=[8]), None, **fit)
    for bad in (0, -1, 1.5, True, 1025):
        with pytest.raises(ValueError, match="negatives"):
            implicit.fit_implicit(_mf(), None, negatives=bad, **fit)
    with pytest.raises(ValueError, match="loss"):
        implicit.fit_implicit(_mf(), None, loss="mse", **fit)
    with pytest.raises(ValueError, match="graph"):
        implicit.fit_implicit(_mf(), None, graph=object(), **fit)
    with pytest.raises(TypeError, match="ImplicitFeedback"):
        implicit.fit_implicit(_mf(), None, **fit)


def test_eval_sampled_refuses_shapes_that_do_not_match():
    users, held, cand = torch.arange(3), torch.arange(3), torch.zeros((3, 4), dtype=torch.int64)
    for u, h, c in ((users, held[:2], cand), (users, held, cand[:2]), (users, held, cand[:, :0]), (users, held, cand.reshape(-1)),
                    (users, held.int(), cand), (users[:, None], held, cand)):
        with pytest.raises(ValueError, match="eval_sampled"):
            implicit.eval_sampled(_mf(), u, h, c)
    with pytest.raises(ValueError, match="cutoffs"):
        implicit.eval_sampled(_mf(), users, held, cand, cutoffs=(0,))
    with pytest.raises(TypeError, match="BasicNCF.*MF.*GraphNCF"):
        implicit.eval_sampled(torch.nn.Linear(2, 1), users, held, cand)
    with pytest.raises(RuntimeError, match="GPU"):                    # well-formed CPU tensors: there is no CPU path
        implicit.eval_sampled(_mf(), users, held, cand)


def test_the_package_exports_the_protocol():
    import deeprecommendation_amd as pkg
    for name in ("leave_one_out", "ImplicitFeedback", "fit_implicit", "sampled_candidates", "eval_sampled"):
        assert getattr(pkg, name) is getattr(implicit, name)


def test_sample_unseen_refuses_bad_arguments_before_the_device():
    from deeprecommendation_amd import native
    rowptr, col, pick = torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)
    for kw in (dict(k=0), dict(k=1025), dict(n_items=0), dict(n_items=2 ** 31), dict(slot0=-1), dict(seed=1.5), dict(pick=pick.int()),
               dict(seen=(rowptr.int(), col)), dict(seen=(rowptr, col.long())), dict(out=torch.zeros((1, 2), dtype=torch.int64))):
        args = dict(seen=(rowptr, col), n_items=5, pick=pick, k=1, seed=0)
        args.update(kw)
        with pytest.raises(ValueError, match="sample_unseen"):
            native.sample_unseen(**args)
    with pytest.raises(RuntimeError, match="GPU"):
        native.sample_unseen((rowptr, col), 5, pick, 1, 0)
    flag = torch.zeros(1, dtype=torch.int32)
    native.check_unseen(torch.device("cpu"), flag=flag)
    for word, exc, text in ((native.UNSEEN_FLAG_PICK, IndexError, "a pick outside the users"),
                            (native.UNSEEN_FLAG_FEW, ValueError, "a user has fewer unseen items than the draws asked for"),
                            (native.UNSEEN_FLAG_PICK | native.UNSEEN_FLAG_FEW, IndexError, "fewer unseen items")):
        flag.fill_(word)
        with pytest.raises(exc, match=text):
            native.check_unseen(torch.device("cpu"), flag=flag)
        assert int(flag) == 0
