"""CPU tests of the KernelMF baseline: the stratified epoch of tests/kmf_ref.py does not depend on the order of a stratum's blocks,
is the plain sequential pass at W = 1 and tracks its float64 twin; the plan holds every sample once, in its block; the two entry
points are declared, exported, bound and built with THE CONTRACT in the header; their refusals, the binding's and KernelMF's come
before the device."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import kmf_ref as K


def _lib():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load_library()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("F,W", [(65, 5), (4, 2), (100, 23), (3, 64)])
def test_block_order_inside_a_stratum_does_not_change_a_bit(F, W):
    mu, plan = K.ratings_case()[3], K.plan_case(W)
    (_, _, _), (P3, Q3, sse3) = K.epoch_case(F, W)
    P, Q = K.init_tables(F)
    sse = K.epoch_ref(P, Q, F, plan, mu, K.LR, K.REG, 3, reverse=True)
    assert np.array_equal(_bits(P), _bits(P3)) and np.array_equal(_bits(Q), _bits(Q3)) and np.array_equal(_bits(sse), _bits(sse3))


@pytest.mark.parametrize("F", [1, 65, 256])
def test_one_block_is_the_sequential_pass_over_the_input_order(F):
    us, it, r, mu = K.ratings_case()
    plan = K.plan_case(1)
    assert np.array_equal(plan["order"], np.arange(K.N)) and not plan["user_block"].any() and not plan["item_block"].any()
    (P1, Q1, sse1), _ = K.epoch_case(F, 1)
    P, Q = K.init_tables(F)
    acc = K.sequential_ref(P, Q, F, us, it, r, mu, K.LR, K.REG)
    assert np.array_equal(_bits(P), _bits(P1)) and np.array_equal(_bits(Q), _bits(Q1)) and sse1.shape == (1, 1) and sse1[0, 0] == acc


@pytest.mark.parametrize("W", K.W_LIST)
@pytest.mark.parametrize("n", [K.N, 1])
def test_plan_holds_every_sample_once_in_its_block(W, n):
    us, it, r, _ = K.ratings_case(n)
    plan = K.plan_case(W, n)
    ptr = plan["block_ptr"]
    assert ptr[0] == 0 and ptr[-1] == n and (np.diff(ptr) >= 0).all() and len(ptr) == W * W + 1
    assert np.array_equal(np.sort(plan["order"]), np.arange(n))
    assert np.array_equal(plan["user"], us[plan["order"]]) and np.array_equal(plan["item"], it[plan["order"]])
    assert np.array_equal(plan["rating"], r[plan["order"]])
    for s in range(W):
        for a in range(W):
            k = slice(ptr[s * W + a], ptr[s * W + a + 1])
            assert (plan["user_block"][plan["user"][k]] == a).all() and (plan["item_block"][plan["item"][k]] == (a + s) % W).all()
            assert (np.diff(plan["order"][k]) > 0).all()               # input order survives within a block
    for block, ids, count in ((plan["user_block"], us, K.U), (plan["item_block"], it, K.I)):
        sizes = np.bincount(block, minlength=W)
        assert sizes.max() - sizes.min() <= 1
        counts = np.bincount(ids, minlength=count)
        heavy = np.argsort(-counts, kind="stable")[:W]                 # the W heaviest ids sit in W different blocks
        assert len(set(block[heavy])) == min(W, count)


def test_fp32_loop_tracks_its_float64_twin_on_every_case():
    worst = 0.0
    for F in K.F_LIST:
        for W in K.W_LIST:
            (_, _, _), (P, Q, sse) = K.epoch_case(F, W)
            (_, _, _), (Pd, Qd, ssed) = K.epoch_case(F, W, dt=np.float64)
            dev = max(np.abs(P.astype(np.float64) - Pd).max(), np.abs(Q.astype(np.float64) - Qd).max())
            print(f"F={F} W={W}: max |fp32 - float64| = {dev:.3e} (max |entry| {max(np.abs(Pd).max(), np.abs(Qd).max()):.3f})")
            worst = max(worst, dev)
    print(f"worst {worst:.3e} = {worst * 2 ** 24:.2f} * 2^-24; recorded {K.F32_VS_F64_MEASURED:.3e}")
    assert worst <= 8 * K.F32_VS_F64_MEASURED


def test_float64_twin_train_rmse_falls_in_each_epoch():
    _, (_, _, sse) = K.epoch_case(65, 5, dt=np.float64)
    rmse = np.sqrt(sse.sum(1) / K.N)
    assert rmse[0] > rmse[1] > rmse[2] and rmse[2] < 0.8 * rmse[0]


def test_fold_in_leaves_the_item_table_and_other_users_alone():
    F = 65
    users, rowptr, col, rating = K.fold_case(F)
    P0, Q0 = K.init_tables(F)
    P, Q = P0.copy(), Q0.copy()
    sse, flag = K.fold_users_ref(P, Q, F, users, rowptr, col, rating, 2.75, K.LR, K.REG, 2)
    others = np.setdiff1d(np.arange(K.U), users)
    assert flag == 0 and np.array_equal(Q, Q0) and np.array_equal(P[others], P0[others])
    assert np.array_equal(P[11], P0[11]) and not np.array_equal(P[3], P0[3])      # user 11's row of the CSR is empty
    assert (sse[:, [0, 1, 3]] > 0).all() and not sse[:, 2].any() and (sse[1] <= sse[0]).all()


def test_entry_points_are_declared_exported_bound_and_built():
    from deeprecommendation_amd import native
    from deeprecommendation_amd.csrc import build
    hdr = open(os.path.join(ROOT, "include", "ncf_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+ncf_kmf_epoch\s*\(", code) and re.search(r"\bint\s+ncf_kmf_fold_users\s*\(", code)
    for line in ("column c (0 <= c < F) belongs to lane (c / 4) mod 64",
                 "part_l = +0.0f;  for the lane's columns in ascending order:  part_l = part_l + p[c] * q[c]",
                 "dot    = balanced tree over lanes 0..63 in lane order: adjacent pairs first, then pairs of pairs, ... (6 levels)",
                 "pred   = ((mu + bi) + bu) + dot", "err    = pred - r", "bu'    = bu - lr * (err + reg * bu)",
                 "bi'    = bi - lr * (err + reg * bi)", "for every c:  p'[c] = p[c] - lr * (err * q[c] + reg * p[c])",
                 "q'[c] = q[c] - lr * (err * p[c] + reg * q[c])      (both from the OLD p[c], q[c])"):
        assert line in hdr, line                                       # the contract is part of the ABI
    lib = _lib()
    for name, nargs in (("ncf_kmf_epoch", 22), ("ncf_kmf_fold_users", 20)):
        assert hasattr(lib, name) and len(native.SIGNATURES[name][1]) == nargs
    assert callable(native.kmf_epoch) and callable(native.kmf_fold_users)
    assert "kmf.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["kmf.hip"]
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd import baselines
    assert "KernelMF" in pkg._BASELINES and pkg.KernelMF is baselines.KernelMF


def test_epoch_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()
    a = 16                                       # a non-null, 16-byte aligned stand-in: every refusal comes before any launch
    inf, nan = float("inf"), float("nan")

    def call(PU=a, ldu=8, U=3, QI=a, ldq=8, I=4, F=7, user=a, item=a, rating=a, n=10, ptr=a, ub=a, ib=a, W=2, mu=3.0, lr=0.01, reg=0.1,
             epochs=1, sse=a, flag=a):
        return lib.ncf_kmf_epoch(PU, ldu, U, QI, ldq, I, F, user, item, rating, n, ptr, ub, ib, W, mu, lr, reg, epochs, sse, flag, None)

    assert call(n=0) == native.NCF_OK and call(epochs=0) == native.NCF_OK and call(n=0, user=None, item=None, rating=None) == native.NCF_OK
    assert call(epochs=0, sse=None, flag=None) == native.NCF_OK
    for bad in (dict(U=-1), dict(I=-1), dict(n=-1), dict(epochs=-1), dict(F=0), dict(F=-2), dict(ldu=7), dict(ldq=7), dict(W=0), dict(W=-1),
                dict(W=1025), dict(PU=None), dict(QI=None), dict(ptr=None), dict(ub=None), dict(ib=None), dict(user=None), dict(item=None),
                dict(rating=None), dict(lr=inf), dict(lr=nan), dict(reg=-inf), dict(reg=nan), dict(n=0, F=0), dict(epochs=0, W=0),
                dict(n=0, PU=None)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_kmf_epoch" in lib.ncf_last_error(), bad
    assert call(F=257, ldu=300, ldq=300) == native.NCF_EUNSUPPORTED and b"ncf_kmf_epoch" in lib.ncf_last_error()
    assert call(F=256, ldu=257, ldq=257, n=0) == native.NCF_OK and call(W=1024, n=0) == native.NCF_OK


def test_fold_refusals_come_before_any_launch():
    from deeprecommendation_amd import native
    lib = _lib()
    a = 16

    def call(PU=a, ldu=8, U=3, QI=a, ldq=8, I=4, F=7, users=a, nu=2, rowptr=a, col=a, rating=a, nnz=10, mu=3.0, lr=0.01, reg=0.1, epochs=1,
             sse=a, flag=a):
        return lib.ncf_kmf_fold_users(PU, ldu, U, QI, ldq, I, F, users, nu, rowptr, col, rating, nnz, mu, lr, reg, epochs, sse, flag, None)

    assert call(nu=0) == native.NCF_OK and call(epochs=0) == native.NCF_OK
    assert call(nu=0, nnz=0, PU=None, QI=None, users=None, rowptr=None, col=None, rating=None, sse=None, flag=None) == native.NCF_OK
    for bad in (dict(U=-1), dict(I=-1), dict(nu=-1), dict(nnz=-1), dict(epochs=-1), dict(F=0), dict(ldu=7), dict(ldq=7), dict(PU=None),
                dict(users=None), dict(rowptr=None), dict(QI=None), dict(col=None), dict(rating=None), dict(lr=float("nan")),
                dict(reg=float("inf")), dict(nu=0, F=0)):
        assert call(**bad) == native.NCF_EINVAL and b"ncf_kmf_fold_users" in lib.ncf_last_error(), bad
    assert call(F=300, ldu=301, ldq=301) == native.NCF_EUNSUPPORTED


def test_binding_refuses_mistyped_and_strided_tensors_before_the_device():
    from deeprecommendation_amd import native
    _lib()
    F, W = 3, 2
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    good = dict(PU=torch.zeros(5, 4), QI=torch.zeros(6, 32), F=F, user=i32(0, 1, 2), item=i32(0, 1, 2), rating=torch.ones(3),
                block_ptr=torch.tensor([0, 1, 2, 3, 3]), user_block=torch.zeros(5, dtype=torch.int32),
                item_block=torch.zeros(6, dtype=torch.int32), mu=3.0, lr=0.1, reg=0.1)
    for key, bad in (("PU", torch.zeros(5, 4, dtype=torch.float64)), ("PU", torch.zeros(5, 3)), ("PU", torch.zeros(4, 5).t()), ("PU", torch.zeros(20)),
                     ("QI", torch.zeros(6, 64)[:, ::2]), ("F", 0), ("F", 4), ("user", good["user"].long()), ("item", i32(0, 1)),
                     ("item", torch.zeros(6, dtype=torch.int32)[::2]), ("rating", torch.ones(3, dtype=torch.float64)), ("rating", torch.ones(4)),
                     ("block_ptr", good["block_ptr"].to(torch.int32)), ("block_ptr", torch.tensor([0, 1, 2, 3])), ("block_ptr", torch.tensor([0])),
                     ("user_block", torch.zeros(6, dtype=torch.int32)), ("item_block", torch.zeros(6, dtype=torch.int64)), ("n_epochs", -1),
                     ("sse", torch.zeros(1, 2)), ("sse", torch.zeros(3, dtype=torch.float64)), ("flag", torch.zeros(1)),
                     ("flag", torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            native.kmf_epoch(**dict(good, **{key: bad}))
    with pytest.raises(RuntimeError, match="GPU"):        # well-formed host tensors: only now the device is asked for
        native.kmf_epoch(**good)
    fold = dict(PU=good["PU"], QI=good["QI"], F=F, users=i32(1, 4), rowptr=torch.tensor([0, 2, 3]), col=i32(0, 5, 1), rating=torch.ones(3),
                mu=3.0, lr=0.1, reg=0.1)
    for key, bad in (("PU", torch.zeros(5, 3)), ("QI", torch.zeros(6, 32, dtype=torch.float16)), ("users", torch.tensor([1, 4])),
                     ("rowptr", torch.tensor([0, 2])), ("rowptr", fold["rowptr"].to(torch.int32)), ("col", fold["col"].long()),
                     ("rating", torch.ones(2)), ("n_epochs", -2), ("sse", torch.zeros(3, dtype=torch.float64)), ("F", 40)):
        with pytest.raises(ValueError):
            native.kmf_fold_users(**dict(fold, **{key: bad}))
    with pytest.raises(RuntimeError, match="GPU"):
        native.kmf_fold_users(**fold)


def test_kernel_mf_refuses_bad_arguments_before_the_device():
    import deeprecommendation_amd as pkg
    for bad in (dict(n_factors=0), dict(n_factors=257), dict(n_factors=2.5), dict(n_epochs=-1), dict(lr=0.0), dict(lr=float("nan")),
                dict(reg=-1.0), dict(reg=float("inf")), dict(init_sd=-0.1), dict(min_rating=5.0, max_rating=5.0), dict(n_blocks=0),
                dict(n_blocks=1025), dict(n_blocks=2.0), dict(lr="0.1")):
        with pytest.raises(ValueError):
            pkg.KernelMF(**bad)
    m = pkg.KernelMF(n_factors=8, n_epochs=4, n_blocks=2)
    u, i, r = torch.tensor([0, 1, 2]), torch.tensor([1, 0, 1]), torch.ones(3)
    for args in ((u.to(torch.int32), i, r, 3, 2), (u, i[:2], r, 3, 2), (u, i, r.double(), 3, 2), (u, i, torch.ones(4), 3, 2), (u[:0], i[:0], r[:0], 3, 2),
                 (u, i, r, 0, 2), (u, i, r, 3, 0), (u[None], i, r, 3, 2), (u.numpy(), i, r, 3, 2)):
        with pytest.raises(ValueError):
            m.fit(*args)
    for kw in (dict(at_epochs=(2, 2), epoch_callback=print), dict(at_epochs=(0,), epoch_callback=print), dict(at_epochs=(5,), epoch_callback=print),
               dict(at_epochs=(3, 1), epoch_callback=print), dict(at_epochs=(2,))):
        with pytest.raises(ValueError):
            m.fit(u, i, r, 3, 2, **kw)
    with pytest.raises(RuntimeError, match="GPU"):        # well-formed host tensors: only now the device is asked for
        m.fit(u, i, r, 3, 2)
    for call in (m.as_mf, m.check, lambda: m.predict(u, i), lambda: m.update_users(None, None, None, u)):
        with pytest.raises(RuntimeError, match="not fitted"):
            call()


def test_device_plan_builder_equals_the_restated_one():
    """KernelMF.build_plan is torch ops on whatever device the samples are on: on the host it must be tests/kmf_ref.py's plan."""
    import deeprecommendation_amd as pkg
    us, it, r, _ = K.ratings_case()
    for W in K.W_LIST:
        want = K.plan_case(W)
        got = pkg.KernelMF(n_factors=4).build_plan(torch.from_numpy(us.copy()), torch.from_numpy(it.copy()), torch.from_numpy(r.copy()), K.U, K.I, W)
        for k in ("user", "item", "rating", "block_ptr", "user_block", "item_block"):
            assert got[k].dtype == torch.from_numpy(want[k]).dtype and np.array_equal(got[k].numpy(), want[k]), (W, k)
        assert np.array_equal(got["user_count"].numpy(), np.bincount(us, minlength=K.U))
