"""CPU tests of tests/attn_cross_ref.py: the float64 table formulation (logit table, then per user a gather, a column softmax and
the weighted sum) equals attention64 on the expanded (user, candidate) pairs; the fp32 emulator of attn_cross_kernel's index walk
passes the check the GPU test applies (attn_forms_ref.check_forward under the project's bar), and each of six seeded defects fails
it.  Also the host-only parts of the new entry points: ncf_attn_cross_supported / ncf_attn_cross_plan and the refusals."""
import os

import pytest
import torch

import attn_cross_ref as X
import attn_forms_ref as R
from test_gpu_basic import assert_close

MODES = [(R.ATT_MLP, 12), (R.ATT_MLP_SCALED, 8), (R.ATT_COS, 12), (R.ATT_LINEAR, 1)]
SHORT = (0, 1, 7, 33, 64, 65, 130)


def _close(got, ref, tag):
    assert_close(got, ref)


@pytest.fixture(scope="module")
def native():
    from deeprecommendation_amd import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    n.load_library()
    return n


@pytest.mark.parametrize("mode,A", MODES)
@pytest.mark.parametrize("subset", [False, True])
def test_table_formulation_equals_attention64_on_the_expanded_pairs(mode, A, subset):
    case = X.make_cross_case(mode, A, 10, 37, 11 + mode, lengths=SHORT, cand_subset=subset)
    got = X.cross64(case["st64"], case["rowptr"], case["col"], case["val"], case["user_rows"], case["cand_ids"], case["feat"],
                    torch.zeros(10) if case["bias"] is None else case["bias"])
    assert got.shape == case["out64"].shape == (case["U"] * case["I"], 10)
    assert torch.allclose(got, case["out64"], rtol=1e-12, atol=1e-13)
    dead = case["pair_dead"]
    assert bool(dead.any()) and torch.equal(got[dead], case["bias"].double().expand(int(dead.sum()), 10))
    # the case holds what it promises: a repeated user, users out of order, every row listed, an empty and an all-masked row
    rows = case["user_rows"].tolist()
    assert len(set(rows)) == case["n_rows"] < len(rows) and rows != sorted(rows)
    assert case["all_masked_row"] in rows
    if subset:
        ids = case["cand_ids"].tolist()
        assert len(set(ids)) == len(ids) - 1 and ids != sorted(ids) and len(set(ids)) < case["Ic"]


@pytest.fixture(scope="module")
def emu_case():
    case = X.make_cross_case(R.ATT_MLP, 8, 32, 300, 5, lengths=SHORT, cand_subset=True)
    assert case["I"] % X.CAND_TILE and case["I"] > X.CAND_TILE and case["Ic"] == case["Ir"]
    return case


def test_the_right_walk_passes_the_gpu_check(emu_case):
    st = emu_case["st64"].float()
    for per_call in (None, 4):
        R.check_forward(emu_case, X.emulate_cross(emu_case, st, users_per_call=per_call), None, _close, "emulator")


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_each_seeded_defect_fails_the_gpu_check(emu_case, defect):
    st = emu_case["st64"].float()
    per_call = 4 if defect == "block_offset_not_on_user_rows" else None
    with pytest.raises(AssertionError):
        R.check_forward(emu_case, X.emulate_cross(emu_case, st, defect=defect, users_per_call=per_call), None, _close, defect)


def test_supported_and_plan_are_host_only(native):
    lib = native.load_library()
    for Fdim in range(0, 321, 8):
        ok = Fdim % 32 == 0 and 32 <= Fdim <= 256
        assert native.attn_cross_supported(Fdim) == ok
        assert lib.ncf_attn_cross_supported(Fdim) == (1 if ok else native.NCF_EUNSUPPORTED)
        if ok:
            nb, te, lds, grid = native.attn_cross_plan(Fdim, 7, 300)
            assert (nb, te, grid) == (Fdim // 32, 64 if Fdim <= 128 else 32, 7 * 3) and lds == te * Fdim * 4 + te * 8 <= 64 * 1024
        else:
            with pytest.raises(native.NativeError) as e:
                native.attn_cross_plan(Fdim)
            assert e.value.code == native.NCF_EUNSUPPORTED
    assert native.attn_cross_plan(64, 0, 0)[3] == 0
    with pytest.raises(native.NativeError) as e:
        native.attn_cross_plan(64, 1 << 40, 1 << 40)                   # more workgroups than a grid holds
    assert e.value.code == native.NCF_EUNSUPPORTED


def test_entry_points_refuse_before_launching(native):
    """Refusals that need no device: stand-in pointers, every row refused (or accepted as empty) before anything is launched."""
    lib, P = native.load_library(), 16
    EINVAL, EUNSUP, OK = native.NCF_EINVAL, native.NCF_EUNSUPPORTED, native.NCF_OK
    cross = lambda **kw: lib.ncf_attn_cross(*{**dict(st=P, ldst=100, Ir=100, Ic=100, rowptr=P, col=P, val=P, n_rows=4, user_rows=P, U=4,
                                                     cand_ids=None, I=100, feat=P, ldfeat=64, Fdim=64, bias=None, out=P, ldout=64, oob=None,
                                                     stream=None), **kw}.values())
    assert cross(Fdim=48, ldfeat=48, ldout=48) == EUNSUP and b"Fdim" in lib.ncf_last_error()
    assert cross(Fdim=0) == EUNSUP and cross(Fdim=288, ldfeat=288, ldout=288) == EUNSUP
    assert cross(U=0, st=None) == OK and cross(I=0, cand_ids=P, st=None) == OK
    assert cross(st=None) == EINVAL and cross(user_rows=None) == EINVAL and cross(out=None) == EINVAL
    assert cross(ldst=99) == EINVAL and cross(ldfeat=63) == EINVAL and cross(ldout=63) == EINVAL
    assert cross(I=101) == EINVAL and b"dev_cand_ids" in lib.ncf_last_error()
    logits = lambda **kw: lib.ncf_attn_logits(*{**dict(mode=0, pc=P, ldpc=8, Ic=10, pr=P, ldpr=8, Ir=10, A=8, w1=P, b1=0.0, st=P, ldst=10,
                                                       stream=None), **kw}.values())
    assert logits(mode=4) == EINVAL and logits(A=0) == EINVAL and logits(w1=None) == EINVAL and logits(mode=3, w1=None) == EINVAL
    assert logits(mode=1) == EINVAL and b"linear" in lib.ncf_last_error()
    assert logits(ldst=9) == EINVAL and logits(ldpc=7) == EINVAL and logits(pc=None) == EINVAL
    assert logits(Ic=0, pc=None) == OK and logits(Ir=0, st=None) == OK
