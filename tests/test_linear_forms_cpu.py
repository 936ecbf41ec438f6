"""CPU tests of the generic Linear's case table and references (tests/linear_forms_ref.py): the launch plan of every row (asked
through ncf_linear_plan, host only), the coverage the table claims, and the two checks the GPU tests hold the kernels to
(tests/test_gpu_linear_forms.py), run here against CPU models of a split-K Linear.  The right model passes; each wrong model is
rejected by the exact check.  That is what shows the GPU tests fail for a subtly wrong kernel."""
import os

import pytest
import torch

import linear_forms_ref as R


@pytest.fixture(scope="module")
def native():
    from deeprecommendation_amd import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    n.load_library()
    return n


def _plan_under(native, c, M=None):
    try:
        R.set_case_options(native.set_option, c)
        return native.linear_plan(c.M if M is None else M, c.N, c.K)
    finally:
        native.set_option("linear_kernel", "auto")
        native.set_option("linear_kslices", "auto")


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_plan_of_every_row(native, c):
    assert _plan_under(native, c) == c.plan
    assert _plan_under(native, c, M=0) == ("none", 0, 1, 1, 0)


def test_plan_is_host_only_and_checks_its_arguments(native):
    lib = native.load_library()
    assert lib.ncf_linear_plan(5, 0, 3, None, None, None, None, None) == native.NCF_EINVAL
    assert lib.ncf_linear_plan(-1, 4, 3, None, None, None, None, None) == native.NCF_EINVAL
    assert lib.ncf_linear_plan(5, 4, 0, None, None, None, None, None) == native.NCF_EINVAL
    assert lib.ncf_linear_plan(5, 4, 3, None, None, None, None, None) == native.NCF_OK      # any output may be NULL
    assert native.get_option("linear_kernel") == 0 and native.get_option("linear_kslices") == 0


def test_table_reaches_every_form():
    plans = [c.plan for c in R.CASES]
    kinds = {p[:4] for p in plans}
    assert ("tiled" in {p[0] for p in plans}) and ("rowdot" in {p[0] for p in plans})
    for nt in (1, 2, 4):
        for ks in (1, 2, 4):
            assert ("rs", nt, ks, 1) in kinds, (nt, ks)
    assert ("rs", 8, 1, 1) in kinds
    for ks in (4, 8):
        for cb in (2, 4):
            assert ("rs", 1, ks, cb) in kinds, (ks, cb)
    for nt in (1, 2, 4, 8):
        assert ("rsp", nt, 1, 1) in kinds, nt
    assert {1, 2, 3} <= {R.rsp_tiles_per_wave(c) for c in R.CASES if c.plan[0] == "rsp"}
    # the edges the table's comments name
    assert any(c.plan[0] == "rsp" and (c.M + 31) // 32 < 4 * c.plan[4] for c in R.CASES)          # waves without a tile
    assert any(c.plan[0] == "rowdot" and c.M * c.N > 16384 * 16 for c in R.CASES)                 # past the grid cap
    assert any(c.plan[0] == "tiled" and c.N in (32, 64, 128, 256) and c.K < 8 for c in R.CASES)
    assert any(c.plan[0] == "tiled" and c.plan[3] >= 3 for c in R.CASES)
    assert max(c.K for c in R.CASES) == R.K_MAX
    assert len({(c.M, c.N, c.K, c.force, c.ks) for c in R.CASES}) == len(R.CASES)


# ------------------------------------------------------------------------------------------------ CPU models of a kernel
FAULTS = ("drop_group", "last_group_twice", "tail_unguarded", "prev_tile_rows", "bias_per_slice", "relu_per_slice")


def model(x, w, b, relu, ks=1, fault=None):
    """A split-K Linear as the row-streaming kernels organise it: K in 8-groups, groups [s Q / ks, (s + 1) Q / ks) to slice s, the
    ragged tail (zero-filled to a whole group) to the last slice, slices added, then bias, then ReLU, rows in tiles of 32.
    float64 on integer data is exact, so only ``fault`` separates it from the reference."""
    M, K = x.shape
    Q = K // 8
    xd, wd = x.double(), w.double()
    if K % 8:
        pad = 8 * Q + 8 - K
        if fault == "tail_unguarded":          # the elements after the row's end: the next row's first ones (1 after the last row)
            xd = torch.cat((xd, torch.cat((xd[1:, :pad], torch.ones(1, pad, dtype=xd.dtype)))), 1)
            wd = torch.cat((wd, torch.cat((wd[1:, :pad], torch.ones(1, pad, dtype=wd.dtype)))), 1)
        else:
            xd = torch.nn.functional.pad(xd, (0, pad))
            wd = torch.nn.functional.pad(wd, (0, pad))
    G = xd.shape[1] // 8                       # groups, the tail's included
    bd = torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b.double()
    out = torch.zeros(M, w.shape[0], dtype=torch.float64)
    for s in range(ks):
        lo, hi = s * Q // ks, ((s + 1) * Q // ks if s < ks - 1 else G)
        groups = [g for g in range(lo, hi) if not (fault == "drop_group" and g == Q // 2)]
        if fault == "last_group_twice" and s == ks - 1:
            groups.append(Q - 1)
        cols = torch.tensor([8 * g + j for g in groups for j in range(8)], dtype=torch.long)
        part = xd[:, cols] @ wd[:, cols].t()
        if fault == "bias_per_slice" or (fault == "relu_per_slice" and s == 0):
            part = part + bd
        if fault == "relu_per_slice" and relu:
            part = torch.relu(part)
        out += part
    if fault not in ("bias_per_slice", "relu_per_slice"):
        out += bd
    if relu and fault != "relu_per_slice":
        out = torch.relu(out)
    if fault == "prev_tile_rows":
        t0 = 32 * ((M - 1) // 32)
        out[t0:] = out[t0 - 32:M - 32]
    return out.float()


def _ints(c, seed=0):
    return R.int_operands(c.M, c.N, c.K, torch.Generator().manual_seed(1000 * seed + c.M + c.N + c.K))


SMALL = [c for c in R.CASES if c.M * c.N * c.K <= 40_000_000]


@pytest.mark.parametrize("c", SMALL, ids=R.case_id)
def test_right_model_meets_the_exact_check(c):
    """... and the float64 route of the reference is the plain int64 product."""
    x, w, b = _ints(c)
    ks = c.plan[2]
    for relu in (False, True):
        for bias in (b, None):
            assert R.exact_check(model(x, w, bias, relu, ks), x, w, bias, relu)
    plain = x.long() @ w.long().t() + b.long()
    assert torch.equal(R.exact_reference(x, w, b, False), plain) and torch.equal(R.exact_reference(x, w, b, True), plain.clamp_min(0))
    assert int(plain.abs().max()) <= 49 * c.K + 7 < 2 ** 24


def _row(M, N, K):
    return next(c for c in R.CASES if (c.M, c.N, c.K) == (M, N, K))


# rows for the wrong models: a tail and more than one tile everywhere; one, two, four and eight slices
WRONG_ROWS = [_row(40, 256, 143), _row(70, 64, 63), _row(100, 64, 135), _row(70, 128, 1055), _row(129, 65, 33)]


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("c", WRONG_ROWS, ids=R.case_id)
def test_wrong_models_fail_the_exact_check(c, fault):
    ks = c.plan[2]
    if fault in ("bias_per_slice", "relu_per_slice") and ks == 1:
        ks = 4                                     # these two faults need slices: model the row as a 4-slice kernel would run it
    x, w, b = _ints(c, seed=1)
    assert c.K % 8 and c.M > 32 and c.K >= 16
    assert R.exact_check(model(x, w, b, True, ks), x, w, b, True)
    assert not R.exact_check(model(x, w, b, True, ks, fault), x, w, b, True), fault
    if fault != "relu_per_slice":
        assert not R.exact_check(model(x, w, b, False, ks, fault), x, w, b, False), fault


def test_fp32_matmul_stays_inside_the_bound_on_every_row():
    """torch's fp32 matmul on the CPU is a correct fp32 Linear whatever its blocking: inside the bound on every row of the table,
    with ReLU and without; its worst use of the bound is printed."""
    worst, where = 0.0, None
    for c in R.CASES:
        x, w, b = R.random_operands(c.M, c.N, c.K, torch.Generator().manual_seed(c.M + c.N + c.K))
        out = torch.nn.functional.linear(x, w, b)
        for relu in (False, True):
            ok, frac, err, bound, _ = R.bound_check(torch.relu(out) if relu else out, x, w, b, relu)
            assert ok, (R.case_id(c), frac, err, bound)
            if frac > worst:
                worst, where = frac, R.case_id(c)
    print(f"fp32 CPU matmul: worst use of the bound {worst:.4f} at {where}")
    assert 0.0 < worst < 1.0


def test_bound_check_rejects_an_error_of_one_group():
    """A dropped 8-group on random data is far outside the bound (the bound is no looser than the old 1e-5 bar here), a NaN
    is outside it, and one rounding of the output (half an ulp) is inside it."""
    c = _row(100, 64, 135)
    x, w, b = R.random_operands(c.M, c.N, c.K, torch.Generator().manual_seed(3))
    ref = R.reference64(x, w, b, False)
    assert R.bound_check(ref.float(), x, w, b, False)[0]
    bad = (ref - x[:, 8:16].double() @ w[:, 8:16].double().t()).float()
    assert not R.bound_check(bad, x, w, b, False)[0]
    nan = ref.float().clone()
    nan[5, 7] = float("nan")
    assert not R.bound_check(nan, x, w, b, False)[0]
