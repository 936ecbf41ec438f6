"""The attention kernels of csrc/attn.hip on every launch form they can take, against the float64 reference of
tests/attn_forms_ref.py (which holds the case tables, the inputs and the checks; tests/test_attn_forms_cpu.py shows on the CPU that
the checks reject ten index defects).

The calls go through the C ABI directly: every operand is a column slice of a wider buffer whose padding is poisoned, and every
output buffer, padding included, starts as a sentinel.  A lane that reads past its row, a row that is never written and a store
past the row all show."""
import pytest
import torch

import attn_forms_ref as R
from conftest import record_error
from test_gpu_basic import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    assert (n.ATT_MLP, n.ATT_LINEAR, n.ATT_COS, n.ATT_MLP_SCALED, n.ATT_SCALE_LOG2) == (R.ATT_MLP, R.ATT_LINEAR, R.ATT_COS, R.ATT_MLP_SCALED, R.SCALE_LOG2)
    return n


def _close(got, ref, tag):
    assert_close(got, ref)                                          # the project's bar; records its margin itself


def _bar_check(got, ref, bar, tag):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, tag
    err = (got - ref).abs()
    used = err / bar.clamp_min(1e-300)
    k = int(used.argmax())
    record_error(tag, float(err.flatten()[k]), float(bar.flatten()[k]))
    print(f"{tag}: max err {float(err.max()):.3e}, worst {float(used.max()):.3f} of its bar")
    assert bool((err <= bar).all()), f"{tag}: max err {float(err.max()):.3e}, worst {float(used.max()):.2f} of its bar"


def _p(t):
    return None if t is None else t.data_ptr()


class Dev:
    """The case's operands on the device (buffers keep their padding)."""

    def __init__(self, case, gpu):
        for k in ("pc_buf", "pr_buf", "feat_buf", "w1_buf", "bias_buf", "rowptr", "col", "val", "pair_row", "x_rowptr", "x_col", "x_val"):
            setattr(self, k, None if case[k] is None else case[k].to(gpu))
        self.w1, self.bias = self.w1_buf, self.bias_buf             # the kernels get the heads of the poisoned vectors


def _forward(native, case, d, gpu):
    out, wts = (t.to(gpu) for t in R.fresh_outputs(case))
    ld = case["ld"]
    rc = native.load_library().ncf_attn_forward(case["mode"], _p(d.pc_buf), ld["pc"], _p(d.pr_buf), ld["pr"], case["A"], _p(d.w1), case["b1"],
                                                _p(d.x_rowptr), _p(d.x_col), _p(d.x_val), case["B"], case["I"], _p(d.feat_buf), ld["feat"],
                                                case["Fdim"], _p(d.bias), _p(out), ld["out"], _p(wts), native._stream(out))
    torch.cuda.synchronize()
    return rc, out.cpu(), wts.cpu()


# ------------------------------------------------------------------------------------------------ per-pair forward
@pytest.mark.parametrize("c", R.PER_PAIR_CASES, ids=R.case_id)
def test_per_pair_forward_forms(native, gpu, c):
    case = R.per_pair_inputs(c)
    ld = case["ld"]
    print("form", R.per_pair_form(c.A, ld["pc"], ld["pr"], c.Fdim, ld["feat"], ld["out"], c.mode), "grid", R.per_pair_grid(c.B))
    d = Dev(case, gpu)
    rc, out, wts = _forward(native, case, d, gpu)
    assert rc == native.NCF_OK, native.load_library().ncf_last_error()
    R.check_forward(case, out, wts, _close, "attn_kernel")
    rc2, out2, wts2 = _forward(native, case, d, gpu)
    assert rc2 == native.NCF_OK and torch.equal(out, out2) and torch.equal(wts, wts2)


# ------------------------------------------------------------------------------------------------ backward
def _backward(native, case, d, dout_buf, wts, gpu, lds=None):
    got = {k: v.to(gpu) for k, v in R.fresh_gradients(case).items()}
    ds = torch.full((case["x_col"].numel() + R.WTS_PAD,), R.SENTINEL, device=gpu)
    ld = dict(case["ld"], **(lds or {}))
    rc = native.load_library().ncf_attn_backward(case["mode"], _p(d.pc_buf), ld["pc"], _p(d.pr_buf), ld["pr"], case["A"], _p(d.w1), _p(d.x_rowptr),
                                                 _p(d.x_col), _p(d.x_val), case["B"], case["I"], _p(d.feat_buf), ld["feat"], case["Fdim"], _p(wts),
                                                 _p(dout_buf), ld["dout"], _p(got["d_pc"]), ld["d_pc"], _p(got["d_pr"]), ld["d_pr"],
                                                 _p(got["d_w1_part"]), _p(got["d_feat"]), ld["d_feat"], _p(ds), 0, 0.0,
                                                 native._stream(ds))
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in got.items()}, ds.cpu()


@pytest.mark.parametrize("c", R.BACKWARD_CASES, ids=R.case_id)
def test_backward_forms(native, gpu, c):
    """The weights given to the kernel are the float64 reference's, rounded to fp32 (6e-8 relative, far inside the bars): the backward
    is tested on its own, not through the forward kernel."""
    case, dout, dout_buf = R.backward_inputs(c)
    print("form (LPA, LPF)", R.backward_form(c.A, c.Fdim))
    assert native.attn_backward_supported(c.mode, c.A, c.Fdim)
    d = Dev(case, gpu)
    wts = torch.cat((case["w64"].float(), torch.full((R.WTS_PAD,), R.SENTINEL))).to(gpu)
    rc, got, ds = _backward(native, case, d, dout_buf.to(gpu), wts, gpu)
    assert rc == native.NCF_OK, native.load_library().ncf_last_error()
    assert bool((ds[case["x_col"].numel():] == R.SENTINEL).all())
    R.check_backward(case, dout, got, _close, _bar_check, "attn_backward")


def test_backward_refusals_match_the_binding(native, gpu):
    """native.attn_backward_supported == (the call returns NCF_OK) over a grid of (mode, A, Fdim); a refused call writes nothing."""
    seen = set()
    for mode in (R.ATT_MLP, R.ATT_LINEAR, R.ATT_COS, R.ATT_MLP_SCALED):
        for A in ((1,) if mode == R.ATT_LINEAR else (4, 6, 64, 256, 260)):
            for Fdim in (3, 4, 50, 256, 260):
                case = R.make_inputs(mode, A, Fdim, [9, 0, 17], [1, 1, 2], 7, lds={"dout": Fdim + 4}, masked_row_pairs=0)
                d = Dev(case, gpu)
                dout_buf = R.wide(torch.ones(case["B"], Fdim), Fdim + 4).to(gpu)
                wts = torch.cat((case["w64"].float(), torch.full((R.WTS_PAD,), R.SENTINEL))).to(gpu)
                got0 = R.fresh_gradients(case)
                rc, got, ds = _backward(native, case, d, dout_buf, wts, gpu)
                ok = native.attn_backward_supported(mode, A, Fdim)
                assert (rc == native.NCF_OK) == ok, (mode, A, Fdim, rc)
                seen.add(ok)
                if not ok:
                    assert rc == native.NCF_EUNSUPPORTED
                    assert all(torch.equal(got[k], got0[k]) for k in got0) and bool((ds == R.SENTINEL).all()), (mode, A, Fdim)
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------ grouped forms
def _grouped(native, case, d, grp, c, weights, gpu):
    out, wts = (None if t is None else t.to(gpu) for t in R.fresh_outputs(case, weights))
    off = None
    if weights:
        lens = (case["x_rowptr"][1:] - case["x_rowptr"][:-1])
        off = (torch.cumsum(lens, 0) - lens).contiguous().to(gpu)
    grp_ptr, pair_ids, wg_ptr = grp
    ld = case["ld"]
    rc = native.load_library().ncf_attn_forward_grouped(case["mode"], _p(d.pc_buf), ld["pc"], _p(d.pr_buf), ld["pr"], case["A"], _p(d.w1), case["b1"],
                                                        _p(d.rowptr), _p(d.col), _p(d.val), case["R"], case["I"], _p(grp_ptr), _p(pair_ids), _p(wg_ptr),
                                                        case["B"], c.ppw, _p(d.feat_buf), ld["feat"], case["Fdim"], _p(d.bias), _p(out), ld["out"],
                                                        _p(wts), _p(off), native._stream(out))
    torch.cuda.synchronize()
    return rc, out.cpu(), None if wts is None else wts.cpu()


@pytest.mark.parametrize("c", R.GROUPED_CASES, ids=R.case_id)
def test_grouped_forms(native, gpu, kernel_option, c):
    kernel_option("attn_grouped_kernel", c.force)
    case = R.grouped_inputs(c)
    want = R.grouped_form(c.mode, c.A, c.Fdim, c.ldfeat, c.ppw, c.force)
    assert want is not None
    plan = native.attn_grouped_plan(c.mode, c.A, c.Fdim, c.ldfeat, c.ppw, case["B"], case["R"])
    assert plan == want[0] + (want[1], R.grouped_grid(case["B"], case["R"], c.ppw)), (plan, want)
    if c.force == "auto":
        assert plan[0] == ("sc" if c.Fdim % 4 == 0 and c.ldfeat % 4 == 0 else "lds")
    else:
        assert plan[0] == {"scalar": "sc", "lds": "lds"}[c.force]
    print("plan", plan)
    d = Dev(case, gpu)
    grp = native.group_pairs(d.pair_row, case["R"], c.ppw)
    native.check_oob(gpu)
    for weights in (False, True):
        what = f"attn_grouped_{plan[0]}" + ("_w" if weights else "")
        rc, out, wts = _grouped(native, case, d, grp, c, weights, gpu)
        assert rc == native.NCF_OK, native.load_library().ncf_last_error()
        R.check_forward(case, out, wts, _close, what)
        rc2, out2, wts2 = _grouped(native, case, d, grp, c, weights, gpu)
        assert rc2 == native.NCF_OK and torch.equal(out, out2) and (wts is None or torch.equal(wts, wts2))
