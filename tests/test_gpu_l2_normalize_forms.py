"""native.l2_normalize_rows (l2_normalize_rows_kernel, csrc/attn.hip) against the float64 formula
x / max(sqrt(sum x^2), float(float32(1e-12))) on every form: widths on either side of the 16-lane sub-group, row counts on either
side of the four sub-groups of a wave (the Rpad rounding) and of a 16-row workgroup, both sides of the 8192-block grid cap, strided
input and output, and rows of zeros, one non-zero element, a norm below the clamp, a NaN and an infinity.

THE BAR.  |out - ref| <= (ceil(E/16) + 8) 2^-24 |ref| per element (prep_forms_ref.l2_bar): derived from the kernel's operation
order, not fitted to its output.  The largest ratio observed is recorded (conftest.record_error) and printed."""
import pytest
import torch
from conftest import record_error

import prep_forms_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = (1, 15, 16, 17, 64, 100, 257, 2094)
ROW_COUNTS = (1, 3, 4, 5, 15, 16, 17, 1000)
SENTINEL = -6.5


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def _hold_to_bar(out, x, E, tag):
    """out (device) against the float64 reference of x (CPU): NaN positions, exact zeros, +-1 of the single-element rows, the bar."""
    ref = R.l2_reference(x)
    out = out.cpu()
    ratio = R.l2_ratio(out, ref, E)
    print(f"l2_normalize {tag}: largest |out - ref| / bar = {ratio:.4f}")
    record_error(tag, ratio, 1.0)
    kind = torch.arange(x.shape[0]) % 8
    single = out[kind == 4]
    assert bool(((single == 0) | (single.abs() == 1)).all()) and bool((single.abs().sum(1) == 1).all())    # +-1 exactly
    assert torch.equal(single != 0, x[kind == 4] != 0)
    assert bool(torch.isnan(out[kind == 6]).all())                                                        # a NaN row is all NaN
    assert ratio <= 1.0, ratio
    return ratio


@pytest.mark.parametrize("E", WIDTHS)
def test_every_width_and_row_count(native, gpu, E):
    for Rn in ROW_COUNTS:
        x = R.l2_case(Rn, E, seed=21)
        wide = torch.full((Rn, E + 9), SENTINEL)
        wide[:, 5:5 + E] = x
        d = wide.to(gpu)
        out = native.l2_normalize_rows(d[:, 5:5 + E])                 # a column slice: ld = E + 9
        _hold_to_bar(out, x, E, f"E{E}_R{Rn}")
        again = native.l2_normalize_rows(d[:, 5:5 + E].contiguous())   # the same rows, contiguous, a second call: the same bits
        assert torch.equal(out.view(torch.int32), again.view(torch.int32))
        assert torch.equal(d.view(torch.int32), wide.to(gpu).view(torch.int32))          # the input is left alone


@pytest.mark.parametrize("Rn", [131072, 131077])
def test_both_sides_of_the_grid_cap(native, gpu, Rn):
    """8192 workgroups of 16 rows: R = 131 072 is the last single pass, 131 077 sends sub-groups 0..4 (and the padded 5..7 of
    Rpad = 131 080) into a second pass."""
    E = 16
    x = R.l2_case(Rn, E, seed=22)
    out = native.l2_normalize_rows(x.to(gpu))
    _hold_to_bar(out, x, E, f"E{E}_R{Rn}")
    assert torch.equal(out.view(torch.int32), native.l2_normalize_rows(x.to(gpu)).view(torch.int32))


@pytest.mark.parametrize("E,Rn", [(1, 5), (17, 17), (100, 37), (2094, 6)])
def test_strided_output_through_the_entry_point(native, gpu, E, Rn):
    """ncf_l2_normalize_rows with ldout > E: the side columns of the output keep their sentinel."""
    lib = native.load_library()
    x = R.l2_case(Rn, E, seed=23)
    d = x.to(gpu)
    wide = torch.full((Rn, E + 7), SENTINEL, device=gpu)
    rc = lib.ncf_l2_normalize_rows(d.data_ptr(), E, Rn, E, wide[:, 3:].data_ptr(), E + 7, torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == native.NCF_OK
    _hold_to_bar(wide[:, 3:3 + E], x, E, f"E{E}_R{Rn}_ldo")
    assert bool((wide[:, :3] == SENTINEL).all()) and bool((wide[:, 3 + E:] == SENTINEL).all())
    assert torch.equal(wide[:, 3:3 + E].contiguous().view(torch.int32), native.l2_normalize_rows(d).view(torch.int32))
    # R = 0 is a no-op; a leading dimension below E is refused and nothing is written
    before = wide.clone()
    assert lib.ncf_l2_normalize_rows(d.data_ptr(), E, 0, E, wide.data_ptr(), E + 7, None) == native.NCF_OK
    assert lib.ncf_l2_normalize_rows(d.data_ptr(), E, Rn, E + 8, wide.data_ptr(), E + 7, None) == native.NCF_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(wide.view(torch.int32), before.view(torch.int32))
