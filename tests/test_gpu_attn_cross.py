"""ncf_attn_cross (csrc/attn_cross.hip): attention of listed users against a ranked list from the logit table, against the float64
reference attn_forms_ref.attention64 on the expanded (user, candidate) pairs, through attn_forms_ref.check_forward under the
project's bar (tests/attn_cross_ref.py builds the cases; tests/test_attn_cross_cpu.py shows that the check rejects six index defects).

The kernel gets the exact table (the cases' logits are exact in fp32), so what is tested is the gather, the masking, the softmax and
the aggregation on the matrix cores.  Every operand is a column slice of a wider poisoned buffer; the output starts as a sentinel."""
import numpy as np
import pytest
import torch

import attn_cross_ref as X
import attn_forms_ref as R
from test_gpu_basic import assert_close

pytestmark = pytest.mark.gpu

MODES = (R.ATT_MLP, R.ATT_MLP_SCALED, R.ATT_COS, R.ATT_LINEAR)
# (I_c, Fdim, cand_ids a shuffled subset with a repeat?, ldfeat or None): every I_c and every Fdim with and without cand_ids; the two
# entry tiles (64 entries for Fdim <= 128, 32 above); two feat buffers whose leading dimension takes the scalar staging
SHAPES = [(1, 32, False, None), (127, 64, False, None), (128, 128, False, None), (129, 256, False, None), (300, 64, False, None),
          (300, 256, False, None), (300, 128, True, None), (129, 32, True, None), (128, 64, True, None), (127, 256, True, None),
          (1, 128, True, None), (300, 32, True, None), (129, 64, False, 65), (300, 160, True, 163), (128, 96, False, None),
          (127, 224, True, None), (65, 192, False, None)]
CASES = [(MODES[k % 4], 1 if MODES[k % 4] == R.ATT_LINEAR else 8, F, Ic, 40 + k, sub, ld, k % 5 != 3) for k, (Ic, F, sub, ld) in enumerate(SHAPES)]


def _close(got, ref, tag):
    assert_close(got, ref)


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


class Dev:
    def __init__(self, case, gpu):
        Ic = case["Ic"]
        self.st = R.wide(case["st64"].float(), Ic + 4).to(gpu)[:, :Ic]
        self.feat = case["feat_buf"].to(gpu)[:, :case["Fdim"]]
        self.bias = None if case["bias_buf"] is None else case["bias_buf"].to(gpu)[:case["Fdim"]]
        self.rowptr, self.col, self.val = (case[k].to(gpu) for k in ("rowptr", "col", "val"))
        self.user_rows = case["user_rows"].to(gpu)
        self.cand_ids = None if case["cand_ids"] is None else case["cand_ids"].to(gpu)


def _run(native, case, d, gpu):
    out = X.fresh_out(case).to(gpu)
    got = native.attn_cross(d.st, d.rowptr, d.col, d.val, d.user_rows, d.feat, d.bias, cand_ids=d.cand_ids, out=out[:, :case["Fdim"]])
    assert got.data_ptr() == out.data_ptr()
    return out.cpu()


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"{R.MODE_NAMES[c[0]]}-F{c[2]}-Ic{c[3]}-{'ids' if c[5] else 'all'}-ld{c[6]}-{'b' if c[7] else 'nb'}")
def test_cross_attention_against_float64(native, gpu, c):
    case = X.cross_inputs(*c)
    assert case["ld"]["feat"] == (c[6] or c[2] + 4) and bool(case["pair_dead"].any())
    print("plan", native.attn_cross_plan(case["Fdim"], case["U"], case["I"]), "pairs", case["B"])
    d = Dev(case, gpu)
    out = _run(native, case, d, gpu)
    native.check_oob(gpu)
    R.check_forward(case, out, None, _close, "attn_cross")
    assert torch.equal(out, _run(native, case, d, gpu)), "two calls on the same inputs must give the same bits"


@pytest.mark.parametrize("k", [0, 6, 9])          # MLP / all candidates, COS / a subset, scaled MLP / a subset
def test_cross_agrees_with_the_grouped_kernel(native, gpu, k):
    """On the gathered operands native.attn_forward_grouped computes the same rows: both within the bar of float64, and of each other."""
    case = X.cross_inputs(*CASES[k])
    assert case["mode"] != R.ATT_LINEAR
    d = Dev(case, gpu)
    Fdim, U, I = case["Fdim"], case["U"], case["I"]
    cross = _run(native, case, d, gpu)[:, :Fdim]
    cands = torch.arange(case["Ic"]) if case["cand_ids"] is None else case["cand_ids"]
    pc = case["pc"][cands.repeat(U)].contiguous().to(gpu)
    w1 = None if case["w1"] is None else case["w1"].contiguous().to(gpu)
    grouped = native.attn_forward_grouped(case["mode"], pc, case["pr"].contiguous().to(gpu), w1, case["b1"], d.rowptr, d.col, d.val,
                                          case["user_rows"].repeat_interleave(I).to(gpu), d.feat.contiguous(),
                                          out_bias=None if d.bias is None else d.bias.contiguous()).cpu()
    native.check_oob(gpu)
    assert_close(grouped, case["out64"])
    assert_close(cross, case["out64"])
    assert_close(cross, grouped)


# ------------------------------------------------------------------------------------------------ a peaked softmax
def _peaked_case():
    """Linear-mode logits pc[i] + pr[e] (exact: pc odd multiples of 1/32 in [-1/2, 1/2], pr multiples of 1/16): users whose logits all lie
    in [82, 92] (exp overflows without the max subtraction) and in [-200, -190] (0 / 0 without it), and leaders with the rest 60 below,
    first, last and in the middle of the set."""
    rng = np.random.default_rng(99)
    noise = lambda n: rng.integers(-160, 161, n) / 16.0
    rows = [rng.integers(82 * 16, 92 * 16 + 1, 150) / 16.0, rng.integers(-200 * 16, -190 * 16 + 1, 150) / 16.0]
    for n, at in ((100, 0), (65, 64), (200, 130)):
        t = noise(n)
        t[at] = 70.0
        rows.append(t)
    lens = [len(t) for t in rows]
    Ir, Ic, Fdim = sum(lens) + 8, 130, 64
    rowptr = torch.zeros(len(rows) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(lens), 0)
    pr = torch.zeros(Ir, 1)
    pr[:sum(lens), 0] = torch.tensor(np.concatenate(rows), dtype=torch.float32)
    pc = torch.tensor((2 * rng.integers(-8, 8, (Ic, 1)) + 1) / 32.0, dtype=torch.float32)
    col = torch.arange(sum(lens), dtype=torch.int32)
    val = torch.tensor(rng.integers(1, 11, sum(lens)) * 0.5 - 2.9, dtype=torch.float32)
    g = torch.Generator().manual_seed(99)
    feat, bias = torch.randn(Ir, Fdim, generator=g), torch.randn(Fdim, generator=g)
    user_rows = torch.tensor([4, 0, 1, 2, 3, 1], dtype=torch.int64)
    U = user_rows.numel()
    st64 = X.table64(R.ATT_LINEAR, pc, pr, None, 0.0)
    assert torch.equal(st64, st64.float().double())
    out64, w64, _ = R.attention64(R.ATT_LINEAR, pc.double()[torch.arange(Ic).repeat(U)], pr.double(), None, 0.0, rowptr, col, val,
                                  user_rows.repeat_interleave(Ic), feat.double(), bias.double())
    assert float(w64.max()) >= 1 - 1e-12                             # a leader takes all the weight
    return dict(Fdim=Fdim, Ic=Ic, Ir=Ir, I=Ic, U=U, B=U * Ic, st64=st64, feat_buf=R.wide(feat, Fdim + 4), bias_buf=R.wide(bias[None], Fdim + 8)[0],
                bias=bias, rowptr=rowptr, col=col, val=val, user_rows=user_rows, cand_ids=None, out64=out64,
                pair_dead=torch.zeros(U * Ic, dtype=torch.bool), ld={"out": Fdim + 4}, x_col=torch.zeros(0, dtype=torch.int32))


def test_peaked_rows(native, gpu):
    case = _peaked_case()
    out = _run(native, case, Dev(case, gpu), gpu)
    assert bool(torch.isfinite(out).all())
    R.check_forward(case, out, None, _close, "attn_cross peaked")


# ------------------------------------------------------------------------------------------------ refusals and the sticky flag
def test_out_of_range_user_row_raises_at_check_oob(native, gpu):
    case = X.cross_inputs(*CASES[1])
    d = Dev(case, gpu)
    native.check_oob(gpu)
    d.user_rows = torch.tensor([2, case["n_rows"], 5, -1], dtype=torch.int64, device=gpu)
    Fdim, I = case["Fdim"], case["I"]
    out = native.attn_cross(d.st, d.rowptr, d.col, d.val, d.user_rows, d.feat, d.bias, cand_ids=d.cand_ids)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.check_oob(gpu)                                              # the raise reset the flag
    want = torch.zeros(Fdim) if case["bias"] is None else case["bias"]
    out = out.cpu().view(4, I, Fdim)
    assert torch.equal(out[1], want.expand(I, Fdim)) and torch.equal(out[3], want.expand(I, Fdim))       # the refused users: bias rows
    ids = torch.arange(case["Ic"], dtype=torch.int64, device=gpu)
    ids[3] = case["Ic"]
    out = native.attn_cross(d.st, d.rowptr, d.col, d.val, d.user_rows[:1], d.feat, d.bias, cand_ids=ids).cpu()
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    assert torch.equal(out[3], want)


@pytest.mark.parametrize("Fdim", [0, 48, 288])
def test_unsupported_widths_are_refused(native, gpu, Fdim):
    assert not native.attn_cross_supported(Fdim)
    case = X.cross_inputs(*CASES[1])
    d = Dev(case, gpu)
    feat = torch.zeros((case["Ir"], Fdim), device=gpu)
    with pytest.raises(native.NativeError) as e:
        native.attn_cross(d.st, d.rowptr, d.col, d.val, d.user_rows, feat)
    assert e.value.code == native.NCF_EUNSUPPORTED
