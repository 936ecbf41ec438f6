"""CPU tests of the bf16 contract checks (tests/bf16_contract_ref.py): before a GPU kernel is held to them (tests/test_gpu_bf16_contract.py)
the checks are run against CPU models of a bf16 scorer, through the same probe weights.  The right model (operands in bf16, fp32
``torch.matmul``, the first of two hidden layers re-rounded to nearest even, everything else in fp32) passes every one of them; each wrong
model is rejected by the checks named beside it in WRONG.  That is what shows the GPU tests fail for a subtly wrong kernel."""
import pytest
import torch

import bf16_contract_ref as R

SHAPES = [(64, 64), (128, 128), (192, 64)]
B_EXACT, B_RANDOM = 4096, 1024


def _round32(h, mode):
    """fp32 -> bf16 precision, as fp32: "rne" is the hardware conversion; the wrong ones go through the float64 restatement (exact: an
    fp32 number rounded to 8 bits is an fp32 number)."""
    return h.to(torch.bfloat16).float() if mode == "rne" else R.round_bf16(h, mode).float()


class Model:
    """A bf16 scorer on the CPU for one batch of rows ``x`` (fp32 holding bf16 numbers).  ``fault`` names what it gets wrong:
    None, "trunc", "half_up", "relu_before_bias", "h2_bf16", "last_bf16", "swap" (two hidden units change pack slots: the two of largest bias, which are alive whatever the rows)."""

    def __init__(self, x, fault=None):
        self.x, self.fault, self._l1 = x.float(), fault, None

    def _layer1(self, w, b):
        if self._l1 is None or self._l1[0] is not w:              # layer 1 does not depend on the probe: computed once per W1
            acc = self.x @ w.to(torch.bfloat16).float().t()
            h = torch.relu(acc) + b if self.fault == "relu_before_bias" else torch.relu(acc + b)
            self._l1 = (w, h)
        return self._l1[1]

    def __call__(self, ws, bs):
        h = self._layer1(ws[0], bs[0])
        if len(ws) == 3:
            h = _round32(h, self.fault if self.fault in ("trunc", "half_up") else "rne")
            if self.fault == "swap":
                i, j = bs[0].topk(2).indices.tolist()
                h = h.clone()
                h[:, [i, j]] = h[:, [j, i]]
            h = torch.relu(h @ ws[1].to(torch.bfloat16).float().t() + bs[1])
            if self.fault == "h2_bf16":
                h = _round32(h, "rne")
        wl = ws[-1].to(torch.bfloat16).float() if self.fault == "last_bf16" else ws[-1]
        return (h @ wl.t() + bs[-1])[:, 0]


# fault -> the checks that must reject it ("exact": Part A's bit-for-bit comparison; the others are Part B's, by Check.name)
WRONG = {"trunc": {"exact", "layer 1"}, "half_up": {"exact"}, "relu_before_bias": {"exact", "layer 1"},
         "h2_bf16": {"exact", "layer 2"}, "last_bf16": {"last layer"}, "swap": {"exact", "layer 1"}}


def _exact_rows(EA, EB, hidden):
    ta, tb, ws, bs = R.exact_case(EA, EB, hidden)
    ia, ib = R.batch_ids(B_EXACT, (ta.shape[0], tb.shape[0]), seed=B_EXACT)
    return R.gather_rows(ta, ia, tb, ib), ws, bs


def _random_rows(EA, EB, hidden):
    ta, tb, ws, bs, state = R.ncf_case(EA, EB, hidden)
    ia, ib = R.batch_ids(B_RANDOM, (ta.shape[0], tb.shape[0]), seed=B_RANDOM)
    return R.gather_rows(ta, ia, tb, ib), ws, bs, state, ia, ib


def _failed(EA, EB, fault):
    """Names of the checks that reject the model with ``fault`` at hidden [256, 128]."""
    x, ws, bs = _exact_rows(EA, EB, [256, 128])
    failed = set() if torch.equal(Model(x, fault)(ws, bs).double(), R.contract64(x, ws, bs)[0]) else {"exact"}
    x, ws, bs, _, _, _ = _random_rows(EA, EB, [256, 128])
    checks, share, repeat_equal = R.contract_checks(Model(x, fault), x, ws, bs)
    assert repeat_equal
    return failed | {c.name for c in checks if not c.ok}, checks, share


def test_rounding_restatement_matches_the_hardware_conversion():
    """round_bf16("rne") is torch's fp32 -> bf16 conversion on every fp32 pattern tried, ties and binade edges included; truncation is the
    pattern with its low 16 bits cleared; half-up differs from RNE exactly on the ties whose kept part is even."""
    g = torch.Generator().manual_seed(0)
    bits = torch.randint(0x38000000, 0x47000000, (200_000,), generator=g, dtype=torch.int32)       # 2^-15 .. 2^15
    bits[:70_000] = (bits[:70_000] & ~0xFFFF) | 0x8000                                              # exact ties
    bits[70_000:80_000] |= 0x7FFF                                                                  # just below a tie / a binade edge
    v = torch.cat((bits.view(torch.float32), -bits.view(torch.float32), torch.zeros(1)))
    assert torch.equal(R.round_bf16(v).float(), v.to(torch.bfloat16).float())
    assert torch.equal(R.round_bf16(v, "trunc").float(), (v.view(torch.int32) & ~0xFFFF).view(torch.float32))
    up, rne = R.round_bf16(v, "half_up"), R.round_bf16(v)
    tie_even = ((v.view(torch.int32) & 0xFFFF) == 0x8000) & ((v.view(torch.int32) & 0x10000) == 0)
    assert torch.equal(up != rne, tie_even) and bool(R.is_bf16(rne.float()).all())
    assert torch.equal(R.ulp_bf16(torch.tensor([0.0, 1.0, 1.99, 2.0, 255.0, 256.0, 0.75])).float(),
                       torch.tensor([0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0, 2.0 ** -8]))


def test_rounding_census_counts_by_hand():
    """256 .. 264 step 1 in the binade [256, 512) (spacing 2): 257 / 261 tie downwards (kept part even), 259 / 263 upwards;
    512.5 and 515.5 in [512, 1024) (spacing 4) round downwards and upwards without a tie."""
    c = R.rounding_census(torch.tensor([256.0, 257.0, 258.0, 259.0, 260.0, 261.0, 263.0, 512.5, 515.5, -4.0]))
    assert (c["tie_down"], c["tie_up"], c["down"], c["up"]) == (2, 2, 1, 1) and c["negative_share"] == 0.1


@pytest.mark.parametrize("hidden", [[256, 128], [256]])
@pytest.mark.parametrize("EA,EB", SHAPES)
def test_exact_cases_meet_their_conditions_and_the_right_model(EA, EB, hidden):
    """Part A without a GPU: the integer construction satisfies every condition the GPU test relies on (exact partial sums, enough
    roundings of every kind, truncation and half-up each change more than 90 % of the scores), and the right model equals the float64
    contract bit for bit."""
    x, ws, bs = _exact_rows(EA, EB, hidden)
    for name, holds, detail in R.exact_conditions(x, ws, bs):
        assert holds, (name, detail)
    assert torch.equal(Model(x)(ws, bs).double(), R.contract64(x, ws, bs)[0])


def test_exact_case_out_of_range_ids_read_as_zero_rows():
    ta, tb, ws, bs = R.exact_case(64, 64, [256, 128])
    ia, ib = torch.tensor([3, 3000, 5, -1, 7]), torch.tensor([1, 2, 700, 4, 699])
    x = R.gather_rows(ta, ia, tb, ib)
    assert float(x[1, :64].abs().sum()) == 0 and float(x[3, :64].abs().sum()) == 0 and float(x[2, 64:].abs().sum()) == 0
    assert torch.equal(x[0], torch.cat((ta[3], tb[1])).double()) and torch.equal(x[4, 64:], tb[699].double())


@pytest.mark.parametrize("EA,EB", SHAPES)
def test_right_model_passes_every_bound(EA, EB):
    """Part B without a GPU: fp32 matmul with RNE passes checks 1 to 4 through the probes; its accumulation uses a small part of the
    bounds' accumulation term, and few of its hidden units differ from RNE of the float64 value."""
    failed, checks, share = _failed(EA, EB, None)
    assert not failed, checks
    assert share < 1e-3, share


@pytest.mark.parametrize("E", [64, 128])
def test_right_model_one_hidden_layer_against_the_oracle(E):
    from oracle import ncf_oracle as O
    x, ws, bs, state, ia, ib = _random_rows(E, E, [256])
    checks, _, repeat_equal = R.contract_checks(Model(x), x, ws, bs, oracle=O.basic_ncf_forward_indexed_bf16(state, ia, ib)[:, 0])
    assert repeat_equal and all(c.ok for c in checks), checks
    assert torch.equal(R.contract64(x, ws, bs)[0].float(), O.basic_ncf_forward_indexed_bf16(state, ia, ib)[:, 0])


@pytest.mark.parametrize("fault", sorted(WRONG))
@pytest.mark.parametrize("EA,EB", SHAPES)
def test_wrong_models_are_rejected(EA, EB, fault):
    failed, checks, _ = _failed(EA, EB, fault)
    assert WRONG[fault] <= failed, (fault, failed, checks)


def test_probes_read_the_models_own_values():
    """The probe weights return exactly what the model holds: h1 and H2 of the right model, read through 256 + 128 scorings, equal the
    same values computed directly."""
    x, ws, bs, _, _, _ = _random_rows(64, 64, [256, 128])
    m = Model(x)
    h1 = torch.relu(x.float() @ ws[0].to(torch.bfloat16).float().t() + bs[0]).to(torch.bfloat16).float()
    h2 = torch.relu(h1 @ ws[1].to(torch.bfloat16).float().t() + bs[1])
    assert torch.equal(R.read_h1(m, ws, bs), h1) and torch.equal(R.read_h2(m, ws, bs), h2)
