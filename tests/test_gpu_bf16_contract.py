"""The bf16 scoring kernels (slab-streaming, 4-wave and 8-wave weight-stationary) held to their arithmetic contract, stated in float64 in
tests/bf16_contract_ref.py: operands RNE-rounded to bf16, fp32 accumulate, the first of two hidden layers re-rounded RNE to bf16, biases /
second hidden layer / 1-wide layer / output in fp32.

Part A (test_exact_*): integer-valued inputs for which every fp32 partial sum is exact in any order, so the float64 evaluation of the
contract is THE answer and torch.equal the assertion, with dense layer-1 weights and hidden pre-activations that need rounding, ties
included.  What the construction guarantees is asserted on the inputs before the GPU is looked at (bf16_contract_ref.exact_conditions).

Part B (test_random_*): random operands, one layer at a time.  The kernels' intermediate values are read out through the public entry
point with probe weights (a 0/1 selection matrix as W2 and a one-hot last layer return the rounded h1; the real W2 and a one-hot last
layer return the fp32 H2), and each layer is compared per element with its float64 value at a bound derived from the formats alone:
half a bf16 ulp for the re-rounding plus (terms + 1) * 2^-23 * sum|terms| for an fp32 accumulation in any order, with either rounding of
the accumulator.  Stages after the first take the kernel's OWN observed input (an input of that stage, not a bar).  No bound here comes
from what a kernel gives.  tests/test_bf16_contract_cpu.py shows on CPU models that these checks reject truncation, round-half-up, ReLU
before the bias, a bf16 second hidden layer, bf16 last-layer weights and two hidden units in each other's pack slots.

The layer-1 bound, ulp_bf16(relu(a)) / 2 + D with D = (K0 + 1) * 2^-23 * S1, is what RNE of an fp32-accumulated sum a' satisfies while
|a' - a| stays a small part of D (it cannot exceed D; a model that accumulates in fp32 uses under 2 % of it)."""
import functools

import pytest
import torch

import bf16_contract_ref as R
from conftest import record_error

pytestmark = pytest.mark.gpu

KERNELS = ["stream", "ws", "ws8"]
EXACT_SHAPES = [(64, 64, (256, 128)), (128, 128, (256, 128)), (64, 64, (256,)), (128, 128, (256,)), (192, 64, (256, 128))]
EXACT_BATCHES = [1, 63, 255, 256, 257, 3000, 40000, 100001, 140000]
AUTO_BATCHES = [3000, 140000]                  # one batch on each side of where the library's own dispatch changes kernels
RANDOM_SHAPES = [(64, 64, (256, 128)), (128, 128, (256, 128)), (192, 64, (256, 128))]
RANDOM_BATCHES = [4129, 40000]                 # below / above one tile per workgroup of the persistent kernels, ragged tails
N_CONDITION_PAIRS = 4096


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def _scorer(native, gpu, ta, ia, tb, ib):
    """score(ws, bs) of bf16_contract_ref on the GPU: packs the weights for the bf16 family and scores the fixed batch."""
    tag, tbg, iag, ibg = ta.to(torch.bfloat16).to(gpu), tb.to(torch.bfloat16).to(gpu), ia.to(gpu), ib.to(gpu)

    def score(ws, bs):
        packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs], dtype=torch.bfloat16)
        return native.score_fused(tag, iag, tbg, ibg, packed)[:, 0].cpu()

    return score


# ----------------------------------------------------------------------------------------------------------------- Part A
@functools.lru_cache(maxsize=None)
def _exact_case(EA, EB, hidden):
    """The integer case of one shape, with the conditions it has to meet asserted on a standing batch of 4096 pairs."""
    ta, tb, ws, bs = R.exact_case(EA, EB, hidden)
    ia, ib = R.batch_ids(N_CONDITION_PAIRS, (ta.shape[0], tb.shape[0]), seed=N_CONDITION_PAIRS)
    for name, holds, detail in R.exact_conditions(R.gather_rows(ta, ia, tb, ib), ws, bs):
        assert holds, (name, detail)
    return ta, tb, ws, bs


@functools.lru_cache(maxsize=None)
def _exact_batch(EA, EB, hidden, B, out_of_range=False):
    """ids and the float64 answer of one batch; exactness in any summation order is asserted on THIS batch's pairs."""
    ta, tb, ws, bs = _exact_case(EA, EB, hidden)
    ia, ib = R.batch_ids(B, (ta.shape[0], tb.shape[0]), seed=B)
    if out_of_range:
        ia[[2, B // 2, B - 1]] = torch.tensor([ta.shape[0], -1, 1 << 40])
        ib[[3, B // 2, B - 2]] = torch.tensor([tb.shape[0], -7, tb.shape[0] + 5])      # pair B // 2: both halves read as zeros
    x = R.gather_rows(ta, ia, tb, ib)
    worst = max(R.magnitudes64(x, ws, bs))
    assert worst < 2 ** 24, worst
    ref = R.contract64(x, ws, bs)[0]
    assert bool((ref == ref.float().double()).all())
    return ia, ib, ref


def _exact_params():
    for EA, EB, hidden in EXACT_SHAPES:
        for kernel in KERNELS + ["auto"]:
            for B in (AUTO_BATCHES if kernel == "auto" else EXACT_BATCHES):
                yield pytest.param(EA, EB, hidden, kernel, B, id=f"{EA}+{EB}-{'x'.join(map(str, hidden))}-{kernel}-{B}")


@pytest.mark.parametrize("EA,EB,hidden,kernel,B", list(_exact_params()))
def test_exact_integers_with_real_rounding(native, gpu, kernel_option, EA, EB, hidden, kernel, B):
    """Bit for bit against the float64 contract where layer 1 is dense and 16-22 % of its activations are inexact in bf16 (more than
    50 000 ties each way among 4096 pairs): replacing RNE by truncation or by round-half-up changes more than 99 % of these scores.
    Every batch of the ragged set through every kernel; ids cover row 0 and the last row of both tables."""
    ta, tb, ws, bs = _exact_case(EA, EB, hidden)
    ia, ib, ref = _exact_batch(EA, EB, hidden, B)
    kernel_option("bf16_kernel", kernel)
    out = _scorer(native, gpu, ta, ia, tb, ib)(ws, bs)
    native.check_oob(gpu)
    wrong = int((out.double() != ref).sum())
    record_error("exact", wrong, 1.0)              # a count, not an error: anything above 0 fails
    assert torch.equal(out.double(), ref), f"{wrong} of {B} scores differ, first at pair {int((out.double() != ref).nonzero()[0])}"


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("EA,EB,hidden", EXACT_SHAPES)
def test_exact_integers_out_of_range_ids(native, gpu, kernel_option, EA, EB, hidden, kernel):
    """A few out-of-range ids (too large by one, negative, huge; one pair with both): that table's half of the row reads as zeros, the
    score is still the exact float64 answer, and the sticky flag raises on check."""
    B = 3000
    ta, tb, ws, bs = _exact_case(EA, EB, hidden)
    ia, ib, ref = _exact_batch(EA, EB, hidden, B, out_of_range=True)
    kernel_option("bf16_kernel", kernel)
    out = _scorer(native, gpu, ta, ia, tb, ib)(ws, bs)
    assert torch.equal(out.double(), ref), f"{int((out.double() != ref).sum())} of {B} scores differ"
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.check_oob(gpu)


@pytest.mark.parametrize("hidden", [(256, 128), (256,)])
def test_ws8_option_on_other_shapes_is_the_4_wave_kernel(native, gpu, kernel_option, hidden):
    """(EA, EB) = (192, 64) is not the 8-wave kernel's shape, nor is a single hidden layer: the option then selects the 4-wave kernel."""
    for EA, EB in ((192, 64), (128, 128)) if hidden == (256,) else ((192, 64),):
        ta, tb, ws, bs = R.ncf_case(EA, EB, hidden)[:4]
        ia, ib = R.batch_ids(5000, (ta.shape[0], tb.shape[0]), seed=5)
        outs = {}
        for kernel in ("ws", "ws8", "auto"):
            kernel_option("bf16_kernel", kernel)
            outs[kernel] = _scorer(native, gpu, ta, ia, tb, ib)(ws, bs)
        assert torch.equal(outs["ws8"], outs["ws"]) and torch.equal(outs["auto"], outs["ws"])


# ----------------------------------------------------------------------------------------------------------------- Part B
def wide_case(EA, EB, hidden, rows=(3000, 700)):
    """Operands beside the freshly initialised model's (whose table entries are below 0.08, so that a third of its hidden units never
    fire): N(0, 0.5) tables, N(0, 1/K) weights, N(0, 0.1) biases as in test_score_fused_vs_oracle: every hidden unit alive on about half
    of the pairs, activations over many binades."""
    g = torch.Generator().manual_seed(EA + 7 * EB + len(hidden))
    dims = [EA + EB] + list(hidden) + [1]
    ta = (torch.randn(rows[0], EA, generator=g) * 0.5).to(torch.bfloat16)
    tb = (torch.randn(rows[1], EB, generator=g) * 0.5).to(torch.bfloat16)
    ws = [torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    bs = [torch.randn(dims[i + 1], generator=g) * 0.1 for i in range(len(dims) - 1)]
    return ta, tb, ws, bs, None


@functools.lru_cache(maxsize=None)
def _random_batch(operands, EA, EB, hidden, B):
    ta, tb, ws, bs, state = (R.ncf_case if operands == "ncf" else wide_case)(EA, EB, hidden)
    ia, ib = R.batch_ids(B, (ta.shape[0], tb.shape[0]), seed=B)
    x = R.gather_rows(ta, ia, tb, ib)
    if len(hidden) == 2:
        return ta, tb, ws, bs, ia, ib, x, None
    from oracle import ncf_oracle as O
    oracle = O.basic_ncf_forward_indexed_bf16(state, ia, ib)[:, 0] if state is not None else R.contract64(x, ws, bs)[0].float()
    return ta, tb, ws, bs, ia, ib, x, oracle


def _assert_checks(kernel, checks, share, repeat_equal):
    for c in checks:
        print(f"{kernel}: {c}; used {c.err / max(c.bar, 1e-300):.4f} of the bound")
        record_error(c.name, c.err, c.bar)
    if share is not None:
        print(f"{kernel}: share of hidden units whose h1 differs from RNE of the float64 value: {share:.3e}")
        record_error("h1 != RNE(float64), share of units (reported, no bar)", share, 1.0)
    assert repeat_equal, "a repeated launch gave other bits"
    assert all(c.ok for c in checks), [c for c in checks if not c.ok]


# on (192, 64) the 8-wave option is the 4-wave kernel (asserted above): it is not probed twice
LAYERED = [(k, EA, EB, h) for k in KERNELS for EA, EB, h in RANDOM_SHAPES if k != "ws8" or EA == EB]


@pytest.mark.parametrize("B", RANDOM_BATCHES)
@pytest.mark.parametrize("operands", ["ncf", "wide"])
@pytest.mark.parametrize("kernel,EA,EB,hidden", LAYERED)
def test_random_operands_layer_by_layer(native, gpu, kernel_option, kernel, operands, EA, EB, hidden, B):
    """Checks 1 to 4 of bf16_contract_ref on every hidden unit (256 + 128 probe launches: every accumulator register and pack slot is
    read), and the reported share 5."""
    ta, tb, ws, bs, ia, ib, x, _ = _random_batch(operands, EA, EB, hidden, B)
    kernel_option("bf16_kernel", kernel)
    checks, share, repeat_equal = R.contract_checks(_scorer(native, gpu, ta, ia, tb, ib), x, ws, bs)
    native.check_oob(gpu)
    _assert_checks(kernel, checks, share, repeat_equal)


@pytest.mark.parametrize("B", RANDOM_BATCHES)
@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("operands", ["ncf", "wide"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_random_operands_one_hidden_layer(native, gpu, kernel_option, kernel, operands, E, B):
    """Hidden [256]: nothing is re-rounded, so the score itself is held to the float64 oracle on the bf16 operands at the fp32 bar."""
    ta, tb, ws, bs, ia, ib, x, oracle = _random_batch(operands, E, E, (256,), B)
    kernel_option("bf16_kernel", kernel)
    checks, share, repeat_equal = R.contract_checks(_scorer(native, gpu, ta, ia, tb, ib), x, ws, bs, oracle=oracle)
    native.check_oob(gpu)
    _assert_checks(kernel, checks, share, repeat_equal)


@pytest.mark.parametrize("B", RANDOM_BATCHES)
@pytest.mark.parametrize("EA,EB,hidden", RANDOM_SHAPES)
def test_random_operands_auto_dispatch_is_one_of_the_kernels(native, gpu, kernel_option, EA, EB, hidden, B):
    """The library's own choice computes, bit for bit, what one of the three forced kernels computes (each of which is held to the bounds
    above): on the real weights, on a layer-1 probe and on a layer-2 probe."""
    ta, tb, ws, bs, ia, ib, _, _ = _random_batch("wide", EA, EB, hidden, B)
    score = _scorer(native, gpu, ta, ia, tb, ib)
    launches = [(ws, bs), R.layer1_probe(ws, bs, 1, 77)[:2], R.layer2_probe(ws, bs, 99)]
    outs = {}
    for kernel in KERNELS + ["auto"]:
        kernel_option("bf16_kernel", kernel)
        outs[kernel] = [score(w, b) for w, b in launches]
    assert any(all(torch.equal(a, f) for a, f in zip(outs["auto"], outs[k])) for k in KERNELS)
