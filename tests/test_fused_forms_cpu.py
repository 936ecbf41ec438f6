"""CPU tests of the fp32 scorer family's restatements (tests/fused_forms_ref.py) and of its root reference, the extended
kernel-order C oracle (oracle/ncf_oracle_c.c): the launch plan at the values mlp_fused.hip's rule turns on, the packed-blob
layout, the prefetch-ring split list, and the oracle itself against float64 — within the suite's 1e-5 bar on random data for all
11 instances, exactly on integer data (with the 2^24 condition asserted on the data), and folded == fused there.  What the GPU
tests (tests/test_gpu_fused_forms.py) then require of the kernels is the oracle's bits, so everything the oracle adds to the
plain chain (range rule, identity ids, EB = 0, NULL biases) is checked here against float64 as well."""
import numpy as np
import pytest
import torch

import fused_forms_ref as R
from oracle import c_oracle
from test_gpu_basic import assert_close


# ------------------------------------------------------------------------------------------------ the launch plan
def test_plan_table_at_256_cus():
    cus, T = 256, 32
    assert R.fused_plan(1, cus, True) == [("small", 1)]
    assert R.fused_plan(767 * T, cus, True) == [("small", 767 * T)]
    assert R.fused_plan(767 * T, cus, False) == [("small", 767 * T)]
    for tiles in (768, 800, 870):                                   # full = 0: the whole batch is the ragged rest
        assert R.fused_plan(tiles * T, cus, True) == [("small", tiles * T)]
        assert R.fused_plan(tiles * T - 31, cus, True) == [("small", tiles * T - 31)]
    for tiles in (871, 1000, 1024):
        assert R.fused_plan(tiles * T, cus, True) == [("main", tiles * T)]
    assert R.fused_plan(1024 * T + 1, cus, True) == [("main", 1024 * T), ("small", 1)]
    assert R.fused_plan(1025 * T, cus, True) == [("main", 1024 * T), ("small", T)]
    assert R.fused_plan((1024 + 870) * T, cus, True) == [("main", 1024 * T), ("small", 870 * T)]
    assert R.fused_plan((1024 + 871) * T, cus, True) == [("main", (1024 + 871) * T)]
    assert R.fused_plan(2048 * T, cus, True) == [("main", 2048 * T)]
    for tiles in (768, 769, 870, 871, 1025, 1024 + 870):            # identity ids: no split, main from 768 tiles on
        assert R.fused_plan(tiles * T, cus, False) == [("main", tiles * T)]


@pytest.mark.parametrize("cus", [256, 304, 64, 120])
def test_boundaries_follow_the_cu_count(cus):
    b = R.boundaries(cus)
    rnd = 4 * cus
    assert b["round"] == rnd and b["rem_main"] == b["rem_small"] + 1
    assert b["rem_small"] * 1000 < rnd * R.PERMILLE <= b["rem_main"] * 1000
    if cus == 256:
        assert (b["rem_small"], b["rem_main"], b["main_min"]) == (870, 871, 871)
    assert R.fused_plan(32 * b["main_min"], cus, True) == [("main", 32 * b["main_min"])]
    assert R.fused_plan(32 * (b["main_min"] - 1), cus, True)[-1][0] == "small"
    assert b["main_min"] >= R.SMALL_TILES
    if rnd >= R.SMALL_TILES:                                         # one round + one pair: a one-pair tail
        assert R.fused_plan(32 * rnd + 1, cus, True) == [("main", 32 * rnd), ("small", 1)]


# ------------------------------------------------------------------------------------------------ the blob
@pytest.mark.parametrize("inst", [(64, 128, 64), (128, 256, 128), (256, 128, 0)])
def test_blob_restatement(inst):
    dims = R.dims_of(inst)
    g = torch.Generator().manual_seed(sum(inst))
    ws, bs = R.random_mlp(g, dims)
    L = R.blob_layout(dims)
    K0, N1, N2 = inst
    want = N1 * K0 + N1 + (N2 * N1 + N2 if N2 else 0) + (N2 or N1) + 4
    assert L["total"] == want and L["total"] % 4 == 0
    blob = R.pack_blob([w.numpy() for w in ws], [b.numpy() for b in bs])
    assert blob.shape == (want,)
    # the formula, element by element, on a sample of (q, nt, lane, j)
    W = ws[0].numpy()
    rng = np.random.default_rng(0)
    for _ in range(200):
        q, nt, lane, j = rng.integers(K0 // 8), rng.integers(N1 // 32), rng.integers(64), rng.integers(4)
        assert blob[L["wp1"] + ((q * (N1 // 32) + nt) * 64 + lane) * 4 + j] == W[32 * nt + (lane & 31), 8 * q + 4 * (lane >> 5) + j]
    assert np.array_equal(blob[L["b1"]:L["b1"] + N1], bs[0].numpy())
    assert np.array_equal(blob[L["wl"]:L["wl"] + (N2 or N1)], ws[-1].numpy().reshape(-1))
    assert blob[L["bl"]] == bs[-1].numpy()[0] and not blob[L["bl"] + 1:].any()
    # packing is a permutation of the weights
    assert np.array_equal(np.sort(blob[L["wp1"]:L["wp1"] + N1 * K0]), np.sort(W.reshape(-1)))
    zero = R.pack_blob([w.numpy() for w in ws], None)
    assert not zero[L["b1"]:L["b1"] + N1].any() and zero[L["bl"]] == 0


# ------------------------------------------------------------------------------------------------ the split list
@pytest.mark.parametrize("K0", [64, 128, 256])
def test_split_list_meets_the_ring_at_every_position(K0):
    eas = R.split_list(K0)
    Q1 = K0 // 8
    assert all(ea % 8 == 0 and 0 < ea <= K0 for ea in eas)
    qa = {ea // 8 for ea in eas}
    assert {1, 2, 3} <= qa and any(q >= R.XD for q in qa)
    assert {0, 1, 2, 3} <= {Q1 - q for q in qa}
    assert K0 // 2 in eas
    if K0 == 64:
        assert eas == [8, 16, 24, 32, 40, 48, 56, 64]
    else:
        assert eas == sorted({8, 16, 24, K0 // 2, K0 - 24, K0 - 16, K0 - 8, K0})


# ------------------------------------------------------------------------------------------------ the one comparison
def test_same_bits_helper_rejects_an_ulp_a_zero_sign_and_a_moved_nan():
    a = torch.tensor([1.0, -0.0, float("nan"), float("inf"), 3.5])
    payload = a.clone()
    payload.view(torch.int32)[2] = 0x7FC00123                      # another NaN payload at the same position: accepted
    R.assert_same_bits(payload, a)
    for i, v in [(0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))), (1, 0.0), (2, 0.0), (3, float("nan")), (4, -3.5)]:
        b = a.clone()
        b[i] = v
        with pytest.raises(AssertionError):
            R.assert_same_bits(b, a)


# ------------------------------------------------------------------------------------------------ the oracle
def _random_case(inst, EA=None, B=257, seed=0):
    K0 = inst[0]
    EA = K0 // 2 if EA is None else EA
    g = torch.Generator().manual_seed(1000 * seed + sum(inst) + EA)
    ta = torch.randn(90, EA, generator=g) * 0.5
    tb = torch.randn(40, K0 - EA, generator=g) * 0.5 if EA < K0 else None
    ws, bs = R.random_mlp(g, R.dims_of(inst))
    ia = torch.randint(0, 90, (B,), generator=g)
    ib = torch.randint(0, 40, (B,), generator=g)
    return g, ta, tb, ia, ib, ws, bs


@pytest.mark.parametrize("inst", R.INSTANCES)
def test_oracle_within_the_bar_of_float64_on_random_data(inst):
    g, ta, tb, ia, ib, ws, bs = _random_case(inst)
    out, oob = c_oracle.score_fused_f32_ex(ta, tb, ia, ib, ws, bs)
    assert not oob
    assert_close(out, R.score_f64(ta, tb, ia, ib, ws, bs))
    assert torch.equal(out, c_oracle.score_fused_f32(ta, tb, ia, ib, ws, bs))      # the entry the existing tests call
    # out-of-range ids on both sides: zero rows in float64, and the flag
    ia[3], ia[200], ib[7], ib[200], ia[-1] = -1, 90, 40 + 5, -(2 ** 40), 95
    out, oob = c_oracle.score_fused_f32_ex(ta, tb, ia, ib, ws, bs)
    assert oob
    assert_close(out, R.score_f64(ta, tb, ia, ib, ws, bs))


@pytest.mark.parametrize("inst", R.INSTANCES)
def test_oracle_is_exact_on_integer_data_and_folded_equals_fused(inst):
    K0, N1, N2 = inst
    g = torch.Generator().manual_seed(sum(inst))
    B = 300
    for EA in (K0 // 2, 8, K0 - 8):
        ta, tb, ws, bs = R.int_case(g, EA, K0 - EA, [N1] + ([N2] if N2 else []), 70, 50)
        ia = torch.randint(-3, 75, (B,), generator=g)                # some out of range on both sides
        ib = torch.randint(-3, 55, (B,), generator=g)
        assert R.int_margin(ta, tb, ia, ib, ws, bs) < 2 ** 24       # THE INTEGER CONDITION, on this data
        ref = R.score_f64(ta, tb, ia, ib, ws, bs)
        assert float(ref.abs().max()) < 2 ** 24
        out, oob = c_oracle.score_fused_f32_ex(ta, tb, ia, ib, ws, bs)
        assert oob
        assert torch.equal(out.double(), ref)
        if (N1, N2) in R.FOLDED_INSTANCES:
            # in-range ids: the two forms agree bit for bit (an out-of-range A id drops b1 in the folded form only, below)
            ia, ib = ia.clamp(0, 69), ib.clamp(0, 49)
            PA, PB = R.fold_tables(ta, tb, ws[0], bs[0])
            fo, oob = c_oracle.score_folded_f32(PA, PB, ia, ib, ws[1:], bs[1:])
            fu, _ = c_oracle.score_fused_f32_ex(ta, tb, ia, ib, ws, bs)
            assert not oob
            R.assert_same_bits(fo, fu, "folded oracle vs fused oracle")
            assert torch.equal(fo.double(), R.score_f64(ta, tb, ia, ib, ws, bs))


@pytest.mark.parametrize("nm", R.FOLDED_INSTANCES)
def test_folded_oracle_within_the_bar_and_drops_b1_with_an_out_of_range_a_id(nm):
    """Random P tables against float64 relu(PA[ia] z + PB[ib] z) -> tail, and the rule the GPU tests pin: b1 lives in PA, so an
    out-of-range A id leaves relu(PB[ib]) — the fused form keeps b1 there."""
    N1, N2 = nm
    g = torch.Generator().manual_seed(N1 + N2)
    PA, PB = torch.randn(60, N1, generator=g), torch.randn(30, N1, generator=g)
    ws, bs = R.random_mlp(g, [N1, N2, 1])
    ia, ib = torch.randint(0, 60, (200,), generator=g), torch.randint(0, 30, (200,), generator=g)
    ia[5], ib[9], ia[199], ib[199] = 60, -1, -(2 ** 40), 35

    def f64(ia, ib):
        h = torch.relu(R._gather64(PA, ia, 200) + R._gather64(PB, ib, 200))
        return torch.relu(h @ ws[0].double().t() + bs[0].double()) @ ws[1].double().t() + bs[1].double()

    out, oob = c_oracle.score_folded_f32(PA, PB, ia, ib, ws, bs)
    assert oob
    assert_close(out, f64(ia, ib))
    zero_a = torch.cat((torch.zeros(1, N1), PA[1:]))                 # an out-of-range A id == a PA row of zeros (b1 gone with it)
    out0, oob0 = c_oracle.score_folded_f32(zero_a, PB, torch.zeros(1, dtype=torch.long), ib[5:6], ws, bs)
    assert not oob0 and torch.equal(out0, out[5:6])


def test_oracle_forms_agree_with_each_other():
    """Identity ids == arange ids; EB = 0 == the same table split in two; a None bias == a bias of zeros; and the range rule is a
    real multiply: inf * 0 and nan * 0 reach layer 1 as NaN (the ReLU then reads it as 0), -x * 0 as -0.0."""
    inst = (64, 128, 64)
    g, ta, tb, ia, ib, ws, bs = _random_case(inst, B=90)
    ar = torch.arange(40)
    a, _ = c_oracle.score_fused_f32_ex(ta, tb, None, None, ws, bs, B=40)
    b, _ = c_oracle.score_fused_f32_ex(ta, tb, ar, ar, ws, bs)
    assert torch.equal(a, b)
    a, oob = c_oracle.score_fused_f32_ex(ta, tb, None, None, ws, bs, B=45)      # pairs 40 .. 44 run past table B
    assert oob and torch.equal(a[:40], b)
    wide = torch.cat((ta[:40], tb), 1)
    one, _ = c_oracle.score_fused_f32_ex(wide, None, ar, None, ws, bs)
    assert torch.equal(one, b)
    zb = [None, torch.zeros(64), None]
    a, _ = c_oracle.score_fused_f32_ex(ta, tb, ia, ib, ws, zb)
    b, _ = c_oracle.score_fused_f32_ex(ta, tb, ia, ib, ws, [torch.zeros(128), None, torch.zeros(1)])
    assert torch.equal(a, b)
    # P of the partial kernel: the chain cut after table A; its last row is row 0 times 0
    P = c_oracle.layer1_partial_f32(ta, ws[0], bs[0])
    assert P.shape == (91, 128)
    assert torch.equal(P[90], bs[0])                                  # finite row 0: +-0 products leave b1 (no -0.0 in b1)
    ta2 = ta.clone()
    ta2[0, 0], ta2[0, 1] = float("inf"), float("nan")
    P2 = c_oracle.layer1_partial_f32(ta2, ws[0], bs[0])
    assert torch.isnan(P2[90]).all() and torch.isnan(P2[0]).all() and torch.equal(P2[1:90], P[1:90])
    # ... and after the ReLU a NaN accumulator is 0: the score of an out-of-range pair over a non-finite row 0 is finite
    bad = torch.full((4,), 90, dtype=torch.long)
    s, oob = c_oracle.score_fused_f32_ex(ta2, tb, bad, ib[:4], ws, bs)
    assert oob and torch.isfinite(s).all()
