"""CPU tests of the references in tests/prep_forms_ref.py: the dense matrix -> shared-row CSR definition, the L2 norm's bar and the
exchange's definitions.  Each reference accepts a right model of its kernel and rejects the wrong ones a subtly broken kernel
would give; that is what shows the GPU tests (test_gpu_dense_csr_forms.py, test_gpu_l2_normalize_forms.py,
test_gpu_exchange_forms.py) fail for such a kernel."""
import numpy as np
import pytest
import torch

import prep_forms_ref as R


# ------------------------------------------------------------------------------------------------ dense -> CSR
def _csr_model(um, share, wrong=None):
    """A model of the conversion that groups rows by the bits of their listed entries (what the kernels' hash does), independent
    of the reference's canonical-form route.  ``wrong``: "second" shares with the second-smallest index, "neg_zero" lists -0,
    "denormal" drops denormals, "nan_share" lets bitwise-identical NaN rows share."""
    um = um.contiguous()
    B, I = um.shape
    v, raw = um.numpy(), um.view(torch.int32).numpy() if I else np.zeros((B, 0), np.int32)
    entries = []
    for b in range(B):
        if wrong == "neg_zero":
            nz = raw[b] != 0
        elif wrong == "denormal":
            nz = np.abs(v[b]) >= np.finfo(np.float32).tiny
            nz |= np.isnan(v[b])
        else:
            nz = v[b] != 0
        entries.append([(int(c), int(raw[b, c])) for c in np.nonzero(nz)[0]])
    pair_row = list(range(B))
    if share:
        groups = {}
        for b in range(B):
            if np.isnan(v[b]).any() and wrong != "nan_share":
                continue
            members = groups.setdefault(tuple(entries[b]), [])
            members.append(b)
            pair_row[b] = members[1] if wrong == "second" and len(members) > 2 else members[0]
    col, val, rowptr = [], [], [0]
    for b in range(B):
        if pair_row[b] == b:
            col += [c for c, _ in entries[b]]
            val += [x for _, x in entries[b]]
        rowptr.append(len(col))
    return (torch.tensor(rowptr, dtype=torch.int64), torch.tensor(col, dtype=torch.int32), torch.tensor(val, dtype=torch.int32),
            torch.tensor(pair_row, dtype=torch.int64))


@pytest.mark.parametrize("B,I", [(1, 1), (5, 1), (30, 7), (64, 65), (90, 257), (70, 513), (64, 1025)])
def test_dense_reference_is_the_definition(B, I):
    """The reference's canonical-form grouping equals the quadratic definition and an independent model, with and without
    sharing."""
    _, um = R.dense_case(B, I, "repeated", seed=1)
    for share in (True, False):
        ref = R.dense_csr_reference(um, share)
        assert R.dense_csr_mismatch(_csr_model(um, share), ref) is None
        assert torch.equal(ref[3], R.dense_pair_row_by_definition(um) if share else torch.arange(B))
    rowptr, col, val, pair = R.dense_csr_reference(um, True)
    assert int(rowptr[-1]) == col.numel() == val.numel() and bool((rowptr[1:] >= rowptr[:-1]).all())
    assert not bool((val == 0).any()) and not bool((val == -2 ** 31).any())                # neither +0 nor -0 is listed
    assert not bool((um == R.DENSE_SENTINEL).any())                                       # the slice under test holds no sentinel


def test_dense_planted_rows_share_as_described():
    I, B = 800, 64
    _, um = R.dense_case(B, I, "repeated", seed=2)
    at = R.dense_planted_map(B, I)
    assert {"win512", "win768"} <= set(at) and len(set(at.values())) == len(at) <= B // 2
    assert R.dense_planted_map(5, I) == {"t": 0, "nan0": 1, "nan1": 2, "t_again": 3, "nan2": 4}     # a small batch takes the first rows
    rowptr, col, val, pair = R.dense_csr_reference(um, True)
    p = lambda name: int(pair[at[name]])
    for name in ("nan0", "nan1", "nan2"):                                                  # identical NaN rows: each represents itself
        assert p(name) == at[name]
        lo, hi = int(rowptr[at[name]]), int(rowptr[at[name] + 1])
        assert bool(torch.isnan(val[lo:hi].view(torch.float32)).any())                     # and lists its NaN
    assert p("t_again") == at["t"] and p("t_last") == at["t"]                              # the NaN rows' non-NaN twin still shares
    for name in ("col0", "last", "win512", "win768", "pos_denormal"):
        assert p(name) == at[name] and p(name + "_again") == at[name]                      # differs from t in one column only; its twin shares
    assert p("pos_zero") == at["pos_zero"] and p("neg_zero") == at["pos_zero"]             # -0 == +0
    for name in ("neg_denormal", "pos_inf", "neg_inf", "one_ulp", "permuted"):
        assert p(name) == at[name]
    b = at["pos_denormal"]
    assert int(torch.tensor(R.DENORMAL).view(torch.int32)) in val[int(rowptr[b]):int(rowptr[b + 1])].tolist()
    assert R.DENORMAL != 0 and float(torch.tensor(R.DENORMAL)) < float(np.finfo(np.float32).tiny)


@pytest.mark.parametrize("wrong,part", [("second", "pair_row"), ("neg_zero", "rowptr"), ("denormal", "rowptr"), ("nan_share", "rowptr")])
def test_dense_reference_rejects_wrong_conversions(wrong, part):
    _, um = R.dense_case(64, 300, "repeated", seed=3)
    ref = R.dense_csr_reference(um, True)
    assert R.dense_csr_mismatch(_csr_model(um, True), ref) is None
    assert R.dense_csr_mismatch(_csr_model(um, True, wrong), ref) == part


def test_dense_mismatch_sees_every_part_and_ignores_the_tail():
    _, um = R.dense_case(40, 70, "repeated", seed=4)
    ref = R.dense_csr_reference(um, True)
    rowptr, col, val, pair = (t.clone() for t in ref)
    longer = (rowptr, torch.cat([col, torch.full((9,), -5, dtype=torch.int32)]), torch.cat([val, torch.full((9,), -5, dtype=torch.int32)]), pair)
    assert R.dense_csr_mismatch(longer, ref) is None
    for k, name in enumerate(("rowptr", "col", "val", "pair_row")):
        bad = [t.clone() for t in ref]
        bad[k][bad[k].numel() // 2] += 1
        assert R.dense_csr_mismatch(tuple(bad), ref) == name
    # one ulp in a value is a different bit pattern, and a float view of val is compared by bits (a NaN equals itself)
    as_float = (rowptr, col, val.view(torch.float32), pair)
    assert R.dense_csr_mismatch(as_float, ref) is None


def test_dense_empty_shapes():
    for B, I in ((0, 5), (4, 0), (0, 0)):
        _, um = R.dense_case(B, I)
        for share in (True, False):
            rowptr, col, val, pair = R.dense_csr_reference(um, share)
            assert rowptr.tolist() == [0] * (B + 1) and col.numel() == 0 and val.numel() == 0
            assert pair.tolist() == ([0] * B if share else list(range(B)))                 # rows without columns are all equal


# ------------------------------------------------------------------------------------------------ L2 normalisation
L2_E = (1, 15, 16, 17, 64, 100, 257, 2094)


def test_l2_clamp_is_the_fp32_constant():
    assert R.L2_CLAMP == float(np.float32(1e-12)) and R.L2_CLAMP != 1e-12
    assert R.l2_bar(1) == 9 * 2.0 ** -24 and R.l2_bar(16) == 9 * 2.0 ** -24 and R.l2_bar(17) == 10 * 2.0 ** -24
    assert R.l2_bar(2094) == (131 + 8) * 2.0 ** -24


@pytest.mark.parametrize("E", L2_E)
def test_l2_reference_rows_and_kernel_order_stay_inside_the_bar(E):
    x = R.l2_case(40, E, seed=5)
    ref = R.l2_reference(x)
    kind = torch.arange(40) % 8
    assert bool((ref[kind == 3] == 0).all())                                               # zeros stay zeros
    single = ref[kind == 4]
    assert bool(((single == 0) | (single.abs() == 1)).all()) and bool((single.abs().sum(1) == 1).all())    # +-1 exactly
    tiny = kind == 5
    assert torch.equal(ref[tiny], x[tiny].double() / R.L2_CLAMP) and bool((x[tiny].double().norm(dim=1) < 1e-12).all())
    assert bool(torch.isnan(ref[kind == 6]).all())                                         # a NaN row is all NaN
    inf_rows, inf_x = ref[kind == 7], x[kind == 7]
    assert torch.equal(torch.isnan(inf_rows), torch.isinf(inf_x)) and bool((inf_rows[~torch.isinf(inf_x)] == 0).all())
    for k in (0, 1, 2):                                                                    # random rows have unit norm
        assert bool(((ref[kind == k].norm(dim=1) - 1).abs() < 1e-12).all())
    ratio = R.l2_ratio(R.l2_kernel_order_model(x), ref, E)
    assert ratio <= 0.5, ratio                                                             # first-order bound: half the bar (the bar doubles it)


def test_l2_bar_rejects_wrong_kernels():
    """On the random rows: one of the 16 sub-lanes dropped from the sum, a clamp of 1e-6, a division by the squared norm."""
    worst = {"lane": 0.0, "clamp": 0.0, "squared": 0.0}
    for E in L2_E:
        x = R.l2_case(64, E, seed=6)
        rnd = torch.arange(64) % 8 < 3
        x, ref = x[rnd], R.l2_reference(x[rnd])
        assert R.l2_ratio(R.l2_kernel_order_model(x), ref, E) <= 0.5
        lane = R.l2_ratio(R.l2_kernel_order_model(x, drop_lane=min(5, E - 1)), ref, E)
        assert lane > 1, (E, lane)                                                         # at every E
        squared = R.l2_ratio(R.l2_kernel_order_model(x, squared=True), ref, E)
        assert squared > 1, (E, squared)
        worst["clamp"] = max(worst["clamp"], R.l2_ratio(R.l2_kernel_order_model(x, clamp=1e-6), ref, E))
    assert worst["clamp"] > 1          # the scale-1e-6 rows of E = 1 have norms below 1e-6


def test_l2_ratio_asserts_nan_positions_and_exact_zeros():
    x = R.l2_case(16, 17, seed=7)
    ref = R.l2_reference(x)
    good = R.l2_kernel_order_model(x)
    assert R.l2_ratio(good, ref, 17) <= 0.5
    with pytest.raises(AssertionError, match="NaN"):                                       # fmaxf(NaN, 1e-12) = 1e-12: finite outputs in a NaN row
        R.l2_ratio(torch.where(torch.isnan(good) & ~torch.isnan(x), x / 1e-12, good), ref, 17)
    bad = good.clone()
    bad[3, 0] = 1e-30
    with pytest.raises(AssertionError, match="zero"):
        R.l2_ratio(bad, ref, 17)


# ------------------------------------------------------------------------------------------------ exchange
def _ids(B, total, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, total, (B,), generator=g)
    idx[B // 2:] = idx[:B - B // 2]                                                        # repeats
    idx[1], idx[2], idx[3], idx[4], idx[5] = total - 1, total, -1, 1 << 40, -(1 << 40)
    return idx


@pytest.mark.parametrize("world,cap", [(1, 70), (3, 9), (7, 64), (257, 3)])
def test_exchange_models_satisfy_their_definitions(world, cap):
    rpr = 13
    total = rpr * (world - 1) + 6                                                          # a short last rank: `total` has an owner below world
    idx = _ids(60, total, world)
    send, slot, counts, oob, overflow = R.bucket_ids_model(idx, rpr, total, world, cap)
    kept = R.check_bucket_ids(idx, rpr, total, world, cap, send, slot, counts, overflow)
    assert oob == 1 and bool(kept[1]) and not bool(kept[2:6].any()) and total // rpr < world
    send, slot, counts, oob, overflow = R.bucket_ids_model(idx, rpr, total, world, cap, dedup=True)
    kept = R.check_bucket_ids_dedup(idx, rpr, total, world, cap, send, slot, counts, overflow)
    assert oob == 1 and bool(kept[1]) and not bool(kept[2:6].any())


def test_exchange_reference_rejects_wrong_bucketing():
    world, cap, rpr = 3, 6, 13
    total = rpr * world - 7
    idx = _ids(60, total, 11)
    for dedup, check in ((False, R.check_bucket_ids), (True, R.check_bucket_ids_dedup)):
        send, slot, counts, oob, overflow = R.bucket_ids_model(idx, rpr, total, world, cap, dedup=dedup)
        assert overflow == 1 and int(counts.max()) > cap                                   # some bucket is over its capacity
        check(idx, rpr, total, world, cap, send, slot, counts, overflow)
        # a slot that names another id's bucket entry (same owner, another local row)
        kept = (slot >= 0).nonzero().view(-1)
        p = int(kept[0])
        other = [int(q) for q in kept if int(slot[q]) // cap == int(slot[p]) // cap and int(idx[q]) != int(idx[p])][0]
        bad = slot.clone()
        bad[p] = slot[other]
        with pytest.raises(AssertionError):
            check(idx, rpr, total, world, cap, send, bad, counts, overflow)
        # a dropped pair that got a slot, and a missing overflow flag
        bad = slot.clone()
        bad[2] = 0
        with pytest.raises(AssertionError):
            check(idx, rpr, total, world, cap, send, bad, counts, overflow)
        with pytest.raises(AssertionError):
            check(idx, rpr, total, world, cap, send, slot, counts, 0)
    # a header of `counts` in place of min(counts, cap)
    send, slot, counts, oob, overflow = R.bucket_ids_model(idx, rpr, total, world, cap, dedup=True)
    bad = send.clone()
    bad.view(world, cap + 1)[:, 0] = counts.long()
    with pytest.raises(AssertionError):
        R.check_bucket_ids_dedup(idx, rpr, total, world, cap, bad, slot, counts, overflow)
    # a pair of a kept id that was dropped on its own
    p = int((slot >= 0).nonzero()[0])
    twin = [q for q in range(60) if q != p and int(idx[q]) == int(idx[p])]
    assert twin
    bad = slot.clone()
    bad[twin[0]] = -1
    with pytest.raises(AssertionError):
        R.check_bucket_ids_dedup(idx, rpr, total, world, cap, send, bad, counts, overflow)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gather_buckets_reference(dtype):
    g = torch.Generator().manual_seed(3)
    world, cap, rows, E = 4, 5, 11, 8
    tab = R.bit_table(rows, E + 8, dtype, g)[:, 8:]                                        # a column slice
    recv = torch.full((world, cap + 1), -9, dtype=torch.int64)
    recv[:, 0] = torch.tensor([0, cap, 2, 3])
    recv[1, 1:] = torch.tensor([3, 10, 0, 3, 7])
    recv[2, 1:3] = torch.tensor([5, 5])
    recv[2, 3:] = torch.tensor([-1, rows, 1 << 40])                                        # bad ids in the padding: ignored, no flag
    recv[3, 1:4] = torch.tensor([1, 2, 9])
    before = R.bit_table(world * cap + 2, E, dtype, g)
    exp, flag = R.gather_buckets_expected(tab, recv.view(-1), world, cap, before)
    assert not flag
    want = before.clone()
    for r, ids in ((1, [3, 10, 0, 3, 7]), (2, [5, 5]), (3, [1, 2, 9])):
        for k, i in enumerate(ids):
            want[r * cap + k] = tab[i]
    assert torch.equal(R.bits(exp), R.bits(want))
    # a padding row that was written is seen, bit for bit
    wrong = want.clone()
    wrong[2 * cap + 3] = tab[0]
    assert not torch.equal(R.bits(exp), R.bits(wrong))
    wrong = want.clone()
    wrong[world * cap] = tab[0]                                                            # a row past world * cap
    assert not torch.equal(R.bits(exp), R.bits(wrong))
    # bad ids inside the filled prefix: zero rows and the flag
    for badid in (-1, rows, 1 << 40):
        rc = recv.clone()
        rc[3, 2] = badid
        exp, flag = R.gather_buckets_expected(tab, rc.view(-1), world, cap, before)
        assert flag
        z = want.clone()
        z[3 * cap + 1] = 0
        assert torch.equal(R.bits(exp), R.bits(z))
    assert [R.gather_lanes_per_row(c) for c in (1, 3, 4, 7, 8, 15, 16, 33)] == [1, 1, 4, 4, 8, 8, 16, 16]
    assert all(R.gather_lanes_per_row(c) == l for l, cs in R.GATHER_CHUNKS.items() for c in cs)
