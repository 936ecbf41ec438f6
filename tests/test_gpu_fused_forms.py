"""GPU tests (MI355X): the fp32 MLP scorers on every form they take, bit for bit against the kernel-order C oracle
(oracle/ncf_oracle_c.c, the root reference of the family; tests/test_fused_forms_cpu.py holds it to float64).  Every comparison
with a kernel is exact: NaN at the same positions, int32-view equality elsewhere (fused_forms_ref.assert_same_bits).  Every run
writes into a slice of a sentinel-filled buffer and checks the floats around it, and checks the sticky out-of-range flag: clear
when the oracle saw no bad id, raised exactly once (check_oob raises, then is clear) when it did.

WHICH BOUNDARY EACH BATCH SIZE STANDS ON.  All sizes derive from the device's CU count through fused_forms_ref.boundaries (the
restatement of launch_inst, mlp_fused.hip): round = 4 x CUs tiles of 32 pairs (1024 at 256 CUs), rem_small = the largest ragged
rest that goes to the small kernel (rem * 1000 < round * 850: 870), rem_main = rem_small + 1 (871), main_min = the smallest tile
count that runs whole on the main kernel with ids (871); NCF_SMALL_TILES = 768 does not depend on the device.

ncf_score_fused
* every instance / table splits / strided operands, "both kernels": B = 33 (small kernel, a second tile of one pair) and
  B = 32 main_min - 31 (main kernel with ids: a last tile of one pair, tiles % 4 = 3, so one dead wave in the last workgroup).
  The single-table splits (EA = K0, tabB and idxB None) also run B = 32 round + 1: a main head and a one-pair small tail whose
  idxB stays NULL.
* table splits: EA over fused_forms_ref.split_list(K0), the A -> B switch at every position of the XD = 4 row ring.
* small kernel with ids: B = 1, 31, 32, 33, 64 and 32 x 767 (the last size below NCF_SMALL_TILES).
* main kernel through identity ids (no split, main from 768 tiles on): tiles 767 (still small), 768, 769, 770, 771 (every
  tiles % 4, i.e. 0 .. 3 dead waves) x B % 32 in {0, 1, 31}; identity on A, on B, on both; tables of exactly B rows, and B - 7
  rows (the last 7 pairs run past the table: row 0 times 0, flag raised).
* ragged rounds: tiles = rem_small (small, full = 0), rem_main (main, full = 0), round + rem_small (main head + small tail),
  round + rem_main (main, whole), and B = 32 round + 1 (a one-pair tail); the same sizes with identity ids (no split) give the
  same bits as ids 0 .. B-1.
* out-of-range ids -1, rows, rows + 5, -2^40 on A, on B, on both: in the first tile, on both sides of the head / tail seam, in the
  partial last tile and at pair B - 1 (the clamped lanes past B repeat it), at B = 33, 32 main_min - 31 and 32 round + 33.

ncf_score_folded: one wave per 32-pair tile, four per workgroup: B = 1, 31, 32, 33 (tile edge), 127, 128, 129 (workgroup edge),
4097 (129 tiles, a last workgroup of one live wave).  THE FOLDED FORM'S OUT-OF-RANGE RULE differs from the fused form's: b1 is
folded into PA (PA = TA W1a^T + b1), so an out-of-range A id, which reads row 0 of PA times 0, drops b1 with the row — the pair
scores relu(PB[ib]) -> tail, where ncf_score_fused keeps b1.  An out-of-range B id keeps b1.  Both raise the sticky flag, which
is what tells the caller; the behaviour is pinned as it is.

ncf_layer1_partial / ncf_score_fused_partial: P's bits against the oracle's layer-1 chain cut after table A's k-groups (tables of
33 rows: P has 34, a second tile of two rows; and 900), and one strided run at R / 2 + 33 pairs (R = 32 round: the smallest batch
the partial kernel keeps, tests/test_gpu_partial_seam.py) compared with the oracle over the whole batch."""
import numpy as np
import pytest
import torch

import fused_forms_ref as R

pytestmark = pytest.mark.gpu

ROWS_A, ROWS_B = 900, 400
SENT = -7.5e33          # sentinel around every output
PAD = 8


def BAD_IDS(rows):
    return [-1, rows, rows + 5, -(2 ** 40)]


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


@pytest.fixture(scope="module")
def bounds(gpu):
    return R.boundaries(torch.cuda.get_device_properties(gpu).multi_processor_count)


@pytest.fixture(autouse=True)
def _clear_flag(native, gpu):
    native._oob_flag(gpu).zero_()
    yield


def _both_sizes(bounds):
    return [33, 32 * bounds["main_min"] - 31]


def _out(B, gpu):
    buf = torch.full((B + 2 * PAD,), SENT, device=gpu)
    return buf, buf[PAD:PAD + B].view(B, 1)


def _guards_intact(buf, B):
    edge = torch.cat((buf[:PAD], buf[PAD + B:])).cpu()
    assert bool((edge == SENT).all()), "a float outside out[0 .. B-1] was written"


def _flag(native, gpu, raised):
    if raised:
        with pytest.raises(IndexError):
            native.check_oob(gpu)
    native.check_oob(gpu)           # clear: not raised, or raised exactly once


def _strided(t, pad, gpu, fill=3.0e30):
    """``t`` (CPU) as a column slice of a wider device buffer: ld = cols + pad, base 16 bytes into the allocation."""
    rows, cols = t.shape
    flat = torch.full((rows * (cols + pad) + 4,), fill, device=gpu)
    v = flat[4:].view(rows, cols + pad)[:, :cols]
    v.copy_(t.to(gpu))
    assert v.stride(0) == cols + pad and v.data_ptr() % 16 == 0 and v.data_ptr() == flat.data_ptr() + 16
    return v


_cases = {}


def _case(native, gpu, inst, EA=None, rowsA=ROWS_A, rowsB=ROWS_B, nonfinite=False):
    """Tables (CPU and device), weights and the packed MLP of one instance and split, built once per module."""
    K0 = inst[0]
    EA = K0 // 2 if EA is None else EA
    key = (inst, EA, rowsA, rowsB, nonfinite)
    if key not in _cases:
        g = torch.Generator().manual_seed(sum(inst) * 131 + EA)
        ta = torch.randn(rowsA, EA, generator=g) * 0.5
        tb = torch.randn(rowsB, K0 - EA, generator=g) * 0.5 if EA < K0 else None
        ws, bs = R.random_mlp(g, R.dims_of(inst))
        if nonfinite:           # row 0 of A: inf and -inf; row 0 of B: NaN and inf; row 2 of A: one inf, read directly
            ta[0, 1], ta[0, 5], ta[2, 3] = float("inf"), -float("inf"), float("inf")
            if tb is not None:
                tb[0, 2], tb[0, 6] = float("nan"), float("inf")
        packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
        _cases[key] = dict(ta=ta, tb=tb, ws=ws, bs=bs, packed=packed, tag=ta.to(gpu), tbg=None if tb is None else tb.to(gpu))
    return _cases[key]


def _ids(B, rowsA, rowsB, seed, lo=0):
    """In-range ids; pair B - 1 reads the last row of both tables."""
    g = torch.Generator().manual_seed(seed)
    ia, ib = torch.randint(lo, rowsA, (B,), generator=g), torch.randint(lo, rowsB, (B,), generator=g)
    ia[-1], ib[-1] = rowsA - 1, rowsB - 1
    return ia, ib


def _run_fused(native, gpu, c, ia, ib, B=None, tag=None, tbg=None, rowsA=None, rowsB=None, expect_oob=None):
    """One ncf_score_fused launch set against the oracle: bits, guards, flag.  Returns the scores (CPU)."""
    from oracle import c_oracle
    ta = c["ta"] if rowsA is None else c["ta"][:rowsA]
    tb = c["tb"] if rowsB is None or c["tb"] is None else c["tb"][:rowsB]
    tag = (c["tag"] if rowsA is None else c["tag"][:rowsA]) if tag is None else tag
    tbg = (c["tbg"] if rowsB is None or c["tbg"] is None else c["tbg"][:rowsB]) if tbg is None else tbg
    if B is None:
        B = len(ia) if ia is not None else len(ib)
    buf, out = _out(B, gpu)
    native.score_fused(tag, None if ia is None else ia.to(gpu), tbg, None if ib is None else ib.to(gpu), c["packed"], out=out, B=B)
    ref, oob = c_oracle.score_fused_f32_ex(ta, tb, ia, ib, c["ws"], c["bs"], B=B)
    if expect_oob is not None:
        assert oob == expect_oob
    got = out.cpu()
    _guards_intact(buf, B)
    R.assert_same_bits(got, ref, f"score_fused B={B}")
    _flag(native, gpu, oob)
    return got


# ================================================================================================ ncf_score_fused
@pytest.mark.parametrize("inst", R.INSTANCES, ids=str)
def test_every_instance_on_both_kernels(native, gpu, bounds, inst):
    c = _case(native, gpu, inst)
    for B in _both_sizes(bounds):
        ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B)
        _run_fused(native, gpu, c, ia, ib, expect_oob=False)


SPLITS = [(inst, EA) for inst in [(64, 128, 64), (128, 256, 128), (256, 256, 0)] for EA in R.split_list(inst[0])]


@pytest.mark.parametrize("inst,EA", SPLITS, ids=lambda v: str(v))
def test_table_splits_meet_the_prefetch_ring_everywhere(native, gpu, bounds, inst, EA):
    c = _case(native, gpu, inst, EA)
    single = EA == inst[0]
    assert (c["tb"] is None) == single
    sizes = _both_sizes(bounds) + ([32 * bounds["round"] + 1] if single else [])
    for B in sizes:
        ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B + EA)
        _run_fused(native, gpu, c, ia, None if single else ib, expect_oob=False)
        if single and B == 33:      # an idxB given beside a NULL tabB is not read
            _run_fused(native, gpu, c, ia, ib, expect_oob=False)


@pytest.mark.parametrize("pad", [4, 12])
def test_strided_tables_and_guarded_out(native, gpu, bounds, pad):
    c = _case(native, gpu, R.HEADLINE)
    tag, tbg = _strided(c["ta"], pad, gpu), _strided(c["tb"], pad, gpu)
    for B in _both_sizes(bounds):
        ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B + pad)
        _run_fused(native, gpu, c, ia, ib, tag=tag, tbg=tbg, expect_oob=False)


@pytest.mark.parametrize("B", [1, 31, 32, 33, 64, 32 * (R.SMALL_TILES - 1)])
def test_batch_edges_of_the_small_kernel(native, gpu, bounds, B):
    assert R.fused_plan(B, bounds["round"] // 4, True) == [("small", B)]
    c = _case(native, gpu, R.HEADLINE)
    ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B)
    _run_fused(native, gpu, c, ia, ib, expect_oob=False)


IDENT_ROWS = 32 * (R.SMALL_TILES + 3)


@pytest.mark.parametrize("rem", [0, 1, 31])
@pytest.mark.parametrize("tiles", [R.SMALL_TILES - 1 + t for t in range(5)])
def test_batch_edges_of_the_main_kernel_through_identity_ids(native, gpu, bounds, tiles, rem):
    """Identity ids never split: 767 tiles run the small kernel, 768 .. 771 the main one, and both sides of the crossover give
    the oracle's bits.  Tables have exactly B rows (``rows=B`` of a longer allocation)."""
    B = 32 * tiles if rem == 0 else 32 * (tiles - 1) + rem
    cus = bounds["round"] // 4
    assert R.fused_plan(B, cus, False) == [("small" if tiles < R.SMALL_TILES else "main", B)]
    c = _case(native, gpu, R.HEADLINE, rowsA=IDENT_ROWS, rowsB=IDENT_ROWS)
    ia, ib = _ids(B, B, B, seed=B)
    _run_fused(native, gpu, c, None, ib, B=B, rowsA=B, rowsB=B, expect_oob=False)
    _run_fused(native, gpu, c, ia, None, B=B, rowsA=B, rowsB=B, expect_oob=False)
    _run_fused(native, gpu, c, None, None, B=B, rowsA=B, rowsB=B, expect_oob=False)
    if rem == 31:                   # the last 7 pairs run past either table: row 0 times 0, and the flag
        _run_fused(native, gpu, c, None, ib.clamp(max=B - 8), B=B, rowsA=B - 7, rowsB=B - 7, expect_oob=True)
        _run_fused(native, gpu, c, None, None, B=B, rowsA=B, rowsB=B - 7, expect_oob=True)


RAGGED = ["rem_small", "rem_main", "round+rem_small", "round+rem_main", "round+1pair"]


@pytest.mark.parametrize("which", RAGGED)
@pytest.mark.parametrize("inst", [R.HEADLINE, (128, 256, 0), (64, 128, 64)], ids=str)
def test_ragged_round_split_on_both_sides_of_the_permille_rule(native, gpu, bounds, inst, which):
    rnd, rs, rm = bounds["round"], bounds["rem_small"], bounds["rem_main"]
    cus = rnd // 4
    B = {"rem_small": 32 * rs, "rem_main": 32 * rm, "round+rem_small": 32 * (rnd + rs), "round+rem_main": 32 * (rnd + rm),
         "round+1pair": 32 * rnd + 1}[which]
    plan = R.fused_plan(B, cus, True)
    want = {"rem_small": [("small", B)], "rem_main": [("main", B)], "round+rem_small": [("main", 32 * rnd), ("small", 32 * rs)],
            "round+rem_main": [("main", B)], "round+1pair": [("main", 32 * rnd), ("small", 1)]}[which]
    if rs >= R.SMALL_TILES and rnd >= R.SMALL_TILES:
        assert plan == want
    assert R.fused_plan(B, cus, False) == [("main" if (B + 31) // 32 >= R.SMALL_TILES else "small", B)]
    rows = 32 * (rnd + rm)
    c = _case(native, gpu, inst, rowsA=rows, rowsB=rows)
    ia, ib = _ids(B, rows, rows, seed=B)
    _run_fused(native, gpu, c, ia, ib, expect_oob=False)
    ar = torch.arange(B)
    split = _run_fused(native, gpu, c, ar, ar, expect_oob=False)
    whole = _run_fused(native, gpu, c, None, None, B=B, expect_oob=False)
    R.assert_same_bits(whole, split, "identity ids (no split) vs ids 0 .. B-1 (split)")


@pytest.mark.parametrize("nonfinite", [False, True], ids=["row0_finite", "row0_inf_nan"])
@pytest.mark.parametrize("side", ["A", "B", "both"])
def test_out_of_range_ids_everywhere_a_tile_ends(native, gpu, bounds, side, nonfinite):
    """Finite row 0: the oracle's zero-half score, exactly.  Row 0 of inf, -inf and NaN: times 0 it is NaN in layer 1, which the
    ReLU reads as 0; read directly (ids 0 and 2) the infinities reach the score — NaN where the oracle says so, its bits elsewhere.
    At the N2 = 0 instance the one inf of row 2 meets last-layer weights of both signs: pair 7 scores NaN."""
    rnd = bounds["round"]
    for inst, B in [(i, b) for i in (R.HEADLINE, (128, 256, 0)) for b in (33, 32 * bounds["main_min"] - 31, 32 * rnd + 33)]:
        c = _case(native, gpu, inst, nonfinite=nonfinite)
        ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B, lo=3)
        plan = R.fused_plan(B, rnd // 4, True)
        seam = plan[0][1] if len(plan) == 2 else B // 2
        last = 32 * ((B - 1) // 32)
        where = sorted({p for p in (0, 5, 31, 32, seam - 33, seam - 1, seam, seam + 1, seam + 31, last, B - 2, B - 1) if 0 <= p < B})
        for n, p in enumerate(where):
            if side in ("A", "both"):
                ia[p] = BAD_IDS(ROWS_A)[n % 4]
            if side in ("B", "both"):
                ib[p] = BAD_IDS(ROWS_B)[(n + 1) % 4]
        for p in (1, 7, B - 3):     # direct reads of the non-finite rows
            if 0 <= p < B and p not in where:
                ia[p], ib[p] = (0, 0) if p != 7 else (2, 1)
        got = _run_fused(native, gpu, c, ia, ib, expect_oob=True)
        if not nonfinite:
            assert bool(torch.isfinite(got).all())
        elif inst[2] == 0:
            assert bool(torch.isnan(got[7]))


# ------------------------------------------------------------------------------------------------ ncf_mlp_pack
def _blob_f32(packed):
    return packed.blob.view(torch.float32).cpu().numpy()


def _np(ts):
    return [None if t is None else t.numpy() for t in ts]


@pytest.mark.parametrize("inst", [(64, 128, 64), (128, 256, 128), (256, 128, 0)], ids=str)
def test_packed_blob_is_the_restated_layout(native, gpu, inst):
    lib = native.load_library()
    dims = R.dims_of(inst)
    g = torch.Generator().manual_seed(sum(inst))
    ws, bs = R.random_mlp(g, dims)
    want = R.pack_blob(_np(ws), _np(bs))
    d = native._dims_array(dims)
    assert lib.ncf_mlp_packed_bytes(native.NCF_F32, len(ws), d) == 4 * R.blob_layout(dims)["total"] == want.nbytes
    packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
    assert np.array_equal(_blob_f32(packed).view(np.uint32), want.view(np.uint32))
    # a NULL single bias reads as zeros (every position in turn)
    for k in range(len(bs)):
        some = [None if i == k else b for i, b in enumerate(bs)]
        packed = native.PackedMLP([w.to(gpu) for w in ws], [None if b is None else b.to(gpu) for b in some])
        assert np.array_equal(_blob_f32(packed).view(np.uint32), R.pack_blob(_np(ws), _np(some)).view(np.uint32))
    # a NULL bias array: through the raw entry, into a blob full of sentinels
    wg = [w.to(gpu) for w in ws]
    blob = torch.full((want.size,), SENT, device=gpu)
    assert lib.ncf_mlp_pack(native.NCF_F32, len(ws), d, native._ptr_array(wg), None, blob.data_ptr(), want.nbytes,
                            native._stream(blob)) == native.NCF_OK
    assert np.array_equal(blob.cpu().numpy().view(np.uint32), R.pack_blob(_np(ws), None).view(np.uint32))
    # a non-contiguous weight source packs as its contiguous copy
    wide = [torch.randn(w.shape[0], 2 * w.shape[1], generator=g) for w in ws]
    views = [x.to(gpu)[:, ::2] for x in wide]
    assert not views[0].is_contiguous()
    packed = native.PackedMLP(views, [b.to(gpu) for b in bs])
    assert np.array_equal(_blob_f32(packed).view(np.uint32), R.pack_blob([x[:, ::2].numpy() for x in wide], _np(bs)).view(np.uint32))


def test_mlp_pack_refusals_write_nothing(native, gpu):
    lib = native.load_library()
    ws = [torch.randn(256, 128, device=gpu), torch.randn(128, 256, device=gpu), torch.randn(1, 128, device=gpu)]
    dims = [128, 256, 128, 1]
    nbytes = 4 * R.blob_layout(dims)["total"]
    blob = torch.full((nbytes // 4,), SENT, device=gpu)
    W = native._ptr_array(ws)

    def call(n_layers=3, d=dims, w=W, packed=blob.data_ptr(), size=nbytes, dtype=native.NCF_F32):
        rc = lib.ncf_mlp_pack(dtype, n_layers, None if d is None else native._dims_array(d), w, None, packed, size, native._stream(blob))
        torch.cuda.synchronize(gpu)
        assert bool((blob == SENT).all()), "a refused ncf_mlp_pack wrote to the blob"
        return rc

    E, U, WS = native.NCF_EINVAL, native.NCF_EUNSUPPORTED, native.NCF_EWORKSPACE
    assert call(d=[124, 256, 128, 1]) == U                       # K % 8
    assert call(d=[128, 240, 128, 1]) == U                       # N % 32
    assert call(d=[128, 256, 128, 2]) == U                       # last layer not 1 wide
    assert call(w=native._ptr_array([ws[0], None, ws[2]])) == E  # a null W[i]
    assert call(w=None) == E and call(d=None) == E and call(packed=None) == E
    assert call(n_layers=1, d=[128, 1]) == E and call(n_layers=4, d=[128, 256, 128, 64, 1]) == E
    assert call(dtype=7) == E
    assert call(size=nbytes - 4) == WS                           # a short buffer
    assert lib.ncf_mlp_packed_bytes(native.NCF_F32, 1, native._dims_array([128, 1])) == 0


# ------------------------------------------------------------------------------------------------ refusals of ncf_score_fused
def test_score_fused_refusals_launch_nothing(native, gpu):
    """Every refused call leaves a sentinel-filled ``out`` and the flag word as they were, though the ids hold an out-of-range
    entry that any launch would flag.  Return codes as mlp_fused.hip gives them: the shape is judged first (NCF_EUNSUPPORTED),
    then B == 0 (NCF_OK), then the arguments (NCF_EINVAL)."""
    lib = native.load_library()
    c = _case(native, gpu, R.HEADLINE)
    B = 40
    wideA = torch.zeros(ROWS_A, 72, device=gpu)
    ia = torch.randint(0, ROWS_A, (B,), device=gpu)
    ib = torch.randint(0, ROWS_B, (B,), device=gpu)
    ia[3] = ROWS_A
    out = torch.full((B,), SENT, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    ok = dict(dtype=native.NCF_F32, tabA=c["tag"].data_ptr(), rowsA=ROWS_A, ldA=64, tabB=c["tbg"].data_ptr(), rowsB=ROWS_B, ldB=64,
              idxA=ia.data_ptr(), idxB=ib.data_ptr(), B=B, EA=64, EB=64, n_layers=3, dims=[128, 256, 128, 1],
              packed=c["packed"].blob.data_ptr(), out=out.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.ncf_score_fused(a["dtype"], a["tabA"], a["rowsA"], a["ldA"], a["tabB"], a["rowsB"], a["ldB"], a["idxA"], a["idxB"],
                                 a["B"], a["EA"], a["EB"], a["n_layers"], native._dims_array(a["dims"]), a["packed"], a["out"],
                                 flag.data_ptr(), native._stream(out))
        torch.cuda.synchronize(gpu)
        assert bool((out == SENT).all()), f"a refused call wrote to out: {kw}"
        assert int(flag.item()) == 0, f"a refused call raised the flag: {kw}"
        return rc

    E, U = native.NCF_EINVAL, native.NCF_EUNSUPPORTED
    assert call(EA=60, EB=68) == U                                       # EA % 8
    assert call(EA=64, EB=32) == U                                       # EA + EB != dims[0]
    assert call(n_layers=2, dims=[128, 96, 1]) == U                      # not an instance
    assert call(dims=[128, 256, 64, 1]) == U
    assert call(n_layers=1, dims=[128, 1]) == U                          # 1 layer
    assert call(n_layers=4, dims=[128, 256, 128, 64, 1]) == U            # 4 layers
    assert call(dims=[128, 256, 128, 2]) == U                            # last width != 1
    assert call(B=-1) == E
    assert call(tabA=None) == E
    assert call(tabB=None) == E                                          # null tabB with EB > 0
    assert call(packed=None) == E
    assert call(out=None) == E
    assert call(ldA=32) == E and call(ldB=56) == E                       # ld < E
    assert call(tabA=wideA.data_ptr(), ldA=66) == E and call(ldB=70) == E  # ld % 4
    assert call(tabA=wideA.data_ptr() + 4, ldA=68) == E                  # a base 4 bytes off 16-byte alignment
    assert call(tabB=c["tbg"].data_ptr() + 4) == E
    assert call(packed=c["packed"].blob.data_ptr() + 4) == E
    assert call(B=0) == native.NCF_OK
    assert call(B=0, tabA=None, out=None) == native.NCF_OK
    # the same arguments unrefused do launch: the guard against a check that could not fail
    rc = lib.ncf_score_fused(ok["dtype"], ok["tabA"], ROWS_A, 64, ok["tabB"], ROWS_B, 64, ok["idxA"], ok["idxB"], B, 64, 64, 3,
                             native._dims_array(ok["dims"]), ok["packed"], ok["out"], flag.data_ptr(), native._stream(out))
    assert rc == native.NCF_OK and int(flag.item()) == 1 and not bool((out == SENT).any())


# ================================================================================================ ncf_score_folded
_fcases = {}


def _fcase(native, gpu, nm, rowsA=ROWS_A, rowsB=ROWS_B, nonfinite=False):
    key = (nm, rowsA, rowsB, nonfinite)
    if key not in _fcases:
        N1, N2 = nm
        g = torch.Generator().manual_seed(7 * N1 + N2)
        PA, PB = torch.randn(rowsA, N1, generator=g), torch.randn(rowsB, N1, generator=g)
        ws, bs = R.random_mlp(g, [N1, N2, 1])
        if nonfinite:
            PA[0, 1], PA[0, 6], PA[0, 9] = float("inf"), -float("inf"), float("nan")
            PB[0, 2], PB[0, 6], PB[0, 12] = float("nan"), float("inf"), -float("inf")
            PA[2, 3] = float("inf")
        tail = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
        _fcases[key] = dict(PA=PA, PB=PB, ws=ws, bs=bs, tail=tail, PAg=PA.to(gpu), PBg=PB.to(gpu))
    return _fcases[key]


def _run_folded(native, gpu, c, ia, ib, B=None, PAg=None, PBg=None, rowsA=None, rowsB=None, expect_oob=None):
    from oracle import c_oracle
    PA = c["PA"] if rowsA is None else c["PA"][:rowsA]
    PB = c["PB"] if rowsB is None else c["PB"][:rowsB]
    PAg = (c["PAg"] if rowsA is None else c["PAg"][:rowsA]) if PAg is None else PAg
    PBg = (c["PBg"] if rowsB is None else c["PBg"][:rowsB]) if PBg is None else PBg
    if B is None:
        B = len(ia) if ia is not None else len(ib)
    buf, out = _out(B, gpu)
    native.score_folded(PAg, None if ia is None else ia.to(gpu), PBg, None if ib is None else ib.to(gpu), c["tail"], out=out, B=B)
    ref, oob = c_oracle.score_folded_f32(PA, PB, ia, ib, c["ws"], c["bs"], B=B)
    if expect_oob is not None:
        assert oob == expect_oob
    got = out.cpu()
    _guards_intact(buf, B)
    R.assert_same_bits(got, ref, f"score_folded B={B}")
    _flag(native, gpu, oob)
    return got


FOLDED_B = [1, 31, 32, 33, 127, 128, 129, 4097]


@pytest.mark.parametrize("B", FOLDED_B)
@pytest.mark.parametrize("nm", R.FOLDED_INSTANCES, ids=str)
def test_folded_every_instance_at_tile_and_workgroup_edges(native, gpu, nm, B):
    assert native.folded_supported(*nm)
    c = _fcase(native, gpu, nm)
    ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B)
    _run_folded(native, gpu, c, ia, ib, expect_oob=False)


@pytest.mark.parametrize("nm", R.FOLDED_INSTANCES, ids=str)
def test_folded_identity_ids(native, gpu, nm):
    c = _fcase(native, gpu, nm, rowsA=4097, rowsB=4097)
    for B in (33, 129, 4097):
        ia, ib = _ids(B, B, B, seed=B)
        _run_folded(native, gpu, c, None, ib, B=B, rowsA=B, rowsB=B, expect_oob=False)
        _run_folded(native, gpu, c, ia, None, B=B, rowsA=B, rowsB=B, expect_oob=False)
        _run_folded(native, gpu, c, None, None, B=B, rowsA=B, rowsB=B, expect_oob=False)
    _run_folded(native, gpu, c, None, None, B=129, rowsA=129, rowsB=122, expect_oob=True)
    _run_folded(native, gpu, c, None, ib[:129].clamp(max=100), B=129, rowsA=126, rowsB=129, expect_oob=True)


@pytest.mark.parametrize("nm", R.FOLDED_INSTANCES, ids=str)
def test_folded_strided_p_tables(native, gpu, nm):
    c = _fcase(native, gpu, nm)
    PAg, PBg = _strided(c["PA"], 4, gpu), _strided(c["PB"], 4, gpu)
    for B in (33, 4097):
        ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B + 1)
        _run_folded(native, gpu, c, ia, ib, PAg=PAg, PBg=PBg, expect_oob=False)


@pytest.mark.parametrize("nonfinite", [False, True], ids=["row0_finite", "row0_inf_nan"])
@pytest.mark.parametrize("side", ["A", "B", "both"])
def test_folded_out_of_range_ids(native, gpu, side, nonfinite):
    """b1 lives in PA: an out-of-range A id reads row 0 of PA times 0 and so drops b1 with the row (the pair scores
    relu(PB[ib]) -> tail), where ncf_score_fused keeps b1; an out-of-range B id keeps it.  Pinned as it is — the sticky flag is
    what tells the caller.  With a finite row 0 and the A id out of range the score is that of a PA row of zeros, exactly."""
    from oracle import c_oracle
    for nm in R.FOLDED_INSTANCES:
        c = _fcase(native, gpu, nm, nonfinite=nonfinite)
        for B in (33, 129):
            ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B, lo=3)
            where = [0, 5, 31, 32, B - 2, B - 1]
            for n, p in enumerate(where):
                if side in ("A", "both"):
                    ia[p] = BAD_IDS(ROWS_A)[n % 4]
                if side in ("B", "both"):
                    ib[p] = BAD_IDS(ROWS_B)[(n + 1) % 4]
            ia[1], ib[1], ia[7], ib[7] = 0, 0, 2, 1      # direct reads of row 0 and of the row with one inf
            got = _run_folded(native, gpu, c, ia, ib, expect_oob=True)
            if not nonfinite:
                assert bool(torch.isfinite(got).all())
                if side == "A":     # b1 is gone with the row: a table whose row 0 is zeros, read in range, gives the same bits
                    zero = torch.cat((torch.zeros(1, nm[0]), c["PA"][1:]))
                    ref, oob = c_oracle.score_folded_f32(zero, c["PB"], torch.zeros(1, dtype=torch.long), ib[B - 1:], c["ws"], c["bs"])
                    assert not oob
                    R.assert_same_bits(got[B - 1:], ref, "out-of-range A id == a PA row of zeros")


@pytest.mark.parametrize("E", [32, 64])
@pytest.mark.parametrize("nm", R.FOLDED_INSTANCES, ids=str)
def test_folded_equals_fused_equals_float64_on_integer_data(native, gpu, nm, E):
    """Integer data under THE INTEGER CONDITION (fused_forms_ref): PA = linear(tabA, W1[:, :E], b1) and PB = linear(tabB,
    W1[:, E:]) computed on the device are exact, so score_folded equals float64 exactly — and score_fused, for the (N1, N2) that
    have a fused instance at K0 = 2 E ((256, 64) and (128, 128) have none and are held to float64 and the oracle alone).  In-range
    ids: the two forms differ on an out-of-range A id (test_folded_out_of_range_ids)."""
    from oracle import c_oracle
    N1, N2 = nm
    g = torch.Generator().manual_seed(N1 + N2 + E)
    ta, tb, ws, bs = R.int_case(g, E, E, [N1, N2], 300, 200)
    B = 32 * 9 + 5
    ia, ib = _ids(B, 300, 200, seed=E)
    assert R.int_margin(ta, tb, ia, ib, ws, bs) < 2 ** 24
    ref = R.score_f64(ta, tb, ia, ib, ws, bs)
    dev = lambda t: t.to(gpu)
    PA = native.linear(dev(ta), dev(ws[0][:, :E].contiguous()), dev(bs[0]))
    PB = native.linear(dev(tb), dev(ws[0][:, E:].contiguous()))
    PAr, PBr = R.fold_tables(ta, tb, ws[0], bs[0])
    assert torch.equal(PA.cpu(), PAr) and torch.equal(PB.cpu(), PBr)
    tail = native.PackedMLP([dev(w) for w in ws[1:]], [dev(b) for b in bs[1:]])
    folded = native.score_folded(PA, dev(ia), PB, dev(ib), tail).cpu()
    assert torch.equal(folded.double(), ref)
    R.assert_same_bits(folded, c_oracle.score_folded_f32(PAr, PBr, ia, ib, ws[1:], bs[1:])[0], "folded vs folded oracle")
    dims = [2 * E, N1, N2, 1]
    if native.fused_supported(E, E, dims):
        packed = native.PackedMLP([dev(w) for w in ws], [dev(b) for b in bs])
        fused = native.score_fused(dev(ta), dev(ia), dev(tb), dev(ib), packed).cpu()
        R.assert_same_bits(fused, folded, "score_fused vs score_folded")
        assert torch.equal(fused.double(), ref)
    else:
        assert (2 * E, N1, N2) not in R.INSTANCES
    native.check_oob(gpu)


def test_score_folded_refusals_launch_nothing(native, gpu):
    lib = native.load_library()
    c = _fcase(native, gpu, (256, 128))
    B = 40
    wide = torch.zeros(ROWS_A, 264, device=gpu)
    ia = torch.randint(0, ROWS_A, (B,), device=gpu)
    ib = torch.randint(0, ROWS_B, (B,), device=gpu)
    ib[B - 1] = -1
    out = torch.full((B,), SENT, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    ok = dict(dtype=native.NCF_F32, PA=c["PAg"].data_ptr(), rowsA=ROWS_A, ldA=256, PB=c["PBg"].data_ptr(), rowsB=ROWS_B, ldB=256,
              idxA=ia.data_ptr(), idxB=ib.data_ptr(), B=B, N1=256, N2=128, tail=c["tail"].blob.data_ptr(), out=out.data_ptr())

    def raw(a):
        return lib.ncf_score_folded(a["dtype"], a["PA"], a["rowsA"], a["ldA"], a["PB"], a["rowsB"], a["ldB"], a["idxA"], a["idxB"],
                                    a["B"], a["N1"], a["N2"], a["tail"], a["out"], flag.data_ptr(), native._stream(out))

    def call(**kw):
        rc = raw(dict(ok, **kw))
        torch.cuda.synchronize(gpu)
        assert bool((out == SENT).all()), f"a refused call wrote to out: {kw}"
        assert int(flag.item()) == 0, f"a refused call raised the flag: {kw}"
        return rc

    E, U = native.NCF_EINVAL, native.NCF_EUNSUPPORTED
    assert call(dtype=native.NCF_BF16) == U and call(dtype=7) == U       # a wrong dtype
    assert call(N1=256, N2=256) == U and call(N1=64, N2=64) == U         # an (N1, N2) without a kernel
    assert call(ldA=128) == E and call(ldB=252) == E                     # ld < N1
    assert call(PA=wide.data_ptr(), ldA=258) == E and call(ldB=262) == E  # ld % 4
    assert call(PA=wide.data_ptr() + 4, ldA=260) == E                    # misaligned PA / PB / tail
    assert call(PB=c["PBg"].data_ptr() + 8) == E
    assert call(tail=c["tail"].blob.data_ptr() + 4) == E
    assert call(PA=None) == E and call(PB=None) == E and call(tail=None) == E and call(out=None) == E
    assert call(B=-1) == E
    assert call(B=0) == native.NCF_OK and call(B=0, PA=None, out=None) == native.NCF_OK
    assert raw(ok) == native.NCF_OK and int(flag.item()) == 1 and not bool((out == SENT).any())


# ================================================================================================ the partial scorer
@pytest.mark.parametrize("rows", [33, 900])
@pytest.mark.parametrize("N1", [128, 256])
@pytest.mark.parametrize("EA,EB", [(32, 32), (64, 64), (32, 96), (128, 128)])
def test_partial_p_is_the_oracles_truncated_layer1_chain(native, gpu, EA, EB, N1, rows):
    from oracle import c_oracle
    g = torch.Generator().manual_seed(EA + 3 * EB + N1 + rows)
    ta = torch.randn(rows, EA, generator=g) * 0.5
    ws, bs = R.random_mlp(g, [EA + EB, N1, 1])
    packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
    assert native.partial_supported(EA, EB, packed)
    ref = c_oracle.layer1_partial_f32(ta, ws[0], bs[0])
    buf = torch.full((rows + 1 + 2, N1), SENT, device=gpu)
    P = native.layer1_partial(ta.to(gpu), packed, out=buf[1:rows + 2])
    assert P.shape == (rows + 1, N1)
    R.assert_same_bits(P.cpu().reshape(-1), ref.reshape(-1), "P")
    R.assert_same_bits(P[rows].cpu(), ref[rows], "P's out-of-range row")
    assert bool((buf[0] == SENT).all()) and bool((buf[rows + 2] == SENT).all())


def test_partial_strided_operands_against_the_oracle_over_the_whole_batch(native, gpu, bounds):
    """tabA, tabB and P strided (ldP = N1 + 4, every base 16 bytes into its buffer) at R / 2 + 33 pairs, the smallest batch the
    partial kernel keeps — compared with the oracle, not with score_fused, on every pair, the out-of-range ones included."""
    from oracle import c_oracle
    EA, EB, hidden = 64, 64, [256, 128]
    c = _case(native, gpu, (EA + EB, hidden[0], hidden[1]), EA)
    B = 32 * bounds["round"] // 2 + 33
    tiles, rnd = (B + 31) // 32, bounds["round"]
    assert tiles < rnd and tiles * 1000 > rnd * R.PART_PERMILLE          # past the share that goes back to ncf_score_fused
    tag, tbg = _strided(c["ta"], 4, gpu), _strided(c["tb"], 12, gpu)
    Pbuf = _strided(torch.zeros(ROWS_A + 1, hidden[0]), 4, gpu, fill=SENT)
    P = native.layer1_partial(tag, c["packed"], out=Pbuf)
    R.assert_same_bits(P.cpu().reshape(-1), c_oracle.layer1_partial_f32(c["ta"], c["ws"][0], c["bs"][0]).reshape(-1), "strided P")
    ia, ib = _ids(B, ROWS_A, ROWS_B, seed=B)
    for n, p in enumerate((0, 31, 32, B // 2, B - 34, B - 33, B - 2)):
        ia[p] = BAD_IDS(ROWS_A)[n % 4]
        ib[p + 1] = BAD_IDS(ROWS_B)[n % 4]
    buf, out = _out(B, gpu)
    native.score_fused_partial(P, tag, ia.to(gpu), tbg, ib.to(gpu), c["packed"], out=out)
    ref, oob = c_oracle.score_fused_f32_ex(c["ta"], c["tb"], ia, ib, c["ws"], c["bs"])
    assert oob
    _guards_intact(buf, B)
    R.assert_same_bits(out.cpu(), ref, "score_fused_partial, strided")
    _flag(native, gpu, True)
