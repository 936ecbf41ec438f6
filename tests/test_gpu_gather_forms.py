"""GPU: the embedding gather (gather.hip) in every launch form it can take, and gather_dot, against exact references.

gather_concat moves bytes, so its reference is torch indexing on the INTEGER view of the tables and every comparison is
bitwise on the integer view of the output: tables hold random 32-bit / 16-bit patterns (NaN payloads, -0.0 and denormals
included), which a float ``==`` could not tell apart.  Each case runs the one-step-per-wave kernel, the persistent kernel
(``gather_kernel`` = "step" / "persistent") and the automatic choice; all three must give the reference's bits.

Batch sizes come from the launch rule of gather.hip, not from the workloads: LPP lanes (8 / 16 / 32 / 64, the smallest that
holds the row's 16-byte chunks) share a pair, a wave moves PPW = 64 / LPP pairs per step, and the persistent form runs
W = 4 * min(8 * CUs, ceil(B / (4 * PPW))) waves which keep three steps in flight.  With W at its cap, B around W * PPW,
2 * W * PPW and 3 * W * PPW gives every wave one, two and three-or-more pipeline steps, each with a ragged tail.

gather_dot has two references that need no measured tolerance: integer tables (every partial sum exact in fp32, so the
result equals the int64 dot product whatever the order) and random tables against float64 under the forward bound
|out - ref| <= (ceil(E / 16) + 4) * 2^-24 * sum_e |a_e * b_e| — a lane chains at most ceil(E / 16) FMAs (inputs and
products exact inside the FMA), four shuffle adds follow.
"""
import pytest
import torch

from conftest import record_error

pytestmark = pytest.mark.gpu

FORMS = ("step", "persistent", None)      # None: the library's own choice
G_MAXBLOCKS = 256 * 128                   # NCF_G_MAXBLOCKS of gather.hip: the step form's grid cap (4 waves per block)
SCALAR_MAXBLOCKS = 8192                   # grid cap of the scalar fallback (256 threads per block, one element each)
DOT_MAXBLOCKS = 8192                      # grid cap of gather_dot (16 pairs per block)
ROWS_A, ROWS_B = 1013, 257


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


@pytest.fixture(scope="module")
def waves_cap(gpu):
    """Waves of the persistent form at its cap: 8 workgroups of 4 waves per CU."""
    return 4 * 8 * torch.cuda.get_device_properties(gpu).multi_processor_count


def _int_dtype(dtype):
    return torch.int32 if dtype == torch.float32 else torch.int16


def _ints(t):
    return t.view(_int_dtype(t.dtype))


def _pattern_table(gen, rows, E, dtype, pad_left=0, pad_right=0):
    """(rows, E) table of random bit patterns, a column slice of a (rows, pad_left + E + pad_right) buffer; the first row
    starts with -0.0, the smallest denormal, a signalling-NaN pattern and a negative quiet NaN with a payload."""
    it = _int_dtype(dtype)
    lim = 2 ** 31 if it == torch.int32 else 2 ** 15
    buf = torch.randint(-lim, lim, (rows, pad_left + E + pad_right), generator=gen, device=gen.device, dtype=torch.int64).to(it)
    special = [-lim, 1, 0x7F800001, -0x3EDCBB] if it == torch.int32 else [-lim, 1, 0x7F81, -0x3F]
    n = min(E, 4)
    buf[0, pad_left:pad_left + n] = torch.tensor(special[:n], device=gen.device).to(it)
    return buf.view(dtype)[:, pad_left:pad_left + E]


def _ids(gen, rows, B):
    idx = torch.randint(0, rows, (B,), generator=gen, device=gen.device)
    idx[0] = 0                             # row 0 carries the special patterns; both ends of the table are always hit
    idx[-1] = rows - 1
    if B > 2:
        idx[B // 2] = 0
    return idx


def _half(t, idx, B):
    """Integer rows of one table for ids ``idx`` (None: identity); an id outside the table reads as a zero row."""
    rows = t.shape[0]
    idx = torch.arange(B, device=t.device) if idx is None else idx
    ok = (idx >= 0) & (idx < rows)
    got = _ints(t)[idx.clamp(0, rows - 1)]
    return torch.where(ok[:, None], got, torch.zeros_like(got)), bool(ok.all())


def _reference(ta, ia, tb, ib, B):
    a, good = _half(ta, ia, B)
    if tb is None:
        return a, good
    b, good_b = _half(tb, ib, B)
    return torch.cat((a, b), 1), good and good_b


def _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B, forms=FORMS, ref=None, good=True):
    """Every form gives the reference's bits; the out-of-range flag is raised exactly when an id was bad, once."""
    if ref is None:
        ref, good = _reference(ta, ia, tb, ib, B)
    for form in forms:
        kernel_option("gather_kernel", form)
        out = native.gather_concat(ta, ia, tb, ib, B=B)
        assert out.shape == ref.shape
        assert torch.equal(_ints(out), ref), f"form {form}, B {B}"
        if good:
            native.check_oob(gpu)
        else:
            with pytest.raises(IndexError):
                native.check_oob(gpu)
            native.check_oob(gpu)          # raised once, then clear
    return ref


def _lpp(EA, EB, dtype):
    cpp = (EA + EB) * (4 if dtype == torch.float32 else 2) // 16
    return next(l for l in (8, 16, 32, 64) if cpp <= l) if cpp <= 64 else 64


def _pipeline_batches(W, PPW):
    return [1, PPW + 1, W * PPW - 1, W * PPW, W * PPW + 1, 2 * W * PPW + 1, 3 * W * PPW + PPW + 1]


F32, BF16 = torch.float32, torch.bfloat16
# (dtype, EA, EB): every launch_vec16<LPP> instantiation at full and partly idle rows, even and uneven A/B splits
WIDTHS = [
    (F32, 4, 0), (F32, 16, 4), (F32, 16, 16), (BF16, 8, 0), (BF16, 32, 8), (BF16, 32, 32),          # LPP 8: cpp 1, 5, 8
    (F32, 20, 16), (F32, 32, 32), (F32, 8, 56), (BF16, 40, 32), (BF16, 64, 64), (BF16, 16, 112),    # LPP 16: cpp 9, 16
    (F32, 36, 32), (F32, 64, 64), (BF16, 72, 64), (BF16, 128, 128),                                 # LPP 32: cpp 17, 32
    (F32, 68, 64), (F32, 128, 128), (BF16, 136, 128), (BF16, 256, 256),                             # LPP 64: cpp 33, 64
    (F32, 256, 256), (BF16, 512, 512),                                     # cpp 128: "persistent" falls back to the step form
]


@pytest.mark.parametrize("dtype,EA,EB", WIDTHS, ids=lambda v: str(v).replace("torch.", ""))
def test_every_width_fills_the_pipeline(native, gpu, kernel_option, waves_cap, dtype, EA, EB):
    gen = torch.Generator(device=gpu).manual_seed(EA * 1031 + EB)
    PPW = 64 // _lpp(EA, EB, dtype)
    ta = _pattern_table(gen, ROWS_A, EA, dtype)
    tb = _pattern_table(gen, ROWS_B, EB, dtype) if EB else None
    for B in _pipeline_batches(waves_cap, PPW):
        ia = _ids(gen, ROWS_A, B)
        ib = _ids(gen, ROWS_B, B) if EB else None
        _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B)
    for B in (2 * waves_cap * PPW - 1, 2 * waves_cap * PPW + 1):          # either side of the automatic switch between forms
        ia = _ids(gen, ROWS_A, B)
        ib = _ids(gen, ROWS_B, B) if EB else None
        _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B, forms=(None,))


OPERAND_WIDTHS = [(F32, 16, 4), (BF16, 64, 64), (F32, 64, 64), (F32, 68, 64)]     # LPP 8 (idle lanes), 16, 32, 64 (idle lanes)


@pytest.mark.parametrize("dtype,EA,EB", OPERAND_WIDTHS, ids=lambda v: str(v).replace("torch.", ""))
def test_operand_forms(native, gpu, kernel_option, waves_cap, dtype, EA, EB):
    gen = torch.Generator(device=gpu).manual_seed(EA * 77 + EB)
    PPW = 64 // _lpp(EA, EB, dtype)
    B = 2 * waves_cap * PPW + PPW + 1                                      # three steps for the first waves, ragged tail
    per16 = 16 // (4 if dtype == F32 else 2)
    # tables that are column slices of wider buffers (ld > E, 16-byte aligned)
    ta = _pattern_table(gen, ROWS_A, EA, dtype, pad_left=per16, pad_right=2 * per16)
    tb = _pattern_table(gen, ROWS_B, EB, dtype, pad_left=3 * per16, pad_right=0)
    assert ta.stride(0) > EA and tb.stride(0) > EB
    ia, ib = _ids(gen, ROWS_A, B), _ids(gen, ROWS_B, B)
    ref = _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B)
    # EB = 0: the single-table call shape
    _check_forms(native, kernel_option, gpu, ta, ia, None, None, B)
    # heavy repeats of one id
    ia_hot = ia.clone()
    ia_hot[::2] = 5
    ib_hot = torch.full_like(ib, ROWS_B - 1)
    _check_forms(native, kernel_option, gpu, ta, ia_hot, tb, ib_hot, B)
    # out= a column slice of a wider buffer with more rows than B: nothing outside [0:B, 0:E] may change
    E = EA + EB
    it = _int_dtype(dtype)
    sentinel = 0x5A5A if it == torch.int16 else 0x5A5A5A5A
    for form in FORMS:
        kernel_option("gather_kernel", form)
        wide = torch.full((B + 3, per16 + E + per16), sentinel, dtype=it, device=gpu).view(dtype)
        got = native.gather_concat(ta, ia, tb, ib, out=wide[:, per16:per16 + E], B=B)
        assert got.data_ptr() == wide[:, per16:].data_ptr()
        w = _ints(wide)
        assert torch.equal(w[:B, per16:per16 + E], ref), f"form {form}"
        assert bool((w[:B, :per16] == sentinel).all()) and bool((w[:B, per16 + E:] == sentinel).all()) and bool((w[B:] == sentinel).all())
    native.check_oob(gpu)
    # identity indices (None): both, A only, B only; tables as long as the batch
    ida = _pattern_table(gen, B, EA, dtype)
    idb = _pattern_table(gen, B, EB, dtype)
    _check_forms(native, kernel_option, gpu, ida, None, idb, None, B)
    _check_forms(native, kernel_option, gpu, ida, None, tb, ib, B)
    _check_forms(native, kernel_option, gpu, ta, ia, idb, None, B)
    _check_forms(native, kernel_option, gpu, ida, None, None, None, B)
    # ... and B > rows: the rows past the table read as zeros and raise the flag
    ref, good = _reference(ida[:B - 5], None, idb, None, B)
    assert not good and int(ref[B - 5:, :EA].abs().max()) == 0
    _check_forms(native, kernel_option, gpu, ida[:B - 5], None, idb, None, B, ref=ref, good=False)
    ref, good = _reference(ida, None, idb[:B - PPW - 2], None, B)
    _check_forms(native, kernel_option, gpu, ida, None, idb[:B - PPW - 2], None, B, ref=ref, good=False)


@pytest.mark.parametrize("dtype,EA,EB", [(F32, 64, 64), (BF16, 32, 8), (F32, 68, 0)], ids=lambda v: str(v).replace("torch.", ""))
def test_bad_ids_in_every_pipeline_step(native, gpu, kernel_option, waves_cap, dtype, EA, EB):
    """A negative id or one equal to the row count, in A, in B or in both, in the first, a middle and the last pipeline
    step: the bad half of that row reads as zeros, everything else is exact, the flag raises once."""
    gen = torch.Generator(device=gpu).manual_seed(EA + 3 * EB)
    PPW = 64 // _lpp(EA, EB, dtype)
    B = 2 * waves_cap * PPW + PPW + 1
    ta = _pattern_table(gen, ROWS_A, EA, dtype)
    tb = _pattern_table(gen, ROWS_B, EB, dtype) if EB else None
    ia = _ids(gen, ROWS_A, B)
    ib = _ids(gen, ROWS_B, B) if EB else None
    good_ref = _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B)      # good ids leave the flag clear
    places = {"first": 0, "middle": waves_cap * PPW + PPW // 2, "last": B - 1}
    for where, p in places.items():
        for which in (("A", "B", "AB") if EB else ("A",)):
            for bad_a, bad_b in ((-1, ROWS_B), (ROWS_A, -1)):
                ja, jb = ia.clone(), ib.clone() if EB else None
                ref = good_ref.clone()
                if "A" in which:
                    ja[p] = bad_a
                    ref[p, :EA] = 0
                if "B" in which:
                    jb[p] = bad_b
                    ref[p, EA:] = 0
                _check_forms(native, kernel_option, gpu, ta, ja, tb, jb, B, ref=ref, good=False)
    _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B, ref=good_ref)   # and the flag is clear again afterwards


def test_step_form_grid_stride(native, gpu, kernel_option):
    """The one-step-per-wave kernel beyond its grid cap: B > NCF_G_MAXBLOCKS * 4 * PPW at LPP = 64 (PPW = 1), cpp = 33."""
    gen = torch.Generator(device=gpu).manual_seed(11)
    EA, EB = 68, 64
    B = G_MAXBLOCKS * 4 * 1 + 3
    ta = _pattern_table(gen, ROWS_A, EA, F32)
    tb = _pattern_table(gen, ROWS_B, EB, F32)
    ia, ib = _ids(gen, ROWS_A, B), _ids(gen, ROWS_B, B)
    ia[B - 2] = ROWS_A                                                      # a bad id in the strided part
    ref, good = _reference(ta, ia, tb, ib, B)
    assert not good
    _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B, forms=("step", "persistent"), ref=ref, good=False)


@pytest.mark.parametrize("dtype,EA,EB", [(F32, 5, 3), (BF16, 4, 4), (F32, 7, 0)], ids=lambda v: str(v).replace("torch.", ""))
def test_scalar_fallback(native, gpu, kernel_option, dtype, EA, EB):
    """Rows that are no multiple of 16 bytes take the element-granular kernel, whatever form is asked for."""
    gen = torch.Generator(device=gpu).manual_seed(EA)
    ta = _pattern_table(gen, ROWS_A, EA, dtype, pad_left=1, pad_right=2)
    tb = _pattern_table(gen, ROWS_B, EB, dtype, pad_left=0, pad_right=1) if EB else None
    for B in (1, 2, 255, 257, 1000):
        ia = _ids(gen, ROWS_A, B)
        ib = _ids(gen, ROWS_B, B) if EB else None
        _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B)
    B = 1000
    ia[3], ia[B - 1] = -1, ROWS_A
    if EB:
        ib[3], ib[500] = ROWS_B, -7
    ref, good = _reference(ta, ia, tb, ib, B)
    assert not good
    _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B, ref=ref, good=False)
    # identity ids, B > rows of A
    ref, good = _reference(ta, None, tb, ib, B) if EB else _reference(ta[:990], None, None, None, B)
    _check_forms(native, kernel_option, gpu, ta if EB else ta[:990], None, tb, ib if EB else None, B, ref=ref, good=good)
    # out= inside a wider sentinel buffer
    it = _int_dtype(dtype)
    E = EA + EB
    ia = _ids(gen, ROWS_A, B)
    ref, _ = _reference(ta, ia, tb, ib, B)
    wide = torch.full((B + 2, E + 3), 0x5A5A, dtype=it, device=gpu).view(dtype)
    native.gather_concat(ta, ia, tb, ib, out=wide[:, 1:1 + E], B=B)
    if EB:
        with pytest.raises(IndexError):                                     # ib still holds the bad ids
            native.check_oob(gpu)
    w = _ints(wide)
    assert torch.equal(w[:B, 1:1 + E], ref)
    assert bool((w[:B, 0] == 0x5A5A).all()) and bool((w[:B, 1 + E:] == 0x5A5A).all()) and bool((w[B:] == 0x5A5A).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_scalar_fallback_unaligned_base(native, gpu, kernel_option, dtype):
    """16-byte-tileable rows whose table starts one element into its allocation: not 16-byte aligned, so the scalar kernel."""
    gen = torch.Generator(device=gpu).manual_seed(5)
    EA, EB, B = 64, 64, 777
    flat = _pattern_table(gen, 1, ROWS_A * EA + 1, dtype)[0]
    ta = flat[1:].view(ROWS_A, EA)
    assert ta.data_ptr() % 16 != 0
    tb = _pattern_table(gen, ROWS_B, EB, dtype)
    _check_forms(native, kernel_option, gpu, ta, _ids(gen, ROWS_A, B), tb, _ids(gen, ROWS_B, B), B)


def test_scalar_fallback_grid_stride(native, gpu, kernel_option):
    """B * (EA + EB) > 8192 * 256: the scalar kernel's stride loop runs."""
    gen = torch.Generator(device=gpu).manual_seed(6)
    EA, EB = 5, 3
    B = SCALAR_MAXBLOCKS * 256 // (EA + EB) + 1001
    assert B * (EA + EB) > SCALAR_MAXBLOCKS * 256
    ta = _pattern_table(gen, ROWS_A, EA, F32)
    tb = _pattern_table(gen, ROWS_B, EB, F32)
    ia, ib = _ids(gen, ROWS_A, B), _ids(gen, ROWS_B, B)
    _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B, forms=(None,))
    ib[B - 3] = ROWS_B
    ref, good = _reference(ta, ia, tb, ib, B)
    _check_forms(native, kernel_option, gpu, ta, ia, tb, ib, B, forms=(None,), ref=ref, good=False)


# ----------------------------------------------------------------------------- gather_dot
DOT_E = [1, 5, 15, 16, 17, 64, 100, 128, 256]
DOT_B = [1, 2, 3, 4, 5, 777, DOT_MAXBLOCKS * 16 + 5]
U24 = 2.0 ** -24


def _dot_tables(gen, E, dtype, integer):
    """Two tables that are column slices of wider buffers (leading dimension > E, odd element offsets)."""
    def one(rows, left, right):
        shape = (rows, left + E + right)
        if integer:
            t = torch.randint(-8, 9, shape, generator=gen, device=gen.device).to(dtype)
        else:
            t = torch.randn(shape, generator=gen, device=gen.device).to(dtype)
        return t[:, left:left + E]
    return one(301, 3, 1), one(203, 0, 5)


def _dot_bound_check(out, a, b, E, tag):
    a, b = a.double(), b.double()
    ref = (a * b).sum(1, keepdim=True)
    bound = ((E + 15) // 16 + 4) * U24 * (a * b).abs().sum(1, keepdim=True)
    err = (out.double() - ref).abs()
    used = err / bound.clamp_min(1e-300)
    k = int(used.argmax())
    record_error(tag, float(err.flatten()[k]), float(bound.flatten()[k]), scale_rel=float(err.max()) / max(float(ref.abs().max()), 1e-300))
    assert bool((err <= bound).all()), f"{tag}: worst {float(used.max()):.3f} of the bound"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("E", DOT_E)
def test_gather_dot_exact_and_bounded(native, gpu, dtype, E):
    gen = torch.Generator(device=gpu).manual_seed(E)
    ti_a, ti_b = _dot_tables(gen, E, dtype, integer=True)
    tr_a, tr_b = _dot_tables(gen, E, dtype, integer=False)
    assert ti_a.stride(0) > E
    for B in DOT_B:
        ia, ib = _ids(gen, 301, B), _ids(gen, 203, B)
        out = native.gather_dot(ti_a, ia, ti_b, ib)
        assert out.shape == (B, 1) and out.dtype == torch.float32
        assert torch.equal(out.double(), (ti_a[ia].long() * ti_b[ib].long()).sum(1, keepdim=True).double()), f"B {B}"
        out = native.gather_dot(tr_a, ia, tr_b, ib)
        _dot_bound_check(out, tr_a[ia], tr_b[ib], E, "")
    native.check_oob(gpu)
    # null index arrays: identity rows
    for B in (1, 5, 203):
        ib = _ids(gen, 203, B)
        ia = _ids(gen, 301, B)
        assert torch.equal(native.gather_dot(ti_a, None, ti_b, ib, B=B).double(), (ti_a[:B].long() * ti_b[ib].long()).sum(1, keepdim=True).double())
        assert torch.equal(native.gather_dot(ti_a, ia, ti_b, None, B=B).double(), (ti_a[ia].long() * ti_b[:B].long()).sum(1, keepdim=True).double())
        assert torch.equal(native.gather_dot(ti_a, None, ti_b, None, B=B).double(), (ti_a[:B].long() * ti_b[:B].long()).sum(1, keepdim=True).double())
        _dot_bound_check(native.gather_dot(tr_a, None, tr_b, None, B=B), tr_a[:B], tr_b[:B], E, "")
    native.check_oob(gpu)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("E", [5, 16, 100])
def test_gather_dot_bad_ids(native, gpu, dtype, E):
    """A bad id on either side: the pair's output is exactly +0.0, the others are untouched, the flag raises once."""
    gen = torch.Generator(device=gpu).manual_seed(E + 1)
    ta, tb = _dot_tables(gen, E, dtype, integer=True)
    ta, tb = ta.abs() + 1, tb.abs() + 1                                     # every true dot product is positive
    for B in (1, 3, 5, 777, DOT_MAXBLOCKS * 16 + 5):
        ia, ib = _ids(gen, 301, B), _ids(gen, 203, B)
        ref = (ta[ia].long() * tb[ib].long()).sum(1, keepdim=True).double()
        assert torch.equal(native.gather_dot(ta, ia, tb, ib).double(), ref)
        native.check_oob(gpu)                                               # good ids: flag clear
        bad = sorted({0, B // 2, B - 1})
        for n, p in enumerate(bad):
            if n % 2 == 0:
                ia[p] = -1 if p else 301
            else:
                ib[p] = 203
            ref[p] = 0
        out = native.gather_dot(ta, ia, tb, ib)
        assert torch.equal(out.double(), ref)
        assert int(out.view(torch.int32)[bad].abs().max()) == 0             # +0.0, bit for bit
        with pytest.raises(IndexError):
            native.check_oob(gpu)
        native.check_oob(gpu)
    # identity ids past the end of a table
    out = native.gather_dot(ta, None, tb, None, B=210)
    ref = (ta[:210].long() * torch.cat((tb, tb[:7])).long()).sum(1, keepdim=True).double()
    ref[203:] = 0
    assert torch.equal(out.double(), ref)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
