"""GPU: ncf_dot_topk (native.dot_topk) equals score-then-select — native.topk_rows over native.gather_dot's score matrix — bit for
bit (scores, ids, counts): every supported width class, k up to the fused limit, one and many column tiles, with and without an
item id list, exclusion lists; exact ties, zero rows, NaN / inf; refusals are status codes that launch nothing; bad ids set the
out-of-range flag; the call captures into a HIP graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _csr(lists, dev):
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64, device=dev)
    col = torch.tensor(np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]), dtype=torch.int32, device=dev)
    return rowptr, col


def _rand(rows, D, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(rows, D, device=dev, generator=g)


def _reference(A, ia, B, ib, k, seen):
    from deeprecommendation_amd import native
    rows = ia if ia is not None else torch.arange(A.shape[0], device=A.device)
    cols = ib if ib is not None else torch.arange(B.shape[0], device=A.device)
    nu, ni = rows.numel(), cols.numel()
    s = native.gather_dot(A, rows.repeat_interleave(ni), B, cols.repeat(nu)).view(nu, ni)
    return native.topk_rows(s, k, seen)


def _check(A, ia, B, ib, k, seen=None):
    from deeprecommendation_amd import native
    got = native.dot_topk(A, ia, B, ib, k, seen)
    ref = _reference(A, ia, B, ib, k, seen)
    torch.cuda.synchronize()
    assert torch.equal(got[2], ref[2])
    assert torch.equal(got[1], ref[1])
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))
    return got


@pytest.mark.parametrize("D", [1, 15, 16, 64, 100, 256])
@pytest.mark.parametrize("k", [1, 10, 100, 128])
def test_dot_topk_equals_score_then_select(gpu, D, k):
    A = _rand(150, D, D * 31 + k, gpu)
    B = _rand(12000, D, D * 37 + k, gpu)
    g = torch.Generator(device=gpu).manual_seed(k)
    ia = torch.randint(0, 150, (70,), device=gpu, generator=g)            # 70 users: one full and one ragged user block
    _check(A, ia, B, None, k)
    ib = torch.randint(0, 12000, (9000,), device=gpu, generator=g)        # an id list (with repeats) instead of every row
    _check(A, ia, B, ib, k)


@pytest.mark.parametrize("I", [1, 100, 8191, 8192, 8193, 70000])
def test_dot_topk_column_tiles(gpu, I):
    A = _rand(130, 64, I, gpu)
    B = _rand(I, 64, I + 1, gpu)
    _check(A, None, B, None, 100)
    _check(A, None, B, None, 7)


def test_dot_topk_above_2_20_columns(gpu):
    I = (1 << 20) + 3000
    A = _rand(3, 32, 5, gpu)
    B = _rand(I, 32, 6, gpu)
    _check(A, None, B, None, 100)


def test_dot_topk_many_users_and_strided_tables(gpu):
    """Tables with leading dimension > D (views) and ten 64-user blocks.  The rows still fit one pass over the key workspace
    (chunk_rows == rows); the chunked form is test_gpu_rank_forms.test_dot_topk_in_row_chunks."""
    A = _rand(600, 80, 1, gpu)[:, :72]
    B = _rand(20000, 80, 2, gpu)[:, :72]
    _check(A, None, B, None, 50)


def test_dot_topk_exclusion(gpu):
    I, k = 20000, 100
    A = _rand(6, 64, 3, gpu)
    B = _rand(I, 64, 4, gpu)
    rng = np.random.default_rng(0)
    lists = [[],                                                   # nothing excluded
             list(range(0, I, 3)),                                 # a third of the columns
             list(range(I)),                                       # everything: count 0
             [c for c in range(I) if c % 4000 != 7],               # all but 5 columns: count 5 < k
             rng.integers(0, I, 5000).tolist() + [-1, I, I + 50],  # unsorted, duplicates, ids outside the list
             rng.permutation(I)[:15000].tolist()]
    s, i, n = _check(A, None, B, None, k, _csr(lists, gpu))
    n = n.cpu()
    assert n[2] == 0 and n[3] == 5 and n[0] == k
    ib = torch.randint(0, I, (I // 2,), device=gpu)
    _check(A, None, B, ib, k, _csr([x[: I // 4] for x in lists], gpu))


def test_dot_topk_ties_zero_rows_and_specials(gpu):
    from deeprecommendation_amd import native
    D, I = 64, 10000
    base = _rand(40, D, 7, gpu)
    B = base[torch.randint(0, 40, (I,), device=gpu)].contiguous()            # duplicated rows: exact ties, lower column first
    A = _rand(20, D, 8, gpu)
    A[3] = 0.0                                                                # every score +0: the first k columns
    s, i, n = _check(A, None, B, None, 100)
    assert torch.equal(i[3].cpu(), torch.arange(100, dtype=torch.int32))
    Bi = torch.randint(-3, 4, (I, D), device=gpu).float()                     # small integers: exact sums, heavy ties
    Ai = torch.randint(-3, 4, (20, D), device=gpu).float()
    _check(Ai, None, Bi, None, 128)
    # NaN / inf: ranks like topk_rows (NaN last); a NaN's payload need not survive, so NaN scores are compared as NaN
    Bs = B.clone()
    Bs[5, 3] = float("nan")
    Bs[17, 0] = float("inf")
    Bs[18, :] = float("-inf")
    Bs[19, 0], Bs[19, 1] = float("inf"), float("-inf")
    As = A.clone()
    As[4, 0] = float("inf")
    ib = torch.tensor([5, 17, 18, 19, 0, 1, 2, 3, 4, 6], device=gpu)            # a short list: the NaN scores make the top k
    got = native.dot_topk(As, None, Bs, ib, 10)
    ref = _reference(As, None, Bs, ib, 10, None)
    torch.cuda.synchronize()
    assert torch.equal(got[2], ref[2]) and torch.equal(got[1], ref[1])
    nan = torch.isnan(ref[0])
    assert torch.equal(torch.isnan(got[0]), nan)
    assert torch.equal(got[0][~nan].view(torch.int32), ref[0][~nan].view(torch.int32))
    assert bool(nan.any())
    # every score NaN: all ranked last, by column
    An = A.clone()
    An[0, 0] = float("nan")
    got = native.dot_topk(An[:1], None, B, None, 10)
    assert torch.equal(got[1][0].cpu(), torch.arange(10, dtype=torch.int32)) and bool(torch.isnan(got[0]).all())


def test_dot_topk_refusals_launch_nothing(gpu):
    from deeprecommendation_amd import native
    lib = native.load_library()
    A = _rand(4, 64, 0, gpu)
    B = _rand(100, 64, 1, gpu)
    Bw = _rand(100, 300, 1, gpu)
    out_s = torch.full((4, 1100), 7.0, device=gpu)
    out_i = torch.full((4, 1100), 7, dtype=torch.int32, device=gpu)
    out_n = torch.full((4,), 7, dtype=torch.int32, device=gpu)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)
    st = torch.cuda.current_stream().cuda_stream
    cases = ((A, B, 64, 129, native.NCF_EUNSUPPORTED, b"fused limit"), (A, B, 64, 1024, native.NCF_EUNSUPPORTED, b"fused limit"),
             (Bw[:4], Bw, 300, 10, native.NCF_EUNSUPPORTED, b"width"), (A, B, 64, 0, native.NCF_EINVAL, b"k = 0"),
             (A, B, 64, 1025, native.NCF_EINVAL, b"k = 1025"))
    for ta, tb, D, k, code, what in cases:
        assert lib.ncf_dot_topk_workspace_bytes(4, 100, D, k) == 0
        rc = lib.ncf_dot_topk(ta.data_ptr(), ta.shape[0], ta.stride(0), tb.data_ptr(), tb.shape[0], tb.stride(0), None, None, 4, 100, D,
                              None, None, k, out_s.data_ptr(), out_i.data_ptr(), out_n.data_ptr(), ws.data_ptr(), ws.numel(), None, st)
        assert rc == code and what in lib.ncf_last_error()
    need = lib.ncf_dot_topk_workspace_bytes(4, 100, 64, 10)
    assert need > 0
    rc = lib.ncf_dot_topk(A.data_ptr(), 4, 64, B.data_ptr(), 100, 64, None, None, 4, 100, 64, None, None, 10, out_s.data_ptr(),
                          out_i.data_ptr(), out_n.data_ptr(), ws.data_ptr(), need - 1, None, st)
    assert rc == native.NCF_EWORKSPACE and b"workspace" in lib.ncf_last_error()
    torch.cuda.synchronize()
    assert bool((out_s == 7.0).all()) and bool((out_i == 7).all()) and bool((out_n == 7).all())
    with pytest.raises(native.NativeError) as e:
        native.dot_topk(A, None, B, None, 200)
    assert e.value.code == native.NCF_EUNSUPPORTED
    with pytest.raises(RuntimeError, match="GPU"):
        native.dot_topk(A.cpu(), None, B.cpu(), None, 10)


def test_dot_topk_bad_ids_set_the_flag(gpu):
    from deeprecommendation_amd import native
    A = _rand(10, 64, 0, gpu)
    B = _rand(500, 64, 1, gpu)
    native.check_oob(gpu)                                       # start clean
    native.dot_topk(A, torch.tensor([0, 10], device=gpu), B, None, 5)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.dot_topk(A, None, B, torch.tensor([3, -1, 2], device=gpu), 2)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.dot_topk(A, None, B, None, 5)
    native.check_oob(gpu)                                       # good ids leave it clear


def test_dot_topk_captures_into_a_graph(gpu):
    from deeprecommendation_amd import native
    A = _rand(100, 64, 11, gpu)
    B = _rand(30000, 64, 12, gpu)
    lists = [list(range(r, 30000, 97)) for r in range(100)]
    seen = _csr(lists, gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        native.dot_topk(A, None, B, None, 50, seen)               # warm-up outside the capture (library load, allocator)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = native.dot_topk(A, None, B, None, 50, seen)
    g.replay()
    torch.cuda.synchronize()
    ref = _reference(A, None, B, None, 50, seen)
    torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
