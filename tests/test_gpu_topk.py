"""GPU: ncf_topk_rows (native.topk_rows) equals the CPU statement of its ordering contract (test_topk_cpu.topk_oracle) exactly:
same ids, same score bits, same counts — single- and multi-tile rows, every k, ld > cols, heavy ties, NaN / +-inf / +-0,
exclusion lists; refusals are status codes; the call captures into a HIP graph."""
import numpy as np
import pytest
import torch

from test_topk_cpu import topk_oracle

pytestmark = pytest.mark.gpu


def _csr(lists, dev):
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64, device=dev)
    col = torch.tensor(np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if lists else np.zeros(0), dtype=torch.int32, device=dev)
    return rowptr, col


def _check(scores, k, seen_lists=None, gpu=None):
    from deeprecommendation_amd import native
    seen = None if seen_lists is None else _csr(seen_lists, scores.device)
    s, i, n = native.topk_rows(scores, k, seen)
    torch.cuda.synchronize()
    rs, ri, rn = topk_oracle(scores.cpu(), k, seen_lists)
    assert torch.equal(n.cpu().long(), rn)
    assert torch.equal(i.cpu().long(), ri)
    assert torch.equal(s.cpu().view(torch.int32), rs.view(torch.int32))      # bit-exact, NaN included


def _rand(rows, cols, seed, dev, ld=None):
    g = torch.Generator(device=dev).manual_seed(seed)
    if ld is None:
        return torch.randn(rows, cols, device=dev, generator=g)
    return torch.randn(rows, ld, device=dev, generator=g)[:, :cols]


@pytest.mark.parametrize("cols", [1, 100, 8191, 8192, 8193, 50000])
@pytest.mark.parametrize("k", [1, 10, 100, 1000, 1024])
def test_topk_random_rows(gpu, cols, k):
    _check(_rand(3, cols, cols * 7 + k, gpu), k)


@pytest.mark.parametrize("k", [1, 100, 1024])
def test_topk_long_row(gpu, k):
    """2^20 + 17 columns: 129 tiles, three (k = 100) to four (k = 1024) launches."""
    _check(_rand(1, (1 << 20) + 17, k, gpu), k)


def test_topk_k_above_cols_and_ld_above_cols(gpu):
    _check(_rand(4, 37, 1, gpu, ld=41), 100)
    _check(_rand(2, 20000, 2, gpu, ld=20003), 1000)      # rows not 16-byte aligned: the scalar load path
    base = _rand(1, 30001, 3, gpu)
    _check(base[:, 1:], 64)                               # a view starting one float in


@pytest.mark.parametrize("cols", [500, 8192, 70000])
@pytest.mark.parametrize("k", [10, 1000])
def test_topk_heavy_ties(gpu, cols, k):
    """Scores quantised to 8 values: the column tie rule decides almost every slot."""
    g = torch.Generator(device=gpu).manual_seed(cols + k)
    x = torch.randint(0, 8, (3, cols), device=gpu, generator=g).float() * 0.25 - 1.0
    _check(x, k)


def test_topk_special_values(gpu):
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(5)
    rows = []
    for C in (7, 300, 9000):
        pool = torch.tensor([nan, inf, -inf, 0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1e-45])
        rows.append(pool[torch.randint(0, len(pool), (C,), generator=g)])
    for r in rows:
        for k in (1, 5, 100, 1024):
            _check(r[None].to(gpu), k)
    allnan = torch.full((2, 20000), nan, device=gpu)
    _check(allnan, 1000)
    mixed = torch.randn(2, 20000, device=gpu)
    mixed[:, ::3] = nan
    mixed[:, 1::7] = -0.0
    mixed[:, 2::11] = 0.0
    mixed[0, 5] = -inf
    mixed[1, 19999] = inf
    _check(mixed, 1024)
    _check(torch.tensor([[-inf, nan, -inf, nan]], device=gpu), 4)


def test_topk_exclusion(gpu):
    rng = np.random.default_rng(9)
    for rows, cols, k in ((5, 300, 50), (4, 20000, 1000), (3, 100000, 100)):
        x = _rand(rows, cols, rows + cols, gpu)
        lists = [rng.integers(-5, cols + 5, int(rng.integers(0, 400))).tolist() for _ in range(rows)]
        lists[0] = []                                            # empty list
        lists[1] = list(range(cols)) + [3, 3, -1, cols]          # everything excluded (count 0), with duplicates / out of range
        _check(x, k, lists)
        lists[1] = list(range(0, cols, 2))                       # half of the row
        _check(x, k, lists)
    x = _rand(3, 1000, 11, gpu)
    _check(x, 10, [[], [], []])                                  # a CSR with no entries at all


def test_topk_exclusion_heavy_ties_multi_tile(gpu):
    g = torch.Generator(device=gpu).manual_seed(12)
    x = torch.randint(0, 4, (2, 40000), device=gpu, generator=g).float()
    lists = [list(range(0, 40000, 3)), list(range(17, 30000, 5))]
    _check(x, 1000, lists)


def test_topk_many_short_rows(gpu):
    """4096 x 3706: the evaluation shape (every user against the ML-1M catalogue), one workgroup per row."""
    from deeprecommendation_amd import native
    x = _rand(4096, 3706, 4, gpu)
    s, i, n = native.topk_rows(x, 100)
    ref_s, ref_i = torch.sort(x, dim=1, descending=True, stable=True)
    assert torch.equal(i.long(), ref_i[:, :100]) and torch.equal(s, ref_s[:, :100]) and bool((n == 100).all())


def test_topk_rows_processed_in_chunks(gpu):
    """Rows of 2^24 columns at k = 1024 need 18.9 MB of workspace each: 16 rows take two chunks of 13 and 3 (the workspace stays near 256 MB).
    Oracle: torch's stable sort on the device (no NaN in the data)."""
    from deeprecommendation_amd import native
    lib = native.load_library()
    R, C, k = 16, 1 << 24, 1024
    assert lib.ncf_topk_workspace_bytes(R, C, k) < R * lib.ncf_topk_workspace_bytes(1, C, k)
    c = torch.arange(C, device=gpu, dtype=torch.int64)
    x = torch.stack([((c * 2654435761 + r * 977) % 4099).float() for r in range(R)])    # ties of 4099 values
    s, i, n = native.topk_rows(x, k)
    for r in range(R):
        ref_s, ref_i = torch.sort(x[r], descending=True, stable=True)
        assert torch.equal(i[r].long(), ref_i[:k]) and torch.equal(s[r], ref_s[:k])
    assert bool((n == k).all())


def test_topk_refusals_launch_nothing(gpu):
    from deeprecommendation_amd import native
    lib = native.load_library()
    x = _rand(2, 100, 0, gpu)
    out_s = torch.full((2, 1100), 7.0, device=gpu)
    out_i = torch.full((2, 1100), 7, dtype=torch.int32, device=gpu)
    out_n = torch.full((2,), 7, dtype=torch.int32, device=gpu)
    st = torch.cuda.current_stream().cuda_stream
    for rows, cols, ld, k, what in ((2, 100, 100, 0, b"k = 0"), (2, 100, 100, 1025, b"k = 1025"), (2, (1 << 24) + 1, (1 << 24) + 1, 10, b"cols"),
                                    (65537, 100, 100, 10, b"rows"), (2, 100, 99, 10, b"ld")):
        rc = lib.ncf_topk_rows(x.data_ptr(), rows, cols, ld, None, None, k, out_s.data_ptr(), out_i.data_ptr(), out_n.data_ptr(), None, 0, st)
        assert rc != native.NCF_OK and what in lib.ncf_last_error()
    rc = lib.ncf_topk_rows(x.data_ptr(), 1, 20000, 20000, None, None, 10, out_s.data_ptr(), out_i.data_ptr(), out_n.data_ptr(), None, 0, st)
    assert rc == native.NCF_EWORKSPACE and b"workspace" in lib.ncf_last_error()
    torch.cuda.synchronize()
    assert bool((out_s == 7.0).all()) and bool((out_i == 7).all()) and bool((out_n == 7).all())
    with pytest.raises(native.NativeError, match="k = 2000"):
        native.topk_rows(x, 2000)
    with pytest.raises(RuntimeError, match="GPU"):
        native.topk_rows(x.cpu(), 10)


def test_topk_captures_into_a_graph(gpu):
    """No host synchronisation inside: the multi-tile call (workspace, two launches) captures and replays to the same result."""
    from deeprecommendation_amd import native
    x = _rand(8, 30000, 21, gpu)
    lists = [list(range(r, 30000, 97)) for r in range(8)]
    seen = _csr(lists, gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        native.topk_rows(x, 500, seen)                    # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = native.topk_rows(x, 500, seen)
    rs, ri, rn = topk_oracle(x.cpu(), 500, lists)
    for _ in range(2):
        for t in out:
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[1].cpu().long(), ri) and torch.equal(out[2].cpu().long(), rn)
        assert torch.equal(out[0].cpu().view(torch.int32), rs.view(torch.int32))
