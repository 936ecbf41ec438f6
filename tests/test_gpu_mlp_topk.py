"""GPU: ncf_mlp_topk (native.mlp_topk) equals score-then-select — native.topk_rows over native.score_fused's all-pairs score matrix —
bit for bit (scores, ids, counts): every fused MLP instance in both concat orders (user first: BasicNCF; item first: GraphNCF),
uneven splits, k up to the fused limit, one and many column tiles and ranges, one and thousands of users, with and without an item
id list, exclusion lists; exact ties, NaN / inf, a -0.0 output bias; refusals are status codes that launch nothing; bad ids set
the out-of-range flag; the call captures into a HIP graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INSTANCES = [(64, 256, 128), (64, 256, 0), (64, 128, 0), (64, 128, 64), (128, 256, 128), (128, 256, 0), (128, 128, 0),
             (128, 128, 64), (256, 256, 128), (256, 256, 0), (256, 128, 0)]


def _csr(lists, dev):
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64, device=dev)
    col = torch.tensor(np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]), dtype=torch.int32, device=dev)
    return rowptr, col


def _rand(rows, D, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(rows, D, device=dev, generator=g)


def _mlp(dims, seed, dev, dtype=torch.float32):
    """PackedMLP for dims [K0, N1, (N2,) 1] with weights at the scale of a trained model (fan-in scaled)."""
    from deeprecommendation_amd import native
    g = torch.Generator(device=dev).manual_seed(seed)
    W = [torch.randn(o, i, device=dev, generator=g) / i ** 0.5 for i, o in zip(dims[:-1], dims[1:])]
    b = [0.1 * torch.randn(o, device=dev, generator=g) for o in dims[1:]]
    return native.PackedMLP(W, b, dtype=dtype), W, b


def _dims(K0, N1, N2):
    return [K0, N1, N2, 1] if N2 else [K0, N1, 1]


def _reference(tA, iA, tB, iB, packed, k, seen, user_first):
    from deeprecommendation_amd import native
    a = iA if iA is not None else torch.arange(tA.shape[0], device=tA.device)
    b = iB if iB is not None else torch.arange(tB.shape[0], device=tA.device)
    if user_first:
        nu, ni = a.numel(), b.numel()
        s = native.score_fused(tA, a.repeat_interleave(ni), tB, b.repeat(nu), packed)
    else:
        nu, ni = b.numel(), a.numel()
        s = native.score_fused(tA, a.repeat(nu), tB, b.repeat_interleave(ni), packed)
    return native.topk_rows(s.view(nu, ni), k, seen)


def _check(tA, iA, tB, iB, packed, k, seen=None, user_first=True):
    from deeprecommendation_amd import native
    got = native.mlp_topk(tA, iA, tB, iB, packed, k, seen, user_first=user_first)
    ref = _reference(tA, iA, tB, iB, packed, k, seen, user_first)
    torch.cuda.synchronize()
    assert torch.equal(got[2], ref[2])
    assert torch.equal(got[1], ref[1])
    nan = torch.isnan(ref[0])
    assert torch.equal(torch.isnan(got[0]), nan)
    assert torch.equal(got[0][~nan].view(torch.int32), ref[0][~nan].view(torch.int32))
    return got


@pytest.mark.parametrize("user_first", [True, False])
@pytest.mark.parametrize("inst", INSTANCES)
def test_mlp_topk_every_instance(gpu, inst, user_first):
    K0, N1, N2 = inst
    packed, _, _ = _mlp(_dims(K0, N1, N2), K0 + N1 + N2, gpu)
    E = K0 // 2
    k = [1, 10, 100, 128][INSTANCES.index(inst) % 4]
    g = torch.Generator(device=gpu).manual_seed(K0 * N1 + N2)
    if user_first:                                   # A = users, B = items
        tA, tB = _rand(150, E, 1, gpu), _rand(5000, E, 2, gpu)
        users = torch.randint(0, 150, (70,), device=gpu, generator=g)
        _check(tA, users, tB, None, packed, k, user_first=True)
        items = torch.randint(0, 5000, (3000,), device=gpu, generator=g)   # an id list with repeats
        _check(tA, users, tB, items, packed, k, user_first=True)
    else:                                            # A = items, B = users
        tA, tB = _rand(5000, E, 3, gpu), _rand(150, E, 4, gpu)
        users = torch.randint(0, 150, (70,), device=gpu, generator=g)
        _check(tA, None, tB, users, packed, k, user_first=False)
        items = torch.randint(0, 5000, (3000,), device=gpu, generator=g)
        _check(tA, items, tB, users, packed, k, user_first=False)


@pytest.mark.parametrize("EA,EB", [(32, 96), (96, 32), (8, 120), (120, 8)])
@pytest.mark.parametrize("user_first", [True, False])
def test_mlp_topk_uneven_split(gpu, EA, EB, user_first):
    packed, _, _ = _mlp([128, 256, 128, 1], EA, gpu)
    tA, tB = _rand(3000, EA, EA, gpu), _rand(3000, EB, EB + 1, gpu)
    users = torch.randint(0, 3000, (40,), device=gpu)
    if user_first:
        _check(tA, users, tB, None, packed, 50, user_first=True)
    else:
        _check(tA, None, tB, users, packed, 50, user_first=False)


@pytest.mark.parametrize("k", [1, 10, 100, 128])
@pytest.mark.parametrize("user_first", [True, False])
def test_mlp_topk_k(gpu, k, user_first):
    packed, _, _ = _mlp([128, 256, 128, 1], k, gpu)
    U, I = _rand(300, 64, 5, gpu), _rand(20000, 64, 6, gpu)
    users = torch.randint(0, 300, (130,), device=gpu)
    if user_first:
        _check(U, users, I, None, packed, k, user_first=True)
    else:
        _check(I, None, U, users, packed, k, user_first=False)


@pytest.mark.parametrize("cols", [1, 31, 32, 33, 2049, 8193, 65536])
@pytest.mark.parametrize("n_users", [1, 2000])
def test_mlp_topk_column_ranges(gpu, cols, n_users):
    """One user (the column range shrinks to a single 32-column tile per wave) and thousands (8192-column ranges, several merge
    levels), in both orders."""
    packed, _, _ = _mlp([128, 256, 128, 1], 7, gpu)
    U, I = _rand(n_users, 64, cols, gpu), _rand(cols, 64, cols + 1, gpu)
    _check(U, None, I, None, packed, 100, user_first=True)
    if n_users == 1 or cols <= 8193:
        _check(I, None, U, None, packed, 10, user_first=False)


def test_mlp_topk_exclusion(gpu):
    I, k = 20000, 100
    packed, _, _ = _mlp([128, 256, 128, 1], 8, gpu)
    U, T = _rand(6, 64, 3, gpu), _rand(I, 64, 4, gpu)
    rng = np.random.default_rng(0)
    lists = [[],                                                   # nothing excluded
             list(range(0, I, 3)),                                 # a third of the columns
             list(range(I)),                                       # everything: count 0
             [c for c in range(I) if c % 4000 != 7],               # all but 5 columns: count 5 < k
             rng.integers(0, I, 5000).tolist() + [-1, I, I + 50],  # unsorted, duplicates, ids outside the list
             rng.permutation(I)[:15000].tolist()]
    seen = _csr(lists, gpu)
    for user_first in (True, False):
        tA, tB = (U, T) if user_first else (T, U)
        s, i, n = _check(tA, None, tB, None, packed, k, seen, user_first=user_first)
        n = n.cpu()
        assert n[2] == 0 and n[3] == 5 and n[0] == k
        assert bool((i[2] == -1).all()) and bool(torch.isneginf(s[2]).all())
        assert bool((i[3, 5:] == -1).all()) and bool(torch.isneginf(s[3, 5:]).all())
    ib = torch.randint(0, I, (I // 2,), device=gpu)
    seen2 = _csr([x[: I // 4] for x in lists], gpu)
    _check(U, None, T, ib, packed, k, seen2, user_first=True)
    _check(T, ib, U, None, packed, k, seen2, user_first=False)


def test_mlp_topk_ties_and_specials(gpu):
    from deeprecommendation_amd import native
    packed, _, _ = _mlp([128, 256, 128, 1], 9, gpu)
    D, I = 64, 10000
    base = _rand(40, D, 7, gpu)
    T = base[torch.randint(0, 40, (I,), device=gpu)].contiguous()             # duplicated item rows: exact ties, lower column first
    U = _rand(20, D, 8, gpu)
    _check(U, None, T, None, packed, 100, user_first=True)
    _check(T, None, U, None, packed, 100, user_first=False)
    Ti = torch.randint(-3, 4, (I, D), device=gpu).float()                     # small integers: heavy ties
    Ui = torch.randint(-3, 4, (20, D), device=gpu).float()
    _check(Ui, None, Ti, None, packed, 128, user_first=True)
    # NaN / inf in either table (the ReLUs turn most of them into finite scores; what is left is compared as NaN)
    Ts = T.clone()
    Ts[5, 3] = float("nan")
    Ts[17, 0] = float("inf")
    Ts[18, :] = float("-inf")
    Ts[19, 0], Ts[19, 1] = float("inf"), float("-inf")
    Us = U.clone()
    Us[4, 0] = float("inf")
    Us[6, 2] = float("nan")
    ib = torch.tensor([5, 17, 18, 19, 0, 1, 2, 3, 4, 6], device=gpu)
    for user_first in (True, False):
        tA, iA, tB, iB = (Us, None, Ts, ib) if user_first else (Ts, ib, Us, None)
        _check(tA, iA, tB, iB, packed, 10, user_first=user_first)
        _check(tA, None, tB, None, packed, 100, user_first=user_first)
    # a NaN last-layer weight makes every score NaN: all ranked last, by column
    dims = [128, 256, 128, 1]
    _, W, b = _mlp(dims, 9, gpu)
    W[-1][0, 5] = float("nan")
    nanp = native.PackedMLP(W, b)
    for user_first in (True, False):
        tA, tB = (U, T) if user_first else (T, U)
        got = _check(tA, None, tB, None, nanp, 10, user_first=user_first)
        assert torch.equal(got[1][0].cpu(), torch.arange(10, dtype=torch.int32)) and bool(torch.isnan(got[0]).all())


def test_mlp_topk_negative_zero_bias(gpu):
    """Zeroed last-layer weights and a -0.0 last bias: every fused score is +0 + -0 = +0, and so is every recovered score."""
    from deeprecommendation_amd import native
    dims = [128, 256, 128, 1]
    g = torch.Generator(device=gpu).manual_seed(3)
    W = [torch.randn(o, i, device=gpu, generator=g) / i ** 0.5 for i, o in zip(dims[:-1], dims[1:])]
    b = [torch.randn(o, device=gpu, generator=g) for o in dims[1:]]
    W[-1].zero_()
    b[-1].fill_(-0.0)
    packed = native.PackedMLP(W, b)
    U, T = _rand(9, 64, 1, gpu), _rand(3000, 64, 2, gpu)
    for user_first in (True, False):
        tA, tB = (U, T) if user_first else (T, U)
        s, i, _ = _check(tA, None, tB, None, packed, 20, user_first=user_first)
        assert bool((s.view(torch.int32) == 0).all())
        assert torch.equal(i[0].cpu(), torch.arange(20, dtype=torch.int32))


def test_mlp_topk_bad_ids_set_the_flag(gpu):
    from deeprecommendation_amd import native
    packed, _, _ = _mlp([128, 256, 128, 1], 10, gpu)
    U, T = _rand(10, 64, 0, gpu), _rand(500, 64, 1, gpu)
    native.check_oob(gpu)                                       # start clean
    for user_first in (True, False):
        tA, tB = (U, T) if user_first else (T, U)
        bad_u = torch.tensor([0, 10, -1], device=gpu)
        bad_i = torch.tensor([3, -1, 2, 500], device=gpu)
        args = (tA, bad_u, tB, None) if user_first else (tA, None, tB, bad_u)
        _check(*args, packed, 5, user_first=user_first)          # bad rows read as zero rows, like the fused scorer
        with pytest.raises(IndexError):
            native.check_oob(gpu)
        args = (tA, None, tB, bad_i) if user_first else (tA, bad_i, tB, None)
        _check(*args, packed, 2, user_first=user_first)
        with pytest.raises(IndexError):
            native.check_oob(gpu)
        native.mlp_topk(tA, None, tB, None, packed, 5, user_first=user_first)
        torch.cuda.synchronize()
        native.check_oob(gpu)                                   # good ids leave it clear
        # without the reference's score_fused call: only the prefix pass reads the first part's ids, so the flag is its own
        native.mlp_topk(tA, bad_u if user_first else bad_i, tB, None, packed, 2, user_first=user_first)
        with pytest.raises(IndexError):
            native.check_oob(gpu)


def test_mlp_topk_refusals_launch_nothing(gpu):
    from deeprecommendation_amd import native
    lib = native.load_library()
    U, T = _rand(4, 64, 0, gpu), _rand(100, 64, 1, gpu)
    packed, _, _ = _mlp([128, 256, 128, 1], 11, gpu)
    odd, _, _ = _mlp([128, 64, 1], 12, gpu)                   # N1 = 64: no fused instance
    out_s = torch.full((4, 1100), 7.0, device=gpu)
    out_i = torch.full((4, 1100), 7, dtype=torch.int32, device=gpu)
    out_n = torch.full((4,), 7, dtype=torch.int32, device=gpu)
    ws = torch.zeros(1 << 24, dtype=torch.uint8, device=gpu)
    st = torch.cuda.current_stream().cuda_stream

    def call(pk, k, dt=native.NCF_F32, ws_bytes=ws.numel()):
        return lib.ncf_mlp_topk(dt, U.data_ptr(), 4, 64, T.data_ptr(), 100, 64, 64, 64, 1, None, None, 4, 100, pk.n_layers,
                                native._dims_array(pk.dims), pk.blob.data_ptr(), None, None, k, out_s.data_ptr(), out_i.data_ptr(),
                                out_n.data_ptr(), ws.data_ptr(), ws_bytes, None, st)

    cases = ((packed, 129, native.NCF_F32, native.NCF_EUNSUPPORTED, b"fused limit"),
             (packed, 1024, native.NCF_F32, native.NCF_EUNSUPPORTED, b"fused limit"),
             (odd, 10, native.NCF_F32, native.NCF_EUNSUPPORTED, b"no fused instance"),
             (packed, 10, native.NCF_BF16, native.NCF_EUNSUPPORTED, b"no fused instance"),
             (packed, 0, native.NCF_F32, native.NCF_EINVAL, b"k = 0"),
             (packed, 1025, native.NCF_F32, native.NCF_EINVAL, b"k = 1025"))
    for pk, k, dt, code, what in cases:
        rc = call(pk, k, dt)
        assert rc == code and what in lib.ncf_last_error(), (k, dt, rc, lib.ncf_last_error())
    need = lib.ncf_mlp_topk_workspace_bytes(4, 100, 1, 3, native._dims_array(packed.dims), 10)
    assert need > 0
    assert call(packed, 10, ws_bytes=need - 1) == native.NCF_EWORKSPACE and b"workspace" in lib.ncf_last_error()
    torch.cuda.synchronize()
    assert bool((out_s == 7.0).all()) and bool((out_i == 7).all()) and bool((out_n == 7).all())
    for args in ((U, None, T, None, packed, 129), (U, None, T, None, odd, 10)):
        with pytest.raises(native.NativeError) as e:
            native.mlp_topk(*args)
        assert e.value.code == native.NCF_EUNSUPPORTED
    bf, _, _ = _mlp([128, 256, 128, 1], 13, gpu, dtype=torch.bfloat16)
    with pytest.raises(native.NativeError) as e:
        native.mlp_topk(U.bfloat16(), None, T.bfloat16(), None, bf, 10)
    assert e.value.code == native.NCF_EUNSUPPORTED
    with pytest.raises(RuntimeError, match="GPU"):
        native.mlp_topk(U.cpu(), None, T.cpu(), None, packed, 10)


def test_mlp_topk_captures_into_a_graph(gpu):
    from deeprecommendation_amd import native
    packed, _, _ = _mlp([128, 256, 128, 1], 14, gpu)
    U, T = _rand(100, 64, 11, gpu), _rand(30000, 64, 12, gpu)
    users = torch.randint(0, 100, (100,), device=gpu)
    seen = _csr([list(range(r, 30000, 97)) for r in range(100)], gpu)
    for user_first in (True, False):
        args = (U, users, T, None) if user_first else (T, None, U, users)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            native.mlp_topk(*args, packed, 50, seen, user_first=user_first)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = native.mlp_topk(*args, packed, 50, seen, user_first=user_first)
        g.replay()
        torch.cuda.synchronize()
        ref = _reference(*args, packed, 50, seen, user_first)
        torch.cuda.synchronize()
        for a, b in zip(out, ref):
            assert torch.equal(a, b)
