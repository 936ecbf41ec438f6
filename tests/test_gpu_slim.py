"""GPU tests of the SLIM baseline against tests/slim_ref.py.  ncf_slim_solve holds no reduction over floats, so everything here is bit
for bit: the weights, the sweep and step counts and the last sweep's largest move, on the five shared cases (both workgroup sizes,
signed weights, a catalogue of several screening blocks), in pieces and in reverse, capped, warm, with q above 64 KiB of LDS and at
the largest catalogue; then the bounds, the entry's refusals, the model, the ranking front ends, a planted structure and
tools/slim_baseline.py.  Every case's restatement converges under its cap (tests/test_slim_cpu.py asserts it, and _case does again),
so no cap hides a column."""
import ctypes

import numpy as np
import pytest
import torch

import ease_ref as E
import slim_ref as S

pytestmark = pytest.mark.gpu
SENTINEL = 7.25


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _dev(arrays, gpu):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays)


def _padded(gpu, M, pad):
    """M on the device inside rows of len + pad floats; returns (the view, the buffer)."""
    M = torch.as_tensor(M)
    buf = torch.full((M.shape[0], M.shape[1] + pad), SENTINEL, dtype=torch.float32, device=gpu)
    buf[:, :M.shape[1]] = M.to(gpu)
    return buf[:, :M.shape[1]], buf


def _solve(gpu, G, lists, l1, l2, positive=True, max_sweeps=S.CAP, tol=S.TOL, Wt0=None):
    """native.slim_solve of the column lists ``lists``, one call each, into ONE output whose rows are 5 floats longer than I and
    start as SENTINEL (or as the rows ``Wt0``, for a warm start); G too sits in padded rows.  Checks that the padding and every row
    that was not listed are untouched.  Returns (Wt numpy (I, I), sweeps, steps, last) with the per-column outputs concatenated."""
    from deeprecommendation_amd import native
    I = len(G)
    Gd, _ = _padded(gpu, G, 3)
    start = np.full((I, I), SENTINEL, np.float32) if Wt0 is None else Wt0
    Wt, buf = _padded(gpu, start, 5)
    outs = []
    for cols in lists:
        c = torch.tensor(list(cols), dtype=torch.int32, device=gpu)
        out, sweeps, steps, last = native.slim_solve(Gd, l1, l2, c, positive, Wt0 is not None, max_sweeps, tol, out=Wt)
        assert out.data_ptr() == buf.data_ptr()
        outs.append((sweeps, steps, last))
    assert bool((buf[:, I:] == SENTINEL).all())
    got = Wt.cpu().numpy()
    listed = sorted({int(j) for cols in lists for j in cols if 0 <= j < I})
    rest = np.setdiff1d(np.arange(I), listed)
    assert _same(got[rest], start[rest])
    return (got,) + tuple(torch.cat([o[k] for o in outs]).cpu().numpy() for k in range(3))


def _case(name):
    s = S.solved(name)
    assert (s["last"] <= S.TOL).all() and s["sweeps"].max() < s["cap"]    # the restatement first: every listed column converged
    return s


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name", ["A", "B", "C", "S", "W"])
def test_solve_matches_the_restatement_bit_for_bit_whole_in_pieces_and_reversed(gpu, name):
    from deeprecommendation_amd import native
    s = _case(name)
    cols = s["cols"]
    args = (s["l1"], s["l2"], s["positive"], s["cap"])
    half = len(cols) // 2 + 1
    for lists in ([cols], [cols[:half], cols[half:]], [cols[::-1]]):
        Wt, sweeps, steps, last = _solve(gpu, s["G"], lists, *args)
        order = np.concatenate(lists)
        pos = {int(j): c for c, j in enumerate(cols)}
        at = np.array([pos[int(j)] for j in order])
        assert _same(Wt[order], s["W"][at])
        assert _same(sweeps, s["sweeps"][at]) and _same(steps, s["steps"][at]) and _same(last, s["last"][at])
    assert (s["W"] < 0).any() == (name == "S")
    native.check_oob(gpu)


def test_a_solve_repeats_its_bits_and_the_default_list_is_every_column(gpu):
    from deeprecommendation_amd import native
    s = _case("A")
    Gd = torch.from_numpy(s["G"]).to(gpu)
    a = native.slim_solve(Gd, s["l1"], s["l2"], max_sweeps=s["cap"])
    b = native.slim_solve(Gd, s["l1"], s["l2"], max_sweeps=s["cap"])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert _same(a[0], s["W"]) and _same(a[1], s["sweeps"]) and _same(a[2], s["steps"]) and _same(a[3], s["last"])
    sub = native.slim_solve(Gd, s["l1"], s["l2"], torch.tensor([5, 2], dtype=torch.int32, device=gpu), max_sweeps=s["cap"])[0]
    want = np.zeros_like(s["W"])                                          # rows that are not listed: zeros in a tensor allocated there
    want[[5, 2]] = s["W"][[5, 2]]
    assert _same(sub, want)
    c = _solve(gpu, s["G"], [s["cols"]], s["l1"], s["l2"], True, s["cap"])
    d = _solve(gpu, s["G"], [s["cols"]], s["l1"], s["l2"], True, s["cap"])
    assert all(_same(x, y) for x, y in zip(c, d))


# ------------------------------------------------------------------ 2. the cap
def test_a_capped_solve_is_the_restatement_at_that_sweep_and_says_so(gpu):
    _, _, G = S.gram("B")
    cols = tuple(range(0, 257, 4))
    l1, l2 = S.CASES["B"][1]
    want = S.solve(G, cols, l1, l2, max_sweeps=5)
    assert (want[1] == 5).all() and (want[3] > S.TOL).all()               # measured: all 65 columns are unconverged after 5 sweeps
    Wt, sweeps, steps, last = _solve(gpu, G, [cols], l1, l2, True, 5)
    assert _same(Wt[list(cols)], want[0]) and _same(sweeps, want[1]) and _same(steps, want[2]) and _same(last, want[3])
    assert (last > S.TOL).all()
    one = _solve(gpu, G, [cols[:3]], l1, l2, True, 1)
    ref = S.solve(G, cols[:3], l1, l2, max_sweeps=1)
    assert _same(one[0][list(cols[:3])], ref[0]) and _same(one[1], ref[1]) and _same(one[3], ref[3])


# ------------------------------------------------------------------ 3. warm start
def test_a_warm_solve_is_the_restatements_warm_run_and_from_zeros_the_cold_one(gpu):
    _, I, G = S.gram("B")
    cols = tuple(range(0, 257, 4))
    l1, l2 = S.CASES["B"][1]
    first = S.solve(G, cols, 2 * l1, l2)
    assert (first[3] <= S.TOL).all()
    Wt0 = np.full((I, I), SENTINEL, np.float32)
    Wt0[list(cols)] = first[0]
    Wt0[4, 4] = 3.0                                                       # a warm row's own coordinate is read as +0.0
    want = S.solve(G, cols, l1, l2, Wt0=Wt0)
    cold = S.solve(G, cols, l1, l2)
    assert (want[3] <= S.TOL).all() and want[1].sum() < cold[1].sum() and not _same(want[0], cold[0])
    Wt, sweeps, steps, last = _solve(gpu, G, [cols], l1, l2, Wt0=Wt0)
    assert _same(Wt[list(cols)], want[0]) and _same(sweeps, want[1]) and _same(steps, want[2]) and _same(last, want[3])
    zeros = np.full((I, I), SENTINEL, np.float32)
    zeros[list(cols)] = 0.0
    Wt, sweeps, steps, last = _solve(gpu, G, [cols], l1, l2, Wt0=zeros)
    assert _same(Wt[list(cols)], cold[0]) and _same(sweeps, cold[1]) and _same(steps, cold[2]) and _same(last, cold[3])


# ------------------------------------------------------------------ 4. LDS above 64 KiB, and the largest catalogue
def test_q_above_64_kib_of_lds_gives_the_small_cases_rows_followed_by_zeros(gpu):
    """Case C's Gram matrix in the top-left of an I = 16 448 matrix that is zero elsewhere except a diagonal of 1.0: a coordinate
    >= 600 sees rho = 0 exactly, so the 16 listed columns are case C's rows followed by zeros, with its sweeps and steps."""
    from deeprecommendation_amd import native
    s = _case("C")
    I, n = 16448, s["I"]
    assert 4 * I > 64 * 1024
    G = torch.zeros((I, I), dtype=torch.float32, device=gpu)
    G.diagonal().fill_(1.0)
    G[:n, :n] = torch.from_numpy(s["G"]).to(gpu)
    at = np.arange(16)
    cols = torch.from_numpy(s["cols"][at]).to(gpu)
    Wt = torch.full((I, I), SENTINEL, dtype=torch.float32, device=gpu)
    out, sweeps, steps, last = native.slim_solve(G, s["l1"], s["l2"], cols, max_sweeps=s["cap"], out=Wt)
    rows = out[cols.to(torch.int64)]
    assert _same(rows[:, :n], s["W"][at]) and not bool(rows[:, n:].any()) and not bool(torch.signbit(rows[:, n:]).any())
    assert _same(sweeps, s["sweeps"][at]) and _same(steps, s["steps"][at]) and _same(last, s["last"][at])
    assert bool((out[1] == SENTINEL).all()) and bool((out[I - 1] == SENTINEL).all())
    native.check_oob(gpu)


def _lib():
    from deeprecommendation_amd import native
    return native, native.load_library()


def _entry(lib, native, G, I, ldg, cols, n, l1, l2, positive, warm, max_sweeps, tol, Wt, ldw, sweeps, steps, last, flag, like):
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
    return lib.ncf_slim_solve(ptr(G), I, ldg, ptr(cols), n, l1, l2, positive, warm, max_sweeps, tol, ptr(Wt), ldw, ptr(sweeps), ptr(steps),
                              ptr(last), ptr(flag), native._stream(like))


def test_the_largest_catalogue_runs_and_one_item_more_is_refused(gpu):
    """NCF_SLIM_MAX_ITEMS items: q fills 128 KiB of LDS.  Both calls get buffers of the sizes they claim.  The matrix is 2 on the
    diagonal with G[0][1] = G[1][0] = 1 and (l1, l2) = (0.25, 0): column 0 is w[1] = (1 - 0.25) / 2 after one step and two sweeps."""
    native, lib = _lib()
    N = native.SLIM_MAX_ITEMS
    G = torch.zeros((N + 1, N + 1), dtype=torch.float32, device=gpu)
    G.diagonal().fill_(2.0)
    G[0, 1] = G[1, 0] = 1.0
    Wt = torch.empty((N + 1, N + 1), dtype=torch.float32, device=gpu)
    Wt[0].fill_(SENTINEL)
    cols = torch.tensor([0, N - 1], dtype=torch.int32, device=gpu)
    out, sweeps, steps, last = native.slim_solve(G[:N, :N], 0.25, 0.0, cols, out=Wt[:N, :N])
    want = S.solve(G[:4, :4].cpu().numpy(), [0, 3], 0.25, 0.0)
    assert sweeps.tolist() == want[1].tolist() == [2, 1] and steps.tolist() == want[2].tolist() == [1, 0]
    assert _same(last, want[3]) and _same(out[0, :4], want[0][0]) and float(out[0, 1]) == 0.375
    assert not bool(out[0, 4:].any()) and not bool(out[N - 1].any()) and float(Wt[0, N]) == SENTINEL
    per = [torch.zeros(2, dtype=dt, device=gpu) for dt in (torch.int32, torch.int32, torch.float32)]
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    rc = _entry(lib, native, G, N + 1, N + 1, cols, 2, 0.25, 0.0, 1, 0, 100, 1e-4, Wt, N + 1, *per, flag, G)
    assert rc == native.NCF_EUNSUPPORTED
    msg = lib.ncf_last_error().decode()
    assert msg.startswith("ncf_slim_solve: ") and str(N + 1) in msg and str(N) in msg
    with pytest.raises(ValueError, match=f"^slim_solve: {N + 1} items"):
        native.slim_solve(G, 0.25, 0.0)
    torch.cuda.synchronize()
    assert int(flag) == 0 and not any(bool(p.any()) for p in per)         # refused before any launch


# ------------------------------------------------------------------ 5. bounds and repeated columns
def test_a_column_outside_the_items_is_flagged_and_skipped_and_a_repeated_one_reports_twice(gpu):
    from deeprecommendation_amd import native
    s = _case("A")
    I = s["I"]
    native.check_oob(gpu)
    lists = [[-1, 3, I, 5, 3, 5, 3]]
    Wt, sweeps, steps, last = _solve(gpu, s["G"], lists, s["l1"], s["l2"], True, s["cap"])    # also: every other row is untouched
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.check_oob(gpu)                                                # raised once, then cleared
    at = np.array([3, 5, 3, 5, 3])
    good = np.array([1, 3, 4, 5, 6])
    assert _same(Wt[[3, 5]], s["W"][[3, 5]])
    assert _same(sweeps[good], s["sweeps"][at]) and _same(steps[good], s["steps"][at]) and _same(last[good], s["last"][at])
    assert sweeps[[0, 2]].tolist() == [0, 0] and steps[[0, 2]].tolist() == [0, 0] and _same(last[[0, 2]], np.zeros(2, np.float32))


# ------------------------------------------------------------------ 6. the entry's refusals
def test_the_entry_refuses_before_any_launch_with_its_name_in_the_message(gpu):
    native, lib = _lib()
    I, n = 8, 2
    G = torch.eye(I, device=gpu) * 2
    Wt = torch.full((I, I), SENTINEL, device=gpu)
    cols = torch.tensor([0, 1], dtype=torch.int32, device=gpu)
    per = [torch.full((n,), 77, dtype=dt, device=gpu) for dt in (torch.int32, torch.int32, torch.float32)]
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    base = dict(G=G, I=I, ldg=I, cols=cols, n=n, l1=1.0, l2=1.0, positive=1, warm=0, max_sweeps=10, tol=1e-4, Wt=Wt, ldw=I,
                sweeps=per[0], steps=per[1], last=per[2], flag=flag)
    nan, inf = float("nan"), float("inf")
    refusals = [(dict(I=-1), "negative size"), (dict(n=-1), "negative size"), (dict(ldg=I - 1), "ldg"), (dict(ldw=I - 1), "ldw"),
                (dict(l1=-1.0), "l1"), (dict(l1=nan), "l1"), (dict(l2=-0.5), "l2"), (dict(l2=inf), "l2"), (dict(tol=-1e-3), "tol"),
                (dict(tol=nan), "tol"), (dict(max_sweeps=0), "max_sweeps"), (dict(G=G.data_ptr() + 2), "misaligned"),
                (dict(cols=cols.data_ptr() + 1), "misaligned"), (dict(Wt=Wt.data_ptr() + 2), "misaligned"),
                (dict(last=per[2].data_ptr() + 2), "misaligned"), (dict(G=None), "null"), (dict(cols=None), "null"),
                (dict(Wt=None), "null"), (dict(sweeps=None), "null"), (dict(steps=None), "null"), (dict(last=None), "null")]
    for change, text in refusals:
        rc = _entry(lib, native, like=G, **{**base, **change})
        msg = lib.ncf_last_error().decode()
        assert rc == native.NCF_EINVAL, (change, rc, msg)
        assert msg.startswith("ncf_slim_solve: ") and text in msg, (change, msg)
    assert _entry(lib, native, like=G, **{**base, "n": 0}) == native.NCF_OK
    torch.cuda.synchronize()
    assert bool((Wt == SENTINEL).all()) and all(bool((p == 77).all()) for p in per) and int(flag) == 0      # nothing was launched
    assert _entry(lib, native, like=G, **{**base, "flag": None}) == native.NCF_OK                           # the flag is optional
    torch.cuda.synchronize()
    assert per[0].tolist() == [1, 1] and per[1].tolist() == [0, 0] and not bool(Wt[:2].any()) and bool((Wt[2:] == SENTINEL).all())


# ------------------------------------------------------------------ 7. the model
def test_fit_is_the_restatement_transposed_from_a_csr_from_samples_and_on_a_grid(gpu):
    import deeprecommendation_amd as pkg
    s = _case("A")
    I, (rowptr, col, val) = s["I"], s["csr"]
    d = _dev(s["csr"], gpu)
    m = pkg.SLIM(s["l1"], s["l2"], max_sweeps=s["cap"]).fit_csr(*d, I)
    assert m.num_items_ == I and m.weights_.is_contiguous()
    assert _same(m.weights_, np.ascontiguousarray(s["W"].T))              # weights_[i][j] = column j's weight of source item i
    assert _same(m.sweeps_, s["sweeps"]) and _same(m.steps_, s["steps"]) and _same(m.last_delta_, s["last"])
    assert m.n_unconverged_ == 0 and m.density_ == np.count_nonzero(s["W"]) / I ** 2 and 0.1 < m.density_ < 0.5
    us = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    perm = np.random.default_rng(5).permutation(len(us))
    u, i, r = _dev((us[perm], col.astype(np.int64)[perm], val[perm]), gpu)
    f = pkg.SLIM(s["l1"], s["l2"], max_sweeps=s["cap"]).fit(u, i, r, len(rowptr) - 1, I, block_bytes=4 * I * 10)
    assert torch.equal(f.weights_, m.weights_) and torch.equal(f.sweeps_, m.sweeps_)
    grid = [(2 * s["l1"], s["l2"]), (s["l1"], s["l2"])]
    cold = pkg.SLIM(9.0, 9.0, max_sweeps=s["cap"]).fit_csr(*d, I, at_regs=grid)
    assert [(g.l1_reg, g.l2_reg, g.max_sweeps) for g in cold] == [(2.0, 5.0, s["cap"]), (1.0, 5.0, s["cap"])]
    assert torch.equal(cold[1].weights_, m.weights_) and torch.equal(cold[1].steps_, m.steps_)
    single = pkg.SLIM(*grid[0], max_sweeps=s["cap"]).fit_csr(*d, I)
    assert torch.equal(cold[0].weights_, single.weights_) and not torch.equal(cold[0].weights_, m.weights_)
    warm = pkg.SLIM(9.0, 9.0, max_sweeps=s["cap"]).fit_csr(*d, I, at_regs=grid, warm_path=True)
    assert torch.equal(warm[0].weights_, single.weights_)                 # the first point of a path is a cold fit
    want = S.solve(s["G"], s["cols"], s["l1"], s["l2"], Wt0=single.weights_.t().cpu().numpy(), max_sweeps=s["cap"])
    assert _same(warm[1].weights_, np.ascontiguousarray(want[0].T)) and _same(warm[1].sweeps_, want[1])
    assert int(warm[1].sweeps_.sum()) < int(m.sweeps_.sum())
    capped = pkg.SLIM(s["l1"], s["l2"], max_sweeps=3).fit_csr(*d, I)      # no error: the model counts its unconverged columns
    assert capped.n_unconverged_ == int((S.solve(s["G"], s["cols"], s["l1"], s["l2"], max_sweeps=3)[3] > S.TOL).sum()) > 0
    b = pkg.SLIM(s["l1"], s["l2"], max_sweeps=s["cap"], binary=True).fit_csr(d[0], d[1], d[2] * 3, I)
    assert torch.equal(b.weights_, m.weights_)                            # case A's values are ones already
    users = torch.tensor([0, 7, 399, 7], device=gpu)
    W = m.weights_.cpu().numpy()
    want = E.scores_ref(*s["csr"], users.tolist(), W)
    assert _same(m.scores(d, users), want) and np.abs(want).max() > 0
    assert torch.equal(b.scores((d[0], d[1], d[2] * 3), users), m.scores(d, users))
    items = torch.tensor([5, 0, 95, 40], device=gpu)
    assert _same(m.predict(d, users, items), E.predict_ref(*s["csr"], users.tolist(), items.tolist(), W))
    m.check()


def test_a_row_that_does_not_ascend_raises_what_ease_raises(gpu):
    import deeprecommendation_amd as pkg
    s = _case("A")
    rowptr, col, val = (a.copy() for a in s["csr"])
    u = int(np.argmax(np.diff(rowptr)))
    b = rowptr[u]
    col[b], col[b + 1] = col[b + 1], col[b]
    with pytest.raises(ValueError, match="^EASE: .*ascending"):
        pkg.SLIM(1.0, 5.0, max_sweeps=2).fit_csr(*_dev((rowptr, col, val), gpu), s["I"])
    pkg.SLIM(1.0, 5.0, max_sweeps=2).fit_csr(*_dev(s["csr"], gpu), s["I"])   # raised once, then cleared


# ------------------------------------------------------------------ 8. ranking
def test_front_ends_are_topk_and_rank_rows_over_the_scores_and_eases_are_unchanged(gpu):
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd import native
    from types import SimpleNamespace
    s = _case("A")
    I = s["I"]
    d = _dev(s["csr"], gpu)
    users = torch.arange(40, device=gpu)
    k = 7
    exclude = pkg.rated_exclusion(SimpleNamespace(rowptr=d[0], col=d[1]), users)
    targets = (torch.arange(0, 81, 2, device=gpu), torch.arange(80, device=gpu, dtype=torch.int32) * 3 % I)
    ease = pkg.EASE(reg=5.0).fit_csr(*d, I)
    slim = pkg.SLIM(s["l1"], s["l2"], max_sweeps=s["cap"]).fit_csr(*d, I)
    assert not torch.equal(ease.weights_, slim.weights_)
    for m, top_k, ranks in ((slim, pkg.slim_top_k, pkg.slim_ranks), (ease, pkg.ease_top_k, pkg.ease_ranks)):
        scores = m.scores(d, users)
        for ex in (None, exclude):
            ws, wi, wc = native.topk_rows(scores, k, ex)
            wr, wn = native.rank_rows(scores, targets, ex)
            for block_bytes in (64 << 20, 4 * I * 3):                   # one block of users; blocks of 3
                gs, gp, gc = top_k(m, d, users, k, exclude=ex, block_bytes=block_bytes)
                assert torch.equal(gs, ws) and torch.equal(gp, wi.to(torch.int64)) and torch.equal(gc, wc)
                rank, ranked = ranks(m, d, users, targets, exclude=ex, block_bytes=block_bytes)
                assert torch.equal(rank, wr) and torch.equal(ranked, wn)
        ids = torch.tensor([5, 20, 95], device=gpu)
        sub_s, sub_p, _ = top_k(m, d, users, 2, item_ids=ids)
        assert torch.equal(sub_s, native.topk_rows(scores.index_select(1, ids), 2)[0]) and set(sub_p.reshape(-1).tolist()) <= {5, 20, 95}
    items = torch.tensor([0, 95, 17], device=gpu)
    ns, npos, ncnt = slim.similar_items(items, 5)
    ws, wi, wc = native.topk_rows(slim.weights_[items].contiguous(), 5)
    assert torch.equal(ns, ws) and torch.equal(npos, wi.to(torch.int64)) and torch.equal(ncnt, wc) and npos.dtype == torch.int64
    slim.check()


# ------------------------------------------------------------------ 9. planted structure and the tool
def test_planted_blocks_put_the_missing_item_first(gpu):
    """On the restatement: 40 of 40, smallest score margin 0.86."""
    import deeprecommendation_amd as pkg
    from types import SimpleNamespace
    csr, held = E.planted_case()
    d = _dev(csr, gpu)
    m = pkg.SLIM(0.5, 1.0).fit_csr(*d, 24)
    assert m.n_unconverged_ == 0
    users = torch.arange(40, device=gpu)
    exclude = pkg.rated_exclusion(SimpleNamespace(rowptr=d[0], col=d[1]), users)
    score, pos, cnt = pkg.slim_top_k(m, d, users, 2, exclude=exclude)
    assert np.array_equal(pos.cpu().numpy()[:, 0], held) and (cnt == 2).all()
    margin = float((score[:, 0] - score[:, 1]).min())
    print(f"smallest margin of the held-out item over the next unrated one: {margin:.3f}")
    assert margin > 0.5
    targets = (torch.arange(41, device=gpu), torch.from_numpy(held.astype(np.int32)).to(gpu))
    rank, ranked = pkg.slim_ranks(m, d, users, targets, exclude=exclude)
    assert not rank.any() and (ranked == 24 - 7).all()
    # ease_top_k on an EASE over the shared block generator: the tuple tests/test_gpu_ease.py has held it to since EASE was added
    e = pkg.EASE(reg=1.0).fit_csr(*d, 24)
    _, epos, ecnt = pkg.ease_top_k(e, d, users, 1, exclude=exclude)
    assert np.array_equal(epos.cpu().numpy()[:, 0], held) and (ecnt == 1).all() and epos.dtype == torch.int64


def test_slim_baseline_tool_searches_the_grid_and_scores_the_best(gpu, tmp_path, monkeypatch, capsys):
    import importlib.util
    import os
    import pandas as pd
    from conftest import ROOT
    (rowptr, col, val), held = E.planted_case()
    n = len(held)
    us = np.repeat(np.arange(n), np.diff(rowptr))
    last = rowptr[1:] - 1                                              # each user's last planted item goes to VAL, the held-out one to TEST
    keep = np.ones(len(col), bool)
    keep[last] = False

    def frame(u, i):
        return pd.DataFrame({"userId": u * 3 + 5, "movieId": i.astype(np.int64) * 7 + 2, "rating": np.full(len(u), 4.0)})

    for name, f in (("train", frame(us[keep], col[keep])), ("val", frame(us[last], col[last])), ("test", frame(np.arange(n), held))):
        f.to_csv(tmp_path / (name + ".csv"), index=False)
    spec = importlib.util.spec_from_file_location("slim_baseline_tool", os.path.join(ROOT, "tools", "slim_baseline.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr("sys.argv", ["slim_baseline.py", str(tmp_path / "train"), str(tmp_path / "val"), str(tmp_path / "test.csv"), "--l1", "0.5",
                                     "2", "--l2", "1", "50", "--binary"])
    tool.main()
    lines = capsys.readouterr().out.strip().splitlines()
    grid = [l for l in lines if l.startswith("l1=")]
    assert [l.split(":")[0] for l in grid] == [f"l1={a} l2={b} positive=True binary=True" for b in (50.0, 1.0) for a in (2.0, 0.5)]
    assert all("density 0." in l and "sweeps <= " in l and "unconverged 0" in l for l in grid)
    ndcg = [float(l.split("NDCG@10 ")[1].split(",")[0]) for l in grid]
    assert all(f"({n} users)" in l for l in grid) and all(0.0 < v <= 1.0 for v in ndcg)
    best = lines[len(grid)]
    assert best.startswith("best by val NDCG@10:") and grid[int(np.argmax(ndcg))].split(":")[0] in best
    assert f"(val NDCG@10 {max(ndcg):.4f})" in best
    assert lines[-1].startswith("test HR@10 ") and f"({n} users)" in lines[-1] and 0.0 < float(lines[-1].split()[2].rstrip(",")) <= 1.0
