"""GPU tests of the EASE baseline against tests/ease_ref.py: the Gram rows, the weights, the scores and predict bit for bit against the
fp32 restatements; the blocked MFMA inversion against the float64 inverse, held to 8 x the error (and the residual) of the fp32
restatement of the same blocked algorithm, at every size where a partial panel or tile can go wrong, with repeatability and the pivot
flag; the fit, the ranking front ends, similar_items, a planted structure and tools/ease_baseline.py.

Why 8 x: the device sums each panel product as an MFMA k-chain, the restatement through BLAS — two orders of the same fp32 sums, both
a decade above LAPACK's fp32 inverse on these matrices.  Each test first holds the restatement's own figure under 1e-5 of max|P|, so the
yardstick cannot go slack."""
import numpy as np
import pytest
import torch

import ease_ref as E

pytestmark = pytest.mark.gpu
NB = E.NB
_cache = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _dev(arrays, gpu):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays)


def _csr_t(csr, I, gpu):
    return _dev(csr + E.transpose_ref(*csr, I), gpu)


def _invert(gpu, G, lam, pad=5, sentinel=7.25):
    """The device inverse of G + lam 1 from a buffer with rows of N + pad floats; also checks that the padding is untouched."""
    from deeprecommendation_amd import native
    N = len(G)
    buf = torch.full((N, N + pad), sentinel, dtype=torch.float32, device=gpu)
    buf[:, :N] = torch.from_numpy(G).to(gpu)
    out = native.ease_invert(buf[:, :N], lam)
    assert out.data_ptr() == buf.data_ptr() and bool((buf[:, N:] == sentinel).all())
    return buf[:, :N].cpu().numpy()


def _case_inverse(gpu, c):
    if c not in _cache:
        s = E.solved(c)
        _cache[c] = _invert(gpu, s["G"], s["lam"])
    return _cache[c]


# ------------------------------------------------------------------ 1. Gram
@pytest.mark.parametrize("c", range(len(E.CASES)))
def test_gram_rows_match_the_restatement_bit_for_bit_whole_and_in_blocks(gpu, c):
    from deeprecommendation_amd import native
    s = E.solved(c)
    I = s["I"]
    d = _csr_t(s["csr"], I, gpu)
    G = native.ease_gram(*d)
    assert _same(G, s["G"]) and torch.equal(G, G.t())
    cut = (0, 37, I // 2 + 1, I)
    parts = [native.ease_gram(*d, (a, b)) for a, b in zip(cut[:-1], cut[1:])]
    assert _same(torch.cat(parts), s["G"])
    native.check_oob(gpu), native.check_ease(gpu)


def test_gram_over_two_column_tiles_and_a_row_longer_than_the_whole_walk(gpu):
    from deeprecommendation_amd import native
    csr = E.wide_case()
    d = _csr_t(csr, E.WIDE_I, gpu)
    rows = (E.WIDE_I - 70, E.WIDE_I)                                    # items of the second tile
    G = native.ease_gram(*d, rows)
    want = E.gram_ref(*csr, E.WIDE_I)
    assert _same(G, want[rows[0]:rows[1]])
    assert _same(native.ease_gram(*d, (0, 40)), want[:40])
    native.check_oob(gpu), native.check_ease(gpu)


def test_gram_flags_a_column_outside_the_items_and_a_row_that_does_not_ascend(gpu):
    from deeprecommendation_amd import native
    from deeprecommendation_amd.baselines import build_transpose
    s = E.solved(0)
    I = s["I"]
    rowptr, col, val = (a.copy() for a in s["csr"])
    u = int(np.argmax(np.diff(rowptr)))
    e = rowptr[u + 1] - 1                                              # the last entry of the longest row: still ascending
    col[e] = I + 5
    d = _dev((rowptr, col, val), gpu)
    G = native.ease_gram(*d, *build_transpose(*d, I))
    keep = np.ones(len(col), bool)
    keep[e] = False
    rp = rowptr.copy()
    rp[u + 1:] -= 1
    assert _same(G, E.gram_ref(rp, col[keep], val[keep], I))            # the entry adds nothing
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.check_oob(gpu), native.check_ease(gpu)
    rowptr, col, val = (a.copy() for a in s["csr"])
    b = rowptr[u]
    col[b], col[b + 1] = col[b + 1], col[b]
    d = _dev((rowptr, col, val), gpu)
    native.ease_gram(*d, *build_transpose(*d, I))
    with pytest.raises(ValueError, match="ascending"):
        native.check_ease(gpu)
    native.check_ease(gpu), native.check_oob(gpu)


# ------------------------------------------------------------------ 2. inversion shapes
@pytest.mark.parametrize("N", [1, 2, NB - 1, NB, NB + 1, 2 * NB + 1, 600, 1000])
def test_inversion_at_every_panel_and_tile_edge(gpu, N):
    s = E.solved(3)
    G, lam = np.ascontiguousarray(s["G"][:N, :N]), s["lam"]
    P64 = E.inverse64(G, lam)
    Pb = E.blocked_inverse_ref(G, lam)
    ref_err, ref_res = E.rel_err(Pb, P64), E.residual(G, lam, Pb)
    P = _invert(gpu, G, lam)
    err, res = E.rel_err(P, P64), E.residual(G, lam, P)
    print(f"N={N}: device {err:.3e} (residual {res:.3e}), restatement {ref_err:.3e} (residual {ref_res:.3e})")
    assert ref_err < 1e-5
    assert err <= 8 * ref_err and res <= 8 * ref_res
    if N <= NB:                                                         # one panel: every product is with 0 or 1, so the scalar elimination's bits
        assert _same(P, Pb)


# ------------------------------------------------------------------ 3. / 4. accuracy and residual
@pytest.mark.parametrize("c", range(len(E.CASES)))
def test_inversion_accuracy_and_residual_within_8x_the_blocked_fp32_restatement(gpu, c):
    s = E.solved(c)
    P = _case_inverse(gpu, c)
    err, res = E.rel_err(P, s["P64"]), E.residual(s["G"], s["lam"], P)
    print(f"case {E.CASES[c]}: device {err:.3e} / restatement {s['err_P']:.3e} = {err / s['err_P']:.2f}; "
          f"residual {res:.3e} / {s['res']:.3e} = {res / s['res']:.2f}")
    assert s["err_P"] < 1e-5
    assert err <= 8 * s["err_P"]
    assert res <= 8 * s["res"]


# ------------------------------------------------------------------ 5. repeatability and pivots
def test_inversion_repeats_its_bits_and_a_bad_pivot_gives_zeros_and_raises(gpu):
    from deeprecommendation_amd import native
    s = E.solved(2)
    a, b = _invert(gpu, s["G"], s["lam"]), _invert(gpu, s["G"], s["lam"], pad=0)
    assert _same(a, b) and _same(a, _case_inverse(gpu, 2))
    native.check_ease(gpu)
    bad = s["G"].copy()
    bad[5, 300] = bad[300, 5] = np.nan
    assert not _invert(gpu, bad, s["lam"]).any()
    with pytest.raises(ValueError, match="pivot"):
        native.check_ease(gpu)
    native.check_ease(gpu)                                              # raised once, then cleared
    bad = s["G"].copy()
    bad[200, 200] = -1.0                                                # indefinite: the second panel's elimination meets it
    assert not _invert(gpu, bad, 1e-3).any()
    with pytest.raises(ValueError, match="pivot"):
        native.check_ease(gpu)
    assert _same(_invert(gpu, s["G"], s["lam"]), a)                     # a clean call after all that
    native.check_ease(gpu)


# ------------------------------------------------------------------ 6. weights
@pytest.mark.parametrize("c", [0, 2])
def test_weights_match_the_restatement_from_the_devices_own_inverse(gpu, c):
    from deeprecommendation_amd import native
    P = _case_inverse(gpu, c)
    N = len(P)
    buf = torch.full((N, N + 3), -2.5, dtype=torch.float32, device=gpu)
    buf[:, :N] = torch.from_numpy(P).to(gpu)
    diag = torch.empty(N, dtype=torch.float32, device=gpu)
    W = native.ease_weights(buf[:, :N], diag).cpu().numpy()
    assert _same(W, E.weights_ref(P)) and _same(diag, np.diag(P).copy()) and bool((buf[:, N:] == -2.5).all())
    assert not np.diag(W).any() and not np.signbit(np.diag(W)).any()


# ------------------------------------------------------------------ 7. scores and predict
def _wide_model(gpu):
    if "wide" not in _cache:
        import deeprecommendation_amd as pkg
        d = _dev(E.wide_case(), gpu)
        m = pkg.EASE(reg=E.WIDE_LAM).fit_csr(*d, E.WIDE_I)
        _cache["wide"] = (m, d, m.weights_.cpu().numpy())
    return _cache["wide"]


def test_scores_and_predict_match_the_restatement_from_the_devices_own_weights(gpu):
    from deeprecommendation_amd import native
    m, d, W = _wide_model(gpu)
    csr = E.wide_case()
    R = E.WIDE_ROWS
    assert [int(csr[0][r + 1] - csr[0][r]) for r in R.values()] == [0, 1, 64, 65, 2049]
    rows = [R["long"], R["empty"], R["one"], 3, R["n64"], R["n65"], 3]
    users = torch.tensor(rows, device=gpu)
    want = E.scores_ref(*csr, rows, W)
    assert _same(m.scores(d, users), want) and not want[1].any() and np.abs(want[0]).max() > 0
    assert _same(m.scores(d, users, stage_cap=64), want)                # 65 entries: past this cap, the same bits
    i0, i1 = 100, 1300                                                  # cuts the 1024-column tile at both ends
    big = torch.full((len(rows), i1 - i0 + 3), 9.5, dtype=torch.float32, device=gpu)
    out = native.ease_scores(*d, users, m.weights_, (i0, i1), out=big[:, :i1 - i0])
    assert _same(out, want[:, i0:i1]) and bool((big[:, i1 - i0:] == 9.5).all())
    m.check()
    items = torch.tensor([0, 99, 1023, 1024, 2047, 2048, E.WIDE_I - 1], device=gpu)
    uu, ii = torch.meshgrid(users, items, indexing="ij")
    pred = m.predict(d, uu.reshape(-1).contiguous(), ii.reshape(-1).contiguous())
    assert _same(pred.view(len(rows), -1), want[:, items.cpu().numpy()])  # predict(u, i) == scores[u, i] bit for bit
    m.check()
    n_rows = len(csr[0]) - 1
    got = m.scores(d, torch.tensor([3, n_rows, -1], device=gpu))        # rows that do not exist score as empty ones
    with pytest.raises(IndexError):
        m.check()
    m.check()
    assert _same(got[:1], want[3:4]) and not got[1:].cpu().numpy().any()
    pred = m.predict(d, torch.tensor([3, 3, n_rows], device=gpu), torch.tensor([7, E.WIDE_I, 7], device=gpu))
    with pytest.raises(IndexError):
        m.check()
    assert _same(pred[:1], want[3, 7:8]) and not pred[1:].cpu().numpy().any()


# ------------------------------------------------------------------ 8. fit
def test_fit_is_the_closed_form_and_a_grid_of_regs_shares_one_gram_matrix(gpu):
    import deeprecommendation_amd as pkg
    s = E.solved(1)
    d = _dev(s["csr"], gpu)
    m = pkg.EASE(reg=s["lam"]).fit_csr(*d, s["I"])
    W = m.weights_.cpu().numpy()
    assert m.num_items_ == s["I"] and W.shape == (s["I"], s["I"])
    err, kkt = E.rel_err(W, s["W64"]), E.kkt(s["G"], s["lam"], W)
    print(f"fit: |W - W64| / max|W64| = {err:.3e} (restatement {s['err_W']:.3e}); KKT {kkt:.3e} (restatement {s['kkt']:.3e})")
    assert s["err_W"] < 1e-5 and err <= 8 * s["err_W"] and kkt <= 8 * s["kkt"]
    assert _same(W, E.weights_ref(_case_inverse(gpu, 1)))               # the fit is gram -> invert -> weights, bit for bit
    two = pkg.EASE().fit_csr(*d, s["I"], at_regs=[20, 200.0])
    assert [t.reg for t in two] == [20.0, 200.0]
    assert torch.equal(two[0].weights_, m.weights_)
    assert torch.equal(two[1].weights_, pkg.EASE(reg=200.0).fit_csr(*d, s["I"], block_bytes=4 * s["I"] * 100).weights_)
    assert not torch.equal(two[0].weights_, two[1].weights_)


def test_binary_fit_is_a_fit_on_ones_and_samples_may_come_in_any_order(gpu):
    import deeprecommendation_amd as pkg
    s = E.solved(2)
    rowptr, col, val = s["csr"]
    assert val.max() == 5.0
    d = _dev(s["csr"], gpu)
    a = pkg.EASE(reg=50.0, binary=True).fit_csr(*d, s["I"])
    b = pkg.EASE(reg=50.0).fit_csr(d[0], d[1], torch.ones_like(d[2]), s["I"])
    assert torch.equal(a.weights_, b.weights_)
    users = torch.arange(9, device=gpu)
    assert torch.equal(a.scores(d, users), b.scores((d[0], d[1], torch.ones_like(d[2])), users))
    us = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    perm = np.random.default_rng(5).permutation(len(us))
    u, i, r = _dev((us[perm], col.astype(np.int64)[perm], val[perm]), gpu)
    c = pkg.EASE(reg=50.0).fit(u, i, r, len(rowptr) - 1, s["I"])
    assert torch.equal(c.weights_, pkg.EASE(reg=50.0).fit_csr(*d, s["I"]).weights_)


# ------------------------------------------------------------------ 9. ranking and neighbours
def test_front_ends_are_topk_and_rank_rows_over_the_scores_block_by_block(gpu):
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd import native
    from types import SimpleNamespace
    s = E.solved(1)
    I = s["I"]
    d = _dev(s["csr"], gpu)
    m = pkg.EASE(reg=s["lam"]).fit_csr(*d, I)
    users = torch.arange(40, device=gpu)
    k = 7
    scores = m.scores(d, users)
    exclude = pkg.rated_exclusion(SimpleNamespace(rowptr=d[0], col=d[1]), users)
    targets = (torch.arange(0, 81, 2, device=gpu), torch.arange(80, device=gpu, dtype=torch.int32) * 3 % I)
    for ex in (None, exclude):
        ws, wi, wc = native.topk_rows(scores, k, ex)
        wr, wn = native.rank_rows(scores, targets, ex)
        for block_bytes in (64 << 20, 4 * I * 3):                       # one block of users; blocks of 3
            gs, gp, gc = pkg.ease_top_k(m, d, users, k, exclude=ex, block_bytes=block_bytes)
            assert torch.equal(gs, ws) and torch.equal(gp, wi.to(torch.int64)) and torch.equal(gc, wc)
            rank, ranked = pkg.ease_ranks(m, d, users, targets, exclude=ex, block_bytes=block_bytes)
            assert torch.equal(rank, wr) and torch.equal(ranked, wn)
    rowptr, col, _ = s["csr"]
    p = gp.cpu().numpy()                                                # the last pass excluded the rated items
    assert all(not set(p[b].tolist()) & set(col[rowptr[b]:rowptr[b + 1]].tolist()) for b in range(40)) and (gc == k).all()
    ids = torch.tensor([5, 200, 256], device=gpu)
    sub_s, sub_p, _ = pkg.ease_top_k(m, d, users, 2, item_ids=ids)
    assert torch.equal(sub_s, native.topk_rows(scores.index_select(1, ids), 2)[0]) and set(sub_p.reshape(-1).tolist()) <= {5, 200, 256}
    items = torch.tensor([0, 256, 17], device=gpu)
    ns, npos, ncnt = m.similar_items(items, 5)
    ws, wi, wc = native.topk_rows(m.weights_[items].contiguous(), 5)
    assert torch.equal(ns, ws) and torch.equal(npos, wi.to(torch.int64)) and torch.equal(ncnt, wc) and npos.dtype == torch.int64
    m.check()


# ------------------------------------------------------------------ 10. planted structure and the tool
def test_planted_blocks_put_the_missing_item_first(gpu):
    import deeprecommendation_amd as pkg
    from types import SimpleNamespace
    csr, held = E.planted_case()
    d = _dev(csr, gpu)
    m = pkg.EASE(reg=1.0).fit_csr(*d, 24)
    users = torch.arange(40, device=gpu)
    exclude = pkg.rated_exclusion(SimpleNamespace(rowptr=d[0], col=d[1]), users)
    _, pos, cnt = pkg.ease_top_k(m, d, users, 1, exclude=exclude)
    assert np.array_equal(pos.cpu().numpy()[:, 0], held) and (cnt == 1).all()
    targets = (torch.arange(41, device=gpu), torch.from_numpy(held.astype(np.int32)).to(gpu))
    rank, ranked = pkg.ease_ranks(m, d, users, targets, exclude=exclude)
    assert not rank.any() and (ranked == 24 - 7).all()
    assert pkg.ranking_metrics(rank, targets[0], ranked, cutoffs=(1,))["hr@1"] == 1.0


def test_ease_baseline_tool_searches_the_grid_and_scores_the_best(gpu, tmp_path, monkeypatch, capsys):
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
    spec = importlib.util.spec_from_file_location("ease_baseline_tool", os.path.join(ROOT, "tools", "ease_baseline.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr("sys.argv", ["ease_baseline.py", str(tmp_path / "train"), str(tmp_path / "val"), str(tmp_path / "test.csv"), "--regs", "0.5",
                                     "5", "500", "--binary"])
    tool.main()
    lines = capsys.readouterr().out.strip().splitlines()
    grid = [l for l in lines if l.startswith("reg=")]
    assert [l.split(":")[0] for l in grid] == [f"reg={r} binary=True" for r in (0.5, 5.0, 500.0)]
    ndcg = [float(l.split("NDCG@10 ")[1].split(",")[0]) for l in grid]
    assert all(f"({n} users)" in l for l in grid) and all(0.0 < v <= 1.0 for v in ndcg)
    best = lines[len(grid)]
    assert best.startswith("best by val NDCG@10:") and grid[int(np.argmax(ndcg))].split(":")[0] in best
    assert f"(val NDCG@10 {max(ndcg):.4f})" in best
    assert lines[-1].startswith("test HR@10 ") and f"({n} users)" in lines[-1] and 0.0 < float(lines[-1].split()[2].rstrip(",")) <= 1.0
