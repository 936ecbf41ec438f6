"""Reference, inputs and emulator for the explanation kernel of csrc/attn_explain.hip (CPU only: nothing here touches a GPU).

``make_explain_case`` builds on ``attn_cross_ref.make_cross_case`` (exact dyadic logits, a row of every length in
attn_forms_ref.LENGTHS, masked entries, an all-masked row, repeated and shuffled ``user_rows``) with one more row of 300 entries —
longer than a wave's 256-key buffer — and draws ``items (U, k)`` from the catalogue with one -1 slot and one repeated column.  The
float64 weights of a pair are ``softmax(st64[col_ok][:, item])``.  The builder asserts two margins, so that the expected lists are
exact whatever the fp32 rounding of the kernel: no weight lies within ``MARGIN`` (relative) of its user's threshold, and within a
pair two weights are either equal (equal logits) or more than ``MARGIN`` apart.  ``MARGIN`` = 1e-4 is ten times the project's bar
(test_gpu_basic.assert_close, rtol 1e-5).

``expected`` lists per pair the entries with w64 > thr by (-w64, entry order); ``check`` holds a result to it; ``emulate`` walks the
kernel's indices in fp32 with one optional seeded defect (tests/test_attn_explain_cpu.py: the right walk passes ``check``, each
defect fails it)."""
import functools

import numpy as np
import torch

import attn_cross_ref as X
import attn_forms_ref as R

MARGIN = 1e-4
LONG_ROW = 300                     # longer than the 256-key wave buffer of the kernel
FDIM = 64                          # make_cross_case's feature width (the explanation never reads feat)
FACTORS = (1.0, 1.07, 0.93, 1.19, 0.81, 1.31, 0.69, 1.43)
PAD = 16                           # guard words after each output buffer
SENTINEL_I = -77725
STRIPE = 64                        # entries per pass of a wave
DEFECTS = ("table_not_transposed", "col_not_masked", "tie_order_reversed", "count_capped_at_E", "thr_from_slot",
           "last_partial_stripe_dropped", "minus1_slot_as_column0", "val_from_sorted_position")
# the threshold kind on which each defect is shown (tests/test_attn_explain_cpu.py)
DEFECT_THR = {"table_not_transposed": "rule", "col_not_masked": "all", "tie_order_reversed": "all", "count_capped_at_E": "all",
              "thr_from_slot": "rule", "last_partial_stripe_dropped": "rule", "minus1_slot_as_column0": "all",
              "val_from_sorted_position": "rule"}


def _pair_weights(case, r, c):
    """(entry offsets within row r of the valid entries, their float64 weights towards table column c); None for a row without one."""
    rp = case["rowptr"]
    beg, end = int(rp[r]), int(rp[r + 1])
    cols = case["col"][beg:end].long()
    ok = (cols >= 0) & (cols < case["Ir"])
    if not bool(ok.any()):
        return None
    w = torch.softmax(case["st64"][cols[ok]][:, c], 0)
    return ok.nonzero().view(-1).numpy(), w.numpy()


@functools.lru_cache(maxsize=None)
def _cross_case(mode, A, Ic, seed):
    """The cross case every explanation case of one (mode, A, I_c, seed) shares; read only."""
    return X.make_cross_case(mode, A, FDIM, Ic, seed, lengths=R.LENGTHS + (LONG_ROW,))


MODES = ((R.ATT_MLP, 12), (R.ATT_MLP_SCALED, 8), (R.ATT_COS, 12), (R.ATT_LINEAR, 1))
SEED = 41


def _gpu_cases():
    """(mode, A, I_c, k, E, thr_kind, seed) of the GPU test: the four modes x I_c in {1, 130} x k in {1, 3, 4, 5} (3 pairs short of,
    at and past a 4-wave workgroup per user), with E in {1, 8, 64} and the three threshold kinds rotating so that every (k, E), (k, kind)
    and (E, kind) combination occurs."""
    ks, es, kinds = (1, 3, 4, 5), (1, 8, 64), ("rule", "all", "none")
    cases = []
    for i, (mode, A) in enumerate(MODES):
        for h, Ic in enumerate((130, 1)):
            for j, k in enumerate(ks):
                cases.append((mode, A, Ic, k, es[(i + j + h) % 3], kinds[(2 * i + j + 2 * h) % 3], SEED))
    return cases


GPU_CASES = _gpu_cases()


def case_id(c):
    return f"{R.MODE_NAMES[c[0]]}-Ic{c[2]}-k{c[3]}-E{c[4]}-{c[5]}"


def make_explain_case(mode, A, Ic, k, E, thr_kind, seed):
    """One explanation batch on the CPU: the cross case's CSR and ``user_rows``, ``items (U, k)``, ``thr (U,)`` fp32 of kind
    ``thr_kind`` ("rule": 1.5 / n + 0.025 per user, scaled by the first of FACTORS that keeps every weight of the user more than
    MARGIN away; "all": -1, everything qualifies; "none": 2), the float64 weights per pair (``pairs[u][s]`` = (entry offsets, w64) or
    None for a dead pair) and the asserted margins."""
    assert thr_kind in ("rule", "all", "none") and 1 <= E <= 64 and k >= 1
    base = _cross_case(mode, A, Ic, seed)
    rng = np.random.default_rng(seed + 104729)
    user_rows = base["user_rows"]
    U = user_rows.numel()
    rp = base["rowptr"]
    lens = (rp[1:] - rp[:-1])[user_rows]
    items = rng.integers(0, Ic, (U, k))
    long_u = int((lens == LONG_ROW).nonzero()[0])
    other_u = int((lens == 200).nonzero()[0])
    if k >= 2:
        items[other_u, 1] = items[other_u, 0]                         # one repeated column
    else:
        items[other_u, 0] = items[long_u, 0]
    empty_slot = (long_u, k - 1) if k >= 2 else (int((lens == 129).nonzero()[0]), 0)
    items[empty_slot] = -1                                            # one empty slot, on a user whose row is live
    case = dict(mode=mode, A=A, Ic=Ic, Ir=base["Ir"], k=k, E=E, U=U, thr_kind=thr_kind, n_rows=base["n_rows"], rowptr=rp, col=base["col"],
                val=base["val"], user_rows=user_rows, items=torch.tensor(items, dtype=torch.int64), st64=base["st64"],
                all_masked_row=base["all_masked_row"], empty_slot=empty_slot)
    pairs = [[None if items[u, s] < 0 else _pair_weights(case, int(user_rows[u]), int(items[u, s])) for s in range(k)] for u in range(U)]
    thr = np.zeros(U, dtype=np.float32)
    for u in range(U):
        if thr_kind != "rule":
            thr[u] = -1.0 if thr_kind == "all" else 2.0
            continue
        n = max(int(lens[u]), 1)
        ws = np.concatenate([p[1] for p in pairs[u] if p is not None] + [np.zeros(0)])
        for f in FACTORS:
            t = np.float32((1.5 / n + 0.025) * f)
            if not bool((np.abs(ws - float(t)) <= MARGIN * float(t)).any()):
                break
        else:
            raise AssertionError(f"user {u}: no factor keeps the weights away from the threshold")
        thr[u] = t
    case["pairs"], case["thr"] = pairs, torch.from_numpy(thr)
    check_margins(case)
    return case


def check_margins(case):
    """The builder's two margins, and what the case promises (a -1 slot, a repeated column, the long row, a dead row)."""
    thr = case["thr"].double().numpy()
    gap = np.inf
    for u, row in enumerate(case["pairs"]):
        for p in row:
            if p is None:
                continue
            w = p[1]
            assert not bool((np.abs(w - thr[u]) <= MARGIN * abs(thr[u])).any()), "a weight within the margin of its threshold"
            d = np.unique(w)                                           # ascending; equal logits give equal float64 weights
            if d.size > 1:
                rel = (d[1:] - d[:-1]) / d[1:]
                assert float(rel.min()) > MARGIN, "two distinct weights of a pair closer than the margin"
                gap = min(gap, float(rel.min()))
    case["min_gap"] = gap
    items = case["items"]
    assert int((items == -1).sum()) == 1 and int(items[case["empty_slot"]]) == -1
    lens = (case["rowptr"][1:] - case["rowptr"][:-1])[case["user_rows"]]
    assert int(lens.max()) == LONG_ROW > 256 and case["all_masked_row"] in case["user_rows"].tolist() and int(lens.min()) == 0
    if case["k"] >= 2:
        assert any(len(set(r)) < len(r) for r in items.tolist())
    return case


@functools.lru_cache(maxsize=None)
def explain_inputs(mode, A, Ic, k, E, thr_kind, seed):
    return make_explain_case(mode, A, Ic, k, E, thr_kind, seed)


def expected(case):
    """Per pair ``(cnt, entry offsets of the first E)``: the valid entries with w64 > thr by (-w64, entry order)."""
    thr, E = case["thr"].double().numpy(), case["E"]
    out = []
    for u, row in enumerate(case["pairs"]):
        res = []
        for p in row:
            if p is None:
                res.append((0, np.zeros(0, dtype=np.int64), np.zeros(0)))
                continue
            idx, w = p
            q = w > thr[u]
            order = np.lexsort((idx[q], -w[q]))
            res.append((int(q.sum()), idx[q][order][:E], w[q][order][:E]))
        out.append(res)
    return out


def fresh_outputs(case):
    """(col int32, w fp32, val fp32, cnt int32) flat buffers with PAD guard words, every word a sentinel."""
    n, m = case["U"] * case["k"] * case["E"], case["U"] * case["k"]
    return (torch.full((n + PAD,), SENTINEL_I, dtype=torch.int32), torch.full((n + PAD,), R.SENTINEL, dtype=torch.float32),
            torch.full((n + PAD,), R.SENTINEL, dtype=torch.float32), torch.full((m + PAD,), SENTINEL_I, dtype=torch.int32))


def views(case, bufs):
    """The (U, k, E) / (U, k) heads of the four flat buffers: what the kernel is given as ``out``."""
    U, k, E = case["U"], case["k"], case["E"]
    n = U * k * E
    return bufs[0][:n].view(U, k, E), bufs[1][:n].view(U, k, E), bufs[2][:n].view(U, k, E), bufs[3][:U * k].view(U, k)


def check(case, bufs, close, what):
    """``bufs``: the four flat buffers of fresh_outputs() as the kernel left them, on the CPU.  ``close(got, ref64, tag)`` is the
    project's bar (test_gpu_basic.assert_close with its defaults)."""
    U, k, E = case["U"], case["k"], case["E"]
    n = U * k * E
    assert all(bool((b[m:] == s).all()) for b, m, s in zip(bufs, (n, n, n, U * k), (SENTINEL_I, R.SENTINEL, R.SENTINEL, SENTINEL_I))), \
        f"{what}: a guard word after an output buffer was written"
    rc, rw, rv, cnt = views(case, bufs)
    assert not bool((rc == SENTINEL_I).any() or (rw == R.SENTINEL).any() or (rv == R.SENTINEL).any() or (cnt == SENTINEL_I).any()), \
        f"{what}: output words never written"
    exp = expected(case)
    rp, col, val = case["rowptr"], case["col"], case["val"]
    got_w, ref_w = [], []
    for u in range(U):
        beg = int(rp[int(case["user_rows"][u])])
        t = case["thr"][u]
        for s in range(k):
            c, idx, w64 = exp[u][s]
            assert int(cnt[u, s]) == c, f"{what}: pair ({u}, {s}) counts {int(cnt[u, s])} reasons, expected {c}"
            m = min(c, E)
            e = torch.from_numpy(idx).long() + beg
            assert torch.equal(rc[u, s, :m], col[e]), f"{what}: pair ({u}, {s}) lists {rc[u, s, :m].tolist()}, expected {col[e].tolist()}"
            assert torch.equal(rv[u, s, :m].view(torch.int32), val[e].view(torch.int32)), f"{what}: pair ({u}, {s}) ratings are not the row's"
            w = rw[u, s, :m]
            assert bool((w > t).all()), f"{what}: pair ({u}, {s}) lists a weight that is not above the threshold"
            assert bool((w[1:] <= w[:-1]).all()), f"{what}: pair ({u}, {s}) weights are not in descending order"
            assert bool((rc[u, s, m:] == -1).all()) and bool((rw[u, s, m:] == 0).all()) and bool((rv[u, s, m:] == 0).all()), \
                f"{what}: pair ({u}, {s}) unused slots must hold (-1, 0, 0)"
            got_w.append(w)
            ref_w.append(torch.from_numpy(w64))
    if sum(w.numel() for w in ref_w):                                 # nothing listed (thr = 2): nothing to compare
        close(torch.cat(got_w), torch.cat(ref_w), what + " weights")


def emulate(case, defect=None):
    """attn_explain_kernel's walk in fp32 on the CPU — one pair at a time: the table column gathered over the row's valid entries in
    stripes of 64, the exact maximum, exp / sum, w = p / l, the threshold of the pair's USER, the count, the E best by (weight,
    entry order) — with one optional seeded defect.  Returns the four flat buffers."""
    assert defect is None or defect in DEFECTS
    U, k, E, Ir, Ic = case["U"], case["k"], case["E"], case["Ir"], case["Ic"]
    bufs = fresh_outputs(case)
    rc, rw, rv, cnt = (v.numpy() for v in views(case, bufs))
    st = case["st64"].float().numpy()
    flat = st.reshape(-1)
    rp, col, val = case["rowptr"].numpy(), case["col"].numpy().astype(np.int64), case["val"].numpy()
    thr, items, rows = case["thr"].numpy(), case["items"].numpy(), case["user_rows"].numpy()
    for u in range(U):
        beg, end = int(rp[rows[u]]), int(rp[rows[u] + 1])
        if defect == "last_partial_stripe_dropped":
            end = beg + (end - beg) // STRIPE * STRIPE
        for s in range(k):
            rc[u, s], rw[u, s], rv[u, s], cnt[u, s] = -1, 0.0, 0.0, 0
            c = int(items[u, s])
            if c == -1 and defect == "minus1_slot_as_column0":
                c = 0
            if c < 0:
                continue
            cc = col[beg:end]
            if defect == "col_not_masked":
                ok = np.ones(cc.shape, dtype=bool)
                cc = cc.clip(0, Ir - 1)
            else:
                ok = (cc >= 0) & (cc < Ir)
            if not ok.any():
                continue
            idx = np.nonzero(ok)[0]
            lg = flat[(c * Ic + cc[ok]) % flat.size] if defect == "table_not_transposed" else st[cc[ok], c]
            p = np.exp(lg - lg.max(), dtype=np.float32)
            w = (p / p.sum(dtype=np.float32)).astype(np.float32)
            t = thr[s % U] if defect == "thr_from_slot" else thr[u]
            q = w > t
            tie = -idx[q] if defect == "tie_order_reversed" else idx[q]
            order = np.lexsort((tie, -w[q]))
            n = int(q.sum())
            m = min(n, E)
            cnt[u, s] = m if defect == "count_capped_at_E" else n
            e = beg + idx[q][order][:m]
            rc[u, s, :m], rw[u, s, :m] = col[e], w[q][order][:m]
            rv[u, s, :m] = val[beg + np.arange(m)] if defect == "val_from_sorted_position" else val[e]
    return bufs
