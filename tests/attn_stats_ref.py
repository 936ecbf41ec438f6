"""Reference, inputs and emulator for the attention-statistics kernels of csrc/attn_stats.hip (CPU only: nothing here touches a GPU).

``make_stats_case`` builds on ``attn_cross_ref.make_cross_case(..., lengths=R.LENGTHS + (300,))`` — exact dyadic logits, masked
entries, an all-masked row, an empty row, a row longer than four stripes — and draws a shuffled sample file ``(user_rows, cands)``:
with a catalogue of 100 or more candidates a third of the candidates get no sample, one gets 80 (a chain longer than a wave's 64
headers), three get 20, and one whose table column is all -inf (no finite logit: every weight 0, every valid entry still counted) gets
6; two logits of the busiest column are -inf as well (a valid entry whose weight is exactly 0).  One (user, candidate) pair is
repeated.  The builder asserts that the valid columns of every row are distinct — the kernel's documented precondition.

``expected`` adds float64 softmax weights in sample order onto the initial tables (NaN -> 0 as the reference does); ``count`` is exact.
``check`` holds a pair of buffers to it: ``count`` with torch.equal, ``sum`` through ``close`` (the project's bar), guard words after
and between the rows untouched.  ``emulate`` walks the two kernels' indices in fp32 with one optional seeded defect
(tests/test_attn_stats_cpu.py: the right walk passes ``check``, each defect fails it)."""
import functools

import numpy as np
import torch

import attn_cross_ref as X
import attn_explain_ref as XR
import attn_forms_ref as R

SLAB = 512                         # native.ATTN_STATS_SLAB: rated columns owned by one wave of the accumulation kernel
STRIPE = 64                        # entries per pass of a wave; sample headers fetched at a time
LONG_ROW = XR.LONG_ROW
PAD = 16                           # guard words after each table
LD_EXTRA = 3                       # guard words after each row of a table
SENTINEL_F = -777.25
SENTINEL_I = -77725
SEED = 43
HOT, WARM, DEAD = 5, (17, 64, 129), 9      # candidates with 80 / 20 / 6 samples; DEAD's table column is all -inf
ZERO_LOGITS = (3, 40)              # rated rows of the table whose logit towards HOT is -inf (3 is rated by most rows)
DEFECTS = ("table_not_transposed", "masked_column_counted", "last_partial_stripe_dropped", "accumulators_not_initialised",
           "count_from_positive_weight", "order_ignored", "empty_candidate_misattributed", "slab_boundary_off_by_one")
# (I_c, I_r) of the case on which each defect is shown
DEFECT_SHAPE = {d: (130, R.N_ITEMS) for d in DEFECTS}
DEFECT_SHAPE["slab_boundary_off_by_one"] = (2, SLAB + 1)

# (mode, A, I_c, I_r, seed) of the GPU test: the four attention modes x I_c in {1, 130}, and one case of two slabs with the boundary
GPU_CASES = tuple((m, A, Ic, R.N_ITEMS, SEED) for m, A in XR.MODES for Ic in (1, 130)) + ((R.ATT_MLP, 12, 2, SLAB + 1, SEED),)


def case_id(c):
    return f"{R.MODE_NAMES[c[0]]}-Ic{c[2]}-Ir{c[3]}"


def _draw_samples(Ic, n_rows, special_rows, rng):
    """(user_rows, cands) int64 in shuffled order; ``special_rows`` (the long, the empty and the all-masked row) stand in the
    busiest candidate's chain."""
    if Ic >= 100:
        named = (HOT, DEAD) + WARM
        pool = np.array([c for c in range(Ic) if c % 3 != 0 and c not in named])       # multiples of 3 (but 9, 129): no sample
        cands = np.concatenate([[HOT] * 80] + [[w] * 20 for w in WARM] + [[DEAD] * 6, rng.choice(pool, 100)])
    else:
        cands = np.concatenate([np.zeros(80, dtype=np.int64), rng.integers(0, Ic, 70)])
    S = len(cands)
    users = rng.integers(0, n_rows, S)
    users[:len(special_rows)] = special_rows
    users, cands = np.append(users, users[0]), np.append(cands, cands[0])               # one repeated (user, candidate) pair
    p = rng.permutation(S + 1)
    return torch.tensor(users[p], dtype=torch.int64), torch.tensor(cands[p], dtype=torch.int64)


def make_stats_case(mode, A, Ic, Ir, seed):
    base = X.make_cross_case(mode, A, XR.FDIM, Ic, seed, lengths=R.LENGTHS + (LONG_ROW,), Ir=Ir)
    rng = np.random.default_rng(seed + 15485863)
    rp, col = base["rowptr"], base["col"]
    n_rows = base["n_rows"]
    lens = rp[1:] - rp[:-1]
    for r in range(n_rows):                                            # the precondition: valid columns are distinct within a row
        c = col[int(rp[r]):int(rp[r + 1])]
        c = c[(c >= 0) & (c < Ir)]
        assert c.unique().numel() == c.numel(), f"row {r} repeats a valid column"
    special = [int((lens == LONG_ROW).nonzero()[0]), int((lens == 0).nonzero()[0]), base["all_masked_row"]]
    user_rows, cands = _draw_samples(Ic, n_rows, special, rng)
    st64 = base["st64"].clone()
    if Ic >= 100:
        st64[:, DEAD] = -np.inf
        st64[list(ZERO_LOGITS), HOT] = -np.inf
    case = dict(mode=mode, A=A, Ic=Ic, Ir=Ir, n_rows=n_rows, rowptr=rp, col=col, user_rows=user_rows, cands=cands, S=user_rows.numel(),
                st64=st64, special_rows=special)
    # what the case promises
    per = torch.bincount(cands, minlength=Ic)
    assert int(per.max()) >= 70 and int(lens.max()) == LONG_ROW > 4 * STRIPE
    pairs = list(zip(user_rows.tolist(), cands.tolist()))
    assert len(set(pairs)) < len(pairs), "no repeated (user, candidate) pair"
    assert Ic == 1 or not torch.equal(cands, cands.sort().values), "the sample file is not shuffled"
    busiest = int(per.argmax())
    assert set(special) <= set(user_rows[cands == busiest].tolist())
    if Ic >= 100:
        assert int((per == 0).sum()) >= Ic // 4 and int(per[:HOT].min()) == 0 and int(per[DEAD]) > 0
    if Ir > SLAB:                                                      # the first column of the second slab is rated and sampled
        hit = [r for r in range(n_rows) if SLAB in col[int(rp[r]):int(rp[r + 1])].tolist()]
        assert set(hit) & set(user_rows.tolist())
    return case


@functools.lru_cache(maxsize=None)
def stats_inputs(mode, A, Ic, Ir, seed):
    return make_stats_case(mode, A, Ic, Ir, seed)


def initial_tables(case, seed=1):
    """Non-zero tables to continue: (sum (I_c, I_r) float64, count (I_c, I_r) int64)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((case["Ic"], case["Ir"]), generator=g, dtype=torch.float64) * 4,
            torch.randint(0, 50, (case["Ic"], case["Ir"]), generator=g, dtype=torch.int64))


def sample_weights64(case, s):
    """(valid columns of sample s's row, their float64 weights towards its candidate), NaN -> 0."""
    r, c = int(case["user_rows"][s]), int(case["cands"][s])
    cols = case["col"][int(case["rowptr"][r]):int(case["rowptr"][r + 1])].long()
    cols = cols[(cols >= 0) & (cols < case["Ir"])]
    w = torch.softmax(case["st64"][cols, c], 0) if cols.numel() else torch.zeros(0, dtype=torch.float64)
    return cols, torch.nan_to_num(w, nan=0.0)


def expected(case, init=None, samples=None):
    """The tables after the listed samples (default: the whole file), added in sample order onto ``init`` (default zeros)."""
    Ic, Ir = case["Ic"], case["Ir"]
    sum64 = torch.zeros((Ic, Ir), dtype=torch.float64) if init is None else init[0].clone()
    count = torch.zeros((Ic, Ir), dtype=torch.int64) if init is None else init[1].clone()
    for s in (range(case["S"]) if samples is None else samples):
        cols, w = sample_weights64(case, s)
        c = int(case["cands"][s])
        sum64[c, cols] += w                                            # distinct columns: a plain indexed add
        count[c, cols] += 1
    return sum64, count


def fresh_tables(case, init=None):
    """(sum float64, count int64) flat buffers: I_c rows of I_r + LD_EXTRA words and PAD more, every word a sentinel except the
    tables' cells, which hold ``init`` (default zeros)."""
    Ic, Ir = case["Ic"], case["Ir"]
    n = Ic * (Ir + LD_EXTRA) + PAD
    bufs = (torch.full((n,), SENTINEL_F, dtype=torch.float64), torch.full((n,), SENTINEL_I, dtype=torch.int64))
    for v, t in zip(views(case, bufs), init or (0.0, 0)):
        v.copy_(t) if torch.is_tensor(t) else v.fill_(t)
    return bufs


def views(case, bufs):
    """The (I_c, I_r) tables inside the two flat buffers (row stride I_r + LD_EXTRA): what the kernel is given."""
    Ic, Ir = case["Ic"], case["Ir"]
    ld = Ir + LD_EXTRA
    return tuple(b[:Ic * ld].view(Ic, ld)[:, :Ir] for b in bufs)


def check(case, bufs, close, what, init=None, samples=None):
    """``bufs``: the two flat buffers of fresh_tables() as the kernel left them, on the CPU.  ``close(got, ref64, tag)`` is the
    project's bar (test_gpu_basic.assert_close with its defaults: 1e-5 |ref| + 1e-6 max |ref|)."""
    Ic, Ir = case["Ic"], case["Ir"]
    ld = Ir + LD_EXTRA
    for b, sent in zip(bufs, (SENTINEL_F, SENTINEL_I)):
        assert bool((b[Ic * ld:] == sent).all()) and bool((b[:Ic * ld].view(Ic, ld)[:, Ir:] == sent).all()), \
            f"{what}: a guard word after a table or after one of its rows was written"
    got_sum, got_count = views(case, bufs)
    ref_sum, ref_count = expected(case, init, samples)
    assert torch.equal(got_count, ref_count), f"{what}: {int((got_count != ref_count).sum())} cells of count differ"
    close(got_sum, ref_sum, what + " sum")


def emulate(case, defect=None, init=None):
    """The two kernels' walk in fp32 on the CPU with one optional seeded defect: (m, l) per sample over stripes of 64 entries, then
    per (candidate, slab) the candidate's samples in the order of the stable sort, the weights added as float64 onto accumulators
    initialised from the tables.  Returns the two flat buffers."""
    assert defect is None or defect in DEFECTS
    Ic, Ir, S = case["Ic"], case["Ir"], case["S"]
    bufs = fresh_tables(case, init)
    tsum, tcnt = (v.numpy() for v in views(case, bufs))
    st = case["st64"].float().numpy()
    flat = st.reshape(-1)
    rp, col = case["rowptr"].numpy(), case["col"].numpy().astype(np.int64)
    rows, cands = case["user_rows"].numpy(), case["cands"].numpy()

    def entries(s):
        beg, end = int(rp[rows[s]]), int(rp[rows[s] + 1])
        if defect == "last_partial_stripe_dropped":
            end = beg + (end - beg) // STRIPE * STRIPE
        cc = col[beg:end]
        if defect == "masked_column_counted":
            return cc.clip(0, Ir - 1)
        return cc[(cc >= 0) & (cc < Ir)]

    def logits(cc, c):
        return flat[(c * Ic + cc) % flat.size] if defect == "table_not_transposed" else st[cc, c]

    # kernel 1: the softmax statistics of every sample
    m, l = np.full(S, -np.inf, dtype=np.float32), np.zeros(S, dtype=np.float32)
    for s in range(S):
        lg = logits(entries(s), int(cands[s]))
        if lg.size and np.isfinite(lg.max()):
            m[s] = lg.max()
            l[s] = np.exp(lg - m[s], dtype=np.float32).sum(dtype=np.float32)
    # the sample lists: a stable sort of the candidates and the bucket offsets
    order = np.argsort(cands, kind="stable")
    cand_rowptr = np.searchsorted(cands[order], np.arange(Ic + 1))
    if defect == "empty_candidate_misattributed":                      # offsets of the candidates that occur, packed to the front
        occ = np.unique(cand_rowptr)
        cand_rowptr = np.concatenate([occ, np.full(Ic + 1 - len(occ), S)])
    # kernel 2: owner computes
    for c in range(Ic):
        for lo in range(0, Ir, SLAB):
            width = min(SLAB, Ir - lo)
            acc, cnt = tsum[c, lo:lo + width].copy(), tcnt[c, lo:lo + width].copy()
            if defect == "accumulators_not_initialised":
                acc[:], cnt[:] = 0.0, 0
            for k in range(int(cand_rowptr[c]), int(cand_rowptr[c + 1])):
                s = k if defect == "order_ignored" else int(order[k])
                cc = entries(s)
                w = np.zeros(cc.size, dtype=np.float32)
                if np.isfinite(m[s]) and l[s] > 0:
                    w = (np.exp(logits(cc, c) - m[s], dtype=np.float32) / l[s]).astype(np.float32)
                i = cc - lo
                own = (i > 0 if defect == "slab_boundary_off_by_one" and lo else i >= 0) & (i < width)
                np.add.at(acc, i[own], w[own].astype(np.float64))
                np.add.at(cnt, i[own], (w[own] > 0).astype(np.int64) if defect == "count_from_positive_weight" else 1)
            tsum[c, lo:lo + width], tcnt[c, lo:lo + width] = acc, cnt
    return bufs
