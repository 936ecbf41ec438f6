"""References, inputs and case tables for the kernels AttentionNCF inference runs (CPU only: nothing here touches a GPU):
  csrc/attn_cand.hip    candidate embeddings + the candidate half of AttentionNet.0 (+ the fused grouping): the LDS-staged form, the
                        packed-weight form, and its split-K pair (cand_splitk_kernel + cand_finish_kernel), cand_pack_kernel;
  csrc/attn_split.hip   attn_split_kernel <MODE in {0, 2, 3}, NW in {4, 8, 16}, FD in {64, 128}> and attn_combine_kernel;
  csrc/attn_tail.hip    attn_tail_kernel <E in {64, 128}, plain | packed weights>, tail_pack_kernel.

``cand_form`` .. ``tail_form`` mirror the dispatch; the tables below reach every form.  The candidate and tail cases are EXACT:
small integers (multiples of 2^-3 on the tail's user half) chosen so that every product and every partial sum in any order is exact
in fp32 — the builders assert it from the sum of the absolute values of the terms — so the kernels must equal the reference bit for
bit whatever their summation order, and a dropped, doubled or misplaced k shows.  The entry-split cases are attn_forms_ref.make_inputs'
(exact logits, spread <= 8, masked entries, poisoned buffers) with a float64 reference of every (pair, slice) partial added.  Every
operand is a column slice of a wider poisoned buffer; every output starts as a sentinel.  The checks are shared by
tests/test_gpu_serve_forms.py and by the CPU emulators of tests/test_serve_forms_cpu.py, which show that index defects fail them."""
import collections
import functools

import numpy as np
import torch

import attn_forms_ref as R
from attn_forms_ref import ATT_COS, ATT_MLP, ATT_MLP_SCALED, POISON, SENTINEL

EXACT_MAX = float(1 << 24)         # integers below 2^24 are exact in fp32
GROUP_LDS_ROWS = 4096              # group_pairs.h kGroupLdsRows
PART_HEAD = 4                      # attn_split.hip kPartHead / attn_tail.hip kTailHead
OUT_PAD = 16                       # sentinel words after a vector output
TAIL_N1, TAIL_N2 = 256, 128


# ------------------------------------------------------------------------------------------------ mirrors of the dispatch
def cand_splitk_pieces(B):
    """attn_cand.hip cand_splitk_pieces (:488-493): pieces of the K range of a row tile, packed form."""
    tiles = (B + 15) // 16
    if tiles < 1 or tiles > 128:
        return 1
    return min(8, 256 // tiles)


def cand_form(packed, B, N1):
    """("staged" | "packed" | "splitk", KS): cand_launch's choice (attn_cand.hip:512 and :557-575)."""
    assert N1 in (64, 128)
    if not packed:
        return "staged", 1
    ks = cand_splitk_pieces(B)
    return ("splitk", ks) if ks > 1 else ("packed", 1)


def cand_slices(K, KS):
    """([(s_lo, s_hi)] of slice 0 .. 8 KS - 1 over the K // 32 whole steps, ragged): attn_cand_kernel :62-63, attn_cand_packed_kernel
    :237-238 (KS = 1) and cand_splitk_kernel :369-371; ``ragged`` = K & 31 != 0, the block slice 0 adds (:139, :299, :393)."""
    SF, nsl = K // 32, 8 * KS
    return [(s * SF // nsl, (s + 1) * SF // nsl) for s in range(nsl)], bool(K & 31)


SplitForm = collections.namedtuple("SplitForm", "inst path swizzled lds_bytes raised")


def split_supported(mode, A, Fdim, ppw):
    """ncf_attn_split_supported (attn_split.hip:443-450)."""
    if mode not in (ATT_MLP, ATT_COS, ATT_MLP_SCALED) or A <= 0 or A % 32 or A > 256 or Fdim not in (64, 128) or not 1 <= ppw <= 64:
        return False
    pp = 16 if ppw <= 16 else 32 if ppw <= 32 else 64
    return (64 * (A + Fdim) + pp * 66 + pp + 2 * pp) * 4 <= 160 * 1024


def split_form(mode, A, Fdim, ppw):
    """ncf_attn_forward_split's instantiation (attn_split.hip:483-508) and attn_split_kernel's pr-DMA path (``issue``, :131-155):
    rows of 16 / 32 / 64 chunks go by readlane (4 / 2 / 1 rows per piece), A = 32 by shifts, the other widths by division."""
    assert split_supported(mode, A, Fdim, ppw)
    pp = 16 if ppw <= 16 else 32 if ppw <= 32 else 64
    A4 = A // 4
    path = {16: "readlane4", 32: "readlane2", 64: "readlane1", 8: "shift"}.get(A4, "divide")
    lds = (64 * (A + Fdim) + pp * 66 + pp + 2 * pp) * 4
    return SplitForm(({ATT_MLP: 0, ATT_COS: 2, ATT_MLP_SCALED: 3}[mode], pp // 4, Fdim), path, A4 % 16 == 0, lds, lds > 64 * 1024)


def split_slices(length, nsplit):
    """[(t0, t1)] tile range of every slice of a row of ``length`` entries (attn_split.hip:99-100)."""
    T = (length + 63) // 64
    return [(s * T // nsplit, (s + 1) * T // nsplit) for s in range(nsplit)]


def split_slots(cnt, NW):
    """The np of every wave of a group of ``cnt`` pairs (attn_split.hip:106); the score loop is compiled for slot_width(np) slots."""
    return {(cnt - w + NW - 1) // NW if cnt > w else 0 for w in range(NW)}


def slot_width(n):
    return 0 if n == 0 else 1 if n == 1 else 2 if n == 2 else 4          # score_dispatch, attn_split.hip:272-277


def tail_form(E, packed, source, nsplit):
    """(E, packed, "user" | "partials<=8" | "partials>8"): ncf_attn_tail's instantiation (attn_tail.hip:235-241) and the fill of the
    user half (:56-103)."""
    assert E in (64, 128)
    if source == "user":
        return E, bool(packed), "user"
    return E, bool(packed), "partials<=8" if nsplit <= 8 else "partials>8"


def group_ref(pair_row, n_rows, ppw):
    """ncf_group_pairs' output: (grp_ptr, pair_ids (pairs of a row in ascending order: the order inside a row is unspecified),
    wg_ptr, wg_row[:n_wg])."""
    pr = np.asarray(pair_row, dtype=np.int64)
    counts = np.bincount(pr, minlength=n_rows)[:n_rows]
    wgs = (counts + ppw - 1) // ppw
    z = lambda c: torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64))
    return z(counts), torch.from_numpy(np.argsort(pr, kind="stable").astype(np.int64)), z(wgs), torch.from_numpy(np.repeat(np.arange(n_rows), wgs).astype(np.int32))


# ------------------------------------------------------------------------------------------------ candidates
CandCase = collections.namedtuple("CandCase", "B K N1 N2 users bias seed")
CAND_K = (1, 31, 32, 33, 63, 65, 255, 256, 257, 2094)
CAND_N2 = (16, 48, 128, 144, 256)
CAND_B = (1, 15, 16, 17, 512, 513, 576, 600, 700, 900, 1200, 2048, 2049, 2061)
PPW_GROUP = 32


def _cand_cases():
    cases, n = [], 0
    for i, B in enumerate(CAND_B):
        for j, N1 in enumerate((64, 128)):
            K = CAND_K[(i + 3 * j) % len(CAND_K)]
            users = (1, 5, B)[n % 3]
            cases.append(CandCase(B, K, N1, CAND_N2[(i + 2 * j) % 5], users, n % 4 != 2, 2000 + n))
            n += 1
    for i, B in enumerate((513, 600, 1200, 900, 700, 2048, 17, 2049)):   # the reference's K on every KS, both widths
        for j, N1 in enumerate((64, 128)):
            cases.append(CandCase(B, 2094, N1, CAND_N2[(i + j + 2) % 5], (5, 1, B)[n % 3], n % 4 != 1, 2000 + n))
            n += 1
    for k, K in enumerate(CAND_K):                                      # every K on the split-K form (small batches) ...
        cases.append(CandCase((33, 17, 100)[k % 3], K, (64, 128)[k % 2], CAND_N2[k % 5], (5, 1)[k % 2], k % 3 != 0, 2100 + k))
    cases.append(CandCase(33, 65, 64, 48, GROUP_LDS_ROWS + 1, True, 2200))   # R > kGroupLdsRows: the global-counter grouping body
    return cases


CAND_CASES = _cand_cases()


def cand_id(c):
    return f"B{c.B}-K{c.K}-N{c.N1}x{c.N2}-u{c.users}-{'b' if c.bias else 'nob'}-s{c.seed}"


def _pvec(v, pad=8):
    """``v`` as the head of a poisoned vector."""
    return torch.cat((torch.as_tensor(np.asarray(v), dtype=torch.float32), torch.full((pad,), POISON)))


def build_cand(B, K, N1, N2, users, bias, seed, lds=None, exact=True):
    rng = np.random.default_rng(seed)
    k, r = np.arange(K)[None, :], np.arange(B)[:, None]
    if exact:
        nz = (rng.random((B, K)) < 0.12) | ((k + 3 * r) % 7 == 0) | (k == K - 1)       # every 32-wide block of every row holds a term
        x = np.where(nz, rng.integers(1, 3, (B, K)), 0).astype(np.float64)
        Wi = rng.integers(-3, 4, (N1, K)).astype(np.float64)
        Wi[:, K - 1][Wi[:, K - 1] == 0] = 1.0
        Wc = rng.integers(-2, 3, (N2, N1)).astype(np.float64)
        bi = rng.integers(-4, 5, N1).astype(np.float64) if bias else None
        b0 = rng.integers(-4, 5, N2).astype(np.float64) if bias else None
    else:                                                                                 # the earlier tests' data (float)
        x = ((rng.random((B, K)) < 0.1) + rng.random((B, K)) * 0.1).astype(np.float32).astype(np.float64)
        Wi = (rng.standard_normal((N1, K)) / K ** 0.5).astype(np.float32).astype(np.float64)
        Wc = (rng.standard_normal((N2, N1)) / N1 ** 0.5).astype(np.float32).astype(np.float64)
        bi = (rng.standard_normal(N1) * 0.1).astype(np.float32).astype(np.float64)
        b0 = (rng.standard_normal(N2) * 0.1).astype(np.float32).astype(np.float64)
    zb = lambda b, n: np.zeros(n) if b is None else b
    emb = x @ Wi.T + zb(bi, N1)
    pc = emb @ Wc.T + zb(b0, N2)
    emb_abs = np.abs(x) @ np.abs(Wi).T + np.abs(zb(bi, N1))          # bounds every partial sum of an emb element in any order
    pc_abs = emb_abs @ np.abs(Wc).T + np.abs(zb(b0, N2))
    ld = {"x": K + (3 if seed % 2 else 5), "w": K + 1 + seed % 3, "emb": N1 + 4, "pc": N2 + 8}
    ld.update(lds or {})
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    pair_row = rng.integers(0, users, B).astype(np.int64)
    case = dict(B=B, K=K, N1=N1, N2=N2, R=users, ld=ld, exact=exact, bound=float(max(emb_abs.max(), pc_abs.max())),
                x_buf=R.wide(t(x), ld["x"]), wi_buf=R.wide(t(Wi), ld["w"]), wc_buf=_pvec(Wc.reshape(-1), 16),
                bi_buf=None if bi is None else _pvec(bi), b0_buf=None if b0 is None else _pvec(b0),
                emb64=torch.from_numpy(emb), pc64=torch.from_numpy(pc), pair_row=torch.from_numpy(pair_row), ppw=PPW_GROUP)
    case["x"], case["wi"], case["wc"] = case["x_buf"][:, :K], case["wi_buf"][:, :K], case["wc_buf"][:N2 * N1].view(N2, N1)
    return case


@functools.lru_cache(maxsize=None)
def cand_inputs(c):
    return build_cand(c.B, c.K, c.N1, c.N2, c.users, c.bias, c.seed)


def check_cand_inputs(case):
    assert case["bound"] < EXACT_MAX, case["bound"]
    for name, w in (("x", case["K"]), ("wi", case["K"])):
        buf = case[name + "_buf"]
        assert buf.shape[1] > w and bool((buf[:, w:] == POISON).all()) and torch.equal(buf[:, :w], buf[:, :w].round()), name
    assert bool((case["x"] >= 0).all()) and bool((case["x"] <= 2).all()) and bool((case["wi"].abs() <= 3).all()) and bool((case["wc"].abs() <= 2).all())
    dens = float((case["x"] != 0).float().mean())
    assert 0.10 <= dens <= 0.45 or case["K"] < 8, dens
    assert bool((case["x"].view(case["B"], -1)[:, -1] != 0).all()) and bool((case["wi"][:, -1] != 0).all())
    assert torch.equal(case["emb64"], case["emb64"].float().double()) and torch.equal(case["pc64"], case["pc64"].float().double())


def cand_outputs(case):
    return (torch.full((case["B"], case["ld"]["emb"]), SENTINEL), torch.full((case["B"], case["ld"]["pc"]), SENTINEL))


def group_outputs(B, n_rows, ppw):
    """Sentinel-filled (grp_ptr, pair_ids, wg_ptr, wg_row) of the fused grouping (wg_row sized as native.group_pairs sizes it)."""
    return (torch.full((n_rows + 1,), -7, dtype=torch.int64), torch.full((max(B, 1),), -7, dtype=torch.int64),
            torch.full((n_rows + 1,), -7, dtype=torch.int64), torch.full(((B + ppw - 1) // ppw + min(n_rows, B) + 1,), -7, dtype=torch.int32))


def check_grouping(got, ref, n_rows, what):
    """``got`` = (grp_ptr, pair_ids, wg_ptr, wg_row, oob), ``ref`` = ncf_group_pairs' (grp_ptr, pair_ids, wg_ptr, wg_row)."""
    n_wg = int(ref[2][-1])
    assert torch.equal(got[0], ref[0]), f"{what}: grp_ptr"
    assert torch.equal(got[2], ref[2]), f"{what}: wg_ptr"
    assert torch.equal(got[3][:n_wg], ref[3][:n_wg]), f"{what}: wg_row"
    assert bool((got[3][n_wg:] == -7).all()), f"{what}: wg_row written past the workgroups"
    gp = ref[0].tolist()
    a, b = got[1].tolist(), ref[1].tolist()
    for r in range(n_rows):
        if gp[r + 1] > gp[r]:
            assert sorted(a[gp[r]:gp[r + 1]]) == sorted(b[gp[r]:gp[r + 1]]), f"{what}: pairs of row {r}"
    assert int(got[4]) == 0, f"{what}: the out-of-range flag is set"


def check_cand(case, emb_buf, pc_buf, grouping, close=None, what="candidates"):
    """``emb_buf`` (B, ldemb) and ``pc_buf`` (B, ldpc) as a candidate kernel left them; ``grouping``: None or (got, ref) of
    check_grouping.  Exact cases: torch.equal; the float cases of the record of the gap: ``close``."""
    N1, N2 = case["N1"], case["N2"]
    for name, buf, w, ref in (("emb", emb_buf, N1, case["emb64"]), ("pc", pc_buf, N2, case["pc64"])):
        assert bool((buf[:, w:] == SENTINEL).all()), f"{what}: a padding column of {name} was written"
        un = (buf[:, :w] == SENTINEL).any(1)
        assert not bool(un.any()), f"{what}: rows of {name} never written: {un.nonzero().view(-1).tolist()[:8]}"
        if case["exact"]:
            bad = (buf[:, :w].double() != ref).nonzero()
            assert torch.equal(buf[:, :w].double(), ref), f"{what}: {name} differs from the exact product at {bad[:4].tolist()} ({bad.shape[0]} elements)"
        else:
            close(buf[:, :w], ref, f"{what} {name}")
    if grouping is not None:
        check_grouping(grouping[0], grouping[1], case["R"], what)


def cand_pack_layout(W, K, N1):
    """The packed copy as attn_cand.hip's comment states it (:200): Wp[(((s NT + nt) 2 + h) 64 + lane) 4 + j] =
    Wi[16 nt + (lane & 15)][32 s + 16 h + 4 (lane >> 4) + j], zero past K.  ``W``: (N1, >= K) tensor."""
    S, NT = (K + 31) // 32, N1 // 16
    Wz = torch.zeros(N1, 32 * S)
    Wz[:, :K] = W[:, :K]
    # [nt, i, s, h, g, j] -> [s, nt, h, g, i, j]   (lane = 16 g + i)
    return Wz.view(NT, 16, S, 2, 4, 4).permute(2, 0, 3, 4, 1, 5).reshape(-1).contiguous()


def tail_pack_layout(W):
    """attn_tail.hip:199: packed[((kb * (N / 16) + tile) * 64 + lane) * 4 + j] = W[16 tile + (lane & 15)][16 kb + 4 (lane >> 4) + j]."""
    N, K = W.shape
    return W.reshape(N // 16, 16, K // 16, 4, 4).permute(2, 0, 3, 1, 4).reshape(-1).contiguous()


# ------------------------------------------------------------------------------------------------ entry-split attention
SplitCase = collections.namedtuple("SplitCase", "mode A Fdim ppw nsplit merge wg_row bias seed")
SPLIT_A = (32, 64, 96, 128, 160, 192, 224, 256)
SPLIT_PPW = (5, 16, 32, 40, 64)
SPLIT_NSPLIT = (1, 2, 3, 8, 64)
SPLIT_LENGTHS = R.LENGTHS + (300, 40)                             # + a row of 5 tiles; the last row has entries and no pair


def _split_cases():
    cases, n = [], 0
    for mi, mode in enumerate((ATT_MLP, ATT_COS, ATT_MLP_SCALED)):
        k = 0
        for ppw in SPLIT_PPW:
            for Fdim in (64, 128):
                A = SPLIT_A[(k + 3 * mi) % 8]
                cases.append(SplitCase(mode, A, Fdim, ppw, SPLIT_NSPLIT[(k + mi) % 5], int((k + mi) % 3 != 0), (k + mi) % 2 == 0, (k // 2 + mi) % 3 != 0, 3000 + n))
                k += 1
                n += 1
    # the widths the rotation above leaves out of a mode, the swizzled divide path on every mode, the largest LDS image
    for mode in (ATT_MLP, ATT_COS, ATT_MLP_SCALED):
        have = {c.A for c in cases if c.mode == mode}
        for A in SPLIT_A:
            if A not in have or A in (96, 192):
                cases.append(SplitCase(mode, A, (64, 128)[n % 2], SPLIT_PPW[n % 5], SPLIT_NSPLIT[1 + n % 4], n % 2, n % 3 != 0, n % 2 == 0, 3000 + n))
                n += 1
    cases.append(SplitCase(ATT_MLP_SCALED, 256, 128, 64, 3, 0, False, True, 3000 + n))
    return cases


SPLIT_CASES = _split_cases()
MODE_NAMES = {ATT_MLP: "mlp", ATT_COS: "cos", ATT_MLP_SCALED: "mlps"}


def split_id(c):
    return f"{MODE_NAMES[c.mode]}-A{c.A}-F{c.Fdim}-ppw{c.ppw}-ns{c.nsplit}-m{c.merge}-{'wgrow' if c.wg_row else 'search'}-{'b' if c.bias else 'nob'}-s{c.seed}"


def split_pairs_per_row(ppw, seed):
    """Pairs of every row of SPLIT_LENGTHS: group sizes 1, NW, NW + 1, 2 NW, 2 NW + 1, 3 NW + 1 (where <= ppw), ppw, a row of two
    groups (ppw and 1); the rows are dealt from a seed-dependent start; the last row has none."""
    nw = (16 if ppw <= 16 else 32 if ppw <= 32 else 64) // 4
    big = [c for c in (1, nw, nw + 1, 2 * nw, 2 * nw + 1, 3 * nw + 1) if c <= ppw] + [ppw, ppw + 1, 2, 3]
    n = len(SPLIT_LENGTHS) - 1
    per = [big[k] if k < len(big) else (1, 2, 4)[k % 3] for k in range(n)]
    s = seed % n
    return per[s:] + per[:s] + [0]


def _part_reference(case, nsplit):
    """float64 (m (B, nsplit), l (B, nsplit), O (B, nsplit, Fdim)) of every (pair, slice): m = the slice's largest logit (-inf when it
    has no valid entry), l = sum e^(s - m), O = sum e^(s - m) val feat."""
    B, Fdim = case["B"], case["Fdim"]
    m = torch.full((B, nsplit), -float("inf"), dtype=torch.float64)
    l = torch.zeros(B, nsplit, dtype=torch.float64)
    O = torch.zeros(B, nsplit, Fdim, dtype=torch.float64)
    xp, feat = case["x_rowptr"].tolist(), case["feat"].double()
    for b in range(B):
        n = xp[b + 1] - xp[b]
        for s, (t0, t1) in enumerate(split_slices(n, nsplit)):
            lo, hi = xp[b] + 64 * t0, xp[b] + min(64 * t1, n)
            ok = case["x_ok"][lo:hi]
            if hi > lo and bool(ok.any()):
                sv = case["s64"][lo:hi][ok]
                m[b, s] = sv.max()
                e = torch.exp(sv - sv.max())
                l[b, s] = e.sum()
                O[b, s] = (e * case["x_val"][lo:hi][ok].double()) @ feat[case["x_col"][lo:hi][ok].long()]
    return m, l, O


@functools.lru_cache(maxsize=None)
def split_inputs(c):
    case = R.make_inputs(c.mode, c.A, c.Fdim, SPLIT_LENGTHS, split_pairs_per_row(c.ppw, c.seed), c.seed, bias=c.bias, masked_row_pairs=3)
    case["nsplit"], case["ldpart"] = c.nsplit, c.Fdim + PART_HEAD
    if c.nsplit > 1:
        case["m64"], case["l64"], case["O64"] = _part_reference(case, c.nsplit)
    return case


def split_groups(case, ppw):
    """(row, start into the flat pair list, cnt) of every workgroup, and the flat list (pairs of a row ascending)."""
    flat, out = [], []
    for r in range(case["R"]):
        pairs = (case["pair_row"] == r).nonzero().view(-1).tolist()
        for g in range(0, len(pairs), ppw):
            out.append((r, len(flat) + g, min(ppw, len(pairs) - g)))
        flat += pairs
    return out, np.array(flat, dtype=np.int64)


def split_workspace(case):
    """The partials' workspace, every word the sentinel (+ OUT_PAD words that must stay so)."""
    return torch.full((case["B"] * case["nsplit"] * case["ldpart"] + OUT_PAD,), SENTINEL)


def check_split_out(case, out_buf, close, what):
    """check_forward (padding untouched, every row written, dead pairs = the bias bits, values at the bar)."""
    R.check_forward(case, out_buf, None, close, what)


def check_split_partials(case, ws, close, what):
    """``ws``: split_workspace() after the kernel.  m bit-equal (exact logits), l and O at the bar, head words 2-3 ignored, and the
    merge of the kernel's own partials, formed in float64, at the bar of out64."""
    B, ns, ldp, Fdim = case["B"], case["nsplit"], case["ldpart"], case["Fdim"]
    assert bool((ws[B * ns * ldp:] == SENTINEL).all()), f"{what}: partials written past the workspace"
    p = ws[:B * ns * ldp].view(B, ns, ldp)
    m, l, O = p[:, :, 0].double(), p[:, :, 1].double(), p[:, :, PART_HEAD:].double()
    un = (p[:, :, 0] == SENTINEL) | (p[:, :, 1] == SENTINEL) | (p[:, :, PART_HEAD:] == SENTINEL).any(2)
    assert not bool(un.any()), f"{what}: (pair, slice) partials never written: {un.nonzero()[:6].tolist()}"
    bad = (m != case["m64"]).nonzero()
    assert torch.equal(m, case["m64"]), f"{what}: m differs at (pair, slice) {bad[:6].tolist()}"
    empty = case["m64"] == -float("inf")
    assert bool((l[empty] == 0).all()) and bool((O[empty] == 0).all()), f"{what}: an empty slice must hold l = 0, O = 0"
    close(l, case["l64"], what + " l")
    close(O, case["O64"], what + " O")
    M = m.max(1, keepdim=True).values
    w = torch.where(m == -float("inf"), torch.zeros_like(m), torch.exp(m - torch.where(M == -float("inf"), torch.zeros_like(M), M)))
    L = (l * w).sum(1, keepdim=True)
    bias = torch.zeros(Fdim, dtype=torch.float64) if case["bias"] is None else case["bias"].double()
    merged = torch.where(L > 0, (O * w[:, :, None]).sum(1) / L.clamp_min(1e-300), torch.zeros(B, Fdim, dtype=torch.float64)) + bias
    close(merged, case["out64"], what + " merged")


# ------------------------------------------------------------------------------------------------ tail
TailCase = collections.namedtuple("TailCase", "E packed B source nsplit ubias lduser kind seed")
TAIL_B = (1, 15, 16, 17, 33)
TAIL_SOURCES = (("user", 0), ("part", 1), ("part", 2), ("part", 8), ("part", 9), ("part", 16), ("part", 64))


def _tail_cases():
    cases, n = [], 0
    for E in (64, 128):
        for si, (src, ns) in enumerate(TAIL_SOURCES):
            for packed in (False, True):
                cases.append(TailCase(E, packed, TAIL_B[(n + si) % 5], src, ns, n % 3 != 1, E + 4, "exact", 4000 + n))
                n += 1
        for k, B in enumerate((17, 33)):                            # lduser != ldcand: the two halves' leading dimensions told apart
            cases.append(TailCase(E, bool(k), B, "user", 0, True, E + 8, "exact", 4000 + n))
            n += 1
        for si, (src, ns) in enumerate(TAIL_SOURCES):               # float: unequal m, the rescale path
            cases.append(TailCase(E, bool(si % 2), (33, 17)[si % 2], src, ns, si % 3 != 2, E + 4, "float", 4000 + n))
            n += 1
    return cases


TAIL_CASES = _tail_cases()


def tail_id(c):
    return f"E{c.E}-{'packed' if c.packed else 'plain'}-B{c.B}-{c.source}{c.nsplit or ''}-{'ub' if c.ubias else 'noub'}-ldu{c.lduser}-{c.kind}-s{c.seed}"


def _merge64(m, l, O, ubias):
    M = m.max(1, keepdim=True).values
    w = torch.where(m == -float("inf"), torch.zeros_like(m), torch.exp(m - torch.where(M == -float("inf"), torch.zeros_like(M), M)))
    L = (l * w).sum(1, keepdim=True)
    return torch.where(L > 0, (O * w[:, :, None]).sum(1) / L.clamp_min(1e-300), torch.zeros_like(O[:, 0])) + ubias


def build_tail(c, lds=None):
    rng = np.random.default_rng(c.seed)
    E, B, ns = c.E, c.B, c.nsplit
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    sparse = lambda shape, lo, hi, dens: np.where(rng.random(shape) < dens, rng.integers(lo, hi + 1, shape), 0).astype(np.float64)
    exact = c.kind == "exact"
    if exact:
        cand = sparse((B, E), -2, 2, 0.3)
        W1, W2, w3 = sparse((TAIL_N1, 2 * E), -1, 1, 0.25), sparse((TAIL_N2, TAIL_N1), -1, 1, 0.25), sparse((TAIL_N2,), -1, 1, 0.5)
        b1, b2, b3 = rng.integers(-2, 3, TAIL_N1).astype(np.float64), rng.integers(-2, 3, TAIL_N2).astype(np.float64), 0.375
        ubias = rng.integers(-8, 9, E) / 8.0 if c.ubias else None
    else:
        f = lambda a: a.astype(np.float32).astype(np.float64)
        cand = f(rng.standard_normal((B, E)))
        W1, W2 = f(rng.standard_normal((TAIL_N1, 2 * E)) / (2 * E) ** 0.5), f(rng.standard_normal((TAIL_N2, TAIL_N1)) / TAIL_N1 ** 0.5)
        w3, b1, b2, b3 = f(rng.standard_normal(TAIL_N2) / TAIL_N2 ** 0.5), f(rng.standard_normal(TAIL_N1) * 0.1), f(rng.standard_normal(TAIL_N2) * 0.1), 0.37
        ubias = f(rng.standard_normal(E) * 0.1) if c.ubias else None
    ub = np.zeros(E) if ubias is None else ubias
    ld = {"cand": E + 4, "user": c.lduser}
    ld.update(lds or {})
    case = dict(E=E, B=B, nsplit=ns, source=c.source, exact=exact, ld=ld, b3=b3, ldpart=E + PART_HEAD)
    if c.source == "user":
        user = rng.integers(-16, 17, (B, E)) / 8.0 * (rng.random((B, E)) < 0.5) if exact else rng.standard_normal((B, E)).astype(np.float32).astype(np.float64)
        case["user_buf"] = R.wide(t64(user).float(), ld["user"])
        user64 = t64(user)
    else:
        m = np.full((B, ns), -np.inf)
        l, O = np.zeros((B, ns)), np.zeros((B, ns, E))
        dead = min(3, B - 1) if B > 1 else -1                        # the pair whose slices are all empty
        for b in range(B):
            if b == dead:
                continue
            if exact:
                L = int(2 ** rng.integers(0, 4))                     # 1, 2, 4 or 8: the merged row is a multiple of 2^-3
                nf = int(min(ns, rng.integers(1, L + 1)))
                pos = rng.permutation(ns)[:nf]
                if b == 0 and ns - 1 not in pos:
                    pos[0] = ns - 1                                  # pair 0 always has a term in the last slice ...
                if b == 1 and ns > 1:
                    pos = np.array([0] + [p for p in pos if p not in (0, ns - 1)][:max(nf - 1, 0)])   # ... pair 1 one in the first, none in the last
                    nf = len(pos)
                cuts = np.sort(rng.permutation(L - 1)[:nf - 1] + 1) if nf > 1 else np.zeros(0, dtype=np.int64)
                ls = np.diff(np.concatenate([[0], cuts, [L]]))       # positive integers that sum to L
                m[b, pos] = rng.integers(-8, 9) / 2.0                # all finite m of a pair equal: exp_le0(0) = 1
                l[b, pos] = ls
                O[b, pos] = rng.integers(-3, 4, (nf, E))
                O[b, pos[0], 0] += 1 if O[b, pos, 0].sum() == 0 else 0
            else:
                fin = rng.random(ns) < 0.8
                fin[rng.integers(0, ns)] = True
                m[b, fin] = (rng.standard_normal(int(fin.sum())) * 3).astype(np.float32)
                l[b, fin] = (rng.random(int(fin.sum())) * 5 + 0.1).astype(np.float32)
                O[b, fin] = (rng.standard_normal((int(fin.sum()), E)) * 2).astype(np.float32)
        part = np.full((B, ns, E + PART_HEAD), POISON)               # head words 2-3: unused, poisoned
        part[:, :, 0], part[:, :, 1], part[:, :, PART_HEAD:] = m, l, O
        case["part_buf"] = torch.cat((torch.from_numpy(part.astype(np.float32)).reshape(-1), torch.full((OUT_PAD,), POISON)))
        case["m"], case["l"], case["O"] = t64(m), t64(l), t64(O)
        user64 = _merge64(t64(m), t64(l), t64(O), t64(ub))
    x64 = torch.cat((t64(cand), user64), 1)
    h1 = torch.relu(x64 @ t64(W1).t() + t64(b1))
    h2 = torch.relu(h1 @ t64(W2).t() + t64(b2))
    case["out64"] = h2 @ t64(w3) + b3
    if exact:                                                        # sums of |terms| at every layer, in units of 2^-3
        a1 = x64.abs() @ t64(W1).abs().t() + t64(b1).abs()
        a2 = a1 @ t64(W2).abs().t() + t64(b2).abs()
        a3 = a2 @ t64(w3).abs() + abs(b3)
        case["bound"] = 8.0 * float(max(a1.max(), a2.max(), a3.max()))
        if c.source != "user":
            case["bound"] = max(case["bound"], 8.0 * float(case["O"].abs().sum(1).max() + t64(ub).abs().max()))
        case["user64"] = user64
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    case.update(cand_buf=R.wide(f32(cand), ld["cand"]), w1_buf=_pvec(W1.reshape(-1), 16), w2_buf=_pvec(W2.reshape(-1), 16), w3_buf=_pvec(w3),
                b1_buf=_pvec(b1), b2_buf=_pvec(b2), ubias_buf=None if ubias is None else _pvec(ubias))
    case["W1"], case["W2"] = case["w1_buf"][:TAIL_N1 * 2 * E].view(TAIL_N1, 2 * E), case["w2_buf"][:TAIL_N2 * TAIL_N1].view(TAIL_N2, TAIL_N1)
    return case


@functools.lru_cache(maxsize=None)
def tail_inputs(c):
    return build_tail(c)


def check_tail_inputs(case):
    if case["exact"]:
        assert case["bound"] < EXACT_MAX, case["bound"]
        assert torch.equal(case["out64"] * 8, (case["out64"] * 8).round()) and torch.equal(case["out64"], case["out64"].float().double())
        assert torch.equal(case["user64"] * 8, (case["user64"] * 8).round())
        if case["source"] != "user":
            m, l = case["m"], case["l"]
            fin = torch.isfinite(m)
            for b in range(case["B"]):
                mv = m[b][fin[b]]
                assert mv.numel() == 0 or bool((mv == mv[0]).all())
                L = float(l[b].sum())
                assert L in (0.0, 1.0, 2.0, 4.0, 8.0) and bool((l[b][~fin[b]] == 0).all()) and bool((case["O"][b][~fin[b]] == 0).all())
            if case["B"] > 1:
                assert bool((~fin).all(1).any())                      # a pair with every slice empty
            if case["nsplit"] > 1 and case["B"] > 1:
                assert bool(fin[0, -1]) and bool(fin[1, 0]) and not bool(fin[1, -1])
            if case["nsplit"] > 2 and case["B"] > 1:
                assert bool((~fin).any())
    assert bool((case["cand_buf"][:, case["E"]:] == POISON).all())


def tail_output(case):
    return torch.full((case["B"] + OUT_PAD,), SENTINEL)


def check_tail(case, out_buf, close, what):
    B = case["B"]
    assert bool((out_buf[B:] == SENTINEL).all()), f"{what}: out written past B"
    assert not bool((out_buf[:B] == SENTINEL).any()), f"{what}: outputs never written"
    if case["exact"]:
        bad = (out_buf[:B].double() != case["out64"]).nonzero().view(-1)
        assert torch.equal(out_buf[:B].double(), case["out64"]), f"{what}: differs from the exact MLP at pairs {bad[:8].tolist()}"
    else:
        close(out_buf[:B], case["out64"], what)
