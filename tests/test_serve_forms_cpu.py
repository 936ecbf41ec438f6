"""CPU tests of tests/serve_forms_ref.py: the builders' conditions on every table row (the 2^24 bounds of the exact cases, every
logit of the entry-split cases exact), the coverage the tables claim (every launch form of csrc/attn_cand.hip, attn_split.hip and
attn_tail.hip), and the checks of tests/test_gpu_serve_forms.py run against numpy emulators that restate each kernel's INDEX
ARITHMETIC (K slices and the ragged block, row clamp, pack layouts as the consumers address them, slice-to-tile map, pair slots, the
DMA image write and the swizzled read, partial addressing, the tail's tile fill and merge; not its timing).  The right walk passes,
using at most half of a bar where a bar applies; each of fourteen index defects, injected one at a time, is rejected by every table
case that exercises the form concerned.  The last test runs the same defects on the shapes and checks the suite had before."""
import numpy as np
import pytest
import torch

import attn_forms_ref as R
import serve_forms_ref as S
from test_attn_forms_cpu import Worst

F32 = np.float32
LANE = np.arange(64)
J4 = np.arange(4)


class Stray(AssertionError):
    """A read outside the operand's buffer (what a bounds audit of the emulated walk reports; on a device: a neighbour's memory)."""


def _take(flat, idx, audit=True):
    idx = np.asarray(idx)
    if audit and idx.size and (idx.min() < 0 or idx.max() >= flat.size):
        raise Stray(f"read at {int(idx.max())} of a buffer of {flat.size}")
    return flat[np.clip(idx, 0, flat.size - 1)]


def _put(flat, idx, v):
    idx, v = np.asarray(idx).ravel(), np.broadcast_to(v, np.shape(idx)).ravel()
    keep = (idx >= 0) & (idx < flat.size)                          # a stray store past the buffer is dropped
    flat[idx[keep]] = v[keep]


# ------------------------------------------------------------------------------------------------ the builders, on every row
def test_builder_conditions_hold_on_every_case():
    worst = 0.0
    for c in S.CAND_CASES:
        case = S.cand_inputs(c)
        S.check_cand_inputs(case)
        worst = max(worst, case["bound"])
    print(f"candidates: largest sum of |terms| {worst:.0f} = {worst / S.EXACT_MAX:.3f} of 2^24")
    worst = 0.0
    for c in S.TAIL_CASES:
        case = S.tail_inputs(c)
        S.check_tail_inputs(case)
        worst = max(worst, case.get("bound", 0.0))
    print(f"tail: largest sum of |terms| in units of 2^-3 {worst:.0f} = {worst / S.EXACT_MAX:.3f} of 2^24")
    for c in S.SPLIT_CASES:
        case = S.split_inputs(c)
        R.check_inputs(case)                                        # every logit exact, spread <= 8, poisoned padding
        assert all(v == w + 4 for v, w in ((case["ld"]["pc"], c.A), (case["ld"]["pr"], c.A), (case["ld"]["feat"], c.Fdim), (case["ld"]["out"], c.Fdim)))
        assert case["B"] <= 400 and case["I"] == 300
        lens = (case["x_rowptr"][1:] - case["x_rowptr"][:-1]).tolist()
        assert set(S.SPLIT_LENGTHS[:-1]) <= set(lens)
        assert bool(case["pair_empty"].any()) and bool((case["pair_dead"] & ~case["pair_empty"]).any())
        if c.nsplit > 1:
            m = case["m64"]
            assert torch.equal(m, m.float().double()) and bool((m == -float("inf")).any())
            assert bool((m[case["pair_dead"]] == -float("inf")).all())


# ------------------------------------------------------------------------------------------------ the tables reach every form
def test_tables_reach_every_form():
    for N1 in (64, 128):
        assert {S.cand_form(True, c.B, c.N1)[1] for c in S.CAND_CASES if c.N1 == N1} == set(range(1, 9))
        assert {S.cand_form(True, c.B, c.N1)[1] for c in S.CAND_CASES if c.N1 == N1 and c.K == 2094} == set(range(1, 9))
        assert {S.cand_form(p, c.B, c.N1)[0] for c in S.CAND_CASES if c.N1 == N1 for p in (False, True)} == {"staged", "packed", "splitk"}
    assert {c.K for c in S.CAND_CASES} == set(S.CAND_K) and {c.N2 for c in S.CAND_CASES} == set(S.CAND_N2) and {c.B for c in S.CAND_CASES} >= set(S.CAND_B)
    assert {c.K for c in S.CAND_CASES if S.cand_form(True, c.B, c.N1)[0] == "splitk"} == set(S.CAND_K)
    assert {c.bias for c in S.CAND_CASES} == {True, False} and any(c.users > S.GROUP_LDS_ROWS and c.B == 33 for c in S.CAND_CASES)
    assert {1, 5} <= {c.users for c in S.CAND_CASES} and any(c.users == c.B > 5 for c in S.CAND_CASES)
    assert any(c.B > 2048 and c.B % 16 for c in S.CAND_CASES)
    assert max(c.B * S.cand_inputs(c)["ld"]["x"] for c in S.CAND_CASES) <= 2061 * 2100
    sl, ragged = S.cand_slices(2094, 8)                              # 65 steps over 64 slices: one or two steps each, + the ragged 14
    assert {hi - lo for lo, hi in sl} == {1, 2} and ragged and S.cand_slices(256, 1) == ([(w, w + 1) for w in range(8)], False)
    assert any(hi == lo for lo, hi in S.cand_slices(65, 8)[0])

    forms = {S.split_form(c.mode, c.A, c.Fdim, c.ppw) for c in S.SPLIT_CASES}
    assert {f.inst for f in forms} == {(m, nw, fd) for m in (0, 2, 3) for nw in (4, 8, 16) for fd in (64, 128)}            # all 18
    assert {(c.mode, c.ppw, c.Fdim) for c in S.SPLIT_CASES} >= {(m, p, f) for m in (0, 2, 3) for p in S.SPLIT_PPW for f in (64, 128)}
    assert {f.path for f in forms} == {"readlane4", "readlane2", "readlane1", "shift", "divide"}
    assert any(f.path == "divide" and f.swizzled for f in forms) and any(f.path == "divide" and not f.swizzled for f in forms)
    assert {f.raised for f in forms} == {True, False}
    for mode in (R.ATT_MLP, R.ATT_COS, R.ATT_MLP_SCALED):
        assert {c.A for c in S.SPLIT_CASES if c.mode == mode} == set(S.SPLIT_A), mode
        assert any(c.A == 192 for c in S.SPLIT_CASES if c.mode == mode) and any(c.A == 96 for c in S.SPLIT_CASES if c.mode == mode)
    assert {c.nsplit for c in S.SPLIT_CASES} == set(S.SPLIT_NSPLIT) and {c.merge for c in S.SPLIT_CASES if c.nsplit > 1} == {0, 1}
    assert {c.wg_row for c in S.SPLIT_CASES} == {True, False} and {c.bias for c in S.SPLIT_CASES} == {True, False}
    assert {tuple(S.split_slices(300, n)) for n in (3, 8)} and {t1 - t0 for n in (3, 8) for t0, t1 in S.split_slices(300, n)} == {0, 1, 2}
    for c in S.SPLIT_CASES:
        nw = S.split_form(c.mode, c.A, c.Fdim, c.ppw).inst[1]
        cnts = {cnt for _, _, cnt in S.split_groups(S.split_inputs(c), c.ppw)[0]}
        assert cnts >= {k for k in (1, nw, nw + 1, 2 * nw, 2 * nw + 1, 3 * nw + 1) if k <= c.ppw} | {c.ppw}, (c, cnts)
        nps = set().union(*(S.split_slots(cnt, nw) for cnt in cnts))
        assert 0 in nps and {S.slot_width(n) for n in nps} >= ({0, 1, 2, 4} if c.ppw >= 3 * nw else {0, 1, 2}), (c, nps)

    assert {S.tail_form(c.E, c.packed, c.source, c.nsplit) for c in S.TAIL_CASES if c.kind == "exact"} == \
        {(E, p, s) for E in (64, 128) for p in (False, True) for s in ("user", "partials<=8", "partials>8")}
    assert {(c.E, c.source, c.nsplit) for c in S.TAIL_CASES if c.kind == "float"} == {(E, s, n) for E in (64, 128) for s, n in S.TAIL_SOURCES}
    assert {c.B for c in S.TAIL_CASES} == set(S.TAIL_B) and {c.ubias for c in S.TAIL_CASES} == {True, False}
    assert {(c.E, c.source, c.nsplit, c.packed) for c in S.TAIL_CASES if c.kind == "exact" and c.lduser == c.E + 4} == \
        {(E, s, n, p) for E in (64, 128) for s, n in S.TAIL_SOURCES for p in (False, True)}


def test_mirrors_agree_with_the_library():
    """ncf_attn_split_supported / ncf_attn_tail_supported / ncf_attn_candidates_supported and the workspace sizes, where the
    library is built (host functions: no GPU needed)."""
    import os
    from deeprecommendation_amd import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = n.load_library()
    for mode in (0, 1, 2, 3):
        for A in (0, 16, 32, 48, 64, 96, 160, 192, 224, 256, 288):
            for Fdim in (32, 64, 96, 128):
                for ppw in (0, 1, 5, 16, 17, 32, 33, 64, 65):
                    assert bool(lib.ncf_attn_split_supported(mode, A, Fdim, ppw)) == S.split_supported(mode, A, Fdim, ppw), (mode, A, Fdim, ppw)
    for B in list(range(1, 70)) + [511, 512, 513, 576, 577, 592, 593, 672, 673, 1024, 1025, 1040, 1041, 1360, 1361, 2048, 2049, 5000]:
        for N1 in (64, 128):
            ks = S.cand_splitk_pieces(B)
            want = ks * ((B + 15) // 16) * 16 * N1 * 4 if ks > 1 else 0
            assert lib.ncf_attn_candidates_packed_workspace_bytes(B, N1, -1) == want, (B, N1)
    assert lib.ncf_attn_candidates_pack_floats(2094, 128) == 66 * 32 * 128 and lib.ncf_attn_split_workspace_bytes(7, 64, 3) == 7 * 3 * 68 * 4


# ------------------------------------------------------------------------------------------------ emulators: candidates
def emu_cand_pack(wflat, ldw, K, N1, fault=None):
    """cand_pack_kernel: one thread per packed word."""
    Sx, NT = (K + 31) // 32, N1 // 16
    idx = np.arange(Sx * NT * 512)
    j, lane, h, q = idx & 3, (idx >> 2) & 63, (idx >> 8) & 1, idx >> 9
    if fault == "pack_transpose":
        lane = (lane & 15) * 4 + (lane >> 4)
    nt, s = q % NT, q // NT
    n, k = 16 * nt + (lane & 15), 32 * s + 16 * h + 4 * (lane >> 4) + j
    return np.where(k < K, _take(wflat, n * ldw + np.minimum(k, K - 1)), 0.0)


def emu_cand(case, packed, fault=None, bufs=None, audit=True):
    """The three forms' walk: row clamp, (piece, wave) slices of the whole 32-wide steps, the ragged block, the pieces added in order,
    the second product, the stores with their leading dimensions.  Products of a slice are formed in float64 and rounded (exact on
    the exact cases), slices and pieces are added in fp32 in the kernels' order."""
    B, K, N1, N2, ld = case["B"], case["K"], case["N1"], case["N2"], case["ld"]
    form, KS = S.cand_form(packed, B, N1)
    xf, wf = case["x_buf"].numpy().ravel().astype(np.float64), case["wi_buf"].numpy().ravel().astype(np.float64)
    wc = case["wc_buf"].numpy().astype(np.float64)
    tiles, NT, SF = (B + 15) // 16, N1 // 16, K // 32
    rows = np.arange(16 * tiles)
    m = rows if fault == "no_row_clamp" else np.minimum(rows, B - 1)
    n = np.arange(N1)
    X = lambda k: _take(xf, m[:, None] * ld["x"] + k[None, :], audit)
    if packed:
        Wp = emu_cand_pack(wf, ld["w"], K, N1, fault)

        def W(k):                                                   # the consumers' addressing of the packed copy
            s, h, g, j = k // 32, (k % 32) // 16, (k % 16) // 4, k % 4
            lane = 16 * g[None, :] + (n % 16)[:, None]
            return Wp[(((s[None, :] * NT + (n // 16)[:, None]) * 2 + h[None, :]) * 64 + lane) * 4 + j[None, :]]
    else:
        W = lambda k: _take(wf, n[:, None] * ld["w"] + k[None, :], audit)
    slices, ragged = S.cand_slices(K, KS)
    pieces = []
    for ks in range(KS):
        acc = np.zeros((16 * tiles, N1), F32)
        for wave in range(8):
            sl = ks * 8 + wave
            lo, hi = slices[sl]
            if fault == "splitk_last_short" and form == "splitk" and sl == 8 * KS - 1:
                hi -= 1
            part = np.zeros((16 * tiles, N1))
            if hi > lo:
                k = np.arange(32 * lo, 32 * hi)
                part = part + X(k) @ W(k).T
            first = wave == 0 if (form != "splitk" or fault == "ragged_every_piece") else sl == 0
            if ragged and first:
                k = np.arange(32 * SF, 32 * SF + 32)
                g = k <= K if fault == "ragged_guard_le" else k < K
                kc = np.where(g, k, 0)
                xv = np.where(g[None, :], X(kc), 0.0)
                wv = W(k) if packed else np.where(g[None, :], W(kc), 0.0)
                part = part + xv @ wv.T
            acc = (acc + part.astype(F32)).astype(F32)
        pieces.append(acc)
    v = pieces[0]
    for ks in range(1, KS):
        v = (v + pieces[ks]).astype(F32)
    if fault == "finish_ks_plus_1" and form == "splitk" and KS < 8:
        v = (v + pieces[KS - 1]).astype(F32)
    if case["bi_buf"] is not None:
        v = (v + _take(case["bi_buf"].numpy(), n)[None, :]).astype(F32)
    emb_t, pc_t = bufs or S.cand_outputs(case)
    emb, pc = emb_t.numpy().ravel(), pc_t.numpy().ravel()
    live = rows < B
    _put(emb, (rows[:, None] * ld["emb"] + n[None, :])[live], v[live])
    n2 = np.arange(N2)
    Wc = _take(wc, n2[:, None] * N1 + n[None, :])
    p = (v.astype(np.float64) @ Wc.T).astype(F32)
    if case["b0_buf"] is not None:
        p = (p + _take(case["b0_buf"].numpy(), n2)[None, :]).astype(F32)
    _put(pc, (rows[:, None] * (ld["emb"] if fault == "ldemb_for_pc" else ld["pc"]) + n2[None, :])[live], p[live])
    return emb_t, pc_t


# ------------------------------------------------------------------------------------------------ emulators: entry-split attention
def _stage(tab, ldt, x4, xorj, cols, fault):
    """attn_split_kernel's ``issue``: the 64-entry tile image, piece by piece (64 16-byte chunks per wave instruction)."""
    gi = np.arange(64 * x4)
    sh = x4.bit_length() - 1 if x4 & (x4 - 1) == 0 else -1
    rpp = 64 >> sh if sh >= 0 else 0
    if 1 <= rpp <= 4:                                               # readlane: a piece covers rpp whole rows
        piece, lane = gi // 64, gi % 64
        e, j = piece * rpp + (lane >> sh), lane & (x4 - 1)
    elif sh >= 0:
        e, j = gi >> sh, gi & (x4 - 1)
    else:
        e = gi >> 5 if fault == "divide_shift5" else gi // x4
        j = gi - e * x4
    ci = cols[np.clip(e, 0, 63)]
    jj = j ^ (e & (7 if fault == "swizzle_e7" else 15)) if xorj else j
    img = np.zeros(256 * x4, F32)
    img[4 * gi[:, None] + J4] = _take(tab, (np.where(ci >= 0, ci, 0) * ldt + 4 * jj)[:, None] + J4)   # a masked entry gathers row 0
    return img


def emu_split(case, c, fault=None, bufs=None):
    """attn_split_kernel + attn_combine_kernel: (workgroup, slice) -> tiles, pair slots, DMA image and swizzled read, the online
    softmax over the slice's tiles, the partials' addresses, the merge.  Returns (out buffer, workspace)."""
    A, Fdim, I, B, ld, ns = case["A"], case["Fdim"], case["I"], case["B"], case["ld"], c.nsplit
    form = S.split_form(c.mode, A, Fdim, c.ppw)
    NW, ldp = form.inst[1], Fdim + S.PART_HEAD
    km = 2 if c.mode == R.ATT_COS else 0
    pcf, prf, ftf = (case[k].numpy().ravel() for k in ("pc_buf", "pr_buf", "feat_buf"))
    w1 = None if case["w1"] is None else case["w1_buf"].numpy()[:A]
    b1 = F32(case["b1"]) if km == 0 else F32(0)
    bias = np.zeros(Fdim, F32) if case["bias"] is None else case["bias_buf"].numpy()[:Fdim]
    rp, col, val = case["rowptr"].numpy(), case["col"].numpy().astype(np.int64), case["val"].numpy()
    out_t, ws_t = bufs or (R.fresh_outputs(case, False)[0], S.split_workspace(case))
    out, ws = out_t.numpy().ravel(), ws_t.numpy()
    groups, flat = S.split_groups(case, c.ppw)
    A4, F4 = A // 4, Fdim // 4
    for r, start, cnt in groups:
        pairs = flat[start:start + cnt]
        npw = [cnt // NW if fault == "np_div" else ((cnt - w + NW - 1) // NW if cnt > w else 0) for w in range(NW)]
        scored = np.array([j // NW < npw[j % NW] for j in range(cnt)])
        rbeg, rend = int(rp[r]), int(rp[r + 1])
        T = (rend - rbeg + 63) // 64
        pcs = np.stack([_take(pcf, b * ld["pc"] + np.arange(A)) for b in pairs])
        for split in range(ns):
            t0 = split * T // ns
            t1 = split * T // ns + 1 if fault == "t1_plus1" else (split + 1) * T // ns
            beg, end = rbeg + 64 * t0, min(rbeg + 64 * t1, rend)
            m, l, o = np.full(cnt, -np.inf, F32), np.zeros((cnt, 64), F32), np.zeros((cnt, Fdim), F32)
            for ti in range(t1 - t0):
                ee = beg + 64 * ti + LANE
                if end > beg:
                    ec = np.where(ee < end, ee, end - 1)
                    cols, vl = col[ec], val[ec]
                else:
                    cols, vl = np.full(64, -1), np.zeros(64, F32)
                ok = (ee < end) & (cols >= 0) & (cols < I)
                cols, vl = np.where(ok, cols, -1), np.where(ok, vl, F32(0)).astype(F32)
                prt = _stage(prf, ld["pr"], A4, form.swizzled, cols, fault)
                fct = _stage(ftf, ld["feat"], F4, False, cols, fault).reshape(64, Fdim)
                sw = (LANE & 15) if form.swizzled else np.zeros(64, np.int64)
                rows = prt[LANE[:, None, None] * A + 4 * (np.arange(A4)[None, :, None] ^ sw[:, None, None]) + J4].reshape(64, A)
                if km == 0:
                    s = np.sum(w1 * np.maximum(pcs[:, None, :] + rows[None], F32(0)), axis=-1, dtype=F32) + b1
                else:
                    s = np.sum(pcs[:, None, :] * rows[None], axis=-1, dtype=F32)
                scv = np.where(ok[None] & scored[:, None], s, -np.inf).astype(F32)
                mnew = np.maximum(m, scv.max(1))
                anyv = mnew != -np.inf
                with np.errstate(invalid="ignore"):
                    scale = np.where(anyv, np.exp(np.where(anyv, m - mnew, 0), dtype=F32), F32(1)).astype(F32)
                    pe = np.where(anyv[:, None] & ok[None] & scored[:, None], np.exp(np.where(anyv[:, None], scv - mnew[:, None], -np.inf), dtype=F32), F32(0)).astype(F32)
                m = np.where(scored, mnew, m)
                l = l * scale[:, None] + pe
                o = o * np.where(scored, scale, F32(0))[:, None] + ((pe * vl[None]) @ fct).astype(F32)
            lt = l.sum(1, dtype=F32)
            f = np.arange(Fdim)
            if ns > 1:
                for k, b in enumerate(pairs):
                    base = (b * ns) * ldp + split if fault == "part_addr" else (b * ns + split) * ldp
                    if scored[k]:
                        _put(ws, np.array([base, base + 1]), np.array([m[k], lt[k]], F32))
                    _put(ws, base + S.PART_HEAD + f, o[k])
            else:
                inv = np.where(scored & (lt > 0), F32(1) / np.where(lt > 0, lt, F32(1)), F32(0)).astype(F32)
                for k, b in enumerate(pairs):
                    _put(out, b * ld["out"] + f, o[k] * inv[k] + bias)
    if ns > 1 and c.merge:                                          # attn_combine_kernel
        p = ws[:B * ns * ldp].reshape(B, ns, ldp)
        ms = p[:, :, 0]
        M = ms.max(1, keepdims=True)
        with np.errstate(invalid="ignore"):
            w = np.where(ms == -np.inf, F32(0), np.exp(ms - M, dtype=F32)).astype(F32)
            L = (p[:, :, 1] * w).sum(1, dtype=F32)
            o = (p[:, :, S.PART_HEAD:] * w[:, :, None]).sum(1, dtype=F32)
        inv = np.where(L > 0, F32(1) / np.where(L > 0, L, F32(1)), F32(0)).astype(F32)
        _put(out, np.arange(B)[:, None] * ld["out"] + np.arange(Fdim)[None, :], o * inv[:, None] + bias[None, :])
    return out_t, ws_t


# ------------------------------------------------------------------------------------------------ emulators: tail
def emu_tail_pack(wflat, N, K, fault=None):
    """tail_pack_kernel: one thread per packed word."""
    idx = np.arange(N * K)
    j, lane, q = idx & 3, (idx >> 2) & 63, idx >> 8
    if fault == "pack_transpose":
        lane = (lane & 15) * 4 + (lane >> 4)
    tiles = N // 16
    tile, kb = q % tiles, q // tiles
    return _take(wflat, (16 * tile + (lane & 15)) * K + 16 * kb + 4 * (lane >> 4) + j)


def emu_tail(case, c, fault=None, out_t=None):
    """attn_tail_kernel: the tile fill (row clamp, candidate half, user half from finished rows or from the merge of the partials in
    slice order), the two hidden layers through the plain or the packed weight addressing, the last layer, the guarded store."""
    E, B, ld, ns, ldp = case["E"], case["B"], case["ld"], case["nsplit"], case["ldpart"]
    dt = np.float64 if case["exact"] else F32                      # exact cases: any order gives the same bits
    tiles = (B + 15) // 16
    rows = np.arange(16 * tiles)
    b = np.minimum(rows, B - 1)
    e = np.arange(E)
    xc = _take(case["cand_buf"].numpy().ravel(), b[:, None] * ld["cand"] + e[None, :])
    ub = np.zeros(E, F32) if case["ubias_buf"] is None else case["ubias_buf"].numpy()[:E]
    if case["source"] == "user":
        xu = _take(case["user_buf"].numpy().ravel(), b[:, None] * (ld["cand"] if fault == "tail_user_ldcand" else ld["user"]) + e[None, :])
    else:
        pf = case["part_buf"].numpy()
        p0 = b * ns * ldp
        sl = np.arange(ns - 1 if fault == "tail_merge_skip" else ns)
        ms = _take(pf, p0[:, None] + sl[None, :] * ldp) if sl.size else np.full((rows.size, 0), -np.inf, F32)
        ls = _take(pf, p0[:, None] + sl[None, :] * ldp + 1) if sl.size else np.zeros((rows.size, 0), F32)
        Os = _take(pf, p0[:, None, None] + sl[None, :, None] * ldp + S.PART_HEAD + e[None, None, :]) if sl.size else np.zeros((rows.size, 0, E), F32)
        M = ms.max(1, keepdims=True) if sl.size else np.full((rows.size, 1), -np.inf, F32)
        with np.errstate(invalid="ignore"):
            w = np.where(ms == -np.inf, F32(0), np.exp(ms - M, dtype=F32)).astype(F32)
        L = (ls * w).sum(1, dtype=F32)
        acc = (Os * w[:, :, None]).sum(1, dtype=F32)
        inv = np.where(L > 0, F32(1) / np.where(L > 0, L, F32(1)), F32(0)).astype(F32)
        xu = (acc * inv[:, None] + ub[None, :]).astype(F32)
    x = np.concatenate([xc, xu], 1).astype(dt)

    def weight(buf, N, K):
        wflat = buf.numpy()[:N * K]
        n, k = np.arange(N)[:, None], np.arange(K)[None, :]
        if not c.packed:
            return _take(wflat, n * K + k).astype(dt)
        wp = emu_tail_pack(wflat, N, K, fault)
        lane = 16 * ((k % 16) // 4) + n % 16
        return wp[(((k // 16) * (N // 16) + n // 16) * 64 + lane) * 4 + k % 4].astype(dt)

    h1 = np.maximum((x @ weight(case["w1_buf"], S.TAIL_N1, 2 * E).T).astype(dt) + case["b1_buf"].numpy()[:S.TAIL_N1].astype(dt), 0).astype(dt)
    h2 = np.maximum((h1 @ weight(case["w2_buf"], S.TAIL_N2, S.TAIL_N1).T).astype(dt) + case["b2_buf"].numpy()[:S.TAIL_N2].astype(dt), 0).astype(dt)
    o = (h2 @ case["w3_buf"].numpy()[:S.TAIL_N2].astype(dt)).astype(dt) + dt(case["b3"])
    out_t = S.tail_output(case) if out_t is None else out_t
    _put(out_t.numpy(), rows[rows < B], o[rows < B].astype(F32))
    return out_t


# ------------------------------------------------------------------------------------------------ the GPU tests' checks, on the emulators
def _run_cand(key, fault=None, worst=None):
    c, packed = key
    case = S.cand_inputs(c)
    emb, pc = emu_cand(case, packed, fault)
    S.check_cand(case, emb, pc, None, what=f"emu {S.cand_form(packed, c.B, c.N1)} {S.cand_id(c)}")


def _run_split(c, fault=None, worst=None):
    case = S.split_inputs(c)
    w = worst or Worst()
    out, ws = emu_split(case, c, fault)
    what = "emu split " + S.split_id(c)
    if c.nsplit > 1:
        S.check_split_partials(case, ws, w.close, what)
    if c.nsplit == 1 or c.merge:
        S.check_split_out(case, out, w.close, what)
    else:
        assert bool((out == R.SENTINEL).all()), f"{what}: merge = 0 must leave out alone"


def _run_tail(c, fault=None, worst=None):
    case = S.tail_inputs(c)
    S.check_tail(case, emu_tail(case, c, fault), (worst or Worst()).close, "emu tail " + S.tail_id(c))


def test_emulators_pass_within_half_of_the_bar():
    """The right index walks meet every check of the GPU tests on every table case: bit for bit on the exact cases, and with at
    most half of the bar where a bar applies (fp32 in numpy's summation order, not the kernels')."""
    for c in S.CAND_CASES:
        for packed in (False, True):
            _run_cand((c, packed))
    worst = {"split": Worst(), "tail": Worst()}
    for c in S.SPLIT_CASES:
        _run_split(c, worst=worst["split"])
    for c in S.TAIL_CASES:
        _run_tail(c, worst=worst["tail"])
    for k, w in worst.items():
        print(f"{k}: worst use of a bar {w.frac:.4f} at {w.where}")
        assert 0.0 < w.frac <= 0.5, (k, w.frac, w.where)


def test_pack_emulators_give_the_stated_layouts():
    """emu_cand_pack / emu_tail_pack (thread index -> source element, as the kernels decode it) == the layouts the kernels' comments
    state, built by reshaping; the transposed-lane defect differs."""
    for c in S.CAND_CASES[:12]:
        case = S.cand_inputs(c)
        got = emu_cand_pack(case["wi_buf"].numpy().ravel(), case["ld"]["w"], c.K, c.N1)
        assert torch.equal(torch.from_numpy(got.astype(F32)), S.cand_pack_layout(case["wi_buf"], c.K, c.N1)), c
        assert not np.array_equal(emu_cand_pack(case["wi_buf"].numpy().ravel(), case["ld"]["w"], c.K, c.N1, "pack_transpose"), got)
    for N, K in ((16, 16), (48, 80), (256, 128), (128, 256), (256, 256)):
        W = torch.arange(N * K, dtype=torch.float32).view(N, K)
        assert torch.equal(torch.from_numpy(emu_tail_pack(W.numpy().ravel(), N, K)), S.tail_pack_layout(W))
        assert not np.array_equal(emu_tail_pack(W.numpy().ravel(), N, K, "pack_transpose"), S.tail_pack_layout(W).numpy())


FAULTS = ("splitk_last_short", "finish_ks_plus_1", "ragged_every_piece", "ragged_guard_le", "no_row_clamp", "ldemb_for_pc", "divide_shift5",
          "swizzle_e7", "t1_plus1", "part_addr", "np_div", "tail_user_ldcand", "tail_merge_skip", "pack_transpose")


def _cand_keys(pred):
    return [(c, p) for c in S.CAND_CASES for p in (False, True) if pred(c, S.cand_form(p, c.B, c.N1))]


def _split_cs(pred):
    return [c for c in S.SPLIT_CASES if pred(c, S.split_form(c.mode, c.A, c.Fdim, c.ppw))]


# defect -> [(runner, the table cases that exercise the form concerned)]: EVERY listed case must reject the defect
DEFECT_CASES = {
    "splitk_last_short": [(_run_cand, _cand_keys(lambda c, f: f[0] == "splitk" and c.K >= 32))],
    "finish_ks_plus_1": [(_run_cand, _cand_keys(lambda c, f: f[0] == "splitk" and f[1] < 8 and c.K >= 32))],
    "ragged_every_piece": [(_run_cand, _cand_keys(lambda c, f: f[0] == "splitk" and c.K % 32))],
    "ragged_guard_le": [(_run_cand, _cand_keys(lambda c, f: f[0] == "staged" and c.K % 32))],     # the packed W is zero past K
    "no_row_clamp": [(_run_cand, _cand_keys(lambda c, f: c.B % 16 != 0))],                         # shown by the bounds audit alone
    "ldemb_for_pc": [(_run_cand, _cand_keys(lambda c, f: c.B > 1))],
    "divide_shift5": [(_run_split, _split_cs(lambda c, f: f.path == "divide"))],
    "swizzle_e7": [(_run_split, _split_cs(lambda c, f: f.swizzled))],
    "t1_plus1": [(_run_split, S.SPLIT_CASES)],
    "part_addr": [(_run_split, _split_cs(lambda c, f: c.nsplit > 1))],
    "np_div": [(_run_split, S.SPLIT_CASES)],
    "tail_user_ldcand": [(_run_tail, [c for c in S.TAIL_CASES if c.source == "user" and c.lduser != c.E + 4])],
    "tail_merge_skip": [(_run_tail, [c for c in S.TAIL_CASES if c.source == "part"])],
    "pack_transpose": [(_run_cand, _cand_keys(lambda c, f: f[0] != "staged")), (_run_tail, [c for c in S.TAIL_CASES if c.packed])],
}


@pytest.mark.parametrize("fault", FAULTS)
def test_each_defect_is_rejected(fault):
    n = 0
    for run, cases in DEFECT_CASES[fault]:
        assert cases, fault
        for c in cases:
            with pytest.raises(AssertionError):
                run(c, fault)
            n += 1
    print(f"{fault}: rejected on {n} table cases")
    assert n >= 2


# ------------------------------------------------------------------------------------------------ the record of the gap
# the shapes the suite ran before this table, all on contiguous operands, random floats, outputs from torch.empty, values at the bar:
# test_attn_candidates_both_weight_forms (B, K, N1, N2), test_entry_split_kernel_vs_per_pair ((A, Fdim) x (ppw, nsplit), merged, with
# wg_row; eight of its 96 cases here, every A and every (ppw, nsplit) among them), test_attention_tail_kernel (E, B, nsplit)
OLD_CAND = [(4096, 2094, 64, 128), (100, 2094, 128, 128), (33, 96, 64, 16), (17, 31, 64, 32), (512, 1000, 128, 256), (1, 65, 64, 64),
            (2100, 300, 128, 64), (2048, 77, 64, 128), (700, 2094, 64, 128),
            (1000, 257, 64, 96), (255, 1024, 128, 48)]              # two of test_attn_candidates_random_shapes' draws (B = 1000: KS = 4)
OLD_SPLIT = [S.SplitCase((R.ATT_MLP, R.ATT_MLP_SCALED, R.ATT_COS)[k % 3], A, F, ppw, ns, 1, True, True, 60 + k)
             for k, ((A, F), (ppw, ns)) in enumerate(zip([(128, 64), (32, 64), (64, 128), (256, 128)] * 2,
                                                         [(32, 1), (32, 4), (16, 2), (32, 3), (5, 8), (64, 4), (64, 1), (40, 2)]))]
OLD_TAIL = [(64, 4096, 4), (64, 333, 1), (128, 1000, 3), (64, 17, 8), (128, 16, 1)]
# the defects the earlier shapes and checks could have shown, as computed below (everything else needed this table)
OLD_CATCHES = {"splitk_last_short", "finish_ks_plus_1", "ragged_every_piece", "ragged_guard_le", "ldemb_for_pc", "swizzle_e7", "t1_plus1",
               "part_addr", "np_div", "tail_merge_skip", "pack_transpose"}


def _fails(fn):
    try:
        fn()
    except Stray:
        return False                                                # no earlier check audits bounds: a stray read inside the process goes unseen
    except AssertionError:
        return True
    return False


def test_what_the_earlier_shapes_would_have_caught():
    """Each defect on the shapes and with the checks the suite had before: values at the 1e-5 bar, contiguous operands, outputs from
    torch.empty — modelled at its most forgiving for a defect, the block an identical earlier call just freed (those tests run every
    call twice), so a word that is never written holds the right value; no padding, no sentinel, no look at the partials."""
    old_ks = {S.cand_splitk_pieces(B) for B, _, _, _ in OLD_CAND}
    assert old_ks == {1, 2, 4, 5, 8}, old_ks                        # KS in {3, 6, 7}: live code no test ran
    assert not any(S.split_form(c.mode, c.A, c.Fdim, c.ppw).path == "divide" for c in OLD_SPLIT)
    runs = []
    for k, (B, K, N1, N2) in enumerate(OLD_CAND):
        case = S.build_cand(B, K, N1, N2, 5, True, 90 + k, lds={"x": K, "w": K, "emb": N1, "pc": N2}, exact=False)
        for packed in (False, True):
            def run(f, case=case, packed=packed):
                bufs = (case["emb64"].float().clone(), case["pc64"].float().clone())
                emb, pc = emu_cand(case, packed, f, bufs, audit=False)
                w = Worst()
                w.close(emb, case["emb64"], "emb")
                w.close(pc, case["pc64"], "pc")
            runs.append((f"cand {B}x{K}x{N1}x{N2} {'packed' if packed else 'staged'}", run))
    for c in OLD_SPLIT:
        case = R.make_inputs(c.mode, c.A, c.Fdim, S.SPLIT_LENGTHS, S.split_pairs_per_row(c.ppw, c.seed), c.seed,
                             lds={"pc": c.A, "pr": c.A, "feat": c.Fdim, "out": c.Fdim}, masked_row_pairs=0, mask_entries=False)
        case["nsplit"], case["ldpart"] = c.nsplit, c.Fdim + S.PART_HEAD

        def run(f, case=case, c=c):
            out, _ = emu_split(case, c, f, (case["out64"].float().clone(), S.split_workspace(case)))
            Worst().close(out, case["out64"], "out")
        runs.append(("split " + S.split_id(c), run))
    for k, (E, B, ns) in enumerate(OLD_TAIL):
        for src in ("user", "part"):
            for packed in (False, True):
                c = S.TailCase(E, packed, B, src, max(ns, 1) if src == "part" else 0, src == "part", E, "float", 70 + k)
                case = S.build_tail(c, lds={"cand": E, "user": E})

                def run(f, case=case, c=c):
                    out = emu_tail(case, c, f, torch.cat((case["out64"].float(), torch.full((S.OUT_PAD,), R.SENTINEL))))
                    Worst().close(out[:case["B"]], case["out64"], "tail")
                runs.append((f"tail {S.tail_id(c)}", run))
    for name, run in runs:
        run(None)
    caught = set()
    for fault in FAULTS:
        hit = [name for name, run in runs if _fails(lambda: run(fault))]
        print(f"{fault}: caught by {len(hit)} of the {len(runs)} earlier runs", hit[:3])
        if hit:
            caught.add(fault)
    print("missed by every earlier run:", sorted(set(FAULTS) - caught))
    assert caught == OLD_CATCHES, (sorted(caught), sorted(set(FAULTS) - caught))
