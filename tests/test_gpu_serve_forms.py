"""The kernels AttentionNCF inference runs — csrc/attn_cand.hip, attn_split.hip, attn_tail.hip — on every launch form they can take,
against the references of tests/serve_forms_ref.py (which holds the dispatch mirrors, the case tables, the inputs and the checks;
tests/test_serve_forms_cpu.py shows on the CPU that the checks reject fourteen index defects).

The calls go through the C ABI directly: every operand is a column slice of a wider buffer whose padding is poisoned, and every
output buffer, padding included, starts as a sentinel.  The candidate and tail cases are exact-integer: the kernels must equal the
reference bit for bit in every weight form (staged, packed, split-K; plain and packed tail weights).  Every call runs twice and must
repeat bit for bit."""

import pytest
import torch

import attn_forms_ref as R
import serve_forms_ref as S
from test_gpu_basic import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    assert (n.ATT_MLP, n.ATT_COS, n.ATT_MLP_SCALED, n.ATT_SCALE_LOG2) == (R.ATT_MLP, R.ATT_COS, R.ATT_MLP_SCALED, R.SCALE_LOG2)
    return n


def _close(got, ref, tag):
    assert_close(got, ref)                                          # the project's bar; records its margin itself


def _p(t, off=0):
    return None if t is None else t.data_ptr() + off


def _err(native):
    return native.load_library().ncf_last_error().decode()


def _dev(case, keys, gpu):
    return {k: (None if case.get(k) is None else case[k].to(gpu)) for k in keys}


# ------------------------------------------------------------------------------------------------ candidates
CAND_KEYS = ("x_buf", "wi_buf", "wc_buf", "bi_buf", "b0_buf", "pair_row")


def _pack_cand(native, d, case, gpu):
    lib = native.load_library()
    n = lib.ncf_attn_candidates_pack_floats(case["K"], case["N1"])
    wp = torch.full((n + S.OUT_PAD,), R.SENTINEL, device=gpu)
    rc = lib.ncf_attn_candidates_pack(_p(d["wi_buf"]), case["ld"]["w"], case["K"], case["N1"], _p(wp), native._stream(wp))
    torch.cuda.synchronize()
    assert rc == native.NCF_OK, _err(native)
    return wp, n


def _candidates(native, case, d, packed, wp, grouping, gpu, oob=None):
    """One call; returns (rc, emb, pc, grouping outputs or None) on the CPU."""
    lib = native.load_library()
    B, K, N1, N2, ld, Rr, ppw = case["B"], case["K"], case["N1"], case["N2"], case["ld"], case["R"], case["ppw"]
    emb, pc = (t.to(gpu) for t in S.cand_outputs(case))
    g = [t.to(gpu) for t in S.group_outputs(B, Rr, ppw)] if grouping else [None] * 4
    oob = torch.zeros(1, dtype=torch.int32, device=gpu) if oob is None else oob
    nbytes = (lib.ncf_attn_candidates_packed_workspace_bytes(B, N1, Rr if grouping else -1) if packed
              else lib.ncf_attn_candidates_workspace_bytes(Rr) if grouping else 0)
    ws = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=gpu) if nbytes else None
    tail = (_p(d["bi_buf"]), N1, _p(d["wc_buf"]), _p(d["b0_buf"]), N2, _p(emb), ld["emb"], _p(pc), ld["pc"],
            _p(d["pair_row"]) if grouping else None, Rr if grouping else 0, ppw, _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]), _p(ws), nbytes,
            _p(oob), native._stream(emb))
    if packed:
        rc = lib.ncf_attn_candidates_packed(_p(d["x_buf"]), B, ld["x"], K, _p(wp), *tail)
    else:
        rc = lib.ncf_attn_candidates(_p(d["x_buf"]), B, ld["x"], K, _p(d["wi_buf"]), ld["w"], *tail)
    torch.cuda.synchronize()
    return rc, emb.cpu(), pc.cpu(), ([t.cpu() for t in g] + [oob.cpu()] if grouping else None)


@pytest.mark.parametrize("c", S.CAND_CASES, ids=S.cand_id)
def test_candidate_forms_exact(native, gpu, c):
    """Staged, packed and split-K forms, with and without the grouping workgroup: torch.equal with the exact integer product."""
    case = S.cand_inputs(c)
    d = _dev(case, CAND_KEYS, gpu)
    ref = native.group_pairs(d["pair_row"], case["R"], case["ppw"])
    native.check_oob(gpu)
    ref = [ref[0].cpu(), ref[1].cpu(), ref[2].cpu(), ref.wg_row.cpu()]
    mine = S.group_ref(case["pair_row"], case["R"], case["ppw"])
    assert torch.equal(ref[0], mine[0]) and torch.equal(ref[2], mine[2]) and torch.equal(ref[3][:mine[3].numel()], mine[3])
    wp, n = _pack_cand(native, d, case, gpu)
    assert torch.equal(wp[:n].cpu(), S.cand_pack_layout(case["wi_buf"], c.K, c.N1)), "cand_pack_kernel: not the stated layout"
    assert bool((wp[n:] == R.SENTINEL).all())
    for packed in (False, True):
        form = S.cand_form(packed, c.B, c.N1)
        print("form", form, "slices", S.cand_slices(c.K, form[1])[0][:3], "...")
        for grouping in (False, True):
            what = f"{form[0]} KS={form[1]}" + (" + grouping" if grouping else "")
            rc, emb, pc, g = _candidates(native, case, d, packed, wp, grouping, gpu)
            assert rc == native.NCF_OK, _err(native)
            S.check_cand(case, emb, pc, (g, ref) if grouping else None, what=what)
            rc2, emb2, pc2, g2 = _candidates(native, case, d, packed, wp, grouping, gpu)
            assert rc2 == native.NCF_OK and torch.equal(emb, emb2) and torch.equal(pc, pc2), what + ": not repeatable"


def test_candidate_grouping_flags_an_out_of_range_row(native, gpu):
    c = S.CandCase(17, 33, 64, 16, 5, True, 2300)
    case = dict(S.cand_inputs(c))
    bad = case["pair_row"].clone()
    bad[9] = 5                                                     # one entry past the last row
    d = _dev(dict(case, pair_row=bad), CAND_KEYS, gpu)
    wp, _ = _pack_cand(native, d, case, gpu)
    for packed in (False, True):
        rc, emb, pc, g = _candidates(native, case, d, packed, wp, True, gpu)
        assert rc == native.NCF_OK and int(g[4]) == 1
        S.check_cand(case, emb, pc, None)                          # the product does not depend on the grouping
        good = _dev(case, CAND_KEYS, gpu)
        rc, emb, pc, g = _candidates(native, case, good, packed, wp, True, gpu)
        assert rc == native.NCF_OK and int(g[4]) == 0


@pytest.mark.parametrize("K", [1, 31, 33, 2094])
@pytest.mark.parametrize("N1", [64, 128])
def test_cand_pack_kernel_layout(native, gpu, K, N1):
    """Wp[(((s NT + nt) 2 + h) 64 + lane) 4 + j] = Wi[16 nt + (lane & 15)][32 s + 16 h + 4 (lane >> 4) + j], zero past K, from a
    weight with ldw > K whose padding is poisoned; distinct values, so a misplaced word shows."""
    ldw = K + 3
    W = R.wide(torch.arange(1, N1 * K + 1, dtype=torch.float32).view(N1, K), ldw)
    case = {"K": K, "N1": N1, "ld": {"w": ldw}}
    wp, n = _pack_cand(native, {"wi_buf": W.to(gpu)}, case, gpu)
    assert n == (K + 31) // 32 * 32 * N1
    want = torch.zeros(n)
    idx = torch.arange(n)
    j, lane, h, q = idx & 3, (idx >> 2) & 63, (idx >> 8) & 1, idx >> 9
    nt, s = q % (N1 // 16), q // (N1 // 16)
    row, k = 16 * nt + (lane & 15), 32 * s + 16 * h + 4 * (lane >> 4) + j
    want[k < K] = W[row[k < K], k[k < K]]
    assert torch.equal(wp[:n].cpu(), want) and torch.equal(want, S.cand_pack_layout(W, K, N1))
    assert bool((wp[n:] == R.SENTINEL).all()), "packed words written past the packed size"


# ------------------------------------------------------------------------------------------------ entry-split attention
SPLIT_KEYS = ("pc_buf", "pr_buf", "feat_buf", "w1_buf", "bias_buf", "rowptr", "col", "val", "pair_row")


def _split(native, case, d, grp, c, gpu, **over):
    """One ncf_attn_forward_split call; ``over`` replaces arguments (the refusal tests).  Returns (rc, out, workspace) on the CPU."""
    lib = native.load_library()
    a = dict(mode=case["mode"], pc=_p(d["pc_buf"]), ldpc=case["ld"]["pc"], pr=_p(d["pr_buf"]), ldpr=case["ld"]["pr"], A=case["A"],
             w1=_p(d["w1_buf"]), b1=case["b1"], Fdim=case["Fdim"], ppw=c.ppw, nsplit=c.nsplit, merge=c.merge,
             wg_row=_p(grp.wg_row) if c.wg_row else None, bias=_p(d["bias_buf"]), ws_off=0, ws_short=0, ldfeat=case["ld"]["feat"])
    a.update(over)
    out = R.fresh_outputs(case, False)[0].to(gpu)
    ns = max(a["nsplit"], 1)
    ws = torch.full((case["B"] * ns * (case["Fdim"] + S.PART_HEAD) + S.OUT_PAD,), R.SENTINEL, device=gpu)
    nbytes = lib.ncf_attn_split_workspace_bytes(case["B"], a["Fdim"], a["nsplit"])
    if a["Fdim"] == case["Fdim"] and a["nsplit"] > 1:
        assert nbytes == (ws.numel() - S.OUT_PAD) * 4
    rc = lib.ncf_attn_forward_split(a["mode"], a["pc"], a["ldpc"], a["pr"], a["ldpr"], a["A"], a["w1"], a["b1"], _p(d["rowptr"]), _p(d["col"]),
                                    _p(d["val"]), case["R"], case["I"], _p(grp[0]), _p(grp[1]), _p(grp[2]), a["wg_row"], case["B"], a["ppw"],
                                    _p(d["feat_buf"]), a["ldfeat"], a["Fdim"], a["bias"], _p(out), case["ld"]["out"], a["nsplit"], a["merge"],
                                    _p(ws, a["ws_off"]), max(nbytes - a["ws_short"], 0), native._stream(out))
    torch.cuda.synchronize()
    return rc, out.cpu(), ws.cpu()


@pytest.mark.parametrize("c", S.SPLIT_CASES, ids=S.split_id)
def test_entry_split_forms(native, gpu, c):
    case = S.split_inputs(c)
    form = S.split_form(c.mode, c.A, c.Fdim, c.ppw)
    assert native.attn_split_supported(c.mode, c.A, c.Fdim, c.ppw)
    print("form", form)
    d = _dev(case, SPLIT_KEYS, gpu)
    grp = native.group_pairs(d["pair_row"], case["R"], c.ppw)
    native.check_oob(gpu)
    what = f"attn_split{form.inst} {form.path}"
    rc, out, ws = _split(native, case, d, grp, c, gpu)
    assert rc == native.NCF_OK, _err(native)
    if c.nsplit > 1:
        S.check_split_partials(case, ws, _close, what)
    else:
        assert bool((ws == R.SENTINEL).all()), "nsplit = 1 must not touch the workspace"
    if c.nsplit == 1 or c.merge:
        S.check_split_out(case, out, _close, what)
    else:
        assert bool((out == R.SENTINEL).all()), "merge = 0 must leave out alone"
    rc2, out2, ws2 = _split(native, case, d, grp, c, gpu)
    live = case["B"] * c.nsplit * case["ldpart"]
    heads = ws[:live].view(-1, case["ldpart"])[:, [0, 1]], ws2[:live].view(-1, case["ldpart"])[:, [0, 1]]
    assert rc2 == native.NCF_OK and torch.equal(out, out2) and torch.equal(heads[0], heads[1])
    assert torch.equal(ws[:live].view(-1, case["ldpart"])[:, S.PART_HEAD:], ws2[:live].view(-1, case["ldpart"])[:, S.PART_HEAD:])


# ------------------------------------------------------------------------------------------------ tail
TAIL_KEYS = ("cand_buf", "user_buf", "part_buf", "ubias_buf", "w1_buf", "w2_buf", "w3_buf", "b1_buf", "b2_buf")


def _pack_tail(native, w_buf, N, K, gpu):
    lib = native.load_library()
    packed = torch.full((N * K + S.OUT_PAD,), R.SENTINEL, device=gpu)
    rc = lib.ncf_attn_tail_pack_weight(_p(w_buf), N, K, _p(packed), native._stream(packed))
    torch.cuda.synchronize()
    assert rc == native.NCF_OK, _err(native)
    assert bool((packed[N * K:] == R.SENTINEL).all()), "packed words written past N * K"
    return packed


def _tail(native, case, d, packed, weights, gpu, **over):
    lib = native.load_library()
    E = case["E"]
    part = case["source"] != "user"
    a = dict(cand=_p(d["cand_buf"]), ldcand=case["ld"]["cand"], EA=E, UE=E, part=_p(d["part_buf"]) if part else None, nsplit=case["nsplit"] if part else 0,
             user=None if part else _p(d["user_buf"]), lduser=0 if part else case["ld"]["user"], ubias=_p(d["ubias_buf"]), N1=S.TAIL_N1, N2=S.TAIL_N2)
    a.update(over)
    out = S.tail_output(case).to(gpu)
    rc = lib.ncf_attn_tail(a["cand"], a["ldcand"], a["EA"], a["part"], a["nsplit"], a["user"], a["lduser"], a["UE"], a["ubias"], _p(weights[0]),
                           _p(d["b1_buf"]), a["N1"], _p(weights[1]), _p(d["b2_buf"]), a["N2"], _p(d["w3_buf"]), case["b3"], int(packed), _p(out),
                           case["B"], native._stream(out))
    torch.cuda.synchronize()
    return rc, out.cpu()


@pytest.mark.parametrize("c", S.TAIL_CASES, ids=S.tail_id)
def test_tail_forms(native, gpu, c):
    """Exact cases: torch.equal with the exact MLP of the exact merge, plain and packed weights alike; float cases: the bar."""
    case = S.tail_inputs(c)
    print("form", S.tail_form(c.E, c.packed, c.source, c.nsplit))
    d = _dev(case, TAIL_KEYS, gpu)
    weights = (d["w1_buf"], d["w2_buf"])
    if c.packed:
        weights = (_pack_tail(native, d["w1_buf"], S.TAIL_N1, 2 * c.E, gpu), _pack_tail(native, d["w2_buf"], S.TAIL_N2, S.TAIL_N1, gpu))
        assert torch.equal(weights[0][:S.TAIL_N1 * 2 * c.E].cpu(), S.tail_pack_layout(case["W1"])), "tail_pack_kernel: not the stated layout"
        assert torch.equal(weights[1][:S.TAIL_N2 * S.TAIL_N1].cpu(), S.tail_pack_layout(case["W2"]))
    rc, out = _tail(native, case, d, c.packed, weights, gpu)
    assert rc == native.NCF_OK, _err(native)
    S.check_tail(case, out, _close, "attn_tail " + S.tail_id(c))
    rc2, out2 = _tail(native, case, d, c.packed, weights, gpu)
    assert rc2 == native.NCF_OK and torch.equal(out, out2)


@pytest.mark.parametrize("N,K", [(16, 16), (48, 80), (256, 128), (128, 256), (256, 256)])
def test_tail_pack_kernel_layout(native, gpu, N, K):
    """packed[((kb N / 16 + tile) 64 + lane) 4 + j] = W[16 tile + (lane & 15)][16 kb + 4 (lane >> 4) + j]; distinct values."""
    W = torch.arange(1, N * K + 1, dtype=torch.float32).view(N, K)
    packed = _pack_tail(native, torch.cat((W.reshape(-1), torch.full((16,), R.POISON))).to(gpu), N, K, gpu)
    idx = torch.arange(N * K)
    j, lane, q = idx & 3, (idx >> 2) & 63, idx >> 8
    tile, kb = q % (N // 16), q // (N // 16)
    want = W[16 * tile + (lane & 15), 16 * kb + 4 * (lane >> 4) + j]
    assert torch.equal(packed[:N * K].cpu(), want) and torch.equal(want, S.tail_pack_layout(W))


# ------------------------------------------------------------------------------------------------ the chain the model runs
@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("nsplit", [3, 9])
def test_split_partials_feed_the_tail(native, gpu, E, nsplit):
    """ncf_attn_forward_split(merge = 0), then ncf_attn_tail on the workspace it left, against the float64 attention followed by a
    float64 MLP; and against merge = 1 followed by the tail on the finished user embeddings."""
    c = S.SplitCase(R.ATT_MLP, 128, E, 32, nsplit, 0, True, True, 5000 + E + nsplit)
    case = S.split_inputs(c)
    d = _dev(case, SPLIT_KEYS, gpu)
    grp = native.group_pairs(d["pair_row"], case["R"], c.ppw)
    tc = S.TailCase(E, True, case["B"], "user", 0, False, E + 4, "float", 5100 + E + nsplit)
    tcase = S.build_tail(tc)
    td = _dev(tcase, TAIL_KEYS, gpu)
    t64 = lambda k, n: tcase[k][:n].double()
    W1, W2 = tcase["W1"].double(), tcase["W2"].double()
    x64 = torch.cat((tcase["cand_buf"][:, :E].double(), case["out64"]), 1)
    h = torch.relu(torch.relu(x64 @ W1.t() + t64("b1_buf", S.TAIL_N1)) @ W2.t() + t64("b2_buf", S.TAIL_N2))
    ref = h @ t64("w3_buf", S.TAIL_N2) + tcase["b3"]
    weights = (_pack_tail(native, td["w1_buf"], S.TAIL_N1, 2 * E, gpu), _pack_tail(native, td["w2_buf"], S.TAIL_N2, S.TAIL_N1, gpu))
    lib = native.load_library()

    def tail(part, ns, user, lduser, ubias):
        out = S.tail_output(tcase).to(gpu)
        rc = lib.ncf_attn_tail(_p(td["cand_buf"]), E + 4, E, _p(part), ns, _p(user), lduser, E, _p(ubias), _p(weights[0]), _p(td["b1_buf"]), S.TAIL_N1,
                               _p(weights[1]), _p(td["b2_buf"]), S.TAIL_N2, _p(td["w3_buf"]), tcase["b3"], 1, _p(out), case["B"], native._stream(out))
        torch.cuda.synchronize()
        assert rc == native.NCF_OK, _err(native)
        return out.cpu()

    # merge = 0: the partials stay on the device and the tail merges them (+ the UserEmbeddings bias)
    out = R.fresh_outputs(case, False)[0].to(gpu)
    ws = S.split_workspace(case).to(gpu)
    args = lambda merge: (case["mode"], _p(d["pc_buf"]), case["ld"]["pc"], _p(d["pr_buf"]), case["ld"]["pr"], case["A"], _p(d["w1_buf"]), case["b1"],
                          _p(d["rowptr"]), _p(d["col"]), _p(d["val"]), case["R"], case["I"], _p(grp[0]), _p(grp[1]), _p(grp[2]), _p(grp.wg_row),
                          case["B"], c.ppw, _p(d["feat_buf"]), case["ld"]["feat"], E, _p(d["bias_buf"]), _p(out), case["ld"]["out"], nsplit, merge,
                          _p(ws), (ws.numel() - S.OUT_PAD) * 4, native._stream(out))
    assert lib.ncf_attn_forward_split(*args(0)) == native.NCF_OK, _err(native)
    got = tail(ws, nsplit, None, 0, d["bias_buf"])
    S.check_tail(dict(tcase, out64=ref), got, _close, "split(merge=0) -> tail")
    assert bool((out == R.SENTINEL).all())
    # merge = 1: finished user embeddings (bias added by the combine), then the tail on them
    assert lib.ncf_attn_forward_split(*args(1)) == native.NCF_OK, _err(native)
    got1 = tail(None, 0, out, case["ld"]["out"], None)
    S.check_tail(dict(tcase, out64=ref), got1, _close, "split(merge=1) -> tail")
    _close(got[:case["B"]], got1[:case["B"]].double(), "the two routes")


# ------------------------------------------------------------------------------------------------ refusals launch nothing
def test_split_refusals_launch_nothing(native, gpu):
    c = S.SplitCase(R.ATT_MLP, 64, 64, 16, 3, 1, True, True, 5200)
    case = R.make_inputs(c.mode, c.A, c.Fdim, [9, 0, 70, 17], [3, 1, 20, 2], c.seed, lds={"pc": 72}, masked_row_pairs=1)
    d = _dev(case, SPLIT_KEYS, gpu)
    grp = native.group_pairs(d["pair_row"], case["R"], c.ppw)
    native.check_oob(gpu)
    U, I, W = native.NCF_EUNSUPPORTED, native.NCF_EINVAL, native.NCF_EWORKSPACE
    refusals = [(dict(A=48), U), (dict(A=288), U), (dict(Fdim=96), U), (dict(ppw=0), U), (dict(ppw=65), U), (dict(nsplit=0), I), (dict(nsplit=65), I),
                (dict(ldpc=70), U), (dict(pc=_p(d["pc_buf"], 4)), I), (dict(ws_short=1), W), (dict(ws_off=4), W)]
    for over, code in refusals:
        rc, out, ws = _split(native, case, d, grp, c, gpu, **over)
        assert rc == code, (over, rc, _err(native))
        assert "ncf_attn_forward_split" in _err(native), over
        assert bool((out == R.SENTINEL).all()) and bool((ws == R.SENTINEL).all()), f"{over}: a refused call wrote something"
    native.check_oob(gpu)
    seen = set()
    for mode in (0, 1, 2, 3):                                       # ncf_attn_split_supported == (the call returns NCF_OK)
        for A in (32, 48, 64, 288):
            for Fdim in (64, 96):
                for ppw in (0, 16, 65):
                    ok = native.load_library().ncf_attn_split_supported(mode, A, Fdim, ppw)
                    assert bool(ok) == S.split_supported(mode, A, Fdim, ppw)
                    rc, out, ws = _split(native, case, d, grp, c, gpu, mode=mode, A=A, Fdim=Fdim, ppw=ppw)
                    assert (rc == native.NCF_OK) == bool(ok), (mode, A, Fdim, ppw, rc)
                    seen.add(bool(ok))
                    if not ok:
                        assert rc == U and bool((out == R.SENTINEL).all()) and bool((ws == R.SENTINEL).all())
    assert seen == {True, False}


def test_candidate_refusals_launch_nothing(native, gpu):
    lib = native.load_library()
    case = S.build_cand(40, 65, 128, 16, 5, True, 5300, lds={"emb": 132, "pc": 280})
    d = _dev(case, CAND_KEYS, gpu)
    wp, _ = _pack_cand(native, d, case, gpu)
    U, I, W = native.NCF_EUNSUPPORTED, native.NCF_EINVAL, native.NCF_EWORKSPACE

    def call(packed, grouping=True, **o):
        B, Rr = o.get("B", case["B"]), o.get("R", case["R"])
        emb, pc = (t.to(gpu) for t in S.cand_outputs(case))
        g = [t.to(gpu) for t in S.group_outputs(case["B"], case["R"], case["ppw"])]
        oob = torch.zeros(1, dtype=torch.int32, device=gpu)
        nbytes = lib.ncf_attn_candidates_packed_workspace_bytes(case["B"], case["N1"], case["R"]) if packed else lib.ncf_attn_candidates_workspace_bytes(case["R"])
        ws = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=gpu)
        tail = (_p(d["bi_buf"]), o.get("N1", case["N1"]), _p(d["wc_buf"], o.get("wc_off", 0)), _p(d["b0_buf"]), o.get("N2", case["N2"]), _p(emb),
                o.get("ldemb", case["ld"]["emb"]), _p(pc), case["ld"]["pc"], _p(d["pair_row"]) if grouping else None, Rr, case["ppw"], _p(g[0]), _p(g[1]),
                _p(g[2]), _p(g[3]), _p(ws), nbytes - o.get("ws_short", 0), _p(oob), native._stream(emb))
        if packed:
            rc = lib.ncf_attn_candidates_packed(_p(d["x_buf"]), B, o.get("ldx", case["ld"]["x"]), case["K"], _p(wp, o.get("wp_off", 0)), *tail)
        else:
            rc = lib.ncf_attn_candidates(_p(d["x_buf"]), B, o.get("ldx", case["ld"]["x"]), case["K"], _p(d["wi_buf"]), case["ld"]["w"], *tail)
        torch.cuda.synchronize()
        untouched = (bool((emb == R.SENTINEL).all()) and bool((pc == R.SENTINEL).all()) and all(bool((t == -7).all()) for t in g)
                     and int(oob) == 0 and bool((ws == 0x5A).all()))
        return rc, untouched

    who = {False: "ncf_attn_candidates", True: "ncf_attn_candidates_packed"}
    refusals = [(dict(N1=96), U, None), (dict(N2=8), U, None), (dict(N2=272), U, None), (dict(ldx=case["K"] - 1), I, None), (dict(ldemb=127), I, None),
                (dict(wc_off=4), I, None), (dict(wp_off=4), I, True), (dict(ws_short=lib.ncf_attn_candidates_workspace_bytes(case["R"]) + 1), W, True),
                (dict(B=32769), U, None), (dict(R=32769), U, None)]
    for over, code, only in refusals:
        for packed in ((False, True) if only is None else (only,)):
            rc, untouched = call(packed, **over)
            assert rc == code, (over, packed, rc, _err(native))
            assert who[packed] in _err(native) and untouched, (over, packed)
    for N1 in (64, 96, 128):                                        # ncf_attn_candidates_supported == (the call returns NCF_OK)
        for N2 in (8, 16, 272):
            ok = bool(lib.ncf_attn_candidates_supported(case["K"], N1, N2))
            assert ok == (N1 in (64, 128) and N2 == 16)
            for packed in (False, True):
                if packed and N1 != case["N1"]:
                    continue                                        # the packed copy is N1's own
                rc, untouched = call(packed, grouping=False, N1=N1, N2=N2)
                assert (rc == native.NCF_OK) == ok and (ok or (rc == U and untouched)), (N1, N2, packed, rc)


def test_tail_refusals_launch_nothing(native, gpu):
    lib = native.load_library()
    U, I = native.NCF_EUNSUPPORTED, native.NCF_EINVAL
    for src, ns in (("user", 0), ("part", 3)):
        c = S.TailCase(128, False, 17, src, ns, True, 132, "exact", 5400 + ns)
        case = S.tail_inputs(c)
        d = _dev(case, TAIL_KEYS, gpu)
        weights = (d["w1_buf"], d["w2_buf"])
        refusals = [(dict(EA=64, UE=128), U), (dict(N1=128), U), (dict(ldcand=130), I), (dict(ubias=_p(d["ubias_buf"], 4)), I)]
        if src == "part":
            refusals += [(dict(nsplit=0), I), (dict(nsplit=65), I)]
        for over, code in refusals:
            rc, out = _tail(native, case, d, False, weights, gpu, **over)
            assert rc == code, (over, rc, _err(native))
            assert "ncf_attn_tail" in _err(native) and bool((out == R.SENTINEL).all()), over
        for EA, UE in ((64, 64), (64, 128), (128, 64), (128, 128)):      # ncf_attn_tail_supported == (the call returns NCF_OK)
            for N1 in (256, 128):
                ok = bool(lib.ncf_attn_tail_supported(EA, UE, N1, S.TAIL_N2))
                assert ok == (EA == UE and N1 == 256)
                rc, out = _tail(native, case, d, False, weights, gpu, EA=EA, UE=UE, N1=N1)
                assert (rc == native.NCF_OK) == ok and (ok or (rc == U and bool((out == R.SENTINEL).all()))), (EA, UE, N1, rc)
