"""GPU: AttentionNCF's message dropout on the HIP attention kernels — ncf_attn_forward_train / ncf_attn_backward_train, the binding,
AttnFn, the model's opt-in (AttentionNCF.message_dropout_on_device) and train_model — against the float64 restatement of
tests/attn_msgdrop_ref.py (shown to be the reference's rule, and the bars attainable in fp32, by tests/test_attn_msgdrop_cpu.py).
The entry mask is a pure function of (seed, entry), so outputs and gradients are deterministic and are held to the bars the suite
uses for the same kernels without it: assert_close at 1e-5, _grads_close at ATT_RTOL = 1e-4, the model step's 2e-5 / 1e-5 / 1e-4."""
import copy
import functools

import numpy as np
import pytest
import torch

from attn_msgdrop_ref import (ATT_COS, ATT_LINEAR, ATT_MLP, ATT_MLP_SCALED, MSG_PS, ROWS, SHAPES, EntryMaskDropout, entry_keep,
                              hidden_and_message, msg_seed_of, reference)
from conftest import record_error
from dropout_mask_ref import threshold
from test_gpu_basic import assert_close
from test_gpu_dropout_masks import ATT_RTOL, P_THR0, _Grads, _MaskDropout, _att_case, _misses_bar, _mlp_dropout_off, _record, _record_grads
from test_gpu_training import _attention_batch, _grads_close

pytestmark = pytest.mark.gpu

NCF_EUNSUPPORTED = -2
GRADS = ("d_pc", "d_pr", "d_w1", "d_feat")


def _run(native, case, gpu, msg_seed, msg_p, hidden=None, msg_p_bwd=None):
    """Forward and backward through the binding.  ``hidden`` = (p, seed) of AttentionNet's hidden dropout or None."""
    d = {k: (v.to(gpu) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    msg = None if msg_p is None else (msg_p, msg_seed)
    out, wts = native.attn_forward(case["mode"], d["pc"], d["pr"], d["w1"], case["b1"], d["rowptr"], d["col"], d["val"], d["feat"],
                                   out_bias=d["bias"], dropout=hidden, msg_dropout=msg)
    msg_b = msg if msg_p_bwd is None else (msg_p_bwd, msg_seed)
    grads = native.attn_backward(case["mode"], d["pc"], d["pr"], d["w1"], d["rowptr"], d["col"], d["val"], d["feat"], wts, d["dout"],
                                 dropout=hidden, msg_dropout=msg_b)
    grads = dict(zip(GRADS, grads))
    if case["mode"] == ATT_COS:
        grads.pop("d_w1")
    return out, wts, grads


def _hold(tag, got, ref, mode):
    out, wts, grads = got
    out64, w64, g64 = ref[:3]
    g64 = {k: g64[k] for k in grads}
    _record(f"{tag} out", out, out64, 1e-5 * float(out64.abs().max()))
    _record(f"{tag} weights", wts, w64, 1e-5 * float(w64.abs().max()))
    assert_close(out, out64)
    assert_close(wts, w64)
    for k in grads:
        _record(f"{tag} {k}", grads[k], g64[k], ATT_RTOL * float(g64[k].abs().max()))
    _grads_close(_Grads(grads), _Grads(g64), rtol=ATT_RTOL)


# =============================================================================================== kernels against float64
@pytest.mark.parametrize("mode", [ATT_MLP, ATT_MLP_SCALED, ATT_COS])
@pytest.mark.parametrize("A,Fdim", SHAPES)
def test_message_dropout_forward_and_backward_match_float64(gpu, A, Fdim, mode):
    """out and the weights at assert_close's 1e-5, d_pc / d_pr / d_w1 / d_feat by _grads_close at 1e-4, for p in {0.1, 0.3, 0.5}; and
    with AttentionNet's hidden dropout active at the same time under another seed (MLP modes).  Dropped entries have weight exactly 0."""
    from deeprecommendation_amd import native
    assert native.attn_backward_supported(mode, A, Fdim)
    case = _att_case(A, Fdim, mode, lengths=ROWS)
    nnz = case["col"].numel()
    for msg_p in MSG_PS:
        msg_seed = msg_seed_of(A, msg_p)
        ref = reference(case, 0, None, msg_seed, msg_p)
        unit = 2.0 ** -64 if mode == ATT_MLP_SCALED else 1.0
        assert mode == ATT_COS or float(ref[3].abs().min()) >= unit / 32          # no element on the ReLU kink
        got = _run(native, case, gpu, msg_seed, msg_p)
        _hold(f"p={msg_p}", got, ref, mode)
        dropped = torch.from_numpy(~entry_keep(msg_seed, nnz, msg_p))
        assert 0 < int(dropped.sum()) < nnz and bool((got[1].cpu()[dropped] == 0).all())
    if mode != ATT_COS:
        hidden, msg_seed, msg_p = hidden_and_message(A)
        ref = reference(case, hidden[1], hidden[0], msg_seed, msg_p)
        _hold("hidden+message", _run(native, case, gpu, msg_seed, msg_p, hidden=hidden), ref, mode)
        w_plain = reference(case, 0, None, msg_seed, msg_p)[1]
        assert _misses_bar(w_plain, ref[1])                                      # the hidden mask was part of what was compared


def test_rows_whose_entries_are_all_dropped_give_the_bias(gpu):
    """One-entry rows: a dropped entry leaves an all -inf row — weight 0 and out == bias exactly; a kept one has weight exactly 1."""
    from deeprecommendation_amd import native
    msg_seed, msg_p = 5, 0.5
    for mode in (ATT_MLP, ATT_COS):
        case = _att_case(36, 100, mode, lengths=(1,) * 40, items=300)
        keep = torch.from_numpy(entry_keep(msg_seed, 40, msg_p))
        assert 0 < int(keep.sum()) < 40                               # the case holds dropped and kept one-entry rows
        out, wts, _ = _run(native, case, gpu, msg_seed, msg_p)
        out, wts = out.cpu(), wts.cpu()
        assert torch.equal(wts, keep.float())
        assert torch.equal(out[~keep], case["bias"].expand(int((~keep).sum()), -1))
        assert not bool((out[keep] == case["bias"]).all())
        _hold("one-entry rows", _run(native, case, gpu, msg_seed, msg_p), reference(case, 0, None, msg_seed, msg_p), mode)


@functools.lru_cache(maxsize=None)
def _zero_case(mode):
    """Rows of 1 .. 130 entries in which every third entry (and the whole of row 2) has a raw score of exactly 0.  Cosine: pc lives on
    the first half of the A = 16 columns and the pr row of a 'zero' item on the second half (disjoint supports: every product is 0).
    MLP (b1 = 0): pc <= -17/32 everywhere and the pr row of a 'zero' item <= 1/2, so every pc + pr < 0 and the ReLU gives 0; the other
    items have pr in [0, 3): some units active, some not (with every unit active d_pc would be w1 x sum_e ds_e = 0, and its bar with it).  Items 0..99 are 'zero' items, 100..399 are not."""
    rng = np.random.default_rng(17 + mode)
    A, Fdim, items, lengths = 16, 8, 400, (1, 7, 5, 64, 65, 130, 1, 20)
    B = len(lengths)
    rowptr = np.zeros(B + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lengths)
    cols, zero = [], []
    for b, n in enumerate(lengths):
        z = np.arange(n) % 3 == 0 if b != 2 else np.ones(n, dtype=bool)
        if b == 6:
            z[:] = False
        c = np.empty(n, dtype=np.int64)
        c[z], c[~z] = rng.permutation(100)[:int(z.sum())], 100 + rng.permutation(300)[:int((~z).sum())]
        order = np.argsort(c)
        cols.append(c[order]), zero.append(z[order])
    col, zero = np.concatenate(cols), np.concatenate(zero)
    if mode == ATT_COS:
        pc = np.concatenate([(2 * rng.integers(-16, 16, (B, A // 2)) + 1) / 32.0, np.zeros((B, A // 2))], axis=1)
        pr = rng.integers(1, 17, (items, A)) / 16.0
        pr[:100, :A // 2] = 0.0
    else:
        pc = -(2 * rng.integers(8, 16, (B, A)) + 1) / 32.0                       # -17/32 .. -31/32
        pr = np.concatenate([rng.integers(-16, 9, (100, A)) / 16.0, rng.integers(0, 48, (300, A)) / 16.0])
    g = torch.Generator().manual_seed(3 + mode)
    case = dict(mode=mode, A=A, Fdim=Fdim, B=B, b1=0.0, pc=torch.tensor(pc, dtype=torch.float32), pr=torch.tensor(pr, dtype=torch.float32),
                w1=torch.tensor(rng.standard_normal(A) * 0.5, dtype=torch.float32), rowptr=torch.from_numpy(rowptr),
                col=torch.from_numpy(col.astype(np.int32)), val=torch.tensor(rng.integers(1, 11, col.size) * 0.5 - 2.9, dtype=torch.float32),
                feat=torch.randn(items, Fdim, generator=g), bias=torch.randn(Fdim, generator=g), dout=torch.randn(B, Fdim, generator=g))
    return case, torch.from_numpy(zero)


@pytest.mark.parametrize("mode", [ATT_COS, ATT_MLP])
def test_a_kept_score_of_exactly_zero_is_dropped_too(gpu, mode):
    """The reference's `attOut[attOut == 0] = -inf`: entries whose score is exactly 0 get weight exactly 0 although the mask keeps
    them; row 2 (all such entries) gives the bias.  The float64 reference with the rule agrees at the bar; without it, it misses."""
    from deeprecommendation_amd import native
    case, zero = _zero_case(mode)
    msg_seed, msg_p = 21, 0.3
    keep = torch.from_numpy(entry_keep(msg_seed, zero.numel(), msg_p))
    assert int((zero & keep).sum()) >= 10 and int((~zero & keep).sum()) >= 10 and int((~zero & ~keep).sum()) >= 10
    ref = reference(case, 0, None, msg_seed, msg_p)
    b_of = torch.repeat_interleave(torch.arange(case["B"]), case["rowptr"][1:] - case["rowptr"][:-1])
    raw0 = (case["pc"].double()[b_of] * case["pr"].double()[case["col"].long()]).sum(1) if mode == ATT_COS else \
        torch.relu(case["pc"].double()[b_of] + case["pr"].double()[case["col"].long()]) @ case["w1"].double()
    assert bool((raw0[zero] == 0).all()) and bool((raw0[~zero] != 0).all())
    got = _run(native, case, gpu, msg_seed, msg_p)
    wts = got[1].cpu()
    assert bool((wts[zero] == 0).all()) and bool((wts[~zero & keep] > 0).all()) and bool((wts[~keep] == 0).all())
    assert torch.equal(got[0].cpu()[2], case["bias"])
    _hold("zero rule", got, ref, mode)
    without = reference(case, 0, None, msg_seed, msg_p, zero_rule=False)
    assert _misses_bar(without[1], ref[1]) and _misses_bar(got[1], without[1]) and _misses_bar(got[0], without[0])


def test_the_comparison_fails_for_another_seed_and_another_backward_p(gpu):
    """Another msg_seed misses the forward bar; a backward given another msg_p misses the d_pc, d_pr and d_w1 bars (their scale) while
    d_feat, which depends on the forward's weights alone, still passes."""
    from deeprecommendation_amd import native
    case = _att_case(128, 100, ATT_MLP, lengths=ROWS)
    msg_seed, msg_p = 31, 0.3
    out64, w64, g64, _ = reference(case, 0, None, msg_seed, msg_p)
    out_o, wts_o, _ = _run(native, case, gpu, msg_seed + 1, msg_p)
    assert _misses_bar(out_o, out64) and _misses_bar(wts_o, w64)
    out, wts, grads = _run(native, case, gpu, msg_seed, msg_p, msg_p_bwd=0.5)
    assert_close(out, out64)
    _grads_close(_Grads({"d_feat": grads["d_feat"]}), _Grads({"d_feat": g64["d_feat"]}), rtol=ATT_RTOL)
    for k in ("d_pc", "d_pr", "d_w1"):
        with pytest.raises(AssertionError):
            _grads_close(_Grads({k: grads[k]}), _Grads({k: g64[k]}), rtol=ATT_RTOL)


@pytest.mark.parametrize("mode", [ATT_MLP, ATT_MLP_SCALED, ATT_COS])
@pytest.mark.parametrize("A,Fdim", [(4, 4), (36, 100), (128, 64), (256, 256)])
def test_a_zero_message_threshold_is_the_plain_kernels(gpu, A, Fdim, mode):
    """msg_p = 1e-6 gives thr_m = 0: bit for bit the plain kernels, without and with the hidden dropout (and no zero rule).  No item
    is rated more than twice in this batch, so the float atomics of the backward are deterministic."""
    from deeprecommendation_amd import native
    assert threshold(P_THR0) == 0
    case = _att_case(A, Fdim, mode, lengths=(0, 1, 63, 64, 65, 300, 130), items=600, at_most_twice=True)
    assert int(torch.bincount(case["col"].long()).max()) <= 2
    for hidden in (None,) if mode == ATT_COS else (None, (0.3, 31)):
        out0, wts0, g0 = _run(native, case, gpu, 0, None, hidden=hidden)
        out1, wts1, g1 = _run(native, case, gpu, 77, P_THR0, hidden=hidden)
        assert torch.equal(out0, out1) and torch.equal(wts0, wts1)
        for k in g0:
            assert torch.equal(g0[k], g1[k]), k
        _, wts2, _ = _run(native, case, gpu, 77, 0.1, hidden=hidden)
        assert not torch.equal(wts0, wts2)


def test_train_entry_points_refuse_what_they_cannot_run(gpu):
    """NCF_ATT_LINEAR, A = 6, A = 260, Fdim = 6 and cosine with a hidden p > 0: NCF_EUNSUPPORTED, nothing launched (sentinels intact)."""
    from deeprecommendation_amd import native
    lib = native.load_library()
    B, I, n = 5, 30, 6
    g = torch.Generator().manual_seed(0)
    rowptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=gpu)
    col = torch.stack([torch.randperm(I, generator=g)[:n].sort().values for _ in range(B)]).reshape(-1).to(torch.int32).to(gpu)
    val = torch.ones(B * n, device=gpu)
    for mode, A, Fdim, hidden_p in ((ATT_LINEAR, 1, 8, 0.0), (ATT_MLP, 6, 8, 0.0), (ATT_MLP_SCALED, 6, 8, 0.0), (ATT_MLP, 260, 8, 0.0),
                                    (ATT_MLP, 16, 6, 0.0), (ATT_COS, 16, 8, 0.3)):
        feat = torch.randn(I, Fdim, generator=g).to(gpu)
        pc, pr, w1 = (torch.randn(s, generator=g).to(gpu) for s in ((B, A), (I, A), (A,)))
        out = torch.full((B, Fdim), 777.0, device=gpu)
        wts = torch.full((B * n,), 777.0, device=gpu)
        p = native._ptr
        rc = lib.ncf_attn_forward_train(mode, p(pc), A, p(pr), A, A, p(w1), 0.0, p(rowptr), p(col), p(val), B, I, p(feat), Fdim, Fdim, None,
                                        p(out), Fdim, p(wts), 5, hidden_p, 6, 0.3, native._stream(pc))
        torch.cuda.synchronize()
        assert rc == NCF_EUNSUPPORTED, (mode, A, Fdim, rc)
        assert bool((out == 777.0).all()) and bool((wts == 777.0).all())
        with pytest.raises(native.NativeError) as ei:
            native.attn_forward(mode, pc, pr, w1, 0.0, rowptr, col, val, feat, dropout=(hidden_p, 5), msg_dropout=(0.3, 6))
        assert ei.value.code == NCF_EUNSUPPORTED
        if hidden_p == 0.0:
            d_pc, d_pr, part = (torch.full(s, 777.0, device=gpu) for s in ((B, A), (I, A), (B, A)))
            d_feat, ds, dout = torch.full((I, Fdim), 777.0, device=gpu), torch.full((B * n,), 777.0, device=gpu), torch.ones(B, Fdim, device=gpu)
            rc = lib.ncf_attn_backward_train(mode, p(pc), A, p(pr), A, A, p(w1), p(rowptr), p(col), p(val), B, I, p(feat), Fdim, Fdim, p(wts),
                                             p(dout), Fdim, p(d_pc), A, p(d_pr), A, p(part), p(d_feat), Fdim, p(ds), 0, 0.0, 0.3,
                                             native._stream(pc))
            torch.cuda.synchronize()
            assert rc == NCF_EUNSUPPORTED, (mode, A, Fdim, rc)
            assert all(bool((t == 777.0).all()) for t in (d_pc, d_pr, part, d_feat, ds))


# =============================================================================================== the model
B_M, I_M, F_M = 48, 40, 36
MSG_P = 0.2


def _models(gpu, att_dense, cosine):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.manual_seed(4)
    m = AttentionNCF(item_dim=F_M, item_emb=64, user_emb=64, att_dense=att_dense, mlp_dense_layers=[128], use_cos_sim_instead=cosine,
                     message_dropout=MSG_P).train()
    _mlp_dropout_off(m)
    m_gpu = copy.deepcopy(m).to(gpu).train()
    m_gpu.message_dropout_on_device = True
    return m_gpu, copy.deepcopy(m).double().train()


def _restated(m_gpu, m_cpu, monkeypatch, cosine, seed_h=1301, seed_m=2602):
    """Both dropouts of the float64 CPU module replaced by the restated masks, and the GPU model's seeds fixed to the same two."""
    if not cosine:
        assert float(m_cpu.AttentionNet[2].p) == 0.2
        m_cpu.AttentionNet[2] = _MaskDropout(0.2, lambda call: seed_h, lambda call, n: np.arange(n))
    m_gpu._draw_attention_seeds = lambda: (None if cosine else seed_h, seed_m)
    fake = EntryMaskDropout(torch.nn.functional.dropout, seed_m, MSG_P)
    monkeypatch.setattr(torch.nn.functional, "dropout", fake)
    return fake


@pytest.mark.parametrize("cosine,att_dense", [(False, 32), (False, 128), (True, None)])
def test_model_step_with_message_dropout_on_device_matches_float64(gpu, monkeypatch, cosine, att_dense):
    """AttentionNCF(message_dropout=0.2).train() with the opt-in against the float64 CPU module through its torch branch, hidden and
    message dropout both replaced by the restated masks (entry e of the kernel is element e of the torch branch's logit vector: both
    list the (pair, rated entry) pairs row-major).  Loss 2e-5, weights 1e-5, every parameter gradient by _grads_close at 1e-4."""
    cand, rated, um, y = _attention_batch(B_M, I_M, F_M, seed=21)
    m_gpu, m_cpu = _models(gpu, att_dense, cosine)
    fake = _restated(m_gpu, m_cpu, monkeypatch, cosine)
    out_c, w_c = m_cpu(cand.double(), rated.double(), um.double(), return_attention_weights=True)
    assert fake.calls == 1
    loss_c = torch.nn.functional.mse_loss(out_c, y.double(), reduction="sum")
    loss_c.backward()
    out_g, w_g = m_gpu(cand.to(gpu), rated.to(gpu), um.to(gpu), return_attention_weights=True)
    assert out_g.requires_grad and fake.calls == 1                   # the GPU step drew nothing from F.dropout for the logits
    loss_g = torch.nn.functional.mse_loss(out_g, y.to(gpu), reduction="sum")
    loss_g.backward()
    lc, lg = float(loss_c.detach()), float(loss_g.detach())
    w_err = float((w_g.cpu().double() - w_c).abs().max())
    record_error("loss", abs(lg - lc), 2e-5 * abs(lc))
    record_error("attention weights", w_err, 1e-5)
    assert abs(lg - lc) <= 2e-5 * abs(lc)
    assert w_err <= 1e-5
    assert float(w_c[1, 3]) == 0.0 and float(w_g[1, 3]) == 0.0       # the candidate's own rated entry is masked
    valid = um != 0
    dropped = torch.from_numpy(~entry_keep(2602, int(valid.sum()), MSG_P))
    assert int(dropped.sum()) > 50 and bool((w_g.cpu()[valid][dropped] == 0).all())     # zeros at dropped entries
    zero = () if cosine else ("AttentionNet.3.bias",)
    _record_grads(m_gpu, m_cpu, 1e-4, exactly_zero=zero)
    _grads_close(m_gpu, m_cpu, rtol=1e-4, exactly_zero=zero)


def test_path_selection_and_eval_is_untouched(gpu, monkeypatch):
    """With the opt-in native.attn_forward receives msg_dropout = (p, seed); without it the same model makes no attn_forward call at
    all in training (the torch branch); in .eval() the output is bit-identical with and without the attribute."""
    from deeprecommendation_amd import native
    cand, rated, um, _ = _attention_batch(B_M, I_M, F_M, seed=21)
    m_gpu, _ = _models(gpu, 32, False)
    calls = []
    real = native.attn_forward
    monkeypatch.setattr(native, "attn_forward", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    args = (cand.to(gpu), rated.to(gpu), um.to(gpu))
    torch.manual_seed(9)
    m_gpu(*args)
    assert len(calls) == 1 and calls[0]["msg_dropout"][0] == MSG_P and calls[0]["dropout"][0] == 0.2
    assert calls[0]["msg_dropout"][1] != calls[0]["dropout"][1]
    calls.clear()
    m_gpu.message_dropout_on_device = False
    m_gpu(*args)
    assert calls == []
    m_gpu.eval()
    with torch.no_grad():
        off = m_gpu(*args)
        m_gpu.message_dropout_on_device = True
        on = m_gpu(*args)
    assert torch.equal(off, on) and all("msg_dropout" not in k for k in calls)


def test_forward_pairs_masks_the_two_halves_differently(gpu, monkeypatch):
    """One forward over 2B pairs (split = B): the mask is keyed by the position in the 2B-row CSR, so a user's positive and negative
    pair drop different entries, and the result equals the float64 reference over that CSR."""
    cand, rated, um, y = _attention_batch(B_M, I_M, F_M, seed=21)
    g = torch.Generator().manual_seed(8)
    cand2 = torch.cat([cand, (torch.rand(B_M, F_M, generator=g) < 0.3).float() * torch.rand(B_M, F_M, generator=g)])
    um2, y2 = torch.cat([um, um]), torch.cat([y, 5 - y])
    m_gpu, m_cpu = _models(gpu, 32, False)
    _restated(m_gpu, m_cpu, monkeypatch, False)
    out_c, w_c = m_cpu(cand2.double(), rated.double(), um2.double(), return_attention_weights=True, pair_split=B_M)
    pos, neg = m_gpu.forward_pairs(cand2.to(gpu), rated.to(gpu), um2.to(gpu), B_M)
    _, w_g = m_gpu(cand2.to(gpu), rated.to(gpu), um2.to(gpu), return_attention_weights=True, pair_split=B_M)
    assert pos.shape == neg.shape == (B_M, 1)
    loss_c = float(torch.nn.functional.mse_loss(out_c.detach(), y2.double(), reduction="sum"))
    loss_g = float(torch.nn.functional.mse_loss(torch.cat([pos, neg]).detach(), y2.to(gpu), reduction="sum"))
    record_error("loss", abs(loss_g - loss_c), 2e-5 * abs(loss_c))
    assert abs(loss_g - loss_c) <= 2e-5 * abs(loss_c)
    assert float((w_g.cpu().double() - w_c).abs().max()) <= 1e-5
    w_g = w_g.cpu()
    rows = [b for b in range(3, B_M) if not torch.equal(w_g[b] == 0, w_g[B_M + b] == 0)]
    assert len(rows) > B_M // 2                                       # same rated sets, other entries dropped


# =============================================================================================== train_model
def _fit(gpu, tmp_path, make_ds, val_ds, resident, seed, on_device=True):
    from deeprecommendation_amd.neural_collaborative_filtering.train import train_model
    from test_gpu_attention_resident_training import _model
    m = _model(message_dropout=0.1)
    m.message_dropout_on_device = on_device
    np.random.seed(1)
    torch.manual_seed(seed)
    mm = train_model(m, make_ds(), val_ds, lr=5e-3, weight_decay=0.0, batch_size=128, val_batch_size=256, early_stop=False,
                     final_model_path=None, checkpoint_model_path=str(tmp_path / "c.pt"), max_epochs=3, device=gpu, resident=resident,
                     shuffle=False, verbose=False)
    return mm["train_loss"]


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("pairwise", [False, True])
def test_train_model_runs_every_step_on_the_hip_blocks(gpu, tmp_path, monkeypatch, pairwise, resident):
    """train_model with the opt-in, point- and pair-wise, device-built batches and the DataLoader loop: every attention forward is
    native.attn_forward with msg_dropout, the device-built batches go through native.pair_rows, losses are finite and fall over 3
    epochs.  Two runs under one torch.manual_seed draw the same masks: the (hidden, message) seeds of every forward, which do not
    pass through the device, are EQUAL, step by step; the epoch losses agree to 1e-6 relative.  They cannot be held to ==: the
    backward adds d_pr / d_feat with float atomics in any order, so after the first step the weights of two runs differ in their last
    bits (test_resident_and_dataloader_epochs_agree records 2.9e-7 of the largest weight between two runs of one loop after 2 epochs,
    5 fp32 ulp), and an epoch loss, a smooth function of the weights, inherits a relative difference of that order; 1e-6 is about 3x
    that and 16 fp32 ulp.  A step that drew another mask moves an epoch loss by 1e-3 and more (a run under another seed is asserted
    to be further away than 1e-4).  Measured on an MI355X over the four cases: same seed 0 .. 2.6e-8, another seed 2.4e-3 .. 8.7e-3."""
    from deeprecommendation_amd import native
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import DynamicPointwiseDataset
    from test_gpu_attention_resident_training import _datasets, _toy
    prov, ranking, point, val = _toy()
    make = (lambda: _datasets(prov, ranking, point)[1]) if pairwise else (lambda: _datasets(prov, ranking, point)[0])
    val_ds = DynamicPointwiseDataset(val, prov)
    fwd, rows = [], []
    real_fwd, real_rows = native.attn_forward, native.pair_rows

    def spy_fwd(*a, **k):
        if "dropout" in k:                                            # AttnFn's call (a training step), not the validation pass's
            fwd.append((k.get("msg_dropout"), k.get("dropout")))
        return real_fwd(*a, **k)

    monkeypatch.setattr(native, "attn_forward", spy_fwd)
    monkeypatch.setattr(native, "pair_rows", lambda *a, **k: (rows.append(1), real_rows(*a, **k))[1])
    la = _fit(gpu, tmp_path, make, val_ds, resident, seed=11)
    steps = 3 * -(-len(make()) // 128)
    assert len(fwd) >= steps and all(k is not None and k[0] == 0.1 for k, _ in fwd)
    assert len(set(k[1] for k, _ in fwd)) == len(fwd)                 # a fresh message seed for every forward
    seeds_a = list(fwd)
    fwd.clear()
    assert (len(rows) >= steps) if resident else True
    assert len(la) == 3 and all(np.isfinite(la)) and la[-1] < la[0]
    lb = _fit(gpu, tmp_path, make, val_ds, resident, seed=11)
    assert fwd == seeds_a                                             # the same seeds in the same order: the same masks
    fwd.clear()
    lc = _fit(gpu, tmp_path, make, val_ds, resident, seed=12)
    assert len(fwd) == len(seeds_a) and all(x[0][1] != y[0][1] for x, y in zip(fwd, seeds_a))
    same = max(abs(x - y) / abs(y) for x, y in zip(la, lb))
    other = max(abs(x - y) / abs(y) for x, y in zip(lc, lb))
    print(f"\n[msgdrop train pairwise={pairwise} resident={resident}] losses {la}; same seed {same:.3e}, other seed {other:.3e}")
    record_error("same-seed epoch losses", same, 1e-6)
    assert same <= 1e-6 and other > 1e-4
