"""The training step against the REFERENCE's own numbers (round 3 fixtures g3_att_train_*, g7_grads_*: made by
tests/golden/make_golden.py from the imported reference in deterministic train mode — dropout 0 / None, no message dropout):

  * forward in ``.train()``: AttentionNCF's target mask (attention_ncf.py:195-205) — outputs and attention weights;
  * loss = ``MSELoss(reduction='sum')`` (datasets/base.py:19-20,31-32) and EVERY parameter gradient after ``.backward()``.

CPU tests run the mirror's torch-op path (host logic, `-m "not gpu"`); the `gpu` tests run the HIP autograd blocks
(LinearFn / GatherColumnsConcatFn / AttnFn → libncf_hip.so) and compare with the same reference gradients.
Bars: fp32, summation order differs from the reference's ATen kernels only → 1e-5 of the largest element per tensor
(gradients) and 1e-5 relative (loss, outputs)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, onehot, record_error

ATT_CASES = ["g3_att_train_dense8", "g3_att_train_cos", "g3_att_train_vec64", "g3_att_train_ue50", "g3_att_train_peaked"]
BASIC_CASES = ["g7_grads_basic_small", "g7_grads_basic_e64", "g7_grads_basic_h256", "g7_grads_mf"]


def _compare(model, a, out, att, loss, tag, rtol=1e-5):
    ref_out = torch.from_numpy(a["out"]).double()
    o = out.detach().cpu().double()
    err = float((o - ref_out).abs().max() / ref_out.abs().max())
    record_error(tag + ":out", err, rtol)
    assert err <= rtol, f"out: {err:.3e}"
    if att is not None:
        ref_att = torch.from_numpy(a["att"]).double()
        e = float((att.detach().cpu().double() - ref_att).abs().max())
        record_error(tag + ":att", e, rtol)
        assert e <= rtol, f"attention weights: {e:.3e}"
        assert bool(((att.detach().cpu() == 0) == (ref_att == 0)).all())       # the same entries are masked / unrated
    el = abs(float(loss.detach()) - float(a["loss"])) / abs(float(a["loss"]))
    record_error(tag + ":loss", el, rtol)
    assert el <= rtol
    named = dict(model.named_parameters())
    assert set(named) == set(a["grads"])
    worst = 0.0
    noise = 1e-8 * abs(float(a["loss"]))
    for k, g in a["grads"].items():
        p = named[k]
        assert p.grad is not None, k
        got = p.grad.detach().cpu().double()
        assert got.shape == g.shape, k
        scale = float(g.abs().max())
        e = float((got - g.double()).abs().max())
        if scale <= noise:
            # a gradient that is zero by construction — AttentionNet's output bias: a shift of all scores cancels in the softmax —
            # comes out of the reference's autograd as fp32 rounding noise (6e-8 in g3_att_train_vec64) and out of the HIP
            # backward as an exact 0: both must stay inside the noise floor, 1e-8 of the loss
            assert e <= noise and float(got.abs().max()) <= noise, k
            continue
        worst = max(worst, e / scale)
        assert e <= rtol * scale, f"{k}: max abs err {e:.3e} vs largest reference element {scale:.3e}"
    record_error(tag + ":grads", worst, rtol)


def _attention_step(name, device, tag):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    state, a, kw = load_golden(name)
    m = AttentionNCF(**kw)
    m.load_state_dict(state)
    m = m.to(device).train()
    cand, rated, um = (torch.from_numpy(a[k]).to(device) for k in ("candidate_items", "rated_items", "user_matrix"))
    out, att = m(cand, rated, um, return_attention_weights=True)
    loss = torch.nn.MSELoss(reduction="sum")(out, torch.from_numpy(a["y"]).to(device).view(-1, 1).float())
    loss.backward()
    _compare(m, a, out, att, loss, tag)
    for b, c in enumerate(a["self_cols"]):
        assert float(att[b, c]) == 0.0            # attention_ncf.py:195-205
    return m


def _basic_step(name, device, tag, indexed):
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    state, a, kw = load_golden(name)
    m = (MF if name.endswith("_mf") else BasicNCF)(**kw)
    m.load_state_dict(state)
    m = m.to(device).train()
    if indexed:
        xu, xi = torch.as_tensor(a["user_pos"]).to(device), torch.as_tensor(a["item_pos"]).to(device)
    else:
        xu, xi = onehot(a["user_pos"], kw["user_dim"]).to(device), onehot(a["item_pos"], kw["item_dim"]).to(device)
    out = m(xu, xi)
    loss = torch.nn.MSELoss(reduction="sum")(out, torch.from_numpy(a["y"]).to(device).view(-1, 1).float())
    loss.backward()
    _compare(m, a, out, None, loss, tag)
    return m


# ------------------------------------------------------------------------------------------ CPU: the mirror's torch-op path
@pytest.mark.parametrize("name", ATT_CASES)
def test_attention_train_step_torch_path_vs_reference(name):
    _attention_step(name, torch.device("cpu"), f"cpu:{name}")


@pytest.mark.parametrize("name", BASIC_CASES)
def test_basic_train_step_torch_path_vs_reference(name):
    _basic_step(name, torch.device("cpu"), f"cpu:{name}", indexed=False)


# ------------------------------------------------------------------------------------------ GPU: the HIP autograd blocks
@pytest.mark.gpu
@pytest.mark.parametrize("name", ATT_CASES)
def test_attention_train_step_hip_blocks_vs_reference(gpu, name):
    m = _attention_step(name, gpu, f"hip:{name}")
    from deeprecommendation_amd import native
    kw = m.kwargs
    if name == "g3_att_train_ue50":
        # user_emb = 50 is not a multiple of 4: the attention backward kernel does not take it, the step must still run
        # (torch ops) instead of raising from loss.backward() — ADVICE round 2
        assert not native.attn_backward_supported(native.ATT_MLP, int(kw["att_dense"]), int(kw["user_emb"]))
    else:
        mode = native.ATT_COS if kw["use_cos_sim_instead"] else native.ATT_MLP
        assert native.attn_backward_supported(mode, int(kw["item_emb"] if kw["use_cos_sim_instead"] else kw["att_dense"]), int(kw["user_emb"]))


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [True, False])
@pytest.mark.parametrize("name", BASIC_CASES)
def test_basic_train_step_hip_blocks_vs_reference(gpu, name, indexed):
    _basic_step(name, gpu, f"hip:{name}:{'idx' if indexed else 'onehot'}", indexed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ATT_CASES[:3])
def test_attention_train_mode_forward_eval_kernels_agree_with_reference_eval(gpu, name):
    """The same fixture in eval mode has no reference output stored; the train-mode forward with the target mask lifted
    (no candidate equals a rated row once the candidates are perturbed) must equal the eval kernels' output: ties the
    train path (per-pair AttnFn) to the eval path (grouped / per-pair kernels) that the g3_att_* goldens pin."""
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    state, a, kw = load_golden(name)
    m = AttentionNCF(**kw)
    m.load_state_dict(state)
    m = m.to(gpu)
    cand = torch.from_numpy(a["candidate_items"]).to(gpu) + 0.01
    rated, um = torch.from_numpy(a["rated_items"]).to(gpu), torch.from_numpy(a["user_matrix"]).to(gpu)
    with torch.no_grad():
        ev, ev_att = m.eval()(cand, rated, um, return_attention_weights=True)
    tr, tr_att = m.train()(cand, rated, um, return_attention_weights=True)
    assert float((tr.detach() - ev).abs().max()) <= 1e-5 * float(ev.abs().max())
    assert float((tr_att - ev_att).abs().max()) <= 1e-5
