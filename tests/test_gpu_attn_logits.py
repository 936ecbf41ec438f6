"""ncf_attn_logits: the (rated x candidate) logit table of csrc/attn_cross.hip, bit for bit against the float64 reference.

The operands are dyadic with few significant bits, as attn_forms_ref.make_inputs builds them (pc odd multiples of 1/32, pr multiples of
1/16, w1 in {-1, 0, 1} / 16; cosine rows multiples of 1/8; the scaled mode carries 2^-64 / 2^64): every partial sum of a logit is
exact in fp32 whatever its order, so equality with ``scores64(...).t().float()`` is the right bar.  pc and pr are column slices of
wider poisoned buffers; the table sits in a sentinel-filled buffer with ldst = I_c + 4 whose padding must stay untouched."""
import numpy as np
import pytest
import torch

import attn_forms_ref as R
from attn_cross_ref import table64

pytestmark = pytest.mark.gpu

# (mode, A, I_c, I_r, ld pad of pc / pr): both edges partial, one and several tiles on each axis, every A (and A = 1 for linear)
CASES = [
    (R.ATT_MLP, 4, 1, 1, 4), (R.ATT_MLP, 32, 63, 65, 1), (R.ATT_MLP, 36, 129, 64, 4), (R.ATT_MLP, 128, 300, 63, 4), (R.ATT_MLP, 256, 65, 129, 3),
    (R.ATT_MLP_SCALED, 4, 64, 300, 4), (R.ATT_MLP_SCALED, 32, 129, 1, 4), (R.ATT_MLP_SCALED, 36, 65, 63, 2), (R.ATT_MLP_SCALED, 128, 63, 129, 4),
    (R.ATT_MLP_SCALED, 256, 300, 65, 4),
    (R.ATT_COS, 4, 300, 129, 4), (R.ATT_COS, 32, 1, 300, 4), (R.ATT_COS, 36, 64, 64, 1), (R.ATT_COS, 128, 65, 300, 4), (R.ATT_COS, 256, 129, 63, 4),
    (R.ATT_LINEAR, 1, 300, 65, 4), (R.ATT_LINEAR, 1, 63, 1, 1), (R.ATT_LINEAR, 1, 129, 300, 3),
]


def _operands(mode, A, Ic, Ir, seed):
    rng = np.random.default_rng(seed)
    w1, b1 = None, 0.0
    if mode in (R.ATT_MLP, R.ATT_MLP_SCALED):
        pc = (2 * rng.integers(-8, 8, (Ic, A)) + 1) / 32.0
        pr = rng.integers(-16, 17, (Ir, A)) / 16.0
        w1 = rng.integers(-1, 2, A) / 16.0
        b1 = R.B1
        if mode == R.ATT_MLP_SCALED:
            pc, pr, w1 = pc * 2.0 ** -R.SCALE_LOG2, pr * 2.0 ** -R.SCALE_LOG2, w1 * 2.0 ** R.SCALE_LOG2
    elif mode == R.ATT_LINEAR:
        pc = (2 * rng.integers(-8, 8, (Ic, 1)) + 1) / 32.0
        pr = rng.integers(-48, 49, (Ir, 1)) / 16.0
    else:
        pc = rng.integers(-8, 9, (Ic, A)) / 8.0
        pr = rng.integers(-8, 9, (Ir, A)) / 8.0
    t = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=torch.float32)
    return t(pc), t(pr), t(w1), b1


@pytest.mark.parametrize("mode,A,Ic,Ir,pad", CASES, ids=lambda v: str(v))
def test_logit_table_is_exact(gpu, mode, A, Ic, Ir, pad):
    from deeprecommendation_amd import native
    pc, pr, w1, b1 = _operands(mode, A, Ic, Ir, 31 * A + Ic + 7 * Ir + mode)
    want = table64(mode, pc, pr, w1, b1)
    assert torch.equal(want, want.float().double())                   # exact in fp32: equality is the bar
    pc_buf, pr_buf = R.wide(pc, A + pad).to(gpu), R.wide(pr, A + pad + 4).to(gpu)
    w1_buf = None if w1 is None else R.wide(w1[None], A + 8)[0].to(gpu)
    st = torch.full((Ir, Ic + 4), R.SENTINEL, dtype=torch.float32, device=gpu)
    got = native.attn_logits(mode, pc_buf[:, :A], pr_buf[:, :A], None if w1 is None else w1_buf[:A], b1, out=st[:, :Ic])
    assert got.data_ptr() == st.data_ptr()
    st = st.cpu()
    assert bool((st[:, Ic:] == R.SENTINEL).all()), "a padding column of the table was written"
    assert torch.equal(st[:, :Ic], want.float())
    # the table does not depend on how it was tiled: a sub-table computed on its own has the same bits
    i0, e0 = Ic // 3, Ir // 2
    sub = native.attn_logits(mode, pc_buf[i0:, :A], pr_buf[e0:, :A], None if w1 is None else w1_buf[:A], b1).cpu()
    assert torch.equal(sub, st[e0:, i0:Ic])
    fresh = native.attn_logits(mode, pc_buf[:, :A], pr_buf[:, :A], None if w1 is None else w1_buf[:A], b1)
    assert fresh.shape == (Ir, Ic) and fresh.is_contiguous() and torch.equal(fresh.cpu(), st[:, :Ic])
