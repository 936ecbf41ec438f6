"""The arithmetic contract of the bf16 scoring kernels (score_fused_bf16_kernel, score_ws_bf16_kernel, score_ws8_bf16_kernel), stated in
float64, and the checks that hold a scorer to it (tests/test_gpu_bf16_contract.py on the GPU, tests/test_bf16_contract_cpu.py on CPU
models of a right and of several wrong kernels).

THE CONTRACT (oracle/ncf_oracle.py, basic_ncf_forward_indexed_bf16): table rows and the weight matrices of the hidden layers are bf16
numbers (rounded to nearest even from fp32); every matrix product accumulates in fp32; where a hidden layer feeds another matrix product
(the first of two hidden layers) its ReLU'd activations are rounded to bf16, to nearest even; biases, the last hidden layer, the 1-wide
last layer (its weights too) and the output are fp32.  An out-of-range id makes that table's half of the row zeros.

A "scorer" below is any callable ``score(ws, bs) -> 1-D float32 CPU tensor`` that scores one fixed batch of pairs with the fp32 [out][in]
weight matrices ``ws`` and biases ``bs`` (it rounds the hidden layers' matrices to bf16 itself, as ncf_mlp_pack does).  The intermediate
values of a scorer are read out through that one entry point with PROBE weights (read_h1 / read_h2).

Nothing here needs a GPU or the native library (ncf_case builds a BasicNCF on the CPU for its weights)."""
import numpy as np
import torch

U = 2.0 ** -23          # an fp32 half-ulp, doubled: an accumulator that truncates instead of rounding is still inside the bounds
RTOL = 1e-5             # the project's fp32 bar (tests/test_gpu_basic.py, assert_close at its defaults) ...
FLOOR = 0.1             # ... with its absolute part: a tenth of the relative bar on the largest output


# ------------------------------------------------------------------------------------------------ bf16 in float64
def _mantissa(v):
    """|v| = q * 2^e with q in [128, 256) (bf16 has 8 significant bits): returns (q, 2^e); q = 0 for v = 0."""
    m, e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))
    return m * 256.0, np.ldexp(1.0, e - 8)


def round_bf16(t, mode="rne"):
    """A float64 tensor rounded to bf16 precision directly (no fp32 step in between), result in float64.  ``mode``: "rne" (to nearest,
    ties to even: the contract), "trunc" (drop the low bits: towards zero), "half_up" (to nearest, ties away from zero).  Normal range
    only: the tests' values are far from bf16's subnormals and overflow."""
    v = t.detach().double().numpy()
    q, scale = _mantissa(v)
    q = {"rne": np.rint, "trunc": np.floor, "half_up": lambda x: np.floor(x + 0.5)}[mode](q)
    return torch.from_numpy(np.copysign(q * scale, v))


def ulp_bf16(t):
    """Spacing of the bf16 numbers in the binade of |t| (float64 tensor); 0 for 0."""
    q, scale = _mantissa(t.detach().double().numpy())
    return torch.from_numpy(np.where(q > 0, scale, 0.0))


def is_bf16(t32):
    """Elementwise: the fp32 value is a bf16 number (low 16 bits of its pattern are zero)."""
    assert t32.dtype == torch.float32
    return (t32.contiguous().view(torch.int32) & 0xFFFF) == 0


def rounding_census(pre):
    """How the ReLU'd float64 pre-activations ``pre`` meet bf16: counts of ties resolved downwards / upwards by ties-to-even, of
    non-tie roundings downwards / upwards, of values that need no rounding, and the share of negative pre-activations."""
    v = torch.relu(pre).numpy()
    q, _ = _mantissa(v)
    lo = np.floor(q)
    frac = q - lo
    tie = frac == 0.5
    even = np.mod(lo, 2.0) == 0.0
    return {"tie_down": int((tie & even).sum()), "tie_up": int((tie & ~even).sum()),
            "down": int(((frac > 0) & (frac < 0.5)).sum()), "up": int((frac > 0.5).sum()),
            "inexact_share": float((frac > 0).mean()), "negative_share": float((pre < 0).double().mean())}


# ------------------------------------------------------------------------------------------------ the contract in float64
def gather_rows(ta, ia, tb, ib):
    """cat(ta[ia], tb[ib]) in float64; an out-of-range id reads as a zero row of that table."""
    def rows(t, idx):
        ok = (idx >= 0) & (idx < t.shape[0])
        return t.double()[idx.clamp(0, t.shape[0] - 1)] * ok.double()[:, None]
    return torch.cat((rows(ta, ia), rows(tb, ib)), 1)


def bf16_weights64(ws):
    """The matrices as the kernels use them, in float64: hidden layers rounded to bf16 (RNE), the 1-wide last layer as it is."""
    return [w.to(torch.bfloat16).double() for w in ws[:-1]] + [ws[-1].double()]


def contract64(x, ws, bs, mode="rne"):
    """The contract evaluated in float64 on rows ``x`` (float64, bf16 numbers): returns (scores (B,), [pre-activation of every layer]).
    ``mode`` is how the first of TWO hidden layers is re-rounded (round_bf16); "rne" is the contract."""
    w64 = bf16_weights64(ws)
    h, pre = x, []
    for li, (w, b) in enumerate(zip(w64, bs)):
        a = h @ w.t() + b.double()
        pre.append(a)
        if li == len(w64) - 1:
            return a[:, 0], pre
        h = torch.relu(a)
        if li < len(w64) - 2:
            h = round_bf16(h, mode)


def magnitudes64(x, ws, bs, mode="rne"):
    """Per layer, max over pairs and units of |input| @ |W|^T + |b| along the contract: what no partial sum of that layer, taken in any
    order, exceeds in magnitude."""
    w64 = bf16_weights64(ws)
    h, out = x, []
    for li, (w, b) in enumerate(zip(w64, bs)):
        out.append(float((h.abs() @ w.abs().t() + b.double().abs()).max()))
        h = torch.relu(h @ w.t() + b.double())
        if li < len(w64) - 2:
            h = round_bf16(h, mode)
    return out


# ------------------------------------------------------------------------------------------------ Part A: exact integer cases
def exact_case(EA, EB, hidden, rows=(3000, 700)):
    """Integer-valued tables and weights for which every fp32 partial sum of every layer is an exact integer in any summation order (the
    caller asserts it: magnitudes64 < 2^24), while the first hidden layer's activations DO need rounding to bf16, ties included: table
    entries in [-3, 3], W1 dense in [-31, 31], b1 in [-100, 100]; with two hidden layers W2 dense in [-3, 3], b2 in [-1000, 1000]; last
    layer in {-1, 0, 1}, its bias in [-100, 100].  Returns (ta, tb, ws, bs): fp32 tensors holding integers that are bf16 numbers where
    the kernels keep bf16."""
    g = torch.Generator().manual_seed(1000 * EA + 10 * EB + len(hidden))

    def ri(bound, *shape):
        return torch.randint(-bound, bound + 1, shape, generator=g).float()

    dims = [EA + EB] + list(hidden) + [1]
    ta, tb = ri(3, rows[0], EA), ri(3, rows[1], EB)
    ws, bs = [ri(31, dims[1], dims[0])], [ri(100, dims[1])]
    if len(hidden) == 2:
        ws.append(ri(3, dims[2], dims[1]))
        bs.append(ri(1000, dims[2]))
    ws.append(ri(1, 1, dims[-2]))
    bs.append(ri(100, 1))
    return ta, tb, ws, bs


def batch_ids(B, rows, seed):
    """Random ids that also cover row 0 and the last row of both tables (as far as B allows)."""
    g = torch.Generator().manual_seed(seed)
    ia = torch.randint(0, rows[0], (B,), generator=g)
    ib = torch.randint(0, rows[1], (B,), generator=g)
    ia[0], ib[0] = 0, rows[1] - 1
    if B > 1:
        ia[1], ib[1] = rows[0] - 1, 0
    return ia, ib


def exact_conditions(x, ws, bs):
    """What an exact case has to satisfy BEFORE a scorer is looked at, as a list of (name, holds, detail); conditions on the inputs, not
    measurements.  ``x``: float64 rows of at least a few thousand pairs."""
    ref, pre = contract64(x, ws, bs)
    mags = magnitudes64(x, ws, bs)
    out = [("every partial sum below 2^24", max(mags) < 2 ** 24, mags),
           ("a quarter of layer-1 pre-activations negative", float((pre[0] < 0).double().mean()) >= 0.25, None),
           ("1000 distinct reference scores", ref.unique().numel() >= 1000, ref.unique().numel())]
    if len(ws) == 3:
        c = rounding_census(pre[0])
        out.append(("1000 ties and 1000 non-tie roundings each way", min(c["tie_down"], c["tie_up"], c["down"], c["up"]) >= 1000, c))
        for mode in ("trunc", "half_up"):
            share = float((contract64(x, ws, bs, mode)[0] != ref).double().mean())
            out.append((f"{mode} changes more than 90 % of the scores", share > 0.9, share))
    return out


# ------------------------------------------------------------------------------------------------ Part B: operands and probes
def ncf_case(EA, EB, hidden, rows=(3000, 700)):
    """Tables and MLP of a freshly initialised BasicNCF (the construction of test_score_fused_bf16_vs_oracle): returns (ta, tb, ws, bs,
    state) with the tables already bf16 (RNE of W^T + b, what the model's bf16 scoring path builds) and ws / bs in fp32."""
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from oracle import ncf_oracle as O
    torch.manual_seed(EA + EB + len(hidden))
    m = BasicNCF(item_dim=rows[1], user_dim=rows[0], item_emb=EB, user_emb=EA, mlp_dense_layers=list(hidden)).eval()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ta = O.embedding_table(state["user_embeddings.0.weight"], state["user_embeddings.0.bias"]).to(torch.bfloat16)
    tb = O.embedding_table(state["item_embeddings.0.weight"], state["item_embeddings.0.bias"]).to(torch.bfloat16)
    layers = O.mlp_weights(state)
    return ta, tb, [w for w, _ in layers], [b for _, b in layers], state


def layer1_probe(ws, bs, s, n):
    """Weights under which the score IS the scorer's rounded hidden activation h1[:, unit]: W2 a 0/1 selection matrix (row m picks
    hidden unit m + N2 * s), b2 = 0, last layer one-hot at n, its bias 0.  One product by 1.0 plus exact zeros; h1 >= 0, so the second
    ReLU is the identity.  Returns (ws, bs, unit)."""
    N2, N1 = ws[1].shape
    sel = torch.zeros(N2, N1)
    sel[torch.arange(N2), torch.arange(N2) + N2 * s] = 1.0
    wl = torch.zeros(1, N2)
    wl[0, n] = 1.0
    return [ws[0], sel, wl], [bs[0], torch.zeros(N2), torch.zeros(1)], n + N2 * s


def layer2_probe(ws, bs, n):
    """Weights under which the score IS the scorer's fp32 second hidden activation H2[:, n]: the real first two layers, last layer one-hot."""
    wl = torch.zeros(1, ws[1].shape[0])
    wl[0, n] = 1.0
    return [ws[0], ws[1], wl], [bs[0], bs[1], torch.zeros(1)]


def read_h1(score, ws, bs):
    """(B, N1) float32: every hidden unit of the first layer as the scorer computes it; N1 probe launches."""
    N2, N1 = ws[1].shape
    assert N1 % N2 == 0
    cols = [None] * N1
    for s in range(N1 // N2):
        for n in range(N2):
            pw, pb, unit = layer1_probe(ws, bs, s, n)
            cols[unit] = score(pw, pb)
    return torch.stack(cols, 1)


def read_h2(score, ws, bs):
    """(B, N2) float32: the second hidden layer as the scorer computes it; N2 probe launches."""
    return torch.stack([score(*layer2_probe(ws, bs, n)) for n in range(ws[1].shape[0])], 1)


# ------------------------------------------------------------------------------------------------ Part B: the bounds
class Check:
    """One per-element comparison: ``bad`` elements over their bound, the worst element's error and bound (for record_error)."""

    def __init__(self, name, err, bar, also_bad=None):
        used = err / bar.clamp_min(1e-300)
        k = int(used.argmax())
        self.name, self.err, self.bar = name, float(err.flatten()[k]), float(bar.flatten()[k])
        wrong = err > bar
        if also_bad is not None:
            wrong = wrong | also_bad
        self.bad, self.n = int(wrong.sum()), err.numel()

    @property
    def ok(self):
        return self.bad == 0

    def __repr__(self):
        return f"{self.name}: {self.bad} of {self.n} over the bound, worst {self.err:.3e} against {self.bar:.3e}"


def check_layer1(h1, x, ws, bs):
    """1. Every observed h1 is a bf16 number, >= 0, and within ulp_bf16(relu(a)) / 2 + (K0 + 1) u S1 of relu(a), a = x @ W1^T + b1 and
    S1 = |x| @ |W1|^T + |b1| in float64 on the bf16 operands: RNE of a sum accumulated in fp32, no tolerance added.  ulp_bf16(0) = 0:
    where a < 0 the observed value may be the accumulation term above zero at most."""
    w = bf16_weights64(ws)[0]
    a = torch.relu(x @ w.t() + bs[0].double())
    S1 = x.abs() @ w.abs().t() + bs[0].double().abs()
    bar = ulp_bf16(a) / 2 + (w.shape[1] + 1) * U * S1
    return Check("layer 1", (h1.double() - a).abs(), bar, also_bad=~is_bf16(h1) | (h1 < 0))


def check_layer2(h2, h1, ws, bs):
    """2. |H2 - relu(h1 @ W2^T + b2)| <= (N1 + 1) u S2, float64 from the scorer's OWN observed h1, S2 = h1 @ |W2|^T + |b2|."""
    w = bf16_weights64(ws)[1]
    ref = torch.relu(h1.double() @ w.t() + bs[1].double())
    S2 = h1.double().abs() @ w.abs().t() + bs[1].double().abs()
    return Check("layer 2", (h2.double() - ref).abs(), (w.shape[1] + 1) * U * S2)


def check_last(score, h2, ws, bs):
    """3. |score - (H2 @ wl^T + bl)| <= (N2 + 1) u S3 from the scorer's own observed H2; wl in fp32."""
    w = ws[-1].double()
    ref = (h2.double() @ w.t() + bs[-1].double())[:, 0]
    S3 = (h2.double().abs() @ w.abs().t() + bs[-1].double().abs())[:, 0]
    return Check("last layer", (score.double() - ref).abs(), (w.shape[1] + 1) * U * S3)


def check_close(name, score, ref):
    """4. The fp32 bar of the suite: |a - ref| <= 1e-5 |ref| + 1e-6 max|ref| (assert_close of tests/test_gpu_basic.py at its defaults)."""
    ref = ref.double()
    return Check(name, (score.double() - ref).abs(), RTOL * ref.abs() + FLOOR * RTOL * ref.abs().max())


def tail64(h1, ws, bs):
    """The layers after the first, in float64, from observed first-layer activations."""
    w = bf16_weights64(ws)
    return (torch.relu(h1.double() @ w[1].t() + bs[1].double()) @ w[2].t() + bs[2].double())[:, 0]


def rne_mismatch_share(h1, x, ws, bs):
    """5. Share of hidden units whose observed value differs from RNE of the float64 activation (reported, not bounded)."""
    a = torch.relu(x @ bf16_weights64(ws)[0].t() + bs[0].double())
    return float((h1.double() != round_bf16(a)).double().mean())


def contract_checks(score, x, ws, bs, oracle=None):
    """Every Part B assertion on one scorer and batch.  Two hidden layers: reads h1 and H2 through the probes, repeats one probe launch
    (run-to-run equality is what lets a value observed in one launch be the input of the next stage's reference), and returns
    ([Check ...], share of check 5, repeat_equal).  One hidden layer (nothing is re-rounded): the score against ``oracle`` only."""
    real = score(ws, bs)
    if len(ws) == 2:
        return [check_close("end to end", real, oracle)], None, bool(torch.equal(real, score(ws, bs)))
    h1 = read_h1(score, ws, bs)
    pw, pb, unit = layer1_probe(ws, bs, 1, 5)
    repeat_equal = bool(torch.equal(score(pw, pb), h1[:, unit]))
    h2 = read_h2(score, ws, bs)
    checks = [check_layer1(h1, x, ws, bs), check_layer2(h2, h1, ws, bs), check_last(real, h2, ws, bs),
              check_close("end to end", real, tail64(h1, ws, bs))]
    return checks, rne_mismatch_share(h1, x, ws, bs), repeat_equal
