"""What the NeuMF tests share (test_neumf_cpu.py, test_gpu_neumf.py), none of it needing a GPU:

  * ``gmf_fp32``: the GMF term g of include/ncf_abi.h (under ncf_neumf_score) restated in numpy fp32, one rounded operation per
    line (numpy's float32 array arithmetic rounds every product and sum on its own: there is no FMA to fall into);
  * ``finish_fp32``: the two final sums, fl(fl(s_mlp + g) + bl), taking s_mlp as input;
  * ``forward_f64``: the whole model in float64 from its tables and weights, out-of-range ids reading zero rows;
  * the bar of tests/test_gpu_basic.py:20-33, |a - ref| <= 1e-5 |ref| + 1e-6 max|ref|, as ``assert_close``."""
import numpy as np
import torch

RTOL = 1e-5


def gmf_fp32(w, p, q):
    """g (B,) float32 of the rows p, q (B, D) and weights w (D,), all float32, D a multiple of 8: per lane half h, a_h = +0 then
    for s, j ascending with d = 8 s + 4 h + j: t = fl(w[d] p[d]); v = fl(t q[d]); a_h = fl(a_h + v); g = fl(a_0 + a_1)."""
    w, p, q = (np.ascontiguousarray(x, dtype=np.float32) for x in (w, p, q))
    B, D = p.shape
    assert D % 8 == 0 and q.shape == (B, D) and w.shape == (D,)
    a = [np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.float32)]
    for s in range(D // 8):
        for h in range(2):
            for j in range(4):
                d = 8 * s + 4 * h + j
                t = w[d] * p[:, d]
                v = t * q[:, d]
                a[h] = a[h] + v
                assert t.dtype == v.dtype == a[h].dtype == np.float32
    return a[0] + a[1]


def finish_fp32(s_mlp, g, bl):
    """score = fl(fl(s_mlp + g) + bl), float32 arrays and a float32 scalar."""
    s = np.asarray(s_mlp, dtype=np.float32).reshape(-1) + np.asarray(g, dtype=np.float32).reshape(-1)
    return s + np.float32(bl)


def gather_rows(tab, idx):
    """Rows of ``tab`` (CPU tensor) under the kernels' range rule: an id outside the table reads zeros."""
    i = idx.long().cpu()
    ok = (i >= 0) & (i < tab.shape[0])
    rows = tab[torch.where(ok, i, torch.zeros_like(i))].clone()
    rows[~ok] = 0
    return rows


def forward_f64(tabU, tabI, gmfU, gmfI, weights, biases, w, users, items):
    """(B,) float64 scores: weights = [W1, (W2,) wl (1, N)], biases = [b1, (b2,) bl (1,)], w (D,); every hidden layer has its ReLU."""
    d = lambda t: t.detach().cpu().double()
    x = torch.cat((gather_rows(d(tabU), users), gather_rows(d(tabI), items)), 1)
    for W, b in zip(weights[:-1], biases[:-1]):
        x = torch.relu(x @ d(W).t() + d(b))
    g = (d(w) * gather_rows(d(gmfU), users) * gather_rows(d(gmfI), items)).sum(1)
    return (x @ d(weights[-1]).t()).squeeze(1) + g + d(biases[-1]).reshape(())


def assert_close(a, ref, what=""):
    a, ref = torch.as_tensor(a).detach().cpu().double().reshape(-1), torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    assert a.shape == ref.shape, what
    tol = RTOL * ref.abs() + 0.1 * RTOL * ref.abs().max()
    err = (a - ref).abs()
    assert bool((err <= tol).all()), f"{what}: max abs err {err.max().item():.3e}, ref scale {ref.abs().max().item():.3e}"
