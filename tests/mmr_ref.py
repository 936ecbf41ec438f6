"""THE CONTRACT of ncf_mmr_rerank (include/ncf_abi.h) restated in numpy, three times:

  (a) ``rerank(..., kind="f32")``    the fp32 emulator in the kernel's documented order: every product and sum rounded on its own, a
                                     similarity summed sequentially in ascending d from +0.0f
  (b) ``rerank(..., kind="f64")``    the float64 twin (similarities by a float64 matrix product)
  (c) ``rerank(..., kind="exact")``  a plain loop for exactly representable inputs (small integer vectors, scores that are multiples
                                     of 1/8, lambda a multiple of 1/4): similarities from an exact float64 Gram matrix, so the result
                                     does not depend on any summation order

and the case sets of tests/test_gpu_mmr.py, which tests/test_mmr_cpu.py shows not to be vacuous by seeding defects (``defect=``)
into the reference.  Cases are built once per process and never written to."""
import functools

import numpy as np

MAX_N, MAX_D, MAX_K = 256, 256, 128
DEFECTS = ("tie_high", "last_sim", "no_one_minus", "step0_scaled", "dead_picked", "norm_all")


def _best(v, open_, high=False):
    """The contract's comparator over the open slots: the largest value, ties to the lower slot, NaN last."""
    idx = np.flatnonzero(open_)
    vv = v[idx]
    ok = ~np.isnan(vv)
    if ok.any():
        idx, vv = idx[ok], vv[ok]
        idx = idx[vv == vv.max()]
    return int(idx[-1] if high else idx[0])


def seq_dot_f32(rows, p):
    """sim(j, p) for every row j in fp32: acc = +0.0f; acc = acc + rows[j, d] * rows[p, d] for d ascending (an accumulate runs
    sequentially along a row; the leading zero column makes the first step 0 + product)."""
    prod = np.zeros((rows.shape[0], rows.shape[1] + 1), dtype=np.float32)
    prod[:, 1:] = rows * rows[p]
    return np.add.accumulate(prod, axis=1, dtype=np.float32)[:, -1]


def seq_dot_loop(rows, p):
    """seq_dot_f32 as the explicit loop (slow; tests/test_mmr_cpu.py holds the two together)."""
    acc = np.zeros(rows.shape[0], dtype=np.float32)
    for d in range(rows.shape[1]):
        acc = acc + rows[:, d] * rows[p, d]
    return acc


def rerank_user(vec, score, pos, n, K, lam, normalize, kind="f32", defect=None, trace=None):
    """One user.  vec (n_items, D) fp32, score (N,) fp32, pos (N,) int64, n slots in use.  Returns (slots, values, oob): the picks in
    order (at most K), their values when picked in the kind's dtype, and whether the out-of-range flag is raised.  ``trace``: a list
    that receives every step's (values, open mask)."""
    dt = np.float32 if kind == "f32" else np.float64
    N = score.shape[0]
    n_items = vec.shape[0]
    n = min(max(int(n), 0), N)
    used = np.arange(N) < n
    inside = (pos >= 0) & (pos < n_items)
    live = used & inside & np.isfinite(score)
    oob = bool((used & ~inside & (pos != -1)).any())
    sc = score.astype(dt)
    lam_t = dt(np.float32(lam))
    one_minus = dt(np.float32(1.0) - np.float32(lam)) if kind == "f32" else dt(1.0) - lam_t
    open_ = (used & inside) if defect == "dead_picked" else live.copy()
    with np.errstate(all="ignore"):
        if normalize:
            sel = np.isfinite(score) if defect == "norm_all" else live
            rel = np.zeros(N, dtype=dt)
            if sel.any():
                lo, hi = sc[sel].min(), sc[sel].max()
                if hi != lo:
                    rel = (sc - lo) / (hi - lo)
        else:
            rel = sc
        rows = np.zeros((N, vec.shape[1]), dtype=dt)
        rows[open_] = vec[pos[open_]]
        if kind != "f32":
            gram = rows @ rows.T               # float64; exact for the inputs of kind="exact"
        m = np.full(N, -np.inf, dtype=dt)
        cnt = min(int(K), int(open_.sum()))
        slots, values = [], []
        for t in range(cnt):
            if t == 0:
                v = lam_t * rel if defect == "step0_scaled" else rel
            elif defect == "no_one_minus":
                v = lam_t * rel - m
            else:
                v = lam_t * rel - one_minus * m
            if trace is not None:
                trace.append((v.copy(), open_.copy()))
            s = _best(v, open_, high=defect == "tie_high")
            slots.append(s)
            values.append(v[s])
            open_[s] = False
            if t + 1 == cnt:
                break
            sim = seq_dot_f32(rows, s) if kind == "f32" else gram[:, s]
            upd = open_ if defect == "last_sim" else open_ & (sim > m)
            m[upd] = sim[upd]
    return slots, values, oob


def rerank(case, kind="f32", defect=None):
    """A whole case: (slot (B, K) int32, value (B, K) fp32 [float64 for kind="f64"], count (B,) int32, oob)."""
    B, N = case["score"].shape
    K = case["K"]
    vec = case["vec"][:, :case["D"]]
    slot = np.full((B, K), -1, dtype=np.int32)
    value = np.full((B, K), -np.inf, dtype=np.float64 if kind == "f64" else np.float32)
    count = np.zeros(B, dtype=np.int32)
    oob = False
    for b in range(B):
        n = N if case["count"] is None else case["count"][b]
        s, v, o = rerank_user(vec, case["score"][b], case["pos"][b], n, K, case["lam"], case["normalize"], kind, defect)
        slot[b, :len(s)] = s
        value[b, :len(s)] = v
        count[b] = len(s)
        oob |= o
    return slot, value, count, oob


# ---------------------------------------------------------------------------------------------------------------- exact cases
EXACT_N = (1, 2, 63, 64, 65, 128, 256)
EXACT_D = (4, 60, 64, 128, 256)
EXACT_LAM = (0.0, 0.25, 0.5, 1.0)


def _exact_case(N, D, K, lam, B, seed, ldv=None, null_count=False):
    rng = np.random.default_rng(seed)
    n_items = max(3, N // 2 + 1)                  # fewer items than slots: duplicate positions in every wide pool
    ldv = D if ldv is None else ldv
    vec = rng.integers(-3, 4, size=(n_items, ldv)).astype(np.float32)
    score = (rng.integers(-16, 17, size=(B, N)) / 8.0).astype(np.float32)         # unsorted, few distinct values: ties everywhere
    pos = rng.integers(0, n_items, size=(B, N)).astype(np.int64)
    count = None
    if not null_count:
        menu = [N, 0, 1, max(K - 1, 0), N // 2, N + 5, -3]                        # full, empty, one, below K, half, over N, negative
        count = np.array([menu[(b + seed) % len(menu)] for b in range(B)], dtype=np.int32)
    for b in range(B):
        for j in rng.integers(0, N, size=max(1, N // 8) if N >= 8 or b % 2 else 0):  # dead slots inside the count
            what = rng.integers(0, 4)
            if what == 0:
                pos[b, j] = -1
            else:
                score[b, j] = (np.nan, np.inf, -np.inf)[what - 1]
    return dict(name=f"N{N}-D{D}-K{K}-lam{lam}-B{B}-ldv{ldv}" + ("-nullcount" if null_count else ""), vec=vec, D=D, score=score, pos=pos,
                count=count, K=K, lam=lam, normalize=0, n_items=n_items)


@functools.lru_cache(maxsize=None)
def exact_cases():
    """Every N x D of the grid with K in {1, 2, min(N, 128)}; lambda, the leading dimension (D: 16-byte rows; D + 1: single floats; D + 4)
    and a NULL count rotate through the cases so that each meets each width.  B = 4 pools apart from the B = 0 / 1 / 300 cases."""
    cases, i = [], 0
    for N in EXACT_N:
        for D in EXACT_D:
            for K in sorted({1, min(2, N), min(N, MAX_K)}):
                lam = EXACT_LAM[i % 4]
                ldv = (D, D + 1, D + 4)[(i // 4) % 3]
                cases.append(_exact_case(N, D, K, lam, 4, 1000 + i, ldv, null_count=i % 5 == 4))
                i += 1
    for lam in EXACT_LAM:                             # every lambda on the widest staged and on the unstaged path, at the largest K
        cases.append(_exact_case(256, 128, 128, lam, 2, 2000 + len(cases)))
        cases.append(_exact_case(256, 256, 128, lam, 2, 2000 + len(cases), null_count=True))
    cases.append(_exact_case(65, 60, 2, 0.5, 0, 3000))
    cases.append(_exact_case(64, 64, 64, 0.25, 1, 3001))
    cases.append(_exact_case(65, 60, 20, 0.5, 300, 3002))                          # more pools than CUs
    cases.append(_exact_case(128, 64, 20, 0.25, 300, 3003, null_count=True))
    return tuple(cases)


# ---------------------------------------------------------------------------------------------------------------- float cases
def _float_case(N, D, K, lam, normalize, B, seed, n_items=None, ldv=None, counts=False):
    rng = np.random.default_rng(seed)
    n_items = 4 * N if n_items is None else n_items
    ldv = D if ldv is None else ldv
    vec = np.zeros((n_items, ldv), dtype=np.float32)
    g = rng.standard_normal((n_items, D))
    vec[:, :D] = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    score = rng.uniform(0.0, 1.0, size=(B, N)).astype(np.float32)
    pos = np.stack([rng.permutation(n_items)[:N] for _ in range(B)]).astype(np.int64) if n_items >= N else \
        rng.integers(0, n_items, size=(B, N)).astype(np.int64)
    count = rng.integers(0, N + 1, size=B).astype(np.int32) if counts else None
    return dict(name=f"N{N}-D{D}-K{K}-lam{lam}-norm{normalize}-B{B}-ldv{ldv}", vec=vec, D=D, score=score, pos=pos, count=count, K=K, lam=lam,
                normalize=normalize, n_items=n_items)


@functools.lru_cache(maxsize=None)
def float_cases():
    """The shape grid thinned to a dozen cases, lambda in {0.3, 0.7}, both normalize settings, against the fp32 emulator bit for bit."""
    spec = [(1, 4, 1, 0.3, 1, 5), (2, 60, 2, 0.7, 0, 5), (63, 64, 63, 0.3, 0, 6), (64, 128, 2, 0.7, 1, 6), (65, 256, 65, 0.3, 1, 5),
            (128, 60, 128, 0.7, 1, 5), (128, 64, 20, 0.3, 0, 40), (256, 4, 1, 0.7, 0, 5), (256, 128, 32, 0.3, 1, 12), (256, 256, 128, 0.7, 0, 3),
            (256, 256, 20, 0.3, 1, 6), (65, 64, 20, 0.7, 1, 300)]
    return tuple(_float_case(N, D, K, lam, nz, B, 4000 + i, ldv=(D, D + 1, D + 4)[i % 3], counts=i % 2 == 1)
                 for i, (N, D, K, lam, nz, B) in enumerate(spec))


TWIN_MARGIN = 1e-5        # a pick sequence may leave the float64 twin's only where the twin's two values are closer than this
TWIN_CAP = 0.01           # ... and for at most this share of a case's users


@functools.lru_cache(maxsize=None)
def twin_cases():
    """The three shapes at which sequential fp32 was checked against float64 (200 users each; tests/test_mmr_cpu.py re-checks)."""
    return (_float_case(128, 64, 20, 0.5, 1, 200, 5000), _float_case(256, 128, 32, 0.3, 1, 200, 5001), _float_case(64, 32, 16, 0.7, 0, 200, 5002))


@functools.lru_cache(maxsize=None)
def twin_traces(i):
    """Per user of twin case i: (slots of the float64 twin, the twin's per-step (values, open mask))."""
    case = twin_cases()[i]
    out = []
    for b in range(case["score"].shape[0]):
        tr = []
        s, _, _ = rerank_user(case["vec"][:, :case["D"]], case["score"][b], case["pos"][b], case["score"].shape[1], case["K"], case["lam"],
                              case["normalize"], "f64", trace=tr)
        out.append((s, tr))
    return out


def twin_verdict(i, slots):
    """``slots`` (B, K) against the float64 twin of twin case i: (users left out, users that differ beyond the margin).  A user whose
    sequence leaves the twin's is left out iff at the first differing step the twin's values of the two slots are within TWIN_MARGIN."""
    left_out, wrong = [], []
    for b, (want, tr) in enumerate(twin_traces(i)):
        got = [int(s) for s in slots[b][:len(want)]]
        if got == want:
            continue
        t = next(t for t in range(len(want)) if got[t] != want[t])
        v, open_ = tr[t]
        if 0 <= got[t] < len(v) and open_[got[t]] and abs(v[want[t]] - v[got[t]]) < TWIN_MARGIN:
            left_out.append(b)
        else:
            wrong.append(b)
    return left_out, wrong


# ---------------------------------------------------------------------------------------------------------------- cluster fixture
def cluster_fixture(n_clusters=4, per_cluster=16, D=16, seed=7):
    """Tight clusters of unit vectors and a pool whose relevance favours cluster 0, then 1, ...: (vec (n_items, D) fp32, score (1, N),
    pos (1, N), cluster of every item)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    g = np.repeat(centres, per_cluster, axis=0) + 0.02 * rng.standard_normal((n_clusters * per_cluster, D))
    vec = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    cluster = np.repeat(np.arange(n_clusters), per_cluster)
    score = (1.0 - 0.1 * cluster + 0.05 * rng.uniform(size=cluster.size)).astype(np.float32)
    return vec, score[None, :], np.arange(cluster.size, dtype=np.int64)[None, :], cluster


def ild_ref(positions, counts, vec):
    """intra_list_diversity in float64: the mean over unordered pairs of 1 - vec[a] . vec[b]; NaN under two items; -1 is no item."""
    out = np.full(positions.shape[0], np.nan)
    for b in range(positions.shape[0]):
        p = positions[b, :counts[b]]
        p = p[p >= 0]
        tot, n = 0.0, 0
        for x in range(len(p)):
            for y in range(x + 1, len(p)):
                tot += 1.0 - float(np.dot(vec[p[x]].astype(np.float64), vec[p[y]].astype(np.float64)))
                n += 1
        if n:
            out[b] = tot / n
    return out


def coverage_ref(positions, counts, n_items):
    seen = set()
    for b in range(positions.shape[0]):
        seen.update(int(p) for p in positions[b, :counts[b]] if 0 <= p < n_items)
    return len(seen) / n_items
