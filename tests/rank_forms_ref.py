"""What the tests of the ranking kernels' launch forms share (test_rank_forms_cpu.py, test_gpu_rank_forms.py), none of it needing a GPU:

  * the three host plans restated in Python (topk.hip topk_merge_plan, dot_frag.h dot_topk_tile_cols, mlp_topk.hip mlp_tile_cols),
    held to ncf_ranking_plan and the workspace queries by the CPU test;
  * FORMS: the forms each fused entry point can be launched in, and CASES: the smallest shapes that reach each of them;
  * a vectorised exact oracle in torch (Ranking) that runs on the device of its inputs: the contract of topk_common.h /
    rank_common.h over int64 keys, no Python loop over rows;
  * exact integer data: tables (and MLP weights) whose scores are the same fp32 bits in every summation order, so the reference is
    plain float64 torch and needs no sibling kernel; random rows with heavy ties and adversarial column orders (ascending,
    descending, plateaus over the tile / bitmap-chunk / range boundaries, a sawtooth of period 32, one all-NaN column);
  * exclusion lists and targets that reach every bitmap chunk of a tile."""
import numpy as np
import torch

# ------------------------------------------------------------------------------------------------------------------ the plans
TOPK_TILE = 8192                 # topk_common.h kTopkTile
CHUNK_BYTES = 256 << 20          # kTopkChunkBytes
DOT_BLOCK_USERS, DOT_CHUNK, DOT_TARGET_BLOCKS = 64, 2048, 512        # dot_frag.h
MLP_COLS, MLP_RANK_CHUNK_COLS, MLP_TARGET_WAVES = 32, 512, 2048     # mlp_topk.hip
ENTRIES = ("topk_rows", "rank_rows", "dot_topk", "dot_rank", "mlp_topk", "mlp_rank")


def kp(k):
    return (k + 1) & ~1


def merge_plan(rows, n1, k, align=1):
    """topk_merge_plan: (levels, n1, n2, chunk)."""
    levels, tiles, n = 0, [], n1
    while n > 0:
        t = -(-n // TOPK_TILE)
        tiles.append(t)
        levels += 1
        n = 0 if t == 1 else t * kp(k)
    n2 = tiles[0] * kp(k) if levels > 1 else 0
    per_row = (n1 + n2) * 8
    chunk = max(1, min(rows, CHUNK_BYTES // per_row)) if per_row else rows
    if chunk < rows and chunk > align:
        chunk -= chunk % align
    return levels, n1, n2, chunk


def dot_tile_cols(rows, cols):
    ublocks = -(-rows // DOT_BLOCK_USERS)
    t = TOPK_TILE
    while t > DOT_CHUNK and ublocks * -(-cols // t) < DOT_TARGET_BLOCKS:
        t >>= 1
    return t


def mlp_tile_cols(rows, cols, floor_cols):
    t = TOPK_TILE
    while t > floor_cols and rows * -(-cols // t) < MLP_TARGET_WAVES:
        t >>= 1
    return t


def _merge(entry, rows, cols, kt):
    """(tile_cols, merge_plan or None) of an entry point for (rows, cols) and its k / max_targets."""
    if entry == "topk_rows":
        t0 = -(-cols // TOPK_TILE)
        return TOPK_TILE, merge_plan(rows, t0 * kp(kt) if t0 > 1 else 0, kt)
    if entry == "rank_rows":
        return TOPK_TILE, None
    if entry in ("dot_topk", "dot_rank"):
        t = dot_tile_cols(rows, cols)
        return t, merge_plan(rows, -(-cols // t) * kp(kt), kt, DOT_BLOCK_USERS) if entry == "dot_topk" else None
    if entry == "mlp_topk":
        t = mlp_tile_cols(rows, cols, MLP_COLS)
        return t, merge_plan(rows, -(-cols // t) * kp(kt), kt)
    if entry == "mlp_rank":
        return mlp_tile_cols(rows, cols, MLP_COLS if kt == 1 else MLP_RANK_CHUNK_COLS), None
    raise KeyError(entry)


def plan(entry, rows, cols, kt):
    """(tile_cols, tiles, merge_levels, chunk_rows): what native.ranking_plan answers."""
    t, m = _merge(entry, rows, cols, kt)
    return (t, -(-cols // t), m[0], m[3]) if m else (t, -(-cols // t), 0, rows)


def topk_workspace_bytes(entry, rows, cols, k, n1_state=0, user_first=True):
    """The key workspace a top-K entry's plan implies (+ ncf_mlp_topk's layer-1 state of n1_state floats per first-part row)."""
    _, m = _merge(entry, rows, cols, k)
    state = (rows if user_first else cols) * n1_state * 4 if entry == "mlp_topk" else 0
    return state + m[3] * (m[1] + m[2]) * 8


# ------------------------------------------------------------------------------------------------------------------ the forms
DOT_TILES = (2048, 4096, 8192)
MLP_TILES = (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192)
MLP_MULTI_TILES = (512, 1024, 2048, 4096, 8192)
INSTANCES = [(64, 256, 128), (64, 256, 0), (64, 128, 0), (64, 128, 64), (128, 256, 128), (128, 256, 0), (128, 128, 0),
             (128, 128, 64), (256, 256, 128), (256, 256, 0), (256, 128, 0)]
MAIN = (128, 256, 128)

# A form is (tile_cols, exclusion list given); a top-K form with chunk_rows < rows carries "chunked" in front.
# ncf_mlp_topk in row chunks is left out: its key workspace is 256 MiB, so chunk_rows < rows needs about 3 x 10^9 pairs.
FORMS = {
    "dot_topk": {(t, e) for t in DOT_TILES for e in (False, True)} | {("chunked", 8192, e) for e in (False, True)},
    "dot_rank_one": {(t, e) for t in DOT_TILES for e in (False, True)},
    "dot_rank_multi": {(t, e) for t in DOT_TILES for e in (False, True)},
    "mlp_topk": {(t, e) for t in MLP_TILES for e in (False, True)},
    "mlp_rank_one": {(t, e) for t in MLP_TILES for e in (False, True)},
    "mlp_rank_multi": {(t, e) for t in MLP_MULTI_TILES for e in (False, True)},
}

DOT_ROWS, MLP_ROWS = 12800, 700
CHUNKED = dict(rows=130, cols=1 << 24, k=128, chunks=(64, 64, 2))
K_CYCLE = (1, 10, 100, 128)


def form_cols(tile):
    return 2 * tile + 40


def cases():
    """Every case the GPU tests run (test_gpu_rank_forms.py takes its parameters from here through select()), with the form it
    claims: family, entry, rows, cols, kt (k or max_targets), excl, tile, and per family the data (dot: kind, D, ids = through an
    item id list; MLP: inst)."""
    out = []

    def add(family, entry, rows, tile, kt, excl, **data):
        out.append(dict(family=family, entry=entry, rows=rows, cols=form_cols(tile), tile=tile, kt=kt, excl=excl, form=(tile, excl),
                        **data))

    def dot(tile, excl, ks, mts, **data):
        for k in ks:
            add("dot_topk", "dot_topk", DOT_ROWS, tile, k, excl, **data)
        for mt in mts:
            add("dot_rank_one" if mt == 1 else "dot_rank_multi", "dot_rank", DOT_ROWS, tile, mt, excl, **data)

    for e in (False, True):
        for t in DOT_TILES:
            for kind in ("random", "adversarial"):
                dot(t, e, (1, 100, 128), (1, 16) + ((128,) if t == 8192 else ()), kind=kind, D=16, ids=False)
        for n, inst in enumerate(INSTANCES):
            for t in MLP_TILES if inst == MAIN else (1024,):
                for k in sorted({100, K_CYCLE[(n + MLP_TILES.index(t)) % 4]}):
                    add("mlp_topk", "mlp_topk", MLP_ROWS, t, k, e, inst=inst)
                add("mlp_rank_one", "mlp_rank", MLP_ROWS, t, 1, e, inst=inst)
                if t >= MLP_RANK_CHUNK_COLS:
                    for mt in (3, 128) if inst == MAIN else (16,):
                        add("mlp_rank_multi", "mlp_rank", MLP_ROWS, t, mt, e, inst=inst)
        out.append(dict(family="dot_topk", entry="dot_topk", rows=CHUNKED["rows"], cols=CHUNKED["cols"], tile=8192, kt=CHUNKED["k"],
                        excl=e, form=("chunked", 8192, e), kind="chunked", D=4, ids=False))
    dot(4096, True, (100,), (16,), kind="adversarial", D=16, ids=True)
    dot(8192, True, (100,), (16,), kind="random", D=256, ids=False)
    return out


def select(**want):
    """The cases whose fields equal `want`."""
    return [c for c in cases() if all(c.get(f) == v for f, v in want.items())]


def kts(**want):
    """The k / max_targets values of the selected cases, ascending."""
    return sorted({c["kt"] for c in select(**want)})


def case_form(c, plan_fn=plan):
    """The form a case runs by the plan (plan_fn: the restated plan, or native.ranking_plan)."""
    tile, _, _, chunk = plan_fn(c["entry"], c["rows"], c["cols"], c["kt"])
    return (tile, c["excl"]) if chunk == c["rows"] else ("chunked", tile, c["excl"])


# ------------------------------------------------------------------------------------------------------------------ the oracle
_I64_MIN = -(1 << 63)


def key_map(scores):
    """topk_common.h's topk_map of an fp32 tensor, as int64 in [0, 2^32): -0.0 folded onto +0.0, every NaN mapped to 0."""
    u = scores.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    m = torch.where((u & 0x80000000) != 0, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return torch.where(torch.isnan(scores), torch.zeros_like(m), m)


def keys_of(scores):
    """map(score) << 32 | ~col as a signed int64 that orders like the kernels' unsigned key (the map's top bit flipped).  The
    smallest real key is a NaN's at column 2^24 - 1, far above int64 min, which marks an excluded column."""
    cols = torch.arange(scores.shape[1], device=scores.device, dtype=torch.int64).expand(scores.shape)
    return ((key_map(scores) - (1 << 31)) << 32) | (0xFFFFFFFF - cols)


def seen_mask(seen, R, C, dev):
    """(R, C) bool of a CSR exclusion list (rowptr int64, col int32); duplicates and ids outside [0, C) do nothing."""
    mask = torch.zeros((R, C), dtype=torch.bool, device=dev)
    if seen is None:
        return mask
    rowptr, col = seen
    rowptr, col = rowptr.to(dev), col.to(dev).to(torch.int64)
    n = int(rowptr[-1])
    col = col[:n]
    rows = torch.repeat_interleave(torch.arange(R, device=dev), rowptr[1:] - rowptr[:-1])
    ok = (col >= 0) & (col < C)
    mask[rows[ok], col[ok]] = True
    return mask


class Ranking:
    """The exact ranking of every row of an (R, C) fp32 score matrix with the excluded columns removed: one ascending sort of the
    int64 keys answers top-K for any k and the rank of any target."""

    def __init__(self, scores, seen=None):
        self.scores = scores
        self.R, self.C = scores.shape
        keys = keys_of(scores)
        mask = seen_mask(seen, self.R, self.C, scores.device)
        self.keys = torch.where(mask, torch.full_like(keys, _I64_MIN), keys)
        self.ranked = (self.C - mask.sum(1)).to(torch.int32)
        self.sorted = torch.sort(self.keys, dim=1).values

    def topk(self, k):
        """(score (R, k) fp32, idx (R, k) int32, count (R,) int32), slots past the count -inf / -1."""
        kk = min(k, self.C)
        top = self.sorted[:, self.C - kk:].flip(1)
        live = top != _I64_MIN
        col = 0xFFFFFFFF - (top & 0xFFFFFFFF)
        score = torch.where(live, self.scores.gather(1, col.clamp(0, self.C - 1)), torch.full_like(top, -float("inf"), dtype=torch.float32))
        idx = torch.where(live, col, torch.full_like(col, -1)).to(torch.int32)
        if kk < k:
            pad = (self.R, k - kk)
            score = torch.cat([score, torch.full(pad, -float("inf"), device=score.device)], 1)
            idx = torch.cat([idx, torch.full(pad, -1, dtype=torch.int32, device=idx.device)], 1)
        return score, idx, torch.minimum(self.ranked, torch.tensor(k, dtype=torch.int32, device=idx.device))

    def rank(self, targets):
        """(rank (n_targets,) int32, ranked (R,) int32) of a target CSR (rowptr int64, col int32): the live keys above the
        target's; -1 for a target that is excluded or outside [0, C)."""
        dev = self.scores.device
        rowptr, col = targets[0].to(dev), targets[1].to(dev).to(torch.int64)
        n = int(rowptr[-1])
        col = col[:n]
        lens = rowptr[1:] - rowptr[:-1]
        rows = torch.repeat_interleave(torch.arange(self.R, device=dev), lens)
        place = torch.arange(n, device=dev) - rowptr[:-1][rows]
        ok = (col >= 0) & (col < self.C)
        tkey = self.keys[rows, col.clamp(0, self.C - 1)]
        ok &= tkey != _I64_MIN
        width = max(1, int(lens.max()) if self.R else 1)
        padded = torch.full((self.R, width), (1 << 63) - 1, dtype=torch.int64, device=dev)
        padded[rows, place] = tkey
        above = self.C - torch.searchsorted(self.sorted, padded, right=True)
        rank = torch.where(ok, above[rows, place], torch.full_like(place, -1)).to(torch.int32)
        return rank, self.ranked


def lists_csr(lists, dev="cpu"):
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64, device=dev)
    flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if len(lists) else np.zeros(0, dtype=np.int64)
    return rowptr, torch.tensor(flat, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------------------------ the data
EXACT = 1 << 24        # every integer of magnitude below 2^24 is an fp32 value, and sums of such stay exact while below it
NAN_ITEM = lambda cols: cols // 2 + 1          # the column whose score is a NaN for every user
_DIRS = (-2, -1, 1, 2)


def patterns(cols, tile):
    """(3, cols) int64: g0 ascending (the column itself); g1 plateaus: 5 over [tile - 100, tile + 100) (it straddles the range
    boundary, a 32-column MFMA tile and, from tile 2048 on, a bitmap chunk), 4 over [2032, 2064), 3 over [28, 36), else a value in
    {0, 1, 2}; g2 a sawtooth of period 32."""
    c = torch.arange(cols, dtype=torch.int64)
    g1 = (c * 7919 + 3) % 3
    for lo, hi, v in ((28, 36, 3), (2048 - 16, 2048 + 16, 4), (tile - 100, tile + 100, 5)):
        g1[max(lo, 0):max(min(hi, cols), 0)] = v
    return torch.stack([c, g1, c % 32])


def _randint(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def dot_tables(rows, cols, tile, D, kind):
    """(users (rows, D), items (cols, D)) int64 with sum |a||b| < 2^24 (asserted).  random: every entry in -2 .. 2 (scores in
    -4 D .. 4 D: heavy ties).  adversarial: user r is s e_p with s in {-2, -1, 1, 2} and p = r mod 3, item coordinate p is pattern
    g_p, so the row is +- g_p; one item row is all NaN (set by dot_float)."""
    if kind == "random":
        A, B = _randint((rows, D), -2, 2, 11), _randint((cols, D), -2, 2, 12)
    else:
        B = _randint((cols, D), -3, 3, 13)
        B[:, :3] = patterns(cols, tile).t()
        A = torch.zeros((rows, D), dtype=torch.int64)
        r = torch.arange(rows)
        A[r, r % 3] = torch.tensor(_DIRS)[(r // 3) % 4]
    assert int(A.abs().max(0).values @ B.abs().max(0).values) < EXACT
    return A, B


def dot_float(A, B, kind, dev):
    """fp32 tables on the device; the adversarial item table gets its all-NaN row."""
    a, b = A.to(torch.float32).to(dev), B.to(torch.float32).to(dev)
    if kind != "random":
        b[NAN_ITEM(b.shape[0])] = float("nan")
    return a, b


def dot_scores(a, b):
    """The (rows, cols) fp32 scores of fp32 integer tables, from a float64 product (exact, so equal to any fp32 summation order;
    + 0.0 turns a -0.0 into the +0.0 an fmaf chain from +0.f gives)."""
    return ((a.double() @ b.double().t()) + 0.0).float()


def int_mlp(inst, cols, tile, rows, seed=0):
    """Integer MLP data for a fused instance (K0, N1, N2), both parts K0 / 2 wide: dict(users (rows, E), items (cols, E), Wu, Wi
    (N1, E), b1, W2, b2 (or None), wl (1, N), bl) as int64 / float tensors, with |W| . |h|max + |b| < 2^24 asserted for every neuron
    of every layer (int64; the bound of a layer is the next one's |h|max).
    Item features: g0, g1, g2 (patterns), x (+inf in row NAN_ITEM, else 0), the rest in -2 .. 2.  User features: six 0/1 selectors,
    an `adversarial` flag, the rest in -2 .. 2 (0 for adversarial users).  Even users are adversarial, kind (r / 2) mod 6.
    Layer 1: neuron 2p = relu(g_p - M (1 - f_2p)), neuron 2p + 1 = relu(G_p - g_p - M (1 - f_2p+1)), M = 2^15 > every g: the selected
    one passes +-g_p, the others are 0.  The other neurons have fan-in 8 from {-1, 1} over the random features and -M on the
    adversarial flag.  Layer 2 passes neurons 0 .. 5 through and mixes the rest with fan-in 6; the last layer sums the pattern
    neurons and 12 of the rest.
    The NaN column: the kernels' ReLU is fmaxf(x, 0), which turns a NaN into 0 (relu() below), so a NaN has to be made in the
    last layer.  Its inputs 6 and 7 are both +inf in column NAN_ITEM and 0 elsewhere, with weights +1 and -1: inf - inf = NaN in
    every order.  Without a second hidden layer they are layer-1 neurons reading x; with one, layer-1 neuron 6 alone reads x and
    layer-2 neurons 6 and 7 both read it (a neuron that met 0 * inf is a NaN and leaves its ReLU as 0, so no neuron may see two
    infinities)."""
    K0, N1, N2 = inst
    E, M = K0 // 2, 1 << 15
    g = patterns(cols, tile)
    assert int(g.max()) < M
    items = _randint((cols, E), -2, 2, seed + 1)
    items[:, :3] = g.t()
    items[:, 3] = 0
    users = _randint((rows, E), -2, 2, seed + 2)
    users[:, :7] = 0
    r = torch.arange(rows)
    adv = r % 2 == 0
    users[adv] = 0
    users[r[adv], (r[adv] // 2) % 6] = 1
    users[adv, 6] = 1

    def sparse(n_out, n_in, lo, fan, sd):
        W = torch.zeros((n_out, n_in), dtype=torch.int64)
        gen = torch.Generator().manual_seed(sd)
        for _ in range(fan):
            col = torch.randint(lo, n_in, (n_out,), generator=gen)
            W[torch.arange(n_out), col] = torch.randint(0, 2, (n_out,), generator=gen) * 2 - 1
        return W

    Wu, Wi = sparse(N1, E, 7, 4, seed + 3), sparse(N1, E, 4, 4, seed + 4)
    b1 = _randint((N1,), -2, 2, seed + 5)
    Wu[:8], Wi[:8], b1[:8] = 0, 0, 0
    Wu[8:, 6] = -M
    G = g.max(1).values
    for p in range(3):
        Wi[2 * p, p], Wu[2 * p, 2 * p], b1[2 * p] = 1, M, -M
        Wi[2 * p + 1, p], Wu[2 * p + 1, 2 * p + 1], b1[2 * p + 1] = -1, M, int(G[p]) - M
    Wi[6, 3] = 1
    if not N2:
        Wi[7, 3] = 1
    bound = Wu.abs() @ users.abs().max(0).values + Wi.abs() @ items.abs().max(0).values + b1.abs()
    assert int(bound.max()) < EXACT
    W2 = b2 = None
    n_last = N1
    if N2:
        W2 = sparse(N2, N1, 8, 6, seed + 6)
        b2 = _randint((N2,), -2, 2, seed + 7)
        W2[:8], b2[:8] = 0, 0
        W2[torch.arange(7), torch.arange(7)] = 1
        W2[7, 6] = 1
        bound = W2.abs() @ bound + b2.abs()
        assert int(bound.max()) < EXACT
        n_last = N2
    wl = sparse(1, n_last, 8, 12, seed + 8)
    wl[0, :8] = torch.tensor([1, 1, 1, 1, 1, 1, 1, -1])
    bl = torch.tensor([3], dtype=torch.int64)
    assert int(wl.abs() @ bound + bl.abs()) < EXACT
    items = items.double()
    items[NAN_ITEM(cols), 3] = float("inf")
    return dict(users=users, items=items, Wu=Wu, Wi=Wi, b1=b1, W2=W2, b2=b2, wl=wl, bl=bl, adversarial=adv)


def relu(x):
    """The kernels' ReLU, fmaxf(x, 0): a NaN becomes 0."""
    return torch.fmax(x, torch.zeros((), dtype=x.dtype, device=x.device))


def mlp_weights(m, user_first, dev):
    """([W1, (W2,) wl], [b1, (b2,) bl]) fp32 on the device, layer 1 over cat(user, item) (user_first) or cat(item, user)."""
    W1 = torch.cat([m["Wu"], m["Wi"]] if user_first else [m["Wi"], m["Wu"]], 1)
    W = [W1] + ([m["W2"]] if m["W2"] is not None else []) + [m["wl"]]
    b = [m["b1"]] + ([m["b2"]] if m["b2"] is not None else []) + [m["bl"]]
    return [w.float().to(dev) for w in W], [x.float().to(dev) for x in b]


def mlp_scores(m, dev, block_bytes=1 << 30):
    """The (rows, cols) fp32 scores of int_mlp's data from float64 torch on `dev` (user blocks bound the activations' memory)."""
    d = lambda x: x.double().to(dev)
    U, I = d(m["users"]) @ d(m["Wu"]).t(), d(m["items"]) @ d(m["Wi"]).t() + d(m["b1"])
    per = max(1, block_bytes // (I.shape[0] * I.shape[1] * 8))
    out = []
    for r0 in range(0, U.shape[0], per):
        h = relu(U[r0:r0 + per, None, :] + I[None])
        if m["W2"] is not None:
            h = relu(h @ d(m["W2"]).t() + d(m["b2"]))
        out.append(((h @ d(m["wl"]).t()).squeeze(-1) + d(m["bl"]) + 0.0).float())
    return torch.cat(out)


def exclusion(rows, cols, tile, dev, best=None):
    """A CSR exclusion list with, for every row r: the columns c with (c + r) % 61 == 0 (every 2048-column bitmap chunk of every
    tile, words of the bitmap past the first 64 as soon as a tile is wider than 2048); the columns an adversarial row would
    select: the first and last three, the three around the range boundary, the first of the top plateau and the top of the
    sawtooth's first period; and the row's own columns `best` (rows, m), its best ones without a list: whatever the data, every
    row loses columns it would otherwise select."""
    c = torch.arange(cols, device=dev)
    mask = ((c[None, :] + torch.arange(rows, device=dev)[:, None]) % 61) == 0
    fixed = [0, 1, 2, 31, cols - 3, cols - 2, cols - 1] + [x for x in (tile - 100, tile - 1, tile, tile + 1) if 0 <= x < cols]
    mask[:, torch.tensor(fixed, device=dev)] = True
    if best is not None:
        mask.scatter_(1, best.to(torch.int64).clamp_min(0), True)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), mask.sum(1).cumsum(0)])
    return rowptr, mask.nonzero()[:, 1].to(torch.int32)


def targets(rows, cols, max_targets, dev):
    """A target CSR: row r has max_targets targets (r * 131 + j * 977 + 5) % cols, except: r % 11 == 3 has none; r % 5 == 0 starts
    with cols - 1 (in exclusion()'s list); r % 7 == 0 ends with an id outside the list (-1 or cols); r % 13 == 0 repeats its first."""
    r = torch.arange(rows, device=dev)[:, None]
    j = torch.arange(max_targets, device=dev)[None, :]
    t = (r * 131 + j * 977 + 5) % cols
    t[::5, 0] = cols - 1
    t[::7, -1] = torch.where(r[::7, 0] % 2 == 0, -1, cols)
    if max_targets > 1:
        t[::13, 1] = t[::13, 0]
    lens = torch.where(r[:, 0] % 11 == 3, 0, max_targets)
    keep = j < lens[:, None]
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)])
    return rowptr, t[keep].to(torch.int32)


CHUNKED_DROP = 5


def chunked_case(rows, cols, k, dev):
    """The row-chunked ncf_dot_topk case: rank-one scores s_r g(col), user r = s_r e_0 with s_r = DIRS[(r + r / 64) % 4] — not
    periodic in the chunk length, so rows 0, 64 and 128 differ and a chunk that read another chunk's users would show — and item
    coordinate 0 = g(col) in 0 .. 4092 (every value about 4100 times).  The reference is analytic: one stable sort of g in each
    direction (s > 0: largest g first, s < 0: smallest first, ties to the lower column).  Odd rows (some in every chunk) list their
    own CHUNKED_DROP best columns for exclusion; their answer is the next k of the same order.
    Returns (users, items, seen CSR, reference without the list, reference with it)."""
    col = torch.arange(cols, device=dev, dtype=torch.int64)
    g = ((col * 2654435761) >> 7) % 4093
    r = torch.arange(rows, device=dev)
    s = torch.tensor(_DIRS, device=dev)[(r + r // 64) % 4]
    items = torch.zeros((cols, 4), device=dev)
    items[:, 0] = g.float()
    users = torch.zeros((rows, 4), device=dev)
    users[:, 0] = s.float()
    n = k + CHUNKED_DROP
    down = torch.sort(g, descending=True, stable=True).indices[:n]
    up = torch.sort(g, stable=True).indices[:n]
    order = torch.where((s > 0)[:, None], down[None, :], up[None, :])
    listed = r % 2 == 1
    lens = torch.where(listed, CHUNKED_DROP, 0)
    seen = (torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)]),
            order[listed, :CHUNKED_DROP].reshape(-1).to(torch.int32))

    def ref(idx):
        return (s[:, None] * g[idx]).float() + 0.0, idx.to(torch.int32), torch.full((rows,), k, dtype=torch.int32, device=dev)

    return users, items, seen, ref(order[:, :k]), ref(torch.where(listed[:, None], order[:, CHUNKED_DROP:], order[:, :k]))
