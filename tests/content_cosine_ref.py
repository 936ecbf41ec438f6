"""The content-based baseline (content_cosine_top_k) restated in float64, the data its GPU test uses and the bar it is held to."""
import numpy as np

F, USERS, ITEMS, K, SEED, ZERO_USER = 67, 40, 200, 20, 0, 17
# a fp32 dot of two unit vectors errs by at most about F 2^-24 sum|a||b| <= F 2^-24; the other 8 cover the two normalisations
TOL = (F + 8) * 2.0 ** -24


def cosine_case(seed=SEED):
    """(profiles (40, F) fp32 with one zero row, features (200, F) fp32, float64 cosines, their stable descending order)."""
    rng = np.random.default_rng(seed)
    prof = rng.standard_normal((USERS, F)).astype(np.float32)
    prof[ZERO_USER] = 0.0                                # a user without ratings
    feat = rng.standard_normal((ITEMS, F)).astype(np.float32)
    p64, f64 = prof.astype(np.float64), feat.astype(np.float64)
    pn = p64 / np.maximum(np.linalg.norm(p64, axis=1, keepdims=True), 1e-12)
    fn = f64 / np.maximum(np.linalg.norm(f64, axis=1, keepdims=True), 1e-12)
    cos = pn @ fn.T
    return prof, feat, cos, np.argsort(-cos, axis=1, kind="stable")


def decided(cos, order, k=K):
    """(USERS, k) bool: the slots whose float64 score stands more than twice the tolerance away from both neighbours in the float64
    order (slot k - 1 against the first item left out too): there a correct fp32 ranking has no choice."""
    top = np.take_along_axis(cos, order[:, :k + 1], axis=1)
    gap = top[:, :-1] - top[:, 1:]                       # gap[s]: slot s to slot s + 1
    ok = gap > 2 * TOL
    ok[:, 1:] &= gap[:, :-1] > 2 * TOL
    return ok


def undecided_share(cos, order):
    """The share of (user, slot) comparisons left out for near-ties, over the users with a profile."""
    return 1.0 - float(np.delete(decided(cos, order), ZERO_USER, axis=0).mean())
