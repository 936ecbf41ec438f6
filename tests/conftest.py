import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


# ---- observed parity margins: every comparison records how much of its bar it used; one summary at session end ----
_MARGINS = {}


def record_error(tag, err, bar, scale_rel=None):
    """``err`` / ``bar`` of one comparison (same units).  Kept per test (worst comparison wins); printed at session end and
    written to gpurun_out/parity_margins.json so that the distance to the 1e-5 bar is on record, not just pass / fail."""
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    key = f"{test}|{tag}" if tag else test
    frac = float(err) / float(bar) if bar else float("inf") if err else 0.0
    old = _MARGINS.get(key)
    if old is None or frac > old["frac_of_bar"]:
        _MARGINS[key] = {"err": float(err), "bar": float(bar), "frac_of_bar": frac,
                         "max_err_over_max_ref": None if scale_rel is None else float(scale_rel)}


def pytest_terminal_summary(terminalreporter, exitstatus, config):
    if not _MARGINS:
        return
    rows = sorted(_MARGINS.items(), key=lambda kv: -kv[1]["frac_of_bar"])
    fr = np.array([v["frac_of_bar"] for _, v in rows])
    rel = np.array([v["max_err_over_max_ref"] for _, v in rows if v["max_err_over_max_ref"] is not None])
    tr = terminalreporter
    tr.write_sep("-", "parity margins (observed error / bar)")
    tr.write_line(f"{len(rows)} recorded comparisons: worst {fr.max():.3f} of its bar, median {np.median(fr):.3f}; "
                  + (f"max|a-b|/max|ref| worst {rel.max():.2e}, median {np.median(rel):.2e}" if len(rel) else ""))
    for k, v in rows[:8]:
        tr.write_line(f"  {v['frac_of_bar']:.3f} of bar (err {v['err']:.3e}, bar {v['bar']:.3e})  {k}")
    out = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_margins.json"), "w") as f:
            json.dump({"n": len(rows), "worst_frac_of_bar": float(fr.max()), "median_frac_of_bar": float(np.median(fr)),
                       "worst_max_err_over_max_ref": float(rel.max()) if len(rel) else None, "entries": dict(rows)}, f, indent=1)
    except OSError:
        pass


def hashed_weight(shape, salt, bound):
    """Deterministic float32 weights in [-bound, bound) from an integer hash of (element index, salt): the same bits on any
    machine and numpy version (no RNG stream involved), so a fixture can store the recipe instead of the values."""
    n = int(np.prod(shape))
    h = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(salt) * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    u = (h >> np.uint64(8)).astype(np.float64) / float(1 << 24)
    return ((2.0 * u - 1.0) * float(bound)).astype(np.float32).reshape(shape)


# CPU fingerprint of the goldens' summation order: fp32 linear layers (forward, and the two transposed products of backward)
# at the shapes the goldens exercise and ATen's vectorised reductions (sums, softmax, cosine similarity), one thread, on
# hashed inputs.  tests/golden/blas_probe.npz holds the SHA-256 of each result as computed where the goldens were made.
BLAS_PROBE_SHAPES = [(64, 60, 8), (64, 40, 8), (700, 600, 64), (700, 400, 128), (700, 128, 256), (700, 256, 128), (48, 24, 16),
                     (512, 64, 256), (512, 256, 1), (64, 20, 16), (16, 2094, 128), (96, 256, 128)]


def blas_probe_arrays(torch=torch):
    arrays = {}
    for n, (M, K, N) in enumerate(BLAS_PROBE_SHAPES):
        x = torch.from_numpy(hashed_weight((M, K), 7 * n + 1, 1.0))
        w = torch.from_numpy(hashed_weight((N, K), 7 * n + 2, K ** -0.5))
        b = torch.from_numpy(hashed_weight((N,), 7 * n + 3, 0.5))
        g = torch.from_numpy(hashed_weight((M, N), 7 * n + 4, 1.0))
        arrays[f"linear_{M}x{K}x{N}"] = torch.nn.functional.linear(x, w, b).numpy()
        arrays[f"gw_{M}x{K}x{N}"] = g.t().mm(x).numpy()
        arrays[f"gx_{M}x{K}x{N}"] = g.mm(w).numpy()
        arrays[f"sum_{M}x{K}"] = torch.cat([x.sum(0), x.sum(1)]).numpy()
        arrays[f"softmax_{M}x{K}"] = torch.softmax(x, dim=1).numpy()
        arrays[f"cos_{M}x{K}"] = torch.nn.functional.cosine_similarity(x[:, None, :min(K, 64)], x[None, :8, :min(K, 64)], dim=-1).numpy()
    return arrays


def golden_path_blas():
    """True when this machine (one thread) reproduces the fingerprint bit for bit: its fp32 GEMMs and reductions sum in the order
    of the machine the goldens were made on, so the CPU oracle can be held to the goldens bit-exactly."""
    import hashlib
    ref = np.load(os.path.join(GOLDEN, "blas_probe.npz"), allow_pickle=False)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        got = blas_probe_arrays()
    finally:
        torch.set_num_threads(n)
    return set(got) == set(ref.files) and all(
        hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() == str(ref[k]) for k, v in got.items())


def load_golden(name):
    """Returns (state_dict of torch tensors, dict of other arrays, kwargs dict or None).  A fixture may store some weights
    as a recipe (``hashed_weights``: JSON list of [state key, shape, salt, bound], see hashed_weight) instead of values."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    state, arrays = {}, {}
    for k in z.files:
        if k.startswith("w::"):
            state[k[3:]] = torch.from_numpy(z[k])
        elif k.startswith("g::"):      # reference parameter gradients (round 3 fixtures): arrays["grads"][state key]
            arrays.setdefault("grads", {})[k[3:]] = torch.from_numpy(z[k])
        else:
            arrays[k] = z[k]
    for key, shape, salt, bound in json.loads(str(arrays.pop("hashed_weights"))) if "hashed_weights" in arrays else []:
        state[key] = torch.from_numpy(hashed_weight(tuple(shape), salt, bound))
    kwargs = json.loads(str(arrays.pop("kwargs"))) if "kwargs" in arrays else None
    return state, arrays, kwargs


def onehot(pos, n):
    x = torch.zeros((len(pos), n), dtype=torch.float32)
    x[torch.arange(len(pos)), torch.as_tensor(np.asarray(pos), dtype=torch.long)] = 1.0
    return x


@pytest.fixture(scope="session")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def kernel_option(gpu):
    """set(name, value): ncf_set_option for the duration of one test (kernel-variant overrides; restored to "auto")."""
    from deeprecommendation_amd import native
    touched = []

    def set_(name, value):
        touched.append(name)
        native.set_option(name, "auto" if value is None else value)

    yield set_
    for name in touched:
        native.set_option(name, "auto")
