"""Case table and references for the generic fp32 Linear (csrc/linear.hip) on every launch form.  No GPU needed: the functions
take tensors on any device and compute in float64 / int64 there.

THE CASE TABLE.  One host rule (plan_linear in linear.hip, asked through ``native.linear_plan``) chooses among the LDS-tiled
kernel, the row-dot kernel, ``linear_rs_kernel<NT, KS>`` (one 32-row tile per group of KS waves, optionally one 32-column block
per workgroup) and the persistent ``linear_rsp_kernel<NT>``.  Every row of CASES names a shape, the options it is run under and
the plan the rule must give for it, so that a later change of the rule cannot silently move a case to another kernel.  Each row
sits at the smallest M that reaches its form; neighbouring rows differ in one edge (Q = K / 8 below):

* rs<8,1> (PD = 8 fragments of A in the register ring): Q = 1, 8 = PD, 9, 17, and 17 plus a 7-element tail.
* rs<1,4> at K = 520: slices of 16 = PD and 17 = PD + 1 steps of the NT = 1 ring (PD = 16); (100,32,72): slices of 2, 2, 2, 3.
* rs<1,8> (whole 32-wide blocks of K staged through LDS, split over 8 waves; the rest of K is wave 0's, on the direct path):
  K = 1024 no rest; 1032 one whole 8-group; 1055 three groups and a 7-element tail; 2094 65 blocks over 8 waves unevenly, one
  group and a 6-element tail; 512 / 543 forced: 16 blocks, two per wave.
* rsp: grid capped at 512 workgroups = 2048 waves, so a wave walks ceil((tiles - wave) / 2048) tiles: 1 everywhere; 2 on some
  waves and 1 on others (2049 tiles); 3 and 2 (4097, 4098 tiles); forced on 2 and 4 tiles (waves that own none return early).
* rowdot past its 16 384-block cap (M * N > 262 144); tiled with K < 8 at N = 32 / 256, with 3 and 33 column blocks.

THE REFERENCES.
* Exact.  x, w and bias are integers in [-7, 7] stored as fp32.  Every partial sum is an integer of magnitude <= 49 K + 7
  <= 102 613 < 2^24 at the largest K here (2094), so every order of summation and every split over waves gives the same fp32
  value: the integer product, then ReLU, is the expected output bit for bit.  The product is formed in float64 (exact far
  beyond these magnitudes, and available as a GEMM on every device) and returned as int64; the CPU tests hold that route to a
  plain int64 matmul.
* Bound.  Random N(0,1) operands against float64: |out - ref| <= (K + 16) 2^-24 (sum_k |x_k w_k| + |b|) per element.  On any
  path from a product to the output there are at most K accumulations, KS - 1 <= 7 slice adds (or the row-dot's four shuffle
  adds) and one bias add: n <= K + 8 roundings to nearest (u = 2^-24 each, or none where a product is fused), and the
  standard summation bound gamma_n = n u / (1 - n u) <= (K + 16) u holds for every order of summation at these K.  ReLU is
  1-Lipschitz, so the bound holds after it.  The bound assumes round-to-nearest inside the MFMA accumulate.
"""
from collections import namedtuple

import torch

U24 = 2.0 ** -24
INT_RANGE = 7
K_MAX = 2094

# plan: (form, nt, kslices, col_blocks, grid_x) as native.linear_plan returns it
Case = namedtuple("Case", "M N K force ks plan")


def _c(M, N, K, plan, force=None, ks=None):
    return Case(M, N, K, force, ks, plan)


CASES = [
    # ---- rs<1,1>: K < 32, or more than 2048 tiles
    _c(33, 32, 8, ("rs", 1, 1, 1, 1)),
    _c(33, 32, 31, ("rs", 1, 1, 1, 1)),
    _c(65541, 32, 40, ("rs", 1, 1, 1, 513)),
    # ---- rs<8,1>: N = 256 never splits K
    _c(40, 256, 8, ("rs", 8, 1, 1, 1)),
    _c(40, 256, 64, ("rs", 8, 1, 1, 1)),
    _c(40, 256, 72, ("rs", 8, 1, 1, 1)),
    _c(40, 256, 136, ("rs", 8, 1, 1, 1)),
    _c(40, 256, 143, ("rs", 8, 1, 1, 1)),
    # ---- rs<2,1>, rs<4,1>: above 2048 tiles; NT >= 2 with 8 <= K < 32
    _c(65541, 64, 72, ("rs", 2, 1, 1, 513)),
    _c(65541, 128, 24, ("rs", 4, 1, 1, 513)),
    _c(33, 64, 24, ("rs", 2, 1, 1, 1)),
    # ---- rs<NT,2>: 32 <= K < 64, or 1025 .. 2048 tiles
    _c(33, 32, 40, ("rs", 1, 2, 1, 1)),
    _c(70, 64, 63, ("rs", 2, 2, 1, 2)),
    _c(32800, 128, 72, ("rs", 4, 2, 1, 513)),
    _c(32800, 32, 64, ("rs", 1, 2, 1, 513), force="rs"),
    # ---- rs<NT,4>, one workgroup per tile
    _c(33, 32, 64, ("rs", 1, 4, 1, 2)),
    _c(100, 32, 72, ("rs", 1, 4, 1, 4)),
    _c(100, 32, 128, ("rs", 1, 4, 1, 4)),
    _c(100, 32, 136, ("rs", 1, 4, 1, 4)),
    _c(33, 32, 520, ("rs", 1, 4, 1, 2)),
    _c(100, 64, 135, ("rs", 2, 4, 1, 4)),
    _c(32768, 128, 200, ("rs", 4, 4, 1, 1024)),
    _c(4090, 32, 2094, ("rs", 1, 4, 1, 128)),
    # ---- rs<1,4> with column blocks
    _c(40, 64, 520, ("rs", 1, 4, 2, 2)),
    _c(4096, 128, 512, ("rs", 1, 4, 4, 128)),
    _c(33, 128, 1023, ("rs", 1, 4, 4, 2)),
    _c(500, 64, 2048, ("rs", 1, 4, 2, 16), ks="4"),
    # ---- rs<1,8> with column blocks (staged form)
    _c(33, 64, 1024, ("rs", 1, 8, 2, 2)),
    _c(40, 128, 1032, ("rs", 1, 8, 4, 2)),
    _c(70, 128, 1055, ("rs", 1, 8, 4, 3)),
    _c(33, 64, 2094, ("rs", 1, 8, 2, 2)),
    _c(4096, 128, 1056, ("rs", 1, 8, 4, 128)),
    _c(40, 64, 512, ("rs", 1, 8, 2, 2), ks="8"),
    _c(40, 64, 543, ("rs", 1, 8, 2, 2), ks="8"),
    # ---- rsp, one tile per wave
    _c(4096, 32, 64, ("rsp", 1, 1, 1, 32)),
    _c(4100, 64, 128, ("rsp", 2, 1, 1, 33)),
    _c(16390, 128, 192, ("rsp", 4, 1, 1, 129)),
    _c(33, 256, 64, ("rsp", 8, 1, 1, 1), force="rsp"),
    _c(100, 32, 128, ("rsp", 1, 1, 1, 1), force="rsp"),
    # ---- rsp, 2 tiles on some waves, 1 on others
    _c(65541, 32, 64, ("rsp", 1, 1, 1, 512)),
    _c(65541, 256, 64, ("rsp", 8, 1, 1, 512)),
    # ---- rsp, 3 tiles on some waves, 2 on others
    _c(131080, 32, 64, ("rsp", 1, 1, 1, 512)),
    _c(131105, 64, 128, ("rsp", 2, 1, 1, 512)),
    # ---- rowdot
    _c(7, 5, 3, ("rowdot", 0, 1, 1, 3)),
    _c(3, 3, 16, ("rowdot", 0, 1, 1, 1)),
    _c(5, 8, 17, ("rowdot", 0, 1, 1, 3)),
    _c(1, 1, 1, ("rowdot", 0, 1, 1, 1)),
    _c(32801, 8, 3, ("rowdot", 0, 1, 1, 16384)),
    # ---- tiled
    _c(129, 65, 33, ("tiled", 0, 1, 2, 2)),
    _c(130, 32, 7, ("tiled", 0, 1, 1, 2)),
    _c(5, 256, 1, ("tiled", 0, 1, 4, 1)),
    _c(257, 130, 40, ("tiled", 0, 1, 3, 3)),
    _c(128, 9, 32, ("tiled", 0, 1, 1, 1)),
    _c(40, 2094, 64, ("tiled", 0, 1, 33, 1)),
]


def case_id(c):
    return f"{c.M}x{c.N}x{c.K}" + (f"-{c.force}" if c.force else "") + (f"-ks{c.ks}" if c.ks else "")


def form_name(plan):
    """'rs<1,8>x4', 'rsp<2>', 'tiled', 'rowdot': the kernel instantiation a plan launches."""
    form, nt, ks, cb, _ = plan
    if form == "rs":
        return f"rs<{nt},{ks}>" + (f"x{cb}" if cb > 1 else "")
    return f"rsp<{nt}>" if form == "rsp" else form


def rsp_tiles_per_wave(c):
    """Most row tiles one wave of the persistent form walks: ceil(tiles / (4 * grid_x))."""
    tiles = (c.M + 31) // 32
    return -(-tiles // (4 * c.plan[4]))


def set_case_options(set_option, c):
    """``set_option(name, value)``: native.set_option or the kernel_option fixture."""
    set_option("linear_kernel", c.force or "auto")
    set_option("linear_kslices", c.ks or "auto")


# ----------------------------------------------------------------------------------------------------------- operands
def int_operands(M, N, K, gen):
    """x (M, K), w (N, K), b (N,): integers in [-7, 7] as fp32, on the generator's device."""
    def draw(*shape):
        return torch.randint(-INT_RANGE, INT_RANGE + 1, shape, generator=gen, device=gen.device).float()
    return draw(M, K), draw(N, K), draw(N)


def random_operands(M, N, K, gen):
    def draw(*shape):
        return torch.randn(shape, generator=gen, device=gen.device)
    return draw(M, K), draw(N, K), draw(N)


# --------------------------------------------------------------------------------------------------------- references
def exact_reference(x, w, b, relu):
    """int64 (M, N): x . w^T + b, then ReLU, for integer-valued operands (module docstring)."""
    K = x.shape[1]
    assert INT_RANGE * INT_RANGE * K + INT_RANGE < 2 ** 24
    ref = x.double() @ w.double().t()
    if b is not None:
        ref = ref + b.double()
    ref = ref.round().long()
    return ref.clamp_min(0) if relu else ref


def exact_check(out, x, w, b, relu):
    """The kernel's fp32 output holds the integer reference, element for element."""
    ref = exact_reference(x, w, b, relu)
    return out.shape == ref.shape and out.dtype == torch.float32 and torch.equal(out.double(), ref.double())


def reference64(x, w, b, relu):
    ref = x.double() @ w.double().t()
    if b is not None:
        ref = ref + b.double()
    return torch.relu(ref) if relu else ref


def error_bound(x, w, b):
    """(M, N) float64: (K + 16) 2^-24 (sum_k |x_k w_k| + |b|)."""
    K = x.shape[1]
    mag = x.double().abs() @ w.double().abs().t()
    if b is not None:
        mag = mag + b.double().abs()
    return (K + 16) * U24 * mag


def bound_check(out, x, w, b, relu):
    """(ok, worst fraction of the bound used, error there, bound there, max error / max |ref|)."""
    ref = reference64(x, w, b, relu)
    bound = error_bound(x, w, b)
    err = (out.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    used = err / bound.clamp_min(1e-300)
    k = int(used.argmax())
    return (bool((err <= bound).all()), float(used.flatten()[k]), float(err.flatten()[k]), float(bound.flatten()[k]),
            float(err.max()) / max(float(ref.abs().max()), 1e-300))
