"""Dev tool (GPU box): interleaved in-process A/B of native.score_fused against native.score_fused_partial at the cfg-2 shape
(1 M users x 100 k items, E = 64, MLP 128-256-128-1), back to back, plus the build time of the partial table P.

    python tools/ab_partial.py [--batches 16384,32768,40000,65536,262144] [--reps 50] [--rounds 8] [--emb 64] [--hidden 256,128]
                               [--variants lds0=deeprecommendation_amd/libncf_hip_lds0.so,...]

Every batch size is checked bit for bit (partial == fused) before it is timed.  --variants adds one column per variant
library (tools/ab_build.sh, e.g. `ab_build.sh lds0 mlp_partial.hip -DNCF_PART_LDS=0` for the streaming kernel everywhere): its
ncf_score_fused_partial is timed interleaved with the loaded library's in this process, on the same P, and checked bit for
bit first.  NCF_HIP_LIBRARY replaces the loaded library itself.

--stamp name=lib,... takes libraries built with -DNCF_PART_STAMP=1 (`ab_build.sh stamp mlp_partial.hip -DNCF_PART_STAMP=1`) and
prints, for each, where a wave of the scoring kernel spends its cycles and the clock it holds (stamp_table below), then stops."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import native  # noqa: E402


STAMP_POINTS = ["entry", "first MFMA", "end of layer 1", "layer 2 steady (17th MFMA)", "end of layer 2", "exit"]


def stamp_table(name, lib, via, U, I, dev, g, pairs=65536, seconds=2.0):
    """A -DNCF_PART_STAMP=1 build: every wave reads the shader clock (s_memtime) and the 100 MHz reference (s_memrealtime) at six
    points and lane 0 stores the readings to a buffer of their own.  Random pairs, launches back to back for `seconds` first (the
    clock a kernel holds shows only under sustained load); the last launch's readings are kept.  Medians over waves, in shader
    cycles; clock = d(s_memtime) / d(s_memrealtime) x 100 MHz over the whole wave.  Segment shares only: the stamps cost cycles."""
    import ctypes
    import time
    lib.ncf_partial_stamp_buffer.restype = None
    lib.ncf_partial_stamp_buffer.argtypes = [ctypes.c_void_p]
    waves = (pairs + 31) // 32
    buf = torch.zeros((waves + 4) * 12, dtype=torch.int64, device=dev)
    batches = [(torch.randint(0, U, (pairs,), device=dev, generator=g), torch.randint(0, I, (pairs,), device=dev, generator=g))
               for _ in range(8)]
    out = torch.empty(pairs, 1, device=dev)
    lib.ncf_partial_stamp_buffer(buf.data_ptr())
    t0, k = time.time(), 0
    while time.time() - t0 < seconds:
        for _ in range(200):
            via(lib, batches[k % 8][0], batches[k % 8][1], out)
            k += 1
        torch.cuda.synchronize()
    for _ in range(200):
        via(lib, batches[k % 8][0], batches[k % 8][1], out)
        k += 1
    torch.cuda.synchronize()
    lib.ncf_partial_stamp_buffer(None)
    st = buf[:waves * 12].view(waves, 6, 2).cpu().double()
    cyc, ref = st[:, :, 0], st[:, :, 1]
    seg = (cyc[:, 1:] - cyc[:, :-1]).median(dim=0).values.tolist()
    life = (cyc[:, 5] - cyc[:, 0])
    clock = (life / (ref[:, 5] - ref[:, 0]).clamp(min=1) * 100.0).median().item()
    row = {"segments_cycles": dict(zip([f"{a} -> {b}" for a, b in zip(STAMP_POINTS[:-1], STAMP_POINTS[1:])], seg)),
           "lifetime_cycles": life.median().item(), "clock_mhz": clock, "launches": k}
    print(f"stamp build {name}: wave lifetime {row['lifetime_cycles']:.0f} cycles at {clock:.0f} MHz (median of {waves} waves, "
          f"{k} launches)", flush=True)
    for label, c in row["segments_cycles"].items():
        print(f"    {label:48s} {c:9.0f} cycles  {100 * c / row['lifetime_cycles']:5.1f} %", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stamp", default="", help="name=library,...: print the stamp table of each -DNCF_PART_STAMP=1 build and stop")
    ap.add_argument("--batches", default="16384,32768,40000,65536,262144")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--emb", type=int, default=64)
    ap.add_argument("--hidden", default="256,128")
    ap.add_argument("--variants", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    U, I, E, H = 1_000_000, 100_000, args.emb, tuple(int(h) for h in args.hidden.split(","))
    vlibs = {}
    for item in filter(None, args.variants.split(",")):
        name, path = item.split("=", 1)
        vlibs[name] = native.load_library(os.path.abspath(path))
    g = torch.Generator(device=dev).manual_seed(1234)
    tu = torch.randn(U, E, device=dev, generator=g) * 0.05
    ti = torch.randn(I, E, device=dev, generator=g) * 0.05
    dims = [2 * E, *H, 1]
    nl = len(dims) - 1
    ws = [(torch.rand(dims[i + 1], dims[i], device=dev, generator=g) * 2 - 1) / dims[i] ** 0.5 for i in range(nl)]
    bs = [(torch.rand(dims[i + 1], device=dev, generator=g) * 2 - 1) / dims[i] ** 0.5 for i in range(nl)]
    packed = native.PackedMLP(ws, bs)
    print(f"E = {E} + {E}, hidden {list(H)}: layer-1 weights in LDS = {native.partial_in_lds(E, E, packed)}", flush=True)

    def via(lib, ia, ib, out):   # native.score_fused_partial's call, through a variant library
        native._check(lib.ncf_score_fused_partial(native._dt(tu), native._ptr(P), P.stride(0), native._ptr(tu), U, tu.stride(0),
                                                  native._ptr(ti), I, ti.stride(0), native._ptr(ia), native._ptr(ib), ia.numel(), E, E,
                                                  packed.n_layers, native._dims_array(packed.dims), native._ptr(packed.blob),
                                                  native._ptr(out), native._ptr(native._oob_flag(dev)), native._stream(tu)))

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    P = native.layer1_partial(tu, packed)
    torch.cuda.synchronize()
    build = []
    for _ in range(5):
        e0.record()
        native.layer1_partial(tu, packed, out=P)
        e1.record()
        torch.cuda.synchronize()
        build.append(e0.elapsed_time(e1) * 1e3)
    result = {"P_bytes": P.numel() * 4, "P_build_us": sorted(build)[len(build) // 2], "batches": {}}
    print(f"P: {P.shape[0]} x {P.shape[1]} fp32 = {P.numel() * 4 / 2**30:.2f} GiB, build median {result['P_build_us']:.0f} us", flush=True)

    for item in filter(None, args.stamp.split(",")):
        name, path = item.split("=", 1)
        result.setdefault("stamps", {})[name] = stamp_table(name, native.load_library(os.path.abspath(path)), via, U, I, dev, g)
    if args.stamp:
        print(json.dumps(result))
        return

    for Bsz in [int(b) for b in args.batches.split(",")]:
        batches = [(torch.randint(0, U, (Bsz,), device=dev, generator=g), torch.randint(0, I, (Bsz,), device=dev, generator=g))
                   for _ in range(8)]
        out_f = torch.empty(Bsz, 1, device=dev)
        out_p = torch.empty(Bsz, 1, device=dev)
        variants = {
            "fused": lambda k: native.score_fused(tu, batches[k % 8][0], ti, batches[k % 8][1], packed, out=out_f),
            "partial": lambda k: native.score_fused_partial(P, tu, batches[k % 8][0], ti, batches[k % 8][1], packed, out=out_p),
        }
        out_v = torch.empty(Bsz, 1, device=dev)
        for name, lib in vlibs.items():
            variants[name] = lambda k, lib=lib: via(lib, batches[k % 8][0], batches[k % 8][1], out_v)
        for k in range(8):
            variants["fused"](k)
            for name in variants:
                if name == "fused":
                    continue
                out = out_p if name == "partial" else out_v.fill_(float("nan"))
                variants[name](k)
                if not torch.equal(out_f, out):
                    raise SystemExit(f"B={Bsz} batch {k}: {name} differs from fused (max |diff| {(out_f - out).abs().max().item():.3e})")
        times = {n: [] for n in variants}
        for _ in range(args.rounds):
            for n, fn in variants.items():
                for k in range(5):
                    fn(k)
                e0.record()
                for k in range(args.reps):
                    fn(k)
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e3 / args.reps)
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        spread = {n: (min(t), max(t)) for n, t in times.items()}
        result["batches"][Bsz] = {"fused_us": med["fused"], "partial_us": med["partial"], "speedup": med["fused"] / med["partial"],
                                  "fused_range": spread["fused"], "partial_range": spread["partial"],
                                  "variants": {n: {"us": med[n], "range": spread[n]} for n in vlibs}}
        print(f"B={Bsz:7d}: fused {med['fused']:8.2f} us [{spread['fused'][0]:.2f}, {spread['fused'][1]:.2f}]  "
              f"partial {med['partial']:8.2f} us [{spread['partial'][0]:.2f}, {spread['partial'][1]:.2f}]  "
              f"x{med['fused'] / med['partial']:.3f}  (bit-identical)"
              + "".join(f"\n           {n:>8s} {med[n]:8.2f} us [{spread[n][0]:.2f}, {spread[n][1]:.2f}]  partial is x{med[n] / med['partial']:.3f} of it"
                        + "  (bit-identical)" for n in vlibs), flush=True)
    native.check_oob(dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
