#!/usr/bin/env python3
"""Gauge MD force: the torch paths against the native path-table kernel
(csrc/gauge_path.hip), in one process on one GPU.

Per lattice and action (wilson, symanzik) it times
  parent     gauge_force / the autograd improved_gauge_force, flag off
  reference  paths.path_force_reference on the GPU (analytic torch)
  native     path_gauge_force(native=True)
  fused      path_gauge_force(mom=, dt=, native=True), in-place update
alternating over --rounds rounds, host clock with a device synchronise on
both sides of every timed window, and one leapfrog step with the flag off
and on. Every variant is warmed up once per round before it is timed. Prints
one JSON line per (lattice, action) with the times, the agreement of the
variants and the shape-derived flop and byte counts of the kernel.

Usage: python bench_gauge_force.py [--lattices 16x16x16x32,24x24x24x48]
                                   [--rounds 2] [--min-time 0.3]
"""

from __future__ import annotations

import argparse
import json
import sys
import time

import torch

FP64_PEAK = 78.6e12   # vector fp64 flop/s (spec; as profiles r05/r06)
COPY_PEAK = 6.29e12   # bytes/s, the copy peak measured in profiles r05


def kernel_counts(table, volume: int, fused: bool):
    """Shape-derived flop and bytes of the four launches of one force.
    A 3x3 complex product is 9 x (3 cmul + 2 cadd) = 198 flop, the c_p
    accumulate 36, TA and the scalings about 60. bytes_requested counts
    every link load the lanes issue (144 B each); bytes_compulsory is the
    field read once per launch plus U_mu, the result and, fused, the
    momentum read."""
    flop = 0
    loads = 0
    for tl in table.tails:
        for _, t in tl:
            flop += 198 * max(len(t) - 1, 0) + 36
            loads += len(t)
        flop += 198 + 60 + (36 if fused else 0)
        loads += 1 + (1 if fused else 0)
    req = (loads + 4) * 144  # + one store per direction
    comp = 4 * (4 * 144 + 144 + (144 if fused else 0))
    return flop * volume, req * volume, comp * volume


def timed(fn, min_time: float, max_reps: int = 200):
    fn()  # warm-up of this shape
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while reps < 3 or (total < min_time and reps < max_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
        reps += 1
    return total / reps, reps


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="16x16x16x32,24x24x24x48")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-time", type=float, default=0.3)
    ap.add_argument("--beta", type=float, default=6.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_gauge_force: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import GaugeField, LatticeGeometry
    from quda_amd.gauge import hmc, ops, paths
    from quda_amd.gauge.paths import LoopAction

    beta = args.beta
    for lat in args.lattices.split(","):
        dims = tuple(int(x) for x in lat.split("x"))
        geo = LatticeGeometry(dims)
        u = GaugeField(geo, "double").random_su3_(seed=7).to_complex()
        u = u.cuda().contiguous()
        P0 = hmc.random_momentum(geo, "cuda", seed=8).contiguous()
        for name in ("wilson", "symanzik"):
            act = getattr(LoopAction, name)()
            table = paths.force_table(act)
            mom = P0.clone()
            if name == "wilson":
                def parent():
                    return ops.gauge_force(u, geo, beta, native=False)
            else:
                def parent():
                    return ops.improved_gauge_force(u, geo, beta,
                                                    native=False)
            variants = {
                "parent": parent,
                "reference": lambda: paths.path_force_reference(
                    u, geo, act, beta),
                "native": lambda: ops.path_gauge_force(
                    u, geo, act, beta, native=True),
                "fused": lambda: ops.path_gauge_force(
                    u, geo, act, beta, mom=mom, dt=1e-3, native=True),
                "leapfrog_off": lambda: hmc.leapfrog(
                    u, P0, geo, beta, 1, 0.01, action=act, native=False),
                "leapfrog_on": lambda: hmc.leapfrog(
                    u, P0, geo, beta, 1, 0.01, action=act, native=True),
            }
            times = {k: [] for k in variants}
            reps = {}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    t, n = timed(fn, args.min_time)
                    times[k].append(t)
                    reps[k] = n
            Fp, Fr, Fn = parent(), variants["reference"](), \
                variants["native"]()
            best = {k: min(v) for k, v in times.items()}
            flop, req, comp = kernel_counts(table, geo.volume, False)
            tn = best["native"]
            out = {
                "lattice": list(dims), "action": name, "beta": beta,
                "tails_per_dir": table.n_paths,
                "seconds": {k: [round(t, 7) for t in v]
                            for k, v in times.items()},
                "reps": reps,
                "speedup_native_vs_parent": best["parent"] / tn,
                "speedup_native_vs_reference": best["reference"] / tn,
                "speedup_fused_vs_parent": best["parent"]
                / best["fused"],
                "speedup_leapfrog": best["leapfrog_off"]
                / best["leapfrog_on"],
                "max_abs_native_minus_parent": (Fn - Fp).abs().max().item(),
                "max_abs_native_minus_reference":
                    (Fn - Fr).abs().max().item(),
                "kernel_flop": flop,
                "kernel_bytes_requested": req,
                "kernel_bytes_compulsory": comp,
                "native_tflops": flop / tn / 1e12,
                "native_share_of_fp64_peak": flop / tn / FP64_PEAK,
                "native_requested_tbs": req / tn / 1e12,
                "native_compulsory_share_of_copy_peak":
                    comp / tn / COPY_PEAK,
            }
            print(json.dumps(out), flush=True)
            del Fp, Fr, Fn
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
