#!/usr/bin/env python3
"""Kahler-Dirac block inverse: the torch path (flag off) against the native
kernels (csrc/kd.hip), in one process on one GPU.

Per lattice and precision it times
  build     the constructor's work: torch X + batched LU, against k_kd_build
  apply     one KDBlockInverse.apply (X^-1)
  applyX    one KDBlockInverse.apply_X
  M         one DiracStaggeredKD.M
with the flag off and on, alternating over --rounds rounds. Host clock with a
device synchronise on both sides of every timed window; every variant is
warmed up once per round before it is timed. Prints one JSON line per
(lattice, precision) with the times, the ratios and the shape-derived
compulsory bytes of the native apply: the field in and out once plus the
P, Q, G table once.

Usage: python bench_kd.py [--lattices 16x16x16x32]
                          [--precisions double,single,half]
                          [--rounds 2] [--min-time 0.2] [--mass 0.05]
"""

from __future__ import annotations

import argparse
import json
import sys
import time

import torch

ITEM = {"double": 8, "single": 4, "half": 2}
TABLE_ITEM = {"double": 16, "single": 8, "half": 8}


def compulsory_bytes(volume: int, prec: str) -> int:
    site = 6 * ITEM[prec] + (4 if prec == "half" else 0)
    return volume * 2 * site + (volume // 16) * 1728 * TABLE_ITEM[prec]


def timed(fn, min_time: float, min_reps: int = 3, max_reps: int = 200):
    fn()  # warm-up of this shape
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while reps < min_reps or (total < min_time and reps < max_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
        reps += 1
    return total / reps, reps


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="16x16x16x32")
    ap.add_argument("--precisions", default="double,single,half")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-time", type=float, default=0.2)
    ap.add_argument("--mass", type=float, default=0.05)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_kd: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import GaugeField, LatticeGeometry, SpinorField
    from quda_amd.models.staggered_kd import DiracStaggeredKD, KDBlockInverse
    from quda_amd.ops import dispatch

    m = args.mass
    for lat in args.lattices.split(","):
        dims = tuple(int(x) for x in lat.split("x"))
        geo = LatticeGeometry(dims)
        u = GaugeField(geo, "double").random_su3_(seed=7).to_complex().cuda()
        for prec in args.precisions.split(","):
            g = GaugeField(geo, prec, "cuda").from_complex(u)
            psi = SpinorField(geo, prec, "cuda", nspin=1).gaussian_(seed=8)
            out = psi.clone_empty()
            kd = {flag: KDBlockInverse(u, geo, m, native=flag)
                  for flag in (False, True)}
            kd[True]._table(prec)
            ops = {flag: DiracStaggeredKD(g, m, native=flag)
                   for flag in (False, True)}
            # the operators share the complex128 build of the links
            for flag in (False, True):
                ops[flag].kd = kd[flag]

            variants = {
                "build_torch": (lambda: KDBlockInverse(u, geo, m,
                                                       native=False), 1),
                "build_native": (lambda: dispatch.kd_build(u, geo, m, prec),
                                 3),
            }
            for flag, name in ((False, "torch"), (True, "native")):
                variants[f"apply_{name}"] = (
                    lambda f=flag: kd[f].apply(out, psi), 3)
                variants[f"applyX_{name}"] = (
                    lambda f=flag: kd[f].apply_X(out, psi), 3)
                variants[f"M_{name}"] = (lambda f=flag: ops[f].M(out, psi), 3)
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, (fn, min_reps) in variants.items():
                    t, _n = timed(fn, args.min_time, min_reps)
                    times[k].append(t)
            best = {k: min(v) for k, v in times.items()}
            nbytes = compulsory_bytes(geo.volume, prec)
            print(json.dumps({
                "lattice": list(dims), "precision": prec, "mass": m,
                "seconds": {k: [round(t, 7) for t in v]
                            for k, v in times.items()},
                "speedup_build": best["build_torch"] / best["build_native"],
                "speedup_apply": best["apply_torch"] / best["apply_native"],
                "speedup_applyX": best["applyX_torch"] / best["applyX_native"],
                "speedup_M": best["M_torch"] / best["M_native"],
                "apply_compulsory_bytes": nbytes,
                "apply_compulsory_tbs": nbytes / best["apply_native"] / 1e12,
            }), flush=True)
            del g, psi, out, kd, ops
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
