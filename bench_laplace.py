#!/usr/bin/env python3
"""Laplace family: the torch path (flag off) against the native hop-sum
kernel (csrc/laplace.h), in one process on one GPU.

Per lattice and precision it times
  step      one Wuppertal step, nspin 4 (laplace_apply, 3-d, 6 hops)
  smear     an n-step Wuppertal smear, nspin 4
  lapM      one GaugeLaplace.M, nspin 1
with the flag off and on, every columns-per-thread variant of the step, the
variant that reads the backward link from the neighbour's forward slot, and
the 1-parity staggered dslash of the same precision and lattice, alternating
over --rounds rounds. Host clock with a device synchronise on both sides of
every timed window; every variant is warmed up once per round before it is
timed. Prints one JSON line per (lattice, precision) with the times, the
ratios and the shape-derived compulsory bytes: in and out once plus the
enabled link slots once.

Usage: python bench_laplace.py [--lattices 16x16x16x32,32x32x32x64]
                               [--precisions double,single,half]
                               [--rounds 2] [--min-time 0.2] [--steps 50]
"""

from __future__ import annotations

import argparse
import json
import sys
import time

import torch

ITEM = {"double": 8, "single": 4, "half": 2}
CPTS = {"double": (1, 2, 4), "single": (2, 4), "half": (4,)}


def compulsory_bytes(volume: int, prec: str, nspin: int, nhops: int) -> int:
    site = 6 * nspin * ITEM[prec] + (4 if prec == "half" else 0)
    return volume * (2 * site + nhops * 18 * ITEM[prec])


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
    ap.add_argument("--lattices", default="16x16x16x32,32x32x32x64")
    ap.add_argument("--precisions", default="double,single,half")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-time", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_laplace: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import GaugeField, LatticeGeometry, SpinorField
    from quda_amd.models.laplace import (GaugeLaplace, laplace_apply,
                                         wuppertal_smear)
    from quda_amd.ops import dispatch

    alpha = 3.0
    a = alpha / (1.0 + 6.0 * alpha)
    for lat in args.lattices.split(","):
        dims = tuple(int(x) for x in lat.split("x"))
        geo = LatticeGeometry(dims)
        u = GaugeField(geo, "double").random_su3_(seed=7).to_complex().cuda()
        for prec in args.precisions.split(","):
            g = GaugeField(geo, prec, "cuda").from_complex(u)
            psi = SpinorField(geo, prec, "cuda").gaussian_(seed=8)
            out = psi.clone_empty()
            v1 = SpinorField(geo, prec, "cuda", nspin=1).gaussian_(seed=9)
            o1 = v1.clone_empty()
            sp = SpinorField(geo, prec, "cuda", 1, nspin=1).gaussian_(seed=10)
            so = sp.clone_empty()
            ops = {flag: GaugeLaplace(g, m2=0.5, native=flag)
                   for flag in (False, True)}

            def step(flag):
                return lambda: laplace_apply(g, psi, out, ndim=3, a=a, b=1.0,
                                             native=flag)

            def hops(cpt, nbr):
                return lambda: dispatch.laplace_hops(
                    out, psi, g, 0x77, a, 1.0 - 6.0 * a, cpt=cpt,
                    nbr_link=nbr)

            variants = {
                "step_torch": (step(False), 3),
                "step_native": (step(True), 3),
                "smear_torch": (lambda: wuppertal_smear(
                    g, psi, alpha=alpha, n_steps=args.steps, native=False), 1),
                "smear_native": (lambda: wuppertal_smear(
                    g, psi, alpha=alpha, n_steps=args.steps, native=True), 3),
                "lapM_torch": (lambda: ops[False].M(o1, v1), 3),
                "lapM_native": (lambda: ops[True].M(o1, v1), 3),
                "step_nbr_link": (hops(0, True), 3),
                "staggered_dslash": (lambda: dispatch.dslash_staggered(
                    so, sp, g, 0), 3),
            }
            for cpt in CPTS[prec]:
                variants[f"step_cpt{cpt}"] = (hops(cpt, False), 3)
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, (fn, min_reps) in variants.items():
                    t, _n = timed(fn, args.min_time, min_reps)
                    times[k].append(t)
            best = {k: min(v) for k, v in times.items()}
            b4 = compulsory_bytes(geo.volume, prec, 4, 6)
            b1 = compulsory_bytes(geo.volume, prec, 1, 6)
            bs = compulsory_bytes(geo.volume // 2, prec, 1, 8)
            print(json.dumps({
                "lattice": list(dims), "precision": prec,
                "smear_steps": args.steps,
                "seconds": {k: [round(t, 7) for t in v]
                            for k, v in times.items()},
                "speedup_step": best["step_torch"] / best["step_native"],
                "speedup_smear": best["smear_torch"] / best["smear_native"],
                "speedup_lapM": best["lapM_torch"] / best["lapM_native"],
                "step_compulsory_bytes": b4,
                "step_compulsory_tbs": b4 / best["step_native"] / 1e12,
                "lapM_compulsory_bytes": b1,
                "lapM_compulsory_tbs": b1 / best["lapM_native"] / 1e12,
                "staggered_compulsory_bytes": bs,
                "staggered_compulsory_tbs":
                    bs / best["staggered_dslash"] / 1e12,
            }), flush=True)
            del g, psi, out, v1, o1, sp, so
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
