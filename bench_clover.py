#!/usr/bin/env python3
"""Clover-term construction: the torch path (clover_matrix + from_matrices)
against the native kernel of csrc/clover_term.hip, in one process on one GPU,
double-precision field, random SU(3) links.

Per lattice it times
  torch    CloverField.from_gauge(native=False)
  native   CloverField.from_gauge(native=True): the kernel, the partial sums
           and their read-back
  kernel   k_clover_term alone (both stages)
  stage1   k_clover_term stopped after stage 1 (F_munu to LDS only)
  copy     a device copy moving the bytes the kernel must move: 576 B/site
           of links read, 2 x 576 B/site of packed output written
and, with --force-lattice, one clover_fermion_force(native=True) evaluation
with and without the native clover term (QUDA_AMD_NATIVE_CLOVER). Variants
alternate over --rounds rounds, host clock with a device synchronise on both
sides of every timed window, every variant warmed up once per round before
it is timed; the median of the rounds' means is quoted. Prints one JSON line
per lattice.

Usage: python bench_clover.py [--lattices 16x16x16x32,32x32x32x64]
                              [--force-lattice 16x16x16x32] [--rounds 3]
                              [--min-time 0.3] [--torch-reps 2]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch


def timed(fn, min_time: float, min_reps: int = 3, max_reps: int = 500):
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


def rounds_of(variants, rounds, min_time, torch_reps):
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            if k.startswith("torch"):
                t, _ = timed(fn, 0.0, torch_reps, torch_reps)
            else:
                t, _ = timed(fn, min_time)
            times[k].append(t)
    return times, {k: statistics.median(v) for k, v in times.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="16x16x16x32,32x32x32x64")
    ap.add_argument("--force-lattice", default="16x16x16x32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-time", type=float, default=0.3)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--kappa", type=float, default=0.115)
    ap.add_argument("--csw", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_clover: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import GaugeField, LatticeGeometry
    from quda_amd.fields.clover import CloverField
    from quda_amd.gauge import fermion_force as ff
    from quda_amd.models import DiracClover
    from quda_amd.ops.dispatch import empty_tensor, hip_ext

    ext = hip_ext()
    kappa, csw = args.kappa, args.csw

    def setup(lat):
        dims = tuple(int(x) for x in lat.split("x"))
        geo = LatticeGeometry(dims)
        u = GaugeField(geo, "double").random_su3_(seed=7).to_complex()
        return dims, geo, u.cuda().contiguous()

    for lat in args.lattices.split(","):
        dims, geo, u = setup(lat)
        larg = (list(geo.dims), geo.parity_offset, geo.volume_cb)
        f = CloverField(geo, "double", "cuda")
        none = empty_tensor(u.dtype, u.device)
        none_r = empty_tensor(torch.float64, u.device)
        fbuf = torch.empty((6, 2, geo.volume_cb, 3, 3), dtype=u.dtype,
                           device="cuda")
        moved = geo.volume * 3 * 576
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        variants = {
            "torch": lambda: f.from_gauge(u, kappa, csw, native=False),
            "native": lambda: f.from_gauge(u, kappa, csw, native=True),
            "kernel": lambda: ext.clover_term(f.data, f.inv_data, none, u,
                                              *larg, kappa * csw),
            # stage 1 alone needs the F buffer as its only output
            "stage1": lambda: ext.clover_term(none_r, none_r, fbuf, u, *larg,
                                              kappa * csw),
            "kernel_f": lambda: ext.clover_term(f.data, f.inv_data, fbuf, u,
                                                *larg, kappa * csw),
            "copy": lambda: dst.copy_(src),
        }
        times, med = rounds_of(variants, args.rounds, args.min_time,
                               args.torch_reps)
        t = CloverField(geo, "double", "cuda").from_gauge(u, kappa, csw,
                                                          native=False)
        f.from_gauge(u, kappa, csw, native=True)
        print(json.dumps({
            "lattice": list(dims), "kappa": kappa, "csw": csw,
            "seconds": {k: [round(x, 7) for x in v]
                        for k, v in times.items()},
            "ms_torch": med["torch"] * 1e3,
            "ms_native": med["native"] * 1e3,
            "ms_kernel": med["kernel"] * 1e3,
            "speedup_native_vs_torch": med["torch"] / med["native"],
            "bytes_moved": moved,
            "kernel_copy_fraction": med["copy"] / med["kernel"],
            # both with the F buffer written, so the difference is stage 2
            "stage2_share": 1.0 - med["stage1"] / med["kernel_f"],
            "max_abs_native_minus_torch": max(
                (f.data - t.data).abs().max().item(),
                (f.inv_data - t.inv_data).abs().max().item()),
            "trlog_native": f.trlog, "trlog_torch": t.trlog,
        }), flush=True)
        del f, t, src, dst, fbuf
        torch.cuda.empty_cache()

    if args.force_lattice:
        dims, geo, u = setup(args.force_lattice)
        g = GaugeField(geo, "double", "cuda").from_complex(u)
        cl = CloverField(geo, "double", "cuda").from_gauge(u, kappa, csw,
                                                           native=True)
        phi = ff.pseudofermion_refresh(DiracClover(g, cl, kappa), seed=3)

        def force(flag):
            os.environ["QUDA_AMD_NATIVE_CLOVER"] = flag
            return ff.clover_fermion_force(u, geo, kappa, csw, phi,
                                           native=True)

        variants = {"force_torch_term": lambda: force("0"),
                    "force_native_term": lambda: force("1")}
        times, med = rounds_of(variants, args.rounds, args.min_time, 0)
        print(json.dumps({
            "lattice": list(dims), "kappa": kappa, "csw": csw,
            "seconds": {k: [round(x, 7) for x in v]
                        for k, v in times.items()},
            "ms_force_torch_term": med["force_torch_term"] * 1e3,
            "ms_force_native_term": med["force_native_term"] * 1e3,
        }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
