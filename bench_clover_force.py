#!/usr/bin/env python3
"""Wilson-clover pseudofermion force: the torch path (autograd through the
clover construction, or the einsum Wilson force for csw = 0) against the
native kernels of csrc/clover_force.hip, in one process on one GPU,
complex128, from Gaussian X, Y (the force is bilinear in them: no solve).

Per lattice, csw in {0, 1} and n pairs in {1, 4} it times
  torch    clover_force_from_solutions(native=False)
  native   clover_force_from_solutions(native=True): both kernels
  fused    the same with mom=, dt=: in-place momentum update
  axpy     native, then mom += dt * F in torch
  oprod    k_clover_sigma_oprod alone (csw != 0)
  deriv    k_clover_force alone on a given H
  copy     a device copy moving the bytes deriv must move (u, H, the
           momentum read and written; X and Y are not counted)
alternating over --rounds rounds, host clock with a device synchronise on
both sides of every timed window; every variant is warmed up once per round
before it is timed. Prints one JSON line per case with the times, the
agreement of the two paths and the copy fraction of the derivative kernel.

Usage: python bench_clover_force.py [--lattices 16x16x16x32,32x32x32x64]
                                    [--rounds 2] [--min-time 0.3]
                                    [--torch-reps 2]
"""

from __future__ import annotations

import argparse
import json
import sys
import time

import torch


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
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-time", type=float, default=0.3)
    ap.add_argument("--torch-reps", type=int, default=2,
                    help="timed repetitions of the torch path per round")
    ap.add_argument("--kappa", type=float, default=0.115)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_clover_force: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import GaugeField, LatticeGeometry
    from quda_amd.gauge import fermion_force as ff
    from quda_amd.gauge import hmc
    from quda_amd.ops.dispatch import hip_ext

    ext = hip_ext()
    kappa, dt = args.kappa, 1e-3
    for lat in args.lattices.split(","):
        dims = tuple(int(x) for x in lat.split("x"))
        geo = LatticeGeometry(dims)
        u = GaugeField(geo, "double").random_su3_(seed=7).to_complex()
        u = u.cuda().contiguous()
        P0 = hmc.random_momentum(geo, "cuda", seed=8).contiguous()
        larg = (list(geo.dims), geo.parity_offset, geo.volume_cb)
        gen = torch.Generator(device="cuda").manual_seed(9)
        for n in (1, 4):
            XY = torch.randn((2, n, 2, geo.volume_cb, 4, 3), device="cuda",
                             dtype=torch.complex128, generator=gen)
            X, Y = XY[0].contiguous(), XY[1].contiguous()
            coeffs = [1.0, -0.6, 0.8, 0.3][:n]
            cdev = torch.tensor(coeffs, dtype=torch.float64, device="cuda")
            for csw in (0.0, 1.0):
                mom = P0.clone()
                h = (ff.clover_sigma_oprod(geo, X, Y, coeffs, u) if csw
                     else torch.empty(0, dtype=u.dtype, device="cuda"))
                # deriv moves u, H and the momentum in and out
                moved = u.numel() * 16 * 3 + h.numel() * 16
                src = torch.empty(moved // 2, dtype=torch.uint8,
                                  device="cuda")
                dst = torch.empty_like(src)

                def force(native, **kw):
                    return ff.clover_force_from_solutions(
                        u, geo, kappa, csw, X, Y, coeffs, native=native,
                        **kw)

                def axpy():
                    mom.add_(force(True), alpha=dt)

                variants = {
                    "torch": lambda: force(False),
                    "native": lambda: force(True),
                    "fused": lambda: force(True, mom=mom, dt=dt),
                    "axpy": axpy,
                    "deriv": lambda: ext.clover_force_dir(
                        mom, u, h, X, Y, cdev, *larg, kappa, csw, dt, True),
                    "copy": lambda: dst.copy_(src),
                }
                if csw:
                    variants["oprod"] = lambda: ext.clover_force_oprod(
                        h, u, X, Y, cdev, *larg)
                times = {k: [] for k in variants}
                reps = {}
                for _ in range(args.rounds):
                    for k, fn in variants.items():
                        if k == "torch":
                            t, r = timed(fn, 0.0, args.torch_reps,
                                         args.torch_reps)
                        else:
                            t, r = timed(fn, args.min_time)
                        times[k].append(t)
                        reps[k] = r
                Ft, Fn = force(False), force(True)
                best = {k: min(v) for k, v in times.items()}
                print(json.dumps({
                    "lattice": list(dims), "csw": csw, "n": n,
                    "kappa": kappa,
                    "seconds": {k: [round(t, 7) for t in v]
                                for k, v in times.items()},
                    "reps": reps,
                    "ms_torch": best["torch"] * 1e3,
                    "ms_native": best["native"] * 1e3,
                    "speedup_native_vs_torch": best["torch"]
                    / best["native"],
                    "speedup_fused_vs_axpy": best["axpy"] / best["fused"],
                    "deriv_bytes_moved": moved,
                    "deriv_copy_fraction": best["copy"] / best["deriv"],
                    "max_abs_native_minus_torch":
                        (Fn - Ft).abs().max().item(),
                    "max_abs_force": Ft.abs().max().item(),
                }), flush=True)
                del Ft, Fn, src, dst, h
                torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
