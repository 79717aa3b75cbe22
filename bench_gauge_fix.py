#!/usr/bin/env python3
"""Overrelaxation gauge fixing: the torch path of gauge_fix_ovr (three
maximising hits, native=False) against the native path (one overrelaxed hit,
csrc/gauge_fix.hip), in one process on one GPU, complex128, Landau.

Per lattice it reports
  sweep_s          seconds per sweep of each path (fixed sweep counts, tol < 0)
  solve            seconds and sweeps of each path to theta < --tol from the
                   same randomly gauge-transformed smooth field (the two paths
                   run different algorithms, so only this compares them)
  half_sweep       the native half-sweep kernel alone against its traffic
                   floor 2 * 4V * 144 bytes, as a share of the bandwidth a
                   device copy of the same size achieves in this process
Host clock with a device synchronise on both sides of every timed window;
every variant is warmed up before it is timed. One JSON line per lattice.

Usage: python bench_gauge_fix.py [--lattices 16x16x16x32,32x32x32x64]
                                 [--omega 1.7] [--tol 1e-8] [--max-iter 20000]
                                 [--torch-max-iter 2000]
A run that reaches its sweep cap is reported with converged false and the
theta it reached.
"""

from __future__ import annotations

import argparse
import json
import sys
import time

import torch


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def smooth_transformed(geo, seed: int) -> torch.Tensor:
    """Links near the identity, then a random gauge transformation."""
    from quda_amd import GaugeField
    from quda_amd.fields.gauge import project_su3
    hot = GaugeField(geo, "double").random_su3_(seed=seed).to_complex().cuda()
    eye = torch.eye(3, dtype=hot.dtype, device=hot.device)
    u = project_su3(eye + 0.1 * (hot - eye))
    g = GaugeField(geo, "double").random_su3_(
        seed=seed + 1).to_complex()[0].cuda()
    for mu in range(4):
        for p in (0, 1):
            fwd = geo.neighbor_cb(p, mu, +1).cuda()
            u[mu, p] = g[p] @ u[mu, p] @ g[1 - p][fwd].conj().mT
    return u.contiguous()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="16x16x16x32,32x32x32x64")
    ap.add_argument("--omega", type=float, default=1.7)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--torch-max-iter", type=int, default=2000)
    ap.add_argument("--torch-sweeps", type=int, default=3)
    ap.add_argument("--native-sweeps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_gauge_fix: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import LatticeGeometry
    from quda_amd.gauge import fix
    from quda_amd.gauge.fix import gauge_fix_ovr, gauge_fix_quality
    from quda_amd.ops import dispatch
    ext = dispatch.hip_ext()

    # count the quality evaluations of either engine
    count = [0]

    def counted_quality(*a, **k):
        count[0] += 1
        return gauge_fix_quality(*a, **k)

    class CountingExt:
        def __getattr__(self, name):
            return getattr(ext, name)

        def gauge_fix_quality(self, *a):
            count[0] += 1
            return ext.gauge_fix_quality(*a)

    fix.gauge_fix_quality = counted_quality
    dispatch.hip_ext = lambda required=True: CountingExt()

    for lat in args.lattices.split(","):
        dims = tuple(int(x) for x in lat.split("x"))
        geo = LatticeGeometry(dims)
        u = smooth_transformed(geo, seed=7)
        larg = (list(dims), geo.parity_offset, geo.volume_cb)

        def fixed(native, n):
            return lambda: gauge_fix_ovr(u, geo, omega=args.omega, max_iter=n,
                                         tol=-1.0, native=native,
                                         check_every=n)

        sweep = {"torch": [], "native": []}
        for _ in range(args.rounds):  # alternate the two paths
            for name, native, n in (("torch", False, args.torch_sweeps),
                                    ("native", True, args.native_sweeps)):
                fixed(native, 1)()  # warm-up
                sweep[name].append(wall(fixed(native, n))[0] / n)

        # both paths evaluate theta once per sweep (check_every = 1), so the
        # sweeps of a run are its quality evaluations
        solve = {}
        for name, native in (("torch", False), ("native", True)):
            count[0] = 0
            cap = args.max_iter if native else args.torch_max_iter
            print(f"{lat}: solve {name}, at most {cap} sweeps",
                  file=sys.stderr, flush=True)
            t, uf = wall(lambda: gauge_fix_ovr(
                u, geo, omega=args.omega, max_iter=cap, tol=args.tol,
                native=native))
            sweeps = count[0]
            theta = gauge_fix_quality(uf, geo, 4)[1]
            solve[name] = {"seconds": round(t, 4), "sweeps": sweeps,
                           "theta": theta, "converged": theta < args.tol}
            del uf

        # half-sweep kernel alone, and a copy of the same number of bytes
        w = u.clone()
        src = u.clone()
        n = 40
        half, copy = [], []
        for _ in range(args.rounds):
            ext.gauge_fix_ovr_half(w, *larg, 0, 4, args.omega, False)
            half.append(wall(lambda: [ext.gauge_fix_ovr_half(
                w, *larg, k & 1, 4, args.omega, False)
                for k in range(n)])[0] / n)
            w.copy_(src)
            copy.append(wall(lambda: [w.copy_(src) for _ in range(n)])[0] / n)
        nbytes = 2 * 4 * geo.volume * 144
        out = {
            "lattice": list(dims), "omega": args.omega, "tol": args.tol,
            "sweep_s": {k: [round(t, 7) for t in v]
                        for k, v in sweep.items()},
            "sweep_speedup": min(sweep["torch"]) / min(sweep["native"]),
            "solve": solve,
            "solve_speedup": solve["torch"]["seconds"]
            / solve["native"]["seconds"],
            "half_sweep_s": [round(t, 8) for t in half],
            "copy_s": [round(t, 8) for t in copy],
            "floor_bytes": nbytes,
            "half_sweep_tbs": nbytes / min(half) / 1e12,
            "copy_tbs": nbytes / min(copy) / 1e12,
            "half_sweep_share_of_copy": min(copy) / min(half),
        }
        print(json.dumps(out), flush=True)
        del u, w, src
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
