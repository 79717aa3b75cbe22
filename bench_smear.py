#!/usr/bin/env python3
"""Link smearing: the torch paths of hyp_smear, ape_smear and
over_improved_stout_smear against the native paths (csrc/smear.hip and the
path-table kernel), in one process on one GPU, complex128.

Per lattice it reports
  iter_s     seconds per iteration of each path of HYP, 4-d APE and
             over-improved stout (--iters iterations per timed window, one
             for over-improved stout), the two paths alternating
  max_diff   largest entry difference between the two paths' results
  levels     each of the five level launches alone: seconds, and its
             compulsory traffic (every src, cen and out slot once, 144 bytes
             a link) over that time
Host clock with a device synchronise on both sides of every timed window;
every variant is warmed up before it is timed. One JSON line per lattice.

Usage: python bench_smear.py [--lattices 16x16x16x32,24x24x24x48]
                             [--iters 10] [--torch-iters 10] [--rounds 3]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="16x16x16x32,24x24x24x48")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--level-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_smear: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import GaugeField, LatticeGeometry
    from quda_amd.fields.gauge import project_su3
    from quda_amd.gauge import (ape_smear, hyp_smear,
                                over_improved_stout_smear)
    from quda_amd.gauge import smear as sm
    from quda_amd.ops import dispatch
    ext = dispatch.hip_ext()
    alpha_hyp, alpha_ape, rho = (0.75, 0.6, 0.3), 0.5, 0.06

    for lat in args.lattices.split(","):
        dims = tuple(int(x) for x in lat.split("x"))
        geo = LatticeGeometry(dims)
        hot = GaugeField(geo, "double").random_su3_(
            seed=11).to_complex().cuda()
        eye = torch.eye(3, dtype=hot.dtype, device=hot.device)
        u = project_su3(eye + 0.3 * (hot - eye)).contiguous()
        del hot

        kinds = {
            "hyp": lambda native, n: hyp_smear(u, geo, alpha_hyp, n_iter=n,
                                               native=native),
            "ape": lambda native, n: ape_smear(u, geo, alpha_ape, n_iter=n,
                                               native=native),
            "over_improved_stout": lambda native, n:
                over_improved_stout_smear(u, geo, rho, n_iter=n,
                                          native=native),
        }
        iter_s, max_diff = {}, {}
        for name, fn in kinds.items():
            one = name == "over_improved_stout"
            n_of = {"torch": 1 if one else args.torch_iters,
                    "native": 1 if one else args.iters}
            times = {"torch": [], "native": []}
            for _ in range(args.rounds):  # alternate the two paths
                for path, native in (("torch", False), ("native", True)):
                    fn(native, 1)  # warm-up
                    n = n_of[path]
                    times[path].append(wall(lambda: fn(native, n))[0] / n)
            iter_s[name] = {k: [round(t, 6) for t in v]
                            for k, v in times.items()}
            iter_s[name]["speedup"] = (min(times["torch"])
                                       / min(times["native"]))
            max_diff[name] = (fn(True, 1) - fn(False, 1)).abs().max().item()
            torch.cuda.empty_cache()

        # the five level launches alone
        larg = (list(dims), geo.parity_offset, geo.volume_cb)
        t1, t2, t3 = sm.hyp_tables()
        k1, k2, k3 = sm.hyp_coeffs(alpha_hyp)
        vbar = torch.empty((12,) + u.shape[1:], dtype=u.dtype, device=u.device)
        vtil = torch.empty_like(vbar)
        out4 = torch.empty_like(u)
        calls = {
            "hyp1": (vbar, u, t1, *k1, sm.PROJ_POLAR),
            "hyp2": (vtil, vbar, t2, *k2, sm.PROJ_POLAR),
            "hyp3": (out4, vtil, t3, *k3, sm.PROJ_POLAR),
            "ape4": (out4, u, sm.ape_table(False),
                     *sm.ape_coeffs(alpha_ape, False), sm.PROJ_GS),
            "ape3": (out4, u, sm.ape_table(True),
                     *sm.ape_coeffs(alpha_ape, True), sm.PROJ_GS),
        }
        levels = {}
        for name, (o, s, tb, c0, c1, proj) in calls.items():
            def run():
                ext.smear_level(o, s, u, *larg, tb, c0, c1, proj)
            run()
            ts = [wall(lambda: [run() for _ in range(args.level_reps)])[0]
                  / args.level_reps for _ in range(args.rounds)]
            nbytes = (o.shape[0] + s.shape[0]
                      + (4 if s is not u else 0)) * geo.volume * 144
            levels[name] = {"s": [round(t, 8) for t in ts],
                            "bytes": nbytes,
                            "tbs": nbytes / min(ts) / 1e12}
        print(json.dumps({"lattice": list(dims), "iters": args.iters,
                          "torch_iters": args.torch_iters, "iter_s": iter_s,
                          "max_diff": max_diff, "levels": levels}),
              flush=True)
        del u, vbar, vtil, out4
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
