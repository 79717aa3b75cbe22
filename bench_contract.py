#!/usr/bin/env python3
"""Contraction family: the torch path (flag off) against the native kernels
(csrc/contract.h), in one process on one GPU.

Per lattice and precision it times
  ft      contract_ft for each --n-mom, torch and every NS variant
  dot     the two-field BLAS reduction (blas_op REDOT): the yardstick of ft
  site    contract_dr, torch and native
  evec    evec_project for each --n-ev, torch and every NE variant
with device events around a window of calls (about --window-ms of work, at
most 100 calls), each variant warmed up first and the variants alternated
over --rounds rounds; the figure is the median of the rounds. Before
the timing every native result is compared with the torch one. Prints one
JSON line per (lattice, precision) with the medians, the ratios, the peak
extra device memory of one call, and the shape-derived compulsory bytes:
x and y once (ft, site: plus the [V,16] result), psi once per batch and each
eigenvector once (evec).

Usage: python bench_contract.py [--lattices 16x16x16x32,32x32x32x64]
                                [--precisions double,single]
                                [--n-mom 1,27] [--n-ev 8,64] [--rounds 5]
                                [--window-ms 20]
"""

from __future__ import annotations

import argparse
import itertools
import json
import statistics
import sys

import torch

ITEM = {"double": 8, "single": 4, "half": 2}
NS_VARIANTS = (128, 256)
NE_VARIANTS = (4, 8)


def field_bytes(volume: int, prec: str, nspin: int) -> int:
    return volume * (6 * nspin * ITEM[prec] + (4 if prec == "half" else 0))


def event_ms(fn, reps: int = 1) -> float:
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def peak_extra(fn) -> int:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def ft_torch(x, y, momenta, rd):
    """contract_ft's torch formula with the coordinates moved to the fields'
    device (the function keeps them on the CPU and raises for GPU fields)."""
    import numpy as np
    from quda_amd.ops import contract
    geo = x.geo
    c = contract.contract_dr(x, y, native=False)
    coords = geo.coords.to(c.device, torch.float64)
    tcoord = geo.coords[:, rd].to(c.device, torch.int64)
    out = torch.empty((len(momenta), geo.dims[rd], 16), dtype=c.dtype,
                      device=c.device)
    for ip, p in enumerate(momenta):
        arg = sum(2 * np.pi * p[i] * coords[:, i] / geo.dims[i]
                  for i in range(4) if i != rd)
        w = c * torch.exp(-1j * arg).to(c.dtype).unsqueeze(-1)
        out[ip] = torch.zeros((geo.dims[rd], 16), dtype=c.dtype,
                              device=c.device).index_add_(0, tcoord, w)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="16x16x16x32,32x32x32x64")
    ap.add_argument("--precisions", default="double,single")
    ap.add_argument("--n-mom", default="1,27")
    ap.add_argument("--n-ev", default="8,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_contract: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import LatticeGeometry, SpinorField
    from quda_amd.ops import blas, contract, dispatch

    ext = dispatch.hip_ext()
    n_moms = [int(v) for v in args.n_mom.split(",")]
    n_evs = [int(v) for v in args.n_ev.split(",")]
    all_mom = list(itertools.product((-1, 0, 1), repeat=3))
    all_mom.sort(key=lambda p: sum(c * c for c in p))  # (0,0,0) first
    gam = contract.gamma_table()
    props = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": props.name,
                      "cus": props.multi_processor_count}), flush=True)

    for lat, prec in itertools.product(args.lattices.split(","),
                                       args.precisions.split(",")):
        dims = tuple(int(v) for v in lat.split("x"))
        geo = LatticeGeometry(dims)
        x = SpinorField(geo, prec, "cuda").gaussian_(seed=1)
        y = SpinorField(geo, prec, "cuda").gaussian_(seed=2)
        evs = [SpinorField(geo, prec, "cuda", nspin=1).gaussian_(seed=10 + i)
               for i in range(max(n_evs))]
        variants, same = {}, {}
        variants["dot"] = lambda: blas._gpu_blas(ext.BLAS_REDOT, 0, 0, x, y)
        variants["site_torch"] = lambda: contract.contract_dr(x, y, native=False)
        variants["site_native"] = lambda: contract.contract_dr(x, y, native=True)
        for nm in n_moms:
            mom = [p + (0,) for p in all_mom[:nm]]
            f = contract.phase_table(dims, mom, 3)
            variants[f"ft{nm}_torch"] = (
                lambda mom=mom: ft_torch(x, y, mom, 3))
            for ns in NS_VARIANTS:
                variants[f"ft{nm}_ns{ns}"] = (
                    lambda f=f, ns=ns: dispatch.contract_slices(x, y, gam, f, 3, ns))
                same[f"ft{nm}_ns{ns}"] = f"ft{nm}_torch"
        for nv in n_evs:
            variants[f"evec{nv}_torch"] = (
                lambda nv=nv: contract.evec_project(evs[:nv], x, 3, native=False))
            for ne in NE_VARIANTS:
                variants[f"evec{nv}_ne{ne}"] = (
                    lambda nv=nv, ne=ne: dispatch.evec_project_slices(
                        evs[:nv], x, 3, ne))
                same[f"evec{nv}_ne{ne}"] = f"evec{nv}_torch"
        same["site_native"] = "site_torch"

        # results first: native against torch on the operands that are timed
        ref = {k: variants[k]() for k in set(same.values())}
        rel = {}
        for k, r in same.items():
            rel[k] = ((variants[k]() - ref[r]).abs().max()
                      / ref[r].abs().max()).item()
        del ref
        peaks = {k: peak_extra(fn) for k, fn in variants.items()}
        reps = {k: max(1, min(100, int(args.window_ms / event_ms(fn))))
                for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(event_ms(fn, reps[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        two = 2 * field_bytes(geo.volume, prec, 4)
        out = {"lattice": list(dims), "precision": prec,
               "median_ms": {k: round(v, 4) for k, v in med.items()},
               "min_ms": {k: round(min(v), 4) for k, v in times.items()},
               "max_rel_diff_vs_torch": rel, "peak_extra_bytes": peaks,
               "two_field_bytes": two,
               "dot_tbs": two / med["dot"] / 1e9,
               "site_native_tbs": (two + geo.volume * 256)
               / med["site_native"] / 1e9}
        for nm in n_moms:
            for ns in NS_VARIANTS:
                k = f"ft{nm}_ns{ns}"
                out[f"{k}_tbs"] = two / med[k] / 1e9
                out[f"{k}_over_dot"] = med[k] / med["dot"]
                out[f"{k}_speedup"] = med[f"ft{nm}_torch"] / med[k]
        for nv in n_evs:
            for ne in NE_VARIANTS:
                k = f"evec{nv}_ne{ne}"
                least = (-(-nv // ne) * field_bytes(geo.volume, prec, 4)
                         + nv * field_bytes(geo.volume, prec, 1))
                out[f"{k}_bytes"] = least
                out[f"{k}_tbs"] = least / med[k] / 1e9
                out[f"{k}_speedup"] = med[f"evec{nv}_torch"] / med[k]
        print(json.dumps(out), flush=True)
        del x, y, evs, variants
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
