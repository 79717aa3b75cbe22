#!/usr/bin/env python3
"""Multi-BLAS family: the torch path (flag off, the code of the parent
commit) against the native kernels (csrc/multi_blas.h), in one process on one
GPU, on single-parity nspin-4 fields as the eigensolver holds them.

Per lattice and precision it times
  cdot N    block_cdot of N x N vectors (two sets), for each --sizes
  gram N    block_cdot(xs, xs), native only reads N vectors
  caxpy N   block_caxpy of N x N (double, single)
  rot m,k   the basis rotation: eigen._rotate with the flag off (m k caxpy
            passes) against block_rotate, for each --rotate
  trlm      one TRLM cycle from scratch (n_kr Lanczos steps with full
            re-orthogonalisation, the rotation and n_ev residuals) on a
            Wilson operator, flag off against flag on (--trlm n_ev,n_kr)
with device events around a window of calls (about --window-ms of work, at
most 50 calls), each variant warmed up first and the variants alternated over
--rounds rounds; the figure is the median of the rounds. Before the timing
every native result is compared with the torch one. Prints one JSON line per
(lattice, precision) with the medians, the ratios, the peak extra device
memory of one call and the shape-derived compulsory bytes with the achieved
rate: every operand once per 32 partner vectors, every output once.

Usage: python bench_multi_blas.py [--lattices 16x16x16x32,32x32x32x64]
                                  [--precisions double,single,half]
                                  [--sizes 4,16,32] [--rotate 64x32,128x64]
                                  [--trlm 32,64] [--rounds 5] [--window-ms 20]
"""

from __future__ import annotations

import argparse
import itertools
import json
import os
import statistics
import sys

import torch

ITEM = {"double": 8, "single": 4, "half": 2}
FLAG = "QUDA_AMD_NATIVE_MULTI_BLAS"


def field_bytes(sites: int, prec: str) -> int:
    return sites * (24 * ITEM[prec] + (4 if prec == "half" else 0))


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


def with_flag(on: bool, fn):
    def run():
        os.environ[FLAG] = "1" if on else "0"
        try:
            return fn()
        finally:
            os.environ.pop(FLAG, None)
    return run


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="16x16x16x32,32x32x32x64")
    ap.add_argument("--precisions", default="double,single,half")
    ap.add_argument("--sizes", default="4,16,32")
    ap.add_argument("--rotate", default="64x32,128x64")
    ap.add_argument("--trlm", default="32,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_multi_blas: needs a GPU", file=sys.stderr)
        return 2

    from quda_amd import GaugeField, LatticeGeometry, SpinorField
    from quda_amd.models import DiracWilsonPC
    from quda_amd.ops import dispatch
    from quda_amd.ops.multi_blas import block_caxpy, block_cdot, block_rotate
    from quda_amd.solvers import eigen

    dispatch.hip_ext()
    sizes = [int(v) for v in args.sizes.split(",") if v]
    rots = [tuple(int(c) for c in v.split("x"))
            for v in args.rotate.split(",") if v]
    trlm = [int(v) for v in args.trlm.split(",") if v]
    props = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": props.name,
                      "cus": props.multi_processor_count}), flush=True)

    for lat, prec in itertools.product(args.lattices.split(","),
                                       args.precisions.split(",")):
        dims = tuple(int(v) for v in lat.split("x"))
        geo = LatticeGeometry(dims)
        writes = prec != "half"
        nvec = max(sizes + ([m for m, _ in rots] if writes else []))
        gen = torch.Generator().manual_seed(3)

        def new(seed):
            return SpinorField(geo, prec, "cuda", n_parity=1).gaussian_(seed=seed)

        xs = [new(i) for i in range(nvec)]
        ys = [new(1000 + i) for i in range(max(sizes))]
        fb = field_bytes(geo.volume_cb, prec)
        variants, same, least = {}, {}, {}
        for n in sizes:
            variants[f"cdot{n}_torch"] = (
                lambda n=n: block_cdot(xs[:n], ys[:n], native=False))
            variants[f"cdot{n}_native"] = (
                lambda n=n: block_cdot(xs[:n], ys[:n], native=True))
            variants[f"gram{n}_torch"] = (
                lambda n=n: block_cdot(xs[:n], xs[:n], native=False))
            variants[f"gram{n}_native"] = (
                lambda n=n: block_cdot(xs[:n], xs[:n], native=True))
            least[f"cdot{n}"], least[f"gram{n}"] = 2 * n * fb, n * fb
            if writes:
                A = 1e-3 * torch.randn(n, n, dtype=torch.complex128,
                                       generator=gen)
                for k in ("torch", "native"):
                    variants[f"caxpy{n}_{k}"] = (
                        lambda n=n, A=A, k=k: block_caxpy(
                            A, xs[:n], ys[:n], native=k == "native")[0].data)
                least[f"caxpy{n}"] = 3 * n * fb
        for m, k in rots if writes else []:
            Z = torch.randn(m, k, dtype=torch.float64, generator=gen).numpy()
            variants[f"rot{m}x{k}_torch"] = with_flag(
                False, lambda m=m, Z=Z: eigen._rotate(xs, Z, m)[-1].data)
            variants[f"rot{m}x{k}_native"] = (
                lambda m=m, Z=Z: block_rotate(xs[:m], Z, native=True)[-1].data)
            least[f"rot{m}x{k}"] = (-(-k // 32) * m + k) * fb
        if trlm and prec == "double":
            n_ev, n_kr = trlm
            op = DiracWilsonPC(
                GaugeField(geo, prec, "cuda").random_su3_(seed=5), 0.1)

            def cycle():
                x0 = new(77)
                r = eigen.trlm_solve(op, n_ev, n_kr, x0, tol=1e-30,
                                     max_restarts=1)
                return torch.tensor(r.evals)

            variants["trlm_torch"] = with_flag(False, cycle)
            variants["trlm_native"] = with_flag(True, cycle)

        # results first: native against torch on the operands that are timed
        # (the caxpy pairs update ys in place, so they differ by one update)
        rel = {}
        for k in variants:
            if k.endswith("_native") and not k.startswith("caxpy"):
                ref = variants[k[:-7] + "_torch"]()
                rel[k] = ((variants[k]().to(ref.dtype) - ref).abs().max()
                          / ref.abs().max()).item()
                del ref
        peaks = {k: peak_extra(fn) for k, fn in variants.items()}
        reps = {k: max(1, min(50, int(args.window_ms / event_ms(fn))))
                for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(event_ms(fn, reps[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        out = {"lattice": list(dims), "precision": prec, "field_bytes": fb,
               "median_ms": {k: round(v, 4) for k, v in med.items()},
               "min_ms": {k: round(min(v), 4) for k, v in times.items()},
               "max_rel_diff_vs_torch": rel, "peak_extra_bytes": peaks,
               "speedup": {}, "least_bytes": least, "native_tbs": {}}
        for k in med:
            if k.endswith("_native"):
                b = k[:-7]
                out["speedup"][b] = round(med[b + "_torch"] / med[k], 3)
                if b in least:
                    out["native_tbs"][b] = round(least[b] / med[k] / 1e9, 3)
        print(json.dumps(out), flush=True)
        del xs, ys, variants
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
