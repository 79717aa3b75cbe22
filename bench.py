#!/usr/bin/env python3
"""Flagship benchmark: Wilson-clover even-odd-preconditioned CG,
32^3 x 64 local lattice, double-outer / half-sloppy mixed precision —
the BASELINE.json headline config ("Wilson-clover Dslash GFLOPS/GPU +
CG time-to-solution, 32^3x64 mixed-prec").

One "step" = ONE FULL mixed-precision CG solve from x=0 to --tol
(relative L2 residual) with PRODUCTION settings: reliable updates ON at
delta=0.1, nothing skipped. The gauge field is a random SU(3) field and
the source is gaussian — the reference's own benchmark protocol
(tests/utils/host_utils.cpp constructRandomGaugeField;
tests/invert_test.cpp:300-376 verification scheme). The metric is
aggregate sustained GFLOPS over the whole job from the reference flop
model (include/dslash.h:467: Wilson 1320 flop/site, clover 504; blas and
reliable-update work counted per op from the MEASURED iteration and
update counts). secs-per-solve (time-to-solution) is reported alongside.

Weak scaling: each rank owns a full 32^3x64 local lattice; ranks are laid
out along T (one global 4-d lattice, T-partitioned; the CG reductions and
halo exchanges are global, so the iteration count is rank-independent).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from quda_amd import GaugeField, LatticeGeometry, SpinorField  # noqa: E402
from quda_amd.fields.clover import CloverField, pack_clover  # noqa: E402
from quda_amd.models import DiracCloverPC  # noqa: E402
from quda_amd.ops import blas  # noqa: E402
from quda_amd.ops import reference as ref  # noqa: E402
from quda_amd.parallel import comms  # noqa: E402
from quda_amd.solvers import cg_solve  # noqa: E402

CSW = 1.0


def setup_fields(geo, device, sloppy_prec, seed, kappa):
    """Random SU(3) gauge + clover at double and sloppy precision."""
    g = GaugeField(geo, "double", device)
    # generate directly on device (host gen at 32^3x64 is minutes of QR)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    m = torch.randn((4, 2, geo.volume_cb, 3, 3, 2), generator=gen,
                    dtype=torch.float32)
    from quda_amd.fields.gauge import project_su3
    u = project_su3(torch.view_as_complex(m.to(torch.float64)).to(device))
    g.from_complex(u)
    A = ref.clover_matrix(u, geo, kappa, CSW)
    cl = CloverField(geo, "double", device).from_matrices(A)
    # sloppy copies
    recon = "twelve" if sloppy_prec != "double" else "none"
    gs = GaugeField(geo, sloppy_prec, device, reconstruct=recon).from_complex(u)
    cls = CloverField(geo, sloppy_prec, device)
    cls.data.copy_(cls._to_native(pack_clover(A)))
    cls.inv_data.copy_(cls._to_native(pack_clover(cl.to_complex(inverse=True).to(device))))
    return g, cl, gs, cls


def flops_per_iter(Vcb: int) -> float:
    """Flop count of one sloppy CG iteration on the even-odd clover system.

    MdagM = M (2 fused dslash-clover launches: 2*(1320+504+48 xpay/scale))
          + Mdag (clover-inv 504 + fused 1824 + dslash 1320 + 48)
    blas  = re_dot 48, axpy 48, axpy_norm2 96, xpay 48   (2 flop/real=24/site *2)
    """
    mdagm = (2 * (1320 + 504) + 48) + (504 + 1824 + 1320 + 48)
    blas_f = 48 + 48 + 96 + 48
    return float(Vcb) * (mdagm + blas_f)


def flops_per_reliable(Vcb: int) -> float:
    """One reliable update: precise MdagM + xmy_norm2 + accumulate/copy blas."""
    mdagm = (2 * (1320 + 504) + 48) + (504 + 1824 + 1320 + 48)
    return float(Vcb) * (mdagm + 96 + 48 + 48)


DUMP_MAX_BYTES = 48 << 20


def dump_outputs(out_dir, x, stats, seed, rank, world):
    """Write what the last timed solve handed back: the solution spinor as
    float64 [sites, 4, 3, 2] (re, im) and the solve statistics
    [iters, reliable_updates, resid]. A solution larger than DUMP_MAX_BYTES
    is reduced to a fixed, seeded sample of checkerboard sites (ascending
    site index), the same sites for the same --seed and lattice."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if world == 1 else f"_rank{rank}"
    sol = torch.view_as_real(x.to_complex()[0])            # [Vcb, 4, 3, 2]
    n_sites = sol.shape[0]
    keep = DUMP_MAX_BYTES // (sol[0].numel() * 8)
    if n_sites > keep:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed + 200)
        sites = torch.randperm(n_sites, generator=gen)[:keep].sort().values
        sol = sol[sites.to(sol.device)]
    np.save(os.path.join(out_dir, f"solution{suffix}.npy"),
            sol.to("cpu", torch.float64).contiguous().numpy())
    np.save(os.path.join(out_dir, f"solve_stats{suffix}.npy"),
            np.array([stats.iters, stats.reliable_updates, stats.resid],
                     dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tol", type=float, default=1e-8,
                    help="relative residual target of each solve")
    ap.add_argument("--delta", type=float, default=0.1,
                    help="reliable-update trigger (production default 0.1)")
    ap.add_argument("--maxiter", type=int, default=2000)
    ap.add_argument("--lattice", type=str, default="32,32,32,64")
    ap.add_argument("--kappa", type=float, default=0.34,
                    help="hopping parameter; the default targets a HARD "
                         "near-critical solve on the random field "
                         "(hundreds of iterations), the honest "
                         "time-to-solution regime")
    ap.add_argument("--sloppy", type=str, default="half",
                    choices=["double", "single", "half", "quarter"])
    ap.add_argument("--seed", type=int, default=777)
    ap.add_argument("--device", default=None,
                    help="override (cpu for harness tests; default cuda:LOCAL_RANK)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the solution of the "
                         "last timed solve (and its iteration statistics) "
                         "as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement; the headline "
                         "solve is all this benchmark measures, so there is "
                         "nothing extra to run yet")
    args = ap.parse_args()
    assert args.steps >= 1, "--steps must be at least 1"

    dims = tuple(int(d) for d in args.lattice.split(","))
    # a CPU run talks over gloo even where a GPU is visible: the default
    # backend choice would bind rank r to cuda:r, which need not exist
    on_cpu = args.device is not None and args.device.startswith("cpu")
    rank, world = comms.init_comms(backend="gloo" if on_cpu else None)
    assert world == args.gpus or "WORLD_SIZE" not in os.environ, \
        f"world {world} != --gpus {args.gpus}"
    if args.device:
        device = args.device
    else:
        device = f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}"
        torch.cuda.set_device(device)

    geo = LatticeGeometry(dims, parity_offset=comms.parity_offset_of_rank(dims))
    g, cl, gs, cls = setup_fields(geo, device, args.sloppy, args.seed + rank,
                                  args.kappa)
    d = DiracCloverPC(g, cl, args.kappa)
    ds = DiracCloverPC(gs, cls, args.kappa)

    b = SpinorField(geo, "double", device, n_parity=1).gaussian_(seed=args.seed + 100 + rank)
    x = SpinorField(geo, "double", device, n_parity=1)

    counts = {"iters": 0, "reliable": 0, "resid": 0.0}

    def step(record=False):
        x.zero_()
        # one production solve: solve-to-tolerance, reliable updates ON
        st = cg_solve(d, x, b, op_sloppy=ds, sloppy=args.sloppy,
                      tol=args.tol, maxiter=args.maxiter, delta=args.delta)
        if record:
            counts["iters"] += st.iters
            counts["reliable"] += st.reliable_updates
            counts["resid"] = st.resid
            counts["last"] = st
        return st

    for _ in range(args.warmup):
        st0 = step()
    comms.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(record=True)
    comms.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    # max over ranks
    if comms.is_distributed():
        import torch.distributed as dist
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, x, counts["last"], args.seed, rank, world)

    ms_per_step = elapsed / args.steps * 1000.0
    total_flops = (flops_per_iter(geo.volume_cb) * counts["iters"]
                   + flops_per_reliable(geo.volume_cb) * counts["reliable"]) * world
    gflops = total_flops / elapsed / 1e9

    if rank == 0:
        out = {
            "metric": "wilson_clover_cg_gflops",
            "value": round(gflops, 3),
            "unit": "GFLOPS",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "double-half" if args.sloppy == "half" else f"double-{args.sloppy}",
            "data": "synthetic",
            "config": {
                "model": "wilson_clover_eo_pc_cg",
                "lattice_per_gpu": "x".join(str(v) for v in dims),
                "global_batch": 1,
                "seq_len": geo.volume,
                "kappa": args.kappa,
                "kappa_standard_convention": args.kappa / 2,
                "csw": CSW,
                "solve_tol": args.tol,
                "reliable_delta": args.delta,
                "secs_per_solve": round(elapsed / args.steps, 4),
                "iters_per_solve": counts["iters"] / args.steps,
                "reliable_updates_per_solve": counts["reliable"] / args.steps,
                "final_resid": counts["resid"],
                "parallelism": f"dd_t{world}",
                "gauge_recon_sloppy": 12 if args.sloppy != "double" else 18,
            },
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()
