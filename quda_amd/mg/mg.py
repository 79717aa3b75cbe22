"""Multigrid V-cycle preconditioner (ref: lib/multigrid.cpp MG::operator()
:1145 — pre-smooth -> restrict residual -> coarse solve -> prolong ->
post-smooth; used as the K inside flexible GCR, lib/inv_gcr_quda.cpp)."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import torch

from ..fields.spinor import SpinorField
from ..ops import blas
from ..solvers.gcr import mr_solve
from .coarse import CoarseOp, build_coarse_op, coarse_bicgstab
from .transfer import Transfer, generate_null_vectors


@dataclass
class MGParam:
    block: tuple = (2, 2, 2, 2)
    n_vec: int = 4
    levels: int = 2              # 3 = recurse once more on the coarse op
    block2: tuple = (2, 2, 2, 2)
    n_vec2: int = 4
    nu_pre: int = 0
    nu_post: int = 4
    smoother_omega: float = 0.85
    # V-cycle cost tuning (measured on MI355X, profiles/r02_mg_wallclock
    # .md sweep): coarse_tol 1e-1 + maxiter 100 is 13% faster in
    # wall-clock than 5e-2/200 at kappa 0.37 with the same robustness
    coarse_tol: float = 1e-1
    coarse_maxiter: int = 100
    null_tol: float = 5e-5
    null_maxiter: int = 200
    seed: int = 500
    # HIP restrict/prolong/block-orthonormalize (csrc/transfer.hip) instead
    # of the torch transfer; None = env QUDA_AMD_MG_NATIVE_TRANSFER (off)
    native_transfer: Optional[bool] = None
    # HIP Galerkin build of the coarse operator (csrc/galerkin.hip) instead
    # of the torch column loop; None = env QUDA_AMD_MG_NATIVE_GALERKIN (off).
    # Independent of native_transfer: either transfer feeds either build.
    native_galerkin: Optional[bool] = None


class MG:
    """Two-level (recursion-ready) multigrid preconditioner for the FULL
    (non-PC) fine operator `op`. Use .precond as the K of gcr_solve."""

    def __init__(self, op, param: MGParam = MGParam(),
                 vectors: Optional[List[SpinorField]] = None):
        self.op = op
        self.param = param
        if vectors is None:
            vectors = generate_null_vectors(
                op, param.n_vec, tol=param.null_tol,
                maxiter=param.null_maxiter, seed=param.seed)
        self.null_vectors = vectors
        self.transfer = Transfer(op.geo, param.block, vectors,
                                 native=param.native_transfer)
        self.coarse = build_coarse_op(op, self.transfer,
                                      native=param.native_galerkin)
        # which path built X and Y (True: the HIP kernel)
        self.coarse_native = bool(self.coarse.native)
        self.coarse_mg = None
        if param.levels >= 3:
            from .coarse_level import CoarseMG
            self.coarse_mg = CoarseMG(self.coarse, block2=param.block2,
                                      n_vec2=param.n_vec2)

    # -- verification (ref: multigrid.cpp MG::verify) -----------------------
    def verify(self) -> dict:
        """(1 - P R) V = 0 on the null vectors; R P = identity on coarse;
        Galerkin consistency R M P == coarse.apply."""
        t = self.transfer
        out = {}
        # P R on a random fine vector reproduces its aggregate projection
        dev = t.device
        gen = torch.Generator().manual_seed(1)
        c = torch.randn((t.n_agg, 2, t.nvec, 2), generator=gen,
                        dtype=torch.float64)
        cc = torch.view_as_complex(c).to(dev)
        fine = self.op.new_spinor(n_parity=2)
        t.prolong(cc, fine)
        back = t.restrict(fine)
        out["RP_identity"] = (back - cc).abs().max().item()
        # Galerkin: R M P c == coarse.apply(c)
        Mf = self.op.new_spinor(n_parity=2)
        self.op.M(Mf, fine)
        rmp = t.restrict(Mf).reshape(t.n_agg, -1)
        via_coarse = self.coarse.apply(cc.reshape(t.n_agg, -1))
        out["galerkin"] = (rmp - via_coarse).abs().max().item()
        return out

    # -- V-cycle ------------------------------------------------------------
    def precond(self, z: SpinorField, r: SpinorField) -> None:
        """z ~= M^-1 r (one V-cycle)."""
        p = self.param
        op = self.op
        z.zero_()
        if p.nu_pre > 0:
            mr_solve(op, z, r, tol=1e-10, maxiter=p.nu_pre,
                     omega=p.smoother_omega, zero_init=True)
        # coarse correction on the residual
        tmp = op.new_spinor(n_parity=2)
        if p.nu_pre > 0:
            op.M(tmp, z)
            rr = op.new_spinor(n_parity=2)
            blas.copy(rr, r)
            blas.axpy(-1.0, tmp, rr)
        else:
            rr = r
        rc = self.transfer.restrict(rr).reshape(self.transfer.n_agg, -1)
        if self.coarse_mg is not None:
            ec = self.coarse_mg.solve(rc, tol=p.coarse_tol,
                                      maxiter=p.coarse_maxiter)
        else:
            ec = coarse_bicgstab(self.coarse, rc, tol=p.coarse_tol,
                                 maxiter=p.coarse_maxiter)
        e = op.new_spinor(n_parity=2)
        self.transfer.prolong(ec.reshape(self.transfer.n_agg, 2, -1), e)
        blas.axpy(1.0, e, z)
        # post-smooth on the full system (MR with initial guess z)
        if p.nu_post > 0:
            mr_solve(op, z, r, tol=1e-10, maxiter=p.nu_post,
                     omega=p.smoother_omega, zero_init=False)


    # -- null-space persistence (ref: multigrid.cpp:1249 vec_load /
    # vec_outfile over VectorIO; here utils.io checksummed storage) -------
    def save_vectors(self, path: str) -> None:
        from ..utils.io import save_field
        save_field(path, self.null_vectors,
                   meta={"block": self.param.block,
                         "n_vec": self.param.n_vec})

    @staticmethod
    def load_vectors(path: str, device="cpu", precision="double"):
        from ..utils.io import load_field
        return load_field(path, device=device, precision=precision)
