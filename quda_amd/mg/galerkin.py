"""Native Galerkin coarse-operator build (csrc/galerkin.hip): the tables and
operands the kernel reads, the eligibility rule, and the build itself.

The kernel computes exactly what coarse.build_coarse_op computes — X and the
eight Y[d] of the fine Wilson(-clover) operator — from the aggregate-ordered
Transfer.V in one launch per build instead of 2*Nvec column passes. Rows of
every operand are ab = a*B + b in the (a, b) order of Transfer.sites_by_agg.
ops.reference.galerkin_from_tables consumes the same operands in pure torch.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from ..fields.geometry import LatticeGeometry
from ..ops.reference import _gamma_tensors


def native_galerkin_default() -> bool:
    """QUDA_AMD_MG_NATIVE_GALERKIN=1 opts into the HIP Galerkin build
    (csrc/galerkin.hip); off by default."""
    return os.environ.get("QUDA_AMD_MG_NATIVE_GALERKIN", "0") == "1"


def _sites_by_agg(geo: LatticeGeometry, block) -> torch.Tensor:
    """Flat [Na*B] lex site of every (a, b), as Transfer.sites_by_agg."""
    cd = tuple(geo.dims[i] // block[i] for i in range(4))
    c = geo.coords.to(torch.int64)
    bc = [c[:, i] // block[i] for i in range(4)]
    agg_of_lex = ((bc[3] * cd[2] + bc[2]) * cd[1] + bc[1]) * cd[0] + bc[0]
    return torch.argsort(agg_of_lex, stable=True)


def galerkin_tables(geo: LatticeGeometry, block) -> Tuple[torch.Tensor,
                                                         torch.Tensor]:
    """Index tables of the native Galerkin build, on the CPU:
    nbr_ab [Na*B, 8] int32, the row (a', b') of the d-neighbour (d = 2*mu +
    fwd, periodic wrap) of row (a, b), and bnd [Na*B] uint8 whose bit d says
    the site lies on the d-face of its block: coord[mu] % block[mu] ==
    block[mu]-1 (fwd) or == 0 (bwd). The flag is a property of the
    coordinates, not of where the neighbour lives: with a coarse extent of 1
    the neighbour is in the same aggregate and the hop still belongs to Y[d];
    with a block extent of 1 every site is on both faces."""
    sites = _sites_by_agg(geo, block)
    ab_of_lex = torch.empty_like(sites)
    ab_of_lex[sites] = torch.arange(geo.volume, dtype=torch.int64)
    c = geo.coords.to(torch.int64)[sites]
    nbr = torch.empty((geo.volume, 8), dtype=torch.int64)
    bnd = torch.zeros(geo.volume, dtype=torch.int64)
    for mu in range(4):
        for fwd in (0, 1):
            d = 2 * mu + fwd
            nbr[:, d] = ab_of_lex[geo.neighbor_lex(mu, +1 if fwd else -1)[sites]]
            edge = block[mu] - 1 if fwd else 0
            bnd |= ((c[:, mu] % block[mu]) == edge).to(torch.int64) << d
    return nbr.to(torch.int32).contiguous(), bnd.to(torch.uint8)


def _tables_on(geo: LatticeGeometry, block, device):
    """galerkin_tables plus the lex sites and the lex backward neighbours,
    cached per (block, device) on the geometry (an MG refresh rebuilds the
    coarse operator on the same lattice)."""
    cache = geo.__dict__.setdefault("_galerkin_cache", {})
    key = (tuple(block), str(device))
    if key not in cache:
        nbr, bnd = galerkin_tables(geo, block)
        sites = _sites_by_agg(geo, block)
        back = torch.stack([geo.neighbor_lex(mu, -1)[sites]
                            for mu in range(4)])
        cache[key] = (nbr.to(device), bnd.to(device), sites.to(device),
                      back.to(device))
    return cache[key]


def galerkin_operands(op, geo: LatticeGeometry, sites: torch.Tensor,
                      back: torch.Tensor) -> Tuple[torch.Tensor,
                                                   Optional[torch.Tensor]]:
    """Gather the fine operator once per build, in row order and complex128:
    link_ab [Na*B, 8, 3, 3] with link_ab[:, 2mu+1] = U_mu(x) and
    link_ab[:, 2mu] = U_mu(x-mu)^dagger, and clov_ab [Na*B, 12, 12] (None
    for an operator without a clover term). Boundary phases, anisotropy and
    reconstruction are whatever to_complex() folded in. `sites` [Na*B] are
    the lex sites of the rows, `back` [4, Na*B] their lex -mu neighbours."""
    dev = sites.device
    u_cb = op.gauge.to_complex().to(torch.complex128)
    lo = geo.lex_of_cb.to(dev)
    u_lex = torch.empty((4, geo.volume, 3, 3), dtype=u_cb.dtype, device=dev)
    u_lex[:, lo[0]] = u_cb[:, 0]
    u_lex[:, lo[1]] = u_cb[:, 1]
    link = torch.empty((geo.volume, 8, 3, 3), dtype=u_cb.dtype, device=dev)
    for mu in range(4):
        link[:, 2 * mu + 1] = u_lex[mu][sites]
        link[:, 2 * mu] = u_lex[mu][back[mu]].conj().transpose(-1, -2)
    clov = None
    clover = getattr(op, "clover", None)
    if clover is not None:
        A_cb = clover.to_complex().to(torch.complex128)  # [2, Vcb, 12, 12]
        A_lex = torch.empty((geo.volume, 12, 12), dtype=A_cb.dtype, device=dev)
        A_lex[lo[0]] = A_cb[0]
        A_lex[lo[1]] = A_cb[1]
        clov = A_lex[sites].contiguous()
    return link, clov


def hop_coefficients(kappa, device) -> torch.Tensor:
    """[8, 4, 4] complex128: -kappa * P_d, with P_d the spin projector of the
    non-dagger hop of direction d = 2*mu + fwd (fwd: P[mu, 0], bwd:
    P[mu, 1] of ops.reference._gamma_tensors)."""
    P = _gamma_tensors(device, torch.complex128)
    return (-kappa * torch.stack([P[d // 2, 1 - d % 2] for d in range(8)])
            ).contiguous()


def galerkin_eligible(op, transfer, native: Optional[bool] = None) -> bool:
    """True when build_coarse_op runs the HIP build: the flag is on
    (native, or the environment when native is None), transfer.V is a
    complex128 GPU tensor, the run is single-rank in every direction, and
    `op` is of the class the torch build handles (gauge and kappa, clover
    optional). Everything else takes the torch path unchanged."""
    from ..parallel import comms
    on = native_galerkin_default() if native is None else bool(native)
    V = transfer.V
    return bool(on and V.device.type == "cuda" and V.dtype == torch.complex128
                and comms.comm_mask() == 0
                and hasattr(op, "gauge") and hasattr(op, "kappa"))


def build_coarse_native(op, transfer):
    """(X [Na,Nc,Nc], [Y[0..7]]) of the fine operator through the HIP
    kernel; callers check galerkin_eligible first."""
    from ..ops import dispatch
    geo = transfer.geo
    dev = transfer.V.device
    nbr, bnd, sites, back = _tables_on(geo, transfer.block, dev)
    link, clov = galerkin_operands(op, geo, sites, back)
    coef = hop_coefficients(op.kappa, dev)
    X, Y = dispatch.galerkin_build(transfer.V.contiguous(), nbr, bnd, link,
                                   clov, coef)
    return X, list(Y.unbind(0))
