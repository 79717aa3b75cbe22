"""Native link smearing: the level tables of APE and HYP, their torch
oracle, and the drivers of the HIP level kernel (csrc/smear.hip).

One level computes, for every output slot o with link direction mu_o,

    out[o] = Proj[c0 cen[mu_o] + c1 sum_k staple(src[a_ok], src[b_ok];
                                                 mu_o, eta_ok)]

    staple(A, B; mu, eta)(x) = B(x) A(x+eta) B(x+mu)^dag
                             + B(x-eta)^dag A(x-eta) B(x-eta+mu)

A table is a list of rows [mu, ns, (eta, a, b) x ns]; a row with ns = 0
copies cen[mu] through, unprojected. APE is one level on the thin links;
HYP is three, with the slot order of the dictionaries in gauge.ops.hyp_smear.
Opt-in: QUDA_AMD_NATIVE_LINK_SMEAR=1 or native=True.
"""

from __future__ import annotations

import os

import torch

from ..fields.geometry import LatticeGeometry

PROJ_GS, PROJ_POLAR = 0, 1


def ape_table(spatial_only: bool = False) -> list:
    """APE: slot mu is link mu with the staples of staple_sum, one per
    other direction. ape_smear as it stands keeps the t staples of a
    spatial link under spatial_only (weight alpha / 4 each), so the table
    does too; the t link is a copy row then."""
    table = []
    for mu in range(4):
        row = [mu, 0]
        if not (spatial_only and mu == 3):
            for nu in range(4):
                if nu != mu:
                    row += [nu, mu, nu]
                    row[1] += 1
        table.append(row)
    return table


def hyp_tables() -> tuple:
    """(level 1, level 2, level 3) with the loops and the
    (mu, sorted(nu, rho)) keys of hyp_smear; a slot is a key's position in
    its dictionary's insertion order."""
    t1, bar = [], {}
    for mu in range(4):
        for nu in range(4):
            if nu == mu:
                continue
            for rho in range(nu + 1, 4):
                if rho == mu:
                    continue
                eta = next(d for d in range(4) if d not in (mu, nu, rho))
                bar[(mu, nu, rho)] = len(t1)
                t1.append([mu, 1, eta, mu, eta])
    t2, til = [], {}
    for mu in range(4):
        for nu in range(4):
            if nu == mu:
                continue
            row = [mu, 0]
            for rho in range(4):
                if rho in (mu, nu):
                    continue
                row += [rho, bar[(mu,) + tuple(sorted((nu, rho)))],
                        bar[(rho,) + tuple(sorted((nu, mu)))]]
                row[1] += 1
            til[(mu, nu)] = len(t2)
            t2.append(row)
    t3 = []
    for mu in range(4):
        row = [mu, 0]
        for nu in range(4):
            if nu != mu:
                row += [nu, til[(mu, nu)], til[(nu, mu)]]
                row[1] += 1
        t3.append(row)
    return t1, t2, t3


def smear_level_reference(cen: torch.Tensor, src: torch.Tensor, table,
                          c0: float, c1: float, proj: int,
                          return_cond: bool = False, *,
                          geo: LatticeGeometry):
    """Torch emulation of one level on the kernel's operands (cen
    [4,2,Vcb,3,3], src [Ns,2,Vcb,3,3]; returns [No,2,Vcb,3,3]): the oracle
    of the tables. With return_cond also the conditioning of every
    projected link: for polar the singular values [No,2,Vcb,3] of the
    matrix before projection (descending), for Gram-Schmidt the two norms
    it divides by [No,2,Vcb,2]; ones on copy rows. proj None returns the
    matrices before projection."""
    from ..fields.gauge import project_su3, project_su3_polar
    from ..parallel.halo import shift_lex
    C, S = _lex(cen, geo), _lex(src, geo)
    outs, conds = [], []
    for row in table:
        mu, ns = row[0], row[1]
        if ns == 0:
            outs.append(C[mu])
            conds.append(torch.ones(C[mu].shape[:-2] + (3 if proj else 2,),
                                    dtype=torch.float64, device=cen.device))
            continue
        acc = torch.zeros_like(C[mu])
        for k in range(ns):
            eta, a, b = row[2 + 3 * k: 5 + 3 * k]
            A, B = S[a], S[b]
            fwd = B @ shift_lex(A, geo, eta, +1) @ \
                shift_lex(B, geo, mu, +1).conj().mT
            B_m = shift_lex(B, geo, eta, -1)
            bwd = B_m.conj().mT @ shift_lex(A, geo, eta, -1) @ \
                shift_lex(B_m, geo, mu, +1)
            acc = acc + (fwd + bwd)
        M = c0 * C[mu] + c1 * acc
        if proj is None:
            outs.append(M)
            conds.append(torch.ones(M.shape[:-2] + (3,), dtype=torch.float64,
                                    device=cen.device))
        elif proj == PROJ_POLAR:
            outs.append(project_su3_polar(M))
            conds.append(torch.linalg.svdvals(M))
        else:
            outs.append(project_su3(M))
            r0 = M[..., 0, :]
            n0 = r0.norm(dim=-1)
            r0 = r0 / n0[..., None]
            r1 = M[..., 1, :]
            r1 = r1 - (r0.conj() * r1).sum(-1, keepdim=True) * r0
            conds.append(torch.stack([n0, r1.norm(dim=-1)], dim=-1))
    lo = geo.lex_of_cb.to(cen.device)
    out = torch.stack(outs)
    out = torch.stack([out[:, lo[0]], out[:, lo[1]]], dim=1)
    if not return_cond:
        return out
    cond = torch.stack(conds)
    return out, torch.stack([cond[:, lo[0]], cond[:, lo[1]]], dim=1)


def _lex(f: torch.Tensor, geo: LatticeGeometry) -> torch.Tensor:
    """[n,2,Vcb,3,3] cb -> [n,Vlex,3,3]."""
    lo = geo.lex_of_cb.to(f.device)
    F = torch.empty((f.shape[0], geo.volume, 3, 3), dtype=f.dtype,
                    device=f.device)
    F[:, lo[0]] = f[:, 0]
    F[:, lo[1]] = f[:, 1]
    return F


def ape_coeffs(alpha: float, spatial_only: bool) -> tuple:
    return 1 - alpha, alpha / (4 if spatial_only else 6)


def hyp_coeffs(alpha) -> tuple:
    """((c0, c1) of level 1, 2, 3) for alpha = (a1, a2, a3)."""
    a1, a2, a3 = alpha
    return ((1 - a3, a3 / 2.0), (1 - a2, a2 / 4.0), (1 - a1, a1 / 6.0))


def native_link_smear_default() -> bool:
    """QUDA_AMD_NATIVE_LINK_SMEAR=1 opts into the HIP level kernel
    (default off)."""
    return os.environ.get("QUDA_AMD_NATIVE_LINK_SMEAR", "0") == "1"


def link_smear_eligible(u: torch.Tensor, native=None) -> bool:
    """True when the flag is on (native, or the environment when native is
    None) and u is a [4,2,Vcb,3,3] complex128 GPU tensor of a single-rank
    run. Everything else, an explicit native=True included, takes the
    torch code unchanged."""
    from ..parallel import comms
    on = native_link_smear_default() if native is None else bool(native)
    return bool(on and u.device.type == "cuda"
                and u.dtype == torch.complex128 and u.dim() == 5
                and tuple(u.shape[:2]) == (4, 2)
                and tuple(u.shape[3:]) == (3, 3) and comms.comm_mask() == 0)


def _lat(geo: LatticeGeometry) -> tuple:
    return list(geo.dims), geo.parity_offset, geo.volume_cb


def ape_smear_native(u: torch.Tensor, geo: LatticeGeometry, alpha: float,
                     n_iter: int, spatial_only: bool) -> torch.Tensor:
    """One k_smear_level launch per iteration, ping-pong between two
    buffers; u is not written."""
    from ..ops.dispatch import hip_ext
    ext = hip_ext()
    table = ape_table(spatial_only)
    c0, c1 = ape_coeffs(alpha, spatial_only)
    cur = u.contiguous()
    bufs = [torch.empty_like(cur), torch.empty_like(cur)]
    for it in range(n_iter):
        nxt = bufs[it & 1]
        ext.smear_level(nxt, cur, cur, *_lat(geo), table, c0, c1, PROJ_GS)
        cur = nxt
    return cur if n_iter > 0 else cur.clone()


def hyp_smear_native(u: torch.Tensor, geo: LatticeGeometry, alpha,
                     n_iter: int) -> torch.Tensor:
    """Three k_smear_level launches per iteration; the two slot-major
    scratch fields are allocated once, the result ping-pongs, and nothing
    synchronises with the host inside the loop."""
    from ..ops.dispatch import hip_ext
    ext = hip_ext()
    t1, t2, t3 = hyp_tables()
    k1, k2, k3 = hyp_coeffs(alpha)
    cur = u.contiguous()
    lat = _lat(geo)
    vbar = torch.empty((12,) + cur.shape[1:], dtype=cur.dtype,
                       device=cur.device)
    vtil = torch.empty_like(vbar)
    bufs = [torch.empty_like(cur), torch.empty_like(cur)]
    for it in range(n_iter):
        nxt = bufs[it & 1]
        ext.smear_level(vbar, cur, cur, *lat, t1, *k1, PROJ_POLAR)
        ext.smear_level(vtil, vbar, cur, *lat, t2, *k2, PROJ_POLAR)
        ext.smear_level(nxt, vtil, cur, *lat, t3, *k3, PROJ_POLAR)
        cur = nxt
    return cur if n_iter > 0 else cur.clone()


def over_improved_stout_native(u: torch.Tensor, geo: LatticeGeometry,
                               rho: float, n_iter: int, epsilon: float
                               ) -> torch.Tensor:
    """exp(rho Q) U with Q = 3 TA[U g^dag] from the path-table kernel.
    improved_gauge_force is F = (1/2) TA[U g^dag] = _path_native(scale =
    -beta/6), so Q = 6 F at beta = 1: scale -1."""
    from ..ops.dispatch import hip_ext
    from .ops import _path_native
    ext = hip_ext()
    table = over_improved_table(epsilon)
    cur = u.contiguous()
    lat = _lat(geo)
    for _ in range(n_iter):
        Z = _path_native(cur, geo, table, -1.0, ta=True)
        Z *= rho
        nxt = torch.empty_like(cur)
        for mu in range(4):
            ext.flow_expmul_dir(nxt, cur, Z, *lat, mu)
        cur = nxt
    return cur if n_iter > 0 else cur.clone()


def over_improved_table(epsilon: float):
    """Force table of the over-improved action: plaquettes (5 - 2 eps)/3,
    rectangles -(1 - eps)/12."""
    from .paths import LoopAction, force_table
    c0 = (5.0 - 2.0 * epsilon) / 3.0
    c1 = -(1.0 - epsilon) / 12.0
    loops = LoopAction.symanzik().loops
    return force_table(LoopAction(
        loops, [c0 if len(p) == 4 else c1 for p in loops]))
