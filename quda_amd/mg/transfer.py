"""Multigrid transfer operators (ref: lib/transfer.cpp +
kernels/block_orthogonalize.cuh, restrictor.cuh, prolongator.cuh —
re-derived MI355X-first: aggregation is einsum/batched-GEMM shaped, which
torch dispatches to rocBLAS on the GPU).

Aggregates: geometric blocks of the fine lattice x 2 chiral halves
(DeGrand-Rossi g5 = diag(1,1,-1,-1): chirality 0 = spins 0,1).
Coarse dof per site: Ns_c=2 (chirality) x Nvec "colors".

The fine<->coarse map works on the ORACLE layout [2, Vcb, 4, 3] flattened
to lex [V, 4, 3]; fine fields enter/leave as SpinorFields.
"""

from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch

from ..fields.geometry import LatticeGeometry, checkerboard_join, checkerboard_split
from ..fields.spinor import SpinorField
from ..ops import blas


_NATIVE_PRECISIONS = {"double": torch.complex128, "single": torch.complex64}


def native_transfer_default() -> bool:
    """QUDA_AMD_MG_NATIVE_TRANSFER=1 opts into the HIP transfer kernels
    (csrc/transfer.hip); off by default."""
    return os.environ.get("QUDA_AMD_MG_NATIVE_TRANSFER", "0") == "1"


def transfer_tables(geo: LatticeGeometry, block) -> Tuple[torch.Tensor,
                                                          torch.Tensor]:
    """Index tables of the native transfer kernels, on the CPU:
    agg_of_site [2*Vcb] int32, the aggregate of fine site g = parity*Vcb + x,
    and site_tab [Na, B] int32, the fine site of (a, b) in the (a, b) order
    of Transfer.sites_by_agg (so Transfer.V stays the one source of truth)."""
    cd = tuple(geo.dims[i] // block[i] for i in range(4))
    c = geo.coords.to(torch.int64)
    bc = [c[:, i] // block[i] for i in range(4)]
    agg_of_lex = ((bc[3] * cd[2] + bc[2]) * cd[1] + bc[1]) * cd[0] + bc[0]
    n_agg = cd[0] * cd[1] * cd[2] * cd[3]
    sites_by_agg = torch.argsort(agg_of_lex, stable=True).reshape(n_agg, -1)
    # fine site index of every lex site
    g_of_lex = geo.parity.to(torch.int64) * geo.volume_cb + geo.cb_of_lex
    site_tab = g_of_lex[sites_by_agg]
    agg_of_site = torch.empty(geo.volume, dtype=torch.int64)
    agg_of_site[g_of_lex] = agg_of_lex
    return agg_of_site.to(torch.int32), site_tab.to(torch.int32).contiguous()


def pack_vn(V: torch.Tensor, site_tab: torch.Tensor, geo: LatticeGeometry,
            dtype=None) -> torch.Tensor:
    """Aggregate-ordered V [Na, B, 4, 3, Nv] -> the site-fastest copy
    Vn [2 (chirality), 6 (spin-in-chirality x color), Nv, 2*Vcb] the prolong
    kernel reads: consecutive fine sites are consecutive in memory."""
    Na, B, _, _, Nv = V.shape
    G = geo.volume
    assert Na * B == G, (V.shape, G)
    Vg = torch.empty((G, 12, Nv), dtype=dtype or V.dtype, device=V.device)
    Vg[site_tab.reshape(-1).long().to(V.device)] = \
        V.reshape(G, 12, Nv).to(Vg.dtype)
    return Vg.reshape(G, 2, 6, Nv).permute(1, 2, 3, 0).contiguous()


class Transfer:
    """Prolongator/restrictor over geometric blocks + chiral blocking.

    native=True (or QUDA_AMD_MG_NATIVE_TRANSFER=1 when native is None)
    routes restrict, prolong and the block-orthonormalization through the
    HIP kernels of csrc/transfer.hip where they apply — GPU, nspin=4, ls=1,
    full-parity double/single fields, B*6 >= Nvec — and leaves every other
    input on the torch path. `native_active` tells which one was set up."""

    def __init__(self, geo: LatticeGeometry, block: Tuple[int, int, int, int],
                 vectors: List[SpinorField], native: Optional[bool] = None):
        self.geo = geo
        self.block = tuple(block)
        for i in range(4):
            assert geo.dims[i] % block[i] == 0, (geo.dims, block)
        self.coarse_dims = tuple(geo.dims[i] // block[i] for i in range(4))
        self.nvec = len(vectors)
        self.device = vectors[0].device
        self.precision = vectors[0].precision
        # aggregate index of every fine lex site
        cd = self.coarse_dims
        c = geo.coords.to(torch.int64)
        bc = [c[:, i] // block[i] for i in range(4)]
        self.agg_of_lex = (((bc[3] * cd[2] + bc[2]) * cd[1] + bc[1]) * cd[0]
                           + bc[0]).to(self.device)  # [V]
        self.n_agg = cd[0] * cd[1] * cd[2] * cd[3]
        self.block_vol = geo.volume // self.n_agg
        # site order within aggregates: argsort by aggregate
        order = torch.argsort(self.agg_of_lex, stable=True)
        self.sites_by_agg = order.reshape(self.n_agg, self.block_vol)  # [Na, B]
        self.native = native_transfer_default() if native is None \
            else bool(native)
        self.native_active = (self.native
                              and self.block_vol * 6 >= self.nvec
                              and self._field_native_ok(vectors[0]))
        # V tensor: [Na, B, 4, 3, Nvec] from block-orthonormalized vectors
        if self.native_active:
            agg_of_site, site_tab = transfer_tables(geo, self.block)
            self.agg_of_site = agg_of_site.to(self.device)
            self.site_tab = site_tab.to(self.device)
        self.V = block_orthonormalize(self._pack(vectors),
                                      native=self.native_active)

    # V is the single source of truth: the copies the kernels read (the
    # site-fastest Vn, the complex64 aggregate-ordered one) are derived from
    # it and dropped whenever it is assigned, so R and P cannot disagree.
    # (Writing INTO the tensor in place is not seen; assign a new one.)
    @property
    def V(self) -> torch.Tensor:
        return self._V

    @V.setter
    def V(self, value: torch.Tensor) -> None:
        self._V = value
        self._vn = {}
        self._va = {}
        if self.native_active:
            self._get_vn(self.precision)

    @staticmethod
    def _field_native_ok(f: SpinorField) -> bool:
        return (f.device.type == "cuda" and f.nspin == 4 and f.ls == 1
                and f.n_parity == 2 and f.precision in _NATIVE_PRECISIONS)

    def _get_va(self, precision: str) -> torch.Tensor:
        """Aggregate-ordered V in the complex type of `precision` (the
        restrict kernel's operand; self.V itself for double fields)."""
        dtype = _NATIVE_PRECISIONS[precision]
        if self.V.dtype == dtype and self.V.is_contiguous():
            return self.V
        va = self._va.get(precision)
        if va is None:
            va = self.V.to(dtype).contiguous()
            self._va[precision] = va
        return va

    def _get_vn(self, precision: str) -> torch.Tensor:
        """Site-fastest copy of V in the complex type of `precision`."""
        vn = self._vn.get(precision)
        if vn is None:
            vn = pack_vn(self.V, self.site_tab, self.geo,
                         dtype=_NATIVE_PRECISIONS[precision])
            self._vn[precision] = vn
        return vn

    def _pack(self, vectors: List[SpinorField]) -> torch.Tensor:
        vs = []
        for v in vectors:
            lex = checkerboard_join(v.to_complex(), self.geo)  # [V,4,3]
            vs.append(lex[self.sites_by_agg])                  # [Na,B,4,3]
        return torch.stack(vs, dim=-1)  # [Na,B,4,3,Nvec]

    # -- fine -> coarse -----------------------------------------------------
    def restrict(self, fine: SpinorField) -> torch.Tensor:
        """[Na, 2, Nvec] complex coarse vector: c[a,chi,v] =
        sum_{x in a, s in chi} conj(V[a,x,s,c,v]) psi(x,s,c)."""
        if self.native_active and self._field_native_ok(fine):
            from ..ops import dispatch
            out = dispatch.transfer_restrict(
                fine, self._get_va(fine.precision), self.site_tab)
            return out.to(torch.complex128)
        lex = checkerboard_join(fine.to_complex(), self.geo)[self.sites_by_agg]
        return self.restrict_lex(lex)

    def restrict_lex(self, lex: torch.Tensor) -> torch.Tensor:
        out = torch.empty((self.n_agg, 2, self.nvec), dtype=lex.dtype,
                          device=lex.device)
        for chi, sl in ((0, slice(0, 2)), (1, slice(2, 4))):
            out[:, chi, :] = torch.einsum("abscv,absc->av",
                                          self.V[:, :, sl].conj(), lex[:, :, sl])
        return out

    # -- coarse -> fine -----------------------------------------------------
    def prolong_lex(self, coarse: torch.Tensor) -> torch.Tensor:
        """[Na,2,Nvec] -> aggregate-ordered fine [Na,B,4,3]."""
        out = torch.zeros((self.n_agg, self.block_vol, 4, 3),
                          dtype=coarse.dtype, device=coarse.device)
        for chi, sl in ((0, slice(0, 2)), (1, slice(2, 4))):
            out[:, :, sl] = torch.einsum("abscv,av->absc", self.V[:, :, sl],
                                         coarse[:, chi, :])
        return out

    def prolong(self, coarse: torch.Tensor, out: SpinorField) -> SpinorField:
        if self.native_active and self._field_native_ok(out):
            from ..ops import dispatch
            vn = self._get_vn(out.precision)
            c = coarse.reshape(self.n_agg, 2, self.nvec).to(vn.dtype)
            return dispatch.transfer_prolong(out, c.contiguous(), vn,
                                             self.agg_of_site)
        lex_a = self.prolong_lex(coarse)
        V = self.geo.volume
        lex = torch.empty((V, 4, 3), dtype=lex_a.dtype, device=lex_a.device)
        lex[self.sites_by_agg.reshape(-1)] = lex_a.reshape(V, 4, 3)
        out.from_complex(checkerboard_split(lex, self.geo))
        return out


def block_orthonormalize(V: torch.Tensor, passes: int = 2,
                         native: bool = False) -> torch.Tensor:
    """Per-(aggregate, chirality) modified Gram-Schmidt of the Nvec columns
    (ref: kernels/block_orthogonalize.cuh, 2-pass). native=True runs the
    same algorithm in one HIP kernel where it applies (a complex128 GPU
    tensor with B*6 >= Nvec); every other input takes the torch loop."""
    Na, B, _, _, Nv = V.shape
    if (native and V.device.type == "cuda" and V.dtype == torch.complex128
            and B * 6 >= Nv):
        from ..ops import dispatch
        return dispatch.transfer_block_ortho(V.clone().contiguous(), passes)
    out = V.clone()
    for chi, sl in ((0, slice(0, 2)), (1, slice(2, 4))):
        W = out[:, :, sl].reshape(Na, B * 6, Nv).clone()
        for _ in range(passes):
            for j in range(Nv):
                for i in range(j):
                    c = torch.einsum("ab,ab->a", W[:, :, i].conj(), W[:, :, j])
                    W[:, :, j] -= c.unsqueeze(-1) * W[:, :, i]
                nrm = W[:, :, j].norm(dim=-1, keepdim=True).clamp_min(1e-30)
                W[:, :, j] = W[:, :, j] / nrm
        out[:, :, sl] = W.reshape(Na, B, 2, 3, Nv)
    return out


def generate_null_vectors(op, n_vec: int, *, tol: float = 5e-5,
                          maxiter: int = 500, seed: int = 500,
                          precision: str = "double") -> List[SpinorField]:
    """Smooth random vectors against the fine operator: approximately solve
    MdagM x = 0 from a random start (ref: multigrid.cpp:71
    generateNullVectors — BiCGStab/CG on random sources)."""
    from ..solvers import cg_solve
    vecs = []
    for k in range(n_vec):
        x = op.new_spinor(precision, n_parity=2)
        x.gaussian_(seed=seed + k)
        # inverse-iteration smoothing: solve MdagM y = x loosely
        y = op.new_spinor(precision, n_parity=2)
        cg_solve(op, y, x, tol=tol, maxiter=maxiter)
        vecs.append(y)
    return vecs
