"""Contractions, stochastic sources and LAPH-style projections
(ref: lib/contract.cu + kernels/contraction.cuh contractQuda/contractFTQuda,
lib/evec_project.cu, kernels/spinor_noise.cuh / spinor_dilute.cuh —
re-derived; einsum/batched-GEMM shaped, torch dispatches to rocBLAS)."""

from __future__ import annotations

import functools
from typing import List, Optional

import numpy as np
import torch

from ..fields.gamma import GAMMA, GAMMA5
from ..fields.geometry import LatticeGeometry, checkerboard_join
from ..fields.spinor import SpinorField


def contract_open_spin(x: SpinorField, y: SpinorField,
                       native=None) -> torch.Tensor:
    """Open-spin color-contracted bilinear per site:
    C[x, s, s'] = sum_c conj(x(s,c)) y(s',c)  ->  [V, 4, 4] (lex order)
    (ref: contractQuda QUDA_CONTRACT_TYPE_OPEN). native (None: the
    QUDA_AMD_NATIVE_CONTRACT switch) asks for the HIP kernels of
    csrc/contract.h, here and below, where dispatch.contract_eligible
    holds; every other call runs the torch code."""
    from . import dispatch
    if dispatch.contract_eligible((x, y), native):
        return dispatch.contract_site(x, y, gamma_table(), False).view(
            -1, 4, 4)
    geo = x.geo
    xc = checkerboard_join(x.to_complex(), geo)
    yc = checkerboard_join(y.to_complex(), geo)
    return torch.einsum("vsc,vtc->vst", xc.conj(), yc)


def contract_dr(x: SpinorField, y: SpinorField, native=None) -> torch.Tensor:
    """Gamma-insertion contraction: tr_spin[ G_i^dag X^dag G_i Y ] summed
    over color, for the 16 DeGrand-Rossi gamma-basis elements
    -> [V, 16] (ref: QUDA_CONTRACT_TYPE_DR)."""
    from . import dispatch
    if dispatch.contract_eligible((x, y), native):
        return dispatch.contract_site(x, y, gamma_table(), True)
    C = contract_open_spin(x, y, native=False)  # [V,4,4]
    dev, dt = C.device, C.dtype
    gammas = _gamma_basis(dev, dt)
    # tr[ G^d C^T_spin? ] — standard: sum_{s,s'} G[s',s] C[s,s']
    return torch.einsum("gts,vst->vg", gammas, C)


def _gamma_basis(device, dtype):
    """16-element gamma basis: 1, g1..g4, g5, g5 g_mu, sigma_munu-like
    products (ordered: I, g1, g2, g3, g4, g5, g5g1..g5g4, g1g2,...)."""
    mats = [np.eye(4)]
    mats += [GAMMA[mu] for mu in range(4)]
    mats += [GAMMA5]
    mats += [GAMMA5 @ GAMMA[mu] for mu in range(4)]
    for mu in range(4):
        for nu in range(mu + 1, 4):
            mats.append(GAMMA[mu] @ GAMMA[nu])
    return torch.tensor(np.stack(mats), device=device, dtype=dtype)


@functools.lru_cache(maxsize=None)
def gamma_table() -> tuple:
    """The 16 matrices of _gamma_basis as the table the HIP kernels take:
    word g holds, in nibble t, col | k << 2 of the one non-zero entry i^k of
    row t of G_g, so that D[g] = sum_t i^k C[col, t]. Raises if a matrix is
    not monomial with entries in {1, i, -1, -i}."""
    units = [1, 1j, -1, -1j]
    words = []
    for g, G in enumerate(_gamma_basis("cpu", torch.complex128).numpy()):
        w = 0
        for t in range(4):
            cols = np.flatnonzero(G[t])
            if len(cols) != 1 or G[t, cols[0]] not in units:
                raise ValueError(f"gamma basis element {g} is not monomial "
                                 f"with unit entries: row {t} = {G[t]}")
            w |= (int(cols[0]) | units.index(G[t, cols[0]]) << 2) << (4 * t)
        words.append(w)
    return tuple(words)


def phase_table(dims, momenta, reduct_dim: int) -> torch.Tensor:
    """The separable factors of e^{-i p.x}, CPU complex128 [n_mom, sum of the
    extents other than reduct_dim]: for each momentum the rows
    exp(-i 2 pi p_d x_d / L_d), x_d = 0..L_d-1, of the dimensions
    d != reduct_dim in ascending order."""
    rows = []
    for p in momenta:
        rows.append(torch.cat([
            torch.exp(-1j * (2 * np.pi * p[d]
                             * torch.arange(dims[d], dtype=torch.float64)
                             / dims[d]))
            for d in range(4) if d != reduct_dim]))
    return torch.stack(rows).to(torch.complex128).contiguous()


def contract_ft(x: SpinorField, y: SpinorField, momenta: List[tuple],
                reduct_dim: int = 3, native=None) -> torch.Tensor:
    """Momentum-projected timeslice contraction (ref: contractFTQuda):
    C[p, t, g] = sum_{vec x} e^{-i p.x} tr[...] -> [n_mom, T, 16]."""
    from . import dispatch
    if len(momenta) and dispatch.contract_eligible((x, y), native, reduct_dim):
        from ..parallel.comms import allreduce_tensor
        return allreduce_tensor(dispatch.contract_slices(
            x, y, gamma_table(),
            phase_table(x.geo.dims, momenta, reduct_dim), reduct_dim))
    geo = x.geo
    c = contract_dr(x, y, native=False)  # [V, 16] lex
    coords = geo.coords.to(torch.float64)
    dims = geo.dims
    out = torch.empty((len(momenta), dims[reduct_dim], 16),
                      dtype=c.dtype, device=c.device)
    tcoord = geo.coords[:, reduct_dim].to(torch.int64)
    for ip, p in enumerate(momenta):
        phase_arg = sum(2 * np.pi * p[i] * coords[:, i] / dims[i]
                        for i in range(4) if i != reduct_dim)
        ph = torch.exp(-1j * phase_arg).to(c.dtype)
        w = c * ph.unsqueeze(-1)
        slab = torch.zeros((dims[reduct_dim], 16), dtype=c.dtype,
                           device=c.device)
        slab.index_add_(0, tcoord, w)
        out[ip] = slab
    from ..parallel.comms import allreduce_tensor
    return allreduce_tensor(out)


def evec_project(evecs: List[SpinorField], psi: SpinorField,
                 reduct_dim: int = 3, native=None) -> torch.Tensor:
    """LapH sink projection <evec_i | psi> per timeslice and spin
    -> [n_ev, T, 4] (ref: lib/evec_project.cu; evecs are nspin=1 laplace
    eigenvectors, psi a 4-spin propagator field)."""
    from . import dispatch
    if len(evecs) and dispatch.contract_eligible((psi,), native, reduct_dim,
                                                 evecs):
        from ..parallel.comms import allreduce_tensor
        return allreduce_tensor(dispatch.evec_project_slices(
            evecs, psi, reduct_dim))
    geo = psi.geo
    T = geo.dims[reduct_dim]
    tcoord = geo.coords[:, reduct_dim].to(torch.int64)
    pc = checkerboard_join(psi.to_complex(), geo)  # [V,4,3]
    out = torch.empty((len(evecs), T, 4), dtype=pc.dtype, device=pc.device)
    for i, v in enumerate(evecs):
        vc = checkerboard_join(v.to_complex(), geo)  # [V,3]
        w = torch.einsum("vc,vsc->vs", vc.conj(), pc)
        slab = torch.zeros((T, 4), dtype=pc.dtype, device=pc.device)
        slab.index_add_(0, tcoord.to(pc.device), w)
        out[i] = slab
    from ..parallel.comms import allreduce_tensor
    return allreduce_tensor(out)


# -- stochastic sources (ref: spinor_noise.cuh / spinor_dilute.cuh) ---------

def z4_noise(f: SpinorField, seed: int) -> SpinorField:
    """Z4 noise {±1, ±i}/1 per component."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 4, (f.n_parity, f.volume_cb, *f.site_shape),
                      generator=g)
    vals = torch.tensor([1 + 0j, -1 + 0j, 1j, -1j], dtype=torch.complex128)
    f.from_complex(vals[k].to(f.device))
    return f


def gaussian_noise(f: SpinorField, seed: int) -> SpinorField:
    return f.gaussian_(seed=seed)


def dilute(src: SpinorField, scheme: str = "spin") -> List[SpinorField]:
    """Split a source into orthogonal dilution components
    (ref: spinor_dilute.cuh; schemes: spin, color, even-odd,
    time-slice)."""
    geo = src.geo
    c = src.to_complex()
    out = []
    if scheme == "spin":
        for s in range(src.nspin):
            f = src.clone_empty()
            cc = torch.zeros_like(c)
            if src.nspin > 1:
                cc[:, :, s, :] = c[:, :, s, :]
            else:
                cc = c.clone()
            f.from_complex(cc)
            out.append(f)
    elif scheme == "color":
        for col in range(3):
            f = src.clone_empty()
            cc = torch.zeros_like(c)
            cc[..., col] = c[..., col]
            f.from_complex(cc)
            out.append(f)
    elif scheme == "even-odd":
        assert src.n_parity == 2
        for p in (0, 1):
            f = src.clone_empty()
            cc = torch.zeros_like(c)
            cc[p] = c[p]
            f.from_complex(cc)
            out.append(f)
    elif scheme == "time":
        tcoord = geo.coords[:, 3].to(torch.int64)
        from ..fields.geometry import checkerboard_split
        tc = torch.stack([tcoord[geo.lex_of_cb[0]],
                          tcoord[geo.lex_of_cb[1]]])  # [2, Vcb]
        if src.ls > 1:
            tc = tc.repeat(1, src.ls)
        for t in range(geo.dims[3]):
            f = src.clone_empty()
            cc = torch.zeros_like(c)
            m = (tc == t)
            cc[m] = c[m]
            f.from_complex(cc)
            out.append(f)
    else:
        raise ValueError(scheme)
    return out


def sequential_source(prop_col: SpinorField, t_sink: int,
                      gamma: str = "g5") -> SpinorField:
    """Sequential source for 3-point functions (ref: the sequential-
    propagator workflow the reference's covdev/contract kernels serve):
    restrict one propagator column to the sink timeslice and hit it with
    the sink gamma (g5 for the pion)."""
    import torch
    geo = prop_col.geo
    c = prop_col.to_complex().clone()
    tcoord = geo.coords[:, 3].to(torch.int64)
    tc = torch.stack([tcoord[geo.lex_of_cb[0]], tcoord[geo.lex_of_cb[1]]])
    mask = (tc == t_sink).unsqueeze(-1).unsqueeze(-1)
    c = torch.where(mask, c, torch.zeros_like(c))
    if gamma == "g5":
        c[..., 2:4, :] = -c[..., 2:4, :]
    else:
        raise ValueError(gamma)
    out = prop_col.clone_empty()
    out.from_complex(c)
    return out
