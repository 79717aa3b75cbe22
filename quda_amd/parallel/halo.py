"""Halo (ghost-zone) exchange engine (ref: lib/dslash_policy.hpp +
include/kernels/dslash_pack.cuh + lattice_field.cpp createComms — rebuilt
MI355X-first: spin-projected face buffers packed by HIP kernels, exchanged
with torch.distributed point-to-point ops — RCCL send/recv over xGMI on a
GPU node, gloo for CPU multi-process tests; self-wraparound when a
partitioned dim has grid size 1, which exercises the full comms code path
on a single process exactly like the reference's --partition flags).

Buffer/key conventions (mirror csrc/halo.h):
  key (mu, dir): dir=1 ghost arrives from the +mu neighbor (feeds the
  forward hop), dir=0 from -mu (backward hop). send[(mu,0)] is packed from
  the x_mu=0 face and travels to the -mu neighbor; send[(mu,1)] from the
  x_mu=L-1 face to +mu.

Deterministic op ordering: every rank issues its isend/irecv ops sorted by
(mu, travel-direction) where travel=0 is the +mu-going message
(send[(mu,1)] on the sender, recv (mu,0)... on the receiver recv[(mu,0)]
arrives from -mu, i.e. it is the +mu-going message) — this keeps NCCL's
per-peer order-based matching consistent even when the +mu and -mu
neighbor are the same rank (grid extent 2).
"""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist

from ..fields.geometry import LatticeGeometry
from . import comms

Key = Tuple[int, int]  # (mu, dir)


def active_dims(mask: int) -> List[int]:
    return [mu for mu in range(4) if (mask >> mu) & 1]


def _travel_key(mu: int, travel: int, extra: int = 0):
    return (mu, travel, extra)


def exchange_tensors(sends: Dict[Key, torch.Tensor],
                     recvs: Dict[Key, torch.Tensor]) -> None:
    """Blocking exchange (see exchange_tensors_start)."""
    for r in exchange_tensors_start(sends, recvs):
        r.wait()


def exchange_tensors_start(sends: Dict[Key, torch.Tensor],
                           recvs: Dict[Key, torch.Tensor]) -> list:
    """Start exchanging face tensors: recv[(mu,1)] <- +mu neighbor's
    send[(mu,0)], recv[(mu,0)] <- -mu neighbor's send[(mu,1)]. Complex
    tensors are viewed as real. Returns the request list; self-wraparound
    copies run immediately (stream-ordered). wait() on each request before
    touching recv buffers (on NCCL that makes the CURRENT stream wait — the
    host does not block, so an interior kernel launched in between overlaps
    with the transfer)."""
    ops = []  # (order_key, is_send, tensor, peer)
    # self-wraparound check must use the GLOBAL rank: neighbor_rank returns
    # global ranks, and inside a split-grid sub-communicator comm_rank() is
    # group-local
    my_rank = dist.get_rank() if comms.is_distributed() else 0
    local_copies = []
    for (mu, d), s in sends.items():
        peer = comms.neighbor_rank(mu, -1 if d == 0 else +1)
        # send (mu,0) goes -mu => it is the "-mu-going" message: travel=1
        travel = 1 if d == 0 else 0
        if peer == my_rank:
            # self-wraparound: recv[(mu, 1-d)] = send[(mu, d)]
            local_copies.append(((mu, 1 - d), s))
            continue
        ops.append((_travel_key(mu, travel, 0), True, s, peer))
    for (mu, d), r in recvs.items():
        peer = comms.neighbor_rank(mu, -1 if d == 0 else +1)
        if peer == my_rank:
            continue
        # recv (mu,0) arrives from -mu travelling +mu: travel=0
        travel = 0 if d == 0 else 1
        ops.append((_travel_key(mu, travel, 1), False, r, peer))
    for key, s in local_copies:
        recvs[key].copy_(s)
    if not ops:
        return []
    ops.sort(key=lambda o: (o[0], not o[1]))  # sends before recvs per key
    reqs = []
    for _, is_send, t, peer in ops:
        tt = torch.view_as_real(t) if t.is_complex() else t
        if is_send:
            reqs.append(dist.isend(tt.contiguous(), peer))
        else:
            assert tt.is_contiguous()
            reqs.append(dist.irecv(tt, peer))
    return reqs


# ---------------------------------------------------------------------------
# native (device-layout) spinor halo: persistent buffers + HIP pack kernels
# ---------------------------------------------------------------------------

GHOST_W0 = {"double": 2, "single": 4, "half": 4, "quarter": 4}  # max reals per ghost chunk


def ghost_width(ncomp: int, precision: str) -> int:
    """Mirrors csrc/halo.h GhostAcc<> chunk width."""
    w = GHOST_W0[precision]
    while ncomp % w:
        w //= 2
    return w


class SpinorHalo:
    """Persistent send/recv ghost buffers for one (geometry, precision,
    device, mask, ncomp, depth, n_slab) signature (role of the reference's
    static ghost arenas, lattice_field.h:250). ncomp = 12 (spin-projected
    Wilson) or 6 (staggered full site); depth = ghost layers (3 for the
    staggered Naik term).

    Per (mu, dir) one contiguous tensor [ncomp/gw, depth*Fcb, gw], norms
    [depth*Fcb]. With n_slab (the Ls slices of a 5-d field, or the sides of
    a multi-RHS batch) both gain a leading slab dimension: every slab packs
    into its own slice and the whole buffer still ships as ONE message per
    (mu, dir) (ref: create_comms_batch, dslash_wilson.hpp:48). The multi-RHS
    kernels offset into the slab from the slice they are handed
    (csrc/halo.h load_r), so this layout is load-bearing."""

    def __init__(self, geo: LatticeGeometry, precision: str, device,
                 mask: int, ncomp: int = 12, depth: int = 1,
                 n_slab: Optional[int] = None):
        from ..fields.layout import DTYPE_OF
        self.geo = geo
        self.precision = precision
        self.mask = mask
        self.ncomp = ncomp
        self.depth = depth
        self.n_slab = n_slab
        self.device = torch.device(device)
        self.dtype = DTYPE_OF[precision]
        self.send: Dict[Key, torch.Tensor] = {}
        self.recv: Dict[Key, torch.Tensor] = {}
        self.send_nrm: Dict[Key, torch.Tensor] = {}
        self.recv_nrm: Dict[Key, torch.Tensor] = {}
        gw = ghost_width(ncomp, precision)
        lead = () if n_slab is None else (n_slab,)
        for mu in active_dims(mask):
            fcb = geo.face_volume_cb(mu) * depth
            for key in ((mu, 0), (mu, 1)):
                for bufs, nrms in ((self.send, self.send_nrm),
                                   (self.recv, self.recv_nrm)):
                    bufs[key] = torch.empty(lead + (ncomp // gw, fcb, gw),
                                            dtype=self.dtype, device=device)
                    if precision in ("half", "quarter"):
                        nrms[key] = torch.empty(lead + (fcb,),
                                                dtype=torch.float32,
                                                device=device)

    def faces(self, dagger: bool):
        """(key, s01, edge, fcb) of every face to pack: send[(mu, d)] is the
        x_mu = 0 (d = 0) or X-1 (d = 1) face, with the projector sign the
        consuming hop applies."""
        for mu in active_dims(self.mask):
            fcb = self.geo.face_volume_cb(mu)
            for d in (0, 1):
                yield (mu, d), d ^ (1 if dagger else 0), d, fcb

    def _pack_face(self, ext, dst, dst_nrm, inp, parity: int, mu: int,
                   s01: int, edge: int, fcb: int, v_stride: int,
                   s_offset: int) -> None:
        from ..ops.dispatch import norm_or_empty
        geo = self.geo
        if self.ncomp == 6:  # staggered ghosts carry the full site
            ext.pack_face_stag(dst, dst_nrm, inp.data, norm_or_empty(inp),
                               list(geo.dims), geo.parity_offset,
                               geo.volume_cb, parity, mu, edge, fcb,
                               self.depth)
        else:
            ext.pack_face(dst, dst_nrm, inp.data, norm_or_empty(inp),
                          list(geo.dims), geo.parity_offset, geo.volume_cb,
                          parity, mu, s01, edge, fcb, v_stride=v_stride,
                          s_offset=s_offset)

    def _slot(self, bufs, nrms, key: Key, slab: Optional[int]):
        """(buffer, norm) of one face, or of one slab of it."""
        from ..ops.dispatch import empty_tensor
        b, n = bufs.get(key), nrms.get(key)
        if b is None:  # dim not partitioned
            b = empty_tensor(self.dtype, self.device)
        elif slab is not None:
            b = b[slab]
        if n is None:  # no norms at this precision, or dim not partitioned
            n = empty_tensor(torch.float32, self.device)
        elif slab is not None:
            n = n[slab]
        return b, n

    def pack(self, ext, inp, parity: int, dagger: bool,
             slab: Optional[int] = None, v_stride: int = 0,
             s_offset: int = 0) -> None:
        """Pack all active faces of `inp` (the dslash input, at `parity`)
        into the send buffers, or into their slice `slab`. v_stride /
        s_offset address one 4-d slice of a 5-d input."""
        for key, s01, edge, fcb in self.faces(dagger):
            dst, dst_nrm = self._slot(self.send, self.send_nrm, key, slab)
            self._pack_face(ext, dst, dst_nrm, inp, parity, key[0], s01, edge,
                            fcb, v_stride, s_offset)

    def exchange(self) -> None:
        for r in self.exchange_start():
            r.wait()

    def exchange_start(self) -> list:
        reqs = exchange_tensors_start(self.send, self.recv)
        if self.recv_nrm:
            reqs += exchange_tensors_start(self.send_nrm, self.recv_nrm)
        return reqs

    def ghost_args(self, slab: Optional[int] = None):
        """(ghost[8], ghost_nrm[8], face_cb[4]) lists for ext.dslash_*: the
        recv buffers, or their slice `slab`."""
        slots = [self._slot(self.recv, self.recv_nrm, (mu, d), slab)
                 for mu in range(4) for d in (0, 1)]
        face_cb = [self.geo.face_volume_cb(mu) for mu in range(4)]
        return [b for b, _ in slots], [n for _, n in slots], face_cb


_HALO_CACHE: Dict[tuple, SpinorHalo] = {}


def get_spinor_halo(geo: LatticeGeometry, precision: str, device,
                    mask: int, ncomp: int = 12, depth: int = 1,
                    n_slab: Optional[int] = None) -> SpinorHalo:
    """The cached halo of this signature; the key holds everything the
    object depends on (the pack reads geo.dims and geo.parity_offset)."""
    key = (geo.dims, geo.parity_offset, precision, str(device), mask, ncomp,
           depth, n_slab)
    h = _HALO_CACHE.get(key)
    if h is None:
        h = SpinorHalo(geo, precision, device, mask, ncomp, depth, n_slab)
        _HALO_CACHE[key] = h
    return h


# ---------------------------------------------------------------------------
# oracle (complex-layout) halo for the CPU reference path
# ---------------------------------------------------------------------------

def exchange_psi_oracle(psi: torch.Tensor, geo: LatticeGeometry,
                        parity_in: int, mask: int,
                        depth: int = 1) -> Dict[Key, torch.Tensor]:
    """Exchange full (unprojected) spinor faces of `psi` ([V_cb,4,3] or
    [V_cb,3] complex at parity_in). Returns {(mu,dir): faces} in
    ghost-index order; with depth > 1 each face is [depth, Fcb, ...] where
    layer l of (mu,1) holds the +mu neighbor's x_mu = l sites and layer l
    of (mu,0) the -mu neighbor's x_mu = X-1-l sites (Naik nFace=3)."""
    sends, recvs = {}, {}
    for mu in active_dims(mask):
        hi = geo.dims[mu] - 1
        lo_layers = [psi[geo.face_index_cb(parity_in, mu, l)]
                     for l in range(depth)]
        hi_layers = [psi[geo.face_index_cb(parity_in, mu, hi - l)]
                     for l in range(depth)]
        sends[(mu, 0)] = torch.stack(lo_layers).contiguous()
        sends[(mu, 1)] = torch.stack(hi_layers).contiguous()
        recvs[(mu, 0)] = torch.empty_like(sends[(mu, 1)])
        recvs[(mu, 1)] = torch.empty_like(sends[(mu, 0)])
    exchange_tensors(sends, recvs)
    if depth == 1:
        recvs = {k: v[0] for k, v in recvs.items()}
    return recvs


def exchange_psi5_oracle(psi5: torch.Tensor, geo: LatticeGeometry,
                         parity_in: int, mask: int, ls: int):
    """Oracle 5-d spinor face exchange: psi5 [Ls*V,4,3] -> ghosts
    {(mu,dir): [Ls, Fcb, 4, 3]}."""
    V = geo.volume_cb
    v = psi5.reshape(ls, V, 4, 3)
    sends, recvs = {}, {}
    for mu in active_dims(mask):
        hi = geo.dims[mu] - 1
        idx0 = geo.face_index_cb(parity_in, mu, 0).to(psi5.device)
        idx1 = geo.face_index_cb(parity_in, mu, hi).to(psi5.device)
        sends[(mu, 0)] = v[:, idx0].contiguous()
        sends[(mu, 1)] = v[:, idx1].contiguous()
        recvs[(mu, 0)] = torch.empty_like(sends[(mu, 1)])
        recvs[(mu, 1)] = torch.empty_like(sends[(mu, 0)])
    exchange_tensors(sends, recvs)
    return recvs


# ---------------------------------------------------------------------------
# distributed lexicographic-field shift (gauge-sector halo: staples, field
# strength, smearing, forces become multi-rank correct through this)
# ---------------------------------------------------------------------------

def shift_lex(f: torch.Tensor, geo: LatticeGeometry, mu: int, disp: int
              ) -> torch.Tensor:
    """f: [Vlex, ...] -> f(x + disp*mu). |disp| must be 1 (compose for
    more). On partitioned dims the wrapped face comes from the neighbor
    rank (ref: the gauge exchangeGhost/exchangeExtendedGhost role)."""
    assert disp in (1, -1)
    from . import comms
    idx = geo.neighbor_lex(mu, disp).to(f.device)
    out = f[idx]
    if not ((comms.comm_mask() >> mu) & 1):
        return out
    hi = geo.dims[mu] - 1
    if disp == 1:
        # my x_mu = hi sites need the +mu neighbor's x_mu = 0 slab
        send = {(mu, 0): f[_face_lex(geo, mu, 0).to(f.device)].contiguous()}
        recv = {(mu, 1): torch.empty_like(send[(mu, 0)])}
        exchange_tensors(send, recv)
        out[_face_lex(geo, mu, hi).to(f.device)] = recv[(mu, 1)]
    else:
        send = {(mu, 1): f[_face_lex(geo, mu, hi).to(f.device)].contiguous()}
        recv = {(mu, 0): torch.empty_like(send[(mu, 1)])}
        exchange_tensors(send, recv)
        out[_face_lex(geo, mu, 0).to(f.device)] = recv[(mu, 0)]
    return out


def _face_lex(geo: LatticeGeometry, mu: int, edge: int) -> torch.Tensor:
    """Lex indices of the face x_mu == edge, in natural lex order (both
    ends agree: transverse coords are identical across the boundary)."""
    key = ("face_lex", mu, edge)
    cache = geo.__dict__.setdefault("_nbr_cache", {})
    if key not in cache:
        c = geo.coords[:, mu]
        cache[key] = (c == edge).nonzero(as_tuple=True)[0].contiguous()
    return cache[key]
