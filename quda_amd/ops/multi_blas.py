"""Multi-BLAS / multi-reduce: tiled vector-set operations
(ref: lib/multi_blas_quda.cu caxpy(a[NxM],x,y) + lib/multi_reduce_quda.cu
cDotProduct matrices + rotateVecs).

Two paths. The torch path exposes the vector set as ONE complex matrix and
runs the whole tile as a single rocBLAS complex GEMM through torch.matmul.
The HIP path (csrc/multi_blas.h; native=True or
QUDA_AMD_NATIVE_MULTI_BLAS=1, see dispatch.multi_blas_eligible) reads the
fields in place through a pointer table and runs the tiles on the MFMA
units: no stacking, no upcast copy. Half writes, multi-rank runs, mixed
precision and outputs that alias inputs stay on the torch path."""

from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from ..fields.spinor import SpinorField
from ..parallel.comms import allreduce_tensor
from . import dispatch


def _cview(x: SpinorField) -> torch.Tensor:
    """Flat complex view of the native data (no copy; half dequantizes)."""
    if x.precision == "half":
        return x.to_complex().reshape(-1)
    d = x.data
    c = torch.view_as_complex(d.reshape(*d.shape[:-1], d.shape[-1] // 2, 2))
    return c.reshape(-1)


def _disjoint(outs, xs) -> bool:
    """No output shares its storage start with an input."""
    ptrs = {x.data.data_ptr() for x in xs}
    return all(o.data.data_ptr() not in ptrs for o in outs)


def block_cdot(xs: Sequence[SpinorField], ys: Sequence[SpinorField],
               native=None) -> torch.Tensor:
    """G[i,j] = <x_i, y_j> as one complex GEMM (ref cDotProduct NxM)."""
    if dispatch.multi_blas_eligible(list(xs) + list(ys), native):
        return dispatch.multi_cdot(xs, ys)
    X = torch.stack([_cview(x) for x in xs])
    Y = torch.stack([_cview(y) for y in ys])
    if X.dtype == torch.complex64:
        X, Y = X.to(torch.complex128), Y.to(torch.complex128)
    G = X.conj() @ Y.mT if Y.dim() > 1 else None
    G = X.conj() @ Y.transpose(0, 1) if G is None else G
    return allreduce_tensor(G)


def block_caxpy(A, xs: Sequence[SpinorField], ys: Sequence[SpinorField],
                native=None):
    """y_i += sum_j A[i,j] x_j as one complex GEMM (ref caxpy NxM)."""
    if not torch.is_tensor(A):
        A = torch.tensor(np.asarray(A, dtype=complex))
    if (dispatch.multi_blas_eligible(list(xs) + list(ys), native, writes=True)
            and _disjoint(ys, xs)):
        dispatch.multi_caxpy(A, xs, ys)
        return ys
    X = torch.stack([_cview(x) for x in xs])
    A = A.to(device=X.device, dtype=X.dtype if X.is_complex() else torch.complex128)
    if X.dtype == torch.complex64:
        upd = (A.to(torch.complex64) @ X)
    else:
        upd = A @ X
    for i, y in enumerate(ys):
        if y.precision == "half":
            c = y.to_complex().reshape(-1) + upd[i]
            y.from_complex(c.reshape(y.n_parity, y.volume_cb, *y.site_shape))
        else:
            v = _cview(y)
            v += upd[i].to(v.dtype)
    return ys


def block_rotate(V: Sequence[SpinorField], Z, native=None
                 ) -> List[SpinorField]:
    """Vnew_i = sum_j V[j] Z[j,i] in fresh fields, Z [len(V), k] (ref
    rotateVecs): one pass over V per 32 outputs on the HIP path, one GEMM on
    the torch path."""
    if not torch.is_tensor(Z):
        Z = torch.tensor(np.asarray(Z, dtype=complex))
    V = list(V)
    assert Z.shape[0] == len(V), (Z.shape, len(V))
    out = [V[0].clone_empty() for _ in range(Z.shape[1])]
    if dispatch.multi_blas_eligible(V, native, writes=True):
        dispatch.multi_caxpy(Z.mT, V, None, out)
        return out
    X = torch.stack([_cview(v) for v in V])
    new = Z.mT.to(device=X.device, dtype=X.dtype) @ X
    for o, c in zip(out, new):
        if o.precision == "half":
            o.from_complex(c.reshape(o.n_parity, o.volume_cb, *o.site_shape))
        else:
            _cview(o).copy_(c)
    return out
