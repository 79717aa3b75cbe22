"""HIP multi-BLAS kernels (csrc/multi_blas.h) under block_cdot, block_caxpy,
block_rotate and trlm_solve, against complex128 arithmetic on the CPU on
to_complex() of the very operands the kernels read.

multi_cdot reads its inputs exactly (half as double(norm) * double(stored))
and multiplies and adds in double, so for L complex elements per vector and
any summation order

    |G_ij - ref| <= 2 (L + 16) 2^-53 S_ij,   S_ij = sum_e |x_i[e]| |y_j[e]|

(L terms in a sum, the factor 2 for the two real products behind each part of
a complex product, 16 for the tile and block sums).

multi_caxpy computes in the storage type with unit roundoff u (2^-53 double,
2^-24 single) from A as rounded to that type: a chain of 2 M fused
multiply-adds per real part, so

    |out_i[e] - ref| <= 2 (M + 16) u (beta |y_i[e]| + sum_j |A_ij| |x_j[e]|)

where the 16 covers the second launch of a split input set, which rounds the
partial result once more. No tolerance here is tuned to the kernels' output.

Measured on an MI355X, worst fraction of the bound over all cases: cdot
double 2.9e-2, single 2.3e-2, half 2.3e-2; caxpy double 9.8e-2, single
7.5e-2 (profiles/r13_multi_blas.md).
"""

import functools

import numpy as np
import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField
from quda_amd.ops import dispatch
from quda_amd.ops.multi_blas import block_caxpy, block_cdot, block_rotate

# flat lengths: a fraction of one segment, ragged last segments, several
# segments; on one lattice also nspin 1, a parity view and a 5-d field
FIELDS = [((2, 2, 2, 2), "s4"), ((4, 6, 2, 6), "s4"), ((6, 6, 6, 4), "s4"),
          ((4, 6, 2, 6), "s1"), ((4, 6, 2, 6), "par"), ((4, 6, 2, 6), "ls4")]
UNIT = {"double": 2.0 ** -53, "single": 2.0 ** -24}


@functools.lru_cache(maxsize=None)
def _cpu(dims, kind, prec, seed):
    geo = LatticeGeometry(dims)
    f = SpinorField(geo, prec, "cpu", nspin=1 if kind == "s1" else 4,
                    n_parity=1 if kind == "ls4" else 2,
                    ls=4 if kind == "ls4" else 1).gaussian_(seed=seed + sum(dims))
    return f.parity_view(1) if kind == "par" else f


def _gpu(dims, kind, prec, seed):
    """A fresh GPU copy (a parity view stays a view of a full field)."""
    f = _cpu(dims, "s4" if kind == "par" else kind, prec, seed).to("cuda")
    return f.parity_view(1) if kind == "par" else f


@functools.lru_cache(maxsize=None)
def _flat(dims, kind, prec, seed):
    """What the field stores, as flat complex128."""
    return _cpu(dims, kind, prec, seed).to_complex().reshape(-1)


def check(got, ref, S, n, u, what):
    """Prints the worst fraction of the bound before asserting it."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol = 2 * (n + 16) * u * S
    frac = ((got.cpu().to(torch.complex128) - ref).abs() / tol).max().item()
    print(f"fraction of bound [{what}]: {frac:.3e}")
    assert frac <= 1.0, frac


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def test_cpu_flag_is_inert(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the HIP extension must not be touched here")
    monkeypatch.setattr(dispatch, "hip_ext", boom)
    dims = (4, 6, 2, 6)
    xs = [_cpu(dims, "s4", "double", i) for i in range(3)]
    A = torch.randn(2, 3, dtype=torch.complex128,
                    generator=torch.Generator().manual_seed(5))
    outs = []
    for n in (True, False):
        ys = [SpinorField(LatticeGeometry(dims), "double").copy_(
            _cpu(dims, "s4", "double", 50 + i)) for i in range(2)]
        outs.append([block_cdot(xs, ys, native=n)]
                    + [y.data for y in block_caxpy(A, xs, ys, native=n)]
                    + [v.data for v in block_rotate(xs, A.mT, native=n)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)

    class OnGpu:  # a field as multi_blas_eligible would see it on a GPU
        def __init__(self, f, **kw):
            self.__dict__.update(f.__dict__)
            self.__dict__.update(kw)
            self.device = torch.device("cuda")

    x, y = xs[0], xs[1]
    X, Y = OnGpu(x), OnGpu(y)
    ok = dispatch.multi_blas_eligible
    assert ok((X, Y), True) and ok((X, Y), True, writes=True)
    monkeypatch.delenv("QUDA_AMD_NATIVE_MULTI_BLAS", raising=False)
    assert not ok((X, Y), False) and not ok((X, Y), None)
    assert not ok((X, y), True)  # y on the CPU
    assert not ok((X, OnGpu(y, precision="single")), True)
    assert not ok((OnGpu(x, precision="quarter"),) * 2, True)
    H = OnGpu(_cpu(dims, "s4", "half", 1))
    assert ok((H, H), True) and not ok((H, H), True, writes=True)
    assert not ok((X, OnGpu(_cpu(dims, "s1", "double", 1))), True)  # shapes
    monkeypatch.setenv("QUDA_AMD_NATIVE_MULTI_BLAS", "1")
    assert ok((X, Y), None)
    from quda_amd.parallel import comms
    monkeypatch.setattr(comms, "comm_mask", lambda: 1)
    assert not ok((X, Y), True)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nm", [(1, 1), (5, 3), (16, 16), (17, 2), (33, 40),
                                "same"])
@pytest.mark.parametrize("dims,kind", FIELDS)
@pytest.mark.parametrize("prec", ["double", "single", "half"])
def test_cdot(prec, dims, kind, nm):
    N, M = (33, 33) if nm == "same" else nm
    xs = [_gpu(dims, kind, prec, i) for i in range(N)]
    X = torch.stack([_flat(dims, kind, prec, i) for i in range(N)])
    if nm == "same":
        ys, Y = xs, X
    else:
        ys = [_gpu(dims, kind, prec, 100 + j) for j in range(M)]
        Y = torch.stack([_flat(dims, kind, prec, 100 + j) for j in range(M)])
    G = block_cdot(xs, ys, native=True)
    assert G.dtype == torch.complex128
    check(G, X.conj() @ Y.mT, X.abs() @ Y.abs().mT, X.shape[1], 2.0 ** -53,
          f"cdot {prec}")
    if nm == "same":
        assert torch.equal(G, G.conj().mT)


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [1, 0])
@pytest.mark.parametrize("nm", [(1, 1), (3, 5), (16, 16), (2, 17), (20, 70)])
@pytest.mark.parametrize("dims,kind", FIELDS)
@pytest.mark.parametrize("prec", ["double", "single"])
def test_caxpy(prec, dims, kind, nm, beta):
    N, M = nm
    ctype = torch.complex128 if prec == "double" else torch.complex64
    A = torch.randn(N, M, dtype=torch.complex128,
                    generator=torch.Generator().manual_seed(N + M))
    Ac = A.to(ctype).to(torch.complex128)
    xs = [_gpu(dims, kind, prec, i) for i in range(M)]
    X = torch.stack([_flat(dims, kind, prec, i) for i in range(M)])
    ref, S = Ac @ X, Ac.abs() @ X.abs()
    if beta:  # the block caxpy, in place
        out = block_caxpy(A, xs, [_gpu(dims, kind, prec, 100 + i)
                                  for i in range(N)], native=True)
        Y = torch.stack([_flat(dims, kind, prec, 100 + i) for i in range(N)])
        ref, S = ref + Y, S + Y.abs()
    else:  # the basis rotation Vnew = V Z
        out = block_rotate(xs, A.mT, native=True)
    got = torch.stack([o.to_complex().reshape(-1) for o in out])
    check(got, ref, S, M, UNIT[prec], f"caxpy {prec} beta={beta}")
    for i, x in enumerate(xs):
        assert torch.equal(x.data.cpu(), _cpu(dims, kind, prec, i).data)


@pytest.mark.gpu
def test_reproducible():
    xs = [_gpu((6, 6, 6, 4), "s4", "single", i) for i in range(17)]
    ys = [_gpu((6, 6, 6, 4), "s4", "single", 100 + i) for i in range(17)]
    assert torch.equal(block_cdot(xs, ys, native=True),
                       block_cdot(xs, ys, native=True))


@pytest.mark.gpu
def test_routed(monkeypatch):
    monkeypatch.setattr(dispatch, "_TRACE", True)
    monkeypatch.setattr(dispatch, "_TRACE_LOG", [])
    monkeypatch.delenv("QUDA_AMD_NATIVE_MULTI_BLAS", raising=False)
    dims, A = (4, 6, 2, 6), torch.ones(2, 3, dtype=torch.complex128)

    def run(prec):
        xs = [_gpu(dims, "s4", prec, i) for i in range(3)]
        ys = [_gpu(dims, "s4", prec, 100 + i) for i in range(2)]
        block_cdot(xs, ys)
        block_caxpy(A, xs, ys)
        block_rotate(xs, A.mT)
        return ys

    run("double")  # flag unset: torch
    assert dispatch.trace_log() == []
    monkeypatch.setenv("QUDA_AMD_NATIVE_MULTI_BLAS", "1")
    run("double")
    assert [op for op, _ in dispatch.trace_log()] == [
        "multi_cdot", "multi_caxpy", "multi_caxpy"]
    dispatch.trace_log().clear()
    ys = run("half")  # half writes stay on torch
    assert [op for op, _ in dispatch.trace_log()] == ["multi_cdot"]
    monkeypatch.delenv("QUDA_AMD_NATIVE_MULTI_BLAS")
    for a, b in zip(ys, run("half")):
        assert torch.equal(a.data, b.data) and torch.equal(a.norm, b.norm)


@pytest.mark.gpu
def test_trlm(monkeypatch):
    from quda_amd.models import DiracWilsonPC
    from quda_amd.solvers.eigen import trlm_solve
    monkeypatch.setattr(dispatch, "_TRACE", True)
    monkeypatch.setattr(dispatch, "_TRACE_LOG", [])
    geo = LatticeGeometry((4, 4, 4, 4))
    g = GaugeField(geo, "double").random_su3_(seed=91)
    x0 = SpinorField(geo, "double", n_parity=1).gaussian_(seed=7)
    res = {}
    for dev, flag in (("cuda", "1"), ("cpu", "0")):
        monkeypatch.setenv("QUDA_AMD_NATIVE_MULTI_BLAS", flag)
        res[dev] = trlm_solve(DiracWilsonPC(g.to(dev), 0.1), n_ev=4, n_kr=16,
                              x0=x0.to(dev), tol=1e-8, max_restarts=200)
        assert res[dev].converged
    ops = {op for op, _ in dispatch.trace_log()}
    assert {"multi_cdot", "multi_caxpy"} <= ops
    a, b = res["cuda"], res["cpu"]
    order_a, order_b = np.argsort(a.evals), np.argsort(b.evals)
    for i, j in zip(order_a, order_b):
        print(f"lambda {a.evals[i]:.12e} {b.evals[j]:.12e} "
              f"resid {a.residuals[i]:.2e} {b.residuals[j]:.2e}")
        assert abs(a.evals[i] - b.evals[j]) <= a.residuals[i] + b.residuals[j]
