"""HIP contraction kernels (csrc/contract.h) under contract_open_spin,
contract_dr, contract_ft and evec_project, against the torch functions with
the flag off, evaluated in complex128 on the CPU on to_complex() of the very
operands the kernels read.

Inputs are read exactly and every sum runs in double, so an output that sums
N products obeys

    |native - ref| <= 2 (N + 16) 2^-53 S

with S the same sum over absolute values (phases have modulus 1, so S does
not depend on the momentum): N = 3 for an open-spin entry, 12 for a gamma
trace, 12 * sites per slice for a slice sum of traces, 3 * sites per slice
for the eigenvector projection. The 16 covers the phase product, the tile
sum and the trace signs, the factor 2 non-fused multiply-adds. The torch path
returns complex128 everywhere, so no term for a final cast. No tolerance here
is tuned to the kernels' output.

Measured on an MI355X, worst fraction of the bound over all cases: double
8.6e-2, single 6.2e-2, half 1.1e-1 (profiles/r12_contract.md).
"""

import functools

import pytest
import torch

from quda_amd import LatticeGeometry, SpinorField
from quda_amd.fields.geometry import checkerboard_join
from quda_amd.ops import contract as ct
from quda_amd.ops import dispatch

# (8, 6, 6, 2): a reduct_dim = 3 slice of 288 sites is three tiles of the
# default 128 (two of 256) with a ragged last one
LATTICES = [(2, 2, 2, 2), (4, 6, 2, 6), (6, 6, 6, 4), (8, 6, 6, 2)]
PRECISIONS = ["double", "single", "half"]
MOMENTA = [[(0, 0, 0, 0)],
           [(1, 0, 0, 0), (-1, 2, 0, 1), (0, -2, 1, 0), (1, 0, 0, 0),
            (2, 1, -1, 3)]]
NE = 8  # QA_CT_NE, eigenvectors per launch


@functools.lru_cache(maxsize=None)
def _field(dims, prec, nspin, seed, device):
    return SpinorField(LatticeGeometry(dims), prec, "cpu",
                       nspin=nspin).gaussian_(seed=seed + sum(dims)).to(device)


@functools.lru_cache(maxsize=None)
def _twin(dims, prec, nspin, seed):
    """The complex128 CPU twin of the GPU field: holds exactly what it
    stores."""
    f = _field(dims, prec, nspin, seed, "cuda")
    return SpinorField(f.geo, "double", nspin=nspin).from_complex(
        f.to_complex().cpu())


def _abs_lex(f):
    return checkerboard_join(f.to_complex(), f.geo).abs()


def _slice_sum(s, geo, rd):
    out = torch.zeros((geo.dims[rd],) + s.shape[1:], dtype=s.dtype)
    return out.index_add_(0, geo.coords[:, rd].to(torch.int64), s)


def check(got, ref, S, N, what):
    """Prints the worst fraction of the bound before asserting it."""
    assert got.shape == ref.shape and got.dtype == ref.dtype
    tol = 2 * (N + 16) * 2.0 ** -53 * S
    frac = ((got.cpu() - ref).abs() / tol).max().item()
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
    x, y = _field(dims, "double", 4, 1, "cpu"), _field(dims, "double", 4, 2, "cpu")
    evs = [_field(dims, "double", 1, 10 + i, "cpu") for i in range(3)]
    outs = [(ct.contract_open_spin(x, y, native=n),
             ct.contract_dr(x, y, native=n),
             ct.contract_ft(x, y, MOMENTA[1], 0, native=n),
             ct.evec_project(evs, x, 3, native=n)) for n in (True, False)]
    for a, b in zip(*outs):
        assert torch.equal(a, b)

    class OnGpu:  # a field as contract_eligible would see it on a GPU
        def __init__(self, f, **kw):
            self.__dict__.update(f.__dict__)
            self.__dict__.update(kw)
            self.device = torch.device("cuda")

    X, Y, E = OnGpu(x), OnGpu(y), [OnGpu(v) for v in evs]
    ok = dispatch.contract_eligible
    assert ok((X, Y), True) and ok((X,), True, 0, E)
    monkeypatch.delenv("QUDA_AMD_NATIVE_CONTRACT", raising=False)
    assert not ok((X, Y), False) and not ok((X, Y), None)
    assert not ok((X, y), True)  # y on the CPU
    assert not ok((X, OnGpu(y, precision="single")), True)
    assert not ok((X, OnGpu(y, precision="quarter")), True)
    assert not ok((OnGpu(x, precision="quarter"),) * 2, True)
    assert not ok((X, OnGpu(y, n_parity=1)), True)
    assert not ok((X, OnGpu(y, ls=4)), True)
    assert not ok((X, OnGpu(y, nspin=1)), True)
    assert not ok((X,), True, 3, [OnGpu(x)])  # nspin-4 "eigenvector"
    assert not ok((X, Y), True, 4) and not ok((X, Y), True, -1)
    monkeypatch.setenv("QUDA_AMD_NATIVE_CONTRACT", "1")
    assert ok((X, Y), None)
    from quda_amd.parallel import comms
    monkeypatch.setattr(comms, "comm_mask", lambda: 1)
    assert not ok((X, Y), True)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["open", "dr"])
@pytest.mark.parametrize("dims", LATTICES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_site(prec, dims, mode):
    x, y = _field(dims, prec, 4, 1, "cuda"), _field(dims, prec, 4, 2, "cuda")
    xd, yd = _twin(dims, prec, 4, 1), _twin(dims, prec, 4, 2)
    S = torch.einsum("vsc,vtc->vst", _abs_lex(xd), _abs_lex(yd))
    if mode == "open":
        check(ct.contract_open_spin(x, y, native=True),
              ct.contract_open_spin(xd, yd, native=False), S, 3, prec)
    else:
        G = ct._gamma_basis("cpu", torch.complex128).abs()
        check(ct.contract_dr(x, y, native=True),
              ct.contract_dr(xd, yd, native=False),
              torch.einsum("gts,vst->vg", G, S), 12, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("momenta", MOMENTA, ids=["zero", "five"])
@pytest.mark.parametrize("rd", [3, 0])
@pytest.mark.parametrize("dims", LATTICES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_slices(prec, dims, rd, momenta):
    x, y = _field(dims, prec, 4, 1, "cuda"), _field(dims, prec, 4, 2, "cuda")
    xd, yd = _twin(dims, prec, 4, 1), _twin(dims, prec, 4, 2)
    S = torch.einsum("gts,vsc,vtc->vg",
                     ct._gamma_basis("cpu", torch.complex128).abs(),
                     _abs_lex(xd), _abs_lex(yd))
    S = _slice_sum(S, xd.geo, rd).unsqueeze(0)
    check(ct.contract_ft(x, y, momenta, rd, native=True),
          ct.contract_ft(xd, yd, momenta, rd, native=False), S,
          12 * xd.geo.volume // dims[rd], prec)


@pytest.mark.gpu
@pytest.mark.parametrize("n_ev", [1, 5, NE + 1])
@pytest.mark.parametrize("rd", [3, 0])
@pytest.mark.parametrize("dims", LATTICES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_evec_project(prec, dims, rd, n_ev):
    psi, pd = _field(dims, prec, 4, 1, "cuda"), _twin(dims, prec, 4, 1)
    evs = [_field(dims, prec, 1, 10 + i, "cuda") for i in range(n_ev)]
    evd = [_twin(dims, prec, 1, 10 + i) for i in range(n_ev)]
    S = torch.stack([_slice_sum(torch.einsum(
        "vc,vsc->vs", _abs_lex(v), _abs_lex(pd)), pd.geo, rd) for v in evd])
    check(ct.evec_project(evs, psi, rd, native=True),
          ct.evec_project(evd, pd, rd, native=False), S,
          3 * pd.geo.volume // dims[rd], prec)


def _single(dims=(8, 6, 6, 2)):
    return (_field(dims, "single", 4, 1, "cuda"),
            _field(dims, "single", 4, 2, "cuda"),
            [_field(dims, "single", 1, 10 + i, "cuda") for i in range(NE + 1)])


@pytest.mark.gpu
def test_reproducible():
    x, y, evs = _single()
    a, b = [(ct.contract_ft(x, y, MOMENTA[1], 3, native=True),
             ct.evec_project(evs, x, 3, native=True)) for _ in range(2)]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_routed(monkeypatch):
    monkeypatch.setattr(dispatch, "_TRACE", True)
    monkeypatch.setattr(dispatch, "_TRACE_LOG", [])
    monkeypatch.delenv("QUDA_AMD_NATIVE_CONTRACT", raising=False)
    x, y, evs = _single()
    ct.contract_dr(x, y, native=False)
    ct.evec_project(evs, x, 3)  # flag unset: torch
    assert dispatch.trace_log() == []
    monkeypatch.setenv("QUDA_AMD_NATIVE_CONTRACT", "1")
    ct.contract_ft(x, y, MOMENTA[1], 3)
    ct.evec_project(evs, x, 3)
    ct.contract_open_spin(x, y)
    ct.contract_dr(x, y)
    assert [op for op, _ in dispatch.trace_log()] == [
        "contract_slices", "evec_project", "contract_site", "contract_site"]
