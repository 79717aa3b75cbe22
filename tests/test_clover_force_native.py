"""Native Wilson-clover pseudofermion force (csrc/clover_force.hip) against
autograd_fermion_force / wilson_fermion_force evaluated on the CPU in
complex128, from Gaussian X, Y (the force is bilinear in them: no solve).

Force bound per entry, u = 2^-53, n pairs, written before the first GPU run:

    |native - oracle| <= 2 u kappa (n_c m_c + n_h m_h)

Clover part: a term is a chain of five 3x3 factors, four unitary links and
H. A complex 3-term dot costs at most 5 roundings against its modulus
product, so the chain has 25; 24 terms are added; H brings its own 8 n + 4
(n pairs x 4 spins x 2 products, the trace and the symmetrisation); TA and
the scalings 10: n_c = 63 + 8 n. An entry of the modulus product of the
chain is at most the product of the factors' Frobenius norms, sqrt(3)^4 hF
with hF = max_x,plane ||H||_F, and 24 terms carry csw/8:
m_c = 24 (csw/8) 9 hF = 27 csw hF.
Hop part: projection and weight 2 roundings, the 4 n-term outer-product sum
2 + 4 n, U G 5, TA and scalings 10: n_h = 19 + 4 n. |P Y| <= ymax per
entry, so an entry of G is at most 4 n cmax xmax ymax, one of U G at most 3
times that, and there are two such terms: m_h = 24 n cmax xmax ymax.
The factor 2 is there because the autograd oracle rounds too. Nothing here
is tuned to the kernel's output.

Measured on an MI355X, worst fraction of the bound over the three lattices:
csw 0, n 1: 1.6e-3; csw 0, n 3: 4.9e-4; csw 1.3, n 1: 2.2e-4; csw 1.3, n 3:
1.9e-4; end to end from phi: 1.9e-4; the outer product alone against its own
bound: 1.9e-2 (n 1), 6.7e-3 (n 3).
"""

import functools

import numpy as np
import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry
from quda_amd.fields.gamma import sigma_munu
from quda_amd.gauge import fermion_force as ff
from quda_amd.gauge import hmc
from quda_amd.ops import dispatch

U = 2.0 ** -53
KAPPA = 0.115
LATTICES = [(2, 2, 2, 2), (4, 6, 2, 6), (4, 4, 4, 4)]
COEFFS = {1: [1.0], 3: [0.7, -1.1, 0.4]}
PLANES = [(a, b) for a in range(4) for b in range(a + 1, 4)]


@functools.lru_cache(maxsize=None)
def _geo(dims):
    return LatticeGeometry(dims)


@functools.lru_cache(maxsize=None)
def _field(dims, device="cpu"):
    u = GaugeField(_geo(dims), "double").random_su3_(
        seed=2000 + sum(dims)).to_complex()
    return u.to(device).contiguous()


@functools.lru_cache(maxsize=None)
def _pairs(dims, n, device="cpu"):
    g = torch.Generator().manual_seed(77 + sum(dims) + n)
    shape = (2, n, 2, _geo(dims).volume_cb, 4, 3)
    xy = torch.randn(shape, dtype=torch.complex128, generator=g)
    return xy[0].to(device).contiguous(), xy[1].to(device).contiguous()


@functools.lru_cache(maxsize=None)
def _oracle(dims, csw, n):
    """The torch path on the CPU, computed once per case."""
    X, Y = _pairs(dims, n)
    return ff.clover_force_from_solutions(_field(dims), _geo(dims), KAPPA,
                                          csw, X, Y, COEFFS[n], native=False)


def _h_reference(X, Y, coeffs):
    c = torch.tensor(coeffs, dtype=X.dtype, device=X.device)
    sig = torch.tensor(np.array([sigma_munu(a, b) for a, b in PLANES]),
                       dtype=X.dtype, device=X.device)
    O = torch.einsum("n,npvtj,mst,npvsi->mpvji", c, Y, sig, X.conj())
    O = O - torch.diagonal(O, dim1=-2, dim2=-1).sum(-1)[..., None, None] \
        * torch.eye(3, dtype=X.dtype, device=X.device) / 3.0
    return O + O.conj().mT


def force_bound(csw, X, Y, coeffs):
    n = X.shape[0]
    cmax = max(abs(c) for c in coeffs)
    hF = _h_reference(X, Y, coeffs).abs().pow(2).sum((-2, -1)).max().sqrt()
    m_c = 27.0 * abs(csw) * hF.item()
    m_h = 24.0 * n * cmax * X.abs().max().item() * Y.abs().max().item()
    return 2 * U * KAPPA * ((63 + 8 * n) * m_c + (19 + 4 * n) * m_h)


def _no_ext(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the HIP extension must not be touched here")
    monkeypatch.setattr(dispatch, "hip_ext", boom)


def _phi(dims, csw, device):
    from quda_amd.fields.clover import CloverField
    from quda_amd.models import DiracClover
    from quda_amd.ops.reference import clover_matrix
    geo, u = _geo(dims), _field(dims, device)
    g = GaugeField(geo, "double", device).from_complex(u)
    cl = CloverField(geo, "double", device).from_matrices(
        clover_matrix(u, geo, KAPPA, csw))
    return ff.pseudofermion_refresh(DiracClover(g, cl, KAPPA), seed=3)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def test_ineligible_calls_take_the_torch_path(monkeypatch):
    _no_ext(monkeypatch)
    dims = LATTICES[0]
    geo, u = _geo(dims), _field(dims)
    X, Y = _pairs(dims, 3)
    for csw in (0.0, 1.3):
        F = ff.clover_force_from_solutions(u, geo, KAPPA, csw, X, Y,
                                           COEFFS[3], native=True)
        assert torch.equal(F, _oracle(dims, csw, 3))
    # csw = 0 is the einsum force, and one unstacked pair is n = 1
    Fw = sum(c * ff.wilson_fermion_force(u, geo, KAPPA, x, y)
             for c, x, y in zip(COEFFS[3], X, Y))
    assert torch.equal(Fw, _oracle(dims, 0.0, 3))
    P = hmc.random_momentum(geo, seed=4)
    P1 = ff.clover_force_from_solutions(u, geo, KAPPA, 1.3, X[0], Y[0],
                                        mom=P, dt=0.25, native=True)
    F1 = ff.clover_force_from_solutions(u, geo, KAPPA, 1.3, X[:1], Y[:1])
    assert P1 is not P and torch.equal(P1, P + 0.25 * F1)
    phi = _phi(dims, 1.3, "cpu")
    a = ff.clover_fermion_force(u, geo, KAPPA, 1.3, phi, native=True)
    b = ff.clover_fermion_force(u, geo, KAPPA, 1.3, phi, native=False)
    assert a[0] == b[0] and torch.equal(a[1], b[1])
    a = ff.fermion_action_and_force(u, geo, KAPPA, phi, native=True)
    b = ff.fermion_action_and_force(u, geo, KAPPA, phi)
    assert a[0] == b[0] and torch.equal(a[1], b[1])


def test_eligibility_and_flag(monkeypatch):
    from quda_amd.parallel import comms
    _no_ext(monkeypatch)
    dims = LATTICES[0]
    u = _field(dims)
    X, Y = _pairs(dims, 3)
    # a CPU tensor is never eligible; stand in for a GPU one where the
    # device is all that is in the way
    gpu = torch.device("cuda", 0)
    as_gpu = type("T", (torch.Tensor,), {"device": property(lambda s: gpu)})
    ug, Xg, Yg = (t.as_subclass(as_gpu) for t in (u, X, Y))
    assert not ff.clover_force_eligible(u, X, Y, True)
    assert ff.clover_force_eligible(ug, Xg, Yg, True)
    assert not ff.clover_force_eligible(ug.to(torch.complex64), Xg, Yg, True)
    assert not ff.clover_force_eligible(
        ug, Xg.to(torch.complex64).as_subclass(as_gpu), Yg, True)
    assert not ff.clover_force_eligible(ug, Xg[0], Yg[0], True)   # unstacked
    assert not ff.clover_force_eligible(ug, Xg[:2], Yg, True)     # n differs
    assert not ff.clover_force_eligible(ug, Xg[..., :2], Yg[..., :2], True)
    monkeypatch.setattr(comms, "comm_mask", lambda: 1)
    assert not ff.clover_force_eligible(ug, Xg, Yg, True)         # multi-rank
    monkeypatch.setattr(comms, "comm_mask", lambda: 0)
    # the environment counts only when native is None
    monkeypatch.delenv("QUDA_AMD_NATIVE_CLOVER_FORCE", raising=False)
    assert not ff.native_clover_force_default()
    assert not ff.clover_force_eligible(ug, Xg, Yg, None)
    monkeypatch.setenv("QUDA_AMD_NATIVE_CLOVER_FORCE", "1")
    assert ff.native_clover_force_default()
    assert ff.clover_force_eligible(ug, Xg, Yg, None)
    assert not ff.clover_force_eligible(ug, Xg, Yg, False)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_native_sigma_oprod(n):
    dims = LATTICES[1]
    geo, u = _geo(dims), _field(dims, "cuda")
    X, Y = _pairs(dims, n, "cuda")
    H = ff.clover_sigma_oprod(geo, X, Y, COEFFS[n], u)
    ref = _h_reference(*_pairs(dims, n), COEFFS[n])
    # 8 n products and additions per entry, trace and symmetrisation
    scale = sum(abs(c) for c in COEFFS[n]) * (
        X.abs().max() * Y.abs().max()).item()
    bound = 2 * (8 * n + 4) * U * 8 * scale
    err = (H.cpu() - ref).abs().max().item()
    print(f"oprod n={n}: err {err:.3e} bound {bound:.3e} "
          f"fraction {err / bound:.3e}")
    assert err <= bound
    assert torch.equal(H, H.conj().mT)
    tr = torch.diagonal(H, dim1=-2, dim2=-1).sum(-1)
    # three additions, the division and the three subtractions of tr/3
    assert tr.abs().max().item() <= 16 * U * 8 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("csw", [0.0, 1.3])
@pytest.mark.parametrize("dims", LATTICES, ids=str)
def test_native_force_matches_oracle(dims, csw, n):
    geo, u = _geo(dims), _field(dims, "cuda")
    X, Y = _pairs(dims, n, "cuda")
    assert ff.clover_force_eligible(u, X, Y, True)
    F = ff.clover_force_from_solutions(u, geo, KAPPA, csw, X, Y, COEFFS[n],
                                       native=True)
    bound = force_bound(csw, *_pairs(dims, n), COEFFS[n])
    err = (F.cpu() - _oracle(dims, csw, n)).abs().max().item()
    print(f"force {dims} csw={csw} n={n}: err {err:.3e} bound {bound:.3e} "
          f"fraction {err / bound:.3e}")
    assert err <= bound  # csw = 0: the oracle is wilson_fermion_force
    # bitwise repeatable
    assert torch.equal(F, ff.clover_force_from_solutions(
        u, geo, KAPPA, csw, X, Y, COEFFS[n], native=True))


@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES[:2], ids=str)
def test_native_fused_momentum_update(dims):
    geo, u = _geo(dims), _field(dims, "cuda")
    X, Y = _pairs(dims, 3, "cuda")
    dt = 0.37
    F = ff.clover_force_from_solutions(u, geo, KAPPA, 1.3, X, Y, COEFFS[3],
                                       native=True)
    P = hmc.random_momentum(geo, "cuda", seed=11).contiguous()
    mom = P.clone()
    ptr = mom.data_ptr()
    out = ff.clover_force_from_solutions(u, geo, KAPPA, 1.3, X, Y, COEFFS[3],
                                         mom=mom, dt=dt, native=True)
    assert out is mom and mom.data_ptr() == ptr
    # one rounding per component against P + dt F formed in extended
    # precision on the host (2^-10: that precision's own rounding)
    ld = [torch.view_as_real(t.cpu()).numpy().astype(np.longdouble)
          for t in (mom, P, F)]
    d = ld[0] - (ld[1] + np.longdouble(dt) * ld[2])
    err = torch.from_numpy(np.hypot(d[..., 0], d[..., 1]).astype(np.float64))
    tol = (1 + 2.0 ** -10) * U * (P.abs() + dt * F.abs()).cpu()
    assert bool((err <= tol).all())
    assert not torch.equal(mom, P)


@pytest.mark.gpu
def test_native_end_to_end_from_phi():
    dims, csw = LATTICES[2], 1.3
    geo, u = _geo(dims), _field(dims, "cuda")
    phi = _phi(dims, csw, "cuda")
    Sn, Fn = ff.clover_fermion_force(u, geo, KAPPA, csw, phi, native=True)
    St, Ft = ff.clover_fermion_force(u, geo, KAPPA, csw, phi, native=False)
    assert Sn == St
    _, X, Y = ff.clover_solutions(u, geo, KAPPA, csw, phi)
    bound = force_bound(csw, X[None], Y[None], [1.0])
    err = (Fn - Ft).abs().max().item()
    print(f"end to end: err {err:.3e} bound {bound:.3e} "
          f"fraction {err / bound:.3e}")
    assert err <= bound
    assert Fn.abs().max().item() > 1e3 * bound
