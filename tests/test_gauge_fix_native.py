"""Overrelaxed gauge fixing: the torch oracle ovr_half_sweep_reference, the
native option of gauge_fix_ovr, and the HIP kernels of csrc/gauge_fix.hip
against that oracle.

Half-sweep bound, per entry of a link owned by site x (u = 2^-53):

    |kernel - reference| <= C(omega) u (4 dirs / k_min(x)),
    C(omega) = 2 [3 ((5 omega - 4) S + B + N) + R] = 188 at 1.0, 356 at 1.7

k_min(x) is the smallest of the three subgroup norms sqrt(a0^2 + asq) of the
reference at x. Each of (a0..a3) is a sum over 2 dirs links of numbers of
modulus <= 1, so its rounding error is at most S u 2 dirs with S = 8
additions (the reference adds 2 dirs - 1 matrices in sequence and one pair of
entries; the kernel one pair and three butterfly steps), and the error of the
4-vector at most twice that: S u 4 dirs, a relative S u 4 dirs / k. The map
a -> r has Lipschitz constant (5 omega - 4) / k for omega >= 1: omega from
the scaling by xb <= omega, 4 (omega - 1) from d xb = (omega - 1) d(a0^2/k^2)
with |d(a0^2/k^2)| <= 4 |da| / k, and the normalisation (a projection on the
unit sphere, its denominator >= k) adds nothing. B = 10 roundings form xb
and xb a (three squares, two sums, a product, two sums, a quotient, a
product), N = 6 the norm and the quotient (a square, a product, a sum, a
root, the floor, a quotient); they act on numbers of size k and are counted
with the same factor 4 dirs / k >= 2. That is one hit; there are three. R = 22
covers the three row updates of a link entry, 5 roundings each against a
modulus product of at most sqrt 2 (the reference's g and g U cost no more).
The factor 2 is there because both sides round. The bound is of first order
in each hit's own rounding, the shape the hit's conditioning gives; it is
not tuned to the kernel's output.

reunit = 1 is compared with project_su3 of the reunit = 0 reference under
the same bound plus 2 x 30 u for the Gram-Schmidt roundings (two norms of 8,
a 3-term dot of 5, the subtraction 3, the cross product 4, rounded up).

Quality: Delta_ij sums 2 dirs numbers of modulus <= 1 and loses at most
d = 2 dirs (2 dirs + 4) u; by Cauchy-Schwarz sum 2 |Delta| d <= 2 d
sqrt(3/theta) relative to sum |Delta|^2 = 3 V theta, and the sum of 9 V
non-negative squares adds (9 V + 3) u: relative bound 2 [(9 V + 3) u + 2 d
sqrt(3 / theta)], both sides rounding. The functional is a mean of numbers
of modulus <= 1: absolute bound 2 (3 dirs V + 2) u.

Measured on an MI355X, worst fraction of the bound over all cases:
half-sweep 1.6e-2 (warm; hot 3.6e-3), reunit 1.1e-2, theta 3.1e-3.
"""

import functools

import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry
from quda_amd.fields.gauge import project_su3
from quda_amd.gauge import plaquette
from quda_amd.gauge.fix import (_su3_maximize, gauge_fix_ovr,
                                gauge_fix_quality, ovr_half_sweep_reference)
from quda_amd.ops import dispatch

U = 2.0 ** -53
LATTICES = [(2, 2, 2, 2), (4, 6, 2, 6), (6, 6, 2, 2)]
EYE = torch.eye(3, dtype=torch.complex128)


@functools.lru_cache(maxsize=None)
def _geo(dims):
    return LatticeGeometry(dims)


@functools.lru_cache(maxsize=None)
def _field(dims, kind):
    """hot: random SU(3); warm: the same pulled towards the identity;
    smooth: near the identity, then a random gauge transformation."""
    geo = _geo(dims)
    hot = GaugeField(geo, "double").random_su3_(
        seed=500 + sum(dims)).to_complex().contiguous()
    if kind == "hot":
        return hot
    if kind == "warm":
        return project_su3(EYE + 0.2 * (hot - EYE)).contiguous()
    u = project_su3(EYE + 0.1 * (hot - EYE))
    g = GaugeField(geo, "double").random_su3_(seed=77).to_complex()[0]
    for mu in range(4):
        for p in (0, 1):
            fwd = geo.neighbor_cb(p, mu, +1)
            u[mu, p] = g[p] @ u[mu, p] @ g[1 - p][fwd].conj().mT
    return u.contiguous()


@functools.lru_cache(maxsize=None)
def _ref(dims, kind, parity, dirs, omega):
    """(reference half-sweep, per-entry bound [4,2,Vcb,1,1]), on the CPU."""
    geo = _geo(dims)
    out, kmin = ovr_half_sweep_reference(_field(dims, kind), geo, parity,
                                         dirs, omega, return_norms=True)
    kl = torch.empty((4, 2, geo.volume_cb), dtype=torch.float64)
    kl[:, parity] = kmin
    for mu in range(4):
        kl[mu, 1 - parity, geo.neighbor_cb(parity, mu, -1)] = kmin
    c = 2 * (3 * ((5 * omega - 4) * 8 + 10 + 6) + 22)
    return out, (c * U * 4 * dirs / kl)[..., None, None]


def _lat(dims):
    geo = _geo(dims)
    return list(dims), geo.parity_offset, geo.volume_cb


def _no_ext(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the HIP extension must not be touched here")
    monkeypatch.setattr(dispatch, "hip_ext", boom)


# CPU

@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("dirs", [3, 4])
def test_reference_at_omega_one_is_the_maximising_hit(dims, parity, dirs):
    geo, u = _geo(dims), _field(dims, "hot")
    back = [geo.neighbor_cb(parity, mu, -1) for mu in range(4)]
    w = sum(u[mu, parity] + u[mu, 1 - parity][back[mu]].conj().mT
            for mu in range(dirs))
    g = _su3_maximize(w, hits=1)
    want = u.clone()
    for mu in range(4):
        want[mu, parity] = g @ u[mu, parity]
        want[mu, 1 - parity, back[mu]] = (u[mu, 1 - parity][back[mu]]
                                          @ g.conj().mT)
    got = ovr_half_sweep_reference(u, geo, parity, dirs, 1.0)
    assert (got - want).abs().max().item() <= 16 * U


@pytest.mark.parametrize("gauge,dirs", [("landau", 4), ("coulomb", 3)])
def test_native_option_on_cpu_converges(monkeypatch, gauge, dirs):
    _no_ext(monkeypatch)
    dims = (4, 4, 4, 4)
    geo, u = _geo(dims), _field(dims, "smooth")
    uf = gauge_fix_ovr(u, geo, gauge=gauge, max_iter=400, tol=1e-9,
                       native=True, check_every=5)
    assert gauge_fix_quality(uf, geo, dirs)[1] < 1e-9
    assert gauge_fix_quality(uf, geo, dirs)[0] > gauge_fix_quality(
        u, geo, dirs)[0]
    assert (uf @ uf.conj().mT - EYE).abs().max().item() < 1e-14
    assert abs(plaquette(uf, geo)[0] - plaquette(u, geo)[0]) < 1e-12


def test_native_off_is_the_call_without_the_keyword(monkeypatch):
    monkeypatch.delenv("QUDA_AMD_NATIVE_GAUGE_FIX", raising=False)
    _no_ext(monkeypatch)
    dims = LATTICES[1]
    geo, u = _geo(dims), _field(dims, "warm")
    a = gauge_fix_ovr(u, geo, max_iter=2, tol=1e-30)
    assert torch.equal(a, gauge_fix_ovr(u, geo, max_iter=2, tol=1e-30,
                                        native=False))
    assert torch.equal(a, gauge_fix_ovr(u, geo, max_iter=2, tol=1e-30,
                                        native=None, omega=1.2))
    monkeypatch.setenv("QUDA_AMD_NATIVE_GAUGE_FIX", "1")
    b = gauge_fix_ovr(u, geo, max_iter=2, tol=1e-30, native=None)
    assert torch.equal(b, gauge_fix_ovr(u, geo, max_iter=2, tol=1e-30,
                                        native=True))
    assert not torch.equal(a, b)


# GPU

@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("dirs", [3, 4])
@pytest.mark.parametrize("omega", [1.0, 1.7])
@pytest.mark.parametrize("kind", ["hot", "warm"])
def test_half_sweep_kernel_matches_reference(kind, omega, dirs, parity, dims):
    ext = dispatch.hip_ext()
    ref, bound = _ref(dims, kind, parity, dirs, omega)
    u = _field(dims, kind).cuda()
    ext.gauge_fix_ovr_half(u, *_lat(dims), parity, dirs, omega, False)
    frac = ((u.cpu() - ref).abs() / bound).max().item()
    print(f"half-sweep {dims} {kind} p{parity} d{dirs} w{omega}: "
          f"fraction {frac:.3e}")
    assert frac <= 1.0
    # reunit = 1: Gram-Schmidt of the same result
    v = _field(dims, kind).cuda()
    ext.gauge_fix_ovr_half(v, *_lat(dims), parity, dirs, omega, True)
    v = v.cpu()
    frac = ((v - project_su3(ref)).abs() / (bound + 60 * U)).max().item()
    print(f"  reunit: fraction {frac:.3e}")
    assert frac <= 1.0
    assert (v @ v.conj().mT - EYE).abs().max().item() < 1e-14


@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("dirs", [3, 4])
@pytest.mark.parametrize("kind", ["hot", "warm"])
def test_quality_kernel_matches_torch(kind, dirs, dims):
    geo, u = _geo(dims), _field(dims, kind)
    func, theta = gauge_fix_quality(u, geo, dirs)
    part = dispatch.hip_ext().gauge_fix_quality(u.cuda(), *_lat(dims), dirs)
    assert tuple(part.shape) == ((geo.volume + 255) // 256, 2)
    s = part.sum(0).cpu()
    V = geo.volume
    d = 2 * dirs * (2 * dirs + 4) * U
    rel = 2 * ((9 * V + 3) * U + 2 * d * (3.0 / theta) ** 0.5)
    err = abs(s[0].item() / (3 * V) - theta) / theta
    print(f"quality {dims} {kind} d{dirs}: theta fraction {err / rel:.3e}")
    assert err <= rel
    assert abs(s[1].item() / (3 * V * dirs) - func) <= 2 * (3 * dirs * V
                                                            + 2) * U


@pytest.mark.gpu
@pytest.mark.parametrize("gauge,dirs", [("landau", 4), ("coulomb", 3)])
def test_native_option_on_gpu(monkeypatch, gauge, dirs):
    dims = (4, 4, 4, 4)
    geo, u = _geo(dims), _field(dims, "smooth").cuda()
    kw = dict(gauge=gauge, max_iter=400, tol=1e-9, native=True)
    uf = gauge_fix_ovr(u, geo, check_every=5, **kw)
    assert torch.equal(u, _field(dims, "smooth").cuda())  # input untouched
    assert gauge_fix_quality(uf, geo, dirs)[1] < 1e-9
    assert abs(plaquette(uf, geo)[0] - plaquette(u, geo)[0]) < 1e-12
    assert (uf @ uf.conj().mT - EYE.cuda()).abs().max().item() < 1e-14
    assert torch.equal(uf, gauge_fix_ovr(u, geo, check_every=5, **kw))
    # an ineligible field takes the torch engine
    _no_ext(monkeypatch)
    u32 = gauge_fix_ovr(u.to(torch.complex64), geo, gauge=gauge, max_iter=2,
                        native=True)
    assert u32.dtype == torch.complex64 and u32.is_cuda
