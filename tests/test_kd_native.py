"""HIP Kahler-Dirac kernels (csrc/kd.hip) under KDBlockInverse and the KD
operators, against today's torch build in complex128 on the CPU, applied to
to_complex() of the very field the kernel reads.

Bound per block, 2-norm over its 48 entries, every quantity on the right taken
from the reference alone (kappa = cond of the reference block X):

    ||native - ref|| <= C (u_build kappa^2 + u_tab kappa) ||ref||

u_build = 2^-53 (the build is double: normal matrix, Cholesky, inverse of the
factor, products), u_tab = 2^-53 for double and 2^-24 for single and half (the
table type, which is also the accumulation type), C = 100: about 4n for the
factor-invert-multiply chain at n = 24 plus the 48-term complex dots. Applying
X itself drops the kappa factors. Half adds its output block-float rounding
per entry, 2^-10 |ref entry| + 2^-23 max_site |ref|, as a 2-norm over the
block. No tolerance here is tuned to the kernel's output.

Measured on an MI355X, worst fraction of the bound over all cases (X / X^-1):
double 1.3e-2 / 1.2e-2, single 2.2e-2 / 9.6e-3, half 1.7e-1 / 1.7e-1.
"""

import functools

import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField
from quda_amd.models.staggered_kd import DiracStaggeredKD, KDBlockInverse
from quda_amd.ops import dispatch

U_TAB = {"double": 2.0 ** -53, "single": 2.0 ** -24, "half": 2.0 ** -24}
U_BUILD, C = 2.0 ** -53, 100.0
LATTICES = [(2, 2, 2, 2), (6, 2, 2, 2), (4, 6, 2, 4), (4, 4, 4, 6)]


@functools.lru_cache(maxsize=None)
def _geo(dims, parity_offset=0):
    return LatticeGeometry(dims, parity_offset=parity_offset)


@functools.lru_cache(maxsize=None)
def _links(dims, fat, parity_offset=0):
    u = GaugeField(_geo(dims, parity_offset), "double").random_su3_(
        seed=5 + sum(dims)).to_complex()
    if fat:  # non-unitary, fat-like
        gen = torch.Generator().manual_seed(17 + sum(dims))
        u = u + 0.2 * torch.view_as_complex(
            torch.randn(*u.shape, 2, dtype=torch.float64, generator=gen))
    return u


@functools.lru_cache(maxsize=None)
def _ref(dims, fat, mass, parity_offset=0):
    """Today's torch build on the CPU, and kappa of every block."""
    kd = KDBlockInverse(_links(dims, fat, parity_offset),
                        _geo(dims, parity_offset), mass, native=False)
    return kd, torch.linalg.cond(kd.X)


def _field(dims, prec, parity_offset=0, seed=3):
    return SpinorField(_geo(dims, parity_offset), prec, "cpu",
                       nspin=1).gaussian_(seed=seed + sum(dims)).to("cuda")


def check(kd_ref, kappa, got, ref, prec, kind):
    """got, ref: [nblk, 48] complex128 CPU; prints the worst fraction of the
    bound before asserting it."""
    amp = U_BUILD * kappa ** 2 + U_TAB[prec] * kappa if kind == 1 \
        else torch.full_like(kappa, U_BUILD + U_TAB[prec])
    tol = C * amp * ref.norm(dim=1)
    if prec == "half":
        site_max = torch.view_as_real(ref.reshape(-1, 16, 3)).abs().flatten(
            2).amax(-1, keepdim=True)
        e = 2.0 ** -10 * ref.reshape(-1, 16, 3).abs() + 2.0 ** -23 * site_max
        tol = tol + e.reshape(-1, 48).norm(dim=1)
    frac = ((got - ref).norm(dim=1) / tol).max().item()
    print(f"fraction of bound [{prec}/kind{kind}]: {frac:.3e}")
    assert frac <= 1.0, frac


def _run(dims, prec, kind, dagger, fat, mass, parity_offset=0):
    kd_ref, kappa = _ref(dims, fat, mass, parity_offset)
    kd = KDBlockInverse(_links(dims, fat, parity_offset).cuda(),
                        _geo(dims, parity_offset), mass, native=True)
    psi = _field(dims, prec, parity_offset)
    out = psi.clone_empty()
    dispatch.trace_log().clear()
    (kd.apply if kind else kd.apply_X)(out, psi, dagger=dagger)
    assert kd._X is None and kd._Xinv is None  # no torch build ran
    M = kd_ref.Xinv if kind else kd_ref.X
    M = M.conj().mT if dagger else M
    ref = torch.einsum("bij,bj->bi", M,
                       kd_ref._to_blocks(psi.to_complex().cpu()))
    check(kd_ref, kappa, kd_ref._to_blocks(out.to_complex().cpu()), ref, prec,
          kind)


@pytest.mark.gpu
@pytest.mark.parametrize("mass", [0.05, 0.5])
@pytest.mark.parametrize("fat", [False, True])
@pytest.mark.parametrize("dagger", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("prec", ["double", "single", "half"])
@pytest.mark.parametrize("dims", LATTICES)
def test_kd_apply(dims, prec, kind, dagger, fat, mass, monkeypatch):
    monkeypatch.setattr(dispatch, "_TRACE", True)
    _run(dims, prec, kind, dagger, fat, mass)
    assert [op for op, _ in dispatch.trace_log()] == ["kd_build", "kd_apply"]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "half"])
@pytest.mark.parametrize("kind", [0, 1])
def test_kd_parity_offset(kind, prec):
    _run((4, 6, 2, 4), prec, kind, False, True, 0.05, parity_offset=1)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("mass", [0.05, 0.5])
def test_kd_round_trip(mass, prec):
    dims = (4, 4, 4, 6)
    kd_ref, kappa = _ref(dims, True, mass)
    kd = KDBlockInverse(_links(dims, True).cuda(), _geo(dims), mass,
                        native=True)
    psi = _field(dims, prec)
    t, back = psi.clone_empty(), psi.clone_empty()
    kd.apply(back, kd.apply_X(t, psi))
    check(kd_ref, kappa, kd_ref._to_blocks(back.to_complex().cpu()),
          kd_ref._to_blocks(psi.to_complex().cpu()), prec, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("dagger", [False, True])
def test_kd_operator_m(dagger):
    dims, mass = (4, 4, 4, 6), 0.05
    g = GaugeField(_geo(dims), "double").random_su3_(seed=9).to("cuda")
    v = _field(dims, "double", seed=4)
    ops = [DiracStaggeredKD(g, mass, native=flag) for flag in (True, False)]
    got, ref = (op.M(v.clone_empty(), v, dagger=dagger).to_complex().cpu()
                for op in ops)
    kd_ref = ops[1].kd
    kappa = torch.linalg.cond(kd_ref.X).cpu()
    # the torch side is itself an LU inverse in double: twice the bound
    tol = 2 * C * (U_BUILD * kappa ** 2 + U_BUILD * kappa)
    if dagger:  # M^d (X^-d v): ||M^d|| <= 2m + 8 (eight unitary hops)
        t = kd_ref.apply(v.clone_empty(), v, dagger=True).to_complex()
        bound = (2 * mass + 8) * tol.max().item() * t.norm().item()
        assert (got - ref).norm().item() <= bound
    else:
        gb, rb = (kd_ref._to_blocks(x.to(kd_ref.X.device)).cpu()
                  for x in (got, ref))
        assert ((gb - rb).norm(dim=1) <= tol * rb.norm(dim=1)).all()


@pytest.mark.gpu
def test_kd_routing(monkeypatch):
    dims, mass = (4, 6, 2, 4), 0.5
    monkeypatch.delenv("QUDA_AMD_NATIVE_KD", raising=False)
    monkeypatch.setattr(dispatch, "_TRACE", True)
    u, psi = _links(dims, False).cuda(), _field(dims, "single")
    dispatch.trace_log().clear()
    outs = [KDBlockInverse(u, _geo(dims), mass, **kw).apply(
        psi.clone_empty(), psi).data for kw in ({}, {"native": False})]
    assert torch.equal(*outs)
    # ineligible: in place, native requested -> the torch path, same result
    kd = KDBlockInverse(u, _geo(dims), mass, native=True)
    same = psi.clone_empty()
    same.data.copy_(psi.data)
    assert torch.equal(kd.apply(same, same).data, outs[0])
    assert not any(op.startswith("kd_") for op, _ in dispatch.trace_log())
    monkeypatch.setenv("QUDA_AMD_NATIVE_KD", "1")
    KDBlockInverse(u, _geo(dims), mass).apply(psi.clone_empty(), psi)
    assert dispatch.trace_log()[-1][0] == "kd_apply"
