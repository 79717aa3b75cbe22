"""HIP hop-sum kernel (csrc/laplace.h) under laplace_apply, covdev_apply,
wuppertal_smear, the two-link smear and GaugeLaplace, against the torch
functions with the flag off, evaluated in complex128 on the CPU on
to_complex() of the very operands the kernel reads.

Bound per entry (P = largest column 2-norm of the input, nh = enabled hops,
u = 2^-53 or 2^-24, b_eff = b with the operator's diagonal folded in):

    |native - ref| <= 2 (nh + 8 + r) u (|a| nh + |b_eff|) P

A 3-term complex FMA dot against a row of norm <= 1 costs 5 roundings times
the neighbour's norm; nh accumulations and 3 roundings for the scalings and
the sum make up the rest; r = 6 for recon 12 (third row rebuilt in working
precision); the factor 2 covers non-fused variants. Half adds its output
block-float rounding: 2^-10 |ref entry| + 2^-23 max_site |ref|. Over n steps
the column-norm error obeys E' = sqrt(3) * bound(P_k) + (|a| nh + |b_eff|) E,
P_k taken from the reference's own steps. No tolerance here is tuned to the
kernel's output.

Measured on an MI355X, worst fraction of the bound over all cases: double
1.1e-1, single 2.7e-2, half 4.9e-1; the two sides of the GaugeLaplace.M
hermiticity check agreed to the last bit (defect 0).
"""

import functools

import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField, api
from quda_amd.models import laplace as lap
from quda_amd.models import spin_taste
from quda_amd.ops import dispatch

U_OF = {"double": 2.0 ** -53, "single": 2.0 ** -24, "half": 2.0 ** -24}
LATTICES = [(2, 2, 2, 2), (4, 6, 2, 6), (6, 6, 6, 4)]
A, B = 0.3, -0.7


@functools.lru_cache(maxsize=None)
def _geo(dims):
    return LatticeGeometry(dims)


@functools.lru_cache(maxsize=None)
def _gauge(dims, prec="double", recon="none", device="cpu"):
    return GaugeField(_geo(dims), prec, "cpu", recon).random_su3_(
        seed=7 + sum(dims)).to(device)


@functools.lru_cache(maxsize=None)
def _spinor(dims, prec="double", nspin=4, device="cpu", seed=11):
    return SpinorField(_geo(dims), prec, "cpu", nspin=nspin).gaussian_(
        seed=seed + sum(dims)).to(device)


def _as_double(f):
    """The complex128 CPU twin of a field: holds exactly what f stores."""
    c = f.to_complex().cpu()
    if isinstance(f, GaugeField):
        return GaugeField(f.geo, "double", shift=f.shift).from_complex(c)
    return SpinorField(f.geo, "double", nspin=f.nspin).from_complex(c)


def _colnorm(c):
    return c.reshape(-1, 3).norm(dim=-1).max().item()


def step_bound(prec, recon, nh, a, b_eff, P):
    r = 6 if recon == "twelve" else 0
    return 2 * (nh + 8 + r) * U_OF[prec] * (abs(a) * nh + abs(b_eff)) * P


def check(native, ref, bound, prec):
    """native: SpinorField; ref: complex128 CPU tensor; prints the worst
    fraction of the bound before asserting it."""
    got = native.to_complex().cpu()
    tol = torch.full_like(ref.real, bound)
    if prec == "half":
        site_max = torch.view_as_real(ref).abs().flatten(2).amax(-1)
        tol = tol + 2.0 ** -10 * ref.abs() + 2.0 ** -23 * site_max.reshape(
            *site_max.shape, *([1] * (ref.dim() - 2)))
    frac = ((got - ref).abs() / tol).max().item()
    print(f"fraction of bound [{prec}]: {frac:.3e}")
    assert frac <= 1.0, frac


def _no_ext(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the HIP extension must not be touched here")
    monkeypatch.setattr(dispatch, "hip_ext", boom)


# ---------------------------------------------------------------------------
# 1. CPU
# ---------------------------------------------------------------------------

def test_cpu_flag_is_inert(monkeypatch):
    _no_ext(monkeypatch)
    dims = (4, 6, 2, 6)
    g, psi = _gauge(dims), _spinor(dims)
    outs = []
    for native in (True, False):
        o = lap.laplace_apply(g, psi, psi.clone_empty(), ndim=3, a=A, b=B,
                              native=native)
        c = lap.covdev_apply(g, psi, 1, False, native=native)
        w = lap.wuppertal_smear(g, psi, alpha=3.0, n_steps=2, native=native)
        outs.append((o.data, c.data, w.data))
    for x, y in zip(*outs):
        assert torch.equal(x, y)

    out = psi.clone_empty()

    class OnGpu:  # the fields as laplace_eligible would see them on a GPU
        def __init__(self, f, **kw):
            self.__dict__.update(f.__dict__)
            self.__dict__.update(kw)
            self.device = torch.device("cuda")

    G, P_, O = OnGpu(g), OnGpu(psi), OnGpu(out)
    assert dispatch.laplace_eligible(O, P_, G, True)
    assert not dispatch.laplace_eligible(O, P_, G, False)
    assert not dispatch.laplace_eligible(O, P_, OnGpu(g, precision="single"),
                                         True)
    assert not dispatch.laplace_eligible(OnGpu(out, n_parity=1),
                                         OnGpu(psi, n_parity=1), G, True)
    assert not dispatch.laplace_eligible(P_, P_, G, True)
    assert not dispatch.laplace_eligible(OnGpu(psi), P_, G, True)  # same data
    from quda_amd.parallel import comms
    monkeypatch.setattr(comms, "comm_mask", lambda: 1)
    assert not dispatch.laplace_eligible(O, P_, G, True)


# ---------------------------------------------------------------------------
# 2.-6. GPU
# ---------------------------------------------------------------------------

LAPLACE_CASES = [(p, ns, d, nd, "none") for p in ("double", "single", "half")
                 for ns in (4, 1) for d in LATTICES for nd in (3, 4)]
LAPLACE_CASES += [(p, 4, (4, 6, 2, 6), 3, "twelve") for p in ("single", "half")]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,nspin,dims,ndim,recon", LAPLACE_CASES)
def test_laplace(prec, nspin, dims, ndim, recon):
    g = _gauge(dims, prec, recon, "cuda")
    psi = _spinor(dims, prec, nspin, "cuda")
    out = lap.laplace_apply(g, psi, psi.clone_empty(), ndim=ndim, a=A, b=B,
                            native=True)
    pd = _as_double(psi)
    ref = lap.laplace_apply(_as_double(g), pd, pd.clone_empty(), ndim=ndim,
                            a=A, b=B, native=False).to_complex()
    check(out, ref, step_bound(prec, recon, 2 * ndim, A, B - 2 * ndim * A,
                               _colnorm(pd.to_complex())), prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "half"])
@pytest.mark.parametrize("forward", [True, False])
@pytest.mark.parametrize("mu", range(4))
def test_covdev(mu, forward, prec):
    dims = (4, 6, 2, 6)
    g, psi = _gauge(dims, prec, "none", "cuda"), _spinor(dims, prec, 4, "cuda")
    out = lap.covdev_apply(g, psi, mu, forward, native=True)
    pd = _as_double(psi)
    ref = lap.covdev_apply(_as_double(g), pd, mu, forward,
                           native=False).to_complex()
    check(out, ref, step_bound(prec, "none", 1, 1.0, 0.0,
                               _colnorm(pd.to_complex())), prec)


def _steps_bound(prec, a, b_eff, norms):
    """Column-norm error after len(norms) steps; norms[k] = P of step k."""
    E, G = 0.0, abs(a) * 6 + abs(b_eff)
    for P in norms:
        E = 3 ** 0.5 * step_bound(prec, "none", 6, a, b_eff, P) + G * E
    return E


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "single"])
def test_wuppertal(prec, monkeypatch):
    dims, alpha, n = (4, 6, 2, 6), 3.0, 3
    g, psi = _gauge(dims, prec, "none", "cuda"), _spinor(dims, prec, 4, "cuda")
    before = psi.data.clone()
    out = lap.wuppertal_smear(g, psi, alpha=alpha, n_steps=n, native=True)
    assert out is not psi and torch.equal(psi.data, before)
    gd, cur, norms = _as_double(g), _as_double(psi), []
    for _ in range(n):
        norms.append(_colnorm(cur.to_complex()))
        cur = lap.wuppertal_smear(gd, cur, alpha=alpha, n_steps=1,
                                  native=False)
    a = alpha / (1 + 6 * alpha)
    check(out, cur.to_complex(), _steps_bound(prec, a, 1 - 6 * a, norms), prec)

    torch_out = lap.wuppertal_smear(g, psi, alpha=alpha, n_steps=n,
                                    native=False).to_complex()
    p = api.InvertParam(dslash_type=api.DslashType.WILSON, cuda_prec=prec)
    gp = api.GaugeParam(X=dims, device="cuda", cuda_prec=prec,
                        cuda_prec_sloppy=prec)
    try:
        api.load_gauge_quda(g.to_complex(), gp)
        src = psi.to_complex()
        monkeypatch.setenv("QUDA_AMD_NATIVE_LAPLACE", "1")
        got = api.perform_fermion_smear_quda(src, p, n_steps=n, width=alpha)
        assert torch.equal(got, out.to_complex())
        monkeypatch.delenv("QUDA_AMD_NATIVE_LAPLACE")
        got = api.perform_fermion_smear_quda(src, p, n_steps=n, width=alpha)
        assert torch.equal(got, torch_out)
    finally:
        api.end_quda()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dims", [(2, 2, 2, 2), (4, 6, 2, 6)])
def test_two_link(dims, prec):
    geo, width, n = _geo(dims), 2.0, 2
    u = _gauge(dims).to_complex()
    psi = _spinor(dims, prec, 1, "cuda")
    out = spin_taste.gaussian_smear_two_link(u.cuda(), geo, psi, width=width,
                                             n_steps=n, native=True)
    assert out is not psi
    cur, norms = _as_double(psi), []
    for _ in range(n):  # one step of the n-step smear: same coefficient
        norms.append(_colnorm(cur.to_complex()))
        cur = spin_taste.gaussian_smear_two_link(
            u, geo, cur, width=width / n ** 0.5, n_steps=1, native=False)
    coef = width * width / (4.0 * n)
    check(out, cur.to_complex(),
          _steps_bound(prec, coef, 1 - 6 * coef, norms), prec)


@pytest.mark.gpu
def test_gauge_laplace_m():
    dims, m2, u = (6, 6, 6, 4), 0.5, U_OF["double"]
    g = _gauge(dims, "double", "none", "cuda")
    op = lap.GaugeLaplace(g, m2=m2, native=True)
    v = _spinor(dims, "double", 1, "cuda", seed=21)
    w = _spinor(dims, "double", 1, "cuda", seed=22)
    Mv, Mw = op.M(v.clone_empty(), v), op.M(w.clone_empty(), w)
    ref = lap.GaugeLaplace(_as_double(g), m2=m2, native=False)
    vd = _as_double(v)
    check(Mv, ref.M(vd.clone_empty(), vd).to_complex(),
          step_bound("double", "none", 6, -1.0, m2 + 6.0,
                     _colnorm(vd.to_complex())), "double")
    vc, wc = v.to_complex().flatten(), w.to_complex().flatten()
    lhs = torch.vdot(vc, Mw.to_complex().flatten())
    rhs = torch.vdot(wc, Mv.to_complex().flatten()).conj()
    bound = 64 * u * vc.norm().item() * wc.norm().item() * (12 + m2)
    print(f"hermiticity fraction: {abs(lhs - rhs).item() / bound:.3e}")
    assert abs(lhs - rhs).item() <= bound
