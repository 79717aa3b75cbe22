"""Schedule forms of the Wilson dslash (set_dslash_waves): the 8-gather form,
the fenced 2-round form under the occupancy cap and the fenced 4-round double
body must all compute the same stencil. Every
form is checked against the float64 oracle at every precision, the fused
epilogues must keep their bitwise relations to the plain kernels of the same
form, and the mixed double/half CG must converge under each form."""
import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField
from quda_amd.fields.clover import CloverField
from quda_amd.models import DiracCloverPC
from quda_amd.ops import blas
from quda_amd.ops import dispatch
from quda_amd.ops import reference as ref
from quda_amd.ops.dispatch import CLOV_POST, PLAIN, apply_clover, dslash_wilson
from quda_amd.solvers import cg_solve

# (6,6,4,4): Vcb = 288 = 4*64 + 32, so the last 64-thread workgroup is partial
LATTICES = [(4, 4, 4, 8), (6, 6, 4, 4)]
# set_dslash_waves values. 0: the default form (all 8 gathers in flight;
# double: 4 fenced rounds). 3: 2 fenced rounds in 64-thread workgroups under
# the 3-wave register cap (double keeps its own form). The fenced 2- and
# 4-round forms at the default launch bounds were measured and removed
# (profiles/r07_dslash_rounds.md).
FORMS = [0, 3]
FUSED_FORMS = [0]  # form 3 has no fused-epilogue kernels
RECONS = {"double": [18], "single": [18, 12], "half": [12, 18],
          "quarter": [12, 18]}
# Recons at which MdagM_dot's Ap is checked bitwise against M, M(dagger).
# Known defect, open as an issue of its own and older than the round fence:
# at single / recon 12 the 8-gather k_dslash_wilson_xpay_dot and the plain
# dagger xpay kernel differ in the last float bit (27 of 6144 reals on
# 4x4x4x8, max 1.2e-7 at scale 3.9), so that one relation does not hold and
# is not asserted here; the dual-output relations are, at every recon.
DOT_RECONS = {"double": [18], "single": [18], "half": [12, 18],
              "quarter": [12, 18]}
# tests/test_gpu_kernels.py TOL, and the quarter bound of tests/test_quarter.py
TOL = {"double": 1e-12, "single": 2e-5, "half": 2e-2, "quarter": 0.25}
KAPPA = 0.13
CSW = 1.1
XPAY_A = -0.29

_CACHE = {}


def _host(dims):
    """Gauge, spinors, clover and the oracle's D psi for both parities and
    daggers: computed once per lattice and left unchanged."""
    if dims not in _CACHE:
        geo = LatticeGeometry(dims)
        g = GaugeField(geo, "double").random_su3_(seed=41)
        psi = SpinorField(geo, "double").gaussian_(seed=42).to_complex()
        chi = SpinorField(geo, "double").gaussian_(seed=43).to_complex()
        u = g.to_complex()
        A = ref.clover_matrix(u, geo, KAPPA, CSW)
        D = {(p, dag): ref.dslash_wilson_parity(u, psi[1 - p], geo, p, dag)
             for p in (0, 1) for dag in (False, True)}
        _CACHE[dims] = (geo, u, psi, chi, A, D)
    return _CACHE[dims]


def _gauge(geo, u, prec, recon):
    gd = GaugeField(geo, prec, "cuda",
                    reconstruct="none" if recon == 18 else "twelve")
    return gd.from_complex(u.cuda())


def _spinor(geo, prec, c):
    return SpinorField(geo, prec, "cuda", n_parity=1).from_complex(c.cuda())


def _raw_equal(a: SpinorField, b: SpinorField) -> bool:
    """Bitwise equality of the stored field (body and per-site norm)."""
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    vt = bits[a.data.element_size()]
    same = torch.equal(a.data.view(vt), b.data.view(vt))
    if a.norm is not None:
        same = same and torch.equal(a.norm.view(torch.int32),
                                    b.norm.view(torch.int32))
    return same


class _form:
    """Run at one schedule form with a fixed 64-thread workgroup (the
    autotuner would re-apply its own block size); restores what it found."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        ext = dispatch.hip_ext()
        self.prev = (ext.get_dslash_waves(), ext.get_dslash_block(),
                     dispatch.autotune_enabled())
        dispatch.set_autotune(False)
        ext.set_dslash_block(64)
        ext.set_dslash_waves(self.form)
        assert ext.get_dslash_waves() == self.form, self.form

    def __exit__(self, *exc):
        ext = dispatch.hip_ext()
        ext.set_dslash_waves(self.prev[0])
        ext.set_dslash_block(self.prev[1])
        dispatch.set_autotune(self.prev[2])


# ---------------------------------------------------------------------------
# 1. every form against the float64 oracle
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", ["double", "single", "half", "quarter"])
def test_forms_vs_oracle(prec, form):
    worst = 0.0
    for dims in LATTICES:
        geo, u, psi, chi, A, D = _host(dims)
        cl = CloverField(geo, prec, "cuda").from_matrices(A.cuda())
        out = SpinorField(geo, prec, "cuda", n_parity=1)
        for recon in RECONS[prec]:
            gd = _gauge(geo, u, prec, recon)
            for parity in (0, 1):
                inp = _spinor(geo, prec, psi[1 - parity:2 - parity])
                xd = _spinor(geo, prec, chi[parity:parity + 1])
                for dagger in (False, True):
                    d0 = D[(parity, dagger)]
                    ad0 = ref.apply_clover(A[parity], d0)
                    cases = [
                        (PLAIN, None, 1.0, d0),
                        (PLAIN, xd, XPAY_A, chi[parity] + XPAY_A * d0),
                        (CLOV_POST, None, 1.0, ad0),
                        (CLOV_POST, xd, XPAY_A, chi[parity] + XPAY_A * ad0),
                    ]
                    for mode, x, a, want in cases:
                        with _form(form):
                            dslash_wilson(out, inp, gd, parity, dagger,
                                          mode=mode, a=a, x=x, clover=cl)
                        got = out.to_complex().cpu()[0]
                        err = ((got - want).abs().max()
                               / want.abs().max()).item()
                        worst = max(worst, err)
                        assert err < TOL[prec], (
                            prec, form, dims, recon, parity, dagger, mode,
                            x is not None, err)
    print(f"form {form} {prec}: worst relative error {worst:.3e}")


# ---------------------------------------------------------------------------
# 2. fused epilogues: bitwise relations inside one form
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FUSED_FORMS)
@pytest.mark.parametrize("prec", ["double", "single", "half", "quarter"])
def test_fused_epilogues_in_form(prec, form):
    for dims in LATTICES:
        geo, u, psi, chi, A, D = _host(dims)
        cl = CloverField(geo, prec, "cuda").from_matrices(A.cuda())
        inp = _spinor(geo, prec, psi[1:2])
        p = _spinor(geo, prec, psi[0:1])
        for recon in RECONS[prec]:
            gd = _gauge(geo, u, prec, recon)
            d = DiracCloverPC(gd, cl, KAPPA)
            case = (prec, form, dims, recon)
            with _form(form):
                # dual output against the plain launch and apply_clover
                for xd, a in ((None, 1.0),
                              (_spinor(geo, prec, chi[0:1]), XPAY_A)):
                    out_a, out_b, out2, two = (
                        SpinorField(geo, prec, "cuda", n_parity=1)
                        for _ in range(4))
                    kw = dict(mode=CLOV_POST, a=a, x=xd, clover=cl,
                              clover_inverse=True)
                    dslash_wilson(out_a, inp, gd, 0, **kw)
                    apply_clover(two, out_a, cl, 0, inverse=True)
                    dslash_wilson(out_b, inp, gd, 0, out2=out2, **kw)
                    assert _raw_equal(out_a, out_b), (case, xd is not None)
                    assert _raw_equal(out2, two), (case, xd is not None)
            # fused dot against M, M(dagger) and re_dot
            if recon not in DOT_RECONS[prec]:
                continue
            with _form(form):
                Ap, Ap0, tmp = (SpinorField(geo, prec, "cuda", n_parity=1)
                                for _ in range(3))
                res = torch.zeros(2, dtype=torch.float64, device="cuda")
                d.MdagM_dot(Ap, p, tmp, res)
                want = blas.re_dot(p, Ap)
                d.M(tmp, p, dagger=False)
                d.M(Ap0, tmp, dagger=True)
            assert _raw_equal(Ap, Ap0), case
            rel = abs(res[0].item() - want) / abs(want)
            print(f"fused dot {case}: rel {rel:.3e}")
            assert rel <= 1e-10, (case, res[0].item(), want)


# ---------------------------------------------------------------------------
# 3. mixed double/half CG under each form (assertions of test_cg_clover_gpu)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_cg_clover_in_form(form):
    geo, u, psi, chi, A, D = _host(LATTICES[0])
    gd = _gauge(geo, u, "double", 18)
    gh = _gauge(geo, u, "half", 12)
    cld = CloverField(geo, "double", "cuda").from_matrices(A.cuda())
    clh = CloverField(geo, "half", "cuda").from_matrices(A.cuda())
    d = DiracCloverPC(gd, cld, KAPPA)
    dh = DiracCloverPC(gh, clh, KAPPA)
    b = _spinor(geo, "double", psi[0:1])
    x = SpinorField(geo, "double", "cuda", n_parity=1)
    with _form(form):
        stats = cg_solve(d, x, b, op_sloppy=dh, sloppy="half", tol=1e-8,
                         maxiter=1000)
        out = SpinorField(geo, "double", "cuda", n_parity=1)
        tmp = SpinorField(geo, "double", "cuda", n_parity=1)
        d.MdagM(out, x, tmp)
    assert stats.converged, (form, stats)
    r = blas.xmy_norm2(b, out)
    print(f"form {form}: {stats.iters} iters, {stats.reliable_updates} "
          f"reliable updates, true |r|^2 {r:.3e}")
    assert r < 1e-14 * blas.norm2(b) * 1e6  # rel residual < 1e-4 in norm2
