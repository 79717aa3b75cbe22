"""GPU numerics tests: every HIP kernel vs the plain-PyTorch fp64 oracle.
(analogue of the reference's dslash_ctest / blas_test GPU-vs-host checks)"""
import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField
from quda_amd.fields.clover import CloverField
from quda_amd.models import DiracCloverPC, DiracWilsonPC
from quda_amd.ops import blas
from quda_amd.ops import reference as ref
from quda_amd.ops.dispatch import CLOV_POST, CLOV_X, PLAIN, dslash_wilson
from quda_amd.solvers import cg_solve

pytestmark = pytest.mark.gpu

TOL = {"double": 1e-12, "single": 2e-5, "half": 2e-2}
RECONS = {"double": [18], "single": [18, 12], "half": [12, 18]}
KAPPA = 0.13
CSW = 1.1


@pytest.fixture(scope="module")
def setup():
    geo = LatticeGeometry((8, 8, 8, 8))
    g = GaugeField(geo, "double").random_su3_(seed=31)
    psi = SpinorField(geo, "double").gaussian_(seed=32)
    chi = SpinorField(geo, "double").gaussian_(seed=33)
    A = ref.clover_matrix(g.to_complex(), geo, KAPPA, CSW)
    return geo, g, psi, chi, A


def _gpu_fields(geo, g, psi, prec, recon):
    gd = GaugeField(geo, prec, "cuda", reconstruct="none" if recon == 18 else "twelve")
    gd.from_complex(g.to_complex().cuda())
    sd = SpinorField(geo, prec, "cuda", n_parity=2).from_complex(
        psi.to_complex().cuda())
    return gd, sd


@pytest.mark.parametrize("prec", ["double", "single", "half"])
@pytest.mark.parametrize("dagger", [False, True])
def test_dslash_vs_oracle(setup, prec, dagger):
    geo, g, psi, chi, A = setup
    u = g.to_complex()
    for recon in RECONS[prec]:
        gd, sd = _gpu_fields(geo, g, psi, prec, recon)
        out = SpinorField(geo, prec, "cuda", n_parity=1)
        for parity in (0, 1):
            dslash_wilson(out, sd.parity_view(1 - parity), gd, parity, dagger)
            got = out.to_complex().cpu()[0]
            want = ref.dslash_wilson_parity(u, psi.to_complex()[1 - parity],
                                            geo, parity, dagger)
            err = (got - want).abs().max().item() / want.abs().max().item()
            assert err < TOL[prec], (prec, recon, parity, dagger, err)


@pytest.mark.parametrize("prec", ["double", "single"])
def test_dslash_xpay(setup, prec):
    geo, g, psi, chi, A = setup
    u = g.to_complex()
    gd, sd = _gpu_fields(geo, g, psi, prec, 18)
    xd = SpinorField(geo, prec, "cuda", n_parity=1).from_complex(
        chi.to_complex()[0:1].cuda())
    out = SpinorField(geo, prec, "cuda", n_parity=1)
    a = -0.37
    dslash_wilson(out, sd.parity_view(1), gd, 0, a=a, x=xd)
    got = out.to_complex().cpu()[0]
    want = chi.to_complex()[0] + a * ref.dslash_wilson_parity(
        u, psi.to_complex()[1], geo, 0)
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err < TOL[prec]


@pytest.mark.parametrize("prec", ["double", "single", "half"])
@pytest.mark.parametrize("mode", [CLOV_POST, CLOV_X])
def test_dslash_clover_modes(setup, prec, mode):
    geo, g, psi, chi, A = setup
    u = g.to_complex()
    recon = RECONS[prec][0]
    gd, sd = _gpu_fields(geo, g, psi, prec, recon)
    cl = CloverField(geo, prec, "cuda")
    cl.data.copy_(cl._to_native(
        __import__("quda_amd.fields.clover", fromlist=["pack_clover"])
        .pack_clover(A.cuda())))
    xd = SpinorField(geo, prec, "cuda", n_parity=1).from_complex(
        chi.to_complex()[0:1].cuda())
    out = SpinorField(geo, prec, "cuda", n_parity=1)
    a = -0.29
    D = ref.dslash_wilson_parity(u, psi.to_complex()[1], geo, 0)
    if mode == CLOV_POST:
        dslash_wilson(out, sd.parity_view(1), gd, 0, mode=CLOV_POST, a=a,
                      x=xd, clover=cl)
        want = chi.to_complex()[0] + a * ref.apply_clover(A[0], D)
    else:
        dslash_wilson(out, sd.parity_view(1), gd, 0, mode=CLOV_X, a=a, x=xd,
                      clover=cl)
        want = ref.apply_clover(A[0], chi.to_complex()[0]) + a * D
    got = out.to_complex().cpu()[0]
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err < TOL[prec]


@pytest.mark.parametrize("prec", ["double", "single", "half"])
def test_blas_gpu(setup, prec):
    geo, g, psi, chi, A = setup
    tol = TOL[prec]
    x = SpinorField(geo, prec, "cuda", n_parity=2).from_complex(psi.to_complex().cuda())
    y = SpinorField(geo, prec, "cuda", n_parity=2).from_complex(chi.to_complex().cuda())
    xc, yc = psi.to_complex(), chi.to_complex()
    # reductions
    assert abs(blas.norm2(x) - (xc.abs() ** 2).sum().item()) < tol * abs((xc.abs() ** 2).sum().item())
    rd = blas.re_dot(x, y)
    want_rd = (xc.conj() * yc).real.sum().item()
    assert abs(rd - want_rd) < tol * (abs(want_rd) + 1)
    cd = blas.c_dot(x, y)
    want_cd = (xc.conj() * yc).sum().item()
    assert abs(cd - want_cd) < tol * (abs(want_cd) + 1)
    # axpy_norm2
    r = blas.axpy_norm2(0.7, x, y)
    yc = yc + 0.7 * xc
    assert abs(r - (yc.abs() ** 2).sum().item()) < 10 * tol * r
    # xpay
    blas.xpay(x, -1.3, y)
    yc = xc - 1.3 * yc
    err = (y.to_complex().cpu() - yc).abs().max().item()
    assert err < 10 * tol * yc.abs().max().item()
    # caxpy
    blas.caxpy(0.3 - 0.4j, x, y)
    yc = yc + (0.3 - 0.4j) * xc
    err = (y.to_complex().cpu() - yc).abs().max().item()
    assert err < 20 * tol * yc.abs().max().item()
    # xmy_norm2
    r = blas.xmy_norm2(x, y)
    yc = xc - yc
    assert abs(r - (yc.abs() ** 2).sum().item()) < 20 * tol * (r + 1)
    # scal
    blas.scal(0.5, y)
    yc = 0.5 * yc
    err = (y.to_complex().cpu() - yc).abs().max().item()
    assert err < 20 * tol * (yc.abs().max().item() + 1)


def test_convert_gpu(setup):
    geo, g, psi, chi, A = setup
    d = SpinorField(geo, "double", "cuda", n_parity=2).from_complex(psi.to_complex().cuda())
    s = SpinorField(geo, "single", "cuda", n_parity=2)
    h = SpinorField(geo, "half", "cuda", n_parity=2)
    blas.copy(s, d)
    blas.copy(h, s)
    d2 = SpinorField(geo, "double", "cuda", n_parity=2)
    blas.copy(d2, h)
    ref_c = psi.to_complex()
    assert (s.to_complex().cpu() - ref_c).abs().max().item() < 1e-6
    assert (d2.to_complex().cpu() - ref_c).abs().max().item() < 2e-3


@pytest.mark.parametrize("sloppy", ["double", "single", "half"])
def test_cg_wilson_gpu(setup, sloppy):
    geo, g, psi, chi, A = setup
    gd = GaugeField(geo, "double", "cuda").from_complex(g.to_complex().cuda())
    gs_prec = "single" if sloppy == "single" else ("half" if sloppy == "half" else "double")
    recon_s = "twelve" if sloppy != "double" else "none"
    gs = GaugeField(geo, gs_prec, "cuda", reconstruct=recon_s).from_complex(
        g.to_complex().cuda())
    d = DiracWilsonPC(gd, KAPPA)
    ds = DiracWilsonPC(gs, KAPPA)
    b = SpinorField(geo, "double", "cuda", n_parity=1).from_complex(
        psi.to_complex()[0:1].cuda())
    x = SpinorField(geo, "double", "cuda", n_parity=1)
    stats = cg_solve(d, x, b, op_sloppy=ds, sloppy=sloppy, tol=1e-8,
                     maxiter=500)
    assert stats.converged, (sloppy, stats)
    # independent residual check on the oracle
    u = g.to_complex()
    xe = x.to_complex().cpu()[0]
    t = ref.dslash_wilson_parity(u, xe, geo, 1)
    Mx = xe - KAPPA ** 2 * ref.dslash_wilson_parity(u, t, geo, 0)
    # Mdag
    t = ref.dslash_wilson_parity(u, Mx, geo, 1, dagger=True)
    MdMx = Mx - KAPPA ** 2 * ref.dslash_wilson_parity(u, t, geo, 0, dagger=True)
    rel = (MdMx - psi.to_complex()[0]).abs().max().item()
    assert rel < 1e-6


def test_cg_clover_gpu(setup):
    geo, g, psi, chi, A = setup
    gd = GaugeField(geo, "double", "cuda").from_complex(g.to_complex().cuda())
    gh = GaugeField(geo, "half", "cuda", reconstruct="twelve").from_complex(
        g.to_complex().cuda())
    cld = CloverField(geo, "double", "cuda")
    clh = CloverField(geo, "half", "cuda")
    Ac = A.cuda()
    cld.from_matrices(Ac)
    from quda_amd.fields.clover import pack_clover
    clh.data.copy_(clh._to_native(pack_clover(Ac)))
    Ainv = cld.to_complex(inverse=True)
    clh.inv_data.copy_(clh._to_native(pack_clover(Ainv.to("cuda"))))
    d = DiracCloverPC(gd, cld, KAPPA)
    dh = DiracCloverPC(gh, clh, KAPPA)
    b = SpinorField(geo, "double", "cuda", n_parity=1).from_complex(
        psi.to_complex()[0:1].cuda())
    x = SpinorField(geo, "double", "cuda", n_parity=1)
    stats = cg_solve(d, x, b, op_sloppy=dh, sloppy="half", tol=1e-8,
                     maxiter=1000)
    assert stats.converged, stats
    out = SpinorField(geo, "double", "cuda", n_parity=1)
    tmp = SpinorField(geo, "double", "cuda", n_parity=1)
    d.MdagM(out, x, tmp)
    r = blas.xmy_norm2(b, out)
    assert r < 1e-14 * blas.norm2(b) * 1e6  # rel residual < 1e-4 in norm2


@pytest.mark.gpu
def test_deterministic_reduce_gpu():
    """QUDA_DETERMINISTIC_REDUCE analogue: det path bit-stable and
    consistent with the atomic path."""
    from quda_amd import LatticeGeometry, SpinorField
    from quda_amd.ops import blas
    geo = LatticeGeometry((8, 8, 8, 16))
    x = SpinorField(geo, "double", "cuda").gaussian_(seed=191)
    y = SpinorField(geo, "double", "cuda").gaussian_(seed=192)
    blas.set_deterministic(True)
    try:
        r1 = blas.norm2(x)
        r2 = blas.norm2(x)
        c1 = blas.c_dot(x, y)
        c2 = blas.c_dot(x, y)
        assert r1 == r2 and c1 == c2  # bitwise stable
    finally:
        blas.set_deterministic(False)
    r3 = blas.norm2(x)
    assert abs(r3 - r1) < 1e-10 * abs(r1)


@pytest.mark.gpu
def test_batch_dslash_self_wrap_gpu():
    """Merged-halo multi-RHS dslash (forced self-partition) matches the
    unpartitioned per-RHS result on device."""
    from quda_amd.ops.dispatch import dslash_wilson, dslash_wilson_batch
    from quda_amd.parallel import comms
    geo = LatticeGeometry((4, 6, 4, 8))
    gen = torch.Generator().manual_seed(951)
    from quda_amd.fields.gauge import project_su3
    m = torch.randn((4, 2, geo.volume_cb, 3, 3, 2), generator=gen,
                    dtype=torch.float64)
    u = project_su3(torch.view_as_complex(m)).cuda()
    g = GaugeField(geo, "double", "cuda").from_complex(u)
    n = 3
    srcs = [SpinorField(geo, "double", "cuda", n_parity=1).gaussian_(
        seed=960 + i) for i in range(n)]
    outs_ref = [SpinorField(geo, "double", "cuda", n_parity=1)
                for _ in range(n)]
    for i in range(n):
        dslash_wilson(outs_ref[i], srcs[i], g, 0)
    try:
        comms.set_forced_partition(0b1111)
        g2 = GaugeField(geo, "double", "cuda").from_complex(u)
        outs = [SpinorField(geo, "double", "cuda", n_parity=1)
                for _ in range(n)]
        dslash_wilson_batch(outs, srcs, g2, 0)
    finally:
        comms.set_forced_partition(0)
    for i in range(n):
        err = (outs[i].to_complex()
               - outs_ref[i].to_complex()).abs().max().item()
        assert err < 1e-13, (i, err)


@pytest.mark.parametrize("prec", ["single", "half"])
def test_dslash_occupancy_variant(setup, prec):
    """The LBW=3 (64-thread / 3-wave __launch_bounds__) kernel variant must
    match the oracle exactly like the default variant."""
    from quda_amd.ops.dispatch import hip_ext as _ext
    geo, g, psi, chi, A = setup
    u = g.to_complex()
    gd, sd = _gpu_fields(geo, g, psi, prec, 12)
    out = SpinorField(geo, prec, "cuda", n_parity=1)
    _ext().set_dslash_waves(3)
    try:
        for dagger in (False, True):
            dslash_wilson(out, sd.parity_view(1), gd, 0, dagger)
            got = out.to_complex().cpu()[0]
            want = ref.dslash_wilson_parity(u, psi.to_complex()[1], geo, 0,
                                            dagger)
            err = (got - want).abs().max().item() / want.abs().max().item()
            assert err < TOL[prec], (prec, dagger, err)
    finally:
        _ext().set_dslash_waves(0)


@pytest.mark.parametrize("prec", ["half", "single", "double"])
@pytest.mark.parametrize("nrhs", [2, 4])
def test_dslash_mrhs_vs_per_rhs(setup, prec, nrhs):
    """k_dslash_wilson_mrhs (NRHS sides per gauge load) must match the
    per-RHS kernel bit-for-bit in PLAIN and CLOV_POST(+xpay) modes."""
    from quda_amd.fields.clover import pack_clover
    from quda_amd.ops import dispatch
    from quda_amd.ops.dispatch import dslash_wilson_batch
    geo, g, psi, chi, A = setup
    recon = 12 if prec != "double" else 18
    gd, _ = _gpu_fields(geo, g, psi, prec, recon)
    cl = CloverField(geo, prec, "cuda")
    cl.data.copy_(cl._to_native(pack_clover(A.cuda())))
    cl.inv_data.copy_(cl.data)  # any hermitian packed field works here
    gen = torch.Generator().manual_seed(77)
    inps, outs_m, outs_1, xs = [], [], [], []
    for r in range(nrhs):
        v = torch.view_as_complex(
            torch.randn(1, geo.volume_cb, 4, 3, 2, generator=gen,
                        dtype=torch.float64)).cuda()
        inps.append(SpinorField(geo, prec, "cuda", n_parity=1).from_complex(v))
        xs.append(SpinorField(geo, prec, "cuda", n_parity=1).from_complex(
            0.5 * v))
        outs_m.append(SpinorField(geo, prec, "cuda", n_parity=1))
        outs_1.append(SpinorField(geo, prec, "cuda", n_parity=1))
    # LSB-level fp-contraction differences between the two template
    # instantiations are expected (the compiler fuses mul+add chains
    # differently per kernel); require agreement at the precision's
    # roundoff, not bitwise.
    rtol = {"half": 2e-3, "single": 1e-5, "double": 1e-13}[prec]
    # the group size defaults to 1 (per-RHS launches): switch the multi-RHS
    # kernel on, or the batch would be compared with itself
    saved = dispatch._MRHS_GROUP
    try:
        dispatch._MRHS_GROUP = nrhs
        assert dispatch._mrhs_groups(nrhs)[0]
        for mode, use_x, use_cl in [(PLAIN, False, None), (PLAIN, True, None),
                                    (CLOV_POST, True, cl)]:
            for dag in (False, True):
                dslash_wilson_batch(outs_m, inps, gd, 0, dagger=dag, a=-0.3,
                                    xs=xs if use_x else None, mode=mode,
                                    clover=use_cl)
                for r in range(nrhs):
                    dslash_wilson(outs_1[r], inps[r], gd, 0, dagger=dag,
                                  a=-0.3, x=xs[r] if use_x else None,
                                  mode=mode, clover=use_cl)
                    ref_c = outs_1[r].to_complex()
                    dm = (outs_m[r].to_complex() - ref_c)
                    err = dm.abs().max().item() / ref_c.abs().max().item()
                    assert err < rtol, (prec, nrhs, mode, use_x, dag, r, err)
    finally:
        dispatch._MRHS_GROUP = saved


@pytest.mark.parametrize("prec", ["half", "single"])
def test_dslash_recon8_gpu(setup, prec):
    """recon-8 kernel decode vs the oracle and vs the recon-12 kernel."""
    geo, g, psi, chi, A = setup
    u = g.to_complex()
    g8 = GaugeField(geo, prec, "cuda", reconstruct="eight")
    g8.from_complex(u.cuda())
    sd = SpinorField(geo, prec, "cuda", n_parity=2).from_complex(
        psi.to_complex().cuda())
    out = SpinorField(geo, prec, "cuda", n_parity=1)
    for dagger in (False, True):
        dslash_wilson(out, sd.parity_view(1), g8, 0, dagger)
        want = ref.dslash_wilson_parity(u, psi.to_complex()[1], geo, 0,
                                        dagger)
        err = ((out.to_complex().cpu()[0] - want).abs().max()
               / want.abs().max()).item()
        assert err < TOL[prec], (prec, dagger, err)


@pytest.mark.parametrize("prec", ["double", "single", "half"])
def test_triple_cg_update_gpu(setup, prec):
    """Fused x += a p; r -= a Ap; ||r||^2 vs the two-op composition."""
    geo, g, psi, chi, A = setup
    gen = torch.Generator().manual_seed(515)

    def mk(seed):
        v = torch.view_as_complex(torch.randn(1, geo.volume_cb, 4, 3, 2,
                                              generator=gen,
                                              dtype=torch.float64))
        return SpinorField(geo, prec, "cuda", n_parity=1).from_complex(
            v.cuda())

    p, ap = mk(1), mk(2)
    x1, r1 = mk(3), mk(4)
    x2 = SpinorField(geo, prec, "cuda", n_parity=1).from_complex(
        x1.to_complex())
    r2 = SpinorField(geo, prec, "cuda", n_parity=1).from_complex(
        r1.to_complex())
    a = 0.37
    fused = blas.triple_cg_update(a, p, ap, x1, r1)
    blas.axpy(a, p, x2)
    ref_n = blas.axpy_norm2(-a, ap, r2)
    tol = {"double": 1e-12, "single": 1e-5, "half": 5e-2}[prec]
    assert abs(fused - ref_n) < tol * (abs(ref_n) + 1), (prec, fused, ref_n)
    dx = (x1.to_complex() - x2.to_complex()).abs().max().item()
    dr = (r1.to_complex() - r2.to_complex()).abs().max().item()
    assert dx < tol * 10 and dr < tol * 10, (prec, dx, dr)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["half", "quarter"])
def test_dslash_lds_variant(setup, prec):
    """k_dslash_wilson_lds (in-spinor halo tile staged through LDS) must
    reproduce the gather-first kernel on PLAIN (+dagger), CLOV_POST and
    xpay — same decoded inputs, same accumulation order, so the results
    agree to same-precision roundoff."""
    from quda_amd.fields.clover import CloverField
    from quda_amd.ops.dispatch import CLOV_POST
    from quda_amd.ops.dispatch import hip_ext as _ext
    geo, g, psi, chi, A = setup
    gd, sd = _gpu_fields(geo, g, psi, prec, 12)
    cl = CloverField(geo, prec, "cuda").from_matrices(A.cuda())
    xd = SpinorField(geo, prec, "cuda", n_parity=1).from_complex(
        chi.to_complex()[0:1].cuda())
    out0 = SpinorField(geo, prec, "cuda", n_parity=1)
    out1 = SpinorField(geo, prec, "cuda", n_parity=1)
    cases = [dict(mode=PLAIN, dagger=False), dict(mode=PLAIN, dagger=True),
             dict(mode=CLOV_POST, clover=cl, clover_inverse=False),
             dict(mode=PLAIN, a=-0.4, x=xd)]
    for kw in cases:
        kw2 = dict(kw)
        _ext().set_dslash_lds(0)
        dslash_wilson(out0, sd.parity_view(1), gd, 0, **kw2)
        _ext().set_dslash_lds(1)
        try:
            dslash_wilson(out1, sd.parity_view(1), gd, 0, **kw2)
        finally:
            _ext().set_dslash_lds(0)
        a = out0.to_complex().cpu()
        b = out1.to_complex().cpu()
        err = (a - b).abs().max().item() / a.abs().max().item()
        # same decoded inputs and op order, but the per-site block-float
        # norm can flip one stored ULP between variants
        tol = {"half": 5e-4, "quarter": 5e-3}[prec]
        assert err < tol, (prec, kw.get("mode"), err)
