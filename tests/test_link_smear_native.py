"""Native link smearing: the level tables of gauge/smear.py and their torch
oracle smear_level_reference against ape_smear / hyp_smear, and the HIP level
kernel of csrc/smear.hip against that oracle.

Per-level bound, per entry of an output link (u = 2^-53):

    polar:         |kernel - reference| <= 233 u / sigma_3
    Gram-Schmidt:  |kernel - reference| <= 428 u w^2 / (n_0 n_1)

sigma_3 is the smallest singular value of the reference's matrix M before
projection, n_0 and n_1 the two norms its Gram-Schmidt divides by, and w =
max(1, c0 + 2 ns c1) the weight sum (1 for HYP and 4-d APE, 1 + alpha/2 for
spatial APE, which keeps its t staples). The inputs are unitary, so
sigma_1 <= w and 1/sigma_3 >= (sigma_1/sigma_3) / w: the absolute roundings
of M are measured against w, not against sigma_1.

M: a complex 3-term dot product costs 5 roundings against the modulus
product, entries of a unitary product are <= 1, the second product of a
staple inherits sqrt(3) times the first one's error: 5 (1 + sqrt 3) < 14 per
staple term, weighted by 2 ns c1 <= w; 2 ns - 1 accumulations of numbers
<= 2 ns, weighted by c1: 6; the two scalings and the final addition: 3.
That is 23 u w per entry, 69 u w in Frobenius norm, 138 u w for both sides.
The polar factor moves by at most ||dM||_F / sigma_3.
Newton: one step costs 16 roundings (cofactor 4, determinant 8, quotient 2,
scaling 1, mean 1) against a cofactor inverse whose relative error is the
condition number kappa_k of the iterate times that; the step maps it to a
change kappa_k times 16 u of the polar factor. kappa_k at least halves per
step, so all steps up to the cap POLAR_MAX_ITER = 16 sum to 2 x 16 kappa u;
the same again for the reference's SVD: 64 u sigma_1 / sigma_3. The stopping
test ||X_{k+1} - X_k||_F < 2^-27 leaves delta^2 / 2 < u / 4 by quadratic
convergence. Phase: determinant 8, atan2, division, sincos 4, product 3,
both sides: 30 u. Sum: (138 + 64 + 31) u / sigma_3.
Gram-Schmidt: row 0 errs by d / n_0 (d = 46 u w per entry for both sides),
row 1 by d (1 + 2 / n_0) / n_1 <= 3 d w / (n_0 n_1), row 2 by twice their
sum: at most 8 d w / (n_0 n_1), plus 2 x 30 u for its own roundings
(test_gauge_fix_native.py): (8 x 46 + 60) u w^2 / (n_0 n_1).

End to end the per-level bounds, at the worst conditioning of the first
iteration's reference, are summed over the levels and iterations traversed.
Over-improved stout: rho times the path-force bound of
test_gauge_path_native.py at scale 1 (Q = 6 F at beta = 1), plus 1e-14 for
the exponential.

Measured on an MI355X, worst fraction of the bound over the three lattices:
APE 1.0e-2 (warm; hot 3.6e-3), HYP 1 0.19, HYP 2 0.17, HYP 3 0.18 (warm; hot
0.13, 7.4e-2, 5.2e-2); end to end HYP 3.3e-2, APE 4.1e-3; over-improved
stout 6.3e-3 (eps -0.25) and 3.1e-2 (eps 1).
"""

import functools
import math

import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry
from quda_amd.fields.gauge import project_su3
from quda_amd.gauge import (ape_smear, hyp_smear, over_improved_stout_smear,
                            stout_smear)
from quda_amd.gauge import smear as sm
from quda_amd.ops import dispatch

U = 2.0 ** -53
LATTICES = [(2, 2, 2, 2), (4, 6, 2, 6), (6, 6, 2, 2)]
EYE = torch.eye(3, dtype=torch.complex128)
ALPHA_APE, ALPHA_HYP = 0.5, (0.75, 0.6, 0.3)
LEVELS = ["ape4", "ape3", "hyp1", "hyp2", "hyp3"]
C_POLAR, C_GS = 233, 428


@functools.lru_cache(maxsize=None)
def _geo(dims):
    return LatticeGeometry(dims)


@functools.lru_cache(maxsize=None)
def _field(dims, kind):
    """hot: random SU(3); warm: the same pulled towards the identity."""
    hot = GaugeField(_geo(dims), "double").random_su3_(
        seed=500 + sum(dims)).to_complex().contiguous()
    if kind == "hot":
        return hot
    return project_su3(EYE + 0.2 * (hot - EYE)).contiguous()


@functools.lru_cache(maxsize=None)
def _level(dims, kind, level):
    """(src, table, c0, c1, proj, reference, per-entry bound) on the CPU; the
    src of a HYP level is the reference of the level before it."""
    geo, u = _geo(dims), _field(dims, kind)
    if level.startswith("ape"):
        so = level == "ape3"
        src, table, proj = u, sm.ape_table(so), sm.PROJ_GS
        c0, c1 = sm.ape_coeffs(ALPHA_APE, so)
    else:
        n = int(level[-1]) - 1
        src = u if n == 0 else _level(dims, kind, f"hyp{n}")[5]
        table, proj = sm.hyp_tables()[n], sm.PROJ_POLAR
        c0, c1 = sm.hyp_coeffs(ALPHA_HYP)[n]
    ref, cond = sm.smear_level_reference(u, src, table, c0, c1, proj, True,
                                         geo=geo)
    w = max(1.0, c0 + 2 * max(r[1] for r in table) * c1)
    if proj == sm.PROJ_POLAR:
        bound = C_POLAR * U / cond[..., 2]
    else:
        bound = C_GS * U * w * w / (cond[..., 0] * cond[..., 1])
    return src, table, c0, c1, proj, ref, bound[..., None, None]


def _lat(dims):
    geo = _geo(dims)
    return list(dims), geo.parity_offset, geo.volume_cb


def _no_ext(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the HIP extension must not be touched here")
    monkeypatch.setattr(dispatch, "hip_ext", boom)


# CPU

@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("kind", ["hot", "warm"])
def test_tables_reproduce_the_torch_functions(monkeypatch, kind, dims):
    _no_ext(monkeypatch)
    geo, u = _geo(dims), _field(dims, kind)
    # hyp_smear: a few hundred u, an early level's rounding amplified by the
    # 1 / sigma_3 of the later ones
    amp = math.prod((_level(dims, kind, f"hyp{n}")[6] / (C_POLAR * U)
                     ).max().item() for n in (1, 2, 3))
    err = (_level(dims, kind, "hyp3")[5]
           - hyp_smear(u, geo, ALPHA_HYP)).abs().max().item()
    assert err <= 300 * U * amp
    for level, so in (("ape4", False), ("ape3", True)):
        got, bound = _level(dims, kind, level)[5:]
        want = ape_smear(u, geo, ALPHA_APE, spatial_only=so)
        assert ((got - want).abs() / (bound / C_GS)).max().item() <= 300
        if so:
            assert torch.equal(got[3], u[3])
    # no link of these seeds sits on the cube root's branch cut
    assert _branch_cut_count(dims, kind) == 0


def _branch_cut_count(dims, kind):
    """links of the three HYP levels whose polar factor has arg det within
    1e-6 of +-pi"""
    geo, u, count = _geo(dims), _field(dims, kind), 0
    for n in (1, 2, 3):
        src, table, c0, c1 = _level(dims, kind, f"hyp{n}")[:4]
        raw = sm.smear_level_reference(u, src, table, c0, c1, None, geo=geo)
        U_, _, Vh = torch.linalg.svd(raw)
        ang = torch.linalg.det(U_ @ Vh).angle().abs()
        count += int((math.pi - ang < 1e-6).sum())
    return count


def test_native_off_is_the_call_without_the_keyword(monkeypatch):
    monkeypatch.delenv("QUDA_AMD_NATIVE_LINK_SMEAR", raising=False)
    _no_ext(monkeypatch)
    dims = LATTICES[1]
    geo, u = _geo(dims), _field(dims, "warm")
    assert not sm.native_link_smear_default()
    for fn, args in ((hyp_smear, (ALPHA_HYP,)), (ape_smear, (ALPHA_APE,))):
        a = fn(u, geo, *args)
        assert torch.equal(a, fn(u, geo, *args, native=False))
        assert torch.equal(a, fn(u, geo, *args, native=None))
        assert torch.equal(a, fn(u, geo, *args, native=True))  # CPU tensor
    monkeypatch.setenv("QUDA_AMD_NATIVE_LINK_SMEAR", "1")
    assert sm.native_link_smear_default()
    assert not sm.link_smear_eligible(u)


# GPU

@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("kind", ["hot", "warm"])
@pytest.mark.parametrize("level", LEVELS)
def test_level_kernel_matches_reference(level, kind, dims):
    src, table, c0, c1, proj, ref, bound = _level(dims, kind, level)
    if proj == sm.PROJ_POLAR:
        assert _branch_cut_count(dims, kind) == 0
    out = torch.empty_like(ref).cuda()
    dispatch.hip_ext().smear_level(out, src.cuda(), _field(dims, kind).cuda(),
                                   *_lat(dims), table, c0, c1, proj)
    out = out.cpu()
    frac = ((out - ref).abs() / bound).max().item()
    print(f"level {level} {dims} {kind}: fraction {frac:.3e}")
    assert frac <= 1.0
    proj_rows = [o for o, r in enumerate(table) if r[1] > 0]
    W = out[proj_rows]
    assert (W @ W.conj().mT - EYE).abs().max().item() < 1e-14
    assert (torch.linalg.det(W) - 1).abs().max().item() < 1e-13
    for o, r in enumerate(table):
        if r[1] == 0:
            assert torch.equal(out[o], _field(dims, kind)[r[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("which", ["hyp", "ape4", "ape3"])
def test_smear_functions_native(monkeypatch, which, dims):
    geo, u = _geo(dims), _field(dims, "warm")
    if which == "hyp":
        def fn(x, **kw):
            return hyp_smear(x, geo, ALPHA_HYP, n_iter=2, **kw)
        levels = ["hyp1", "hyp2", "hyp3"]
    else:
        def fn(x, **kw):
            return ape_smear(x, geo, ALPHA_APE, n_iter=2,
                             spatial_only=which == "ape3", **kw)
        levels = [which]
    tol = 2 * sum(_level(dims, "warm", lv)[6].max().item() for lv in levels)
    ug = u.cuda()
    got = fn(ug, native=True)
    assert torch.equal(ug.cpu(), u)  # input untouched
    err = (got.cpu() - fn(u)).abs().max().item()
    print(f"{which} {dims}: err {err:.3e} tol {tol:.3e} "
          f"fraction {err / tol:.3e}")
    assert err <= tol
    assert torch.equal(got, fn(ug, native=True))
    # an ineligible field takes the torch code
    _no_ext(monkeypatch)
    u32 = fn(ug.to(torch.complex64), native=True)
    assert u32.dtype == torch.complex64 and u32.is_cuda


@pytest.mark.gpu
@pytest.mark.parametrize("epsilon", [-0.25, 1.0])
def test_over_improved_stout_native(epsilon):
    dims, rho = LATTICES[1], 0.06
    geo, u = _geo(dims), _field(dims, "warm")
    table = sm.over_improved_table(epsilon)
    L, n = table.max_len + 1, 5 * (table.max_len + 1) + table.n_paths + 10
    tol = rho * (2 * n * U * 3.0 ** ((L - 1) / 2.0)
                 * table.abs_coeff_sum()) + 1e-14
    got = over_improved_stout_smear(u.cuda(), geo, rho, epsilon=epsilon,
                                    native=True).cpu()
    err = (got - over_improved_stout_smear(u, geo, rho, epsilon=epsilon)
           ).abs().max().item()
    print(f"over-improved eps {epsilon}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    if epsilon == 1.0:
        assert (got - stout_smear(u, geo, rho)).abs().max().item() <= tol
