"""Native clover-term construction (csrc/clover_term.hip) against
ops/reference.py field_strength / clover_matrix, torch.linalg.inv and
eigvalsh evaluated on the CPU in complex128.

Per-entry bounds, u = 2^-53, written before the first GPU run; the factor 2
is there because the oracle rounds too, and lmin, lmax (eigenvalues of A) and
fmax = max |F_ab| come from the reference alone.

F: a leaf is a chain of four unitary factors, three 3x3 products whose
complex 3-term dots cost at most 5 roundings each against the modulus
product: 15; adding four leaves 3, Q - Q^dag 1 (the scalings are powers of
two), the trace (two additions, a division) and its subtraction 4: n_F = 23.
An entry of a leaf's modulus product is at most sqrt(3)^4 = 9, and eight of
them (Q and Q^dag) carry 1/8: b_F = 2 u 23 * 9.
A: an entry is delta + coef * (at most four sigma-weighted F entries): three
additions, the scaling and the unit, 5 roundings on at most 1 + 4 coef fmax,
plus the error of F: b_A = 4 coef b_F + 2 u 5 (1 + 4 coef fmax).
A^-1: the L D L^dag factorisation, the triangular inverse and N^dag D^-1 N
are three passes of complex dots of at most 6 terms of three factors, at most
8 roundings a term: 144 roundings, a backward error that the solve scales by
cond(A) ||A^-1||; an entrywise error b_A of a 6x6 block has 2-norm at most
6 b_A and moves the inverse by ||A^-1||^2 times that:
b_inv = 2 u 144 (lmax/lmin) / lmin + 6 b_A / lmin^2.
tr log A, one parity: d log det = tr(A^-1 dA) over 12 pivots per site, each
with the relative error of the two terms above, then the logs and the sum of
12 Vcb terms: b_tl = Vcb 12 (6 b_A / lmin + 2 u 144 lmax/lmin)
+ 2 u (12 Vcb) sum |log lambda|.
Single precision adds one fp32 rounding of the double result, 2^-24 |ref|.
M psi: a row of a 6x6 block times psi, 6 b_A max|psi|, plus the roundings of
two applies of a 12-term complex dot and the hop term, 2 u 64 max|psi|.

Measured on an MI355X, worst fraction of the bound over the three lattices:
F 4.8e-3; A 7.7e-3; A^-1 1.8e-3; tr log A 1.6e-4; M psi 1.8e-3; csw 0 exact.
Single: 0.997 (A) and 0.992 (A^-1) of a tolerance that is the fp32 rounding
itself, the double part of it being 1e-6 of that.
"""

import functools

import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry
from quda_amd.fields import clover as cl
from quda_amd.fields.clover import CloverField, pack_clover
from quda_amd.gauge import fermion_force as ff
from quda_amd.ops import dispatch
from quda_amd.ops import reference as ref

U = 2.0 ** -53
KAPPA = 0.115
LATTICES = [(2, 2, 2, 2), (4, 6, 2, 6), (4, 4, 4, 4)]


@functools.lru_cache(maxsize=None)
def _geo(dims):
    return LatticeGeometry(dims)


@functools.lru_cache(maxsize=None)
def _field(dims, device="cpu"):
    u = GaugeField(_geo(dims), "double").random_su3_(
        seed=2000 + sum(dims)).to_complex()
    return u.to(device).contiguous()


@functools.lru_cache(maxsize=None)
def _fref(dims):
    F = ref.field_strength(_field(dims), _geo(dims))
    return torch.stack([F[k] for k in sorted(F)])


@functools.lru_cache(maxsize=None)
def _oracle(dims, csw):
    """(packed A, packed A^-1, eigenvalues [2, V, 12]) on the CPU, once."""
    A = ref.clover_matrix(_field(dims), _geo(dims), KAPPA, csw)
    Ai = torch.zeros_like(A)
    ev = []
    for b in range(2):
        blk = A[..., 6 * b:6 * b + 6, 6 * b:6 * b + 6]
        Ai[..., 6 * b:6 * b + 6, 6 * b:6 * b + 6] = torch.linalg.inv(blk)
        ev.append(torch.linalg.eigvalsh(blk))
    return pack_clover(A), pack_clover(Ai), torch.cat(ev, -1)


def bounds(dims, csw):
    """(b_F, b_A, b_inv, b_tl) of the module docstring."""
    ev = _oracle(dims, csw)[2]
    lmin, lmax = ev.min().item(), ev.max().item()
    coef, fmax = abs(KAPPA * csw), _fref(dims).abs().max().item()
    b_F = 2 * U * 23 * 9
    b_A = 4 * coef * b_F + 2 * U * 5 * (1 + 4 * coef * fmax)
    b_inv = 2 * U * 144 * (lmax / lmin) / lmin + 6 * b_A / lmin ** 2
    V = _geo(dims).volume_cb
    b_tl = (V * 12 * (6 * b_A / lmin + 2 * U * 144 * lmax / lmin)
            + 2 * U * 12 * V * ev.abs().log().abs().sum((1, 2)).max().item())
    return b_F, b_A, b_inv, b_tl


def _no_ext(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the HIP extension must not be touched here")
    monkeypatch.setattr(dispatch, "hip_ext", boom)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["cpu", "complex64", "half", "flag off"])
def test_ineligible_calls_take_the_torch_path(monkeypatch, case):
    _no_ext(monkeypatch)
    monkeypatch.delenv("QUDA_AMD_NATIVE_CLOVER", raising=False)
    dims = LATTICES[0]
    geo, u = _geo(dims), _field(dims)
    # stand in for a GPU tensor where the device is all that is in the way
    gpu = torch.device("cuda", 0)
    as_gpu = type("T", (torch.Tensor,), {"device": property(lambda s: gpu)})
    f = CloverField(geo, "half" if case == "half" else "double")
    f_gpu = type("F", (), {"precision": f.precision, "device": gpu})()
    ok_gpu = type("F", (), {"precision": "double", "device": gpu})()
    assert cl.clover_term_eligible(u.as_subclass(as_gpu), ok_gpu, True)
    if case == "complex64":
        u = u.to(torch.complex64)
    native = None if case == "flag off" else True
    assert not cl.clover_term_eligible(
        u if case == "cpu" else u.as_subclass(as_gpu),
        f if case == "cpu" else f_gpu, native)
    assert f.from_gauge(u, KAPPA, 1.3, native=native) is f
    A = ref.clover_matrix(u, geo, KAPPA, 1.3)
    want = CloverField(geo, f.precision).from_matrices(A)
    assert torch.equal(f.data, want.data)
    assert torch.equal(f.inv_data, want.inv_data)


def test_trlog_on_the_torch_path_is_the_eigenvalue_sum():
    dims = LATTICES[1]
    f = CloverField(_geo(dims), "double").from_gauge(_field(dims), KAPPA, 1.3)
    want = _oracle(dims, 1.3)[2].log().sum((1, 2))
    b_tl = bounds(dims, 1.3)[3]
    assert abs(f.trlog[0] - want[0].item()) <= b_tl
    assert abs(f.trlog[1] - want[1].item()) <= b_tl


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
def test_native_field_strength(dims):
    geo, u = _geo(dims), _field(dims, "cuda")
    F = torch.full((6, 2, geo.volume_cb, 3, 3), float("nan"),
                   dtype=u.dtype, device="cuda")
    CloverField(geo, "double", "cuda").from_gauge(u, KAPPA, 1.3, native=True,
                                                  fmunu=F)
    b_F = bounds(dims, 1.3)[0]
    err = (F.cpu() - _fref(dims)).abs().amax((1, 2, 3, 4))
    print(f"F {dims}: per-plane err {err.tolist()} bound {b_F:.3e} "
          f"fraction {err.max().item() / b_F:.3e}")
    assert bool((err <= b_F).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dims,csw,prec", [
    (d, c, "double") for d in LATTICES for c in (0.0, 1.3)
] + [(LATTICES[1], 1.3, "single")], ids=str)
def test_native_packed_clover_inverse_and_trlog(dims, csw, prec):
    geo, u = _geo(dims), _field(dims, "cuda")
    pA, pAi, ev = _oracle(dims, csw)
    assert ev.min().item() > 0.5
    f = CloverField(geo, prec, "cuda")
    assert cl.clover_term_eligible(u, f, True)
    te, to, bad = dispatch.clover_term(u, geo, KAPPA, csw, f)
    assert bad == 0
    _, b_A, b_inv, b_tl = bounds(dims, csw)
    w = 4 if prec == "single" else 2
    for name, got, want, b in (("A", f.data, pA, b_A),
                               ("A^-1", f.inv_data, pAi, b_inv)):
        # CloverField._to_native, kept in double
        want = want.reshape(2, geo.volume_cb, -1, w).movedim(2, 1)
        assert got.shape == (2, 72 // w, geo.volume_cb, w)
        tol = b + (2.0 ** -24 * want.abs() if prec == "single" else 0.0)
        err = (got.cpu().double() - want).abs()
        print(f"{name} {dims} csw={csw} {prec}: err {err.max().item():.3e} "
              f"bound {b:.3e} fraction {(err / tol).max().item():.3e}")
        assert bool((err <= tol).all())
        if csw == 0.0:
            assert torch.equal(got.cpu().double(), want)  # the identity
    want_tl = ev.log().sum((1, 2))
    err = max(abs(te - want_tl[0].item()), abs(to - want_tl[1].item()))
    print(f"trlog {dims} csw={csw} {prec}: ({te}, {to}) err {err:.3e} "
          f"bound {b_tl:.3e} fraction {err / b_tl:.3e}")
    assert err <= b_tl
    if csw == 0.0:
        assert te == 0.0 and to == 0.0
    # bitwise repeatable, through from_gauge as well
    g = CloverField(geo, prec, "cuda").from_gauge(u, KAPPA, csw, native=True)
    assert g.trlog == (te, to)
    assert torch.equal(g.data, f.data) and torch.equal(g.inv_data, f.inv_data)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
def test_indefinite_clover_falls_back_to_torch(dims):
    geo, u = _geo(dims), _field(dims, "cuda")
    assert _oracle(dims, 8.0)[2].min().item() < 0.0
    f = CloverField(geo, "double", "cuda")
    assert dispatch.clover_term(u, geo, KAPPA, 8.0, f)[2] > 0
    f.from_gauge(u, KAPPA, 8.0, native=True)
    t = CloverField(geo, "double", "cuda").from_gauge(u, KAPPA, 8.0,
                                                      native=False)
    assert torch.equal(f.data, t.data)
    assert torch.equal(f.inv_data, t.inv_data) and f.trlog == t.trlog


@pytest.mark.gpu
def test_native_end_to_end(monkeypatch):
    from quda_amd import api
    from quda_amd.models import DiracClover
    from quda_amd.api import DslashType, GaugeParam, InvertParam
    dims, csw = LATTICES[1], 1.3
    geo, u = _geo(dims), _field(dims, "cuda")
    api.init_quda()
    api.load_gauge_quda(u, GaugeParam(X=dims, device="cuda",
                                      cuda_prec="double",
                                      cuda_prec_sloppy="single"))
    p = InvertParam(dslash_type=DslashType.CLOVER, clover_csw=csw,
                    kappa=KAPPA)
    out = []
    for native in (True, False):
        api.load_clover_quda(p, native=native)
        d = DiracClover(api._R.gauge, api._R.clover, KAPPA)
        psi, y = d.new_spinor(n_parity=2), d.new_spinor(n_parity=2)
        psi.gaussian_(seed=5)
        d.M(y, psi)
        out.append((y.to_complex(), api._R.clover.trlog,
                    api._R.clover_sloppy.data.clone()))
    pmax = psi.to_complex().abs().max().item()
    _, b_A, _, b_tl = bounds(dims, csw)
    bound = (6 * b_A + 2 * U * 64) * pmax
    err = (out[0][0] - out[1][0]).abs().max().item()
    print(f"M psi: err {err:.3e} bound {bound:.3e} fraction {err / bound:.3e}")
    assert err <= bound
    assert max(abs(a - b) for a, b in zip(out[0][1], out[1][1])) <= b_tl
    assert (out[0][2].double() - out[1][2].double()).abs().max().item() \
        <= b_A + 2.0 ** -23 * out[1][2].abs().max().item()
    api.end_quda()
    # with both switches on a force evaluation never builds A in torch
    phi = ff.pseudofermion_refresh(d, seed=3)
    monkeypatch.setenv("QUDA_AMD_NATIVE_CLOVER", "1")

    def boom(*a, **k):
        raise AssertionError("clover_matrix must not be called")
    monkeypatch.setattr(ref, "clover_matrix", boom)
    S, F = ff.clover_fermion_force(u, geo, KAPPA, csw, phi, native=True)
    assert S > 0 and bool(torch.isfinite(F).all())
