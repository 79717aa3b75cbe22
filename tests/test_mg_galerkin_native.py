"""Native HIP Galerkin coarse-operator build (csrc/galerkin.hip) against the
torch build_coarse_op it replaces.

CPU tests cover the flag, the eligibility rule, the tables (galerkin_tables)
and the pure-torch emulation that consumes exactly the kernel's operands
(ops.reference.galerkin_from_tables); GPU tests compare the kernel with the
torch build on the same Transfer.

Bound. Every entry of X is a sum of 9 terms, each over at most 6B outer
products whose right factor is itself a sum of at most 12 products; both
sides round, so

    |native - torch| <= 2 n u |M|_abs,   n = 54 B + 16,   u = 2^-53

with |M|_abs the torch build_coarse_op run on absolute values (|V|, |U|,
|A|, |P|, -|kappa|). Where the bound is exactly zero the two results must be
exactly equal. No tolerance here is tuned to the kernel's output.

Measured, as fractions of this bound (worst of Wilson and clover): the kernel
on an MI355X 1.3e-2 in case D, 3.7e-3 E, 1.7e-3 A, 5.1e-4 B, 9.9e-5 F,
6.1e-5 C; the emulation on the CPU 1.3e-2 in case D and less elsewhere.
"""

import functools
from types import SimpleNamespace

import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField
from quda_amd.fields.clover import CloverField
from quda_amd.fields.gauge import project_su3
from quda_amd.mg import MG, MGParam, Transfer, build_coarse_op
from quda_amd.mg import coarse as coarse_mod
from quda_amd.mg import galerkin as gk
from quda_amd.models import DiracClover, DiracWilson
from quda_amd.ops import dispatch
from quda_amd.ops import reference as ref

# case: (lattice, block, Nv)
CASES = {
    "A": ((4, 4, 4, 4), (2, 2, 2, 2), 4),    # coarse extent 2: fwd and bwd
                                             # neighbour aggregate coincide
    "B": ((4, 6, 2, 8), (2, 3, 2, 4), 6),    # Nv not 2^k; coarse extent 1 in z
    "C": ((4, 6, 2, 8), (4, 6, 2, 8), 8),    # one aggregate: faces wrap onto it
    "D": ((4, 6, 2, 8), (1, 3, 1, 1), 6),    # B=3; block extent 1: both faces
    "E": ((4, 6, 2, 8), (2, 2, 1, 2), 1),    # Nv=1
    "F": ((4, 4, 4, 8), (4, 4, 4, 4), 24),   # production Nv, B=256, Nc=48
}
CASE_IDS = sorted(CASES)
KINDS = ["wilson", "clover"]
KAPPA = 0.12
U = 2.0 ** -53


def _traced(fn):
    """(fn(), the dispatch ops it recorded)."""
    dispatch.set_trace(True)
    try:
        n0 = len(dispatch.trace_log())
        out = fn()
        ops = [op for op, _ in dispatch.trace_log()[n0:]]
    finally:
        dispatch.set_trace(False)
    return out, ops


def _su3(geo, seed):
    gen = torch.Generator().manual_seed(seed)
    m = torch.randn((4, 2, geo.volume_cb, 3, 3, 2), generator=gen,
                    dtype=torch.float64)
    return project_su3(torch.view_as_complex(m))


def _make_op(geo, u, kind, dev):
    g = GaugeField(geo, "double", dev).from_complex(u.to(dev))
    if kind == "wilson":
        return DiracWilson(g, KAPPA)
    A = ref.clover_matrix(u, geo, KAPPA, 1.0)
    cl = CloverField(geo, "double", dev).from_matrices(A.to(dev))
    return DiracClover(g, cl, KAPPA)


def _vectors(geo, nv, dev="cpu"):
    return [SpinorField(geo, "double").gaussian_(seed=700 + k).to(dev)
            for k in range(nv)]


@functools.lru_cache(maxsize=None)
def _cpu_transfer(case):
    dims, block, nv = CASES[case]
    geo = LatticeGeometry(dims)
    return geo, Transfer(geo, block, _vectors(geo, nv), native=False)


def _abs_build(op, t):
    """|M|_abs: the torch build on |V|, |U|, |A|, |P| and -|kappa|."""
    c128 = torch.complex128
    absu = op.gauge.to_complex().abs().to(c128)
    fake_op = SimpleNamespace(
        gauge=SimpleNamespace(to_complex=lambda: absu), kappa=-abs(op.kappa))
    if getattr(op, "clover", None) is not None:
        absa = op.clover.to_complex().abs().to(c128)
        fake_op.clover = SimpleNamespace(to_complex=lambda: absa)
    fake_t = SimpleNamespace(
        geo=t.geo, device=t.device, nvec=t.nvec, n_agg=t.n_agg,
        block_vol=t.block_vol, block=t.block, coarse_dims=t.coarse_dims,
        sites_by_agg=t.sites_by_agg, V=t.V.abs().to(c128))
    real = coarse_mod._gamma_tensors
    coarse_mod._gamma_tensors = lambda dev, dt: real(dev, dt).abs().to(dt)
    try:
        m = build_coarse_op(fake_op, fake_t, native=False)
    finally:
        coarse_mod._gamma_tensors = real
    return m.X.real, [y.real for y in m.Y]


@functools.lru_cache(maxsize=None)
def _cpu_case(case, kind):
    """(geo, transfer, op, torch build, bound tensors (X, [Y])), on the CPU,
    computed once and shared (never modified)."""
    geo, t = _cpu_transfer(case)
    op = _make_op(geo, _su3(geo, 31), kind, "cpu")
    want = build_coarse_op(op, t)
    aX, aY = _abs_build(op, t)
    f = 2 * (54 * t.block_vol + 16) * U
    return geo, t, op, want, (f * aX, [f * y for y in aY])


def _assert_within(got_X, got_Y, want, bound, what):
    """Every entry within the bound; exactly equal where the bound is 0."""
    worst = 0.0
    pairs = [("X", got_X, want.X, bound[0])] + [
        (f"Y[{d}]", got_Y[d], want.Y[d], bound[1][d]) for d in range(8)]
    for name, g, w, b in pairs:
        g, w, b = g.cpu(), w.cpu(), b.cpu()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        assert torch.isfinite(torch.view_as_real(g)).all(), (what, name)
        err = (g - w).abs()
        zero = b == 0
        assert torch.equal(g[zero], w[zero]), (what, name, "zero-bound entries")
        if (~zero).any():
            worst = max(worst, (err[~zero] / b[~zero]).max().item())
    print(f"{what}: max err/bound = {worst:.3e}")
    assert worst <= 1.0, (what, worst)


# ---------------------------------------------------------------------------
# CPU: flag, eligibility, tables, emulation
# ---------------------------------------------------------------------------
def _fake_gpu_transfer(dtype=torch.complex128):
    return SimpleNamespace(V=SimpleNamespace(
        device=SimpleNamespace(type="cuda"), dtype=dtype))


def test_flag_sources(monkeypatch):
    op = SimpleNamespace(gauge=None, kappa=KAPPA)
    t = _fake_gpu_transfer()
    monkeypatch.delenv("QUDA_AMD_MG_NATIVE_GALERKIN", raising=False)
    assert not gk.native_galerkin_default()
    assert not gk.galerkin_eligible(op, t)
    assert gk.galerkin_eligible(op, t, True)
    monkeypatch.setenv("QUDA_AMD_MG_NATIVE_GALERKIN", "1")
    assert gk.native_galerkin_default()
    assert gk.galerkin_eligible(op, t)
    assert gk.galerkin_eligible(op, t, None)
    assert not gk.galerkin_eligible(op, t, False)
    assert MGParam().native_galerkin is None
    assert MGParam(native_galerkin=True).native_galerkin is True
    # independent of the transfer flag
    assert MGParam(native_galerkin=True).native_transfer is None


def test_eligibility(monkeypatch):
    from quda_amd.parallel import comms
    op = SimpleNamespace(gauge=None, kappa=KAPPA)
    assert gk.galerkin_eligible(op, _fake_gpu_transfer(), True)
    assert not gk.galerkin_eligible(
        op, _fake_gpu_transfer(torch.complex64), True)
    assert not gk.galerkin_eligible(
        SimpleNamespace(kappa=KAPPA), _fake_gpu_transfer(), True)
    assert not gk.galerkin_eligible(
        SimpleNamespace(gauge=None), _fake_gpu_transfer(), True)
    _, t = _cpu_transfer("A")       # a CPU tensor
    assert not gk.galerkin_eligible(op, t, True)
    monkeypatch.setattr(comms, "comm_mask", lambda: 8)
    assert not gk.galerkin_eligible(op, _fake_gpu_transfer(), True)


@pytest.mark.parametrize("kind", KINDS)
def test_native_on_cpu_is_torch_bitwise(kind):
    geo, t, op, want, _ = _cpu_case("A", kind)
    got = build_coarse_op(op, t, native=True)
    assert got.native is False and want.native is False
    assert torch.equal(got.X, want.X)
    for d in range(8):
        assert torch.equal(got.Y[d], want.Y[d])
    dims, block, nv = CASES["A"]
    mg = MG(op, MGParam(block=block, n_vec=nv, native_galerkin=True),
            vectors=_vectors(geo, nv))
    assert mg.coarse_native is False
    assert torch.equal(mg.coarse.X, want.X)


@pytest.mark.parametrize("case", CASE_IDS)
def test_tables(case):
    dims, block, nv = CASES[case]
    geo, t = _cpu_transfer(case)
    nbr, bnd = gk.galerkin_tables(geo, block)
    G = geo.volume
    assert nbr.dtype == torch.int32 and tuple(nbr.shape) == (G, 8)
    assert bnd.dtype == torch.uint8 and tuple(bnd.shape) == (G,)
    assert nbr.is_contiguous()
    ar = torch.arange(G)
    nb = nbr.long()
    for d in range(8):              # every column is a permutation
        assert torch.equal(torch.sort(nb[:, d]).values, ar)
    for mu in range(4):             # bwd o fwd = fwd o bwd = identity
        assert torch.equal(nb[nb[:, 2 * mu + 1], 2 * mu], ar)
        assert torch.equal(nb[nb[:, 2 * mu], 2 * mu + 1], ar)
    # the (a, b) order of sites_by_agg: row r is lex site sites[r]
    sites = t.sites_by_agg.reshape(-1)
    ab_of_lex = torch.empty(G, dtype=torch.int64)
    ab_of_lex[sites] = ar
    c = geo.coords.long()[sites]
    for mu in range(4):
        for fwd in (0, 1):
            d = 2 * mu + fwd
            assert torch.equal(
                nb[:, d],
                ab_of_lex[geo.neighbor_lex(mu, 1 if fwd else -1)[sites]])
            edge = block[mu] - 1 if fwd else 0
            flag = (c[:, mu] % block[mu]) == edge
            assert torch.equal(((bnd.long() >> d) & 1) == 1, flag)
            if block[mu] == 1:
                assert flag.all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASE_IDS)
def test_emulation_matches_torch(case, kind):
    geo, t, op, want, bound = _cpu_case(case, kind)
    nbr, bnd = gk.galerkin_tables(geo, t.block)
    sites = t.sites_by_agg.reshape(-1)
    back = torch.stack([geo.neighbor_lex(mu, -1)[sites] for mu in range(4)])
    link, clov = gk.galerkin_operands(op, geo, sites, back)
    assert tuple(link.shape) == (geo.volume, 8, 3, 3)
    assert link.dtype == torch.complex128
    assert (clov is None) == (kind == "wilson")
    if clov is not None:
        assert tuple(clov.shape) == (geo.volume, 12, 12)
    X, Y = ref.galerkin_from_tables(t.V, nbr, bnd, link, clov, op.kappa)
    _assert_within(X, Y, want, bound, f"emulation {case}/{kind}")


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_case(case, kind):
    """(GPU transfer carrying the CPU case's V, GPU op, torch build on the
    GPU). The bound of _cpu_case applies: same V, U and A."""
    dims, block, nv = CASES[case]
    geo, t_cpu, _, _, _ = _cpu_case(case, kind)
    t = Transfer(geo, block, _vectors(geo, nv, "cuda"), native=False)
    t.V = t_cpu.V.cuda()
    op = _make_op(geo, _su3(geo, 31), kind, "cuda")
    want, ops = _traced(lambda: build_coarse_op(op, t, native=False))
    assert "galerkin_build" not in ops and want.native is False
    return t, op, want


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASE_IDS)
def test_native_matches_torch(case, kind):
    _, _, _, _, bound = _cpu_case(case, kind)
    t, op, want = _gpu_case(case, kind)
    got, ops = _traced(lambda: build_coarse_op(op, t, native=True))
    assert ops.count("galerkin_build") == 1     # the kernel ran, once
    assert got.native is True
    assert got.cd == want.cd and got.mask == 0
    _assert_within(got.X, got.Y, want, bound, f"native {case}/{kind}")
    # fixed summation order: a second build is bitwise the same
    again = build_coarse_op(op, t, native=True)
    assert torch.equal(again.X, got.X)
    for d in range(8):
        assert torch.equal(again.Y[d], got.Y[d])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASE_IDS)
def test_dispatch_writes_every_entry(case, kind):
    _, _, _, _, bound = _cpu_case(case, kind)
    t, op, want = _gpu_case(case, kind)
    nbr, bnd, sites, back = gk._tables_on(t.geo, t.block, t.V.device)
    link, clov = gk.galerkin_operands(op, t.geo, sites, back)
    coef = gk.hop_coefficients(op.kappa, t.V.device)
    Nc = 2 * t.nvec
    nan = complex(float("nan"), float("nan"))
    X = torch.full((t.n_agg, Nc, Nc), nan, dtype=torch.complex128,
                   device="cuda")
    Y = torch.full((8, t.n_agg, Nc, Nc), nan, dtype=torch.complex128,
                   device="cuda")
    (X2, Y2), ops = _traced(lambda: dispatch.galerkin_build(
        t.V, nbr, bnd, link, clov, coef, X=X, Y=Y))
    assert ops == ["galerkin_build"]
    assert X2 is X and Y2 is Y
    _assert_within(X, list(Y.unbind(0)), want, bound,
                   f"dispatch {case}/{kind}")


@functools.lru_cache(maxsize=None)
def _e2e_setup():
    from quda_amd.mg import generate_null_vectors
    geo = LatticeGeometry((8, 8, 8, 8))
    u = _su3(geo, 221).cuda()
    g = GaugeField(geo, "double", "cuda").from_complex(u)
    d = DiracWilson(g, 0.14)
    vecs = generate_null_vectors(d, 4, tol=1e-4, maxiter=200, seed=500)
    return geo, d, vecs


@pytest.mark.gpu
@pytest.mark.parametrize("native_transfer", [False, True])
def test_mg_end_to_end_native_galerkin(native_transfer):
    from quda_amd.solvers import gcr_solve
    geo, d, vecs = _e2e_setup()
    base = dict(block=(2, 2, 2, 2), n_vec=4, nu_post=4, null_tol=1e-4,
                null_maxiter=200, native_transfer=native_transfer)
    iters = {}
    for native in (True, False):
        mg, ops = _traced(lambda: MG(
            d, MGParam(native_galerkin=native, **base), vectors=vecs))
        assert mg.coarse_native == native
        assert ops.count("galerkin_build") == (1 if native else 0)
        assert mg.transfer.native_active == native_transfer
        if native:
            chk = mg.verify()
            assert chk["RP_identity"] < 1e-12, chk
            assert chk["galerkin"] < 1e-9, chk
        b = SpinorField(geo, "double", "cuda").gaussian_(seed=222)
        x = SpinorField(geo, "double", "cuda")
        st = gcr_solve(d, x, b, tol=1e-8, maxiter=300, nkrylov=16,
                       precond=mg.precond)
        assert st.converged
        iters[native] = st.iters
    assert abs(iters[True] - iters[False]) <= 1, iters
