"""Native HIP multigrid transfer (csrc/transfer.hip): restrict, prolong and
block-orthonormalize against the torch transfer they replace.

CPU tests cover the table/repacking logic (transfer_tables, pack_vn and the
pure-torch emulations that consume exactly what the kernels read) and the
fallback rules; GPU tests compare the kernels with the torch path on the
same V under the standard forward-error bound

    |err| <= 2 n u (|V| . |x|)

with n the number of summed terms (6B for restrict, Nv for prolong), u the
unit round-off of the field's real type (2^-53 double, 2^-24 single) and
|V| . |x| the same contraction on absolute values in float64. No tolerance
here is tuned to the kernels' output.

That bound covers the arithmetic on given inputs. For single fields the
inputs are not the same on both sides: the kernels read V, and prolong the
coarse vector, rounded to complex64 (V is stored in the field's type), while
the torch path contracts the complex128 originals. Each such rounding
perturbs every term by at most u, i.e. the result by at most u (|V| . |x|),
whatever n is. The single-precision bound counts them explicitly:

    |err| <= (2 n + k) u (|V| . |x|),  k = 1 restrict (V), 2 prolong (V, coarse)

and k = 0 in double, where nothing is rounded on input. The term matters at
small n only. Measured on an MI355X, as fractions of these bounds: prolong at
Nv=1 (case E, n=1) 0.98 in double and 0.76 in single (3.04 u (|V| . |x|), of
which input rounding can account for 2 u); every other prolong case at most
0.33, every restrict case at most 0.09.
"""

import functools

import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField
from quda_amd.fields.geometry import checkerboard_join, checkerboard_split
from quda_amd.mg import MG, MGParam, Transfer, block_orthonormalize
from quda_amd.mg.transfer import pack_vn, transfer_tables
from quda_amd.ops import dispatch
from quda_amd.ops import reference as ref

# case: (lattice, block, Nv)
CASES = {
    "A": ((4, 4, 4, 4), (2, 2, 2, 2), 4),     # baseline, B=16
    "B": ((4, 6, 2, 8), (2, 3, 2, 4), 6),     # B=48, Nv not a power of two
    "C": ((4, 6, 2, 8), (4, 6, 2, 8), 24),    # one aggregate, B=384 > workgroup
    "D": ((4, 6, 2, 8), (1, 3, 1, 1), 6),     # B=3, uneven parity split, Na=128
    "E": ((4, 6, 2, 8), (2, 2, 1, 2), 1),     # Nv=1
}
CASE_IDS = sorted(CASES)
UNIT_ROUNDOFF = {"double": 2.0 ** -53, "single": 2.0 ** -24}
# inputs the kernel reads rounded to the field's type but the torch path does
# not (see the module docstring)
INPUT_ROUNDINGS = {"restrict": {"double": 0, "single": 1},
                   "prolong": {"double": 0, "single": 2}}


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


def _vectors(geo, nv, prec="double", dev="cpu", **kw):
    return [SpinorField(geo, prec, **kw).gaussian_(seed=700 + k).to(dev)
            for k in range(nv)]


def _field(geo, prec="double", dev="cpu"):
    return SpinorField(geo, prec).gaussian_(seed=9).to(dev)


@functools.lru_cache(maxsize=None)
def _cpu_case(case):
    dims, block, nv = CASES[case]
    geo = LatticeGeometry(dims)
    t = Transfer(geo, block, _vectors(geo, nv))
    return geo, block, nv, t


# ---------------------------------------------------------------------------
# CPU: flag handling, tables, repacking, fallbacks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B"])
def test_native_on_cpu_is_inactive_and_bitwise(case):
    geo, block, nv, t0 = _cpu_case(case)
    t1 = Transfer(geo, block, _vectors(geo, nv), native=True)
    assert t1.native and not t1.native_active
    assert not t0.native and not t0.native_active
    assert torch.equal(t0.V, t1.V)
    f = _field(geo)
    c0, c1 = t0.restrict(f), t1.restrict(f)
    assert torch.equal(c0, c1)
    o0 = t0.prolong(c0, SpinorField(geo))
    o1 = t1.prolong(c0, SpinorField(geo))
    assert torch.equal(o0.data, o1.data)


def test_native_flag_sources(monkeypatch):
    geo, block, nv, _ = _cpu_case("A")
    monkeypatch.setenv("QUDA_AMD_MG_NATIVE_TRANSFER", "1")
    assert Transfer(geo, block, _vectors(geo, nv)).native
    assert not Transfer(geo, block, _vectors(geo, nv), native=False).native
    monkeypatch.delenv("QUDA_AMD_MG_NATIVE_TRANSFER")
    assert not Transfer(geo, block, _vectors(geo, nv)).native
    assert MGParam().native_transfer is None
    assert MGParam(native_transfer=True).native_transfer is True


@pytest.mark.parametrize("case", CASE_IDS)
def test_site_tab_is_a_permutation(case):
    geo, block, nv, t = _cpu_case(case)
    agg_of_site, site_tab = transfer_tables(geo, block)
    assert agg_of_site.dtype == torch.int32 and site_tab.dtype == torch.int32
    assert tuple(site_tab.shape) == (t.n_agg, t.block_vol)
    assert tuple(agg_of_site.shape) == (geo.volume,)
    flat = site_tab.reshape(-1).long()
    assert torch.equal(torch.sort(flat).values, torch.arange(geo.volume))
    a_idx = torch.arange(t.n_agg).unsqueeze(1).expand_as(site_tab)
    assert torch.equal(agg_of_site.long()[site_tab.long()], a_idx)
    # same (a, b) order as sites_by_agg: g = parity*Vcb + cb
    g_of_lex = geo.parity.long() * geo.volume_cb + geo.cb_of_lex
    assert torch.equal(site_tab.long(), g_of_lex[t.sites_by_agg])


@pytest.mark.parametrize("case", CASE_IDS)
def test_tables_reproduce_transfer(case):
    geo, block, nv, t = _cpu_case(case)
    agg_of_site, site_tab = transfer_tables(geo, block)
    vn = pack_vn(t.V, site_tab, geo)
    assert tuple(vn.shape) == (2, 6, nv, geo.volume) and vn.is_contiguous()
    f = _field(geo)
    want = t.restrict(f)
    got = ref.restrict_from_tables(f.to_complex(), t.V, site_tab)
    assert (got - want).abs().max().item() <= 1e-13
    want_f = t.prolong(want, SpinorField(geo)).to_complex()
    got_f = ref.prolong_from_tables(want, vn, agg_of_site)
    assert (got_f - want_f).abs().max().item() <= 1e-13


def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:  # the torch path's own refusal is the oracle here
        return ("raise", type(e))


def _same_outcome(a, b):
    if a[0] != b[0]:
        return False
    return a[1] is b[1] if a[0] == "raise" else torch.equal(a[1], b[1])


def test_ineligible_inputs_fall_back():
    geo, block, nv, t0 = _cpu_case("D")
    t1 = Transfer(geo, block, _vectors(geo, nv), native=True)
    # half-precision field through a double transfer
    fh = _field(geo, "half")
    assert not t1._field_native_ok(fh)
    assert torch.equal(t1.restrict(fh), t0.restrict(fh))
    oh0 = t0.prolong(t0.restrict(fh), SpinorField(geo, "half"))
    oh1 = t1.prolong(t0.restrict(fh), SpinorField(geo, "half"))
    assert torch.equal(oh0.data, oh1.data) and torch.equal(oh0.norm, oh1.norm)
    # half-precision vectors
    th = Transfer(geo, block, _vectors(geo, nv, "half"), native=True)
    assert not th.native_active
    assert torch.equal(
        th.V, Transfer(geo, block, _vectors(geo, nv, "half")).V)
    # single-parity field: whatever the torch path does, native=True does too
    fp = _field(geo).parity_view(0)
    assert not t1._field_native_ok(fp)
    assert _same_outcome(_outcome(lambda: t1.restrict(fp)),
                         _outcome(lambda: t0.restrict(fp)))
    # B*6 < Nv (case D geometry with 24 vectors): dependent columns, torch path
    v24 = _vectors(geo, 24)
    tb = Transfer(geo, block, v24, native=True)
    assert not tb.native_active
    f = _field(geo)
    assert torch.equal(tb.restrict(f), Transfer(geo, block, v24).restrict(f))
    # nspin=1 vectors and fields
    fs = SpinorField(geo, nspin=1).gaussian_(seed=9)
    assert not t1._field_native_ok(fs)
    assert _same_outcome(_outcome(lambda: t1.restrict(fs)),
                         _outcome(lambda: t0.restrict(fs)))
    vs = _vectors(geo, nv, nspin=1)
    mk = [_outcome(lambda n=n: Transfer(geo, block, vs, native=n).V)
          for n in (True, False)]
    assert _same_outcome(*mk)
    # module-level function: native=True on a CPU tensor is the torch loop
    raw = torch.stack([checkerboard_join(v.to_complex(), geo)[t0.sites_by_agg]
                       for v in _vectors(geo, nv)], dim=-1)
    assert torch.equal(block_orthonormalize(raw, native=True),
                       block_orthonormalize(raw))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_case(case, prec):
    """(geo, torch-path transfer, native transfer on the SAME V, test field,
    a generic coarse vector). Built once per (case, precision)."""
    dims, block, nv = CASES[case]
    geo = LatticeGeometry(dims)
    vecs = _vectors(geo, nv, prec, "cuda")
    t0 = Transfer(geo, block, vecs, native=False)
    t1 = Transfer(geo, block, vecs, native=True)
    assert t1.native_active and not t0.native_active
    t1.V = t0.V            # same V: only the transfer arithmetic differs
    f = _field(geo, prec, "cuda")
    coarse = t0.restrict(f)
    return geo, t0, t1, f, coarse


def _abs_agg(t, f):
    """|psi| in aggregate order [Na, B, 4, 3], float64."""
    return checkerboard_join(f.to_complex().abs(), t.geo)[t.sites_by_agg]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("case", CASE_IDS)
def test_restrict_matches_torch(case, prec):
    geo, t0, t1, f, _ = _gpu_case(case, prec)
    want = t0.restrict(f)
    got, ops = _traced(lambda: t1.restrict(f))
    assert ops == ["transfer_restrict"]         # the kernel ran, not torch
    assert _traced(lambda: t0.restrict(f))[1] == []
    assert got.dtype == want.dtype and got.shape == want.shape
    n = 6 * t0.block_vol
    absV, absf = t0.V.abs(), _abs_agg(t0, f)
    bound = torch.empty_like(want.real)
    for chi, sl in ((0, slice(0, 2)), (1, slice(2, 4))):
        bound[:, chi, :] = torch.einsum("abscv,absc->av", absV[:, :, sl],
                                        absf[:, :, sl])
    bound = ((2 * n + INPUT_ROUNDINGS["restrict"][prec])
             * UNIT_ROUNDOFF[prec] * bound)
    err = (got - want).abs()
    ratio = (err / bound).max().item()
    print(f"restrict {case}/{prec}: max err/bound = {ratio:.3e}")
    assert ratio <= 1.0, (case, prec, ratio)
    # deterministic: a second call is bitwise the same
    assert torch.equal(t1.restrict(f), got)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("case", CASE_IDS)
def test_prolong_matches_torch(case, prec):
    geo, t0, t1, f, coarse = _gpu_case(case, prec)
    want = t0.prolong(coarse, SpinorField(geo, prec, "cuda")).to_complex()
    out = SpinorField(geo, prec, "cuda")
    out.data.fill_(float("nan"))  # every site must be written
    _, ops = _traced(lambda: t1.prolong(coarse, out))
    assert ops == ["transfer_prolong"]          # the kernel ran, not torch
    got = out.to_complex()
    nv = t0.nvec
    absV, absc = t0.V.abs(), coarse.abs()
    b_agg = torch.empty((t0.n_agg, t0.block_vol, 4, 3), dtype=torch.float64,
                        device="cuda")
    for chi, sl in ((0, slice(0, 2)), (1, slice(2, 4))):
        b_agg[:, :, sl] = torch.einsum("abscv,av->absc", absV[:, :, sl],
                                       absc[:, chi, :])
    lex = torch.empty((geo.volume, 4, 3), dtype=torch.float64, device="cuda")
    lex[t0.sites_by_agg.reshape(-1)] = b_agg.reshape(geo.volume, 4, 3)
    bound = ((2 * nv + INPUT_ROUNDINGS["prolong"][prec])
             * UNIT_ROUNDOFF[prec] * checkerboard_split(lex, geo))
    err = (got - want).abs()
    assert torch.isfinite(err).all()
    ratio = (err / bound).max().item()
    print(f"prolong {case}/{prec}: max err/bound = {ratio:.3e}")
    assert ratio <= 1.0, (case, prec, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_IDS)
def test_block_ortho_matches_torch(case):
    dims, block, nv = CASES[case]
    geo = LatticeGeometry(dims)
    _, t0, _, _, _ = _gpu_case(case, "double")
    raw = torch.stack([checkerboard_join(v.to_complex(), geo)[t0.sites_by_agg]
                       for v in _vectors(geo, nv, "double", "cuda")], dim=-1)
    keep = raw.clone()
    got, ops = _traced(lambda: block_orthonormalize(raw, native=True))
    assert ops == ["transfer_block_ortho"]      # the kernel ran, once
    assert torch.equal(raw, keep)               # input left alone
    want = block_orthonormalize(raw)
    Na, B = t0.n_agg, t0.block_vol
    eye = torch.eye(nv, dtype=got.dtype, device="cuda")
    for sl in (slice(0, 2), slice(2, 4)):
        W = got[:, :, sl].reshape(Na, 6 * B, nv)
        gram = torch.einsum("arv,arw->avw", W.conj(), W) - eye
        assert gram.abs().max().item() <= 1e-12
    tol = 100 * (6 * B) * UNIT_ROUNDOFF["double"] * 5
    diff = (got - want).abs().max().item()
    print(f"block-ortho {case}: max |native - torch| = {diff:.3e}, tol {tol:.3e}")
    assert diff <= tol, (case, diff, tol)


@pytest.mark.gpu
def test_mg_end_to_end_native_transfer():
    from quda_amd.fields.gauge import project_su3
    from quda_amd.mg import generate_null_vectors
    from quda_amd.models import DiracWilson
    from quda_amd.solvers import gcr_solve
    geo = LatticeGeometry((8, 8, 8, 8))
    gen = torch.Generator().manual_seed(221)
    m = torch.randn((4, 2, geo.volume_cb, 3, 3, 2), generator=gen,
                    dtype=torch.float64)
    u = project_su3(torch.view_as_complex(m)).cuda()
    g = GaugeField(geo, "double", "cuda").from_complex(u)
    d = DiracWilson(g, 0.14)
    base = dict(block=(2, 2, 2, 2), n_vec=4, nu_post=4, null_tol=1e-4,
                null_maxiter=200)
    vecs = generate_null_vectors(d, 4, tol=1e-4, maxiter=200, seed=500)
    iters = {}
    for native in (True, False):
        mg = MG(d, MGParam(native_transfer=native, **base), vectors=vecs)
        assert mg.transfer.native_active == native
        if native:
            chk = mg.verify()
            assert chk["RP_identity"] < 1e-12, chk
            assert chk["galerkin"] < 1e-9, chk
        b = SpinorField(geo, "double", "cuda").gaussian_(seed=222)
        x = SpinorField(geo, "double", "cuda")
        st, ops = _traced(lambda: gcr_solve(d, x, b, tol=1e-8, maxiter=300,
                                            nkrylov=16, precond=mg.precond))
        assert st.converged
        # the V-cycles ran the kernels, or (native off) never touched them
        for op in ("transfer_restrict", "transfer_prolong"):
            assert (op in ops) == native, (native, op)
        iters[native] = st.iters
    assert abs(iters[True] - iters[False]) <= 1, iters
