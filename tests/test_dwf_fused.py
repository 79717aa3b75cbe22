"""Fused domain-wall kernel (4-d hop + dense per-chirality s-stage in one
launch): dispatch op, operator wiring, fallbacks.

Tolerances are tests/test_gpu_kernels.py::TOL — maximum absolute error on
unit-variance input."""
import math

import numpy as np
import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField
from quda_amd.models.dwf import (DiracDomainWallPC, DiracMobius,
                                 DiracMobiusPC)
from quda_amd.ops import blas
from quda_amd.ops import reference as ref
from quda_amd.ops.dispatch import (dslash_wilson_slices, dwf_fused_op,
                                   dwf_fused_supported, hip_ext)
from quda_amd.solvers import cgnr_solve

TOL = {"double": 1e-12, "single": 2e-5, "half": 2e-2}
RECONS = {"double": [18], "single": [18, 12], "half": [12, 18]}
RECON_NAME = {18: "none", 12: "twelve"}
MF, M5 = 0.04, 1.8
LATTICES = {"4444": (4, 4, 4, 4), "6664": (6, 6, 6, 4)}  # Vcb 128 / 432

_cache = {}


def _geo(name):
    if ("geo", name) not in _cache:
        geo = LatticeGeometry(LATTICES[name])
        g = GaugeField(geo, "double").random_su3_(seed=401)
        _cache[("geo", name)] = (geo, g, g.to_complex())
    return _cache[("geo", name)]


def _gauge_gpu(name, prec, recon=18):
    key = ("ggpu", name, prec, recon)
    if key not in _cache:
        geo, _, u = _geo(name)
        _cache[key] = GaugeField(geo, prec, "cuda",
                                 reconstruct=RECON_NAME[recon]).from_complex(
                                     u.cuda())
    return _cache[key]


def _spinor(name, Ls, seed):
    """Seeded double CPU 5-d single-parity field (shared, never modified)."""
    key = ("psi", name, Ls, seed)
    if key not in _cache:
        geo = _geo(name)[0]
        _cache[key] = SpinorField(geo, "double", n_parity=1,
                                  ls=Ls).gaussian_(seed=seed)
    return _cache[key]


def _to_gpu(f, prec):
    return SpinorField(f.geo, prec, "cuda", n_parity=f.n_parity,
                       ls=f.ls).from_complex(f.to_complex().cuda())


def _rand_w(Ls, seed=7):
    """Dense W_u != W_l, entries N(0,1)/sqrt(Ls)."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.normal(size=(2, Ls, Ls)) / math.sqrt(Ls))


def _oracle(name, Ls, parity, dagger, W, a, xpay, prec="double"):
    """'oracle Dhat per slice, then dense matrix per chirality' in double,
    computed once per case from the values the `prec` fields actually hold
    (so the storage rounding of the inputs is not charged to the kernel)."""
    key = ("oracle", name, Ls, parity, dagger, W is not None, a, xpay, prec)
    if key in _cache:
        return _cache[key]
    geo, _, u = _geo(name)

    def held(seed):
        f = _spinor(name, Ls, seed)
        if prec == "double":
            return f.to_complex()[0]
        return SpinorField(geo, prec, n_parity=1, ls=Ls).from_complex(
            f.to_complex()).to_complex()[0]

    psi = held(402)
    V = geo.volume_cb
    hop = torch.cat([ref.dslash_wilson_parity(u, psi[s * V:(s + 1) * V], geo,
                                              parity, dagger)
                     for s in range(Ls)])
    if W is not None:
        v = hop.reshape(Ls, V, 4, 3)
        Wc = W.to(hop.dtype)
        res = torch.empty_like(v)
        res[:, :, 0:2] = torch.einsum("st,tvxc->svxc", Wc[0], v[:, :, 0:2])
        res[:, :, 2:4] = torch.einsum("st,tvxc->svxc", Wc[1], v[:, :, 2:4])
        hop = res.reshape(Ls * V, 4, 3)
    res = a * hop
    if xpay:
        res = held(403) + res
    _cache[key] = res
    return res


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("xpay", [False, True])
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("dagger", [False, True])
def test_fused_op_cpu_vs_oracle(dagger, parity, xpay):
    name, Ls, a = "4444", 5, -0.37
    geo, g, _ = _geo(name)
    W = _rand_w(Ls)
    inp = _spinor(name, Ls, 402)
    x = _spinor(name, Ls, 403) if xpay else None
    out = SpinorField(geo, "double", n_parity=1, ls=Ls)
    dwf_fused_op(out, inp, g, parity, dagger=dagger, W=W, a=a, x=x)
    want = _oracle(name, Ls, parity, dagger, W, a, xpay)
    err = (out.to_complex()[0] - want).abs().max().item()
    assert err < 1e-12, err


@pytest.mark.parametrize("b5,c5", [(1.5, 0.5), (1.0, 0.0)])
def test_s_matrices_compose(b5, c5):
    Ls = 6
    geo, g, _ = _geo("4444")
    d = DiracMobiusPC(g, MF, M5, Ls, b5=b5, c5=c5)
    m = d.s_mats
    psi = _spinor("4444", Ls, 404).to_complex()[0]
    al, be = d.alpha, d.beta

    def close(W, want):
        got = ref.apply_s_matrix(psi, Ls, W)
        err = (got - want).abs().max().item()
        assert err < 1e-12, err

    for W in m.values():
        assert W.dtype == torch.float64 and tuple(W.shape) == (2, Ls, Ls)
    close(m["A"], ref.dslash5(psi, Ls, al, be, MF))
    close(m["B"], ref.dslash5(psi, Ls, b5, c5, MF))
    close(m["Ainv"], ref.m5inv(psi, Ls, al, be, MF))
    close(m["BAinv"], ref.dslash5(ref.m5inv(psi, Ls, al, be, MF), Ls, b5,
                                  c5, MF))
    close(m["Adag"], ref.dslash5(psi, Ls, al, be, MF, dagger=True))
    close(m["Bdag"], ref.dslash5(psi, Ls, b5, c5, MF, dagger=True))
    close(m["Ainvdag"], ref.m5inv(psi, Ls, al, be, MF, dagger=True))
    close(m["AinvdagBdag"],
          ref.m5inv(ref.dslash5(psi, Ls, b5, c5, MF, dagger=True), Ls, al,
                    be, MF, dagger=True))


def _op_pair(cls, g, Ls, **kw):
    return cls(g, MF, M5, Ls, fused=False, **kw), cls(g, MF, M5, Ls,
                                                      fused=True, **kw)


def _apply_all(op, inp, with_mdagm=True):
    res = []
    for dagger in (False, True):
        o = inp.clone_empty()
        op.M(o, inp, dagger=dagger)
        res.append(o.to_complex())
    if with_mdagm:
        o, tmp = inp.clone_empty(), inp.clone_empty()
        op.MdagM(o, inp, tmp)
        res.append(o.to_complex())
    return res


@pytest.mark.parametrize("cls,npar", [(DiracMobiusPC, 1), (DiracMobius, 2),
                                      (DiracDomainWallPC, 1)])
def test_fused_operators_cpu(cls, npar):
    Ls = 6
    geo, g, _ = _geo("4444")
    plain, fused = _op_pair(cls, g, Ls)
    assert fused.fused and not plain.fused
    inp = SpinorField(geo, "double", n_parity=npar, ls=Ls).gaussian_(seed=405)
    for a, b in zip(_apply_all(plain, inp), _apply_all(fused, inp)):
        err = (a - b).abs().max().item()
        assert err < 1e-11, err


def test_fused_default_off_and_env(monkeypatch):
    _, g, _ = _geo("4444")
    monkeypatch.delenv("QUDA_AMD_DWF_FUSED", raising=False)
    assert not DiracMobiusPC(g, MF, M5, 4).fused
    monkeypatch.setenv("QUDA_AMD_DWF_FUSED", "0")
    assert not DiracMobiusPC(g, MF, M5, 4).fused
    monkeypatch.setenv("QUDA_AMD_DWF_FUSED", "1")
    assert DiracMobiusPC(g, MF, M5, 4).fused
    assert not DiracMobiusPC(g, MF, M5, 4, fused=False).fused
    assert not dwf_fused_supported(
        SpinorField(g.geo, "double", n_parity=1, ls=4), g)  # CPU fields


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "single", "half"])
def test_fused_hop_only_gpu(prec):
    """W=None against dslash_wilson_slices on the same GPU fields; odd Ls
    on a lattice whose last tile has a tail."""
    name, Ls, a = "6664", 5, -0.37
    geo = _geo(name)[0]
    inp = _to_gpu(_spinor(name, Ls, 402), prec)
    x = _to_gpu(_spinor(name, Ls, 403), prec)
    for recon in RECONS[prec]:
        g = _gauge_gpu(name, prec, recon)
        assert dwf_fused_supported(inp, g)
        for dagger in (False, True):
            for parity in (0, 1):
                for xf in (None, x):
                    want = SpinorField(geo, prec, "cuda", n_parity=1, ls=Ls)
                    got = SpinorField(geo, prec, "cuda", n_parity=1, ls=Ls)
                    dslash_wilson_slices(want, inp, g, parity, dagger, a=a,
                                         x=xf)
                    dwf_fused_op(got, inp, g, parity, dagger=dagger, a=a,
                                 x=xf)
                    err = (got.to_complex()
                           - want.to_complex()).abs().max().item()
                    print(prec, recon, dagger, parity, xf is not None, err)
                    assert err < TOL[prec], (recon, dagger, parity, err)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "single", "half"])
@pytest.mark.parametrize("Ls", [4, 5, 16])
@pytest.mark.parametrize("name", ["4444", "6664"])
def test_fused_dense_gpu_vs_oracle(name, Ls, prec):
    """Random dense W_u != W_l against the double CPU oracle."""
    geo = _geo(name)[0]
    W = _rand_w(Ls)
    a = -0.37
    inp = _to_gpu(_spinor(name, Ls, 402), prec)
    x = _to_gpu(_spinor(name, Ls, 403), prec)
    g = _gauge_gpu(name, prec)
    for dagger, parity, xpay in [(False, 0, False), (True, 1, True)]:
        want = _oracle(name, Ls, parity, dagger, W, a, xpay, prec)
        got = SpinorField(geo, prec, "cuda", n_parity=1, ls=Ls)
        dwf_fused_op(got, inp, g, parity, dagger=dagger, W=W, a=a,
                     x=x if xpay else None)
        err = (got.to_complex()[0].cpu() - want).abs().max().item()
        print(name, Ls, prec, dagger, parity, xpay, "fused", err)
        if prec == "half":
            # unfused half path: hop stored in half, then the dense stage
            tmp = SpinorField(geo, prec, "cuda", n_parity=1, ls=Ls)
            dslash_wilson_slices(tmp, inp, g, parity, dagger)
            res = a * ref.apply_s_matrix(tmp.to_complex()[0], Ls, W)
            if xpay:
                res = x.to_complex()[0] + res
            unf = SpinorField(geo, prec, "cuda", n_parity=1, ls=Ls)
            unf.from_complex(res.unsqueeze(0))
            err_u = (unf.to_complex()[0].cpu() - want).abs().max().item()
            print(name, Ls, prec, dagger, parity, xpay, "unfused", err_u)
            assert err_u < TOL[prec], err_u
            assert err <= err_u, (err, err_u)
        assert err < TOL[prec], err


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["single", "half"])
def test_fused_wide_tile_gpu(prec):
    """The selectable 32-site tile (512 threads at Ls=16) on the lattice
    with a tile tail; same oracle and tolerance as the default tile."""
    ext = hip_ext()
    name, a = "6664", -0.37
    geo = _geo(name)[0]
    try:
        ext.set_dwf_fused_ns(32)
        for Ls, recon in [(5, 12), (16, 18)]:
            W = _rand_w(Ls)
            g = _gauge_gpu(name, prec, recon)
            inp = _to_gpu(_spinor(name, Ls, 402), prec)
            x = _to_gpu(_spinor(name, Ls, 403), prec)
            want = _oracle(name, Ls, 1, True, W, a, True, prec)
            got = SpinorField(geo, prec, "cuda", n_parity=1, ls=Ls)
            dwf_fused_op(got, inp, g, 1, dagger=True, W=W, a=a, x=x)
            err = (got.to_complex()[0].cpu() - want).abs().max().item()
            print(prec, Ls, recon, err)
            assert err < TOL[prec], (Ls, recon, err)
    finally:
        ext.set_dwf_fused_ns(16)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "single", "half"])
@pytest.mark.parametrize("cls,npar", [(DiracMobiusPC, 1),
                                      (DiracDomainWallPC, 1),
                                      (DiracMobius, 2)])
def test_fused_operators_gpu(cls, npar, prec):
    Ls = 6
    geo = _geo("4444")[0]
    g = _gauge_gpu("4444", prec)
    plain, fused = _op_pair(cls, g, Ls)
    inp = SpinorField(geo, prec, "cuda", n_parity=npar,
                      ls=Ls).gaussian_(seed=405)
    assert fused._use_fused(inp)
    ra = _apply_all(plain, inp, with_mdagm=npar == 1)
    rb = _apply_all(fused, inp, with_mdagm=npar == 1)
    for k, (a, b) in enumerate(zip(ra, rb)):
        err = (a - b).abs().max().item()
        print(cls.__name__, prec, k, err)
        assert err < TOL[prec], (k, err)


@pytest.mark.gpu
@pytest.mark.parametrize("cls,npar", [(DiracMobiusPC, 1), (DiracMobius, 2)])
def test_fused_adjoint_gpu(cls, npar):
    Ls = 6
    geo = _geo("4444")[0]
    op = cls(_gauge_gpu("4444", "double"), MF, M5, Ls, fused=True)
    a = SpinorField(geo, "double", "cuda", n_parity=npar,
                    ls=Ls).gaussian_(seed=406)
    b = SpinorField(geo, "double", "cuda", n_parity=npar,
                    ls=Ls).gaussian_(seed=407)
    Ma, Mdb = a.clone_empty(), a.clone_empty()
    op.M(Ma, a)
    op.M(Mdb, b, dagger=True)
    lhs = (b.to_complex().conj() * Ma.to_complex()).sum()
    rhs = (Mdb.to_complex().conj() * a.to_complex()).sum()
    assert abs(lhs - rhs) < 1e-10 * abs(lhs), (lhs, rhs)


@pytest.mark.gpu
def test_fused_mobius_pc_cg_gpu():
    """Setup of test_dwf.py::test_mobius_pc_cg_gpu with the fused operator;
    true residual recomputed with the unfused one."""
    geo = LatticeGeometry((8, 8, 8, 8))
    gen = torch.Generator().manual_seed(114)
    from quda_amd.fields.gauge import project_su3
    m = torch.randn((4, 2, geo.volume_cb, 3, 3, 2), generator=gen,
                    dtype=torch.float64)
    u = project_su3(torch.view_as_complex(m)).cuda()
    g = GaugeField(geo, "double", "cuda").from_complex(u)
    pc = DiracMobiusPC(g, MF, M5, 8, fused=True)
    b = SpinorField(geo, "double", "cuda", n_parity=1, ls=8).gaussian_(seed=115)
    x = SpinorField(geo, "double", "cuda", n_parity=1, ls=8)
    st = cgnr_solve(pc, x, b, tol=1e-8, maxiter=2000)
    assert st.converged
    r = SpinorField(geo, "double", "cuda", n_parity=1, ls=8)
    DiracMobiusPC(g, MF, M5, 8, fused=False).M(r, x)
    tr = math.sqrt(blas.xmy_norm2(b, r) / blas.norm2(b))
    assert tr <= 1e-7, tr


@pytest.mark.gpu
def test_fused_fallback_ls17_gpu():
    Ls = 17
    geo = _geo("4444")[0]
    g = _gauge_gpu("4444", "double")
    plain, fused = _op_pair(DiracMobiusPC, g, Ls)
    inp = SpinorField(geo, "double", "cuda", n_parity=1,
                      ls=Ls).gaussian_(seed=408)
    assert not dwf_fused_supported(inp, g)
    for a, b in zip(_apply_all(plain, inp), _apply_all(fused, inp)):
        assert (a - b).abs().max().item() < TOL["double"]
    # the op itself stays correct through the composed path
    W = _rand_w(Ls)
    out = SpinorField(geo, "double", "cuda", n_parity=1, ls=Ls)
    dwf_fused_op(out, inp, g, 1, W=W, a=0.5, x=inp)
    tmp = SpinorField(geo, "double", "cuda", n_parity=1, ls=Ls)
    dslash_wilson_slices(tmp, inp, g, 1)
    want = inp.to_complex()[0] + 0.5 * ref.apply_s_matrix(
        tmp.to_complex()[0], Ls, W)
    assert (out.to_complex()[0] - want).abs().max().item() < TOL["double"]


@pytest.mark.gpu
def test_fused_fallback_partitioned_gpu():
    from quda_amd.parallel import comms
    Ls = 6
    geo, _, u = _geo("4444")
    inp = SpinorField(geo, "double", "cuda", n_parity=2,
                      ls=Ls).gaussian_(seed=409)
    ref_out = _apply_all(
        DiracMobius(_gauge_gpu("4444", "double"), MF, M5, Ls, fused=False),
        inp, with_mdagm=False)
    try:
        comms.set_forced_partition(0b1111)
        g2 = GaugeField(geo, "double", "cuda").from_complex(u.cuda())
        assert not dwf_fused_supported(inp, g2)
        got = _apply_all(DiracMobius(g2, MF, M5, Ls, fused=True), inp,
                         with_mdagm=False)
    finally:
        comms.set_forced_partition(0)
    for a, b in zip(ref_out, got):
        assert (a - b).abs().max().item() < TOL["double"]


@pytest.mark.gpu
def test_fused_binding_rejects_bad_arguments_gpu():
    """Host-side validation: each of these raises before any launch."""
    ext = hip_ext()
    geo = _geo("4444")[0]
    g = _gauge_gpu("4444", "single")
    e = torch.empty(0, dtype=torch.float32, device="cuda")

    def call(out, inp, W, Ls):
        ext.dwf_fused(out.data, e, inp.data, e, g.data, out.data, e, W,
                      list(geo.dims), geo.parity_offset, geo.volume_cb, Ls,
                      0, False, False, 1.0, 18)

    def fields(Ls):
        return (SpinorField(geo, "single", "cuda", n_parity=1, ls=Ls),
                SpinorField(geo, "single", "cuda", n_parity=1, ls=Ls))

    o, i = fields(4)
    call(o, i, _rand_w(4), 4)  # the well-formed call goes through
    torch.cuda.synchronize()
    o17, i17 = fields(17)
    with pytest.raises(Exception, match="Ls"):
        call(o17, i17, None, 17)
    with pytest.raises(Exception, match="shape"):
        call(o, i, _rand_w(5), 4)
    with pytest.raises(Exception, match="float64"):
        call(o, i, _rand_w(4).float(), 4)
    with pytest.raises(Exception, match="alias"):
        call(o, o, None, 4)
    with pytest.raises(Exception, match="chunk stride"):
        call(o, i, None, 3)
    torch.cuda.synchronize()
