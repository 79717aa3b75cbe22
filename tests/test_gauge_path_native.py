"""Path-table gauge force, path product and loop traces: the tables of
gauge/paths.py, the torch oracle path_force_reference, and the HIP kernels
of csrc/gauge_path.hip against that oracle.

Force bound (per entry, u = 2^-53; L = links of the longest force product =
longest tail + 1, Np = tails per direction):

    |native - reference| <= 2 n u 3^((L-1)/2) (beta/6) max_mu sum_p |c_p|,
    n = 5 L + Np + 10

A complex 3-term dot product costs at most 5 roundings against the modulus
product; a chain of L unitary matrices has modulus-product entries of at
most 3^((L-1)/2); Np accumulations, TA and the scalings make up the rest;
the factor 2 is there because both sides round. The path-product mode drops
the 5 roundings of TA (difference, two trace additions, division by 3,
subtraction): n = 5 L + Np + 5, with |scale| in place of beta/6. A loop
trace of L links has entries bounded by 3^((L-1)/2) and three of them are
added: 2 (5 L + 3) u 3^((L+1)/2) per site. No tolerance here is tuned to the
kernel's output.

Measured on an MI355X, worst fraction of the force bound per action over the
three lattices: wilson 4.5e-3, symanzik 7.2e-4, iwasaki 7.2e-4, luscher_weisz
5.1e-4, asymmetric 3.3e-4; path product 1.4e-3; loop traces 1.1e-2 per site.
"""

import functools

import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry
from quda_amd.gauge import hmc, ops, paths
from quda_amd.gauge.paths import LoopAction
from quda_amd.ops import dispatch

U = 2.0 ** -53
BETA = 6.0
LATTICES = [(4, 6, 2, 6), (2, 2, 2, 2), (6, 6, 6, 6)]

# one coefficient negative, one loop that takes only backward steps first,
# an 8-link loop (7-step tails, the kernel's limit), a repeated direction
ASYM = LoopAction(
    [(1, 2, -1, -2), (-3, -4, 3, 4), (2, 4, 4, -2, -4, -4),
     (1, 1, 3, 3, -1, -1, -3, -3), (4, -1, -4, 1)],
    [0.7, -0.45, 0.2, 0.05, 0.3])

ACTIONS = {
    "wilson": LoopAction.wilson(),
    "symanzik": LoopAction.symanzik(),
    "iwasaki": LoopAction.iwasaki(),
    "luscher_weisz": LoopAction.luscher_weisz(-1.0 / 12.0, 0.03),
    "asymmetric": ASYM,
}


@functools.lru_cache(maxsize=None)
def _geo(dims):
    return LatticeGeometry(dims)


@functools.lru_cache(maxsize=None)
def _field(dims, device="cpu"):
    u = GaugeField(_geo(dims), "double").random_su3_(
        seed=1000 + sum(dims)).to_complex()
    return u.to(device).contiguous()


@functools.lru_cache(maxsize=None)
def _ref_force(dims, name, device):
    """path_force_reference on `device`, computed once per case."""
    return paths.path_force_reference(_field(dims, device), _geo(dims),
                                      ACTIONS[name], BETA)


def force_bound(table, scale, ta=True):
    L = table.max_len + 1
    n = 5 * L + table.n_paths + (10 if ta else 5)
    return (2 * n * U * 3.0 ** ((L - 1) / 2.0) * abs(scale)
            * table.abs_coeff_sum())


def _no_ext(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the HIP extension must not be touched here")
    monkeypatch.setattr(dispatch, "hip_ext", boom)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def test_table_structure():
    counts = {"wilson": 6, "symanzik": 24, "luscher_weisz": 48}
    for name, n in counts.items():
        t = paths.force_table(ACTIONS[name])
        assert [len(tl) for tl in t.tails] == [n] * 4, name
        assert t.n_paths == n
        assert tuple(t.steps.shape) == (4, n, 8)
        assert t.steps.dtype == torch.int8
        assert tuple(t.lengths.shape) == (4, n)
        assert t.lengths.dtype == torch.int32
        assert tuple(t.coeffs.shape) == (4, n)
        assert t.coeffs.dtype == torch.float64
    for name, act in ACTIONS.items():
        t = paths.force_table(act)
        assert paths.force_table(act) is t  # cached on the action
        for mu in range(4):
            want = tuple(-1 if d == mu else 0 for d in range(4))
            for k, (c, tail) in enumerate(t.tails[mu]):
                assert paths.displacement(tail) == want, (name, mu, tail)
                assert c != 0.0
                # the packed form holds the same table
                assert t.lengths[mu, k].item() == len(tail)
                assert t.coeffs[mu, k].item() == c
                assert tuple(t.steps[mu, k, :len(tail)].tolist()) == tail
                assert not t.steps[mu, k, len(tail):].any()
    # symanzik: each staple carries c0, each rectangle tail c1
    c1 = -1.0 / 12.0
    t = paths.force_table(ACTIONS["symanzik"])
    for mu in range(4):
        assert sorted(len(tl) for _, tl in t.tails[mu]) == [3] * 6 + [5] * 18
        for c, tail in t.tails[mu]:
            assert c == (1.0 - 8.0 * c1 if len(tail) == 3 else c1)
    # luscher_weisz: 24 parallelogram tails of coefficient c2 on top
    t = paths.force_table(ACTIONS["luscher_weisz"])
    for mu in range(4):
        par = [c for c, tail in t.tails[mu]
               if len(tail) == 5 and len({abs(s) for s in tail}) == 3]
        assert par == [0.03] * 24
    # c1 = 0 collapses to exactly the Wilson table; dbw2 keeps 24
    t0 = paths.force_table(LoopAction.symanzik(0.0))
    tw = paths.force_table(LoopAction.wilson())
    assert t0.tails == tw.tails
    assert torch.equal(t0.steps, tw.steps)
    assert torch.equal(t0.coeffs, tw.coeffs)
    assert paths.force_table(LoopAction.dbw2()).n_paths == 24
    assert LoopAction.dbw2().coeffs[-1] == -1.4069
    assert LoopAction.iwasaki().coeffs[-1] == -0.331
    with pytest.raises(ValueError):
        LoopAction([(1, 2, -1)], [1.0])  # does not close


@pytest.mark.parametrize("dims", LATTICES[:2], ids=str)
def test_reference_force_cross_checks(dims):
    geo, u = _geo(dims), _field(dims)
    F = paths.path_force_reference(u, geo, ACTIONS["wilson"], BETA)
    err = (F - ops.gauge_force(u, geo, BETA)).abs().max().item()
    bound = force_bound(paths.force_table(ACTIONS["wilson"]), BETA / 6.0)
    print(f"wilson {dims}: {err:.2e} of {bound:.2e}")
    assert err <= bound
    for c1 in (-1.0 / 12.0, -0.331):
        act = LoopAction.symanzik(c1)
        F = paths.path_force_reference(u, geo, act, BETA)
        Fa = ops.improved_gauge_force(u, geo, BETA, c1=c1)
        err = (F - Fa).abs().max().item()
        bound = force_bound(paths.force_table(act), BETA / 6.0)
        print(f"c1={c1:.3f} {dims}: {err:.2e} of {bound:.2e}")
        assert err <= bound


def test_reference_force_matches_api_path_force():
    """A user list with a loop that repeats a direction, against the autograd
    api entry."""
    from quda_amd import api
    from quda_amd.api import GaugeParam
    dims = LATTICES[0]
    geo, u = _geo(dims), _field(dims)
    try:
        api.load_gauge_quda(u, GaugeParam(X=dims, device="cpu",
                                          cuda_prec="double",
                                          cuda_prec_sloppy="double"))
        Fa = api.compute_gauge_path_force_quda(
            [list(p) for p in ASYM.loops], list(ASYM.coeffs), BETA)
    finally:
        api.free_gauge_quda()
    F = paths.path_force_reference(u, geo, ASYM, BETA)
    err = (F - Fa).abs().max().item()
    bound = force_bound(paths.force_table(ASYM), BETA / 6.0)
    print(f"api path force: {err:.2e} of {bound:.2e}")
    assert err <= bound


def test_loop_action_matches_existing_actions():
    dims = LATTICES[0]
    geo, u = _geo(dims), _field(dims)
    s = ops.loop_action(u, geo, LoopAction.wilson(), BETA)
    s0 = ops.gauge_action(u, geo, BETA)
    assert abs(s - s0) <= 1e-12 * abs(s0)
    for c1 in (-1.0 / 12.0, -0.331):
        s = ops.loop_action(u, geo, LoopAction.symanzik(c1), BETA)
        s0 = ops.improved_gauge_action(u, geo, BETA, c1=c1)
        assert abs(s - s0) <= 1e-12 * abs(s0)


def test_flag_off_is_unchanged_and_never_loads_the_extension(monkeypatch):
    monkeypatch.delenv("QUDA_AMD_NATIVE_GAUGE_FORCE", raising=False)
    assert not ops.native_gauge_force_default()
    monkeypatch.setenv("QUDA_AMD_NATIVE_GAUGE_FORCE", "1")
    assert ops.native_gauge_force_default()
    monkeypatch.delenv("QUDA_AMD_NATIVE_GAUGE_FORCE")
    _no_ext(monkeypatch)
    dims = LATTICES[1]
    geo, u = _geo(dims), _field(dims)
    assert torch.equal(ops.gauge_force(u, geo, BETA),
                       ops.gauge_force(u, geo, BETA))
    assert torch.equal(ops.improved_gauge_force(u, geo, BETA),
                       ops.improved_gauge_force(u, geo, BETA))
    P = hmc.random_momentum(geo, seed=5)
    a = hmc.leapfrog(u, P, geo, 5.5, 2, 0.05)
    b = hmc.leapfrog(u, P, geo, 5.5, 2, 0.05)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # with an action the CPU path is the analytic reference
    c = hmc.leapfrog(u, P, geo, 5.5, 2, 0.05, action=LoopAction.wilson())
    assert (c[0] - a[0]).abs().max().item() < 1e-12
    assert (c[1] - a[1]).abs().max().item() < 1e-12


LONG_LOOP = LoopAction([(1, 1, 1, 2, 2, -1, -1, -1, -2, -2)], [1.0])


def test_ineligible_calls_take_the_torch_path(monkeypatch):
    """The galerkin_eligible convention: an explicit native=True on an
    ineligible call runs the torch path; it is not an error."""
    _no_ext(monkeypatch)
    dims = LATTICES[0]
    geo, u = _geo(dims), _field(dims)
    assert not ops.gauge_native_eligible(u, True)             # CPU tensor
    assert not ops.gauge_native_eligible(u.to(torch.complex64), True)
    assert paths.force_table(LONG_LOOP).max_len == 9
    assert not paths.force_table(LONG_LOOP).native_ok          # 9-step tail
    assert paths.force_table(ACTIONS["luscher_weisz"]).native_ok
    assert not ops.loop_trace_eligible(u, LONG_LOOP.loops, True)
    F = ops.path_gauge_force(u, geo, ACTIONS["symanzik"], BETA, native=True)
    assert torch.equal(F, _ref_force(dims, "symanzik", "cpu"))
    P = hmc.random_momentum(geo, seed=6)
    P1 = ops.path_gauge_force(u, geo, ACTIONS["symanzik"], BETA, mom=P,
                              dt=0.37, native=True)
    assert P1 is not P and torch.equal(P1, P + 0.37 * F)
    u32 = u.to(torch.complex64)
    F32 = ops.path_gauge_force(u32, geo, ACTIONS["wilson"], BETA, native=True)
    assert F32.dtype == torch.complex64
    assert (F32 - _ref_force(dims, "wilson", "cpu")).abs().max() < 1e-4
    Fl = ops.path_gauge_force(u, geo, LONG_LOOP, BETA, native=True)
    assert torch.equal(Fl, paths.path_force_reference(u, geo, LONG_LOOP,
                                                      BETA))
    assert torch.equal(ops.gauge_force(u, geo, BETA, native=True),
                       ops.gauge_force(u, geo, BETA))
    lt = ops.loop_trace(u, geo, [(1, 4, -1, -4)], native=True)
    assert lt == ops.loop_trace(u, geo, [(1, 4, -1, -4)])


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("name", list(ACTIONS))
def test_native_force_matches_reference(name, dims):
    geo, u = _geo(dims), _field(dims, "cuda")
    table = paths.force_table(ACTIONS[name])
    assert ops.gauge_path_eligible(u, table, True)
    F = ops.path_gauge_force(u, geo, ACTIONS[name], BETA, native=True)
    Fr = _ref_force(dims, name, "cuda")
    err = (F - Fr).abs().max().item()
    bound = force_bound(table, BETA / 6.0)
    print(f"force {name} {dims}: err {err:.3e} bound {bound:.3e} "
          f"fraction {err / bound:.3e}")
    assert err <= bound
    # structure: traceless antihermitian, and bitwise repeatable
    fmax = F.abs().max().item()
    assert (F + F.conj().mT).abs().max().item() <= 4 * U * fmax
    tr = torch.diagonal(F, dim1=-2, dim2=-1).sum(-1)
    assert tr.abs().max().item() <= 4 * U * fmax
    F2 = ops.path_gauge_force(u, geo, ACTIONS[name], BETA, native=True)
    assert torch.equal(F, F2)


@pytest.mark.gpu
def test_native_flag_routes_the_existing_entry_points(monkeypatch):
    dims = LATTICES[0]
    geo, u = _geo(dims), _field(dims, "cuda")
    monkeypatch.setenv("QUDA_AMD_NATIVE_GAUGE_FORCE", "1")
    Fw = ops.gauge_force(u, geo, BETA)
    Fs = ops.improved_gauge_force(u, geo, BETA)
    monkeypatch.delenv("QUDA_AMD_NATIVE_GAUGE_FORCE")
    assert torch.equal(Fw, ops.path_gauge_force(
        u, geo, ACTIONS["wilson"], BETA, native=True))
    assert torch.equal(Fs, ops.path_gauge_force(
        u, geo, ACTIONS["symanzik"], BETA, native=True))
    # and against the parent's own paths, flag off
    bw = force_bound(paths.force_table(ACTIONS["wilson"]), BETA / 6.0)
    bs = force_bound(paths.force_table(ACTIONS["symanzik"]), BETA / 6.0)
    assert (Fw - ops.gauge_force(u, geo, BETA)).abs().max().item() <= bw
    assert (Fs - ops.improved_gauge_force(u, geo, BETA)
            ).abs().max().item() <= bs


def _absdiff_exact(mom, P, F, a):
    """|mom - (P + a F)| per entry with the right-hand side formed in
    extended precision on the host, so that only the kernel's own
    roundings are measured."""
    import numpy as np

    def ld(t):
        return torch.view_as_real(t.cpu()).numpy().astype(np.longdouble)

    d = ld(mom) - (ld(P) + np.longdouble(a) * ld(F))
    return torch.from_numpy(np.hypot(d[..., 0], d[..., 1]).astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
def test_native_fused_momentum_update(dims):
    geo, u = _geo(dims), _field(dims, "cuda")
    act, dt = ACTIONS["symanzik"], 0.37
    F = ops.path_gauge_force(u, geo, act, BETA, native=True)
    P = hmc.random_momentum(geo, "cuda", seed=11).contiguous()
    mom = P.clone()
    out = ops.path_gauge_force(u, geo, act, BETA, mom=mom, dt=dt, native=True)
    assert out is mom  # in place
    tol = 2 * U * (P.abs() + dt * F.abs()).cpu()
    assert bool((_absdiff_exact(mom, P, F, dt) <= tol).all())
    # a second call accumulates: the result moves by 2 dt F in all
    ops.path_gauge_force(u, geo, act, BETA, mom=mom, dt=dt, native=True)
    tol2 = 2 * U * (P.abs() + 2 * dt * F.abs()).cpu() + tol
    assert bool((_absdiff_exact(mom, P, F, 2 * dt) <= tol2).all())
    assert (mom - P).abs().max().item() > dt * F.abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
def test_native_path_product(dims):
    geo, u = _geo(dims), _field(dims, "cuda")
    scale = -0.8
    for name in ("symanzik", "asymmetric"):
        table = paths.force_table(ACTIONS[name])
        out = ops.path_gauge_product(u, geo, ACTIONS[name], scale,
                                     native=True)
        ref = paths.path_product_reference(u, geo, ACTIONS[name], scale)
        err = (out - ref).abs().max().item()
        bound = force_bound(table, scale, ta=False)
        print(f"path {name} {dims}: fraction {err / bound:.3e}")
        assert err <= bound
        # not antihermitian: TA was not applied
        assert (out + out.conj().mT).abs().max().item() > 1e-3
        # accumulate into a given tensor
        acc = ref.clone()
        res = ops.path_gauge_product(u, geo, ACTIONS[name], scale, out=acc,
                                     native=True)
        assert res is acc
        assert (acc - 2 * ref).abs().max().item() <= 2 * bound + 4 * U * (
            ref.abs().max().item())


TRACE_LOOPS = [(1, 4, -1, -4), (1, 1, 2, -1, -1, -2), (1, 2, 3, -1, -2, -3),
               (1, 1, 3, 3, -1, -1, -3, -3), (-4, -2, 4, 2)]


def site_trace_bound(L):
    return 2 * (5 * L + 3) * U * 3.0 ** ((L + 1) / 2.0)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", LATTICES, ids=str)
def test_native_loop_traces(dims):
    geo, u = _geo(dims), _field(dims, "cuda")
    assert ops.loop_trace_eligible(u, TRACE_LOOPS, True)
    tr = ops.loop_trace_sites(u, geo, TRACE_LOOPS)
    assert tuple(tr.shape) == (len(TRACE_LOOPS), 2, geo.volume_cb)
    assert torch.equal(tr, ops.loop_trace_sites(u, geo, TRACE_LOOPS))
    lo = geo.lex_of_cb.to(u.device)
    for k, loop in enumerate(TRACE_LOOPS):
        P = ops.path_product(u, geo, loop)
        ref_lex = torch.diagonal(P, dim1=-2, dim2=-1).sum(-1)
        ref = torch.stack([ref_lex[lo[0]], ref_lex[lo[1]]])
        err = (tr[k] - ref).abs().max().item()
        b_site = site_trace_bound(len(loop))
        print(f"trace {loop} {dims}: fraction {err / b_site:.3e}")
        assert err <= b_site
        lt = ops.loop_trace(u, geo, [loop], [0.7], native=True)
        lt0 = ops.loop_trace(u, geo, [loop], [0.7])
        b_sum = (b_site + 2 * geo.volume * U * 3) / 3.0
        assert abs(lt - lt0) <= 0.7 * b_sum
    for name in ("wilson", "symanzik"):
        s = ops.loop_action(u, geo, ACTIONS[name], BETA, native=True)
        s0 = ops.loop_action(u, geo, ACTIONS[name], BETA)
        assert abs(s - s0) <= 1e-12 * abs(s0)


@pytest.mark.gpu
def test_native_ineligible_on_gpu_takes_the_torch_path(monkeypatch):
    _no_ext(monkeypatch)
    dims = LATTICES[1]
    geo, u = _geo(dims), _field(dims, "cuda")
    u32 = u.to(torch.complex64)
    assert not ops.gauge_path_eligible(u32, ACTIONS["wilson"], True)
    assert not ops.gauge_path_eligible(u, LONG_LOOP, True)
    assert not ops.gauge_path_eligible(u, ACTIONS["wilson"], None)
    F32 = ops.path_gauge_force(u32, geo, ACTIONS["wilson"], BETA, native=True)
    assert F32.dtype == torch.complex64
    Fl = ops.path_gauge_force(u, geo, LONG_LOOP, BETA, native=True)
    assert torch.equal(Fl, paths.path_force_reference(u, geo, LONG_LOOP,
                                                      BETA))


@pytest.mark.gpu
def test_native_md_reversible_and_second_order():
    dims = (4, 4, 4, 4)
    geo, u = _geo(dims), _field(dims, "cuda")
    act, beta = ACTIONS["symanzik"], 5.5
    P = hmc.random_momentum(geo, "cuda", seed=21)

    def H(uc, Pc):
        return hmc.mom_action(Pc) + ops.loop_action(uc, geo, act, beta,
                                                    native=True)

    H0 = H(u, P)
    dH = []
    for n in (8, 16):
        u1, P1 = hmc.leapfrog(u, P, geo, beta, n, 0.3 / n, action=act,
                              native=True)
        dH.append(abs(H(u1, P1) - H0))
    print(f"dH at n_md 8, 16: {dH}")
    assert dH[1] < dH[0] / 2.5, dH
    ub, Pb = hmc.leapfrog(u1, -P1, geo, beta, 16, 0.3 / 16, action=act,
                          native=True)
    assert (ub - u).abs().max().item() < 1e-10
    assert (Pb + P).abs().max().item() < 1e-10
    # the caller's momentum is not the one updated in place
    assert torch.equal(P, hmc.random_momentum(geo, "cuda", seed=21))
    _, _, dh = hmc.hmc_trajectory(u, geo, beta, n_md=8, tau=0.3, seed=21,
                                  action=act, native=True)
    assert abs(abs(dh) - dH[0]) <= 1e-9 * max(1.0, abs(H0))


@pytest.mark.gpu
def test_native_evolve_u_matches_torch():
    dims = LATTICES[0]
    geo, u = _geo(dims), _field(dims, "cuda")
    P = hmc.random_momentum(geo, "cuda", seed=31)
    a = hmc._evolve_u(u, P, geo, 0.1, native=True)
    b = hmc._evolve_u(u, P, geo, 0.1)
    assert (a - b).abs().max().item() < 1e-11
    assert not torch.equal(a, u)
