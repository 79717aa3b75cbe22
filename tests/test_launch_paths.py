"""Launch paths between the dispatch layer and the kernels that no other
GPU test reaches: the merged-halo batch with multi-RHS kernel groups, the
domain-wall slices through the slab halo, and the halo cache key.

The GPU cases go through the dispatch API only. Tolerances are those of
tests/test_gpu_kernels.py::test_dslash_mrhs_vs_per_rhs, relative to the
maximum of the reference."""
import pytest
import torch

from quda_amd import GaugeField, LatticeGeometry, SpinorField
from quda_amd.fields.clover import CloverField, pack_clover
from quda_amd.ops import dispatch
from quda_amd.ops import reference as ref
from quda_amd.ops.dispatch import (CLOV_POST, PLAIN, dslash_wilson,
                                   dslash_wilson_batch, dslash_wilson_slices,
                                   dwf_halo_exchange)
from quda_amd.parallel import comms

RTOL = {"half": 2e-3, "single": 1e-5, "double": 1e-13}
A_COEF = -0.3
MASK = 0b1111

_cache = {}


def _host(dims, seed):
    """Seeded double gauge (complex, CPU), shared and never modified."""
    key = ("host", dims)
    if key not in _cache:
        geo = LatticeGeometry(dims)
        g = GaugeField(geo, "double").random_su3_(seed=seed)
        _cache[key] = (geo, g.to_complex())
    return _cache[key]


def _gauge(geo, u, prec):
    recon = "none" if prec == "double" else "twelve"
    return GaugeField(geo, prec, "cuda", reconstruct=recon).from_complex(
        u.cuda())


def _rel_err(got, want):
    w = want.to_complex()
    return (got.to_complex() - w).abs().max().item() / w.abs().max().item()


# ---------------------------------------------------------------------------
# merged-halo batch with kernel groups
# ---------------------------------------------------------------------------
BATCH_DIMS = (4, 6, 4, 8)
NRHS = 5
BATCH_CASES = [(mode, dag) for mode in (PLAIN, CLOV_POST)
               for dag in (False, True)]


def _batch_setup(prec):
    """Inputs, clover and the unpartitioned per-RHS reference of every
    (mode, dagger) case, computed once per precision."""
    key = ("batch", prec)
    if key in _cache:
        return _cache[key]
    geo, u = _host(BATCH_DIMS, 71)
    g = _gauge(geo, u, prec)
    A = ref.clover_matrix(u, geo, 0.13, 1.1)
    cl = CloverField(geo, prec, "cuda")
    cl.data.copy_(cl._to_native(pack_clover(A.cuda())))
    cl.inv_data.copy_(cl.data)  # any hermitian packed field works here
    inps = [SpinorField(geo, prec, "cuda", n_parity=1).gaussian_(seed=720 + r)
            for r in range(NRHS)]
    xs = [SpinorField(geo, prec, "cuda", n_parity=1).gaussian_(seed=740 + r)
          for r in range(NRHS)]
    want = {}
    for mode, dag in BATCH_CASES:
        outs = [SpinorField(geo, prec, "cuda", n_parity=1)
                for _ in range(NRHS)]
        for r in range(NRHS):
            dslash_wilson(outs[r], inps[r], g, 0, dagger=dag, a=A_COEF,
                          x=xs[r], mode=mode,
                          clover=cl if mode == CLOV_POST else None)
        want[(mode, dag)] = outs
    _cache[key] = (geo, u, cl, inps, xs, want)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "half"])
@pytest.mark.parametrize("group", [4, 2])
def test_batch_merged_halo_kernel_groups(prec, group):
    """dslash_wilson_batch under a forced partition with the multi-RHS
    kernel on: 5 sides as one group of 4 (or two of 2) plus a per-RHS
    remainder, every side reading its slice of the merged ghost slab.
    CLOV_POST makes the boundary sites of the interior kernels defer to the
    per-RHS exterior kernel."""
    geo, u, cl, inps, xs, want = _batch_setup(prec)
    saved = dispatch._MRHS_GROUP
    try:
        dispatch._MRHS_GROUP = group
        groups, rem0 = dispatch._mrhs_groups(NRHS)
        assert groups == ([(0, 4)] if group == 4 else [(0, 2), (2, 2)])
        assert rem0 == 4
        comms.set_forced_partition(MASK)
        g2 = _gauge(geo, u, prec)  # rebuilt: its ghost links are exchanged
        for mode, dag in BATCH_CASES:
            outs = [SpinorField(geo, prec, "cuda", n_parity=1)
                    for _ in range(NRHS)]
            dslash_wilson_batch(outs, inps, g2, 0, dagger=dag, a=A_COEF,
                                xs=xs, mode=mode,
                                clover=cl if mode == CLOV_POST else None)
            for r in range(NRHS):
                err = _rel_err(outs[r], want[(mode, dag)][r])
                print(f"batch {prec} g{group} m{mode} dag{int(dag)} r{r} "
                      f"err={err:.3e}")
                assert err < RTOL[prec], (prec, group, mode, dag, r, err)
    finally:
        comms.set_forced_partition(0)
        dispatch._MRHS_GROUP = saved


# ---------------------------------------------------------------------------
# domain-wall slices through the slab halo
# ---------------------------------------------------------------------------
SLICE_DIMS = (4, 4, 4, 8)
LS = 5
SLICE_CASES = [(dag, use_x) for dag in (False, True)
               for use_x in (False, True)]


def _slice_setup(prec):
    """5-d inputs and the unpartitioned, group-size-1 reference of every
    (dagger, x) case, computed once per precision."""
    key = ("slices", prec)
    if key in _cache:
        return _cache[key]
    geo, u = _host(SLICE_DIMS, 81)
    g = _gauge(geo, u, prec)
    inp = SpinorField(geo, prec, "cuda", n_parity=1, ls=LS).gaussian_(seed=811)
    x = SpinorField(geo, prec, "cuda", n_parity=1, ls=LS).gaussian_(seed=812)
    saved = dispatch._MRHS_GROUP
    want = {}
    try:
        dispatch._MRHS_GROUP = 1
        for dag, use_x in SLICE_CASES:
            out = SpinorField(geo, prec, "cuda", n_parity=1, ls=LS)
            dslash_wilson_slices(out, inp, g, 0, dagger=dag, a=A_COEF,
                                 x=x if use_x else None)
            want[(dag, use_x)] = out
    finally:
        dispatch._MRHS_GROUP = saved
    _cache[key] = (geo, u, inp, x, want)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["double", "half"])
def test_dwf_slices_slab_halo(prec):
    """dwf_halo_exchange + dslash_wilson_slices under a forced partition
    with group size 4 at Ls = 5: slices 0-3 in one multi-RHS launch that
    offsets into the ghost slab, slice 4 through dslash_wilson_slice."""
    geo, u, inp, x, want = _slice_setup(prec)
    saved = dispatch._MRHS_GROUP
    try:
        dispatch._MRHS_GROUP = 4
        assert dispatch._mrhs_groups(LS) == ([(0, 4)], 4)
        comms.set_forced_partition(MASK)
        g2 = _gauge(geo, u, prec)
        for dag, use_x in SLICE_CASES:
            out = SpinorField(geo, prec, "cuda", n_parity=1, ls=LS)
            h = dwf_halo_exchange(inp, 1, dag)
            dslash_wilson_slices(out, inp, g2, 0, dagger=dag, a=A_COEF,
                                 x=x if use_x else None, halo=h)
            err = _rel_err(out, want[(dag, use_x)])
            print(f"slices {prec} dag{int(dag)} x{int(use_x)} err={err:.3e}")
            assert err < RTOL[prec], (prec, dag, use_x, err)
    finally:
        comms.set_forced_partition(0)
        dispatch._MRHS_GROUP = saved


# ---------------------------------------------------------------------------
# halo cache key (buffers only: needs neither a GPU nor the extension)
# ---------------------------------------------------------------------------
def test_halo_cache_key():
    """The pack reads geo.parity_offset, so two geometries that differ only
    there must not share a halo, whatever the slab kind (none, Ls slices,
    n right-hand sides; Wilson or staggered depth 3); an equal signature
    returns the same object."""
    from quda_amd.parallel.halo import get_spinor_halo
    dims = (4, 4, 4, 8)
    g0 = LatticeGeometry(dims, parity_offset=0)
    g1 = LatticeGeometry(dims, parity_offset=1)
    seen = set()
    for kw in (dict(), dict(n_slab=LS), dict(n_slab=3),
               dict(ncomp=6, depth=3)):
        h0 = get_spinor_halo(g0, "half", "cpu", MASK, **kw)
        h1 = get_spinor_halo(g1, "half", "cpu", MASK, **kw)
        assert h0 is not h1, kw
        assert (h0.geo.parity_offset, h1.geo.parity_offset) == (0, 1), kw
        again = get_spinor_halo(LatticeGeometry(dims, parity_offset=1),
                                "half", "cpu", MASK, **kw)
        assert again is h1, kw
        seen |= {id(h0), id(h1)}
        n_slab, depth = kw.get("n_slab"), kw.get("depth", 1)
        lead = () if n_slab is None else (n_slab,)
        fcb = g0.face_volume_cb(3) * depth
        assert h0.recv[(3, 0)].is_contiguous()
        assert tuple(h0.recv[(3, 0)].shape)[:-3] == lead, kw
        assert tuple(h0.recv_nrm[(3, 0)].shape) == lead + (fcb,), kw
    assert len(seen) == 8  # no two signatures share an object
