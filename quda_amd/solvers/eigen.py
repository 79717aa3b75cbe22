"""Eigensolvers: thick-restarted Lanczos (TRLM) for hermitian operators,
implicitly-restarted Arnoldi (IRAM) for non-hermitian, Chebyshev
acceleration, and eigenvector deflation
(ref: lib/eig_trlm.cpp, lib/eig_iram.cpp, lib/eigensolve_quda.cpp,
include/polynomial.h, lib/deflation.cpp — algorithms re-derived; the small
dense eigenproblems run on the host via numpy)."""

from __future__ import annotations

from dataclasses import dataclass, field
from math import sqrt
from typing import Callable, List, Optional, Tuple

import numpy as np

from ..fields.spinor import SpinorField
from ..ops import blas, dispatch
from ..ops.multi_blas import block_caxpy, block_cdot, block_rotate


@dataclass
class EigResult:
    evals: List[float] = field(default_factory=list)
    evecs: List[SpinorField] = field(default_factory=list)
    residuals: List[float] = field(default_factory=list)
    iters: int = 0
    converged: bool = False


def _new_like(x: SpinorField) -> SpinorField:
    return SpinorField(x.geo, x.precision, x.device, x.n_parity, nspin=x.nspin, ls=x.ls)


class ChebyshevOp:
    """p(A) with p the Chebyshev polynomial of degree n mapping
    [a_min, a_max] -> [-1, 1]: damps that window, amplifies the spectrum
    below a_min (ref: include/polynomial.h + eig_param poly_acc)."""

    def __init__(self, op, a_min: float, a_max: float, degree: int):
        self.op = op
        self.a_min, self.a_max = a_min, a_max
        self.degree = degree

    def apply(self, out: SpinorField, inp: SpinorField, tmp: SpinorField):
        a, b = self.a_min, self.a_max
        theta = 2.0 / (b - a)
        delta = -(b + a) / (b - a)
        # T_0 = in ; T_1 = (theta A + delta) in
        tkm1 = _new_like(inp)
        blas.copy(tkm1, inp)
        tk = _new_like(inp)
        self.op.MdagM(tk, inp, tmp)
        blas.axpby(delta, tkm1, theta, tk)
        for _ in range(1, self.degree):
            # T_{k+1} = 2 (theta A + delta) T_k - T_{k-1}
            t_next = _new_like(inp)
            self.op.MdagM(t_next, tk, tmp)
            blas.scal(2.0 * theta, t_next)
            blas.axpy(2.0 * delta, tk, t_next)
            blas.axpy(-1.0, tkm1, t_next)
            tkm1, tk = tk, t_next
        blas.copy(out, tk)
        return out


def trlm_solve(op, n_ev: int, n_kr: int, x0: SpinorField, *,
               tol: float = 1e-8, max_restarts: int = 100,
               poly: Optional[ChebyshevOp] = None,
               which: str = "smallest") -> EigResult:
    """Thick-restarted Lanczos on the hermitian MdagM of `op`
    (ref: lib/eig_trlm.cpp): find the n_ev smallest (or largest)
    eigenpairs using an n_kr-dimensional Krylov space. `x0` provides the
    geometry/precision and the initial vector (randomized if zero).
    With `poly`, iterate p(A) but report eigenvalues of A (Rayleigh
    quotients at the end)."""
    res = EigResult()
    assert n_kr > n_ev
    apply_op = (poly.apply if poly is not None
                else (lambda o, i, t: op.MdagM(o, i, t)))

    V = [_new_like(x0) for _ in range(n_kr + 1)]
    tmp = _new_like(x0)
    r = _new_like(x0)
    # the HIP multi-BLAS kernels, when QUDA_AMD_NATIVE_MULTI_BLAS opts in
    block_ops = dispatch.multi_blas_eligible(V + [r], writes=True)
    if blas.norm2(x0) == 0.0:
        x0.gaussian_(seed=1234)
    blas.copy(V[0], x0)
    blas.scal(1.0 / sqrt(blas.norm2(V[0])), V[0])

    alpha = np.zeros(n_kr)
    beta = np.zeros(n_kr)
    n_conv = 0
    num_keep = 0
    iters = 0

    def lanczos_step(j):
        """r = Op V[j] - alpha_j V[j] - (thick-restart / beta couplings)."""
        nonlocal iters
        apply_op(r, V[j], tmp)
        iters += 1
        if j > 0 and j > num_keep:
            blas.axpy(-beta[j - 1], V[j - 1], r)
        a = blas.re_dot(V[j], r)
        alpha[j] = a
        blas.axpy(-a, V[j], r)
        if j == num_keep and num_keep > 0:
            # coupling to all kept vectors after a thick restart
            for i in range(num_keep):
                blas.axpy(-beta[i], V[i], r)
        # full re-orthogonalization (ref blockOrthogonalize)
        if block_ops:
            # block classical Gram-Schmidt, twice: each pass reads the basis
            # once for the dots and once for the update
            for _ in range(2):
                c = block_cdot(V[:j + 1], [r])
                block_caxpy(-c.mT, V[:j + 1], [r])
        else:
            for i in range(j + 1):
                c = blas.c_dot(V[i], r)
                blas.caxpy(-c, V[i], r)
        b = sqrt(blas.norm2(r))
        beta[j] = b
        if b > 0:
            blas.copy(V[j + 1], r)
            blas.scal(1.0 / b, V[j + 1])
        return b

    for restart in range(max_restarts):
        for j in range(num_keep, n_kr):
            lanczos_step(j)
        # build the projected matrix T (tridiagonal + arrowhead from restart)
        T = np.zeros((n_kr, n_kr))
        for j in range(n_kr):
            T[j, j] = alpha[j]
        for j in range(num_keep):
            T[j, n_kr - (n_kr - num_keep)] = 0  # placeholder
        # arrowhead: kept block is diagonal alpha[0..keep) with coupling
        # beta[i] between V[i] and V[keep]; Lanczos part tridiagonal
        for i in range(num_keep):
            T[i, num_keep] = beta[i]
            T[num_keep, i] = beta[i]
        for j in range(num_keep, n_kr - 1):
            T[j, j + 1] = beta[j]
            T[j + 1, j] = beta[j]
        w, Z = np.linalg.eigh(T)
        order = np.argsort(w if which == "smallest" else -w)
        w, Z = w[order], Z[:, order]
        # residual estimates |beta_last * Z[last, i]|
        blast = beta[n_kr - 1]
        rnorms = np.abs(blast * Z[n_kr - 1, :])
        n_conv = int(np.sum(rnorms[:n_ev] < tol * np.maximum(1e-30, np.abs(w[:n_ev]))))
        if n_conv >= n_ev or restart == max_restarts - 1:
            keep = n_ev
            Vnew = _rotate(V, Z[:, :keep], n_kr)
            evals, resids, evecs = [], [], []
            for i in range(keep):
                apply_op(r, Vnew[i], tmp)
                lam = blas.re_dot(Vnew[i], r)
                blas.axpy(-lam, Vnew[i], r)
                evals.append(lam)
                resids.append(sqrt(blas.norm2(r)))
                evecs.append(Vnew[i])
            if poly is not None:
                # recompute Rayleigh quotients on the TRUE operator
                evals = []
                for i in range(keep):
                    op.MdagM(r, evecs[i], tmp)
                    evals.append(blas.re_dot(evecs[i], r))
            res.evals = evals
            res.evecs = evecs
            res.residuals = resids
            res.iters = iters
            res.converged = n_conv >= n_ev
            return res
        # thick restart: keep n_ev + extra Ritz vectors
        num_keep = min(n_ev + (n_kr - n_ev) // 2, n_kr - 1)
        Vkeep = _rotate(V, Z[:, :num_keep], n_kr)
        for i in range(num_keep):
            blas.copy(V[i], Vkeep[i])
        blas.copy(V[num_keep], V[n_kr])  # residual vector continues
        for i in range(num_keep):
            alpha[i] = w[i]
            beta[i] = blast * Z[n_kr - 1, i]
    return res


def _rotate(V, Z, m):
    """Vnew_i = sum_j V[j] Z[j,i] (host-coefficient basis rotation)."""
    k = Z.shape[1]
    if dispatch.multi_blas_eligible(V[:m], writes=True):
        return block_rotate(V[:m], Z[:m])
    out = []
    for i in range(k):
        v = _new_like(V[0])
        v.zero_()
        for j in range(m):
            z = complex(Z[j, i])
            if z != 0:
                blas.caxpy(z, V[j], v)
        out.append(v)
    return out


def iram_solve(op, n_ev: int, n_kr: int, x0: SpinorField, *,
               tol: float = 1e-8, max_restarts: int = 100,
               which: str = "smallest_abs", dagger: bool = False) -> EigResult:
    """Restarted Arnoldi for the (non-hermitian) M of `op` with
    Krylov-Schur restarts (ref: lib/eig_iram.cpp, same role; the restart
    uses an ordered Schur form of the projected matrix, which is the
    numerically robust formulation of implicit restarting). Dense work via
    scipy/numpy on the n_kr x n_kr projected matrix."""
    import scipy.linalg as sla

    res = EigResult()
    V = [_new_like(x0) for _ in range(n_kr + 1)]
    tmp = _new_like(x0)
    r = _new_like(x0)
    B = np.zeros((n_kr + 1, n_kr), dtype=complex)  # projected matrix + resid row
    if blas.norm2(x0) == 0.0:
        x0.gaussian_(seed=4321)
    blas.copy(V[0], x0)
    blas.scal(1.0 / sqrt(blas.norm2(V[0])), V[0])
    iters = 0

    if which == "smallest_abs":
        sel = lambda w: np.argsort(np.abs(w))
    elif which == "largest_abs":
        sel = lambda w: np.argsort(-np.abs(w))
    else:
        sel = lambda w: np.argsort(w.real)

    def arnoldi_step(j):
        nonlocal iters
        op.M(r, V[j], dagger=dagger)
        iters += 1
        for i in range(j + 1):
            B[i, j] = blas.c_dot(V[i], r)
            blas.caxpy(-complex(B[i, j]), V[i], r)
        for i in range(j + 1):  # one reorthogonalization pass
            c = blas.c_dot(V[i], r)
            B[i, j] += c
            blas.caxpy(-complex(c), V[i], r)
        b = sqrt(blas.norm2(r))
        B[j + 1, j] = b
        if b > 0:
            blas.copy(V[j + 1], r)
            blas.scal(1.0 / b, V[j + 1])
        return b

    k = 0  # restart block size currently in B[:k,:k]
    for restart in range(max_restarts):
        for j in range(k, n_kr):
            arnoldi_step(j)
        Bs = B[:n_kr, :n_kr]
        beta_f = B[n_kr, n_kr - 1].real
        w, Z = np.linalg.eig(Bs)
        order = sel(w)
        w, Z = w[order], Z[:, order]
        rnorm_est = np.abs(beta_f * Z[n_kr - 1, :])
        done = np.all(rnorm_est[:n_ev]
                      < tol * np.maximum(np.abs(w[:n_ev]), 1e-30))
        if done or restart == max_restarts - 1:
            evecs = _rotate(V, Z[:, :n_ev], n_kr)
            evals, resids = [], []
            for i in range(n_ev):
                nv = sqrt(blas.norm2(evecs[i]))
                blas.scal(1.0 / nv, evecs[i])
                op.M(r, evecs[i], dagger=dagger)
                lam = blas.c_dot(evecs[i], r)
                blas.caxpy(-lam, evecs[i], r)
                evals.append(lam)
                resids.append(sqrt(blas.norm2(r)))
            res.evals = evals
            res.evecs = evecs
            res.residuals = resids
            res.iters = iters
            res.converged = bool(done)
            return res
        # Krylov-Schur restart: ordered Schur form, keep k wanted vectors
        k = n_ev + (n_kr - n_ev) // 2
        wanted = set(order[:k])
        # scipy gees sort callable gets each eigenvalue; emulate ordering by
        # computing the Schur form then reordering with sort on |.|
        thresh = sorted(np.abs(w))[k - 1] if which == "smallest_abs" else None
        if which == "smallest_abs":
            T, Q, sdim = sla.schur(Bs, output="complex",
                                   sort=lambda x: abs(x) <= thresh + 1e-14)
        elif which == "largest_abs":
            thresh = sorted(np.abs(w))[-k]
            T, Q, sdim = sla.schur(Bs, output="complex",
                                   sort=lambda x: abs(x) >= thresh - 1e-14)
        else:
            thresh = sorted(w.real)[k - 1]
            T, Q, sdim = sla.schur(Bs, output="complex",
                                   sort=lambda x: x.real <= thresh + 1e-14)
        k = int(sdim) if 0 < int(sdim) < n_kr else k
        Vnew = _rotate(V, Q[:, :k], n_kr)
        for i in range(k):
            blas.copy(V[i], Vnew[i])
        blas.copy(V[k], V[n_kr])  # old residual direction becomes V[k]
        B[:, :] = 0
        B[:k, :k] = T[:k, :k]
        B[k, :k] = beta_f * Q[n_kr - 1, :k]
    return res


class Deflation:
    """Galerkin eigenvector deflation (ref: lib/deflation.cpp + solver.cpp
    deflation hookup): given approximate eigenpairs of the hermitian A,
    produce the deflated initial guess x0 = sum_i v_i <v_i, b>/lambda_i."""

    def __init__(self, evals: List[float], evecs: List[SpinorField]):
        self.evals = evals
        self.evecs = evecs

    def guess(self, x: SpinorField, b: SpinorField) -> SpinorField:
        x.zero_()
        for lam, v in zip(self.evals, self.evecs):
            if abs(lam) < 1e-30:
                continue
            c = blas.c_dot(v, b) / lam
            blas.caxpy(c, v, x)
        return x


def block_trlm_solve(op, n_ev: int, n_kr: int, x0: SpinorField, *,
                     block_size: int = 4, tol: float = 1e-8,
                     max_restarts: int = 100,
                     poly: Optional[ChebyshevOp] = None,
                     which: str = "smallest") -> EigResult:
    """Block thick-restarted Lanczos (ref: lib/eig_block_trlm.cpp —
    re-designed: the basis grows in `block_size` panels so the operator
    and BLAS phases batch over the panel (GEMM-shaped on GPU); the
    projected matrix is rebuilt from the explicit orthogonalization
    coefficients, and the thick restart keeps the Ritz vectors plus the
    pending (unprocessed) panel, whose couplings are recomputed when the
    panel is processed — no closed-form boundary algebra to get wrong.
    Per-matvec convergence trails scalar TRLM (smaller Krylov depth per
    restart); the payoff is the batched panel apply on GPU."""
    res = EigResult()
    bs = block_size
    assert n_kr > n_ev + bs
    apply_op = (poly.apply if poly is not None
                else (lambda o, i, t: op.MdagM(o, i, t)))
    tmp = _new_like(x0)
    w = _new_like(x0)

    def ortho_append(vec, V, H, col):
        """Orthogonalize `vec` against V, recording coefficients in
        H[:, col]; append the normalized remainder (returns False on
        breakdown)."""
        for i, u in enumerate(V):
            c = blas.c_dot(u, vec)
            H[i, col] += c
            blas.caxpy(-c, u, vec)
        # second Gram-Schmidt pass for orthogonality at restart scale
        for i, u in enumerate(V):
            c = blas.c_dot(u, vec)
            H[i, col] += c
            blas.caxpy(-c, u, vec)
        nb = sqrt(blas.norm2(vec))
        if nb < 1e-14:
            return False
        H[len(V), col] += nb
        blas.scal(1.0 / nb, vec)
        V.append(vec)
        return True

    # initial panel
    gen_seed = 4321
    V: List[SpinorField] = []
    H = np.zeros((n_kr + bs, n_kr + bs), dtype=complex)
    if blas.norm2(x0) == 0.0:
        x0.gaussian_(seed=gen_seed)
    first = _new_like(x0)
    blas.copy(first, x0)
    blas.scal(1.0 / sqrt(blas.norm2(first)), first)
    V.append(first)
    while len(V) < bs:
        v = _new_like(x0)
        v.gaussian_(seed=gen_seed + len(V))
        scratch = np.zeros((n_kr + bs, 1), dtype=complex)
        if not ortho_append(v, V, scratch, 0):
            v.gaussian_(seed=gen_seed + 1000 + len(V))
            ortho_append(v, V, scratch, 0)

    jp = 0          # processed columns
    iters = 0
    n_conv = 0
    for restart in range(max_restarts):
        # process panels until the basis would exceed n_kr
        while jp + bs <= len(V) and len(V) + bs <= n_kr:
            for c in range(jp, jp + bs):
                apply_op(w, V[c], tmp)
                iters += 1
                vec = _new_like(x0)
                blas.copy(vec, w)
                if not ortho_append(vec, V, H, c):
                    vv = _new_like(x0)
                    vv.gaussian_(seed=gen_seed + 2000 + iters)
                    scratch = np.zeros((n_kr + bs, 1), dtype=complex)
                    ortho_append(vv, V, scratch, 0)
            jp += bs
        # Rayleigh-Ritz over the processed prefix. H[i, c] is filled when
        # column c is processed; the mirror H[c, i] stayed zero whenever
        # row c did not exist yet -- restore it from hermiticity instead
        # of averaging (averaging would halve one-sided couplings).
        Hp = H[:jp, :jp].copy()
        mask = Hp == 0
        Hp[mask] = Hp.conj().T[mask]
        Hp = 0.5 * (Hp + Hp.conj().T)
        wv, Z = np.linalg.eigh(Hp)
        order = np.argsort(wv if which == "smallest" else -wv)
        wv, Z = wv[order], Z[:, order]
        # residual estimates from the pending-panel coupling rows
        C = H[jp:len(V), :jp]
        rnorm = np.linalg.norm(C @ Z, axis=0)
        n_conv = 0
        for i in range(n_ev):
            if rnorm[i] < tol * max(abs(wv[i]), 1e-30):
                n_conv += 1
            else:
                break
        keep = min(max(n_ev + bs, 2 * n_ev), jp - 1)
        if n_conv >= n_ev or restart == max_restarts - 1:
            keep = n_ev
        # rotate: new basis = Ritz vectors (keep) + pending panel
        newV = []
        for jcol in range(keep):
            vj = _new_like(x0)
            vj.zero_()
            for i in range(jp):
                blas.caxpy(complex(Z[i, jcol]), V[i], vj)
            newV.append(vj)
        pend = V[jp:len(V)]
        # re-orthogonalize pending panel against the rotated Ritz basis
        # (exact in theory; re-done for float hygiene)
        Hn = np.zeros((n_kr + bs, n_kr + bs), dtype=complex)
        Hn[:keep, :keep] = np.diag(wv[:keep])
        V2 = list(newV)
        scratch = np.zeros((n_kr + bs, 1), dtype=complex)
        for pv in pend:
            ortho_append(pv, V2, scratch, 0)
        V = V2
        H = Hn
        jp = keep
        if n_conv >= n_ev:
            break
    # final: exact eigenpairs + residuals
    evecs = V[:n_ev]
    evals, resids = [], []
    r = _new_like(x0)
    for i in range(n_ev):
        op.MdagM(r, evecs[i], tmp)
        lam = blas.re_dot(evecs[i], r)
        blas.axpy(-lam, evecs[i], r)
        evals.append(lam)
        resids.append(sqrt(blas.norm2(r)))
    res.evals = evals
    res.evecs = evecs
    res.residuals = resids
    res.iters = iters
    res.converged = n_conv >= n_ev
    return res
