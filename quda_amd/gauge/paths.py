"""Loop actions as path tables (the role of the reference's
computeGaugeForceQuda input_path_buf/loop_coeff interface and of MILC's
gauge-action path tables).

A loop is a tuple of signed steps +-(mu+1) as in gauge.ops.path_product;
(1, 4, -1, -4) is the (0,3) plaquette starting at x. A LoopAction is
S = beta * sum_i c_i * sum_x (1 - Re tr P_i(x) / 3) over closed loops P_i.

Its force table holds, per direction mu, (coefficient, tail) pairs: for
every loop and every step of direction mu the loop (reversed when the step
is negative) is rotated to begin with +(mu+1); the tail is what follows.
In the convention of gauge_force (H = -sum tr P^2 + S, Udot = P U)

    F_mu(x) = -(beta/6) TA[ U_mu(x) sum_p c_p T_p(x+mu) ]

with T_p(x+mu) the ordered link product along tail p starting at x+mu.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

# limits of the native kernels (csrc/gauge_path.hip): 8 packed steps per
# path -> tails of at most 7 steps, closed loops of at most 8
PATH_STEPS = 8
MAX_TAIL = 7
MAX_LOOP = 8
MAX_TAILS = 64

Loop = Tuple[int, ...]


def _check_loop(loop: Sequence[int]) -> Loop:
    loop = tuple(int(s) for s in loop)
    for s in loop:
        if s == 0 or abs(s) > 4:
            raise ValueError(f"path step {s} is not +-(mu+1), mu in 0..3")
    return loop


def displacement(path: Sequence[int]) -> Tuple[int, int, int, int]:
    """Net displacement of a path."""
    d = [0, 0, 0, 0]
    for s in path:
        d[abs(s) - 1] += 1 if s > 0 else -1
    return tuple(d)


def pack_paths(paths: Sequence[Sequence[int]]):
    """(int8 [n, PATH_STEPS] zero-padded steps, int32 [n] lengths) of a flat
    list of paths of at most PATH_STEPS steps — the kernels' device form."""
    n = len(paths)
    steps = torch.zeros((n, PATH_STEPS), dtype=torch.int8)
    lens = torch.zeros((n,), dtype=torch.int32)
    for k, p in enumerate(paths):
        p = _check_loop(p)
        if len(p) > PATH_STEPS:
            raise ValueError(f"path of {len(p)} steps exceeds {PATH_STEPS}")
        lens[k] = len(p)
        for j, s in enumerate(p):
            steps[k, j] = s
    return steps, lens


class ForceTable:
    """Per-direction (coefficient, tail) lists and their packed form:
    steps int8 [4, Np, Lt] (zero padded), lengths int32 [4, Np],
    coeffs float64 [4, Np]. Np is the largest count over the directions;
    a direction with fewer tails is padded with empty tails of
    coefficient 0, which add nothing."""

    def __init__(self, tails: Sequence[Sequence[Tuple[float, Loop]]]):
        assert len(tails) == 4
        self.tails: List[List[Tuple[float, Loop]]] = [
            [(float(c), _check_loop(t)) for c, t in tl] for tl in tails]
        self.n_paths = max(len(tl) for tl in self.tails)
        self.max_len = max([len(t) for tl in self.tails for _, t in tl],
                           default=0)
        Np = max(self.n_paths, 1)
        Lt = max(PATH_STEPS, self.max_len)
        self.steps = torch.zeros((4, Np, Lt), dtype=torch.int8)
        self.lengths = torch.zeros((4, Np), dtype=torch.int32)
        self.coeffs = torch.zeros((4, Np), dtype=torch.float64)
        for mu, tl in enumerate(self.tails):
            for k, (c, t) in enumerate(tl):
                self.lengths[mu, k] = len(t)
                self.coeffs[mu, k] = c
                for j, s in enumerate(t):
                    self.steps[mu, k, j] = s
        self._dev: Dict[str, tuple] = {}

    @property
    def native_ok(self) -> bool:
        """Within the limits of the HIP kernel."""
        return (1 <= self.n_paths <= MAX_TAILS and self.max_len <= MAX_TAIL)

    def abs_coeff_sum(self) -> float:
        """max_mu sum_p |c_p| — the scale of the rounding bound."""
        return max((sum(abs(c) for c, _ in tl) for tl in self.tails),
                   default=0.0)

    def on(self, device):
        """(steps, lengths, coeffs) on `device`, cached."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.steps.to(device).contiguous(),
                              self.lengths.to(device).contiguous(),
                              self.coeffs.to(device).contiguous())
        return self._dev[key]


class LoopAction:
    """Closed loops and their coefficients."""

    def __init__(self, loops: Sequence[Sequence[int]],
                 coeffs: Sequence[float]):
        assert len(loops) == len(coeffs)
        self.loops: Tuple[Loop, ...] = tuple(_check_loop(p) for p in loops)
        self.coeffs: Tuple[float, ...] = tuple(float(c) for c in coeffs)
        for p in self.loops:
            if any(displacement(p)):
                raise ValueError(f"loop {p} does not close")
        self._table: Optional[ForceTable] = None
        self._packed: Dict[str, tuple] = {}

    @property
    def max_loop_len(self) -> int:
        return max((len(p) for p in self.loops), default=0)

    def packed_loops(self, device):
        """(steps int8 [n, 8], lengths int32 [n]) on `device`, cached."""
        key = str(device)
        if key not in self._packed:
            s, l = pack_paths(self.loops)
            self._packed[key] = (s.to(device).contiguous(),
                                 l.to(device).contiguous())
        return self._packed[key]

    # -- constructors -----------------------------------------------------
    @classmethod
    def wilson(cls) -> "LoopAction":
        """The 6 plaquettes mu < nu, coefficient 1."""
        return cls.symanzik(0.0, _keep_zero=False)

    @classmethod
    def symanzik(cls, c1: float = -1.0 / 12.0, *,
                 _keep_zero: bool = True) -> "LoopAction":
        """The 18 loops of improved_gauge_action: 6 plaquettes mu < nu with
        c0 = 1 - 8 c1 and 12 ordered mu != nu 2x1 rectangles with c1."""
        c0 = 1.0 - 8.0 * c1
        loops, coeffs = [], []
        for mu in range(4):
            for nu in range(mu + 1, 4):
                loops.append((mu + 1, nu + 1, -(mu + 1), -(nu + 1)))
                coeffs.append(c0)
        if _keep_zero:
            for mu in range(4):
                for nu in range(4):
                    if mu == nu:
                        continue
                    loops.append((mu + 1, mu + 1, nu + 1, -(mu + 1),
                                  -(mu + 1), -(nu + 1)))
                    coeffs.append(c1)
        return cls(loops, coeffs)

    @classmethod
    def iwasaki(cls) -> "LoopAction":
        return cls.symanzik(-0.331)

    @classmethod
    def dbw2(cls) -> "LoopAction":
        return cls.symanzik(-1.4069)

    @classmethod
    def luscher_weisz(cls, c1: float, c2: float) -> "LoopAction":
        """symanzik(c1) plus the 6-link parallelograms
        (mu, nu, rho, -mu, -nu, -rho) with coefficient c2. mu, nu, rho run
        over distinct axes mu < |nu| < |rho| with nu and rho of either
        sign: the 16 parallelograms per site (4 axis triples x 4 body
        diagonals), each once. The plaquette keeps c0 = 1 - 8 c1."""
        base = cls.symanzik(c1)
        loops, coeffs = list(base.loops), list(base.coeffs)
        for mu in range(4):
            for nu in range(mu + 1, 4):
                for rho in range(nu + 1, 4):
                    for sn in (1, -1):
                        for sr in (1, -1):
                            a, b, c = mu + 1, sn * (nu + 1), sr * (rho + 1)
                            loops.append((a, b, c, -a, -b, -c))
                            coeffs.append(c2)
        return cls(loops, coeffs)


wilson = LoopAction.wilson
symanzik = LoopAction.symanzik
iwasaki = LoopAction.iwasaki
dbw2 = LoopAction.dbw2
luscher_weisz = LoopAction.luscher_weisz


def _reverse(loop: Loop) -> Loop:
    return tuple(-s for s in reversed(loop))


def loop_tails(loop: Sequence[int], mu: int) -> List[Loop]:
    """Tails of one loop for direction mu: one per step of that direction."""
    loop = tuple(loop)
    n = len(loop)
    out = []
    for k, s in enumerate(loop):
        if abs(s) != mu + 1:
            continue
        if s > 0:
            rot = loop[k:] + loop[:k]
        else:
            rev = _reverse(loop)
            j = n - 1 - k  # where the flipped step lands
            rot = rev[j:] + rev[:j]
        assert rot[0] == mu + 1
        out.append(rot[1:])
    return out


def force_table(action: LoopAction) -> ForceTable:
    """The per-direction force table of `action` (cached on it): equal
    tails merged by summing their coefficients, in order of first
    appearance; tails whose merged coefficient is exactly 0 dropped."""
    if action._table is None:
        tails = []
        for mu in range(4):
            merged: Dict[Loop, float] = {}
            for c, loop in zip(action.coeffs, action.loops):
                for t in loop_tails(loop, mu):
                    merged[t] = merged.get(t, 0.0) + c
            tails.append([(c, t) for t, c in merged.items() if c != 0.0])
        action._table = ForceTable(tails)
    return action._table


def as_table(action_or_table) -> ForceTable:
    if isinstance(action_or_table, ForceTable):
        return action_or_table
    return force_table(action_or_table)


def _path_sum_reference(u: torch.Tensor, geo, table: ForceTable, mu: int,
                        U_mu: torch.Tensor) -> torch.Tensor:
    """U_mu(x) sum_p c_p T_p(x+mu) in lex order, [V,3,3]."""
    from ..parallel.halo import shift_lex
    from .ops import path_product
    acc = torch.zeros_like(U_mu)
    for c, tail in table.tails[mu]:
        T = shift_lex(path_product(u, geo, tail), geo, mu, +1)
        acc = acc + c * T
    return U_mu @ acc


def path_product_reference(u: torch.Tensor, geo, action, scale: float = 1.0
                           ) -> torch.Tensor:
    """out_mu(x) = scale * U_mu(x) sum_p c_p T_p(x+mu) by torch ops
    ([4,2,Vcb,3,3]; multi-rank correct through shift_lex)."""
    from .ops import _from_lex, _to_lex
    table = as_table(action)
    U = _to_lex(u, geo)
    out = torch.empty_like(U)
    for mu in range(4):
        out[mu] = scale * _path_sum_reference(u, geo, table, mu, U[mu])
    return _from_lex(out, geo)


def path_force_reference(u: torch.Tensor, geo, action, beta: float
                         ) -> torch.Tensor:
    """Analytic MD force of any loop action from path_product and
    project_ta (no autograd; multi-rank correct through shift_lex). The
    oracle the HIP kernel is tested against."""
    from .ops import _from_lex, _to_lex, project_ta
    table = as_table(action)
    U = _to_lex(u, geo)
    F = torch.empty_like(U)
    for mu in range(4):
        F[mu] = -(beta / 6.0) * project_ta(
            _path_sum_reference(u, geo, table, mu, U[mu]))
    return _from_lex(F, geo)
