"""Per-component operators (somar_comp_set_op) on the launch paths tests/test_gpu_multi_ops.py does not reach.  The
specification and the standard are that file's: a multi call leaves component c -- fields, statistics, residual history, bit
for bit -- as the single-field call does on a SEPARATE one-component handle created with c's BC types, values and coefficients
on the same geometry and metric; every comparison is assert_array_equal (through _same), and where a group says "also the
oracle" one component is held to the oracle's one_cycle for its operator too, so that both GPU paths wrong alike cannot pass.

Groups (layouts: those of tests/test_gpu_multi.py and tests/test_gpu_multi_ops.py, not grown):
  1. no Dirichlet side anywhere, operators that differ in (alpha, beta) only: the DIRI = false forms of the sweep on one operator
     per field, k_gsrb_fused_nf<0,false,2,FieldOps<2>>, <1,false,2,FieldOps<2>>, <1,false,3,FieldOps<3>>.  With two and three components every N-field launch carries different operators
     (opLaunches == batched launches), and no field of any launch has a Dirichlet side: they are those forms by construction.
  2. components that differ in alpha, a Poisson component with Dirichlet sides next to Helmholtz ones, and a heat step whose
     components were created with different aCoef (set_alpha_beta scales each by its own pair).
  3. two components with one own operator that is not the handle's: the `differ == false` branch of sweep_launch / resid_launch
     with an operator that is not the level's (the one-operator kernel handed O.P[0]) -- (a) next to a pair that differs, (b) an own operator
     equal to the handle's in every entry, (c) the pair left over once component 0 has left a solve.
  4. periodic directions: comp_set_op keeps the handle's entries there whatever is passed (7 / 99.0 here), comp_params masks the
     sides by L.periodic, make_diri_ops skips them.
  5. active sets of solveMulti that do not contain component 0 or are not contiguous ({1,2,3}, {1,3}, {0,2,3}, {0,2}), a
     component without a cycle among own operators, and bottom solvers of different kinds inside one solve.
  6. setAlphaAndBeta outside a heat step: every kept-aside operator scaled, an operator set after it scaled through ab_scale_,
     the captured graphs of the kept-aside operators dropped (with graph legs the third call replays what the second captured).
  7. a metric refresh that CHANGES the metric: the face copiers ensure_face_copiers added, the re-probe, the rebuilt depths.
  8. position-dependent Dirichlet values on the handle (setBCFaceValues) together with own operators.

Every case first proves its target: _reaches_layout (K, MG ratios, box widths), the launch counters (_reaches_ops or the
group's own assertion on opLaunches), and for the solves the iteration counts of the SEPARATE handles, which decide the
active sets.

The separate-handle references are computed once per (layout and operators -- the case's name --, sweeps) and left unchanged
(_cycle_refs / _given_refs of tests/test_gpu_multi_ops.py, and _SOLVE_REFS, _SCALED_REFS, _REFRESH_REFS here).

What the layouts themselves decide, found while building this file:
  * wide has no graph-replayed leg under the suite's SOMAR_GRAPH_CELLS = 4096: its first depth that small, 16 x 12 x 12, is
    the bottom level, and the legs start above the bottom (ragged and extra-wide likewise).  Group 6 (a) therefore runs a
    second time with SOMAR_GRAPH_CELLS = 32 x 24 x 24, which makes depth 2 the seam (K = 2 proves it): only there can a stale
    graph of an operator kept aside be replayed.
  * wide's bottom level is one box of 2304 cells, more than the one-launch bottom solvers take (2048): every operator runs
    the host-loop BiCGStab there.  Bottom kinds differ on ragged with OPS_HIGH (asserted on the separate handles).
  * a solve that ends without a cycle on a residual that is not zero has status 2 ("blew up") on either path, and the
    binding raises: the component without a cycle has a right-hand side identically zero, and that solve runs with
    forceHomogeneous = True (under its inhomogeneous walls the residual of a zero right-hand side is not zero).
  * the smooth right-hand side of 1.5 NORM_THRESH takes two cycles under these operators, not one; the active sets are
    asserted through the order of the separate handles' counts, which holds.

Beyond the eight groups: heatStepMulti in the sequential fallback (K = 0) with create-time pairs that differ in alpha, where
set_alpha_beta runs while a component's operator is in place.

Mutations, each applied to a scratch copy of the library and run once on the MI355X against this file and
tests/test_gpu_multi_ops.py (failed tests here / there), when the per-operator kernels were a text of their own (k_*_nfo) and
sweep_launch substituted the operator through a copy of the level (`Ld.P = O.P[0]`):
  * field 1 of k_gsrb_fused_nfo<*, false, *> reads O.P[0].beta: 24 / 0 -- every test of group 1.
  * comp_params without the !L.periodic[a] mask: 15 / 0 -- group 4 and the periodic ragged cases of group 1.
  * sweep_launch without `Ld.P = O.P[0]` (now: handing the launcher L.dev.P instead of O.P[0]): 4 / 0 -- group 3 (a) and (c),
    both layouts.
  * drop_graphs skips the components' graphs: 1 / 0 -- group 6 (a) with graph legs.  (Without the second value of
    SOMAR_GRAPH_CELLS nothing failed: no graph existed.)
  * comp_set_op ignores ab_scale_: 1 / 0 -- group 6 (b).
  * multi_residual0 called with `every` in the loop of solve_multi: 14 / 8 -- every solve and heat step of groups 2 to 5
    and 8; the older file notices it too, as soon as a component other than the last has left (its sets are {0, 2}, {2}).
None is equivalent."""
import numpy as np
import pytest

from tests.helpers import download_valid, upload
from tests.test_gpu_mixed_kernels import RAGGED_BOXES, RAGGED_N, WIDE_BOX, WIDE_N, WIDE_RATIOS, gpu_solver, oracle_cycle, problem, set_env
from tests.test_gpu_multi import (EPS, GHOST_MARK, IMAX, NORM_THRESH, RAGGED_WIDTHS, STAT_KEYS, WIDE_WIDTHS, XWIDE_BOX, XWIDE_N,
                                  XWIDE_RATIOS, XWIDE_WIDTHS, _down, _reaches_layout, _same, _smooth_field, _solver, _up)
from tests.test_gpu_multi_ops import (BETA_SCALAR, OPS, OPS_HIGH, WALL, D, N, Op, _cycle_refs, _given_refs, _layout,
                                      _multi_solver, _own, _reaches_ops, _set_ops, _with_small_walls)

pytestmark = pytest.mark.gpu

RAGGED_L = (1.25, 1.0, 0.5)


@pytest.fixture(autouse=True)
def _large_level_kernels(monkeypatch):
    set_env(monkeypatch.setenv)
    for k in ("SOMAR_NARROW_7PT", "SOMAR_NO_NARROW_TILES", "SOMAR_FUSED_ROWS", "SOMAR_ORDERED_REDUCE_MAX"):
        monkeypatch.delenv(k, raising=False)


def _lay(kind, tag, ops, periodic=(False,) * 3):
    """one of the layouts under a set of operators; the handle is created with ops[0]'s pair.  The name carries both, and
    keys the cached references."""
    name = "%s/%s" % (kind, tag)
    if kind == "wide":
        c = _layout(name, WIDE_N, WIDE_BOX, (1.0, 1.0, 1.0), 3, WIDE_WIDTHS, WIDE_RATIOS, ops=ops)
    elif kind == "ragged":
        c = _layout(name, RAGGED_N, RAGGED_BOXES, RAGGED_L, 2, RAGGED_WIDTHS, [(2, 2, 2)] * 2, ops=ops, periodic=periodic)
    elif kind == "extra-wide":
        c = _layout(name, XWIDE_N, XWIDE_BOX, (1.0, 1.0, 1.0), 4, XWIDE_WIDTHS, XWIDE_RATIOS, ops=ops, tables="tall")
    else:
        assert kind == "anisotropic"
        c = _layout(name, (64, 32, 16), 32, (4.0, 1.0, 0.5), 2, [[32, 32]] * 2, [(1, 2, 2), (2, 2, 2)], ops=ops, periodic=periodic)
    c.alpha, c.beta = ops[0].alpha, ops[0].beta
    return c


def _counts(s, ncomp, K):
    n, k, m = s.getComponents()
    assert (n, k) == (ncomp, K), (n, k, ncomp, K)
    assert m > 0, "no N-field launch was issued"
    assert 0 <= s.opLaunches() <= m
    return m, s.opLaunches()


_ORACLE = {}


def _from_zero(so, case, ncomp, sweeps, passed=None, oracle_comp=None):
    """vcycleMulti(True) against the separate handles; -> (batched launches, of those with different operators)"""
    from somar_amd import api as F
    prob, res, seq = _cycle_refs(so, case, sweeps)
    grids = prob[1]
    s = gpu_solver(case, prob, sweeps=sweeps)
    try:
        s.setComponents(ncomp)
        _set_ops(s, case, ncomp, passed)
        oratios = [tuple(r) for r in s.mgRefRatios()]
        _reaches_layout(s, case, case.K, oratios)
        for c in range(ncomp):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        m, o = _counts(s, ncomp, case.K)
        got = [_down(s, c, F.F_CORR, grids) for c in range(ncomp)]
    finally:
        s.undefine()
    for c in range(ncomp):
        assert all(float(np.max(np.abs(g))) > 0.0 for g in got[c])
        _same(got[c], seq[c], "%s %d/%d/%d component %d of %d vs a separate handle" % (case.name, sweeps, sweeps, sweeps, c, ncomp))
    if oracle_comp is not None and oracle_comp < ncomp:
        key = (case.name, oracle_comp, sweeps)
        if key not in _ORACLE:
            _ORACLE[key] = oracle_cycle(so, _own(case, oracle_comp), prob, res[oracle_comp], sweeps)
        ora, ora_ratios = _ORACLE[key]
        assert ora_ratios == oratios
        _same(got[oracle_comp], ora, "%s component %d of %d vs the oracle's one_cycle for its operator" % (case.name, oracle_comp, ncomp))
    return m, o


def _given(so, case, ncomp, ghost=(0, 0, 0), passed=None):
    """vcycleMulti(False) on a correction whose ghost cells hold GHOST_MARK + c; -> (the fields with `ghost`, launches, op launches)"""
    from somar_amd import api as F
    prob, res, cor, seq = _given_refs(so, case, ghost)
    s = gpu_solver(case, prob)
    try:
        s.setComponents(ncomp)
        _set_ops(s, case, ncomp, passed)
        _reaches_layout(s, case, case.K, [tuple(r) for r in s.mgRefRatios()])
        for c in range(ncomp):
            _up(s, c, F.F_RES, res[c])
            _up(s, c, F.F_CORR, cor[c])
        s.vcycleMulti(False)
        m, o = _counts(s, ncomp, case.K)
        got = [[s.downloadComp(c, F.F_CORR, q, ghost) for q in range(s.num_local_patches)] for c in range(ncomp)]
    finally:
        s.undefine()
    for c in range(ncomp):
        _same(got[c], seq[c], "%s on a given correction, component %d of %d" % (case.name, c, ncomp))
    return got, m, o


def _mark_survives(case, got, ncomp):
    """one box, the ghost layer downloaded: the Neumann sides still hold the caller's mark"""
    for c in range(ncomp):
        (a,) = got[c]
        assert a.shape == tuple(n + 2 for n in case.n)
        faces = [a[0, 1:-1, 1:-1], a[-1, 1:-1, 1:-1], a[1:-1, 0, 1:-1], a[1:-1, -1, 1:-1], a[1:-1, 1:-1, 0], a[1:-1, 1:-1, -1]]
        for side, face in enumerate(faces):
            if case.ops[c].bc[side] == N:
                np.testing.assert_array_equal(face, GHOST_MARK + c)


# ---- 1. no Dirichlet side anywhere, operators differing in the pair only: the DIRI = false forms ------------------------------
PAIR_OPS = [Op([N] * 6, [0] * 6, 1.0, -0.01), Op([N] * 6, [0] * 6, 1.0, -0.003), Op([N] * 6, [0] * 6, 0.5, -0.01),
            Op([N] * 6, [0] * 6, 2.0, -0.02)]
PAIR_LAYOUTS = {c.name: c for c in [
    _lay("wide", "pairs", PAIR_OPS),
    _lay("ragged", "pairs", PAIR_OPS),
    _lay("ragged", "pairs-periodic-xy", PAIR_OPS, periodic=(True, True, False)),
    _lay("extra-wide", "pairs", PAIR_OPS),
]}
PAIR_ORACLE = ("wide/pairs", "ragged/pairs-periodic-xy")   # also the oracle, for the (0.5, -0.01) component


def _only_different_operators(ncomp, m, o):
    """two fields go as one launch, three as one (from zero and the residual) or as 2 + 1 with the odd field in the single-field
    kernel: every N-field launch then pairs fields of different operators, none of which has a Dirichlet side"""
    assert o > 0, "no N-field launch carried different operators"
    if ncomp in (2, 3):
        assert o == m, (o, m)


@pytest.mark.parametrize("ncomp", [2, 3, 4])
@pytest.mark.parametrize("name", list(PAIR_LAYOUTS))
def test_pairs_only_vcycle_from_zero(oracle, name, ncomp):
    """1/1/1: the sweep from zero on two (four: 2 + 2) and three fields; 2/2/2: the plain two-field sweep too"""
    case = PAIR_LAYOUTS[name]
    for sweeps in (1, 2):
        m, o = _from_zero(oracle, case, ncomp, sweeps, oracle_comp=2 if name in PAIR_ORACLE else None)
        _only_different_operators(ncomp, m, o)


@pytest.mark.parametrize("ncomp", [2, 3, 4])
@pytest.mark.parametrize("name", list(PAIR_LAYOUTS))
def test_pairs_only_vcycle_on_a_given_correction(oracle, name, ncomp):
    """plain sweeps on depth 0 from the first one on; extra-wide: the ghost layer compared too, the mark on every side"""
    case = PAIR_LAYOUTS[name]
    xwide = name.startswith("extra-wide")
    got, m, o = _given(oracle, case, ncomp, ghost=(1, 1, 1) if xwide else (0, 0, 0))
    _only_different_operators(ncomp, m, o)
    if xwide:
        _mark_survives(case, got, ncomp)


# ---- 2. components that differ in alpha; a Poisson component with Dirichlet sides ----------------------------------------------
ALPHA_OPS = [Op([D, D, N, N, N, N], [0.25, -0.5, 0, 0, 0, 0]),
             Op([N, N, D, D, N, N], [0, 0, 0.75, 0.1, 0, 0], 0.0, 1.0),        # Poisson: Dirichlet sides, no null space
             Op([N, N, N, N, D, D], [0, 0, 0, 0, -0.3, 0.6], 3.0, -0.01),
             Op([N] * 6, [0] * 6, 0.25, BETA_SCALAR)]
ALPHA_LAYOUTS = {c.name: c for c in [_lay("wide", "alphas", ALPHA_OPS), _lay("ragged", "alphas", ALPHA_OPS)]}


@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("name", list(ALPHA_LAYOUTS))
def test_alphas_vcycle_from_zero(oracle, name, ncomp):
    case = ALPHA_LAYOUTS[name]
    for sweeps in (1, 2):
        m, o = _from_zero(oracle, case, ncomp, sweeps, oracle_comp=1 if name == "wide/alphas" else None)
        assert o > 0
        if ncomp == 3:
            assert o == m, (o, m)


@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("name", list(ALPHA_LAYOUTS))
def test_alphas_vcycle_on_a_given_correction(oracle, name, ncomp):
    got, m, o = _given(oracle, ALPHA_LAYOUTS[name], ncomp)
    assert o > 0


def test_heat_step_multi_with_components_created_with_another_alpha(oracle):
    """backward Euler, (aCoef I - dt bCoef L): create-time pairs (1, 1), (1, 0.3), (2, 1), (1, 1) -- set_alpha_beta(1, -dt)
    must scale each operator kept aside by its OWN pair, aCoef included"""
    from somar_amd import api as F
    so = oracle
    pairs = [(1.0, 1.0), (1.0, 0.3), (2.0, 1.0), (1.0, 1.0)]
    ops = [Op(o.bc, o.values, a, b) for o, (a, b) in zip(OPS, pairs)]
    case = _lay("wide", "heat-alphas", ops)
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    old = [so.random_field(grids, 61 + c, (1, 1, 1), dom.box) for c in range(4)]
    src = [so.random_field(grids, 71 + c, (0, 0, 0), dom.box) for c in range(4)]
    dt = 0.01
    seq = []
    for c in range(4):
        s = _solver(_own(case, c), prob, 1e-8, 20, ops[c].values)
        try:
            upload(s, F.F_HEAT_OLD, old[c])
            upload(s, F.F_HEAT_SRC, src[c])
            st = s.heatStep(0, dt, zeroPhi=True)
            seq.append((download_valid(s, F.F_PHI, grids), dict(st)))
        finally:
            s.undefine()
    s = _multi_solver(case, prob, 4, eps=1e-8, imax=20, norm_thresh=None)
    try:
        for c in range(4):
            _up(s, c, F.F_HEAT_OLD, old[c])
            _up(s, c, F.F_HEAT_SRC, src[c])
        stats = s.heatStepMulti(0, dt, zeroPhi=True)
        _reaches_ops(s, 4, case.K)
        assert [s.getCompOp(c)[2:4] for c in range(4)] == pairs   # the pairs set_alpha_beta scales stay the create-time ones
        for c in range(4):
            assert stats[c]["iters"] > 0
            _same(_down(s, c, F.F_PHI, grids), seq[c][0], "phi of component %d" % c)
            for k in STAT_KEYS:
                assert stats[c][k] == seq[c][1][k], (c, k, stats[c][k], seq[c][1][k])
    finally:
        s.undefine()


@pytest.mark.parametrize("scheme", [0, 2])
def test_heat_step_multi_in_the_sequential_fallback_with_other_alphas(oracle, monkeypatch, scheme):
    """32^3 under the library's own thresholds: K = 0, heatStepMulti is a loop over heatStep with the component's operator IN
    PLACE -- set_alpha_beta then runs with the live pair a component's and the handle's own waiting among the operators kept
    aside (backward Euler: once per component; TGA: four times).  The same create-time pairs as above."""
    from somar_amd import api as F
    for k in ("SOMAR_FUSED_MIN_CELLS", "SOMAR_MARCH_MIN_CELLS", "SOMAR_GRAPH_CELLS"):
        monkeypatch.delenv(k, raising=False)
    so = oracle
    pairs = [(1.0, 1.0), (1.0, 0.3), (2.0, 1.0), (1.0, 1.0)]
    ops = [Op(o.bc, o.values, a, b) for o, (a, b) in zip(OPS, pairs)]
    case = _layout("small/heat-alphas", (32, 32, 32), 16, (1.0, 1.0, 1.0), 0, None, None, ops=ops)
    case.alpha, case.beta = pairs[0]
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    old = [so.random_field(grids, 61 + c, (1, 1, 1), dom.box) for c in range(4)]
    src = [so.random_field(grids, 71 + c, (0, 0, 0), dom.box) for c in range(4)]
    dt = 0.01
    seq = []
    for c in range(4):
        s = _solver(_own(case, c), prob, 1e-8, 20, ops[c].values)
        try:
            upload(s, F.F_HEAT_OLD, old[c])
            upload(s, F.F_HEAT_SRC, src[c])
            st = s.heatStep(scheme, dt, zeroPhi=True)
            seq.append((download_valid(s, F.F_PHI, grids), dict(st)))
        finally:
            s.undefine()
    s = _multi_solver(case, prob, 4, eps=1e-8, imax=20, norm_thresh=None)
    try:
        for again in range(2):   # the second step starts from coefficients the first one scaled
            for c in range(4):
                _up(s, c, F.F_HEAT_OLD, old[c])
                _up(s, c, F.F_HEAT_SRC, src[c])
            stats = s.heatStepMulti(scheme, dt, zeroPhi=True)
            assert s.getComponents() == (4, 0, 0) and s.opLaunches() == 0
            assert [s.getCompOp(c)[2:4] for c in range(4)] == pairs
            for c in range(4):
                assert stats[c]["iters"] > 0
                _same(_down(s, c, F.F_PHI, grids), seq[c][0], "step %d, scheme %d, phi of component %d" % (again, scheme, c))
                for k in STAT_KEYS:
                    assert stats[c][k] == seq[c][1][k], (again, scheme, c, k, stats[c][k], seq[c][1][k])
    finally:
        s.undefine()


# ---- 3. two components with one own operator that is not the handle's -----------------------------------------------------------
SHARED_OPS = [OPS[0], OPS[1], OPS[2], OPS[2]]             # (a): 2 and 3 alike, 1 another
HANDLE_OPS = [OPS[0]] * 4                                  # (b): own operators equal to the handle's in every entry
LEFTOVER_OPS = [OPS[0], OPS[2], OPS[2], OPS[3]]            # (c): 1 and 2 alike (the fourth only fills the reference lists)
SHARED_LAYOUTS = {c.name: c for c in [_lay(kind, tag, ops) for kind in ("wide", "ragged")
                                      for tag, ops in (("shared-23", SHARED_OPS), ("as-handle", HANDLE_OPS), ("shared-12", LEFTOVER_OPS))]}


@pytest.mark.parametrize("kind", ["wide", "ragged"])
def test_two_components_share_an_own_operator(oracle, kind):
    """(a) four components go 2 + 2: (0, 1) differ, (2, 3) share an operator that is not the handle's -- the shared-operator
    kernel runs under THEIR StencilParams (Dirichlet in z, where the handle has Dirichlet in x)"""
    case = SHARED_LAYOUTS[kind + "/shared-23"]
    for sweeps in (1, 2):
        m, o = _from_zero(oracle, case, 4, sweeps)
        assert 0 < o < m, (o, m)
    got, m, o = _given(oracle, case, 4)
    assert 0 < o < m, (o, m)


@pytest.mark.parametrize("kind", ["wide", "ragged"])
def test_own_operators_equal_to_the_handles(oracle, kind):
    """(b) setCompOp with the handle's operator: own (getCompOp(c)[4], asserted by _set_ops), yet no launch differs"""
    case = SHARED_LAYOUTS[kind + "/as-handle"]
    for sweeps in (1, 2):
        m, o = _from_zero(oracle, case, 3, sweeps)
        assert m > 0 and o == 0, (o, m)
    got, m, o = _given(oracle, case, 3)
    assert m > 0 and o == 0, (o, m)


# ---- 5. (and 3c) solves: active sets, bottom kinds, a component without a cycle ------------------------------------------------
# Right-hand sides as tests/test_gpu_multi_ops.py reasons (a V-cycle contracts the residual by a factor between 0.05 and 0.5):
# "small", smooth with maximum 1.5 NORM_THRESH: below NORM_THRESH after one or two cycles; "large", 100 NORM_THRESH: after 2
# to 7, and later than "small" (asserted on the references); "random", of order one: IMAX; "zero", identically zero: no cycle.  Wall values scaled by WALL.  (A right-hand side that is
# merely below NORM_THRESH, or a zero one under inhomogeneous walls, does not serve for "no cycle": a solve that ends without a
# cycle on a residual that is not zero has status 2, "blew up", on either path, and the binding raises.  The case without a
# cycle therefore runs with forceHomogeneous = True.)
# Initial guesses where zero_phi is False: zero for the smooth ones, random for the random ones.
AMPLITUDE = {"zero": 0.0, "small": 1.5 * NORM_THRESH, "large": 100 * NORM_THRESH}
_SOLVE_REFS = {}


def _solve_inputs(so, case, prob, c, kind):
    dom, grids = prob[0], prob[1]
    if kind == "random":
        return so.random_field(grids, 11 + c, (0, 0, 0), dom.box), so.random_field(grids, 53 + c, (1, 1, 1), dom.box)
    return _smooth_field(so, grids, dom, case.n, AMPLITUDE[kind]), so.LevelData(grids, 1, (1, 1, 1))


def _solve_ref(so, case, prob, c, kind, zero_phi, force_homogeneous):
    """component c's solve on a separate handle: (phi, stats, history, bottomKind after it); once per case and input"""
    from somar_amd import api as F
    key = (case.name, c, kind, zero_phi, force_homogeneous)
    if key not in _SOLVE_REFS:
        rhs, guess = _solve_inputs(so, case, prob, c, kind)
        s = _solver(_own(case, c), prob, EPS, IMAX, case.ops[c].values, NORM_THRESH)
        try:
            upload(s, F.F_RHS, rhs)
            if not zero_phi:
                upload(s, F.F_PHI, guess)
            st = s.solveResident(zeroPhi=zero_phi, forceHomogeneous=force_homogeneous)
            _SOLVE_REFS[key] = (download_valid(s, F.F_PHI, prob[1]), dict(st), [float(v) for v in F.last_history()],
                                s.bottomKind())
        finally:
            s.undefine()
    return _SOLVE_REFS[key]


def _solve(so, case, kinds, zero_phi=True, force_homogeneous=False):
    """solveMulti on len(kinds) components against the separate handles; -> (reference iteration counts, reference bottom
    kinds, launches, op launches).  A component without a cycle ("zero") reports the bottom solver's counts as the solve before
    it left them (tests/test_gpu_multi.py, test_component_without_a_cycle_first_reports_the_counts_before_the_call): here those
    of the component before it, whose separate handle holds them."""
    from somar_amd import api as F
    ncomp = len(kinds)
    case = _with_small_walls(case)
    prob = problem(so, case)
    grids = prob[1]
    refs = [_solve_ref(so, case, prob, c, kinds[c], zero_phi, force_homogeneous) for c in range(ncomp)]
    s = _multi_solver(case, prob, ncomp)
    try:
        _reaches_layout(s, case, case.K, [tuple(r) for r in s.mgRefRatios()])
        for c in range(ncomp):
            rhs, guess = _solve_inputs(so, case, prob, c, kinds[c])
            _up(s, c, F.F_RHS, rhs)
            if not zero_phi:
                _up(s, c, F.F_PHI, guess)
        stats = s.solveMulti(zeroPhi=zero_phi, forceHomogeneous=force_homogeneous)
        m, o = _counts(s, ncomp, case.K)
        for c in range(ncomp):
            phi, st, hist, kind = refs[c]
            print("%s component %d (%s): %d V-cycles, exit %d, bottom %d/%d kind %d, final/initial %.3e" % (
                case.name, c, kinds[c], st["iters"], st["exitStatus"], st["bottom_iters"], st["bottom_exit"], kind,
                st["final_rnorm"] / max(st["initial_rnorm"], 1e-300)))
            _same(_down(s, c, F.F_PHI, grids), phi, "phi of component %d" % c)
            expect = dict(st)
            if st["iters"] == 0:
                assert c > 0 and refs[c - 1][1]["iters"] > 0
                expect["bottom_iters"], expect["bottom_exit"] = refs[c - 1][1]["bottom_iters"], refs[c - 1][1]["bottom_exit"]
            for k in STAT_KEYS:
                assert stats[c][k] == expect[k], (c, k, stats[c][k], expect[k])
            assert s.compHistory(c) == hist, c
    finally:
        s.undefine()
    return [r[1]["iters"] for r in refs], [r[3] for r in refs], m, o


SOLVE_LAYOUTS = {"wide": _lay("wide", "ops", OPS), "ragged": _lay("ragged", "ops-high", OPS_HIGH)}


BOTH_WAYS_ON_WIDE = [("wide", True), ("wide", False), ("ragged", True)]   # zero_phi both ways on the wide layout


def _bottom_kinds_differ(name, kinds, cycled):
    """the separate handles prove it.  ragged (OPS_HIGH): an operator with a Dirichlet side takes the host-loop BiCGStab (0),
    one without -- the all-Neumann handle and the scalar -- the one-launch solver (1 or 2), so the bottom counts solveMulti
    carries from component to component cross that boundary.  wide: the bottom level is one box of 16 x 12 x 12 = 2304
    cells, more than the one-launch kernels take, so every operator runs the host loop there."""
    ops = SOLVE_LAYOUTS[name].ops
    if name == "wide":
        assert all(kinds[c] == 0 for c in cycled), kinds
        return
    for c in cycled:
        assert (kinds[c] == 0) == (D in ops[c].bc), (c, kinds)
    assert len({kinds[c] != 0 for c in cycled}) == 2, kinds


@pytest.mark.parametrize("name,zero_phi", BOTH_WAYS_ON_WIDE)
def test_solve_multi_active_sets_without_component_0(oracle, name, zero_phi):
    """(i) the active sets {0, 1, 2, 3}, {1, 2, 3}, {1, 3}"""
    it, kinds, m, o = _solve(oracle, SOLVE_LAYOUTS[name], ["small", "random", "large", "random"], zero_phi)
    assert 0 < it[0] < it[2] < IMAX == it[1] == it[3], it
    assert 0 < o <= m
    _bottom_kinds_differ(name, kinds, range(4))


@pytest.mark.parametrize("name,zero_phi", BOTH_WAYS_ON_WIDE)
def test_solve_multi_active_sets_that_are_not_contiguous(oracle, name, zero_phi):
    """(ii) the active sets {0, 1, 2, 3}, {0, 2, 3}, {0, 2}"""
    it, kinds, m, o = _solve(oracle, SOLVE_LAYOUTS[name], ["random", "small", "random", "large"], zero_phi)
    assert 0 < it[1] < it[3] < IMAX == it[0] == it[2], it
    assert 0 < o <= m
    _bottom_kinds_differ(name, kinds, range(4))


@pytest.mark.parametrize("name", ["wide", "ragged"])
def test_solve_multi_component_without_a_cycle_among_own_operators(oracle, name):
    """(iii) as (i) with component 1 below NORM_THRESH from the start (zero, homogeneous walls): the sets {0, 2, 3}, {2, 3},
    {3}; its bottom counts are the ones component 0's solve left"""
    it, kinds, m, o = _solve(oracle, SOLVE_LAYOUTS[name], ["small", "zero", "large", "random"], True, force_homogeneous=True)
    assert it[1] == 0 and 0 < it[0] < it[2] < IMAX == it[3], it
    assert 0 < o <= m
    _bottom_kinds_differ(name, kinds, (0, 2, 3))


@pytest.mark.parametrize("kind", ["wide", "ragged"])
def test_solve_multi_leaves_a_pair_with_one_operator_that_is_not_the_handles(oracle, kind):
    """(3c) component 0 leaves first; the pair (1, 2) then launches with O.P[0] their operator, not the handle's"""
    it, kinds, m, o = _solve(oracle, SHARED_LAYOUTS[kind + "/shared-12"], ["small", "random", "random"], True)
    assert 0 < it[0] < IMAX == it[1] == it[2], it
    assert 0 < o < m, (o, m)


# ---- 4. periodic directions ------------------------------------------------------------------------------------------------------
# The operators as getCompOp must report them: the handle's entries (Neumann, 0.0) in the periodic directions.  What setCompOp is
# handed there is type 7 and value 99.0 (_dirty).
PERIODIC_XY_OPS = [Op([N, N, N, N, D, N], [0, 0, 0, 0, -0.3, 0]),
                   Op([N, N, N, N, N, D], [0, 0, 0, 0, 0, 0.6]),
                   Op([N, N, N, N, D, D], [0, 0, 0, 0, 0.25, -0.5]),
                   Op([N] * 6, [0] * 6, beta=BETA_SCALAR)]
PERIODIC_Y_OPS = [Op([D, N, N, N, N, D], [0.25, 0, 0, 0, 0, 0.6]),
                  Op([N, D, N, N, D, N], [0, -0.5, 0, 0, -0.3, 0]),
                  Op([D, D, N, N, N, N], [0.75, 0.1, 0, 0, 0, 0]),
                  Op([N] * 6, [0] * 6, beta=BETA_SCALAR)]
PERIODIC_LAYOUTS = {c.name: c for c in [
    _lay("ragged", "periodic-xy", PERIODIC_XY_OPS, periodic=(True, True, False)),
    _lay("anisotropic", "periodic-y", PERIODIC_Y_OPS, periodic=(False, True, False)),
]}


def _dirty(case):
    def passed(op):
        bc = [7 if case.periodic[i // 2] else b for i, b in enumerate(op.bc)]
        values = [99.0 if case.periodic[i // 2] else v for i, v in enumerate(op.values)]
        return bc, values
    return passed


@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("name", list(PERIODIC_LAYOUTS))
def test_periodic_directions_vcycle_from_zero(oracle, name, ncomp):
    case = PERIODIC_LAYOUTS[name]
    for sweeps in (1, 2):
        m, o = _from_zero(oracle, case, ncomp, sweeps, passed=_dirty(case), oracle_comp=2 if name == "ragged/periodic-xy" else None)
        assert o > 0


@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("name", list(PERIODIC_LAYOUTS))
def test_periodic_directions_vcycle_on_a_given_correction(oracle, name, ncomp):
    case = PERIODIC_LAYOUTS[name]
    got, m, o = _given(oracle, case, ncomp, passed=_dirty(case))
    assert o > 0


def test_periodic_directions_solve_multi(oracle):
    from somar_amd import api as F
    so = oracle
    case = _with_small_walls(PERIODIC_LAYOUTS["ragged/periodic-xy"])
    prob = problem(so, case)
    grids = prob[1]
    kinds = ["large", "small", "random"]
    refs = [_solve_ref(so, case, prob, c, kinds[c], True, False) for c in range(3)]
    it = [r[1]["iters"] for r in refs]
    assert 0 < it[1] < it[0] < IMAX == it[2], it
    s = _solver(case, prob, EPS, IMAX, case.ops[0].values, NORM_THRESH)
    try:
        s.setComponents(3)
        _set_ops(s, case, 3, _dirty(case))
        _reaches_layout(s, case, case.K, [tuple(r) for r in s.mgRefRatios()])
        for c in range(3):
            _up(s, c, F.F_RHS, _solve_inputs(so, case, prob, c, kinds[c])[0])
        stats = s.solveMulti(zeroPhi=True)
        _reaches_ops(s, 3, case.K)
        for c in range(3):
            phi, st, hist, kind = refs[c]
            _same(_down(s, c, F.F_PHI, grids), phi, "phi of component %d" % c)
            for k in STAT_KEYS:
                assert stats[c][k] == st[k], (c, k, stats[c][k], st[k])
            assert s.compHistory(c) == hist, c
    finally:
        s.undefine()


# ---- 6. setAlphaAndBeta with own operators, outside heat steps -----------------------------------------------------------------
# create-time pairs as in the heat-step test: (1, 1) for the three with walls, (1, 0.3) for the all-Neumann scalar
SCALED_OPS = [Op(o.bc, o.values, 1.0, 0.3 if c == 3 else 1.0) for c, o in enumerate(OPS)]
SCALED = _lay("wide", "scaled", SCALED_OPS)
SCALE = (1.0, -0.02)
# Under the suite's SOMAR_GRAPH_CELLS = 4096 no depth of this layout is graph-replayed: its bottom level, 16 x 12 x 12, is
# the first one that small, and the legs start above the bottom.  With 18432 = 32 x 24 x 24 depth 2 is the seam: K drops to 2,
# which proves it, and every operator owns a captured pair of legs from there down.
GRAPH_CELLS_DEPTH_2 = 32 * 24 * 24
_SCALED_REFS = {}


def _scaled_refs(so, graph_cells=None):
    """per component: a separate handle put through vcycleFromZero, setAlphaAndBeta(SCALE), vcycleFromZero twice; and the
    handle's operator, scaled, on component 3's residual (what component 3 cycles to after resetCompOp).  Once per value of
    SOMAR_GRAPH_CELLS, which the caller has set."""
    from somar_amd import api as F
    if graph_cells not in _SCALED_REFS:
        prob = problem(so, SCALED)
        dom, grids = prob[0], prob[1]
        res = [so.random_field(grids, 5 + c, (0, 0, 0), dom.box) for c in range(4)]
        seq = []
        for c in range(4):
            s = gpu_solver(_own(SCALED, c), prob)
            try:
                calls = []
                for call in range(3):
                    if call == 1:
                        s.setAlphaAndBeta(*SCALE)
                    upload(s, F.F_RES, res[c])
                    s.vcycleFromZero(F.F_CORR, F.F_RES)
                    calls.append(download_valid(s, F.F_CORR, grids))
                if c == 0:
                    upload(s, F.F_RES, res[3])
                    s.vcycleFromZero(F.F_CORR, F.F_RES)
                    reset3 = download_valid(s, F.F_CORR, grids)
            finally:
                s.undefine()
            assert any(not np.array_equal(a, b) for a, b in zip(calls[0], calls[1])), "the scaling changed nothing"
            seq.append(calls)
        _SCALED_REFS[graph_cells] = (prob, res, seq, reset3)
    return _SCALED_REFS[graph_cells]


def _scaled_call(s, prob, res, seq, call, what, comps=range(4)):
    from somar_amd import api as F
    for c in range(4):
        _up(s, c, F.F_RES, res[c])
    s.vcycleMulti(True)
    for c in comps:
        _same(_down(s, c, F.F_CORR, prob[1]), seq[c][call], "%s, component %d" % (what, c))


@pytest.mark.parametrize("graph_cells", [None, GRAPH_CELLS_DEPTH_2], ids=["no-graph-legs", "graph-legs-from-depth-2"])
def test_set_alpha_beta_scales_the_operators_kept_aside_and_drops_their_graphs(oracle, monkeypatch, graph_cells):
    """(a) with graph legs the first call captures every operator's pair under the create-time coefficients; after
    setAlphaAndBeta the second call must capture them again (a stale graph would replay the old coefficients), the third
    replays"""
    K = SCALED.K
    if graph_cells is not None:
        monkeypatch.setenv("SOMAR_GRAPH_CELLS", str(graph_cells))
        K = 2
    prob, res, seq, reset3 = _scaled_refs(oracle, graph_cells)
    s = gpu_solver(SCALED, prob)
    try:
        assert graph_cells is None or s.tuning("GRAPH_CELLS") == graph_cells
        s.setComponents(4)
        _set_ops(s, SCALED, 4)
        _reaches_layout(s, SCALED, K, [tuple(r) for r in s.mgRefRatios()])
        m = o = 0
        for call in range(3):
            if call == 1:
                s.setAlphaAndBeta(*SCALE)
            _scaled_call(s, prob, res, seq, call, "call %d" % call)
            m, o = _reaches_ops(s, 4, K, m, o)   # both counters grew in this call
        assert [s.getCompOp(c)[2:4] for c in range(4)] == [(op.alpha, op.beta) for op in SCALED_OPS]
    finally:
        s.undefine()


def test_set_comp_op_after_set_alpha_beta_is_scaled_too(oracle):
    """(b) ab_scale_: an operator set after setAlphaAndBeta runs scaled, and reports the unscaled pair; (c) resetCompOp after
    the scaling: the component cycles as the handle does"""
    from somar_amd import api as F
    prob, res, seq, reset3 = _scaled_refs(oracle)
    s = gpu_solver(SCALED, prob)
    try:
        s.setComponents(4)
        s.setAlphaAndBeta(*SCALE)
        _set_ops(s, SCALED, 4)   # (asserts that getCompOp returns the pairs as given)
        _scaled_call(s, prob, res, seq, 1, "setCompOp after setAlphaAndBeta")
        m, o = _reaches_ops(s, 4, SCALED.K)
        s.resetCompOp(3)
        assert s.getCompOp(3) == s.getCompOp(0)
        _scaled_call(s, prob, res, seq, 2, "after resetCompOp(3)", comps=range(3))
        _reaches_ops(s, 4, SCALED.K, m, o)
        _same(_down(s, 3, F.F_CORR, prob[1]), reset3, "component 3 under the handle's scaled operator")
    finally:
        s.undefine()


# ---- 7. a metric refresh that changes the metric -----------------------------------------------------------------------------
REFRESH_LAYOUTS = {"ops-high": _lay("ragged", "refresh-ops-high", OPS_HIGH), "ops": _lay("ragged", "refresh-ops", OPS)}
REFRESH_L = (1.0, 1.3, 0.6)   # the stretch s_a = 1 + 0.3 sin(2 pi x_a / L_a + a) with other periods than RAGGED_L
_REFRESH_REFS = {}


def _write_metric(s, metric):
    Jgup, Jinv = metric
    with s.metricUpdate():
        for q in range(s.num_local_patches):
            _, _, gi = s.patch_box(q)
            s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)], np.asfortranarray(Jinv[gi].a[..., 0]))


def _refresh_inputs(so, case):
    prob = problem(so, case)
    dom, grids, dx = prob[0], prob[1], prob[2]
    metric = so.make_diagonal_metric(grids, dx, REFRESH_L, 3, "stretched", domain=dom)
    refs = _given_refs(so, case, (1, 1, 1))   # residuals and marked corrections (its cycles are under the first metric)
    return prob, metric, refs[1], refs[2]


def _refresh_refs(so, case):
    """per component on a separate handle: the cycle from zero before the refresh, after it, and the cycle on the given
    correction after it with one ghost layer"""
    from somar_amd import api as F
    if case.name not in _REFRESH_REFS:
        prob, metric, res, cor = _refresh_inputs(so, case)
        grids = prob[1]
        seq = []
        for c in range(4):
            s = gpu_solver(_own(case, c), prob)
            try:
                upload(s, F.F_RES, res[c])
                s.vcycleFromZero(F.F_CORR, F.F_RES)
                before = download_valid(s, F.F_CORR, grids)
                _write_metric(s, metric)
                upload(s, F.F_RES, res[c])
                s.vcycleFromZero(F.F_CORR, F.F_RES)
                after = download_valid(s, F.F_CORR, grids)
                upload(s, F.F_RES, res[c])
                upload(s, F.F_CORR, cor[c])
                s.vcycle(F.F_CORR, F.F_RES)
                given = [s.download(F.F_CORR, q, (1, 1, 1)) for q in range(s.num_local_patches)]
            finally:
                s.undefine()
            assert any(not np.array_equal(a, b) for a, b in zip(before, after)), "the refresh changed nothing"
            seq.append((before, after, given))
        _REFRESH_REFS[case.name] = seq
    return _REFRESH_REFS[case.name]


@pytest.mark.parametrize("name", list(REFRESH_LAYOUTS))
def test_metric_refresh_that_changes_the_metric(oracle, name):
    """ops-high: an all-Neumann handle whose component 1 has Dirichlet HIGH sides in x and y -- the face copiers the handle got
    from ensure_face_copiers must carry the new coefficients; every operator is probed again, the batched depths rebuilt"""
    from somar_amd import api as F
    so, case = oracle, REFRESH_LAYOUTS[name]
    seq = _refresh_refs(so, case)
    prob, metric, res, cor = _refresh_inputs(so, case)
    grids = prob[1]
    s = gpu_solver(case, prob)
    try:
        s.setComponents(4)
        _set_ops(s, case, 4)
        _reaches_layout(s, case, case.K, [tuple(r) for r in s.mgRefRatios()])
        for c in range(4):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        m, o = _reaches_ops(s, 4, case.K)
        for c in range(4):
            _same(_down(s, c, F.F_CORR, grids), seq[c][0], "before the refresh, component %d" % c)
        _write_metric(s, metric)
        for c in range(1, 4):
            assert s.getCompOp(c) == (case.ops[c].bc, [float(v) for v in case.ops[c].values], case.ops[c].alpha, case.ops[c].beta, True)
        _reaches_layout(s, case, case.K, [tuple(r) for r in s.mgRefRatios()])
        for c in range(4):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        m, o = _reaches_ops(s, 4, case.K, m, o)
        for c in range(4):
            _same(_down(s, c, F.F_CORR, grids), seq[c][1], "after the refresh, component %d" % c)
        for c in range(4):
            _up(s, c, F.F_RES, res[c])
            _up(s, c, F.F_CORR, cor[c])
        s.vcycleMulti(False)
        _reaches_ops(s, 4, case.K, m, o)
        for c in range(4):
            got = [s.downloadComp(c, F.F_CORR, q, (1, 1, 1)) for q in range(s.num_local_patches)]
            _same(got, seq[c][2], "after the refresh, on a given correction with its ghost layer, component %d" % c)
    finally:
        s.undefine()


# ---- 8. face values on the handle with own operators -------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["face-values-then-ops", "ops-then-face-values"])
def test_face_values_on_the_handle_with_own_operators(oracle, order):
    """the handle's x-low side takes a smooth plane; exchange_op swaps the face-valued op lists out and in again around every
    turn of a component: component 0 solves as a separate handle with the same plane, and so does a plain solve afterwards"""
    from somar_amd import api as F
    so = oracle
    case = _with_small_walls(_lay("wide", "face-values", OPS))
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    j, k = np.meshgrid(np.arange(case.n[1]), np.arange(case.n[2]), indexing="ij")
    plane = WALL * (0.25 + 0.5 * np.cos(np.pi * (j + 0.5) / case.n[1]) * np.sin(2 * np.pi * (k + 0.5) / case.n[2]))
    kinds = ["large", "small", "random"]
    later = so.random_field(grids, 97, (0, 0, 0), dom.box)
    key = (case.name, "component 0")
    if key not in _SOLVE_REFS:
        a = _solver(_own(case, 0), prob, EPS, IMAX, case.ops[0].values, NORM_THRESH)
        try:
            a.setBCFaceValues(0, 0, plane)
            upload(a, F.F_RHS, _solve_inputs(so, case, prob, 0, kinds[0])[0])
            st = a.solveResident(zeroPhi=True)
            first = (download_valid(a, F.F_PHI, grids), dict(st), [float(v) for v in F.last_history()])
            upload(a, F.F_RHS, later)
            st = a.solveResident(zeroPhi=True)
            second = (download_valid(a, F.F_PHI, grids), dict(st))
            a.setBCFaceValues(0, 0, None)
            upload(a, F.F_RHS, _solve_inputs(so, case, prob, 0, kinds[0])[0])
            a.solveResident(zeroPhi=True)
            constant = download_valid(a, F.F_PHI, grids)
        finally:
            a.undefine()
        assert any(not np.array_equal(x, y) for x, y in zip(first[0], constant)), "the plane changed nothing"
        _SOLVE_REFS[key] = (first, second)
    first, second = _SOLVE_REFS[key]
    refs = [first] + [_solve_ref(so, case, prob, c, kinds[c], True, False)[:3] for c in (1, 2)]
    s = _solver(case, prob, EPS, IMAX, case.ops[0].values, NORM_THRESH)
    try:
        if order == "face-values-then-ops":
            s.setBCFaceValues(0, 0, plane)
        s.setComponents(3)
        _set_ops(s, case, 3)
        if order == "ops-then-face-values":
            s.setBCFaceValues(0, 0, plane)
        op0 = s.getCompOp(0)
        for c in range(3):
            _up(s, c, F.F_RHS, _solve_inputs(so, case, prob, c, kinds[c])[0])
        stats = s.solveMulti(zeroPhi=True, forceHomogeneous=False)
        _reaches_ops(s, 3, case.K)
        for c in range(3):
            phi, st, hist = refs[c]
            _same(_down(s, c, F.F_PHI, grids), phi, "phi of component %d" % c)
            for k_ in STAT_KEYS:
                assert stats[c][k_] == st[k_], (c, k_, stats[c][k_], st[k_])
            assert s.compHistory(c) == hist, c
        assert s.getCompOp(0) == op0
        upload(s, F.F_RHS, later)
        st = dict(s.solveResident(zeroPhi=True))
        _same(download_valid(s, F.F_PHI, grids), second[0], "phi of a plain solve after the multi call")
        for k_ in STAT_KEYS:
            assert st[k_] == second[1][k_], (k_, st[k_], second[1][k_])
        assert s.getCompOp(0) == op0
    finally:
        s.undefine()
