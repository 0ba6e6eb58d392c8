"""Components with their own operator on one handle (somar_comp_set_op): BC types, Dirichlet constants and (alpha, beta) per
component.  The specification is the one of solveMulti, extended: the multi calls leave component c exactly -- fields,
statistics, residual history, bit for bit -- as the single-field call would on a SEPARATE one-component handle created with
c's BC types, values and coefficients on the same geometry and metric.  Every comparison here is assert_array_equal against
such handles; in one layout component 2 is also held to the oracle's one_cycle for its operator, so that "both paths wrong
alike" cannot pass.

Operators, on a handle with alpha = 1, beta = -0.01 (free-slip walls per velocity component plus a no-flux scalar with another
diffusivity):
    component 0 (the handle)  [D, D, N, N, N, N]
    component 1               [N, N, D, D, N, N]
    component 2               [N, N, N, N, D, D]
    component 3               all Neumann, beta = -0.003
The components with Dirichlet sides carry different non-zero wall values.

Layouts: those of tests/test_gpu_multi.py and tests/test_gpu_mixed_kernels.py (the smallest at which the marching kernels can
go wrong): the 128-wide box (K = 3), the ragged four boxes without periodic directions, so that the sides run across the box
seams and the global index decides (K = 2), the same boxes with an all-Neumann HANDLE and a component whose Dirichlet sides are
the HIGH ones in x and y (the face copier a Neumann handle never built), extra-wide 256 x 24 x 24 (the last column cut by the
box, K = 4), and ratio-212.

Every case first proves it reached its target: batched_depths == K, and batched_launches and opLaunches both grew -- every
launch shape of the shared-operator kernels has its per-operator twin in the library (the sweep plain on two fields and from
zero on two and three, the residual on two and three, the residual + restriction on two)."""
import numpy as np
import pytest

from tests.helpers import download_valid, make_problem, upload
from tests.test_gpu_mixed_kernels import RAGGED_BOXES, RAGGED_N, WIDE_BOX, WIDE_N, WIDE_RATIOS, gpu_solver, oracle_cycle, problem, set_env
from tests.test_gpu_multi import (EPS, GHOST_MARK, IMAX, NORM_THRESH, RAGGED_WIDTHS, STAT_KEYS, WIDE_WIDTHS, XWIDE_BOX, XWIDE_N,
                                  XWIDE_RATIOS, XWIDE_WIDTHS, _case, _down, _raises, _reaches_layout, _same, _smooth_field, _solver,
                                  _up)

pytestmark = pytest.mark.gpu

D, N = 1, 0
ALPHA, BETA, BETA_SCALAR = 1.0, -0.01, -0.003


class Op:
    def __init__(self, bc, values, alpha=ALPHA, beta=BETA):
        self.bc, self.values, self.alpha, self.beta = bc, values, alpha, beta


OPS = [Op([D, D, N, N, N, N], [0.25, -0.5, 0, 0, 0, 0]),
       Op([N, N, D, D, N, N], [0, 0, 0.75, 0.1, 0, 0]),
       Op([N, N, N, N, D, D], [0, 0, 0, 0, -0.3, 0.6]),
       Op([N] * 6, [0] * 6, beta=BETA_SCALAR)]
# the handle all Neumann (no face copier of its own); component 1 with Dirichlet HIGH sides in x and y
OPS_HIGH = [Op([N] * 6, [0] * 6),
            Op([N, D, N, D, N, N], [0, 0.4, 0, -0.2, 0, 0]),
            Op([N, N, N, N, D, D], [0, 0, 0, 0, -0.3, 0.6]),
            Op([N] * 6, [0] * 6, beta=BETA_SCALAR)]


def _layout(name, n, boxes, L, K, widths, ratios, ops=OPS, tables=None, periodic=(False,) * 3):
    c = _case(name, n, boxes, periodic, L, ops[0].bc, None, K, widths=widths, ratios=ratios, tables=tables)
    c.ops = ops
    return c


LAYOUTS = {c.name: c for c in [
    _layout("wide", WIDE_N, WIDE_BOX, (1.0, 1.0, 1.0), 3, WIDE_WIDTHS, WIDE_RATIOS),
    _layout("ragged", RAGGED_N, RAGGED_BOXES, (1.25, 1.0, 0.5), 2, RAGGED_WIDTHS, [(2, 2, 2)] * 2),
    _layout("ragged-high-sides", RAGGED_N, RAGGED_BOXES, (1.25, 1.0, 0.5), 2, RAGGED_WIDTHS, [(2, 2, 2)] * 2, ops=OPS_HIGH),
    _layout("extra-wide", XWIDE_N, XWIDE_BOX, (1.0, 1.0, 1.0), 4, XWIDE_WIDTHS, XWIDE_RATIOS, tables="tall"),
    _layout("ratio-212", (64, 16, 64), 32, (1.0, 1.0, 1.0), 2, [[32] * 4, [16] * 4], [(2, 1, 2), (2, 1, 2)]),
]}


@pytest.fixture(autouse=True)
def _large_level_kernels(monkeypatch):
    set_env(monkeypatch.setenv)
    for k in ("SOMAR_NARROW_7PT", "SOMAR_NO_NARROW_TILES", "SOMAR_FUSED_ROWS", "SOMAR_ORDERED_REDUCE_MAX"):
        monkeypatch.delenv(k, raising=False)


def _own(case, c):
    """the case of a separate one-component handle with component c's operator"""
    op = case.ops[c]
    return _case("%s-op%d" % (case.name, c), case.n, case.boxes, case.periodic, case.L, op.bc, None, case.K, alpha=op.alpha,
                 beta=op.beta)


def _set_ops(s, case, ncomp, passed=None):
    """passed: None, or op -> the (BC types, values) handed to setCompOp in its place (what getCompOp reports stays the op's)"""
    for c in range(1, ncomp):
        op = case.ops[c]
        bc, values = passed(op) if passed else (op.bc, op.values)
        s.setCompOp(c, bc, values, op.alpha, op.beta)
        assert s.getCompOp(c) == (op.bc, [float(v) for v in op.values], op.alpha, op.beta, True)
    assert s.getCompOp(0) == (case.ops[0].bc, s.getCompOp(0)[1], case.ops[0].alpha, case.ops[0].beta, False)


def _reaches_ops(s, ncomp, K, launches=0, op_launches=0):
    n, k, m = s.getComponents()
    assert (n, k) == (ncomp, K), (n, k, ncomp, K)
    assert m > launches, "no N-field launch was issued"
    assert s.opLaunches() > op_launches, "no N-field launch carried different operators"
    assert s.opLaunches() <= m
    return m, s.opLaunches()


# ---- 1. the V-cycle kernels -------------------------------------------------------------------------------------------------
_CYCLE_REFS = {}


def _cycle_refs(so, case, sweeps):
    """per component: its residual field and the V-cycle from zero of a separate handle with its operator; computed once"""
    from somar_amd import api as F
    key = (case.name, sweeps)
    if key not in _CYCLE_REFS:
        prob = problem(so, case)
        dom, grids = prob[0], prob[1]
        res = [so.random_field(grids, 5 + c, (0, 0, 0), dom.box) for c in range(4)]
        seq = []
        for c in range(4):
            s = gpu_solver(_own(case, c), prob, sweeps=sweeps)
            try:
                upload(s, F.F_RES, res[c])
                s.vcycleFromZero(F.F_CORR, F.F_RES)
                seq.append(download_valid(s, F.F_CORR, grids))
                assert s.getComponents() == (1, 0, 0) and s.opLaunches() == 0
            finally:
                s.undefine()
        _CYCLE_REFS[key] = (prob, res, seq)
    return _CYCLE_REFS[key]


@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_vcycle_multi_is_the_cycle_of_a_separate_handle_per_component(oracle, name, ncomp):
    from somar_amd import api as F
    so, case = oracle, LAYOUTS[name]
    for sweeps in (1, 2):
        prob, res, seq = _cycle_refs(so, case, sweeps)
        grids = prob[1]
        s = gpu_solver(case, prob, sweeps=sweeps)
        try:
            s.setComponents(ncomp)
            _set_ops(s, case, ncomp)
            oratios = [tuple(r) for r in s.mgRefRatios()]
            _reaches_layout(s, case, case.K, oratios)
            for c in range(ncomp):
                _up(s, c, F.F_RES, res[c])
            s.vcycleMulti(True)
            _reaches_ops(s, ncomp, case.K)
            got = [_down(s, c, F.F_CORR, grids) for c in range(ncomp)]
        finally:
            s.undefine()
        for c in range(ncomp):
            assert all(float(np.max(np.abs(g))) > 0.0 for g in got[c])
            _same(got[c], seq[c], "%s %d/%d/%d component %d of %d vs a separate handle" % (name, sweeps, sweeps, sweeps, c, ncomp))
        if name == "wide":
            ora, ora_ratios = oracle_cycle(so, _own(case, 2), prob, res[2], sweeps)
            assert ora_ratios == oratios
            _same(got[2], ora, "%s component 2 of %d vs the oracle's one_cycle for its operator" % (name, ncomp))


_GIVEN_REFS = {}


def _given_refs(so, case, ghost):
    """per component: residual, given correction (ghost cells marked) and the V-cycle of a separate handle on it, with `ghost`
    layers of ghost cells; computed once per layout and left unchanged"""
    from somar_amd import api as F
    key = (case.name, ghost)
    if key not in _GIVEN_REFS:
        prob = problem(so, case)
        dom, grids = prob[0], prob[1]
        res = [so.random_field(grids, 21 + c, (0, 0, 0), dom.box) for c in range(4)]
        cor = [so.random_field(grids, 31 + c, (1, 1, 1), dom.box) for c in range(4)]
        for c in range(4):
            for g, f in zip(grids, cor[c].fabs):
                valid = np.array(f.view(g))
                f.a[...] = GHOST_MARK + c
                f.view(g)[...] = valid
        seq = []
        for c in range(4):
            s = gpu_solver(_own(case, c), prob)
            try:
                upload(s, F.F_RES, res[c])
                upload(s, F.F_CORR, cor[c])
                s.vcycle(F.F_CORR, F.F_RES)
                seq.append([s.download(F.F_CORR, q, ghost) for q in range(s.num_local_patches)])
            finally:
                s.undefine()
        _GIVEN_REFS[key] = (prob, res, cor, seq)
    return _GIVEN_REFS[key]


def _given_correction(so, case, ncomp, ghost=(0, 0, 0)):
    from somar_amd import api as F
    prob, res, cor, seq = _given_refs(so, case, ghost)
    s = gpu_solver(case, prob)
    try:
        s.setComponents(ncomp)
        _set_ops(s, case, ncomp)
        for c in range(ncomp):
            _up(s, c, F.F_RES, res[c])
            _up(s, c, F.F_CORR, cor[c])
        s.vcycleMulti(False)
        _reaches_ops(s, ncomp, case.K)
        got = [[s.downloadComp(c, F.F_CORR, q, ghost) for q in range(s.num_local_patches)] for c in range(ncomp)]
    finally:
        s.undefine()
    for c in range(ncomp):
        _same(got[c], seq[c], "%s, component %d of %d" % (case.name, c, ncomp))
    return got


@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_vcycle_multi_on_a_given_correction(oracle, name, ncomp):
    """from_zero = False: plain sweeps on depth 0 (four components: the pair of the Dirichlet-in-z field and the all-Neumann
    scalar with another beta); the Neumann sides' ghost cells hold the caller's mark, which no operator reads"""
    _given_correction(oracle, LAYOUTS[name], ncomp)


@pytest.mark.parametrize("ncomp", [3, 4])
def test_vcycle_multi_leaves_the_ghost_cells_as_a_separate_handle_does(oracle, ncomp):
    """extra-wide, the ghost layer compared too (tests/test_gpu_multi.py: the cut of the last column by the box).  Each
    component's Dirichlet sides have their ghost cells written by its own operator, the Neumann ones keep the caller's mark."""
    case = LAYOUTS["extra-wide"]
    got = _given_correction(oracle, case, ncomp, ghost=(1, 1, 1))
    for c in range(ncomp):
        (a,) = got[c]
        faces = [a[0, 1:-1, 1:-1], a[-1, 1:-1, 1:-1], a[1:-1, 0, 1:-1], a[1:-1, -1, 1:-1], a[1:-1, 1:-1, 0], a[1:-1, 1:-1, -1]]
        for side, face in enumerate(faces):
            if case.ops[c].bc[side] == N:
                np.testing.assert_array_equal(face, GHOST_MARK + c)


# ---- 2. solves ----------------------------------------------------------------------------------------------------------------
# The solves stop on the ABSOLUTE residual norm or on IMAX, as in tests/test_gpu_multi.py, whose reasoning carries over: a
# V-cycle contracts the residual by a factor between 0.05 and 0.5.  Right-hand sides: smooth with maximum 100 NORM_THRESH (below
# NORM_THRESH after 2 to 7 cycles), smooth with maximum 1.5 NORM_THRESH (after exactly one) and random of order one (IMAX).  The
# wall values of these solves are the operators' scaled by WALL: non-zero and different, but what they add to the residual
# (2 value J g / dx^2 < 1e5 value) stays two decades under NORM_THRESH, so that the counts above hold with inhomogeneous sides
# too; they still reach every bit that is compared (1e-4 of the right-hand side).  Initial guesses (zero_phi = False): zero for
# the two smooth components, random for the third.  The active set therefore shrinks twice in every variant.
WALL = 1e-19


def _solve_rhs(so, case, prob):
    dom, grids = prob[0], prob[1]
    return [_smooth_field(so, grids, dom, case.n, 100 * NORM_THRESH), _smooth_field(so, grids, dom, case.n, 1.5 * NORM_THRESH),
            so.random_field(grids, 11, (0, 0, 0), dom.box)]


def _with_small_walls(case):
    ops = [Op(o.bc, [v * WALL for v in o.values], o.alpha, o.beta) for o in case.ops]
    return _layout(case.name, case.n, case.boxes, case.L, case.K, case.widths, case.ratios, ops=ops, tables=case.tables,
                   periodic=case.periodic)


def _multi_solver(case, prob, ncomp, eps=EPS, imax=IMAX, norm_thresh=NORM_THRESH):
    s = _solver(case, prob, eps, imax, case.ops[0].values, norm_thresh)
    s.setComponents(ncomp)
    _set_ops(s, case, ncomp)
    return s


def _solve_both_ways(so, case, zero_phi, force_homogeneous, expect_K=None):
    from somar_amd import api as F
    case = _with_small_walls(case)
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    rhs = _solve_rhs(so, case, prob)
    guess = [so.LevelData(grids, 1, (1, 1, 1)), so.LevelData(grids, 1, (1, 1, 1)), so.random_field(grids, 53, (1, 1, 1), dom.box)]
    seq = []
    for c in range(3):
        s = _solver(_own(case, c), prob, EPS, IMAX, case.ops[c].values, NORM_THRESH)
        try:
            upload(s, F.F_RHS, rhs[c])
            if not zero_phi:
                upload(s, F.F_PHI, guess[c])
            st = s.solveResident(zeroPhi=zero_phi, forceHomogeneous=force_homogeneous)
            seq.append((download_valid(s, F.F_PHI, grids), dict(st), [float(v) for v in F.last_history()]))
        finally:
            s.undefine()
    s = _multi_solver(case, prob, 3)
    try:
        for c in range(3):
            _up(s, c, F.F_RHS, rhs[c])
            if not zero_phi:
                _up(s, c, F.F_PHI, guess[c])
        stats = s.solveMulti(zeroPhi=zero_phi, forceHomogeneous=force_homogeneous)
        K = case.K if expect_K is None else expect_K
        if K > 0:
            _reaches_ops(s, 3, K)
        else:
            assert s.getComponents() == (3, 0, 0) and s.opLaunches() == 0
        for c in range(3):
            print("%s component %d: %d V-cycles, exit %d, bottom %d/%d, final/initial %.3e" % (
                case.name, c, stats[c]["iters"], stats[c]["exitStatus"], stats[c]["bottom_iters"], stats[c]["bottom_exit"],
                stats[c]["final_rnorm"] / max(stats[c]["initial_rnorm"], 1e-300)))
            _same(_down(s, c, F.F_PHI, grids), seq[c][0], "phi of component %d" % c)
            for k in STAT_KEYS:
                assert stats[c][k] == seq[c][1][k], (c, k, stats[c][k], seq[c][1][k])
            assert s.compHistory(c) == seq[c][2], c
    finally:
        s.undefine()
    return stats


@pytest.mark.parametrize("force_homogeneous", [False, True])
@pytest.mark.parametrize("zero_phi", [True, False])
def test_solve_multi_is_three_solves_on_separate_handles(oracle, zero_phi, force_homogeneous):
    stats = _solve_both_ways(oracle, LAYOUTS["wide"], zero_phi, force_homogeneous)
    iters = [st["iters"] for st in stats]
    # the active set shrinks twice: the two smooth right-hand sides stop on the absolute norm, the smaller one first
    assert 0 < iters[1] < iters[0] < IMAX == iters[2], iters
    assert stats[0]["exitStatus"] == 8 and stats[1]["exitStatus"] == 8 and stats[2]["exitStatus"] == 2, stats


def test_solve_multi_without_graphs(oracle, monkeypatch):
    """SOMAR_GRAPH_CELLS = 0: no graph-replayed legs, every depth below the seam launch by launch with the operator in place"""
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", "0")
    _solve_both_ways(oracle, LAYOUTS["wide"], True, False, expect_K=3)


def test_sequential_fallback_with_default_thresholds(oracle, monkeypatch):
    """32^3 under the library's own thresholds: K = 0, every multi call is a loop over the single-field one with the
    component's operator -- and its own captured graphs -- swapped in.  Twice, so that the second call replays them."""
    from somar_amd import api as F
    for k in ("SOMAR_FUSED_MIN_CELLS", "SOMAR_MARCH_MIN_CELLS", "SOMAR_GRAPH_CELLS"):
        monkeypatch.delenv(k, raising=False)
    so = oracle
    case = _layout("small", (32, 32, 32), 16, (1.0, 1.0, 1.0), 0, None, None)
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    res = [so.random_field(grids, 5 + c, (0, 0, 0), dom.box) for c in range(4)]
    seq = []
    for c in range(4):
        s = gpu_solver(_own(case, c), prob)
        try:
            upload(s, F.F_RES, res[c])
            s.vcycleFromZero(F.F_CORR, F.F_RES)
            seq.append(download_valid(s, F.F_CORR, grids))
        finally:
            s.undefine()
    s = gpu_solver(case, prob)
    try:
        s.setComponents(4)
        _set_ops(s, case, 4)
        assert s.getComponents() == (4, 0, 0)
        for again in range(2):
            for c in range(4):
                _up(s, c, F.F_RES, res[c])
            s.vcycleMulti(True)
            for c in range(4):
                _same(_down(s, c, F.F_CORR, grids), seq[c], "call %d, component %d" % (again, c))
        assert s.getComponents() == (4, 0, 0) and s.opLaunches() == 0
    finally:
        s.undefine()


# ---- 3. heat steps: per-component diffusivity through set_alpha_beta ---------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_heat_step_multi_is_four_heat_steps_on_separate_handles(oracle, scheme):
    from somar_amd import api as F
    so = oracle
    # diffusivities: beta is the pair's second entry, (I - dt beta_c L); 1.0 for the velocities, 0.3 for the scalar
    ops = [Op(o.bc, o.values, 1.0, 0.3 if c == 3 else 1.0) for c, o in enumerate(OPS)]
    case = _layout("wide-heat", WIDE_N, WIDE_BOX, (1.0, 1.0, 1.0), 3, WIDE_WIDTHS, WIDE_RATIOS, ops=ops)
    case.alpha, case.beta = 1.0, 1.0
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
        for c in range(4):
            _up(s, c, F.F_HEAT_OLD, old[c])
            _up(s, c, F.F_HEAT_SRC, src[c])
        stats = s.heatStepMulti(scheme, dt, zeroPhi=True)
        _reaches_ops(s, 4, case.K)
        for c in range(4):
            assert stats[c]["iters"] > 0
            _same(_down(s, c, F.F_PHI, grids), seq[c][0], "scheme %d, phi of component %d" % (scheme, c))
            for k in STAT_KEYS:
                assert stats[c][k] == seq[c][1][k], (scheme, c, k)
    finally:
        s.undefine()


# ---- 4. the handle after the call ----------------------------------------------------------------------------------------------
def test_state_after_a_multi_call(oracle):
    from somar_amd import api as F
    so, case = oracle, LAYOUTS["ragged"]
    prob = problem(so, case)
    dom, grids, dx, Jgup, Jinv = prob
    rhs = so.random_field(grids, 11, (0, 0, 0), dom.box)
    res = [so.random_field(grids, 5 + c, (0, 0, 0), dom.box) for c in range(3)]
    refs = _cycle_refs(so, case, 2)[2]
    a = _solver(_own(case, 0), prob, 1e-8, 20, case.ops[0].values)
    try:
        upload(a, F.F_RHS, rhs)
        st0 = dict(a.solveResident(zeroPhi=True))
        phi0 = download_valid(a, F.F_PHI, grids)
        single = []
        for c in range(3):   # the reference of the shared operator: single-field cycles with the handle's operator
            upload(a, F.F_RES, res[c])
            a.vcycleFromZero(F.F_CORR, F.F_RES)
            single.append(download_valid(a, F.F_CORR, grids))
        a.setComponents(3)   # without setCompOp: the shared operator, and no launch of the new kernels
        for c in range(3):
            _up(a, c, F.F_RES, res[c])
        a.vcycleMulti(True)
        assert a.getComponents()[2] > 0 and a.opLaunches() == 0
        shared = [_down(a, c, F.F_CORR, grids) for c in range(3)]
        for c in range(3):
            _same(shared[c], single[c], "a handle that never called setCompOp, component %d" % c)
    finally:
        a.undefine()
    s = _multi_solver(case, prob, 3, eps=1e-8, imax=20, norm_thresh=None)
    try:
        for c in range(3):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        m, o = _reaches_ops(s, 3, case.K)
        for c in range(3):
            _same(_down(s, c, F.F_CORR, grids), refs[c], "component %d" % c)
        # the handle holds component 0's operator again: a plain solve is the separate handle's
        upload(s, F.F_RHS, rhs)
        st = dict(s.solveResident(zeroPhi=True))
        _same(download_valid(s, F.F_PHI, grids), phi0, "phi of a plain solve after the multi call")
        for k in STAT_KEYS:
            assert st[k] == st0[k], (k, st[k], st0[k])
        # a metric refresh (the same metric written again) keeps the operators
        with s.metricUpdate():
            for q in range(s.num_local_patches):
                _, _, gi = s.patch_box(q)
                s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                                 np.asfortranarray(Jinv[gi].a[..., 0]))
        assert s.getCompOp(1)[4] and s.getCompOp(2)[4]
        for c in range(3):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        m, o = _reaches_ops(s, 3, case.K, m, o)
        for c in range(3):
            _same(_down(s, c, F.F_CORR, grids), refs[c], "after the refresh, component %d" % c)
        # back to the shared operator
        s.resetCompOp(1)
        s.resetCompOp(2)
        assert s.getCompOp(1) == s.getCompOp(0)
        for c in range(3):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        assert s.opLaunches() == o and s.getComponents()[2] > m
        for c in range(3):
            _same(_down(s, c, F.F_CORR, grids), shared[c], "after resetCompOp, component %d" % c)
        # shrinking ncomp drops the operators of the components that go away
        s.setCompOp(2, case.ops[2].bc, case.ops[2].values, ALPHA, BETA)
        s.setComponents(2)
        s.setComponents(3)
        assert not s.getCompOp(2)[4]
    finally:
        s.undefine()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def _small(so):
    case = _layout("small", (32, 32, 32), 16, (1.0, 1.0, 1.0), 0, None, None)
    return gpu_solver(case, problem(so, case)), case


def test_refused_for_component_0_and_out_of_range(oracle):
    s, case = _small(oracle)
    try:
        op = case.ops[1]
        _raises(lambda: s.setCompOp(1, op.bc, op.values, ALPHA, BETA), "set_components")   # before set_components
        s.setComponents(3)
        _raises(lambda: s.setCompOp(0, op.bc, op.values, ALPHA, BETA), "component 0", "not settable")
        _raises(lambda: s.setCompOp(3, op.bc, op.values, ALPHA, BETA), "out of range")
        _raises(lambda: s.setCompOp(-1, op.bc, op.values, ALPHA, BETA), "out of range")
        assert not s.getCompOp(1)[4] and not s.getCompOp(2)[4]
    finally:
        s.undefine()


def test_refused_for_a_type_other_than_neumann_or_dirichlet(oracle):
    s, case = _small(oracle)
    try:
        s.setComponents(2)
        _raises(lambda: s.setCompOp(1, [N, N, 2, N, N, N], [0] * 6, ALPHA, BETA), "Neumann (0) or Dirichlet (1)")
        assert not s.getCompOp(1)[4]
    finally:
        s.undefine()


def test_refused_for_an_operator_with_a_null_space(oracle):
    from somar_amd import api as F
    so = oracle
    s, case = _small(so)
    try:
        s.setComponents(2)
        _raises(lambda: s.setCompOp(1, [N] * 6, [0] * 6, 0.0, 1.0), "null space")
        assert not s.getCompOp(1)[4] and s.getCompOp(1) == s.getCompOp(0)
        # nothing changed: the handle still cycles with its own operator
        prob = problem(so, case)
        res = so.random_field(prob[1], 5, (0, 0, 0), prob[0].box)
        upload(s, F.F_RES, res)
        s.vcycleFromZero(F.F_CORR, F.F_RES)
        got = download_valid(s, F.F_CORR, prob[1])
        s.setCompOp(1, [D] * 6, [0] * 6, 0.0, 1.0)   # Poisson with Dirichlet sides has none
        upload(s, F.F_RES, res)
        s.vcycleFromZero(F.F_CORR, F.F_RES)
        _same(download_valid(s, F.F_CORR, prob[1]), got, "the handle's own cycle")
    finally:
        s.undefine()


def test_refused_during_a_metric_update(oracle):
    s, case = _small(oracle)
    try:
        s.setComponents(2)
        op = case.ops[1]
        with s.metricUpdate():
            _raises(lambda: s.setCompOp(1, op.bc, op.values, ALPHA, BETA), "metric update")
            _raises(lambda: s.resetCompOp(1), "metric update")
        assert not s.getCompOp(1)[4]
    finally:
        s.undefine()
