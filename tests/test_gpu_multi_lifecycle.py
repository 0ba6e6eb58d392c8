"""The life cycle of a handle that carries several components (somar_solver_set_components), beyond one call on a fresh handle
(tests/test_gpu_multi.py, whose helpers and layouts this file uses): everything is compared bit for bit with the single-field
calls of a one-component handle, which is the specification of the multi calls.

  1. A metric refresh of a three-component handle (PressureSolver::refresh_metric decides the batched depths again): the
     components' fields outlive it, K follows the metric (a uniform metric batches nothing), the solves equal those of a fresh
     handle, and going there and back leaves the device memory where it was.
  2. Component 0 is the handle's own fields: the ordinary single-field calls on a three-component handle behave as on a
     one-component handle and leave the other components alone.
  3. Heat steps that keep phi as the initial guess (zeroPhi = False), two steps in a row; the TGA scheme saves and restores the
     guess around its first solve, per component.
  4. Position-dependent Dirichlet values on a layout with Dirichlet and Neumann sides mixed.
  5. The device memory of the heat fields a component allocated on the way is released with the component."""
import numpy as np
import pytest

from tests.helpers import download_valid, upload
from tests.test_gpu_mixed_kernels import problem, set_env
from tests.test_gpu_multi import (ALPHA, BC_VALUES, BETA, EPS, IMAX, LAYOUTS, NORM_THRESH, STAT_KEYS, WIDE_BOX, WIDE_N, D, _case,
                                  _down, _reaches, _same, _solve_both_ways, _solve_rhs, _up)

pytestmark = pytest.mark.gpu

FIELDS = ("F_PHI", "F_RHS", "F_RES", "F_CORR")
L2 = (0.7, 1.3, 0.45)               # another period of the stretched map, as tests/test_gpu_metric_refresh.py takes one
UNIFORM = (2.0, 0.5, 1.5, 0.25)     # Jg^xx, Jg^yy, Jg^zz, Jinv
HEAT = _case("wide-dirichlet-heat", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), [D] * 6, None, 3, alpha=1.0, beta=1.0)
DT = 0.01


@pytest.fixture(autouse=True)
def _large_level_kernels(monkeypatch):
    set_env(monkeypatch.setenv)
    for k in ("SOMAR_NARROW_7PT", "SOMAR_NO_NARROW_TILES", "SOMAR_FUSED_ROWS", "SOMAR_ORDERED_REDUCE_MAX"):
        monkeypatch.delenv(k, raising=False)


def _ortho(s, metric):
    Jgup, Jinv = metric
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)], np.asfortranarray(Jinv[gi].a[..., 0]))


def _handle(case, prob, metric, eps=EPS, imax=IMAX, norm_thresh=NORM_THRESH, bc_values=None):
    """a finalized handle with 2/2/2 sweeps; metric: (Jgup, Jinv) of a diagonal metric, or the four constants of a uniform one"""
    from somar_amd import AMRPressureSolver
    dom, grids, dx = prob[0], prob[1], prob[2]
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh if norm_thresh is None else norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=case.alpha, beta=case.beta,
             bc_type=case.bc)
    if bc_values is not None:
        s.setBCValues(bc_values)
    _set_metric(s, metric)
    s.finalize()
    return s


def _set_metric(s, metric):
    if len(metric) == 4:
        s.setMetricUniform(*metric)
    else:
        _ortho(s, metric)


def _three_solves(case, prob, metric, rhs):
    """three solveResident calls from zero on a fresh one-component handle: (phi, stats, history) per right-hand side"""
    from somar_amd import api as F
    s = _handle(case, prob, metric)
    try:
        out = []
        for r in rhs:
            upload(s, F.F_RHS, r)
            st = s.solveResident(zeroPhi=True)
            out.append((download_valid(s, F.F_PHI, prob[1]), dict(st), [float(v) for v in F.last_history()]))
        assert s.getComponents() == (1, 0, 0)
        return out
    finally:
        s.undefine()


def _assert_multi_is(s, stats, seq, grids, what):
    from somar_amd import api as F
    for c, (phi, st, hist) in enumerate(seq):
        _same(_down(s, c, F.F_PHI, grids), phi, "%s: phi of component %d" % (what, c))
        for k in STAT_KEYS:
            assert stats[c][k] == st[k], (what, c, k, stats[c][k], st[k])
        assert s.compHistory(c) == hist, (what, c)
        assert st["iters"] > 0 or c == 1, (what, c)   # (the right-hand side identically zero is component 1's)


# ---- 1. metric refresh ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [True, False])
def test_metric_refresh_with_three_components(oracle, monkeypatch, graphs):
    """M1 -> M2 -> uniform -> M1 on one three-component handle.  The right-hand sides are those of the solve tests (smooth, zero,
    random), the smooth one first: component 0 runs cycles, so no reported count depends on what the handle did before."""
    from somar_amd import api as F
    so, case = oracle, LAYOUTS["wide-equal"]
    monkeypatch.setenv("SOMAR_NARROW_7PT", case.narrow)
    if not graphs:
        monkeypatch.setenv("SOMAR_GRAPH_CELLS", "0")   # (K stays 3: the 16 x 12 x 12 depth sums in serial order)
    prob = problem(so, case)
    dom, grids, dx = prob[0], prob[1], prob[2]
    M1 = (prob[3], prob[4])
    M2 = so.make_diagonal_metric(grids, dx, L2, 3, "stretched", domain=dom)
    rhs = _solve_rhs(so, case, prob)
    base = F.device_bytes_live()
    a = _handle(case, prob, M1)
    try:
        # The first refresh of a handle's life builds the refresh's own work items (PressureSolver::refresh_metric: one small
        # table per coarse depth, 288 bytes here, kept from then on).  An idempotent refresh of the one-component handle puts
        # them there before anything is measured, so the figures below differ by what the components hold and by nothing else.
        with a.metricUpdate():
            _ortho(a, M1)
        a.setComponents(3)
        held = F.device_bytes_live()
        assert held > base
        for c in range(3):
            _up(a, c, F.F_RHS, rhs[c])
        a.solveMulti(zeroPhi=True)   # graphs exist now (where they are on)
        launches = _reaches(a, 3, case.K, 0)
        before = {(c, f): _down(a, c, getattr(F, f), grids) for c in range(3) for f in ("F_RHS", "F_PHI")}
        assert all(float(np.max(np.abs(before[(c, "F_PHI")][0]))) > 0.0 for c in (0, 2))

        # -- to M2: the fields stay, the batched depths are decided again, the solves are a fresh M2 handle's
        with a.metricUpdate():
            _ortho(a, M2)
        assert a.getComponents()[:2] == (3, 3)
        for (c, f), want in before.items():
            _same(_down(a, c, getattr(F, f), grids), want, "%s of component %d across the refresh" % (f, c))
        stats = a.solveMulti(zeroPhi=True)
        launches = _reaches(a, 3, case.K, launches)
        seq2 = _three_solves(case, prob, M2, rhs)
        _assert_multi_is(a, stats, seq2, grids, "refreshed to M2")

        # -- to a uniform metric: nothing is batched (no coefficient stream to share), no N-field launch is issued
        with a.metricUpdate():
            a.setMetricUniform(*UNIFORM)
        assert a.metricUniform(0) == UNIFORM
        assert a.getComponents() == (3, 0, launches)
        stats = a.solveMulti(zeroPhi=True)
        assert a.getComponents() == (3, 0, launches)
        _assert_multi_is(a, stats, _three_solves(case, prob, UNIFORM, rhs), grids, "refreshed to a uniform metric")

        # -- back to M1: batched again, a fresh M1 handle's solves, and the memory of the first set_components(3)
        with a.metricUpdate():
            _ortho(a, M1)
        assert a.metricUniform(0) is None
        assert a.getComponents()[:2] == (3, 3)
        stats = a.solveMulti(zeroPhi=True)
        _reaches(a, 3, case.K, launches)
        seq1 = _three_solves(case, prob, M1, rhs)
        _assert_multi_is(a, stats, seq1, grids, "refreshed back to M1")
        assert any(not np.array_equal(x, y) for x, y in zip(seq1[2][0], seq2[2][0]))   # (the two metrics do differ)
        now = F.device_bytes_live()
        print("device bytes: base %d, after the first set_components(3) %d, after M1 -> M2 -> uniform -> M1 %d" % (base, held, now))
        assert now == held
    finally:
        a.undefine()
    assert F.device_bytes_live() == base


# ---- 2. component 0 is the handle's own fields ----------------------------------------------------------------------------------
def test_component_0_is_the_handles_own_fields(oracle, monkeypatch):
    """The handles are created with the coefficients of a heat operator (aCoef = bCoef = 1, as the heat tests create theirs: a
    heat step SCALES the coefficients the handle was created with, and -0.01 scaled by -dt / 2 is an indefinite operator) and
    then set to this file's Helmholtz operator, alpha = 1 and beta = -0.01, for the solves and the cycle."""
    from somar_amd import api as F
    so = oracle
    case = _case("wide-equal-heat", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), None, "0", 3, alpha=1.0, beta=1.0)
    monkeypatch.setenv("SOMAR_NARROW_7PT", case.narrow)
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    M1 = (prob[3], prob[4])
    rhs = _solve_rhs(so, case, prob)
    new_rhs = so.random_field(grids, 101, (0, 0, 0), dom.box)
    new_res = so.random_field(grids, 102, (0, 0, 0), dom.box)
    old = so.random_field(grids, 103, (1, 1, 1), dom.box)
    src = so.random_field(grids, 104, (0, 0, 0), dom.box)

    def calls(s):
        """the three single-field calls; yields after each what it left"""
        upload(s, F.F_RHS, new_rhs)
        st = s.solveResident(zeroPhi=True)
        yield "solveResident", download_valid(s, F.F_PHI, grids), dict(st), [float(v) for v in F.last_history()]
        upload(s, F.F_RES, new_res)
        s.vcycleFromZero(F.F_CORR, F.F_RES)
        yield "vcycleFromZero", download_valid(s, F.F_CORR, grids), None, None
        upload(s, F.F_HEAT_OLD, old)
        upload(s, F.F_HEAT_SRC, src)
        st = s.heatStep(1, DT)
        yield "heatStep", download_valid(s, F.F_PHI, grids), dict(st), [float(v) for v in F.last_history()]

    one = _handle(case, prob, M1, eps=1e-8, imax=20, norm_thresh=None)
    try:
        one.setAlphaAndBeta(ALPHA, BETA)
        want = list(calls(one))
    finally:
        one.undefine()
    s = _handle(case, prob, M1, eps=1e-8, imax=20, norm_thresh=None)
    try:
        s.setAlphaAndBeta(ALPHA, BETA)
        s.setComponents(3)
        for c in range(3):
            _up(s, c, F.F_RHS, rhs[2 - c])   # (the random right-hand side first: every component's fields are far from zero)
        s.solveMulti(zeroPhi=True)
        launches = _reaches(s, 3, case.K, 0)
        others = {(c, f): _down(s, c, getattr(F, f), grids) for c in (1, 2) for f in FIELDS}
        assert all(float(np.max(np.abs(others[(2, f)][0]))) > 0.0 for f in FIELDS)
        for (what, field, st, hist), (_, wfield, wst, whist) in zip(calls(s), want):
            _same(field, wfield, "%s on a three-component handle against a one-component handle" % what)
            if wst is not None:
                assert wst["iters"] > 0
                for k in STAT_KEYS:
                    assert st[k] == wst[k], (what, k, st[k], wst[k])
                assert hist == whist, what
            for (c, f), kept in others.items():
                _same(_down(s, c, getattr(F, f), grids), kept, "%s of component %d after %s" % (f, c, what))
            for f in FIELDS:
                _same(_down(s, 0, getattr(F, f), grids), download_valid(s, getattr(F, f), grids),
                      "component 0's %s after %s" % (f, what))
            assert s.getComponents() == (3, case.K, launches), what   # single-field calls issue no N-field launch
    finally:
        s.undefine()


# ---- 3. heat steps that keep phi ------------------------------------------------------------------------------------------------
def _up_valid(s, comp, field, arrays):
    """valid-region arrays (as _down returns them) into a component's field; comp None: through the single-field call"""
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        a = np.asfortranarray(arrays[gi])
        if comp is None:
            s.upload(field, q, a, (0, 0, 0))
        else:
            s.uploadComp(comp, field, q, a, (0, 0, 0))


@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_heat_steps_that_keep_phi(oracle, scheme):
    """zeroPhi = False: F_PHI is the initial guess of the step's solve(s) -- of BOTH solves of the TGA scheme, which keeps it in
    its third heat field while phi carries the first solve's result.  Then a second step from the first one's result.  The
    single-field path shares one handle among the three, so it uploads each component's phi before its step; on the
    multi-component handle every component's phi simply stays where the first step left it."""
    from somar_amd import api as F
    so, case = oracle, HEAT
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    M1 = (prob[3], prob[4])
    old = [so.random_field(grids, 61 + c, (1, 1, 1), dom.box) for c in range(3)]
    src = [so.random_field(grids, 71 + c, (0, 0, 0), dom.box) for c in range(3)]
    guess = [so.random_field(grids, 51 + c, (1, 1, 1), dom.box) for c in range(3)]

    def stats_equal(got, want, what):
        assert want["iters"] > 0, what
        for k in STAT_KEYS:
            assert got[k] == want[k], (what, k, got[k], want[k])

    s = _handle(case, prob, M1, eps=1e-8, imax=20, norm_thresh=None, bc_values=BC_VALUES)
    try:
        seq1, seq2 = [], []
        for c in range(3):
            upload(s, F.F_HEAT_OLD, old[c])
            upload(s, F.F_HEAT_SRC, src[c])
            upload(s, F.F_PHI, guess[c])
            st = s.heatStep(scheme, DT, zeroPhi=False)
            seq1.append((download_valid(s, F.F_PHI, grids), dict(st)))
        for c in range(3):
            _up_valid(s, None, F.F_HEAT_OLD, seq1[c][0])
            upload(s, F.F_HEAT_SRC, src[c])
            _up_valid(s, None, F.F_PHI, seq1[c][0])
            st = s.heatStep(scheme, DT, zeroPhi=False)
            seq2.append((download_valid(s, F.F_PHI, grids), dict(st)))
        # the guess is used: from zero the same step ends elsewhere
        upload(s, F.F_HEAT_OLD, old[0])
        upload(s, F.F_HEAT_SRC, src[0])
        s.heatStep(scheme, DT, zeroPhi=True)
        assert any(not np.array_equal(x, y) for x, y in zip(download_valid(s, F.F_PHI, grids), seq1[0][0]))

        s.setComponents(3)
        for c in range(3):
            _up(s, c, F.F_HEAT_OLD, old[c])
            _up(s, c, F.F_HEAT_SRC, src[c])
            _up(s, c, F.F_PHI, guess[c])
        stats = s.heatStepMulti(scheme, DT, zeroPhi=False)
        launches = _reaches(s, 3, case.K, 0)
        got1 = [_down(s, c, F.F_PHI, grids) for c in range(3)]
        for c in range(3):
            _same(got1[c], seq1[c][0], "scheme %d, first step, phi of component %d" % (scheme, c))
            stats_equal(stats[c], seq1[c][1], (scheme, "first step", c))
        for c in range(3):
            _up_valid(s, c, F.F_HEAT_OLD, got1[c])
        stats = s.heatStepMulti(scheme, DT, zeroPhi=False)
        _reaches(s, 3, case.K, launches)
        for c in range(3):
            _same(_down(s, c, F.F_PHI, grids), seq2[c][0], "scheme %d, second step, phi of component %d" % (scheme, c))
            stats_equal(stats[c], seq2[c][1], (scheme, "second step", c))
            assert any(not np.array_equal(x, y) for x, y in zip(seq1[c][0], seq2[c][0]))
    finally:
        s.undefine()


# ---- 4. position-dependent Dirichlet values -------------------------------------------------------------------------------------
def _smooth_plane(dom_box, dx, d, side):
    """a smooth plane that is nowhere constant, over the whole side's faces (the layout of tests/diri_face.py)"""
    from tests.diri_face import face_positions
    p0, p1 = face_positions(dom_box, dx, d, side)
    return np.asfortranarray(0.3 - 0.2 * d + 0.25 * np.sin(2.0 * np.pi * p0 + 0.3 + side) * np.cos(np.pi * p1 + 0.1 * (d + 1)))


def test_solve_multi_with_face_values_on_mixed_sides(oracle):
    """setBCFaceValues on two of the three Dirichlet sides of wide-mixed-sides (x low, y high; z low keeps its constant): the
    N-field residual of depth 0 takes its inhomogeneous ghosts from apply_diri, field by field"""
    so, case = oracle, LAYOUTS["wide-mixed-sides"]
    assert [case.bc[0], case.bc[3], case.bc[4]] == [D, D, D]
    prob = problem(so, case)
    dom, dx = prob[0], prob[2]
    planes = {(0, 0): _smooth_plane(dom.box, dx, 0, 0), (1, 1): _smooth_plane(dom.box, dx, 1, 1)}
    assert all(float(np.ptp(p)) > 0.1 for p in planes.values())
    phi = {}
    for homogeneous in (False, True):
        phi[homogeneous] = []
        _solve_both_ways(so, case, True, homogeneous, bc_values=BC_VALUES, face_values=planes, phi_out=phi[homogeneous])
    # the values were used: with them every component ends elsewhere than without
    for c in range(3):
        assert any(not np.array_equal(x, y) for x, y in zip(phi[False][c], phi[True][c])), c
    # ... and it was the planes, not only the constants
    flat = []
    _solve_both_ways(so, case, True, False, bc_values=BC_VALUES, phi_out=flat)
    for c in range(3):
        assert any(not np.array_equal(x, y) for x, y in zip(phi[False][c], flat[c])), c


# ---- 5. memory after heat steps -------------------------------------------------------------------------------------------------
def test_heat_fields_of_components_are_released(oracle):
    from somar_amd import api as F
    so, case = oracle, HEAT
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    M1 = (prob[3], prob[4])
    old = [so.random_field(grids, 61 + c, (1, 1, 1), dom.box) for c in range(3)]
    src = [so.random_field(grids, 71 + c, (0, 0, 0), dom.box) for c in range(3)]
    base = F.device_bytes_live()
    one = _handle(case, prob, M1, eps=1e-8, imax=20, norm_thresh=None, bc_values=BC_VALUES)
    try:
        upload(one, F.F_HEAT_OLD, old[0])
        upload(one, F.F_HEAT_SRC, src[0])
        assert one.heatStep(2, DT)["iters"] > 0
        want = F.device_bytes_live() - base
    finally:
        one.undefine()
    assert F.device_bytes_live() == base and want > 0
    s = _handle(case, prob, M1, eps=1e-8, imax=20, norm_thresh=None, bc_values=BC_VALUES)
    try:
        s.setComponents(3)
        for c in range(3):
            _up(s, c, F.F_HEAT_OLD, old[c])
            _up(s, c, F.F_HEAT_SRC, src[c])
        stats = s.heatStepMulti(2, DT)
        _reaches(s, 3, case.K, 0)
        assert all(st["iters"] > 0 for st in stats)
        three = F.device_bytes_live() - base
        elems = s.levelInfo(0)["field_elems"]
        assert three - want >= 2 * 8 * 8 * elems   # two more components: five fields and three heat fields each, at least
        s.setComponents(1)
        assert s.getComponents()[:2] == (1, 0)
        print("device bytes above the base: one component after heatStep(2) %d, three after heatStepMulti(2) %d" % (want, three))
        assert F.device_bytes_live() - base == want
    finally:
        s.undefine()
    assert F.device_bytes_live() == base
