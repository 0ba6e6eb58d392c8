"""Opt-in mixed precision of the level solve (somar_solver_set_precision / _get_precision): the leading MG depths run their
V-cycle in fp32 inside the fp64 defect-correction loop.  Not the reference's arithmetic, so these tests compare the mixed
solver with the same solver in fp64 (mode 0), not with the oracle: the fp32 correction must stay within a few fp32 ulps of
the fp64 one, full solves must reach the same fp64 tolerances in (about) the same number of cycles, and everything that
keeps mode 0's bits (K == 0, switching back, refreshes, determinism) must keep them exactly.

The kernels of the fp32 depths are the large-level ones (fused sweep, marching residual + restriction, folded prolongation);
SOMAR_FUSED_MIN_CELLS / SOMAR_MARCH_MIN_CELLS = 0 put them on levels small enough for a test, SOMAR_GRAPH_CELLS = 4096 keeps
the graph-replayed tail below them.  On the 64^3 grid of 32^3 boxes the depths are 64^3, 32^3, 16^3, ...: depths 0 and 1 run in
fp32 (K = 2), 16^3 = 4096 cells is a serial-order (and graph-replayed) depth that stays fp64."""
import numpy as np
import pytest

from tests.helpers import download_valid, make_problem, upload

pytestmark = pytest.mark.gpu

D, N = 1, 0
GRAPH_CELLS = 4096
K_64 = 2   # fp32 depths of the 64^3 cases with the library's default min_cells

# (name, n, box, periodic, bc types per side, bc values, alpha, beta[, metric variant, default "stretched"])
# The Cartesian cases have a uniform metric on every depth: with Dirichlet sides the fused sweep still streams the coefficient
# arrays (its uniform-metric kernels take no Dirichlet side), so their fp32 copies must exist there.
CASES = [
    ("neumann", (64, 64, 64), 32, (False, False, False), None, None, 0.0, 1.0),
    ("periodic", (64, 64, 64), 32, (True, True, True), None, None, 0.0, 1.0),
    ("dirichlet", (64, 64, 64), 32, (False, False, False), [D] * 6, [0.25, -0.5, 0.75, 0.1, -0.3, 0.6], 0.0, 1.0),
    ("helmholtz", (64, 64, 64), 32, (False, True, False), None, None, 1.0, -0.01),   # a backward-Euler step's operator
    ("cartesian-dirichlet", (64, 64, 64), 32, (False, False, False), [D] * 6, [0.25, -0.5, 0.75, 0.1, -0.3, 0.6], 0.0, 1.0,
     "cartesian"),
    ("cartesian-mixed-sides", (64, 64, 64), 32, (False, True, False), [D, N, N, N, N, D], [0.5, 0.0, 0.0, 0.0, 0.0, -0.25],
     0.0, 1.0, "cartesian"),
]
IDS = [c[0] for c in CASES]


@pytest.fixture(autouse=True)
def _large_level_kernels(monkeypatch):
    monkeypatch.setenv("SOMAR_FUSED_MIN_CELLS", "0")
    monkeypatch.setenv("SOMAR_MARCH_MIN_CELLS", "0")
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", str(GRAPH_CELLS))


def _problem(so, case, L=(1.0, 1.0, 1.0)):
    n, box, per = case[1], case[2], case[3]
    return make_problem(so, n, box, case[8] if len(case) > 8 else "stretched", per, L)


def _solver(so, case, eps=1e-10, L=(1.0, 1.0, 1.0), problem=None, imax=100):
    """2/2/2 LevelGSRB V-cycles, imax large enough for the stretched metric's slow contraction to reach 1e-10"""
    from somar_amd import AMRPressureSolver
    types, values, alpha, beta = case[4:8]
    dom, grids, dx, Jgup, Jinv = problem or _problem(so, case, L)
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=alpha, beta=beta, bc_type=types)
    if values is not None:
        s.setBCValues(values)
    _ortho(s, Jgup, Jinv)
    s.finalize()
    return dom, grids, Jinv, s


def _rhs(so, case, dom, grids, Jinv, seed=11):
    rhs = so.random_field(grids, seed, (0, 0, 0), dom.box)
    if case[4] is None and case[6] == 0.0:
        so.remove_weighted_mean(rhs, Jinv)   # Neumann / periodic Poisson: a compatible right-hand side
    return rhs


def _solve(s, grids, rhs):
    """solve from zero on the resident fields -> (phi per box, stats)"""
    from somar_amd import api as F
    upload(s, F.F_RHS, rhs)
    st = s.solveResident(zeroPhi=True)
    return download_valid(s, F.F_PHI, grids), st


def _assert_same_solve(a, b):
    (pa, sa), (pb, sb) = a, b
    assert (sa["iters"], sa["exitStatus"]) == (sb["iters"], sb["exitStatus"])
    assert sa["history"] == sb["history"]
    for x, y in zip(pa, pb):
        np.testing.assert_array_equal(x, y)


def _rel(a, b, remove_mean=False):
    a = np.concatenate([x.ravel() for x in a])
    b = np.concatenate([x.ravel() for x in b])
    if remove_mean:
        a, b = a - a.mean(), b - b.mean()
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- 1. depth split, K == 0 and mode 0 keep the fp64 bits ------------------------------------------------------------
def test_depth_split_and_fp64_bits_when_no_depth_is_fp32(oracle):
    so = oracle
    case = CASES[0]
    dom, grids, Jinv, s = _solver(so, case)
    try:
        assert s.precision() == (0, 0)
        rhs = _rhs(so, case, dom, grids, Jinv)
        ref = _solve(s, grids, rhs)
        c0, c1 = s.levelInfo(0)["cells"], s.levelInfo(1)["cells"]
        assert (c0, c1, s.levelInfo(2)["cells"]) == (64 ** 3, 32 ** 3, 16 ** 3)
        s.setPrecision(1)
        assert s.precision() == (1, K_64)
        s.setPrecision(1, c1 + 1)
        assert s.precision() == (1, 1)
        mixed = _solve(s, grids, rhs)
        assert mixed[1]["history"] != ref[1]["history"]   # the fp32 cycle does run
        s.setPrecision(1, c0 + 1)                          # larger than the level: nothing in fp32
        assert s.precision() == (1, 0)
        _assert_same_solve(_solve(s, grids, rhs), ref)
        s.setPrecision(1)
        _solve(s, grids, rhs)
        s.setPrecision(0)                                  # back to fp64 after a mixed solve
        assert s.precision() == (0, 0)
        _assert_same_solve(_solve(s, grids, rhs), ref)
    finally:
        s.undefine()


def test_precision_set_before_finalize(oracle):
    from somar_amd import AMRPressureSolver
    so = oracle
    case = CASES[0]
    dom, grids, dx, Jgup, Jinv = _problem(so, case)
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, 100, 1e-10, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
    try:
        s.setPrecision(1)
        assert s.precision() == (1, 0)
        for q in range(s.num_local_patches):
            _, _, gi = s.patch_box(q)
            s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                             np.asfortranarray(Jinv[gi].a[..., 0]))
        s.finalize()
        assert s.precision() == (1, K_64)
        _, _, _, t = _solver(so, case)
        t.setPrecision(1)
        rhs = _rhs(so, case, dom, grids, Jinv)
        _assert_same_solve(_solve(s, grids, rhs), _solve(t, grids, rhs))
        t.undefine()
    finally:
        s.undefine()


# ---- 2. one cycle from zero ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_cycle_from_zero_within_fp32_of_fp64(oracle, case):
    from somar_amd import api as F
    so = oracle
    dom, grids, Jinv, s = _solver(so, case)
    try:
        res = _rhs(so, case, dom, grids, Jinv, seed=5)
        upload(s, F.F_RES, res)
        s.vcycleFromZero(F.F_CORR, F.F_RES)
        c64 = download_valid(s, F.F_CORR, grids)
        s.setPrecision(1)
        assert s.precision() == (1, K_64)
        if len(case) > 8:
            assert all(s.metricUniform(d) is not None for d in range(K_64))   # the uniform-metric case is the one run
        s.vcycleFromZero(F.F_CORR, F.F_RES)
        c32 = download_valid(s, F.F_CORR, grids)
        err = _rel(c32, c64)
        print("%s: max|c32 - c64| / max|c64| = %.3e" % (case[0], err))
        assert 0.0 < err <= 1e-6, err
    finally:
        s.undefine()


# ---- 3. full solves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_full_solves_reach_fp64_tolerances(oracle, case):
    so = oracle
    null_space = case[4] is None and case[6] == 0.0
    for eps in (1e-10, 1e-6):
        dom, grids, Jinv, s = _solver(so, case, eps=eps)
        try:
            rhs = _rhs(so, case, dom, grids, Jinv)
            p64, s64 = _solve(s, grids, rhs)
            s.setPrecision(1)
            p32, s32 = _solve(s, grids, rhs)
            print("%s eps %g: iterations fp64 %d mixed %d, final / initial %.3e / %.3e" % (
                case[0], eps, s64["iters"], s32["iters"], s64["final_rnorm"] / s64["initial_rnorm"],
                s32["final_rnorm"] / s32["initial_rnorm"]))
            assert s32["exitStatus"] & 1 and s64["exitStatus"] & 1, (s32, s64)   # converged: the residual test ended it
            assert s32["final_rnorm"] <= eps * s32["initial_rnorm"]
            if eps == 1e-10:
                assert s32["iters"] <= s64["iters"] + 1
                err = _rel(p32, p64, remove_mean=null_space)
                print("   |phi32 - phi64| / |phi64| = %.3e" % err)
                assert err <= 1e-8, err
            else:
                assert s32["iters"] == s64["iters"]
        finally:
            s.undefine()


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph_cells", [GRAPH_CELLS, 0])
def test_mixed_solves_are_deterministic(oracle, monkeypatch, graph_cells):
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", str(graph_cells))
    so = oracle
    case = CASES[0]
    dom, grids, Jinv, s = _solver(so, case)
    try:
        s.setPrecision(1)
        assert s.precision() == (1, K_64)   # (16^3 is a serial-order depth: fp64 with or without graphs)
        rhs = _rhs(so, case, dom, grids, Jinv)
        first = _solve(s, grids, rhs)
        _assert_same_solve(_solve(s, grids, rhs), first)
    finally:
        s.undefine()


# ---- 5. interplay with the rest of the solver --------------------------------------------------------------------------
def _ortho(s, Jgup, Jinv):
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                         np.asfortranarray(Jinv[gi].a[..., 0]))


@pytest.mark.parametrize("variant2", ["stretched", "cartesian"])
def test_metric_refresh_equals_a_fresh_mixed_solver(oracle, variant2):
    so = oracle
    case = CASES[0]
    L2 = (0.8, 1.2, 0.9)
    dom, grids, dx, _, _ = _problem(so, case)
    # the second metric on the same grid spacing (a metric refresh changes the metric, not dx)
    _, _, _, Jgup2, Jinv2 = make_problem(so, case[1], case[2], variant2, case[3], L2)
    _, _, Jinv, a = _solver(so, case, problem=_problem(so, case))
    b = None
    try:
        a.setPrecision(1)
        rhs = _rhs(so, case, dom, grids, Jinv)
        _solve(a, grids, rhs)                       # graphs captured, fp32 copies of the first metric in use
        with a.metricUpdate():
            _ortho(a, Jgup2, Jinv2)
        _, _, _, b = _solver(so, case, problem=(dom, grids, dx, Jgup2, Jinv2))
        b.setPrecision(1)
        assert a.precision() == b.precision()
        rhs2 = _rhs(so, case, dom, grids, Jinv2, seed=12)
        _assert_same_solve(_solve(a, grids, rhs2), _solve(b, grids, rhs2))
    finally:
        a.undefine()
        if b is not None:
            b.undefine()


def test_set_alpha_beta_after_finalize_equals_a_fresh_mixed_solver(oracle):
    so = oracle
    case = CASES[3]
    dom, grids, Jinv, a = _solver(so, case)
    _, _, _, b = _solver(so, case)
    try:
        a.setPrecision(1)
        b.setPrecision(1)
        rhs = _rhs(so, case, dom, grids, Jinv)
        _solve(a, grids, rhs)
        a.setAlphaAndBeta(1.0, 0.4)
        b.setAlphaAndBeta(1.0, 0.4)
        _assert_same_solve(_solve(a, grids, rhs), _solve(b, grids, rhs))
    finally:
        a.undefine()
        b.undefine()


def test_cc_projection_divergence_within_the_fp64_bound(oracle):
    from somar_amd import api as F
    from tests.helpers import smooth_cc_velocity
    so = oracle
    case = CASES[0]
    ghost = (1, 1, 1)
    out = {}
    for mode in (0, 1):
        dom, grids, Jinv, s = _solver(so, case, eps=1e-8)
        try:
            s.setPrecision(mode)
            vel = smooth_cc_velocity(so, dom, grids, ghost)
            gvel = [vel[s.patch_box(q)[2]].a.copy(order="F") for q in range(s.num_local_patches)]
            for q in range(s.num_local_patches):
                s.uploadCCVel(q, gvel[q], ghost)
            s.divergenceCC(F.F_RHS, 1.0, True)
            div0 = max(float(np.max(np.abs(x))) for x in download_valid(s, F.F_RHS, grids))
            st = s.levelProjectCC(gvel, ghost, 0.5)
            for q in range(s.num_local_patches):
                s.uploadCCVel(q, gvel[q], ghost)
            s.divergenceCC(F.F_RHS, 1.0, True)
            div = max(float(np.max(np.abs(x))) for x in download_valid(s, F.F_RHS, grids))
            out[mode] = (st, div0, div)
        finally:
            s.undefine()
    (s64, d0, d64), (s32, _, d32) = out[0], out[1]
    print("cc projection: max|div| before %.3e, after fp64 %.3e (%d cycles), mixed %.3e (%d cycles)" % (
        d0, d64, s64["iters"], d32, s32["iters"]))
    assert s32["exitStatus"] & 1 and s32["final_rnorm"] <= 1e-8 * s32["initial_rnorm"]
    assert s32["iters"] <= s64["iters"] + 1
    # (the cell-centred projection is approximate: what is left is the fp64 run's own remainder, to the solve's tolerance)
    assert abs(d32 - d64) <= 1e-6 * d0, (d32, d64)


def test_backward_euler_heat_step_matches_fp64(oracle):
    from somar_amd import api as F
    so = oracle
    case = ("heat", (64, 64, 64), 32, (False, False, False), [D] * 6, [0.0] * 6, 1.0, 1e-2)
    res = {}
    for mode in (0, 1):
        dom, grids, Jinv, s = _solver(so, case, eps=1e-10)
        try:
            s.setPrecision(mode)
            assert s.precision()[1] >= (2 if mode else 0)
            upload(s, F.F_HEAT_OLD, so.random_field(grids, 3, (1, 1, 1), dom.box))
            upload(s, F.F_HEAT_SRC, so.random_field(grids, 4, (0, 0, 0), dom.box))
            st = s.heatStep(0, 0.2)
            res[mode] = (download_valid(s, F.F_PHI, grids), st)
        finally:
            s.undefine()
    err = _rel(res[1][0], res[0][0])
    print("heat step: |phi32 - phi64| / |phi64| = %.3e, cycles %d / %d, histories %s / %s" % (
        err, res[1][1]["iters"], res[0][1]["iters"], res[1][1]["history"][:3], res[0][1]["history"][:3]))
    assert res[1][1]["exitStatus"] & 1
    assert res[1][1]["history"] != res[0][1]["history"]   # the fp32 cycle did run
    assert err <= 1e-8, err


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def _raises(fn, *words):
    from somar_amd import SomarError
    with pytest.raises(SomarError) as e:
        fn()
    msg = str(e.value)
    for w in words:
        assert w in msg, msg


def _defined(so, relaxMode=1, numMG=1):
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 32, 32), 16, "stretched")
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, relaxMode, numMG, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
    return s, Jgup, Jinv


def test_refusals(oracle):
    so = oracle
    # relax modes other than LevelGSRB, W-cycles, F-cycles
    for kw, word in (({"relaxMode": 0}, "relax_mode"), ({"relaxMode": 3}, "relax_mode"), ({"numMG": 2}, "num_mg"),
                     ({"numMG": -1}, "num_mg")):
        s, _, _ = _defined(so, **kw)
        try:
            _raises(lambda: s.setPrecision(1), word)
            s.setPrecision(0)   # mode 0 is always accepted
        finally:
            s.undefine()
    # a non-diagonal metric: known at finalize (refused there) or after it
    s, Jgup, Jinv = _defined(so)
    try:
        s.setPrecision(1)
        for q in range(s.num_local_patches):
            _, _, gi = s.patch_box(q)
            jg = []
            for d in range(3):
                a = np.zeros(Jgup[gi][d].a.shape[:3] + (3,), order="F")
                a[..., d] = Jgup[gi][d].a[..., d]
                jg.append(a)
            s.setMetricFull(q, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
        _raises(s.finalize, "non-diagonal")
        s.setPrecision(0)
        s.finalize()
        _raises(lambda: s.setPrecision(1), "non-diagonal")
    finally:
        s.undefine()
    # an open metric update; an unknown mode
    s, Jgup, Jinv = _defined(so)
    try:
        _ortho(s, Jgup, Jinv)
        s.finalize()
        _raises(lambda: s.setPrecision(3), "mode")
        with s.metricUpdate():
            _raises(lambda: s.setPrecision(1), "metric update")
            _raises(lambda: s.setPrecision(0), "metric update")
        s.setPrecision(1)
    finally:
        s.undefine()
    # a level of an AMR hierarchy with two levels
    from somar_amd import AMRPressureSolver
    h = AMRPressureSolver()
    h.defineAMR((0, 0, 0), (15, 15, 15), (False, False, False), (1 / 16.0,) * 3, [(2, 2, 2)],
                [[((0, 0, 0), (15, 15, 15))], [((8, 8, 8), (23, 23, 23))]])
    try:
        for lv in h.levels:
            _raises(lambda: lv.setPrecision(1), "AMR")
    finally:
        h.undefine()
    # the handles of a leptic solver
    from somar_amd.api import LevelLepticSolver
    lep = LevelLepticSolver()
    lep.define((0, 0, 0), (15, 15, 7), (False, False, False), (1 / 16.0, 1 / 16.0, 1 / 16.0), [((0, 0, 0), (15, 15, 7))])
    try:
        _raises(lambda: lep.level.setPrecision(1), "leptic")
    finally:
        lep.undefine()
