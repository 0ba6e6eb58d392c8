"""The fp32 instantiations of the cycle kernels (somar_solver_set_precision mode 1) against the ORACLE's fp64 one_cycle, per
box, at the layouts where the float code differs from the double one: wide class-0 tiles (124 columns, all 64 lanes), the
narrow decompositions of wide boxes (128 -> 124 + 4, 64 -> 60 + 4), equal-column tiling, ragged multi-box layouts with seams
in x and y and periodic seams, semicoarsening ratios, Dirichlet sides, the uniform-metric kernels, a Helmholtz operator, and
the 8-row kernel family (SOMAR_FUSED_ROWS=8, a solver's own choice: run between two 16-row solvers).  Also: scale equivariance of fp64 and mixed
solves, rhs * 2^k for k from -110 to +115.

Every case first proves it reaches its target: the number K of fp32 depths, the box widths and MG ratios of those depths, and
the tile columns the marching kernels get there (march_columns restates the rule).  A case that silently stopped reaching
its target fails instead of passing vacuously.  Then one V-cycle from zero twice: K = 1 with 1/1 sweeps (one fused sweep
from zero, one residual + restriction, one folded prolongation sweep in fp32), and the full K with 2/2/2 sweeps.  The bound
is per box, max|c32 - c_oracle| / max|c_oracle| <= 1e-6 (about 17 fp32 unit roundoffs), so a bug confined to one small box
or to a 4-column remainder cannot hide under a global maximum.  STRETCHED_POISSON_BOUND documents the one exception.

Odd box widths never reach an fp32 depth: a depth with a coarser one below it has every box width a multiple of 4
(coarsenable() with MappedAMRPoissonOp's S_MAX_COARSE = 4), so the `n0 & 1` fall-back of build_march_tiles only runs on the
bottom level.  Equal columns are reached instead through a stretched metric (no narrow classes unless SOMAR_NARROW_7PT = 1)
and through SOMAR_NARROW_7PT = 0."""
import math

import numpy as np
import pytest

from tests.helpers import download_valid, march_columns, upload

pytestmark = pytest.mark.gpu

D, N = 1, 0
GRAPH_CELLS = 4096
BOUND = 1e-6
# The Poisson operator (null space, zero-average cycle) on the stretched metric with ONE sweep per side (K = 1, 1/1) measures
# 1.01e-6 on the 128-wide box, 1.29e-6 on one box of the ragged layout (0.77e-6 - 1.0e-6 on the other three).  The excess is
# arithmetic, not layout: narrow (124 + 4, 60 + 4) and equal columns give the same numbers to every printed digit, so do the
# ragged layout's two tilings, and the Cartesian metric (2.2e-7), Helmholtz (2.2e-7) and semicoarsened (3.2e-7) cases stay
# well inside 1e-6.  The likely cause (not measured): after one sweep from zero the red residuals vanish in exact
# arithmetic, so the fp32 residual + restriction is mostly cancellation of stretched-coefficient terms, whose rounding the
# fp64 coarse correction then carries over the whole box.  2e-6 keeps a factor of 15 below what a 1.001 error in one lane
# class's update gives (3.1e-5).  It applies to that cycle alone: the 2/2/2 cycle of the same cases measures 3.9e-7 and
# 4.6e-7 and is held to 1e-6.
STRETCHED_POISSON_BOUND = 2e-6


def test_march_columns_restatement():
    """the decompositions the comments of march_plan.h name"""
    assert march_columns(128, True) == [(124, 0), (4, 4)]
    assert march_columns(64, True) == [(60, 1), (4, 4)]
    assert march_columns(512, True) == [(104, 0)] * 5   # 4 x 124 + 4 x 4 costs 5 workgroup-marches > 0.85 x 5
    assert march_columns(132, True) == [(124, 0), (4, 4), (4, 4)]
    assert march_columns(32, True) == [(32, 1)]
    assert march_columns(128, False) == [(64, 0)] * 2
    assert march_columns(512, False) == [(104, 0)] * 5
    assert march_columns(45, True) == [(46, 0)]


def _ragged(n, xs, ys):
    """boxes of a (n) domain: x cut at xs, and each x slab cut in y at its own ys[slab]; z whole"""
    out = []
    for a, (x0, x1) in enumerate(zip(xs[:-1], xs[1:])):
        for y0, y1 in zip(ys[a][:-1], ys[a][1:]):
            out.append(((x0, y0, 0), (x1 - 1, y1 - 1, n[2] - 1)))
    return out


class Case:
    """a layout and what its fp32 depths must be.  cols[d][w]: the marching tables' columns of a box w cells wide at fp32
    depth d (the residual + restriction table, and the fused sweep's with 16-row kernels)"""

    def __init__(self, name, n, boxes, variant, periodic, L, bc, alpha, beta, narrow, K, widths, ratios, cols, bound=BOUND):
        self.name, self.n, self.boxes, self.variant, self.periodic, self.L = name, n, boxes, variant, periodic, L
        self.bc, self.alpha, self.beta, self.narrow = bc, alpha, beta, narrow
        self.K, self.widths, self.ratios, self.cols, self.bound = K, widths, ratios, cols, bound

    @property
    def null_space(self):
        return self.bc is None and self.alpha == 0.0


WIDE_N, WIDE_BOX = (128, 48, 48), 128   # 294912 cells; depths 128x48x48, 64x48x48, 32x24x24 in fp32, 16x12x12 graph-replayed
WIDE_RATIOS = [(2, 1, 1), (2, 2, 2), (2, 2, 2)]
NARROW_COLS = {0: {128: [(124, 0), (4, 4)]}, 1: {64: [(60, 1), (4, 4)]}, 2: {32: [(32, 1)]}}
EQUAL_COLS = {0: {128: [(64, 0), (64, 0)]}, 1: {64: [(64, 0)]}, 2: {32: [(32, 0)]}}
RAGGED_N = (80, 64, 32)
RAGGED_BOXES = _ragged(RAGGED_N, [0, 48, 80], [[0, 48, 64], [0, 16, 64]])

CASES = [
    Case("wide-stretched-narrow", WIDE_N, WIDE_BOX, "stretched", (False,) * 3, (1.0, 1.0, 1.0), None, 0.0, 1.0, "1",
         3, [[128], [64], [32]], WIDE_RATIOS, NARROW_COLS, STRETCHED_POISSON_BOUND),
    Case("wide-stretched-equal", WIDE_N, WIDE_BOX, "stretched", (False,) * 3, (1.0, 1.0, 1.0), None, 0.0, 1.0, "0",
         3, [[128], [64], [32]], WIDE_RATIOS, EQUAL_COLS, STRETCHED_POISSON_BOUND),
    # the uniform-metric narrow kernels (no coefficient arrays), with the zero-average mean removal (sweep modes 2 and 4)
    Case("wide-cartesian", WIDE_N, WIDE_BOX, "cartesian", (False,) * 3, (1.0, 1.0, 1.0), None, 0.0, 1.0, None,
         3, [[128], [64], [32]], WIDE_RATIOS, NARROW_COLS),
    # DIRI + NARROW: the uniform-metric tables, but the sweep streams the fp32 metric copies
    Case("wide-cartesian-dirichlet", WIDE_N, WIDE_BOX, "cartesian", (False,) * 3, (1.0, 1.0, 1.0), [D] * 6, 0.0, 1.0, None,
         3, [[128], [64], [32]], WIDE_RATIOS, NARROW_COLS),
    # four boxes, seams in x and (at different heights) in y, periodic in x and y; stretched: equal columns
    Case("ragged-periodic", RAGGED_N, RAGGED_BOXES, "stretched", (True, True, False), (1.25, 1.0, 0.5), None, 0.0, 1.0,
         None, 2, [[32, 32, 48, 48], [16, 16, 24, 24]], [(2, 2, 2)] * 2,
         {0: {48: [(48, 0)], 32: [(32, 0)]}, 1: {24: [(24, 0)], 16: [(16, 0)]}}, STRETCHED_POISSON_BOUND),
    # the same boxes with every table in narrow classes: 24 -> class 1, 16 -> equal (four class-4 columns cost 1.0 > 0.85)
    Case("ragged-periodic-narrow", RAGGED_N, RAGGED_BOXES, "stretched", (True, True, False), (1.25, 1.0, 0.5), None, 0.0,
         1.0, "1", 2, [[32, 32, 48, 48], [16, 16, 24, 24]], [(2, 2, 2)] * 2,
         {0: {48: [(48, 1)], 32: [(32, 1)]}, 1: {24: [(24, 1)], 16: [(16, 0)]}}, STRETCHED_POISSON_BOUND),
    # semicoarsening: depth 0 restricts and folds its prolongation with ratio (1, 2, 2)
    Case("anisotropic", (64, 32, 16), 32, "stretched", (False, True, False), (4.0, 1.0, 0.5), None, 0.0, 1.0, None,
         2, [[32, 32], [32, 32]], [(1, 2, 2), (2, 2, 2)], {0: {32: [(32, 0)]}, 1: {32: [(32, 0)]}}),
    Case("wide-helmholtz", WIDE_N, WIDE_BOX, "stretched", (False,) * 3, (1.0, 1.0, 1.0), None, 1.0, -0.01, "1",
         3, [[128], [64], [32]], WIDE_RATIOS, NARROW_COLS),
]
IDS = [c.name for c in CASES]
SOLVE_CASES = ["wide-stretched-narrow", "wide-stretched-equal", "wide-cartesian", "wide-cartesian-dirichlet",
               "ragged-periodic", "ragged-periodic-narrow"]


def set_env(setenv):
    setenv("SOMAR_FUSED_MIN_CELLS", "0")
    setenv("SOMAR_MARCH_MIN_CELLS", "0")
    setenv("SOMAR_GRAPH_CELLS", str(GRAPH_CELLS))


@pytest.fixture(autouse=True)
def _large_level_kernels(monkeypatch):
    set_env(monkeypatch.setenv)
    monkeypatch.delenv("SOMAR_NARROW_7PT", raising=False)


def problem(so, case):
    n = case.n
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), case.periodic)
    if isinstance(case.boxes, list):
        grids = [so.Box(lo, hi) for lo, hi in case.boxes]
    else:
        grids = so.split_domain(dom.box, case.boxes)
    dx = tuple(case.L[d] / n[d] for d in range(3))
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, case.L, 3, case.variant, domain=dom)
    return dom, grids, dx, Jgup, Jinv


def _bc_holder(so, case):
    if case.bc is None:
        return so.BCHolder()
    return so.BCHolder([[case.bc[2 * d], case.bc[2 * d + 1]] for d in range(3)], None)


def oracle_cycle(so, case, prob, res, sweeps):
    """the oracle's fp64 MultiGrid::one_cycle from zero (homogeneous), a fresh bottom solver as in the GPU handle"""
    dom, grids, dx, Jgup, Jinv = prob
    fac = so.Factory(dom, grids, dx, _bc_holder(so, case), Jgup, Jinv, alpha=case.alpha, beta=case.beta)
    amr = so.AMRMultiGrid(fac, so.BiCGStab())
    amr.pre = amr.post = amr.bottom = sweeps
    amr.mg.pre = amr.mg.post = amr.mg.bottom = sweeps
    corr = so.LevelData(grids, 1, (1, 1, 1))
    amr.mg.init(corr, res)
    amr.mg.bottomSolver = so.BiCGStab()
    amr.mg.bottomSolver.define(amr.mg.ops[-1], True)
    amr.mg.one_cycle(corr, res)
    return [f.view(g)[..., 0] for g, f in zip(corr.grids, corr.fabs)], [tuple(r) for r in amr.mg.mgRefRatios]


def gpu_solver(case, prob, sweeps=2, eps=1e-10, imax=100, norm_thresh=None):
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv = prob
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, sweeps, sweeps, sweeps, p.precond_mode, 1, p.num_mg,
                         p.hang, p.norm_thresh if norm_thresh is None else norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=case.alpha, beta=case.beta,
             bc_type=case.bc)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                         np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return s


def residual_field(so, case, prob, seed=5):
    dom, grids, dx, Jgup, Jinv = prob
    res = so.random_field(grids, seed, (0, 0, 0), dom.box)
    if case.null_space:
        so.remove_weighted_mean(res, Jinv)   # a compatible right-hand side
    return res


def assert_reaches_target(s, case, K, oracle_ratios):
    """precision, fp32 box widths, MG ratios and tile columns of the case's fp32 depths"""
    assert s.precision() == (1, K), (s.precision(), K)
    assert s.mgRefRatios() == oracle_ratios
    assert s.mgRefRatios()[:case.K] == case.ratios, s.mgRefRatios()
    for d in range(K):
        widths = sorted(s.patch_box(q, d)[1][0] - s.patch_box(q, d)[0][0] + 1 for q in range(s.num_local_patches))
        assert widths == case.widths[d], (d, widths)
        # finalize's choice of narrow classes (solver.cpp: SOMAR_NARROW_7PT forces it, else where the metric is uniform)
        uniform = s.metricUniform(d) is not None
        assert uniform == (case.variant == "cartesian"), d
        narrow = case.narrow == "1" if case.narrow is not None else uniform
        for w in set(widths):
            # the residual + restriction table; the fused sweep's is the same with 16-row kernels (8 rows: equal columns)
            assert march_columns(w, narrow) == case.cols[d][w], (d, w, march_columns(w, narrow))


def per_box_errors(got, ref):
    return [float(np.max(np.abs(g - r)) / np.max(np.abs(r))) for g, r in zip(got, ref)]


def check_cycles(so, case, rows=16):
    """the two V-cycles from zero of the module docstring against the oracle; returns the measured per-box errors.  rows:
    the region rows of the fused sweep its solvers must hold (SOMAR_FUSED_ROWS as the caller set it)"""
    from somar_amd import api as F
    prob = problem(so, case)
    grids = prob[1]
    res = residual_field(so, case, prob)
    measured = {}
    for label, sweeps, full_K, bound in (("K=1 1/1", 1, False, case.bound), ("K=%d 2/2/2" % case.K, 2, True, BOUND)):
        ref, oratios = oracle_cycle(so, case, prob, res, sweeps)
        s = gpu_solver(case, prob, sweeps=sweeps)
        try:
            assert s.tuning("FUSED_ROWS") == rows
            if full_K:
                s.setPrecision(1)
            else:
                s.setPrecision(1, s.levelInfo(0)["cells"])   # depth 0 alone reaches min_cells
            assert_reaches_target(s, case, case.K if full_K else 1, oratios)
            upload(s, F.F_RES, res)
            s.vcycleFromZero(F.F_CORR, F.F_RES)
            got = download_valid(s, F.F_CORR, grids)
        finally:
            s.undefine()
        err = per_box_errors(got, ref)
        measured[label] = err
        print("%s %s: per-box max|c32 - c_oracle| / max|c_oracle| = %s (max %.3e)" % (
            case.name, label, " ".join("%.2e" % e for e in err), max(err)))
        assert all(0.0 < e <= bound for e in err), (label, err)   # > 0: the fp32 cycle did run
    return measured


def check_solve(so, case):
    """a full solve to eps 1e-10 in the mixed mode, at most one V-cycle more than fp64"""
    from somar_amd import api as F
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    rhs = residual_field(so, case, prob, seed=11)
    s = gpu_solver(case, prob)
    try:
        out = {}
        for mode in (0, 1):
            s.setPrecision(mode)
            upload(s, F.F_RHS, rhs)
            out[mode] = s.solveResident(zeroPhi=True)
        assert s.precision() == (1, case.K)
    finally:
        s.undefine()
    s64, s32 = out[0], out[1]
    print("%s solve: V-cycles fp64 %d mixed %d, final / initial %.3e / %.3e" % (
        case.name, s64["iters"], s32["iters"], s64["final_rnorm"] / s64["initial_rnorm"],
        s32["final_rnorm"] / s32["initial_rnorm"]))
    assert s32["exitStatus"] & 1 and s64["exitStatus"] & 1, (s32, s64)
    assert s32["final_rnorm"] <= 1e-10 * s32["initial_rnorm"]
    assert s32["iters"] <= s64["iters"] + 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_cycle_matches_the_oracle_per_box(oracle, monkeypatch, case):
    if case.narrow is not None:
        monkeypatch.setenv("SOMAR_NARROW_7PT", case.narrow)
    check_cycles(oracle, case)


@pytest.mark.parametrize("case", [c for c in CASES if c.name in SOLVE_CASES], ids=SOLVE_CASES)
def test_mixed_solve_on_wide_narrow_and_ragged_layouts(oracle, monkeypatch, case):
    if case.narrow is not None:
        monkeypatch.setenv("SOMAR_NARROW_7PT", case.narrow)
    check_solve(oracle, case)


# ---- the 8-row kernel family: SOMAR_FUSED_ROWS is a solver's own value, read when it is created ---------------------------
# (name, n, box, variant, periodic, L, bc types)
SWEEP_LAYOUTS = [
    ("stretched-neumann", (64, 16, 8), (64, 8, 8), "stretched", (False, True, False), (2.0, 1.0, 0.5), None),
    ("cartesian-dirichlet", (64, 32, 16), 32, "cartesian", (False, False, False), (1.0, 0.5, 0.25), [D] * 6),
]


def sweep_bit_exact(so, layout, rows):
    """the fp64 fused sweep of a solver that holds `rows` region rows, bit for bit against the oracle's relax, 1-3 sweeps"""
    from somar_amd import api as F
    name, n, box, variant, periodic, L, bc = layout
    case = Case(name, n, box, variant, periodic, L, bc, 0.0, 1.0, None, 0, None, None, None)
    prob = problem(so, case)
    dom, grids, dx, Jgup, Jinv = prob
    fac = so.Factory(dom, grids, dx, _bc_holder(so, case), Jgup, Jinv)
    op = so.AMRMultiGrid(fac, so.BiCGStab()).mg.ops[0]
    for sweeps in (1, 2, 3):
        s = gpu_solver(case, prob)
        try:
            assert s.tuning("FUSED_ROWS") == rows
            phi = so.random_field(grids, 41, (1, 1, 1), dom.box)
            rhs = so.random_field(grids, 42, (0, 0, 0), dom.box)
            upload(s, F.F_PHI, phi)
            upload(s, F.F_RHS, rhs)
            op.relax(phi, rhs, sweeps)
            s.relax(0, F.F_PHI, F.F_RHS, sweeps)
            got = download_valid(s, F.F_PHI, grids)
        finally:
            s.undefine()
        for g, w in zip(got, [f.view(b)[..., 0] for b, f in zip(phi.grids, phi.fabs)]):
            np.testing.assert_array_equal(g, w)
        print("%s: fp64 fused sweep x%d with %d rows bit-exact" % (name, sweeps, rows))


def test_8_row_kernels_between_16_row_solvers(oracle, monkeypatch):
    """16-row solvers, then 8-row solvers, then 16-row solvers again in one process.  The 8-row fused sweep takes no narrow
    lane classes and no uniform-metric kernel: the fp64 sweep bit for bit against the oracle on two layouts (stretched
    Neumann in 64-wide boxes, Cartesian with Dirichlet sides), and the fp32 cycle per box on the wide Cartesian (uniform-
    metric) case, whose 8-row sweep streams the coefficient arrays -- mp_convert_metric must have made their fp32 copies"""
    for rows in (16, 8, 16):
        if rows == 8:
            monkeypatch.setenv("SOMAR_FUSED_ROWS", "8")
        else:
            monkeypatch.delenv("SOMAR_FUSED_ROWS", raising=False)
        for layout in SWEEP_LAYOUTS:
            sweep_bit_exact(oracle, layout, rows)
        if rows == 8:
            check_cycles(oracle, next(c for c in CASES if c.name == "wide-cartesian"), rows=8)


# ---- scale equivariance ---------------------------------------------------------------------------------------------------
SCALE_KS = (-110, -60, 0, 60, 115)
SCALE_CASES = [
    Case("stretched-neumann", (64, 64, 64), 32, "stretched", (False,) * 3, (1.0, 1.0, 1.0), None, 0.0, 1.0, None, 2,
         None, None, None),
    Case("stretched-dirichlet", (64, 64, 64), 32, "stretched", (False,) * 3, (1.0, 1.0, 1.0), [D] * 6, 0.0, 1.0, None, 2,
         None, None, None),
]


@pytest.mark.parametrize("mode", [0, 1], ids=["fp64", "mixed"])
@pytest.mark.parametrize("case", SCALE_CASES, ids=[c.name for c in SCALE_CASES])
def test_solves_are_scale_equivariant(oracle, case, mode):
    """rhs * 2^k -> phi * 2^k bit for bit, the residual histories * 2^k exactly, the same V-cycles and exit status.  fp64
    (mode 0) is exactly scale-equivariant: every operation is linear and a power of two scales without rounding (no
    subnormal or overflow on this range).  The mixed mode runs its fp32 cycle on the residual normalized by a power of two,
    so it must be equivariant too; unnormalized, fp32 flushes the last corrections of k = -110 to zero and overflows at
    k = +115.  norm_thresh = 0: its default 1e-30 would stop the small cases at once."""
    from somar_amd import api as F
    so = oracle
    prob = problem(so, case)
    grids = prob[1]
    rhs = residual_field(so, case, prob, seed=11)
    s = gpu_solver(case, prob, norm_thresh=0.0)
    runs = {}
    try:
        s.setPrecision(mode)
        assert s.precision() == ((1, case.K) if mode else (0, 0))
        for k in SCALE_KS:
            for q in range(s.num_local_patches):
                _, _, gi = s.patch_box(q)
                s.upload(F.F_RHS, q, np.asfortranarray(np.ldexp(rhs[gi].a[..., 0], k)), rhs.ghost)
            st = s.solveResident(zeroPhi=True)
            runs[k] = (download_valid(s, F.F_PHI, grids), st)
    finally:
        s.undefine()
    p0, s0 = runs[0]
    bad = []
    for k in SCALE_KS:
        pk, sk = runs[k]
        nan = any(not np.all(np.isfinite(x)) for x in pk)
        same_phi = all(np.array_equal(x, np.ldexp(y, k)) for x, y in zip(pk, p0))
        same_hist = sk["history"] == [math.ldexp(h, k) for h in s0["history"]]
        print("%s %s k=%+d: V-cycles %d exitStatus %d final/initial %.3e non-finite phi %s | phi %s, history %s" % (
            case.name, "mixed" if mode else "fp64", k, sk["iters"], sk["exitStatus"],
            sk["final_rnorm"] / sk["initial_rnorm"], nan, "== 2^k phi_0" if same_phi else "differs",
            "== 2^k h_0" if same_hist else "differs"))
        if not (same_phi and same_hist and (sk["iters"], sk["exitStatus"]) == (s0["iters"], s0["exitStatus"])):
            bad.append(k)
    assert s0["exitStatus"] & 1, s0
    assert not bad, bad
