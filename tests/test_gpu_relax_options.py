"""Solver options the deck defaults never reach, on the GPU against the oracle: the relaxers other than LevelGSRB (Jacobi,
LooseGSRB), the preconditioner's mode and sweep count, and smoothing counts other than (2,2,2) / (4,4,2) inside cycles.

  * relax_mode 0 (Jacobi, Jacobi.cpp:54-90) and 2 (LooseGSRB, GSRB.cpp:104-141): sweeps on every test_gpu_parity case,
    with Dirichlet sides (constant and per-face values: the sweeps are homogeneous whatever the values), Helmholtz, 2-D,
    the 19-point / 9-point operator (Jacobi; LooseGSRB is refused there), V-cycles and solves with graphs on and off,
    AMR cycles and solves on the lean and the plain path (ratio-4 levels: mini V-cycles relaxed by the same smoother), and
    LooseGSRB's one exchange per sweep across two ranks;
  * precond_mode -1 / 0 / 1 (None / DiagRelax / DiagLineRelax, MappedAMRPoissonOp.cpp:684-734) with num_smooth_precond
    0 / 1 / 3 (2 the control), on every bottom kind: the launch-by-launch BiCGStab (0), the one-launch k_tiny_bicgstab (1),
    the persistent per-box kernel, 7- and 19-point (2); DiagLineRelax and the point relaxers other than LevelGSRB must land
    on kind 0;
  * (pre, post, bottom) with odd and zero counts: the implicit zero start, the folded prolongation of the first post sweep,
    the ping-pong copy back after an odd count and the zero-count branches, on the three LevelGSRB paths, the 19-point
    marching / fused paths and AMR.

Tolerances as in test_gpu_wcycle.py: bit-exact where every depth sums in serial order (SOMAR_ORDERED_REDUCE_MAX raised);
1e-12 of the correction's scale where a tree-summed mean intervenes; whole solves: same iterations and exit status,
history to 1e-10.  Each oracle result is computed once per module and shared by the GPU variants."""
import multiprocessing as mp
import os
import traceback
import uuid

import numpy as np
import pytest

from helpers import (download_valid, make_amr_levels, make_gpu_amr, make_gpu_solver, make_problem, max_rel_diff, upload,
                     valid_of)
from test_gpu_amr import LAYOUTS, VCYCLES
from test_gpu_parity import CASES
from test_gpu_wcycle import ORDERED_ALL, ORDERED_DEFAULT, TREE_CASES

pytestmark = pytest.mark.gpu

D_, N_ = 1, 0
JACOBI, LEVEL, LOOSE = 0, 1, 2
SMOOTH = [(1, 1, 1), (3, 3, 3), (0, 2, 2), (2, 0, 2), (2, 2, 0), (1, 3, 0)]


@pytest.fixture(scope="module")
def F():
    from somar_amd import api
    return api


@pytest.fixture(scope="module")
def am(oracle):
    from oracle import somar_amr
    return somar_amr


@pytest.fixture(params=["twopass", "fused", "fused-narrow"])
def gsrb_mode(request, monkeypatch):
    """the three LevelGSRB paths of test_gpu_parity.py"""
    monkeypatch.setenv("SOMAR_FUSED_MIN_CELLS", "0" if request.param != "twopass" else "1000000000000")
    if request.param == "fused-narrow":
        monkeypatch.setenv("SOMAR_NARROW_7PT", "1")
    return request.param


@pytest.fixture(params=["graph", "nograph"])
def graphs(request, monkeypatch):
    """SOMAR_GRAPH_CELLS = 0 turns captured cycles off; the default captures from the first depth of <= 262144 cells"""
    if request.param == "nograph":
        monkeypatch.setenv("SOMAR_GRAPH_CELLS", "0")
    else:
        monkeypatch.delenv("SOMAR_GRAPH_CELLS", raising=False)
    return request.param


@pytest.fixture(params=["lean", "plain"])
def amr_path(request, monkeypatch):
    if request.param == "plain":
        monkeypatch.setenv("SOMAR_AMR_PLAIN", "1")
    else:
        monkeypatch.delenv("SOMAR_AMR_PLAIN", raising=False)
    return request.param


def _cells(gpu):
    return [gpu.levelInfo(d)["cells"] for d in range(gpu.depth())]


def _factory(so, prob, bc=None, ndim=3, isDiagonal=True, **kw):
    dom, grids, dx, Jgup, Jinv = prob
    return so.Factory(dom, grids, dx, bc or so.BCHolder(), Jgup, Jinv, ndim=ndim, isDiagonal=isDiagonal, **kw)


def _amr(so, fac, smooth=(2, 2, 2)):
    amr = so.AMRMultiGrid(fac, so.BiCGStab())
    amr.pre, amr.post, amr.bottom = smooth
    amr.mg.pre, amr.mg.post, amr.mg.bottom = smooth
    return amr


def _problem2d(so, n=(48, 40), bs=(24, 40), variant="stretched", per=(False, False), L=(1.0, 3.0)):
    dom = so.Domain(so.Box((0, 0, 0), (n[0] - 1, n[1] - 1, 0)), per + (False,))
    grids = so.split_domain(dom.box, bs + (1,))
    dx = (L[0] / n[0], L[1] / n[1], 1.0)
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, L + (1.0,), 2, variant, domain=dom)
    return dom, grids, dx, Jgup, Jinv


def _full_problem(so, ndim):
    """the sheared (non-diagonal) map: 3-D (16,16,8) boxes of 8, or 2-D 32 x 32 boxes of 16"""
    if ndim == 3:
        n, L = (16, 16, 8), (2.0, 1.0, 0.5)
        dom = so.Domain(so.Box((0, 0, 0), (15, 15, 7)), (False, True, False))
        grids = so.split_domain(dom.box, 8)
        dx = tuple(L[d] / n[d] for d in range(3))
        Jgup, Jinv = so.make_full_metric(grids, dx, L, dom)
    else:
        L = (2.0, 1.0)
        dom = so.Domain(so.Box((0, 0, 0), (31, 31, 0)), (False, False, False))
        grids = so.split_domain(dom.box, (16, 16, 1))
        dx = (L[0] / 32, L[1] / 32, 1.0)
        Jgup, Jinv = so.make_full_metric_2d(grids, dx, L, dom)
    return dom, grids, dx, Jgup, Jinv


def _gpu_full(prob, ndim, relaxMode=LEVEL, smooth=(2, 2, 2), precondMode=None, numSmoothPrecond=None):
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv = prob
    s = AMRPressureSolver()
    s.setSpaceDim(ndim)
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond if numSmoothPrecond is None else numSmoothPrecond,
                         *smooth, p.precond_mode if precondMode is None else precondMode, relaxMode, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        jg = [np.asfortranarray(Jgup[gi][d].a) for d in range(ndim)] + [None] * (3 - ndim)
        s.setMetricFull(q, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
    try:
        s.finalize()
    except Exception:
        s.undefine()
        raise
    return s


def _sweep_check(so, F, op, gpu, grids, dom, sweeps, ghost=(1, 1, 1), seed=41):
    phi = so.random_field(grids, seed, ghost, dom.box)
    rhs = so.random_field(grids, seed + 1, (0, 0, 0), dom.box)
    upload(gpu, F.F_PHI, phi)
    upload(gpu, F.F_RHS, rhs)
    op.relax(phi, rhs, sweeps)
    gpu.relax(0, F.F_PHI, F.F_RHS, sweeps)
    for g, w in zip(download_valid(gpu, F.F_PHI, grids), valid_of(phi)):
        np.testing.assert_array_equal(g, w)


def _solve_check(gpu, F, rhs, want, forceHomogeneous=False, rtol=1e-10):
    iters, exit_status, history = want
    upload(gpu, F.F_RHS, rhs)
    st = gpu.solveResident(True, forceHomogeneous)
    assert st["iters"] == iters and st["exitStatus"] == exit_status, (st, iters, exit_status)
    np.testing.assert_allclose(st["history"], history, rtol=rtol, atol=rtol * history[0])
    return st


def _oracle_solve(amr, rhs, forceHomogeneous=False, ghost=(1, 1, 1)):
    from oracle import somar_oracle as so
    phi = so.LevelData(rhs.grids, 1, ghost)
    amr.solve(phi, rhs, forceHomogeneous=forceHomogeneous)
    return amr.iters, amr.exitStatus, list(amr.history)


# ======================================================================================================================
# 1. Jacobi and LooseGSRB sweeps
# ======================================================================================================================
@pytest.mark.parametrize("relax", [JACOBI, LOOSE])
@pytest.mark.parametrize("case", CASES)
def test_sweeps_bit_exact(oracle, F, case, relax):
    """three sweeps from a non-zero start on every parity case (the 60 + 4 and 124 + 4 lane-class boxes included)"""
    so = oracle
    prob = make_problem(so, *case)
    op = _factory(so, prob, relaxMode=relax).mg_new_op(0, None)
    gpu = make_gpu_solver(*prob, relaxMode=relax)
    try:
        _sweep_check(so, F, op, gpu, prob[1], prob[0], 3)
    finally:
        gpu.undefine()


DIRI_TYPES = [(D_, D_), (N_, N_), (N_, D_)]


def _diri_problem(so):
    return make_problem(so, (16, 16, 8), 8, "stretched", (False, False, False), (1.0, 1.0, 0.5))


@pytest.mark.parametrize("relax", [JACOBI, LOOSE])
@pytest.mark.parametrize("values", ["const", "face"])
def test_sweeps_with_dirichlet_sides_are_homogeneous(oracle, F, relax, values, monkeypatch):
    """Dirichlet sides with non-zero values (constant per side, or a plane per face): the relaxers fill the physical
    ghosts homogeneously (Jacobi's residual(.., true), fillGhostsAndExtrapolate's doBCs with homogeneous ghosts)"""
    import diri_face
    so = oracle
    prob = _diri_problem(so)
    dom, grids, dx, Jgup, Jinv = prob
    const = [(1.0, -2.0), (0.0, 0.0), (0.0, 0.5)]
    if values == "face":
        diri_face.patch(monkeypatch, so)
        planes = {(0, 0): diri_face.step_plane(dom.box, dx, 0, 0), (0, 1): diri_face.step_plane(dom.box, dx, 0, 1),
                  (2, 1): diri_face.step_plane(dom.box, dx, 2, 1)}
        vals = [[planes.get((d, s), const[d][s]) for s in (0, 1)] for d in range(3)]
    else:
        planes, vals = {}, [list(v) for v in const]
    bc = so.BCHolder([list(t) for t in DIRI_TYPES], vals)
    op = _factory(so, prob, bc=bc, relaxMode=relax).mg_new_op(0, None)
    gpu = make_gpu_solver(*prob, relaxMode=relax, bc_type=[t for p in DIRI_TYPES for t in p],
                          bc_values=[v for p in const for v in p])
    try:
        for (d, s), pl in planes.items():
            gpu.setBCFaceValues(d, s, pl)
        _sweep_check(so, F, op, gpu, grids, dom, 2)
    finally:
        gpu.undefine()


@pytest.mark.parametrize("relax", [JACOBI, LOOSE])
@pytest.mark.parametrize("case", CASES[1:4])
def test_helmholtz_sweeps_bit_exact(oracle, F, case, relax):
    so = oracle
    prob = make_problem(so, *case)
    op = _factory(so, prob, relaxMode=relax, alpha=1.0, beta=-0.05).mg_new_op(0, None)
    gpu = make_gpu_solver(*prob, relaxMode=relax, alpha=1.0, beta=-0.05)
    try:
        assert not gpu.zeroAvg(0)
        _sweep_check(so, F, op, gpu, prob[1], prob[0], 2)
    finally:
        gpu.undefine()


@pytest.mark.parametrize("relax", [JACOBI, LOOSE])
@pytest.mark.parametrize("per", [(False, False), (True, False)])
def test_2d_sweeps_bit_exact(oracle, F, relax, per):
    so = oracle
    prob = _problem2d(so, per=per)
    op = _factory(so, prob, ndim=2, relaxMode=relax).mg_new_op(0, None)
    gpu = make_gpu_solver(*prob, relaxMode=relax, ndim=2)
    try:
        _sweep_check(so, F, op, gpu, prob[1], prob[0], 3, ghost=(1, 1, 0))
    finally:
        gpu.undefine()


@pytest.mark.parametrize("ndim", [3, 2])
def test_jacobi_on_the_non_diagonal_operator(oracle, F, ndim):
    """Jacobi with the 19-point (3-D) / 9-point (2-D) operator: sweeps, one V-cycle, a solve"""
    so = oracle
    prob = _full_problem(so, ndim)
    dom, grids = prob[0], prob[1]
    ghost = (1, 1, 1) if ndim == 3 else (1, 1, 0)
    fac = _factory(so, prob, ndim=ndim, isDiagonal=False, relaxMode=JACOBI)
    gpu = _gpu_full(prob, ndim, relaxMode=JACOBI)
    try:
        amr = _amr(so, fac)
        assert gpu.depth() == amr.mg.depth and gpu.depth() >= 2
        assert all(c <= ORDERED_DEFAULT for c in _cells(gpu))
        _sweep_check(so, F, amr.mg.ops[0], gpu, grids, dom, 3, ghost=ghost)
        res = so.random_field(grids, 12345, (0, 0, 0), dom.box)
        so.remove_weighted_mean(res, amr.op.Jinv)
        corr = so.LevelData(grids, 1, ghost)
        amr.mg.init(corr, res)
        amr.mg.one_cycle(corr, res)
        upload(gpu, F.F_RES, res)
        gpu.setVal(F.F_CORR, 0.0)
        gpu.vcycle(F.F_CORR, F.F_RES)
        for a, b in zip(download_valid(gpu, F.F_CORR, grids), valid_of(corr)):
            np.testing.assert_array_equal(a, b)
        rhs = so.LevelData(grids, 1)
        amr.op.apply_op(rhs, so.random_field(grids, 3, ghost, dom.box), True)
        want = _oracle_solve(amr, rhs, ghost=ghost)
        _solve_check(gpu, F, rhs, want, rtol=1e-9)
    finally:
        gpu.undefine()


@pytest.mark.parametrize("ndim", [3, 2])
def test_loose_gsrb_is_refused_with_the_non_diagonal_metric(oracle, ndim):
    so = oracle
    prob = _full_problem(so, ndim)
    with pytest.raises(Exception, match="the non-diagonal metric path offers LevelGSRB, LineGSRB and Jacobi"):
        _gpu_full(prob, ndim, relaxMode=LOOSE)


# ======================================================================================================================
# 2. Jacobi and LooseGSRB in cycles and solves
# ======================================================================================================================
_LEVEL = {}


def _level_oracle(so, case, relax, smooth=(2, 2, 2)):
    """the oracle's one V-cycle from zero and whole solve on a test_gpu_parity case"""
    key = (repr(case), relax, smooth)
    if key not in _LEVEL:
        prob = make_problem(so, *case)
        dom, grids = prob[0], prob[1]
        amr = _amr(so, _factory(so, prob, relaxMode=relax), smooth)
        res = so.random_field(grids, 12345, (0, 0, 0), dom.box)
        so.remove_weighted_mean(res, prob[4])
        corr = so.LevelData(grids, 1, (1, 1, 1))
        amr.mg.init(corr, res)
        amr.mg.one_cycle(corr, res)
        cyc = [np.array(a) for a in valid_of(corr)]
        _LEVEL[key] = (prob, res, cyc, [op.domain.box.numPts() for op in amr.mg.ops], _oracle_solve(amr, res))
    return _LEVEL[key]


@pytest.mark.parametrize("relax", [JACOBI, LOOSE])
@pytest.mark.parametrize("case", [CASES[0], CASES[5]])
def test_level_vcycle_and_solve(oracle, F, case, relax, graphs, monkeypatch):
    """one V-cycle (every depth summed in serial order: bit-exact) and a whole solve, with graphs on and off"""
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", ORDERED_ALL)
    prob, res, cyc, cells, want = _level_oracle(oracle, case, relax)
    gpu = make_gpu_solver(*prob, relaxMode=relax)
    try:
        assert _cells(gpu) == cells and len(cells) >= 3
        upload(gpu, F.F_RES, res)
        gpu.vcycleFromZero(F.F_CORR, F.F_RES)
        for g, w in zip(download_valid(gpu, F.F_CORR, prob[1]), cyc):
            np.testing.assert_array_equal(g, w)
        _solve_check(gpu, F, res, want)
        assert gpu.bottomKind() == 0   # the point relaxers other than LevelGSRB: launch-by-launch bottom
    finally:
        gpu.undefine()


_LEVEL_SOLVES = {}


@pytest.mark.parametrize("relax", [JACOBI, LOOSE])
@pytest.mark.parametrize("kind", ["dirichlet", "helmholtz", "2d"])
def test_level_solves(oracle, F, relax, kind):
    so = oracle
    key = (relax, kind)
    ndim, fh, kw = 3, False, {}
    if kind == "dirichlet":
        prob = _diri_problem(so)
        bc = so.BCHolder([list(t) for t in DIRI_TYPES])
        kw = dict(bc_type=[t for p in DIRI_TYPES for t in p])
        fh = True
    elif kind == "helmholtz":
        prob = make_problem(so, *CASES[1])
        bc = None
        kw = dict(alpha=1.0, beta=-0.05)
    else:
        prob, bc, ndim = _problem2d(so), None, 2
    dom, grids = prob[0], prob[1]
    ghost = (1, 1, 1) if ndim == 3 else (1, 1, 0)
    if key not in _LEVEL_SOLVES:
        fkw = {k: v for k, v in kw.items() if k in ("alpha", "beta")}
        amr = _amr(so, _factory(so, prob, bc=bc, ndim=ndim, relaxMode=relax, **fkw))
        if kind == "dirichlet":
            phi0 = so.random_field(grids, 3, ghost, dom.box)
            rhs = so.LevelData(grids, 1)
            amr.op.apply_op(rhs, phi0, True)
        else:
            rhs = so.random_field(grids, 12345, (0, 0, 0), dom.box)
            if kind == "2d":
                so.remove_weighted_mean(rhs, prob[4])
        _LEVEL_SOLVES[key] = (rhs, amr.mg.depth, _oracle_solve(amr, rhs, forceHomogeneous=fh, ghost=ghost))
    rhs, depth, want = _LEVEL_SOLVES[key]
    gpu = make_gpu_solver(*prob, relaxMode=relax, ndim=ndim, **kw)
    try:
        assert gpu.depth() == depth and depth >= 2
        _solve_check(gpu, F, rhs, want, forceHomogeneous=fh)
    finally:
        gpu.undefine()


def _amr_levels(so, am, layout):
    periodic, ratios, boxes = layout
    fb = [[so.Box(lo, hi) for lo, hi in lev] for lev in boxes]
    return make_amr_levels(so, am, (16, 16, 8), (2.0, 1.0, 0.5), periodic, ratios, fb), ratios


_AMR = {}


def _amr_oracle(so, am, case, relax, smooth):
    """the oracle's AMRVCycle and AMR solve on a test_gpu_amr layout"""
    layout, lmax, lbase = case
    key = (repr(case), relax, smooth)
    if key not in _AMR:
        levels, ratios = _amr_levels(so, am, layout)
        comp = am.AMRComposite(levels, ratios, so.BCHolder(), so.BiCGStab(), relaxMode=relax)
        comp.pre, comp.post, comp.bottom = smooth
        phi = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        res = [so.random_field(L.grids, 70 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
        for l in range(lbase, lmax):
            comp.zero_covered(l, res[l])
        comp.init(phi, res, lmax, lbase)
        comp.set_bottom_solver(lmax, lbase)
        corr = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.amr_vcycle(corr, res, lmax, lmax, lbase)
        cyc = [[np.array(a) for a in valid_of(c)] for c in corr]
        top = len(levels) - 1
        src = [so.random_field(L.grids, 5 + l, (1, 1, 1), L.domain.box) for l, L in enumerate(levels)]
        zero = [so.LevelData(L.grids, 1) for L in levels]
        rhs = [so.LevelData(L.grids, 1) for L in levels]
        comp.init(src, zero, top, 0)
        comp.compute_amr_residual(rhs, src, zero, top, 0, True)
        for r in rhs:
            so.ld_scale(r, -1.0)
        sol = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.solve(sol, rhs, top, 0)
        _AMR[key] = (levels, ratios, res, cyc, [m.maxForcedDepth for m in comp.mg], rhs,
                     (comp.iters, comp.exitStatus, list(comp.history)))
    return _AMR[key]


def _gpu_amr_check(so, am, F, case, relax, smooth):
    layout, lmax, lbase = case
    levels, ratios, res, cyc, forced, rhs, (iters, exit_status, history) = _amr_oracle(so, am, case, relax, smooth)
    pre, post, bottom = smooth
    gpu = make_gpu_amr(levels, ratios, relaxMode=relax, pre=pre, post=post, bottom=bottom)
    try:
        assert all(c <= ORDERED_DEFAULT for c in _cells(gpu.levels[lbase])) and lmax > lbase
        for l in range(lbase + 1, lmax + 1):
            if max(ratios[l - 1]) > 2:     # a mini V-cycle over the forced depths, relaxed by the same smoother
                assert forced[l] >= 1 and gpu.levels[l].depth() >= 2
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RES, res[l])
            v.setVal(F.F_CORR, 0.0)
        gpu.vcycleAMR(lmax, lbase)
        for l in range(lbase, lmax + 1):
            for g, w in zip(download_valid(gpu.levels[l], F.F_CORR, levels[l].grids), cyc[l]):
                np.testing.assert_array_equal(g, w)
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RHS, rhs[l])
        st = gpu.solveAMR(len(levels) - 1, 0)
        assert st["iters"] == iters and st["exitStatus"] == exit_status
        np.testing.assert_allclose(st["history"], history, rtol=1e-10, atol=0.0)
    finally:
        gpu.undefine()


# two levels, three levels (l_base 0), a ratio-4 level (mini V-cycles)
AMR_CASES = [VCYCLES[0], VCYCLES[2], (LAYOUTS[5], 1, 0)]


@pytest.mark.parametrize("relax", [JACOBI, LOOSE])
@pytest.mark.parametrize("case", AMR_CASES)
def test_amr_vcycle_and_solve(oracle, am, F, case, relax, amr_path):
    """the fine levels' sweeps next to coarse-fine faces (homogeneous CF interpolation before each sweep / exchange)"""
    _gpu_amr_check(oracle, am, F, case, relax, (2, 2, 2))


# ---- LooseGSRB across two ranks ---------------------------------------------------------------------------------------
def _loose_worker(rank, nranks, name, q):
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, here)
        sys.path.insert(0, os.path.dirname(here))
        from oracle import somar_oracle as so
        from somar_amd import api as F
        from helpers import make_gpu_solver, make_oracle_solver, make_problem
        comm = F.comm_create_shm(name, rank, nranks)
        dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 32, 32), 16, "stretched", (False, True, False), (2.0, 1.0, 1.0))
        owner = [i % nranks for i in range(len(grids))]
        amr = make_oracle_solver(so, dom, grids, dx, Jgup, Jinv, relaxMode=so.RELAX_LOOSE_GSRB)

        class Mine:
            def __init__(self, x):
                self.x = x

            def __getitem__(self, gi):
                assert owner[gi] == rank
                return self.x[gi]

        gpu = make_gpu_solver(dom, grids, dx, Mine(Jgup), Mine(Jinv), owner=owner, comm=comm, relaxMode=2)
        assert gpu.depth() == amr.mg.depth and gpu.depth() >= 3
        b = so.random_field(grids, 12345, (0, 0, 0), dom.box)
        so.remove_weighted_mean(b, Jinv)
        x = so.LevelData(grids, 1, (1, 1, 1))
        amr.solve(x, b)
        upload(gpu, F.F_RHS, b)
        st = gpu.solveResident(True, False)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus, (st, amr.iters, amr.exitStatus)
        np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-10 * amr.history[0])
        gpu.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_loose_gsrb_solve_on_two_ranks():
    """LooseGSRB's one exchange per sweep is the one that crosses ranks (8 boxes dealt round-robin, shared-memory transport)"""
    nranks = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/somar_%s" % uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=_loose_worker, args=(r, nranks, name, q)) for r in range(nranks)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in procs:
            rank, msg = q.get(timeout=240)
            out[rank] = msg
    finally:
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()
    assert out == {r: "ok" for r in range(nranks)}, "\n".join("rank %d: %s" % kv for kv in sorted(out.items()))


# ======================================================================================================================
# 3. Preconditioner mode and sweep count on every bottom kind
# ======================================================================================================================
PRECONDS = [(m, k) for m in (-1, 0, 1) for k in (0, 1, 3)] + [(0, 2)]
BOTTOM_ENV = {   # kind -> environment that selects it (read when the solver is created)
    0: dict(SOMAR_FUSED_BOTTOM_MAX_CELLS="0", SOMAR_BOX_BOTTOM="0"),
    1: dict(SOMAR_BOX_BOTTOM="0"),
    2: dict(SOMAR_FUSED_BOTTOM_MAX_CELLS="0", SOMAR_BOX_BOTTOM="1", SOMAR_BOX_BOTTOM_MIN_CELLS="1"),
}
PRECOND_CASE = CASES[1]   # [32768, 4096, 512]: a bottom of 8 boxes of 4^3
_PRECOND = {}


def _precond_oracle(so, full, mode, k, relax=LEVEL):
    """the oracle's bottom BiCGStab alone and the whole solve, with AMRMG.precondMode / num_smooth_precond"""
    key = (full, mode, k, relax)
    if key not in _PRECOND:
        if full:
            prob = _full_problem(so, 3)
        else:
            prob = make_problem(so, *PRECOND_CASE)
        dom, grids = prob[0], prob[1]
        amr = _amr(so, _factory(so, prob, isDiagonal=not full, relaxMode=relax, precondMode=mode, precondIters=k))
        opb = amr.mg.ops[-1]
        if full:   # right-hand sides in the operator's range (test_gpu_wcycle's 19-point solves)
            brhs = so.LevelData(opb.grids, 1)
            opb.apply_op(brhs, so.random_field(opb.grids, 91, (1, 1, 1), opb.domain.box), True)
            rhs = so.LevelData(grids, 1)
            amr.op.apply_op(rhs, so.random_field(grids, 3, (1, 1, 1), dom.box), True)
        else:
            brhs = so.random_field(opb.grids, 91, (0, 0, 0), opb.domain.box)
            so.remove_weighted_mean(brhs, opb.Jinv)
            rhs = so.random_field(grids, 12345, (0, 0, 0), dom.box)
            so.remove_weighted_mean(rhs, prob[4])
        bphi = so.LevelData(opb.grids, 1, (1, 1, 1))
        bs = so.BiCGStab()
        bs.define(opb, True)
        bs.solve(bphi, brhs)
        _PRECOND[key] = (prob, amr.mg.depth, opb.grids, brhs, (bs.iters, bs.exitStatus, valid_of(bphi)),
                         rhs, _oracle_solve(amr, rhs))
    return _PRECOND[key]


def _precond_check(so, F, full, mode, k, kind, relax=LEVEL, want_kind=None):
    prob, D, bgrids, brhs, (bit, bex, bsol), rhs, want = _precond_oracle(so, full, mode, k, relax)
    gpu = _gpu_full(prob, 3, relaxMode=relax, precondMode=mode, numSmoothPrecond=k) if full else \
        make_gpu_solver(*prob, relaxMode=relax, precondMode=mode, numSmoothPrecond=k)
    try:
        assert gpu.depth() == D >= 2
        fp, fr = F.FIELD(D - 1, F.F_CORR), F.FIELD(D - 1, F.F_RES)
        upload(gpu, fr, brhs, depth=D - 1)
        gpu.setVal(fp, 0.0)
        it, ex = gpu.bottomSolve(fp, fr)
        assert gpu.bottomKind() == (kind if want_kind is None else want_kind)
        assert (it, ex) == (bit, bex)
        assert max_rel_diff(download_valid(gpu, fp, bgrids, D - 1), bsol) < 1e-11
        _solve_check(gpu, F, rhs, want)
        assert gpu.bottomKind() == (kind if want_kind is None else want_kind)
    finally:
        gpu.undefine()


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("mode,k", PRECONDS)
def test_precond_bottom_and_solve(oracle, F, mode, k, kind, monkeypatch):
    """bottom BiCGStab alone, then a whole solve; DiagLineRelax (a LineGSRB of its own) only on the launch path"""
    for n_, v in BOTTOM_ENV[kind].items():
        monkeypatch.setenv(n_, v)
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", ORDERED_ALL)
    _precond_check(oracle, F, False, mode, k, kind, want_kind=0 if mode == 1 else kind)


# (the 19-point oracle is the slow part: each mode's no-preconditioner and odd-count branches, and the control)
FULL_PRECONDS = [(-1, 1), (0, 0), (0, 1), (0, 3), (1, 1), (0, 2)]


@pytest.mark.parametrize("mode,k", FULL_PRECONDS)
def test_precond_nineteen_point_box_bottom_and_solve(oracle, F, mode, k, monkeypatch):
    for n_, v in BOTTOM_ENV[2].items():
        monkeypatch.setenv(n_, v)
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", ORDERED_ALL)
    _precond_check(oracle, F, True, mode, k, 2, want_kind=0 if mode == 1 else 2)


@pytest.mark.parametrize("relax", [JACOBI, LOOSE])
@pytest.mark.parametrize("k", [1, 3])
def test_precond_with_other_point_relaxers(oracle, F, relax, k, monkeypatch):
    """DiagRelax with Jacobi / LooseGSRB: the preconditioner sweeps with that relaxer; the fused and box bottoms refuse it"""
    monkeypatch.delenv("SOMAR_FUSED_BOTTOM_MAX_CELLS", raising=False)
    monkeypatch.setenv("SOMAR_BOX_BOTTOM", "1")
    monkeypatch.setenv("SOMAR_BOX_BOTTOM_MIN_CELLS", "1")
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", ORDERED_ALL)
    _precond_check(oracle, F, False, 0, k, 0, relax=relax)


def test_precond_level_kernel_every_mode(oracle, F):
    """preCond on depth 0 (the level call): None copies, DiagLineRelax sweeps a LineGSRB, bit for bit"""
    so = oracle
    prob = make_problem(so, *PRECOND_CASE)
    dom, grids = prob[0], prob[1]
    rhs = so.random_field(grids, 82, (0, 0, 0), dom.box)
    for mode, k in PRECONDS:
        op = _factory(so, prob, precondMode=mode, precondIters=k).mg_new_op(0, None)
        phi = so.LevelData(grids, 1, (1, 1, 1))
        op.pre_cond(phi, rhs)
        gpu = make_gpu_solver(*prob, precondMode=mode, numSmoothPrecond=k)
        try:
            upload(gpu, F.F_RHS, rhs)
            gpu.setVal(F.F_PHI, 7.0)
            gpu.preCond(0, F.F_PHI, F.F_RHS)
            for g, w in zip(download_valid(gpu, F.F_PHI, grids), valid_of(phi)):
                np.testing.assert_array_equal(g, w, err_msg=str((mode, k)))
        finally:
            gpu.undefine()


# ======================================================================================================================
# 4. Smoothing counts inside cycles
# ======================================================================================================================
@pytest.mark.parametrize("smooth", SMOOTH)
def test_level_cycle_counts_bit_exact(oracle, F, smooth, gsrb_mode, graphs, monkeypatch):
    """one V-cycle from zero twice on one solver: the second finds the coarse corrections of the first in the arrays (a
    zero count must clear them itself) and must give the same bits; both equal to the oracle"""
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", ORDERED_ALL)
    prob, res, cyc, cells, want = _level_oracle(oracle, CASES[0], LEVEL, smooth)
    pre, post, bottom = smooth
    gpu = make_gpu_solver(*prob, pre=pre, post=post, bottom=bottom)
    try:
        assert _cells(gpu) == cells and len(cells) >= 4
        upload(gpu, F.F_RES, res)
        for _ in range(2):
            gpu.vcycleFromZero(F.F_CORR, F.F_RES)
            for g, w in zip(download_valid(gpu, F.F_CORR, prob[1]), cyc):
                np.testing.assert_array_equal(g, w)
        _solve_check(gpu, F, res, want)
    finally:
        gpu.undefine()


_TREE = {}


@pytest.mark.parametrize("smooth", SMOOTH)
def test_level_cycle_counts_tree_sums(oracle, F, smooth, gsrb_mode, monkeypatch):
    """default ordered-sum limit on [65536, 8192, 1024]: depths 0 and 1 take tree-summed means, and on the fused paths
    the first post sweep folds the prolongation (fold_prolong) when post > 0 and the plain prolongation runs when post = 0"""
    so = oracle
    monkeypatch.delenv("SOMAR_ORDERED_REDUCE_MAX", raising=False)
    case = TREE_CASES[1]
    key = smooth
    if key not in _TREE:
        prob = make_problem(so, *case)
        amr = _amr(so, _factory(so, prob), smooth)
        res = so.random_field(prob[1], 12345, (0, 0, 0), prob[0].box)
        so.remove_weighted_mean(res, prob[4])
        corr = so.LevelData(prob[1], 1, (1, 1, 1))
        amr.mg.init(corr, res)
        amr.mg.one_cycle(corr, res)
        _TREE[key] = (prob, res, [np.array(a) for a in valid_of(corr)])
    prob, res, want = _TREE[key]
    pre, post, bottom = smooth
    gpu = make_gpu_solver(*prob, pre=pre, post=post, bottom=bottom)
    try:
        cells = _cells(gpu)
        assert len(cells) >= 3 and cells[1] > ORDERED_DEFAULT and gpu.zeroAvg(1)
        upload(gpu, F.F_RES, res)
        scale = max(float(np.abs(w).max()) for w in want)
        for _ in range(2):
            gpu.vcycleFromZero(F.F_CORR, F.F_RES)
            for g, w in zip(download_valid(gpu, F.F_CORR, prob[1]), want):
                np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * scale)
    finally:
        gpu.undefine()


@pytest.fixture(params=["march", "fused"])
def full_path(request, monkeypatch):
    """the 19-point marching sweep (two passes per sweep, ping-pong) or the fused red+black marching sweep"""
    monkeypatch.setenv("SOMAR_MARCH_MIN_CELLS", "0")
    monkeypatch.setenv("SOMAR_FUSED19_MIN_BOX", "0" if request.param == "fused" else "-1")
    return request.param


_FULL = {}


@pytest.mark.parametrize("smooth", [(1, 1, 1), (3, 3, 3)])
def test_nineteen_point_cycle_counts(oracle, F, smooth, full_path):
    so = oracle
    prob = _full_problem(so, 3)
    dom, grids = prob[0], prob[1]
    if smooth not in _FULL:
        amr = _amr(so, _factory(so, prob, isDiagonal=False), smooth)
        res = so.random_field(grids, 12345, (0, 0, 0), dom.box)
        so.remove_weighted_mean(res, amr.op.Jinv)
        corr = so.LevelData(grids, 1, (1, 1, 1))
        amr.mg.init(corr, res)
        amr.mg.one_cycle(corr, res)
        rhs = so.LevelData(grids, 1)
        amr.op.apply_op(rhs, so.random_field(grids, 3, (1, 1, 1), dom.box), True)
        _FULL[smooth] = (res, [np.array(a) for a in valid_of(corr)], amr.mg.depth, rhs, _oracle_solve(amr, rhs))
    res, cyc, depth, rhs, want = _FULL[smooth]
    gpu = _gpu_full(prob, 3, smooth=smooth)
    try:
        assert gpu.depth() == depth >= 2 and all(c <= ORDERED_DEFAULT for c in _cells(gpu))
        if full_path == "fused":
            before = gpu.fused19Sweeps()
        upload(gpu, F.F_RES, res)
        gpu.vcycleFromZero(F.F_CORR, F.F_RES)
        if full_path == "fused":
            assert gpu.fused19Sweeps() > before
        for a, b in zip(download_valid(gpu, F.F_CORR, grids), cyc):
            np.testing.assert_array_equal(a, b)
        _solve_check(gpu, F, rhs, want, rtol=1e-9)
    finally:
        gpu.undefine()


@pytest.mark.parametrize("smooth", SMOOTH)
@pytest.mark.parametrize("case", [VCYCLES[2], (LAYOUTS[5], 1, 0)])
def test_amr_cycle_counts(oracle, am, F, case, smooth, amr_path):
    _gpu_amr_check(oracle, am, F, case, LEVEL, smooth)
