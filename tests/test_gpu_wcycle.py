"""W-cycles (numMG >= 2, AMRMG.numMG in every shipped input deck, "2 = W-cycle") on the GPU against the oracle.

What only numMG >= 2 reaches:
  * MappedMultiGrid::cycle's second (third) coarse recursion (MappedMultiGrid.H:628-633): the coarser correction is zeroed
    once, every later recursion starts from the previous one's result -- PressureSolver::cycle passes corr_zero = (img == 0),
    so the fused sweep must READ the array there; a revisited depth above the ordered-sum limit also runs fold_prolong's
    fold sums a second time;
  * agglom_cycle's gather of a non-zero correction into the replicated coarse tail (two ranks);
  * AMRVCycle's numMG recursions (MappedAMRMultiGrid.H:1552-1554): the base level's oneCycle continues from its previous
    visit's correction (tests/test_oracle_amr.py pins that in the oracle), the lean path's per-level visit bookkeeping, and
    the mini V-cycles of ratio-4 levels, which run numMG inner cycles (:742-754 via m_cycle);
  * the graph path refuses numMG != 1 and the plain launches must then give the oracle's answer.

Tolerances as elsewhere: bit-exact where every depth sums in the reference's serial order (at most SOMAR_ORDERED_REDUCE_MAX
cells, default 4096; raised to cover everything in the "ordered" runs); 1e-12 of the correction's scale per box where a
tree-summed mean of a larger depth intervenes; whole solves: same iterations and exit status, history to 1e-10.

Every case first asserts that it reaches what it is for (hierarchy depth, the cells that put a revisited depth on the
ordered or the tree-sum path, the bottom kind)."""
import multiprocessing as mp
import os
import traceback
import uuid

import numpy as np
import pytest

from helpers import (download_valid, make_amr_levels, make_full_amr_levels, make_gpu_amr, make_gpu_solver,
                     make_oracle_solver, make_problem, max_rel_diff, upload, valid_of)
from test_gpu_amr import LAYOUTS, RATIO4, VCYCLES
from test_gpu_parity import CASES

pytestmark = pytest.mark.gpu

ORDERED_DEFAULT = 4096      # PressureSolver::ordered_max_cells_
ORDERED_ALL = "100000000"

# depth >= 3 (a revisited depth that is not the bottom): [cells per depth] in the comments
ORDERED_CASES = [CASES[0],   # [32768, 4096, 512, 64]
                 CASES[1],   # [32768, 4096, 512]
                 CASES[2],   # [32768, 8192, 1024]
                 CASES[5],   # [8192, 4096, 512]: 64-wide tile columns (60 + 4)
                 CASES[6]]   # [8192, 4096, 2048, 256]: 128-wide tile columns (124 + 4)
# a revisited depth above 4096 cells: with the default ordered-sum limit its mean is a tree sum, and on the fused paths
# fold_prolong runs there (fused sweep + not ordered + no coarse-fine faces + zeroAvg with a valid fold, solver.cpp)
TREE_CASES = [CASES[2],    # [32768, 8192, 1024]
              ((64, 64, 16), 32, "stretched", (False, True, False), (1.0, 1.0, 0.25))]   # [65536, 8192, 1024]


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


def _cells(gpu):
    return [gpu.levelInfo(d)["cells"] for d in range(gpu.depth())]


# ---- single level: one cycle -----------------------------------------------------------------------------------------
_LEVEL = {}   # (case, numMG) -> the oracle's cycle, shared by the GPU variants


def _level_cycle(so, case, numMG):
    key = (repr(case), numMG)
    if key not in _LEVEL:
        n, boxsz, variant, periodic, L = case
        dom, grids, dx, Jgup, Jinv = make_problem(so, n, boxsz, variant, periodic, L)
        amr = make_oracle_solver(so, dom, grids, dx, Jgup, Jinv)
        amr.mg.cycle_type = numMG
        res = so.random_field(grids, 12345, (0, 0, 0), dom.box)
        so.remove_weighted_mean(res, Jinv)
        corr = so.LevelData(grids, 1, (1, 1, 1))
        amr.mg.init(corr, res)
        amr.mg.one_cycle(corr, res)
        _LEVEL[key] = (dom, grids, dx, Jgup, Jinv, res, [np.array(a) for a in valid_of(corr)],
                       [op.domain.box.numPts() for op in amr.mg.ops])
    return _LEVEL[key]


def _gpu_level_cycle(F, so, case, numMG):
    dom, grids, dx, Jgup, Jinv, res, want, cells = _level_cycle(so, case, numMG)
    gpu = make_gpu_solver(dom, grids, dx, Jgup, Jinv, numMG=numMG)
    try:
        assert _cells(gpu) == cells and gpu.depth() >= 3
        upload(gpu, F.F_RES, res)
        gpu.setVal(F.F_CORR, 0.0)
        gpu.vcycle(F.F_CORR, F.F_RES)
        return download_valid(gpu, F.F_CORR, grids), want, cells
    finally:
        gpu.undefine()


@pytest.mark.parametrize("case,numMG", [(c, 2) for c in ORDERED_CASES] + [(CASES[0], 3), (CASES[5], 3)])
def test_level_w_cycle_bit_exact(oracle, case, numMG, gsrb_mode, F, monkeypatch):
    """every depth sums in serial order: the whole W-cycle -- revisits of depth >= 1 from a non-zero correction included --
    reproduces the oracle bit for bit"""
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", ORDERED_ALL)
    got, want, _ = _gpu_level_cycle(F, oracle, case, numMG)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("case", TREE_CASES)
def test_level_w_cycle_tree_sums(oracle, case, gsrb_mode, F, monkeypatch):
    """default ordered-sum limit: depth 1 (8192 cells) is revisited above it -- its mean is a tree sum, and on the fused
    paths its prolongation is folded into the up-sweep (fold_prolong) -- so round-off, not bits"""
    monkeypatch.delenv("SOMAR_ORDERED_REDUCE_MAX", raising=False)
    got, want, cells = _gpu_level_cycle(F, oracle, case, 2)
    assert len(cells) >= 3 and cells[1] > ORDERED_DEFAULT
    scale = max(float(np.abs(w).max()) for w in want)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * scale)


# ---- single level: whole solves ------------------------------------------------------------------------------------
def _solve_both(so, dom, grids, dx, Jgup, Jinv, numMG, rhs_seed=12345, compatible=True, oracle_kw=None, **kw):
    amr = make_oracle_solver(so, dom, grids, dx, Jgup, Jinv, **(oracle_kw or {}))
    amr.numMG = numMG
    amr.mg.cycle_type = numMG
    rhs = so.random_field(grids, rhs_seed, (0, 0, 0), dom.box)
    if compatible:
        so.remove_weighted_mean(rhs, Jinv)
    phi = so.LevelData(grids, 1, (1, 1, 1))
    amr.solve(phi, rhs)
    gpu = make_gpu_solver(dom, grids, dx, Jgup, Jinv, numMG=numMG, **kw)
    try:
        gphi = [np.zeros(f.a.shape[:3], order="F") for f in phi.fabs]
        grhs = [np.asfortranarray(f.a[..., 0]) for f in rhs.fabs]
        st = gpu.solve(gphi, grhs, 0, 0, True, False)
        kind = gpu.bottomKind()
        depth = gpu.depth()
    finally:
        gpu.undefine()
    assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus, (st, amr.iters, amr.exitStatus)
    np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-10 * amr.history[0])
    got = [a[1:-1, 1:-1, 1:-1] for a in gphi]
    assert max_rel_diff(got, valid_of(phi)) < 1e-8
    return st, got, kind, depth


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5]])
def test_level_w_solve_history(oracle, case, monkeypatch):
    """numMG = 2 solves with the default graph thresholds and with graphs off: the graph path refuses numMG != 1
    (PressureSolver::graph_cycle), so both run the plain launches and must agree bit for bit, and with the oracle"""
    so = oracle
    n, boxsz, variant, periodic, L = case
    dom, grids, dx, Jgup, Jinv = make_problem(so, n, boxsz, variant, periodic, L)
    out = {}
    for graph in ("default", "0"):
        if graph == "0":
            monkeypatch.setenv("SOMAR_GRAPH_CELLS", "0")
        else:
            monkeypatch.delenv("SOMAR_GRAPH_CELLS", raising=False)
        st, got, _, depth = _solve_both(so, dom, grids, dx, Jgup, Jinv, 2)
        assert depth >= 3
        out[graph] = (st, got)
    np.testing.assert_array_equal(out["default"][0]["history"], out["0"][0]["history"])
    for a, b in zip(out["default"][1], out["0"][1]):
        np.testing.assert_array_equal(a, b)


def test_level_w_solve_helmholtz(oracle):
    """alpha != 0: no zero-average depths, no mean removal"""
    so = oracle
    n, boxsz, variant, periodic, L = CASES[1]
    dom, grids, dx, Jgup, Jinv = make_problem(so, n, boxsz, variant, periodic, L)
    _, _, _, depth = _solve_both(so, dom, grids, dx, Jgup, Jinv, 2, compatible=False,
                                 oracle_kw=dict(alpha=1.0, beta=-0.05), alpha=1.0, beta=-0.05)
    assert depth >= 3


def test_level_w_solve_dirichlet(oracle):
    """Dirichlet sides (homogeneous): the GHOST_DIRI ops on every depth a W-cycle revisits"""
    so = oracle
    D_, N_ = 1, 0
    types = [(D_, D_), (N_, N_), (N_, D_)]
    dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 32, 16), 16, "stretched", (False, False, False), (1.0, 1.0, 0.5))
    bc = so.BCHolder([list(t) for t in types])
    fac = so.Factory(dom, grids, dx, bc, Jgup, Jinv)
    amr = so.AMRMultiGrid(fac, so.BiCGStab())
    amr.numMG = 2
    amr.mg.cycle_type = 2
    phi0 = so.random_field(grids, 3, (1, 1, 1), dom.box)
    b = so.LevelData(grids, 1)
    amr.op.apply_op(b, phi0, True)
    x = so.LevelData(grids, 1, (1, 1, 1))
    amr.solve(x, b, forceHomogeneous=True)
    gpu = make_gpu_solver(dom, grids, dx, Jgup, Jinv, bc_type=[t for pair in types for t in pair], numMG=2)
    try:
        assert gpu.depth() == amr.mg.depth and gpu.depth() >= 3
        gx = [np.zeros(f.a.shape[:3], order="F") for f in x.fabs]
        gb = [np.asfortranarray(f.a[..., 0]) for f in b.fabs]
        st = gpu.solve(gx, gb, 0, 0, True, True)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-13 * amr.history[0])
        assert st["history"][-1] <= 1e-6 * st["history"][0]
    finally:
        gpu.undefine()


def test_level_w_solve_line_relaxation(oracle):
    """relaxMode 3 (vertical-line GSRB) on every depth"""
    so = oracle
    n, boxsz, variant, periodic, L = CASES[0]
    dom, grids, dx, Jgup, Jinv = make_problem(so, n, boxsz, variant, periodic, L)
    _, _, _, depth = _solve_both(so, dom, grids, dx, Jgup, Jinv, 2, oracle_kw=dict(relaxMode=so.RELAX_LINE_GSRB),
                                 relaxMode=3)
    assert depth >= 3


def test_level_w_cycle_box_bottom(oracle, F, monkeypatch):
    """the persistent one-workgroup-per-box BiCGStab bottom (8 boxes of 4^3), entered four times per W-cycle, every second
    visit from a non-zero correction: equal to the launch-by-launch bottom bit for bit, and to the oracle"""
    so = oracle
    monkeypatch.setenv("SOMAR_BOX_BOTTOM_MIN_CELLS", "1")
    monkeypatch.setenv("SOMAR_FUSED_BOTTOM_MAX_CELLS", "0")
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", "1000000")
    case = CASES[1]
    dom, grids, dx, Jgup, Jinv, res, want, cells = _level_cycle(so, case, 2)
    assert cells == [32768, 4096, 512] and len(grids) == 8
    out = {}
    for on in (False, True):
        monkeypatch.setenv("SOMAR_BOX_BOTTOM", "1" if on else "0")
        gpu = make_gpu_solver(dom, grids, dx, Jgup, Jinv, numMG=2)
        try:
            upload(gpu, F.F_RES, res)
            gpu.setVal(F.F_CORR, 0.0)
            gpu.vcycle(F.F_CORR, F.F_RES)
            assert gpu.bottomKind() == (2 if on else 0)
            cyc = download_valid(gpu, F.F_CORR, grids)
            upload(gpu, F.F_RHS, res)
            st = gpu.solveResident(True, False)
            assert gpu.bottomKind() == (2 if on else 0)
            out[on] = (cyc, st)
        finally:
            gpu.undefine()
    for a, b, w in zip(out[False][0], out[True][0], want):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(b, w)
    np.testing.assert_array_equal(out[False][1]["history"], out[True][1]["history"])
    amr = make_oracle_solver(so, dom, grids, dx, Jgup, Jinv)
    amr.numMG = 2
    amr.mg.cycle_type = 2
    x = so.LevelData(grids, 1, (1, 1, 1))
    amr.solve(x, res)
    st = out[True][1]
    assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
    np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-10 * amr.history[0])


# ---- 19-point (non-diagonal metric), 3-D and 2-D ---------------------------------------------------------------------
def _full_setup(so, n, bs, per, L, ndim, numMG):
    from somar_amd import AMRPressureSolver
    if ndim == 3:
        dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), per)
        grids = so.split_domain(dom.box, bs)
        dx = tuple(L[d] / n[d] for d in range(3))
        Jgup, Jinv = so.make_full_metric(grids, dx, L, dom)
    else:
        dom = so.Domain(so.Box((0, 0, 0), (n[0] - 1, n[1] - 1, 0)), (per[0], per[1], False))
        grids = so.split_domain(dom.box, (bs, bs, 1))
        dx = (L[0] / n[0], L[1] / n[1], 1.0)
        Jgup, Jinv = so.make_full_metric_2d(grids, dx, L, dom)
    fac = so.Factory(dom, grids, dx, so.BCHolder(), Jgup, Jinv, isDiagonal=False, ndim=ndim)
    s = AMRPressureSolver()
    s.setSpaceDim(ndim)
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, numMG, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        jg = [np.asfortranarray(Jgup[gi][d].a) for d in range(ndim)] + [None] * (3 - ndim)
        s.setMetricFull(q, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return dom, grids, fac, s


@pytest.mark.parametrize("ndim,n,bs,per,L", [(3, (16, 16, 16), 16, (True, True, True), (1.0, 1.0, 1.0)),   # [4096, 512, 64]
                                             (2, (32, 32), 16, (False, False), (2.0, 1.0))])
def test_full_metric_w_cycle_and_solve(oracle, F, ndim, n, bs, per, L):
    so = oracle
    ghost = (1, 1, 1) if ndim == 3 else (1, 1, 0)
    dom, grids, fac, gpu = _full_setup(so, n, bs, per, L, ndim, 2)
    try:
        amr = so.AMRMultiGrid(fac, so.BiCGStab())
        amr.numMG = 2
        amr.mg.cycle_type = 2
        assert gpu.depth() == amr.mg.depth and gpu.depth() >= 3
        assert all(c <= ORDERED_DEFAULT for c in _cells(gpu))    # serial sums on every depth: bit-exact
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
        phi0 = so.random_field(grids, 3, ghost, dom.box)
        b_ = so.LevelData(grids, 1)
        amr.op.apply_op(b_, phi0, True)
        x = so.LevelData(grids, 1, ghost)
        amr.solve(x, b_)
        gx = [np.zeros(f.a.shape[:3], order="F") for f in x.fabs]
        gb = [np.asfortranarray(f.a[..., 0]) for f in b_.fabs]
        st = gpu.solve(gx, gb, 0, 0, True, False, phi_ghost=ghost)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        np.testing.assert_allclose(st["history"], amr.history, rtol=1e-9, atol=1e-12 * amr.history[0])   # test_gpu_full
        assert st["history"][-1] <= 1e-6 * st["history"][0]
    finally:
        gpu.undefine()


# ---- AMR -------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["twopass", "fused"])
def sweep_kernel(request, monkeypatch):
    monkeypatch.setenv("SOMAR_FUSED_MIN_CELLS", "0" if request.param == "fused" else "1000000000000")
    return request.param


@pytest.fixture(params=["lean", "plain"])
def amr_path(request, monkeypatch):
    """AMRSolver::vcycle's lean path (implicit zeros, residual ping-pong, per-level visit counts) or the plain one"""
    if request.param == "plain":
        monkeypatch.setenv("SOMAR_AMR_PLAIN", "1")
    else:
        monkeypatch.delenv("SOMAR_AMR_PLAIN", raising=False)
    return request.param


def _levels(so, am, layout):
    periodic, ratios, boxes = layout
    fb = [[so.Box(lo, hi) for lo, hi in lev] for lev in boxes]
    return make_amr_levels(so, am, (16, 16, 8), (2.0, 1.0, 0.5), periodic, ratios, fb), ratios


_AMR = {}   # (layout, lmax, lbase, numMG) -> the oracle's AMRVCycle


def _amr_cycle(so, am, case, numMG):
    layout, lmax, lbase = case
    key = (repr(case), numMG)
    if key not in _AMR:
        levels, ratios = _levels(so, am, layout)
        comp = am.AMRComposite(levels, ratios, so.BCHolder(), so.BiCGStab())
        comp.numMG = numMG
        phi = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        res = [so.random_field(L.grids, 70 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
        for l in range(lbase, lmax):
            comp.zero_covered(l, res[l])
        comp.init(phi, res, lmax, lbase)
        comp.set_bottom_solver(lmax, lbase)
        corr = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.amr_vcycle(corr, res, lmax, lmax, lbase)
        _AMR[key] = (levels, ratios, res, [[np.array(a) for a in valid_of(c)] for c in corr],
                     [m.depth for m in comp.mg], [m.maxForcedDepth for m in comp.mg])
    return _AMR[key]


# test_gpu_amr's VCYCLES less (LAYOUTS[3], 1, 1), where l_max == l_base and the one-depth level cycle has nothing to revisit
AMR_CASES = VCYCLES[:4] + [(LAYOUTS[5], 1, 0), (LAYOUTS[6], 1, 0), (LAYOUTS[7], 2, 0), (LAYOUTS[7], 2, 1)]


@pytest.mark.parametrize("case,numMG", [(c, 2) for c in AMR_CASES] + [(VCYCLES[2], 3), (AMR_CASES[-2], 3)])
def test_amr_w_cycle_bit_exact(oracle, am, case, numMG, sweep_kernel, amr_path, F):
    """one AMRVCycle with numMG recursions per level (the standalone cycle: the level solvers got numMG at define).  Two
    and three AMR levels, l_base 0 and 1, ratio-4 levels whose relaxation is a mini V-cycle over their forced depth (run
    numMG times per level visit).  The cycle's only sums (the base level's mean removal and BiCGStab) run on the base
    level's depths, all of at most 4096 cells: serial order, bit-exact."""
    so = oracle
    layout, lmax, lbase = case
    levels, ratios, res, want, depths, forced = _amr_cycle(so, am, case, numMG)
    gpu = make_gpu_amr(levels, ratios, numMG=numMG)
    try:
        base = gpu.levels[lbase]
        assert all(c <= ORDERED_DEFAULT for c in _cells(base)) and lmax > lbase
        for l in range(lbase + 1, lmax + 1):
            if max(ratios[l - 1]) > 2:     # a mini V-cycle: at least one forced depth below the level
                assert forced[l] >= 1 and gpu.levels[l].depth() >= 2
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RES, res[l])
            v.setVal(F.F_CORR, 0.0)
        gpu.vcycleAMR(lmax, lbase)
        for l in range(lbase, lmax + 1):
            for g, w in zip(download_valid(gpu.levels[l], F.F_CORR, levels[l].grids), want[l]):
                np.testing.assert_array_equal(g, w)
    finally:
        gpu.undefine()


_AMR_SOLVES = {}


@pytest.mark.parametrize("layout", LAYOUTS[:4] + RATIO4)
def test_amr_w_solve_history(oracle, am, layout, amr_path):
    from somar_amd import api as F
    so = oracle
    levels, ratios = _levels(so, am, layout)
    lmax = len(levels) - 1
    key = repr(layout)
    if key not in _AMR_SOLVES:
        comp = am.AMRComposite(levels, ratios, so.BCHolder(), so.BiCGStab())
        comp.numMG = 2
        phi = [so.random_field(L.grids, 5 + l, (1, 1, 1), L.domain.box) for l, L in enumerate(levels)]
        zero = [so.LevelData(L.grids, 1) for L in levels]
        rhs = [so.LevelData(L.grids, 1) for L in levels]
        comp.init(phi, zero, lmax, 0)
        comp.compute_amr_residual(rhs, phi, zero, lmax, 0, True)
        for r in rhs:
            so.ld_scale(r, -1.0)
        sol = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.solve(sol, rhs, lmax, 0)
        _AMR_SOLVES[key] = (rhs, [[np.array(x) for x in valid_of(s_)] for s_ in sol], comp.iters, comp.exitStatus,
                            list(comp.history))
    rhs, sol, iters, exit_status, history = _AMR_SOLVES[key]
    gpu = make_gpu_amr(levels, ratios, numMG=2)
    try:
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RHS, rhs[l])
        st = gpu.solveAMR(lmax, 0)
        assert st["iters"] == iters and st["exitStatus"] == exit_status
        np.testing.assert_allclose(st["history"], history, rtol=1e-10, atol=0.0)
        for l in range(lmax + 1):
            assert max_rel_diff(download_valid(gpu.levels[l], F.F_PHI, levels[l].grids), sol[l]) < 1e-8
    finally:
        gpu.undefine()


def test_amr_w_cycle_and_solve_nondiagonal(oracle, am, F):
    """the 19-point operator on two AMR levels (tests/test_gpu_amr_full.py's 3-D two-level layout)"""
    so = oracle
    levels = make_full_amr_levels(so, am, (16, 16, 8), (2.0, 1.0, 0.5), (False, False, False), [(2, 2, 2)],
                                  [[so.Box((8, 8, 4), (23, 23, 11))]], cbox=8)
    ratios = [(2, 2, 2)]
    comp = am.AMRComposite(levels, ratios, so.BCHolder(), so.BiCGStab(), isDiagonal=False)
    comp.numMG = 2
    phi = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
    res = [so.random_field(L.grids, 70 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
    comp.zero_covered(0, res[0])
    comp.init(phi, res, 1, 0)
    comp.set_bottom_solver(1, 0)
    corr = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
    comp.amr_vcycle(corr, res, 1, 1, 0)
    gpu = make_gpu_amr(levels, ratios, full=True, numMG=2)
    try:
        assert gpu.levels[0].depth() >= 2 and all(c <= ORDERED_DEFAULT for c in _cells(gpu.levels[0]))
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RES, res[l])
            v.setVal(F.F_CORR, 0.0)
        gpu.vcycleAMR(1, 0)
        for l in (0, 1):
            for g, w in zip(download_valid(gpu.levels[l], F.F_CORR, levels[l].grids), valid_of(corr[l])):
                np.testing.assert_array_equal(g, w)
        zero = [so.LevelData(L.grids, 1) for L in levels]
        rhs = [so.LevelData(L.grids, 1) for L in levels]
        src = [so.random_field(L.grids, 5 + l, (1, 1, 1), L.domain.box) for l, L in enumerate(levels)]
        comp.init(src, zero, 1, 0)
        comp.compute_amr_residual(rhs, src, zero, 1, 0, True)
        for r in rhs:
            so.ld_scale(r, -1.0)
        sol = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.solve(sol, rhs, 1, 0)
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RHS, rhs[l])
        st = gpu.solveAMR(1, 0)
        assert st["iters"] == comp.iters and st["exitStatus"] == comp.exitStatus
        np.testing.assert_allclose(st["history"], comp.history, rtol=1e-10, atol=0.0)
    finally:
        gpu.undefine()


def test_amr_leptic_w_solve(oracle, am):
    """AMRLepticSolver with numMG = 2: the composite cycle recurses twice into the base level (somar_leptic.py's
    amr_vcycle loop, AMRLepticSolver.cpp's AMRVCycle); tests/test_gpu_amr_leptic.py's cartesian case, base level handed
    the restricted residual"""
    from oracle import somar_leptic as sl
    from somar_amd import api as F
    so = oracle
    H = 0.005
    ratios = [(2, 2, 1)]
    fine = [[so.Box((16, 16, 0), (31, 47, 7)), so.Box((32, 16, 0), (47, 47, 7))]]
    levels = make_amr_levels(so, am, (32, 32, 8), (1.0, 1.0, H), (False, False, False), ratios, fine, variant="cartesian",
                             cbox=(16, 16, 8))
    iters = 3
    amr = sl.AMRLepticSolver(levels, ratios, so.BCHolder(), leptic=dict(maxOrder=3, domainHeight=H), baseFromRestricted=True)
    amr.iterMax = iters
    amr.numMG = 2
    phi = [so.random_field(Lv.grids, 5 + l, (1, 1, 1), Lv.domain.box) for l, Lv in enumerate(levels)]
    zero = [so.LevelData(Lv.grids, 1) for Lv in levels]
    rhs = [so.LevelData(Lv.grids, 1) for Lv in levels]
    amr.init(phi, zero, 1, 0)
    amr.compute_amr_residual(rhs, phi, zero, 1, 0, True)
    for r in rhs:
        so.ld_scale(r, -1.0)
    sol = [so.LevelData(Lv.grids, 1, (1, 1, 1)) for Lv in levels]
    amr.solve(sol, rhs, 1, 0)
    gpu = make_gpu_amr(levels, ratios, imax=iters, numMG=2)
    lp = F.LepticParams()
    F._ck(F.lib().somar_leptic_params_default(lp))
    lp.max_order, lp.domain_height = 3, H
    gpu.enableLeptic(lp, baseFromRestricted=True)
    try:
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RHS, rhs[l])
        st = gpu.solveAMRLeptic(1, 0)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        h = np.array(amr.history)
        np.testing.assert_allclose(st["history"], h, rtol=0, atol=1e-10 * h[0])
        for l in (0, 1):
            ls, lep = gpu.lepticStats(l), amr.leptic[l]
            assert ls["exitStatus"] == lep.exitStatus and ls["horizSolves"] == lep.horizSolves
            want = valid_of(sol[l])
            scale = max(float(np.max(np.abs(w))) for w in want)
            for g_, w_ in zip(download_valid(gpu.levels[l], F.F_PHI, levels[l].grids), want):
                np.testing.assert_allclose(g_, w_, rtol=0, atol=1e-8 * scale)
    finally:
        gpu.undefine()


# ---- two ranks on one GPU --------------------------------------------------------------------------------------------
def _worker(rank, nranks, name, mode, q):
    try:
        os.environ["SOMAR_FUSED_MIN_CELLS"] = "0" if mode == "fused" else "1000000000000"
        # "fused": depth 1 on is agglomerated (replicated on both ranks): its second visit gathers a non-zero correction
        # into the replicated tail (agglom_cycle); "twopass": every depth stays sharded
        if mode == "twopass":
            os.environ["SOMAR_AGGLOM_CELLS"] = "0"
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, here)
        sys.path.insert(0, os.path.dirname(here))
        from oracle import somar_oracle as so
        from oracle import somar_amr as am
        from somar_amd import AMRPressureSolver
        from somar_amd import api as F
        from helpers import download_valid, make_amr_levels, make_gpu_solver, make_oracle_solver, make_problem, upload, valid_of
        comm = F.comm_create_shm(name, rank, nranks)

        # ---- single level: a W solve (8 boxes dealt round-robin) ----
        dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 32, 32), 16, "stretched", (False, True, False), (2.0, 1.0, 1.0))
        owner = [i % nranks for i in range(len(grids))]
        amr = make_oracle_solver(so, dom, grids, dx, Jgup, Jinv)
        amr.numMG = 2
        amr.mg.cycle_type = 2

        class Mine:
            def __init__(self, x):
                self.x = x

            def __getitem__(self, gi):
                assert owner[gi] == rank
                return self.x[gi]

        gpu = make_gpu_solver(dom, grids, dx, Mine(Jgup), Mine(Jinv), owner=owner, comm=comm, numMG=2)
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

        # ---- two AMR levels, both sharded: one W-cycle ----
        periodic, ratios = (True, False, False), [(2, 2, 1)]
        fb = [[so.Box((0, 8, 0), (15, 23, 7)), so.Box((24, 8, 0), (31, 23, 7))]]
        levels = make_amr_levels(so, am, (16, 16, 8), (2.0, 1.0, 0.5), periodic, ratios, fb)
        comp = am.AMRComposite(levels, ratios, so.BCHolder(), so.BiCGStab())
        comp.numMG = 2
        owners = [[i % nranks for i in range(len(L.grids))] for L in levels]
        owners[1] = [(i + 1) % nranks for i in range(len(levels[1].grids))]
        s = AMRPressureSolver()
        p = s._p
        s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, 2, p.hang,
                             p.norm_thresh, 0)
        L0 = levels[0]
        s.defineAMR(L0.domain.box.lo, L0.domain.box.hi, L0.domain.periodic, L0.dx, ratios,
                    [[(g.lo, g.hi) for g in L.grids] for L in levels], owners_per_level=owners, comm=comm)
        for L, v in zip(levels, s.levels):
            for p_ in range(v.num_local_patches):
                _, _, gi = v.patch_box(p_)
                jg = [np.asfortranarray(L.Jgup[gi][d].a[..., d]) for d in range(3)]
                v.setMetricOrtho(p_, jg[0], jg[1], jg[2], np.asfortranarray(L.Jinv[gi].a[..., 0]))
        s.finalize()
        res = [so.random_field(L.grids, 70 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
        comp.zero_covered(0, res[0])
        zero = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.init(zero, res, 1, 0)
        comp.set_bottom_solver(1, 0)
        corr = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        for l, v in enumerate(s.levels):
            upload(v, F.F_RES, res[l])
            v.setVal(F.F_CORR, 0.0)
        comp.amr_vcycle(corr, res, 1, 1, 0)
        s.vcycleAMR(1, 0)
        for l in (0, 1):
            n = 0
            for g, w in zip(download_valid(s.levels[l], F.F_CORR, levels[l].grids), valid_of(corr[l])):
                if g is not None:
                    np.testing.assert_allclose(g, w, rtol=0, atol=1e-10 * float(np.max(np.abs(w))))
                    n += 1
            assert n > 0 or len(levels[l].grids) < nranks
        s.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("mode", ["fused", "twopass"])
def test_w_cycles_on_two_ranks(mode):
    nranks = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/somar_%s" % uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=_worker, args=(r, nranks, name, mode, q)) for r in range(nranks)]
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
