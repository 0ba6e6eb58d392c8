"""The workgroup-local instantiation of k_box_bicgstab -- the BiCGStab bottom solve of a level of ONE box with p~ / s~, the
sums and every barrier inside the workgroup (LDS, __syncthreads) -- against PressureSolver::bottom_solve's launch-by-launch
path (SOMAR_BOX_BOTTOM=0, SOMAR_FUSED_BOTTOM_MAX_CELLS=0) and the oracle's restatement of Chombo's BiCGStabSolver.

Serial-order sums on both GPU paths (SOMAR_ORDERED_REDUCE_MAX covers the level), so they agree BIT FOR BIT: iteration count,
exit code, solution, a second solve from a non-zero guess, a whole V-cycle.  Also here: the host no longer waits for the
bottom solve's (iterations, exit code) before it enqueues the up leg of a graph-replayed cycle (SOMAR_BOTTOM_ASYNC=0 restores
the wait), and the zero-average prolongation's ordered sums on levels of 512 to 13824 cells in one to eight boxes."""
import numpy as np
import pytest

from helpers import download_valid, make_oracle_solver, make_problem, max_rel_diff, upload, valid_of

pytestmark = pytest.mark.gpu

ORDERED_ALL = "1000000"
LAUNCH_ENV = dict(SOMAR_BOX_BOTTOM="0", SOMAR_FUSED_BOTTOM_MAX_CELLS="0")
SWITCHES = ("SOMAR_BOX_BOTTOM", "SOMAR_FUSED_BOTTOM_MAX_CELLS", "SOMAR_BOX_BOTTOM_MIN_CELLS", "SOMAR_GRAPH_CELLS",
            "SOMAR_BOTTOM_ASYNC", "SOMAR_ORDERED_REDUCE_MAX")


@pytest.fixture(scope="module")
def F():
    from somar_amd import api
    return api


class Case:
    def __init__(self, n, periodic=(False, False, False), L=(1.0, 1.0, 1.0), maxDepth=0, variant="stretched", ndim=3,
                 alpha=0.0, beta=1.0, bottom=None, precond=None, cells=None):
        self.n, self.periodic, self.L, self.maxDepth, self.variant, self.ndim = n, periodic, L, maxDepth, variant, ndim
        self.alpha, self.beta = alpha, beta
        self.bottom = bottom or {}     # BiCGStab parameters that differ from the deck's
        self.precond = precond         # (precondMode, num_smooth_precond) or None: the deck's
        self.cells = cells             # cells of the bottom level (checked)

    def __repr__(self):
        s = "x".join(str(a) for a in self.n) + "".join("p" if q else "" for q in self.periodic)
        if self.maxDepth != 0:
            s += "-to-%d" % self.cells
        if self.ndim == 2:
            s += "-2d"
        if self.alpha != 0.0:
            s += "-helmholtz"
        if self.precond is not None:
            s += "-pc%d_%d" % self.precond
        return s + "".join("-%s%g" % kv for kv in sorted(self.bottom.items()))


LAYOUTS = [
    Case((2, 2, 2), cells=8),                                                        # fewer cells than lanes
    Case((3, 3, 3), cells=27),                                                       # ... with an interior cell
    Case((2, 2, 8), L=(1.0, 1.0, 2.0), cells=32),                                    # narrow in two directions only
    Case((16, 16, 16), maxDepth=-1, cells=64),                                       # one wavefront: 4^3 reached from 16^3
    Case((8, 8, 8), cells=512),                                                      # one cell per thread
    Case((8, 12, 10), L=(1.0, 2.0, 1.0), cells=960),                                 # two cells per thread
    Case((16, 16, 8), variant="cartesian", cells=2048),                              # four cells per thread
    Case((12, 20, 4), L=(1.0, 1.0, 3.0), cells=960),                                 # non-cubic
    Case((8, 12, 10), periodic=(False, True, False), cells=960),                     # the box is its own neighbour in y
    Case((32, 32, 32), periodic=(True, True, True), maxDepth=-1, cells=64),          # ... in every direction; 4^3 from 32^3
    Case((12, 10), periodic=(True, False), L=(2.0, 1.0), ndim=2, cells=120),         # 2-D level
    Case((8, 12, 10), alpha=1.0, beta=-0.05, cells=960),                             # Helmholtz: no null space
]
BRANCHES = [Case((8, 12, 10), bottom=dict(normType=nt), cells=960) for nt in (0, 1, 2)] + \
           [Case((8, 12, 10), precond=pc, cells=960) for pc in ((-1, 1), (0, 0), (0, 1), (0, 3))] + \
           [Case((8, 12, 10), bottom=dict(imax=3), cells=960)]
# stagnation: with hang = 0.9 an iteration that does not cut the residual tenfold counts as hung; every second such iteration
# restarts, and the restart after the last allowed one leaves with exit code 3
RESTART = Case((8, 12, 10), bottom=dict(hang=0.9, numRestarts=1), precond=(-1, 1), cells=960)


def _problem(so, case):
    if case.ndim == 2:
        n, per, L = case.n, case.periodic, case.L
        dom = so.Domain(so.Box((0, 0, 0), (n[0] - 1, n[1] - 1, 0)), tuple(per) + (False,))
        grids = so.split_domain(dom.box, tuple(n) + (1,))
        dx = (L[0] / n[0], L[1] / n[1], 1.0)
        Jgup, Jinv = so.make_diagonal_metric(grids, dx, tuple(L) + (1.0,), 2, case.variant, domain=dom)
        return dom, grids, dx, Jgup, Jinv
    return make_problem(so, case.n, case.n, case.variant, case.periodic, case.L)


def _oracle(so, case, prob):
    kw = dict(maxDepth=case.maxDepth, ndim=case.ndim)
    if case.precond is not None:
        kw.update(precondMode=case.precond[0], precondIters=case.precond[1])
    return make_oracle_solver(so, *prob, alpha=case.alpha, beta=case.beta, **kw)


def _gpu(case, prob, env, monkeypatch):
    """a solver created under `env` (the switches are read at construction); every other switch at its default"""
    from somar_amd import AMRPressureSolver
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    dom, grids, dx, Jgup, Jinv = prob
    s = AMRPressureSolver()
    p = s._p
    s.setSpaceDim(case.ndim)
    mode, k = case.precond if case.precond is not None else (p.precond_mode, p.num_smooth_precond)
    s.setAMRMGParameters(p.imin, p.imax, p.eps, case.maxDepth, k, 2, 2, 2, mode, 1, p.num_mg, p.hang, p.norm_thresh, 0)
    b = case.bottom
    s.setBottomParameters(b.get("imax", p.bottom_imax), b.get("numRestarts", p.bottom_num_restarts), p.bottom_eps,
                          p.bottom_reps, b.get("hang", p.bottom_hang), p.bottom_small, b.get("normType", p.bottom_norm_type), 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=case.alpha, beta=case.beta)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        jg = [np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(case.ndim)] + [None] * (3 - case.ndim)
        s.setMetricOrtho(q, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return s


def _bottom_rhs(so, case, opb):
    rhs = so.random_field(opb.grids, 91, (0, 0, 0), opb.domain.box)
    if case.alpha == 0.0:
        so.remove_weighted_mean(rhs, opb.Jinv)
    return rhs


def _oracle_bottom(so, case, opb, rhs):
    bs = so.BiCGStab(**case.bottom)
    bs.define(opb, True)
    phi = so.LevelData(opb.grids, 1, (1, 1, 1))
    bs.solve(phi, rhs)
    return bs.iters, bs.exitStatus, valid_of(phi)


def _both_paths(so, F, case, monkeypatch):
    """-> {False: launch path, True: LOCAL kernel}: (iters, exit, solution), (iters, exit of a second solve, its solution,
    one V-cycle's correction); and the oracle's bottom solve"""
    prob = _problem(so, case)
    dom, grids = prob[0], prob[1]
    amr = _oracle(so, case, prob)
    D = amr.mg.depth
    opb = amr.mg.ops[-1]
    assert len(opb.grids) == 1 and opb.grids[0].numPts() == case.cells
    rhs = _bottom_rhs(so, case, opb)
    res = so.random_field(grids, 92, (0, 0, 0), dom.box)
    if case.alpha == 0.0:
        so.remove_weighted_mean(res, amr.op.Jinv)
    fp, fr = (F.FIELD(D - 1, F.F_CORR), F.FIELD(D - 1, F.F_RES)) if D > 1 else (F.F_CORR, F.F_RES)
    out = {}
    for local in (False, True):
        env = dict(SOMAR_ORDERED_REDUCE_MAX=ORDERED_ALL)
        if not local:
            env.update(LAUNCH_ENV)
        gpu = _gpu(case, prob, env, monkeypatch)
        try:
            assert gpu.depth() == D
            upload(gpu, fr, rhs, depth=D - 1)
            gpu.setVal(fp, 0.0)
            it, ex = gpu.bottomSolve(fp, fr)
            assert gpu.bottomKind() == (2 if local else 0)
            first = (it, ex, download_valid(gpu, fp, opb.grids, D - 1))
            it2, ex2 = gpu.bottomSolve(fp, fr)                      # from the first one's answer: a non-zero guess
            again = download_valid(gpu, fp, opb.grids, D - 1)
            upload(gpu, F.F_RES, res)
            gpu.setVal(F.F_CORR, 0.0)
            gpu.vcycle(F.F_CORR, F.F_RES)
            assert gpu.bottomKind() == (2 if local else 0)
            out[local] = (first, (it2, ex2, again, download_valid(gpu, F.F_CORR, grids)))
        finally:
            gpu.undefine()
    return out, _oracle_bottom(so, case, opb, rhs)


def _same(a_list, b_list):
    for a, b in zip(a_list, b_list):
        np.testing.assert_array_equal(a, b)


def _check_equal(out, want):
    (f0, s0), (f1, s1) = out[False], out[True]
    print("launch path", f0[:2], s0[:2], "local kernel", f1[:2], s1[:2], "oracle", want[:2])
    assert f0[:2] == f1[:2]
    _same(f0[2], f1[2])
    assert s0[:2] == s1[:2]
    _same(s0[2], s1[2])
    _same(s0[3], s1[3])
    assert f1[:2] == want[:2]
    _same(f1[2], want[2])          # the oracle's sums and the kernel's run in the same order: same bits


@pytest.mark.parametrize("case", LAYOUTS + BRANCHES, ids=repr)
def test_local_bottom_solver_equals_the_launch_path_and_the_oracle(oracle, F, case, monkeypatch):
    """(2x2x2, 2x2x8: a domain at most two cells wide in two directions, where the reference's LevelGSRB has no cell to
    visit -- every shell of the domain shrunk by one cell is empty -- and the preconditioner is its diagonal scaling alone)"""
    out, want = _both_paths(oracle, F, case, monkeypatch)
    _check_equal(out, want)
    if "imax" in case.bottom:
        assert out[False][0][0] == case.bottom["imax"]     # stopped by the iteration limit


def test_local_bottom_solver_takes_the_restart_branch(oracle, F, monkeypatch):
    out, want = _both_paths(oracle, F, RESTART, monkeypatch)
    # exit code 3 is only reached from the restart branch, after numRestarts restarts have been taken
    assert out[False][0][1] == 3 and RESTART.bottom["numRestarts"] >= 1
    _check_equal(out, want)


def test_local_bottom_solver_with_tree_sums(oracle, F, monkeypatch):
    """Below the level's size SOMAR_ORDERED_REDUCE_MAX switches the kernel's sums to its fixed tree: the same solve as the
    oracle's up to the rounding of the dot products (the bounds of test_tree_sums_above_the_ordered_limit)."""
    so = oracle
    case = Case((16, 16, 8), variant="cartesian", cells=2048)
    assert case.cells > 1024
    prob = _problem(so, case)
    amr = _oracle(so, case, prob)
    opb = amr.mg.ops[-1]
    rhs = _bottom_rhs(so, case, opb)
    bit, bex, bsol = _oracle_bottom(so, case, opb, rhs)
    gpu = _gpu(case, prob, dict(SOMAR_ORDERED_REDUCE_MAX="1024"), monkeypatch)
    try:
        gpu.upload(F.F_RES, 0, np.asfortranarray(rhs[0].a[..., 0]), rhs.ghost)
        gpu.setVal(F.F_CORR, 0.0)
        it, ex = gpu.bottomSolve(F.F_CORR, F.F_RES)
        assert gpu.bottomKind() == 2
        sol = download_valid(gpu, F.F_CORR, opb.grids)
    finally:
        gpu.undefine()
    print("tree sums", it, ex, "oracle", bit, bex, "difference", max_rel_diff(sol, bsol))
    assert ex == bex and abs(it - bit) <= 1, (it, ex, bit, bex)
    assert max_rel_diff(sol, bsol) < 2e-4


def test_multi_box_tiny_bottom_keeps_the_single_workgroup_kernel(oracle, F, monkeypatch):
    """a bottom of 8 boxes of 4^3 under the default environment: k_tiny_bicgstab (kind 1)"""
    so = oracle
    case = Case((32, 32, 32), maxDepth=-1)
    prob = make_problem(so, (32, 32, 32), 16, "stretched", (False, False, False), (1.0, 1.0, 1.0))
    gpu = _gpu(case, prob, {}, monkeypatch)
    try:
        D = gpu.depth()
        fp, fr = F.FIELD(D - 1, F.F_CORR), F.FIELD(D - 1, F.F_RES)
        gpu.fillHash(fr, 77)
        gpu.removeMean(fr)
        gpu.setVal(fp, 0.0)
        gpu.bottomSolve(fp, fr)
        assert gpu.bottomKind() == 1
    finally:
        gpu.undefine()


def test_graph_cycle_without_the_host_wait(oracle, F, monkeypatch):
    """32^3 in one box, stretched: vcycleFromZero replays the coarse legs as graphs around the bottom solve and reads the
    solve's (iterations, exit code) only after the up leg is enqueued.  Same correction, bit for bit, as without graphs and
    as with the wait restored; what bottomSolve reports afterwards equals the launch path's."""
    so = oracle
    case = Case((32, 32, 32), maxDepth=-1, cells=64)
    prob = _problem(so, case)
    dom, grids = prob[0], prob[1]
    amr = _oracle(so, case, prob)
    D = amr.mg.depth
    opb = amr.mg.ops[-1]
    res = so.random_field(grids, 92, (0, 0, 0), dom.box)
    so.remove_weighted_mean(res, amr.op.Jinv)
    rhs = _bottom_rhs(so, case, opb)
    fp, fr = F.FIELD(D - 1, F.F_CORR), F.FIELD(D - 1, F.F_RES)
    envs = {"graphs": {}, "no graphs": dict(SOMAR_GRAPH_CELLS="0"), "wait restored": dict(SOMAR_BOTTOM_ASYNC="0"),
            "launch path": LAUNCH_ENV}
    got = {}
    for name, env in envs.items():
        gpu = _gpu(case, prob, env, monkeypatch)
        try:
            upload(gpu, F.F_RES, res)
            gpu.vcycleFromZero(F.F_CORR, F.F_RES)
            kind = gpu.bottomKind()
            corr = download_valid(gpu, F.F_CORR, grids)
            gpu.vcycleFromZero(F.F_CORR, F.F_RES)       # the replay (the first call captured the graphs)
            again = download_valid(gpu, F.F_CORR, grids)
            upload(gpu, fr, rhs, depth=D - 1)
            gpu.setVal(fp, 0.0)
            got[name] = (kind, corr, again, gpu.bottomSolve(fp, fr))
        finally:
            gpu.undefine()
    assert got["launch path"][0] == 0
    for name in ("graphs", "no graphs", "wait restored"):
        kind, corr, again, status = got[name]
        assert kind == 2, name
        _same(corr, got["graphs"][1])
        _same(again, got["graphs"][1])
        assert status == got["launch path"][3], name
    # (the launch path sums the 32^3 level's zero-average mean by the same tree: the whole cycle agrees too)
    _same(got["launch path"][1], got["graphs"][1])


# (n, boxsz, L, cells of the levels the prolongation writes, finest first).  The sums stage 2048 terms of the level's one
# sequence at a time: a whole number of chunks, a partial chunk after full ones, a single partial chunk, box ends inside a chunk
PROLONG = {
    "one-16^3-box": ((16, 16, 16), 16, (1.0, 1.0, 1.0), [4096, 512]),
    "eight-8^3-boxes": ((16, 16, 16), 8, (1.0, 1.0, 1.0), [4096]),
    "12x16x12-semicoarsened": ((12, 16, 12), (12, 16, 12), (1.0, 0.4, 1.0), [2304]),               # 2048 + 256
    "20x16x12-semicoarsened-twice": ((20, 16, 12), (20, 16, 12), (1.0, 0.3, 1.0), [3840, 1920]),   # 2048 + 1792; 1920 alone
    "24^3": ((24, 24, 24), 24, (1.0, 1.0, 1.0), [13824]),                                          # 6 x 2048 + 1536
    "six-24x8x8-boxes": ((24, 16, 24), (24, 8, 8), (1.0, 1.0, 1.0), [9216]),                       # box ends at 1536, 3072, ...
    # a level of 15 x 16 x 17 = 4080 cells has no coarser level (the coarsening needs every box a multiple of 4 wide, of 8
    # where it coarsens): one level, no prolongation -- kept as the plain V-cycle check of such a level
    "15x16x17": ((15, 16, 17), (15, 16, 17), (1.0, 1.0, 1.0), []),
}


@pytest.mark.parametrize("name", list(PROLONG))
def test_prolongation_sums_on_ordered_levels(oracle, F, name, monkeypatch):
    """the zero-average prolongation's sums run in the reference's serial order (SOMAR_ORDERED_REDUCE_MAX covers every
    level): one V-cycle equals the oracle's bit for bit.  Every level but the coarsest is a prolongation target with a null
    space (zeroAvg); its cell count is checked.  (A target's boxes are multiples of 4 wide, so its cell count is a multiple
    of 16 and the staged walk's scalar tail is not reachable through a cycle.)"""
    so = oracle
    n, boxsz, L, targets = PROLONG[name]
    case = Case(n, maxDepth=-1)
    prob = make_problem(so, n, boxsz, "stretched", (False, False, False), L)
    dom, grids = prob[0], prob[1]
    amr = _oracle(so, case, prob)
    assert [sum(g.numPts() for g in op.grids) for op in amr.mg.ops[:-1]] == targets
    assert all(op.zeroAvg for op in amr.mg.ops[:-1])
    res = so.random_field(grids, 92, (0, 0, 0), dom.box)
    so.remove_weighted_mean(res, amr.op.Jinv)
    corr = so.LevelData(grids, 1, (1, 1, 1))
    amr.mg.init(corr, res)
    amr.mg.bottomSolver = so.BiCGStab()
    amr.mg.bottomSolver.define(amr.mg.ops[-1], True)
    amr.mg.one_cycle(corr, res)
    gpu = _gpu(case, prob, dict(SOMAR_ORDERED_REDUCE_MAX=ORDERED_ALL), monkeypatch)
    try:
        assert gpu.depth() == amr.mg.depth == len(targets) + 1
        assert not targets or gpu.depth() >= 2
        upload(gpu, F.F_RES, res)
        gpu.setVal(F.F_CORR, 0.0)
        gpu.vcycle(F.F_CORR, F.F_RES)
        _same(download_valid(gpu, F.F_CORR, grids), valid_of(corr))
    finally:
        gpu.undefine()
