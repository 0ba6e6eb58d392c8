"""Tall tiles of the fused 7-point sweep (somar_amd/csrc/march_plan.h): on a level whose metric is not uniform and whose boxes
are even and wider than 128 cells, every tile of the sweep's table is lane class 1 -- two region rows of 64 columns per
wavefront, 60 x 28 outputs -- and the one-body class-1 instantiations of k_gsrb_fused run (gsrb_fused.hip, NARROW = 2).  The
sweep is pointwise arithmetic on the same values, so the fields must not move by a bit: every case runs with the default
tables and with SOMAR_NO_NARROW_TILES=1 (today's equal class-0 columns) and compares the two with array_equal, and where the
oracle can be met bit for bit (serial-order sums over every level) it is.

Shapes: the smallest at which the new paths can go wrong, about 90 K cells.  A 136-wide box gets three columns 46 / 46 / 44;
40 rows are two tile rows 28 + 12, 28 rows exactly one; 16 planes are four k-chunks (tests/test_march_plan.py pins this plan
on the CPU; the library exports no tile table, so here each case asserts the rule's inputs instead: box widths, the metric
flag, the switches the solver holds).

What cannot be shown here: that the tall table and the NARROW = 2 kernels really ran.  Both tables give the same bits by design
and the library may export nothing new (tests/test_capi_exports.py pins the exports), so if the rule quietly evaluated to false
every test of this file would still pass.  assert_tall_rule checks the rule's inputs; that the path engages on such levels is on
record only in the kernel trace and counters of profiles/r11_tall_tiles.md (grids of 760 and 250 workgroups, kernel names).

The sweep's input modes, and the two V-cycles each case runs against the oracle:
  * SOMAR_ORDERED_REDUCE_MAX above every depth: every sum in the reference's serial order, so the oracle is met BIT FOR BIT.
    PressureSolver::fold_prolong is then off (ordered depth): the first up-sweep takes the deferred mean, mode 2 -- modes 1, 0, 2
    (1 and 0 with Dirichlet sides, where there is no mean);
  * SOMAR_ORDERED_REDUCE_MAX = 50000, between depth 0 (87040 or 60928 cells) and every coarser depth (at most 43520): depth 0
    folds prolongation and mean removal into its first up-sweep, mode 4 (mode 3 with Dirichlet sides) -- modes 1, 0, 4 -- and its
    mean is the one tree sum of the cycle, taken AFTER everything below has run in serial order.  The oracle is met to the
    project's tree-sum tolerance, 1e-12 of the correction's scale per box (tests/test_gpu_wcycle.py, test_gpu_amr_wide.py): a
    mean of 9e4 terms summed in another order moves by a few 1e-16 of the scale, and two contracting sweeps follow.
A second cycle on top of the first would start from a non-zero correction, i.e. run mode 0 where the first runs mode 1: nothing
these two do not run.  The default limit (4096) is NOT compared with the oracle: these hierarchies are two depths deep (the
stretched, anisotropic box semicoarsens once), the bottom level has 21760-43520 cells, and BiCGStab with tree-summed dot
products on a singular system that size turns last-bit differences into 4e-6 to 6e-5 of the scale -- with either table, with
and without graph replay, with and without the fold (measured: the same figures to four digits), and not with Dirichlet sides
(3e-15).  The fp32 cycle needs depth 0 above the sum limit and outside graph replay; the AMR level has coarse-fine faces, so
its prolongation is never folded (modes 1, 0, 2)."""
import multiprocessing as mp
import os
import traceback
import uuid

import numpy as np
import pytest

from tests.helpers import download_valid, make_amr_levels, make_gpu_amr, upload, valid_of

pytestmark = pytest.mark.gpu

D = 1                        # BC_DIRI
ORDERED_ALL = "1000000"      # above every level here: every sum in the reference's serial order
ORDERED_BELOW_TOP = "50000"  # depth 0 above it (tree-summed mean, folded prolongation), every coarser depth in serial order
TREE_SUM_TOL = 1e-12         # of the correction's scale: the project's bound where one tree-summed mean intervenes
TABLES = (("tall", None), ("equal", "1"))   # SOMAR_NO_NARROW_TILES


class Case:
    def __init__(self, name, n, boxes, periodic, L, bc=None, alpha=0.0, beta=1.0):
        self.name, self.n, self.boxes, self.periodic, self.L = name, n, boxes, periodic, L
        self.bc, self.alpha, self.beta = bc, alpha, beta

    def __repr__(self):
        return self.name


ONE_BOX = Case("one-box-40", (136, 40, 16), None, (False,) * 3, (2.0, 1.0, 0.5))
ONE_ROW = Case("one-box-28", (136, 28, 16), None, (False,) * 3, (2.0, 1.0, 0.5))
# periodic in x: the one box across x is its own neighbour there; the y seam is exchanged two deep
SEAM = Case("seam-periodic", (136, 80, 8), [((0, 0, 0), (135, 39, 7)), ((0, 40, 0), (135, 79, 7))], (True, False, False),
            (2.0, 1.0, 0.5))
HELMHOLTZ = Case("helmholtz-dirichlet", (136, 40, 16), None, (False,) * 3, (2.0, 1.0, 0.5), [D] * 6, 1.0, -0.01)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("SOMAR_FUSED_MIN_CELLS", "0")
    monkeypatch.setenv("SOMAR_MARCH_MIN_CELLS", "0")
    for k in ("SOMAR_NARROW_7PT", "SOMAR_NO_NARROW_TILES", "SOMAR_FUSED_ROWS", "SOMAR_ORDERED_REDUCE_MAX"):
        monkeypatch.delenv(k, raising=False)


def set_tables(monkeypatch, no_narrow, ordered):
    for k, v in (("SOMAR_NO_NARROW_TILES", no_narrow), ("SOMAR_ORDERED_REDUCE_MAX", ordered)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def problem(so, case):
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in case.n)), case.periodic)
    grids = [so.Box(lo, hi) for lo, hi in case.boxes] if case.boxes else [so.Box(dom.box.lo, dom.box.hi)]
    dx = tuple(case.L[d] / case.n[d] for d in range(3))
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, case.L, 3, "stretched", domain=dom)
    return dom, grids, dx, Jgup, Jinv


def residual_field(so, case, prob):
    res = so.random_field(prob[1], 5, (0, 0, 0), prob[0].box)
    if case.bc is None and case.alpha == 0.0:
        so.remove_weighted_mean(res, prob[4])
    return res


_ORACLE = {}   # case name -> (residual, the oracle's correction per box): computed once, only looked at


def oracle_cycle(so, case):
    """MultiGrid::one_cycle from zero, 2/2/2, a fresh bottom solver as in the GPU handle"""
    if case.name not in _ORACLE:
        prob = problem(so, case)
        dom, grids, dx, Jgup, Jinv = prob
        res = residual_field(so, case, prob)
        bc = so.BCHolder() if case.bc is None else so.BCHolder([[case.bc[2 * d], case.bc[2 * d + 1]] for d in range(3)], None)
        fac = so.Factory(dom, grids, dx, bc, Jgup, Jinv, alpha=case.alpha, beta=case.beta)
        amr = so.AMRMultiGrid(fac, so.BiCGStab())
        amr.pre = amr.post = amr.bottom = 2
        amr.mg.pre = amr.mg.post = amr.mg.bottom = 2
        corr = so.LevelData(grids, 1, (1, 1, 1))
        amr.mg.init(corr, res)
        amr.mg.bottomSolver = so.BiCGStab()
        amr.mg.bottomSolver.define(amr.mg.ops[-1], True)
        amr.mg.one_cycle(corr, res)
        _ORACLE[case.name] = (prob, res, [np.array(f.view(g)[..., 0]) for g, f in zip(corr.grids, corr.fabs)])
    return _ORACLE[case.name]


def gpu_solver(case, prob):
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv = prob
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=case.alpha, beta=case.beta,
             bc_type=case.bc)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                         np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return s


def assert_tall_rule(s, no_narrow, depth=0):
    """the inputs of march_plan.h's rule as the library reports them: 16-row kernels, a metric that is not uniform, every
    box of the depth even and wider than 128, and the two switches that restore today's tables.  Inputs only: the library
    exports no tile table and no launch counter for the 7-point sweep, so this does not prove that the tall table was built
    (see the module docstring)"""
    assert s.tuning("FUSED_ROWS") == 16 and s.tuning("NARROW_7PT") == -1
    assert s.tuning("NO_NARROW_TILES") == (1 if no_narrow else 0)
    assert s.metricUniform(depth) is None
    widths = [s.patch_box(q, depth)[1][0] - s.patch_box(q, depth)[0][0] + 1 for q in range(s.num_local_patches)]
    assert widths and all(w % 2 == 0 and w > 128 for w in widths), widths


def gpu_cycle(case, prob, res, no_narrow, fp32=False, fold=None):
    """fold: whether depth 0 must be on the folded-prolongation path (PressureSolver::fold_prolong: fused sweep, not a
    serial-order depth, no coarse-fine faces) -- its inputs are asserted, the library has no counter for it"""
    from somar_amd import api as F
    s = gpu_solver(case, prob)
    try:
        assert_tall_rule(s, no_narrow)
        if fold is not None:
            cells = [s.levelInfo(d)["cells"] for d in range(s.depth())]
            limit = s.tuning("ORDERED_REDUCE_MAX")
            assert s.tuning("NO_FOLD_PROLONG") == 0 and s.tuning("FUSED_MIN_CELLS") == 0
            assert len(cells) >= 2 and all(c <= limit for c in cells[1:]), (cells, limit)
            assert (cells[0] > limit) == fold, (cells, limit)
        if fp32:
            s.setPrecision(1)
            assert s.precision()[0] == 1 and s.precision()[1] >= 1, s.precision()
        upload(s, F.F_RES, res)
        s.vcycleFromZero(F.F_CORR, F.F_RES)
        return download_valid(s, F.F_CORR, prob[1])
    finally:
        s.undefine()


def assert_same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg="%s, box %d" % (what, i))


@pytest.mark.parametrize("case", [ONE_BOX, ONE_ROW, SEAM, HELMHOLTZ], ids=repr)
def test_vcycle_against_the_oracle_on_both_tables(oracle, monkeypatch, case):
    prob, res, want = oracle_cycle(oracle, case)
    scale = max(float(np.abs(w).max()) for w in want)
    for ordered, fold in ((ORDERED_ALL, False), (ORDERED_BELOW_TOP, True)):
        got = {}
        for label, no_narrow in TABLES:
            set_tables(monkeypatch, no_narrow, ordered)
            got[label] = gpu_cycle(case, prob, res, no_narrow, fold=fold)
        assert_same(got["tall"], got["equal"], "%s, sum limit %s: tall against equal columns" % (case, ordered))
        if not fold:
            assert_same(got["tall"], want, "%s: tall tiles against the oracle, serial-order sums" % case)
        else:
            for i, (g, w) in enumerate(zip(got["tall"], want)):
                print("%s box %d, depth 0 folded (mode %s): max|c - c_oracle| / scale = %.3e" % (
                    case, i, "3" if case.bc else "4", np.abs(g - w).max() / scale))
                np.testing.assert_allclose(g, w, rtol=0, atol=TREE_SUM_TOL * scale, err_msg="%s box %d" % (case, i))


def test_fp32_cycle_same_on_both_tables(oracle, monkeypatch):
    """the float instantiations (modes 1, 0 and 4): the opt-in fp32 cycle on depth 0.  A depth that sums in serial order or is
    replayed as a graph stays fp64 (PressureSolver::mp_setup), so: depth 0 above the sum limit, the bottom below it, and
    SOMAR_GRAPH_CELLS below depth 0 as test_gpu_mixed_kernels.py sets it.  The issue asks for the two tables to agree; the
    distance from the fp64 oracle is printed, not bounded: it measures 2.3e-5 with either table, where the fp32 cycles of
    test_gpu_mixed_kernels.py stay under 1e-6 -- presumably (not examined) because this hierarchy's bottom level is the
    43520-cell depth right below, whose BiCGStab magnifies fp32-sized differences in its right-hand side."""
    case = ONE_BOX
    prob, res, want = oracle_cycle(oracle, case)
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", "4096")
    got = {}
    for label, no_narrow in TABLES:
        set_tables(monkeypatch, no_narrow, ORDERED_BELOW_TOP)
        got[label] = gpu_cycle(case, prob, res, no_narrow, fp32=True, fold=True)
    assert_same(got["tall"], got["equal"], "fp32 cycle: tall against equal columns")
    err = max(float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got["tall"], want))
    print("fp32 cycle on tall tiles: max|c32 - c_oracle| / max|c_oracle| = %.3e" % err)


# ---- AMR: a refined level with one 136-wide box, coarse-fine faces on both x sides ------------------------------------------
AMR_N, AMR_L, AMR_RATIOS = (96, 8, 8), (6.0, 1.0, 0.5), [(2, 2, 1)]
AMR_BOXES = [[((28, 0, 0), (163, 15, 7))]]


def test_amr_vcycle_bit_exact_on_both_tables(oracle, monkeypatch):
    """one AMR V-cycle from zero as test_gpu_amr_wide.py runs it: the coarse-fine ghosts of the black pass are made inside the
    sweep, the x-low face in lane 0 of the first column, the x-high face in the last (clipped) column"""
    from oracle import somar_amr as am
    from somar_amd import api as F
    so = oracle
    fb = [[so.Box(lo, hi) for lo, hi in lev] for lev in AMR_BOXES]
    levels = make_amr_levels(so, am, AMR_N, AMR_L, (False, True, False), AMR_RATIOS, fb, variant="stretched", cbox=AMR_N)
    comp = am.AMRComposite(levels, AMR_RATIOS, so.BCHolder(), so.BiCGStab(), isDiagonal=True)
    phi = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
    res = [so.random_field(L.grids, 70 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
    comp.zero_covered(0, res[0])
    comp.init(phi, res, 1, 0)
    comp.set_bottom_solver(1, 0)
    corr = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
    comp.amr_vcycle(corr, res, 1, 1, 0)
    want = [[np.array(x) for x in valid_of(c)] for c in corr]
    got = {}
    for label, no_narrow in TABLES:
        set_tables(monkeypatch, no_narrow, ORDERED_ALL)
        gpu = make_gpu_amr(levels, AMR_RATIOS)
        try:
            assert_tall_rule(gpu.levels[1], no_narrow)
            assert gpu.levels[1].mgRefRatios() == [tuple(r) for r in comp.mg[1].mgRefRatios]
            for l, v in enumerate(gpu.levels):
                upload(v, F.F_RES, res[l])
                v.setVal(F.F_CORR, 0.0)
            gpu.vcycleAMR(1, 0)
            got[label] = [download_valid(gpu.levels[l], F.F_CORR, levels[l].grids) for l in range(2)]
        finally:
            gpu.undefine()
    for l in range(2):
        assert_same(got["tall"][l], got["equal"][l], "AMR V-cycle level %d: tall against equal columns" % l)
        assert_same(got["tall"][l], want[l], "AMR V-cycle level %d against the oracle" % l)


# ---- two ranks over the shared-memory transport ---------------------------------------------------------------------------
# two 136 x 64 x 8 boxes stacked in y, one per rank: 64 rows, so that a 28-row tile lies between a box's two y faces and reads
# no cell the other rank fills -- the sweeps' exchanges then travel under those tiles (fused_overlap)
RANKS_N, RANKS_BOX, RANKS_L = (136, 128, 8), (136, 64, 8), (2.0, 1.0, 0.5)
SWEEPS = 3


def _ranks_problem(so):
    from tests.helpers import make_problem
    return make_problem(so, RANKS_N, RANKS_BOX, "stretched", (False, True, False), RANKS_L)


def _relax_and_restrict(so, F, gpu, grids, dom):
    phi = so.random_field(grids, 13, (1, 1, 1), dom.box)
    rhs = so.random_field(grids, 14, (0, 0, 0), dom.box)
    upload(gpu, F.F_PHI, phi)
    upload(gpu, F.F_RHS, rhs)
    gpu.relax(0, F.F_PHI, F.F_RHS, SWEEPS)
    out = download_valid(gpu, F.F_PHI, grids)
    gpu.restrictResidual(0, F.FIELD(1, F.F_RES), F.F_PHI, F.F_RHS)
    return out


def _worker(rank, nranks, name, path, q):
    try:
        os.environ["SOMAR_FUSED_MIN_CELLS"] = "0"
        os.environ["SOMAR_MARCH_MIN_CELLS"] = "0"
        os.environ.pop("SOMAR_NO_OVERLAP", None)
        os.environ.pop("SOMAR_NARROW_7PT", None)
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, os.path.dirname(here))
        from oracle import somar_oracle as so
        from somar_amd import api as F
        from tests.helpers import make_gpu_solver
        want = np.load(path)
        comm = F.comm_create_shm(name, rank, nranks)
        dom, grids, dx, Jgup, Jinv = _ranks_problem(so)
        assert len(grids) == nranks
        owner = list(range(nranks))
        for label, no_narrow in TABLES:
            if no_narrow is None:
                os.environ.pop("SOMAR_NO_NARROW_TILES", None)
            else:
                os.environ["SOMAR_NO_NARROW_TILES"] = no_narrow
            gpu = make_gpu_solver(dom, grids, dx, Jgup, Jinv, owner=owner, comm=comm)
            try:
                assert_tall_rule(gpu, no_narrow)
                got = _relax_and_restrict(so, F, gpu, grids, dom)
                assert gpu.counters()["overlapped_sweeps"] >= SWEEPS, gpu.counters()
                n = 0
                for gi, g in enumerate(got):
                    if g is None:
                        continue
                    np.testing.assert_array_equal(g, want["box%d" % gi], err_msg="%s tables, box %d" % (label, gi))
                    n += 1
                assert n == 1
            finally:
                gpu.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_two_ranks_match_one_process(oracle, monkeypatch, tmp_path):
    """three fused sweeps on a level sharded over two ranks, overlap on, on both tables: the bits of the one-process run (which
    in turn is the oracle's relax)"""
    from somar_amd import api as F
    from tests.helpers import make_gpu_solver, make_oracle_solver
    so = oracle
    dom, grids, dx, Jgup, Jinv = _ranks_problem(so)
    gpu = make_gpu_solver(dom, grids, dx, Jgup, Jinv)
    try:
        assert_tall_rule(gpu, None)
        one = _relax_and_restrict(so, F, gpu, grids, dom)
    finally:
        gpu.undefine()
    phi = so.random_field(grids, 13, (1, 1, 1), dom.box)
    rhs = so.random_field(grids, 14, (0, 0, 0), dom.box)
    make_oracle_solver(so, dom, grids, dx, Jgup, Jinv).mg.ops[0].relax(phi, rhs, SWEEPS)
    assert_same(one, valid_of(phi), "one process against the oracle's relax")
    path = str(tmp_path / "one_process.npz")
    np.savez(path, **{"box%d" % i: a for i, a in enumerate(one)})
    nranks = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/somar_%s" % uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=_worker, args=(r, nranks, name, path, q)) for r in range(nranks)]
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
