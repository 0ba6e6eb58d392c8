"""Several components on one NON-diagonal (19-point) handle (somar_solver_set_components_full): the N-field colour pass and
residual (full19_multi.hip) and the lock-step solve, bit for bit against the single-field path -- the specification of the multi
calls is that they leave every component as successive single-field calls would -- and, for one component other than 0, against
the oracle's V-cycle on Factory(..., isDiagonal=False), the standard tests/test_gpu_full.py holds the single-field kernels to.

Environment.  The marching kernels are forced onto these small levels as tests/test_gpu_mixed_kernels.set_env does it
(SOMAR_MARCH_MIN_CELLS = SOMAR_FUSED_MIN_CELLS = 0, and the graph threshold through SOMAR_GRAPH_CELLS), the fused red+black
19-point sweep is off (SOMAR_FUSED19_MIN_BOX = -1).  The layouts below are those of tests/test_gpu_full.py -- the smallest at
which the marching kernel can go wrong -- and have 3072 to 8192 cells: set_env's own graph threshold of 4096 cells, and the
serial-order sums' default of 4096, would leave none of their depths to batch.  Both thresholds are therefore SMALL = 512 here
(SOMAR_GRAPH_CELLS, SOMAR_ORDERED_REDUCE_MAX): a depth of more than 512 cells is batched, and the expected K of a case is that
count taken from the handle's level sizes, never from get_components.  Boxes of (12,8,8) and (128,6,4) do not coarsen (the
reference coarsens a box only to a multiple of 4 cells), so `seams` and `wide` are hierarchies of ONE depth: what is batched
there is the bottom depth's sweeps, and the V-cycle is those sweeps and the bottom solve per component.

Operator: Helmholtz, alpha = 1, beta = -0.01 (no null space); metric: oracle.make_full_metric.

Layouts:
  * seams      (24,16,8) in boxes of (12,8,8), no periodic side: box seams in x and y, six Neumann sides with cross terms
  * periodic   (16,16,16) in boxes of 8, periodic in all three directions: the periodic wrap of the frame
  * wide       (128,6,4) in one box, periodic in x: the N-field table's own columns (64 + 64) against the level's 124 + 4
  * dirichlet  (32,16,16) in boxes of 16^3, sides [D,N,N,D,D,N] with non-zero constants: Dirichlet ghosts in the programs, per
               field.  Under thresholds of 1024 cells (the layout's own): depth 0 batched, a seam to the 1024-cell depth below.
  * dirichlet-deep  the same under 512: two batched depths (8192 and 1024 cells), the restriction lands on a batched depth
  * zero-xy    seams with J g^{xy} on x-faces and J g^{yx} on y-faces exactly zero: the ZXY instantiations (every other layout
               runs the ones that stream those planes)
  * rows-6     seams under SOMAR_FULL_ROWS=6: the level's own tables and single-field launches are the 6-row ones
Every case first proves it reached the N-field path: get_components returns the expected K and the launch count grows."""
import numpy as np
import pytest

from tests.helpers import download_valid, upload
from tests.test_gpu_mixed_kernels import set_env

pytestmark = pytest.mark.gpu

D, N = 1, 0
ALPHA, BETA = 1.0, -0.01
SMALL = 512
BC_VALUES = [0.25, -0.5, 0.75, 0.1, -0.3, 0.6]
MIXED = [D, N, N, D, D, N]


class Layout:
    def __init__(self, name, n, boxes, periodic, L, bc=None, zero_xy=False, rows=None, K=1, ref=None, small=SMALL):
        self.name, self.n, self.boxes, self.periodic, self.L, self.bc = name, n, boxes, periodic, L, bc
        self.zero_xy, self.rows, self.K, self.ref, self.small = zero_xy, rows, K, ref or name, small


LAYOUTS = {c.name: c for c in [
    Layout("seams", (24, 16, 8), (12, 8, 8), (False,) * 3, (1.5, 1.0, 0.5)),
    Layout("periodic", (16, 16, 16), 8, (True,) * 3, (1.0, 1.0, 1.0)),
    Layout("wide", (128, 6, 4), (128, 6, 4), (True, False, False), (4.0, 1.0, 0.5)),
    Layout("dirichlet", (32, 16, 16), (16, 16, 16), (False,) * 3, (2.0, 1.0, 1.0), bc=MIXED, K=1, small=1024),
    Layout("dirichlet-deep", (32, 16, 16), (16, 16, 16), (False,) * 3, (2.0, 1.0, 1.0), bc=MIXED, K=2, ref="dirichlet"),
    Layout("zero-xy", (24, 16, 8), (12, 8, 8), (False,) * 3, (1.5, 1.0, 0.5), zero_xy=True),
    Layout("rows-6", (24, 16, 8), (12, 8, 8), (False,) * 3, (1.5, 1.0, 0.5), rows="6", ref="seams"),
]}


@pytest.fixture(autouse=True)
def _marching_kernels_on_small_levels(monkeypatch):
    set_env(monkeypatch.setenv)
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", str(SMALL))
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", str(SMALL))
    monkeypatch.setenv("SOMAR_FUSED19_MIN_BOX", "-1")
    monkeypatch.delenv("SOMAR_FULL_ROWS", raising=False)


def _rows_env(monkeypatch, lay):
    """the layout's own switches: its row count and its thresholds"""
    if lay.rows:
        monkeypatch.setenv("SOMAR_FULL_ROWS", lay.rows)
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", str(lay.small))
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", str(lay.small))


_PROBLEMS = {}


def problem(so, lay, amp=None):
    key = (lay.ref if not lay.zero_xy else lay.name, amp)
    if key not in _PROBLEMS:
        dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in lay.n)), lay.periodic)
        grids = so.split_domain(dom.box, lay.boxes)
        dx = tuple(lay.L[d] / lay.n[d] for d in range(3))
        Jgup, Jinv = so.make_full_metric(grids, dx, lay.L, dom, **({"amp": amp} if amp else {}))
        if lay.zero_xy:
            for gi in range(len(grids)):
                Jgup[gi][0].a[..., 1] = 0.0   # J g^{xy} on x-faces
                Jgup[gi][1].a[..., 0] = 0.0   # J g^{yx} on y-faces
        _PROBLEMS[key] = (dom, grids, dx, Jgup, Jinv)
    return _PROBLEMS[key]


def _bc_holder(so, lay, values):
    if lay.bc is None:
        return so.BCHolder()
    v = values or [0.0] * 6
    return so.BCHolder([[lay.bc[2 * d], lay.bc[2 * d + 1]] for d in range(3)], [[v[2 * d], v[2 * d + 1]] for d in range(3)])


def _set_metric(s, prob):
    Jgup, Jinv = prob[3], prob[4]
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricFull(q, *[np.asfortranarray(Jgup[gi][d].a) for d in range(3)], np.asfortranarray(Jinv[gi].a[..., 0]))


def handle(lay, prob, sweeps=2, eps=1e-10, imax=100, norm_thresh=None, alpha=ALPHA, beta=BETA, values=None, relax=1, num_mg=None,
           bottom_imax=None):
    """bottom_imax = 0: the BiCGStab bottom solve runs no iteration (it adds its zero correction): a cycle without a sum"""
    from somar_amd import AMRPressureSolver
    dom, grids, dx = prob[0], prob[1], prob[2]
    s = AMRPressureSolver()
    p = s._p
    if bottom_imax is not None:
        s.setBottomParameters(bottom_imax, p.bottom_num_restarts, p.bottom_eps, p.bottom_reps, p.bottom_hang, p.bottom_small,
                              p.bottom_norm_type, p.bottom_verbosity)
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, sweeps, sweeps, sweeps, p.precond_mode, relax,
                         p.num_mg if num_mg is None else num_mg, p.hang, p.norm_thresh if norm_thresh is None else norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=alpha, beta=beta, bc_type=lay.bc)
    if lay.bc is not None:
        s.setBCValues(values or BC_VALUES)
    _set_metric(s, prob)
    s.finalize()
    return s


def expected_K(s, lay):
    """the leading depths of more than lay.small cells (the bottom depth included: seams and wide do not coarsen at all)"""
    K = 0
    while K < s.depth() and s.levelInfo(K)["cells"] > lay.small:
        K += 1
    assert K >= 1 and (lay.K is None or K == lay.K), (lay.name, K, [s.levelInfo(d)["cells"] for d in range(s.depth())])
    return K


def _up(s, comp, field, ld):
    for p in range(s.num_local_patches):
        _, _, gi = s.patch_box(p)
        s.uploadComp(comp, field, p, np.asfortranarray(ld[gi].a[..., 0]), ld.ghost)


def _down(s, comp, field, grids, ghost=(0, 0, 0)):
    out = [None] * len(grids)
    for p in range(s.num_local_patches):
        _, _, gi = s.patch_box(p)
        out[gi] = s.downloadComp(comp, field, p, ghost)
    return out


def _same(got, ref, what):
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(g, r, err_msg="%s, box %d" % (what, b))


def _reaches(s, ncomp, K, before):
    n, k, launches = s.getComponents()
    assert (n, k) == (ncomp, K), (n, k, ncomp, K)
    assert launches > before, "no N-field launch was issued"
    return launches


# ---- 1. the V-cycle kernels -------------------------------------------------------------------------------------------------------
_CYCLE_REFS = {}


def _oracle_cycle(so, lay, prob, res, sweeps, bottom_imax=None):
    dom, grids, dx, Jgup, Jinv = prob
    fac = so.Factory(dom, grids, dx, _bc_holder(so, lay, BC_VALUES), Jgup, Jinv, alpha=ALPHA, beta=BETA, isDiagonal=False)
    amr = so.AMRMultiGrid(fac, so.BiCGStab())
    amr.pre = amr.post = amr.bottom = sweeps
    amr.mg.pre = amr.mg.post = amr.mg.bottom = sweeps
    corr = so.LevelData(grids, 1, (1, 1, 1))
    amr.mg.init(corr, res)
    amr.mg.bottomSolver = so.BiCGStab() if bottom_imax is None else so.BiCGStab(imax=bottom_imax)
    amr.mg.bottomSolver.define(amr.mg.ops[-1], True)
    amr.mg.one_cycle(corr, res)
    return [f.view(g)[..., 0] for g, f in zip(corr.grids, corr.fabs)]


def _cycle_refs(so, lay, sweeps=2, bottom_imax=None):
    """per component seed the residual field and its V-cycle from zero on a separate one-component handle of the same problem
    (under the layout's own row count and thresholds); for component 1 the oracle's V-cycle.  Once per (layout, bottom), left
    unchanged.  The last entry says whether the bottom depth sums in serial order, as the oracle does."""
    from somar_amd import api as F
    key = (lay.name, sweeps, bottom_imax)
    if key not in _CYCLE_REFS:
        prob = problem(so, lay)
        dom, grids = prob[0], prob[1]
        res = [so.random_field(grids, 5 + c, (0, 0, 0), dom.box) for c in range(4)]
        s = handle(lay, prob, sweeps=sweeps, bottom_imax=bottom_imax)
        try:
            serial_bottom = s.levelInfo(s.depth() - 1)["cells"] <= lay.small
            seq = []
            for c in range(4):
                upload(s, F.F_RES, res[c])
                s.vcycleFromZero(F.F_CORR, F.F_RES)
                seq.append(download_valid(s, F.F_CORR, grids))
            assert s.getComponents() == (1, 0, 0)   # the single-field path issues no N-field launch
        finally:
            s.undefine()
        _CYCLE_REFS[key] = (prob, res, seq, _oracle_cycle(so, lay, prob, res[1], sweeps, bottom_imax), serial_bottom)
    return _CYCLE_REFS[key]


def _vcycle_multi(lay, prob, res, ncomp, bottom_imax=None):
    from somar_amd import api as F
    grids = prob[1]
    s = handle(lay, prob, bottom_imax=bottom_imax)
    try:
        assert s.tuning("FULL_ROWS") == (6 if lay.rows else 8)
        s.setComponentsFull(ncomp)
        K = expected_K(s, lay)
        assert s.getComponents() == (ncomp, K, 0)
        for c in range(ncomp):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        _reaches(s, ncomp, K, 0)
        return [_down(s, c, F.F_CORR, grids) for c in range(ncomp)]
    finally:
        s.undefine()


@pytest.mark.parametrize("ncomp", [2, 3, 4])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_vcycle_multi_is_the_single_field_cycle_per_component(oracle, monkeypatch, name, ncomp):
    """Every component against the single-field cycle and component 1 against the oracle's V-cycle, bit for bit.  Where the
    bottom depth is itself batched -- the one-depth layouts, whose boxes do not coarsen -- its BiCGStab bottom solve sums in
    tree order (a batched depth lies above the serial-order threshold), which the oracle's serial sums do not reproduce to the
    last bit on ANY path, the single-field one included.  There the cycle runs a second time with the bottom solver's imax = 0
    on both sides -- the bottom sweeps, restriction and prolongation as before, the bottom solve adding its zero correction --
    and that cycle, which contains no sum, is the one compared with the oracle, bit for bit."""
    so, lay = oracle, LAYOUTS[name]
    _rows_env(monkeypatch, lay)
    prob, res, seq, ora, serial_bottom = _cycle_refs(so, lay)
    got = _vcycle_multi(lay, prob, res, ncomp)
    for c in range(ncomp):
        assert all(float(np.max(np.abs(g))) > 0.0 for g in got[c])
        _same(got[c], seq[c], "%s: component %d of %d vs the single-field cycle" % (name, c, ncomp))
    if serial_bottom:
        _same(got[1], ora, "%s: component 1 of %d vs the oracle's V-cycle" % (name, ncomp))
        return
    prob, res, seq0, ora0, _ = _cycle_refs(so, lay, bottom_imax=0)
    got0 = _vcycle_multi(lay, prob, res, ncomp, bottom_imax=0)
    for c in range(ncomp):
        assert all(float(np.max(np.abs(g))) > 0.0 for g in got0[c])
        _same(got0[c], seq0[c], "%s, no bottom iteration: component %d of %d vs the single-field cycle" % (name, c, ncomp))
    _same(got0[1], ora0, "%s, no bottom iteration: component 1 of %d vs the oracle's V-cycle" % (name, ncomp))
    assert any(not np.array_equal(x, y) for x, y in zip(got0[1], got[1]))   # (the bottom solve does act in the first cycle)


def test_the_oracle_check_is_exact_on_the_layouts_with_a_coarser_depth(oracle, monkeypatch):
    """which branch a layout takes is not left to chance: periodic and dirichlet (sides, Dirichlet programs, a restriction
    and a prolongation on the way) keep the plain oracle comparison, with the bottom solver at work"""
    for name in ("periodic", "dirichlet"):
        lay = LAYOUTS[name]
        _rows_env(monkeypatch, lay)
        assert _cycle_refs(oracle, lay)[4], name


def test_zero_xy_layout_differs_from_the_sheared_one(oracle):
    """the zero planes are the layout's own metric, not the sheared one's: the two layouts' cycles differ"""
    a, b = _cycle_refs(oracle, LAYOUTS["seams"]), _cycle_refs(oracle, LAYOUTS["zero-xy"])
    assert any(not np.array_equal(x, y) for x, y in zip(a[2][0], b[2][0]))
    Jgup = b[0][3]
    for gi in range(len(b[0][1])):
        assert not Jgup[gi][0].a[..., 1].any() and not Jgup[gi][1].a[..., 0].any() and Jgup[gi][0].a[..., 2].any()


# ---- 2. the ghost layer -------------------------------------------------------------------------------------------------------------
GHOST_MARK = 7.5   # what the caller leaves in the ghost cells of a given correction


@pytest.mark.parametrize("name", ["seams", "wide", "periodic", "dirichlet", "dirichlet-deep"])
def test_vcycle_multi_leaves_the_ghost_cells_as_the_single_field_cycle(oracle, monkeypatch, name):
    """from_zero = False on a given correction whose ghost cells hold a mark, the ghost layer compared too: whatever the
    single-field cycle leaves there (exchanged values on the seams and periodic sides, the programs' Neumann ghosts on the
    walls), the N-field passes must leave -- copy_frames carries the frame from buffer to buffer per field, and a tile's last
    column is cut by the box, not by its width.  seams and wide are one depth (bottom sweeps and bottom solve); periodic,
    dirichlet (a seam below depth 0) and dirichlet-deep (two batched depths) have the restriction and the prolongation on the way"""
    from somar_amd import api as F
    so, lay = oracle, LAYOUTS[name]
    _rows_env(monkeypatch, lay)
    prob = problem(so, lay)
    dom, grids = prob[0], prob[1]
    res = [so.random_field(grids, 21 + c, (0, 0, 0), dom.box) for c in range(3)]
    cor = [so.random_field(grids, 31 + c, (1, 1, 1), dom.box) for c in range(3)]
    for c in range(3):
        for g, f in zip(grids, cor[c].fabs):
            valid = np.array(f.view(g))
            f.a[...] = GHOST_MARK + c
            f.view(g)[...] = valid
    s = handle(lay, prob)
    try:
        seq = []
        for c in range(3):
            upload(s, F.F_RES, res[c])
            upload(s, F.F_CORR, cor[c])
            s.vcycle(F.F_CORR, F.F_RES)
            seq.append([s.download(F.F_CORR, q, (1, 1, 1)) for q in range(s.num_local_patches)])
        s.setComponentsFull(3)
        K = expected_K(s, lay)
        for c in range(3):
            _up(s, c, F.F_RES, res[c])
            _up(s, c, F.F_CORR, cor[c])
        s.vcycleMulti(False)
        _reaches(s, 3, K, 0)
        for c in range(3):
            got = [s.downloadComp(c, F.F_CORR, q, (1, 1, 1)) for q in range(s.num_local_patches)]
            _same(got, seq[c], "%s, component %d with its ghost layer" % (name, c))
    finally:
        s.undefine()


# ---- 3. solves ----------------------------------------------------------------------------------------------------------------------
STAT_KEYS = ("iters", "exitStatus", "status", "bottom_iters", "bottom_exit", "initial_rnorm", "final_rnorm", "history")
# The solves stop on the ABSOLUTE residual norm (norm_thresh) or on imax; eps is out of reach.  Random right-hand sides of 5, 1e3
# and 1e12 times NORM_THRESH in the max norm: whatever a V-cycle contracts by (between 0.01 and 0.5, certainly), the first falls
# below NORM_THRESH within 1 to 3 cycles, the second needs 3 decades -- 2 to 10 cycles, and more than the first -- and the third,
# 12 decades away, runs longer still (into IMAX unless a cycle contracts by 0.1 or better).
IMAX, NORM_THRESH, EPS = 12, 1e-12, 1e-30
SCALES = (5.0, 0.0, 1e3, 1e12)   # component 1: identically zero (no cycle; not first)


def _solve_rhs(so, prob):
    dom, grids = prob[0], prob[1]
    out = []
    for c, scale in enumerate(SCALES):
        f = so.random_field(grids, 11 + c, (0, 0, 0), dom.box)
        for fab in f.fabs:
            fab.a[...] *= scale * NORM_THRESH
        out.append(f)
    return out


def _solve_both_ways(so, lay, zero_phi, force_homogeneous):
    from somar_amd import api as F
    prob = problem(so, lay)
    dom, grids = prob[0], prob[1]
    rhs = _solve_rhs(so, prob)
    nc = len(rhs)
    guess = [so.random_field(grids, 51 + c, (1, 1, 1), dom.box) for c in range(nc)]
    s = handle(lay, prob, eps=EPS, imax=IMAX, norm_thresh=NORM_THRESH)
    try:
        seq = []
        for c in range(nc):
            upload(s, F.F_RHS, rhs[c])
            if not zero_phi:
                upload(s, F.F_PHI, guess[c])
            st = s.solveResident(zeroPhi=zero_phi, forceHomogeneous=force_homogeneous)
            seq.append((download_valid(s, F.F_PHI, grids), dict(st), [float(v) for v in F.last_history()]))
        s.setComponentsFull(nc)
        for c in range(nc):
            _up(s, c, F.F_RHS, rhs[c])
            if not zero_phi:
                _up(s, c, F.F_PHI, guess[c])
        stats = s.solveMulti(zeroPhi=zero_phi, forceHomogeneous=force_homogeneous)
        _reaches(s, nc, expected_K(s, lay), 0)
        for c in range(nc):
            print("%s component %d: %d V-cycles, exit %d, bottom %d/%d, final/initial %.3e" % (
                lay.name, c, stats[c]["iters"], stats[c]["exitStatus"], stats[c]["bottom_iters"], stats[c]["bottom_exit"],
                stats[c]["final_rnorm"] / max(stats[c]["initial_rnorm"], 1e-300)))
            _same(_down(s, c, F.F_PHI, grids), seq[c][0], "phi of component %d" % c)
            for k in STAT_KEYS:
                assert stats[c][k] == seq[c][1][k], (c, k, stats[c][k], seq[c][1][k])
            assert s.compHistory(c) == seq[c][2], c
    finally:
        s.undefine()
    return stats


def _assert_active_set_shrinks(stats):
    """4 -> 3 at once (the zero right-hand side), then 3 -> 2 -> 1: three different cycle counts"""
    a, z, b, c = (st["iters"] for st in stats)
    assert z == 0 and 0 < a < b < c <= IMAX, (a, z, b, c)


@pytest.mark.parametrize("name", ["seams", "periodic"])
def test_solve_multi_is_successive_solves(oracle, name):
    """(seams is a hierarchy of one depth: its cycle ends in the bottom solve on the level itself, every right-hand side
    converges in one cycle -- (1, 0, 1, 1) measured -- and only the zero one leaves the set early; the shrinking active set is
    asserted where there is a coarser depth)"""
    stats = _solve_both_ways(oracle, LAYOUTS[name], True, False)
    if name == "seams":
        assert [st["iters"] for st in stats] == [1, 0, 1, 1]
    else:
        _assert_active_set_shrinks(stats)


@pytest.mark.parametrize("zero_phi,force_homogeneous", [(True, False), (False, False), (True, True)])
def test_solve_multi_with_dirichlet_values(oracle, zero_phi, force_homogeneous):
    """(inhomogeneous values: the right-hand side identically zero is no solve without a cycle, so the active set is asserted
    to shrink only with force_homogeneous)"""
    stats = _solve_both_ways(oracle, LAYOUTS["dirichlet-deep"], zero_phi, force_homogeneous)
    if force_homogeneous:
        _assert_active_set_shrinks(stats)


# ---- 4. heat steps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_heat_step_multi_is_three_heat_steps(oracle, scheme):
    from somar_amd import api as F
    so, lay = oracle, LAYOUTS["dirichlet-deep"]
    prob = problem(so, lay)
    dom, grids = prob[0], prob[1]
    old = [so.random_field(grids, 61 + c, (1, 1, 1), dom.box) for c in range(3)]
    src = [so.random_field(grids, 71 + c, (0, 0, 0), dom.box) for c in range(3)]
    dt = 0.01   # (I - dt L)
    s = handle(lay, prob, eps=1e-8, imax=20, alpha=1.0, beta=1.0)
    try:
        seq = []
        for c in range(3):
            upload(s, F.F_HEAT_OLD, old[c])
            upload(s, F.F_HEAT_SRC, src[c])
            st = s.heatStep(scheme, dt, zeroPhi=True)
            seq.append((download_valid(s, F.F_PHI, grids), dict(st)))
        s.setComponentsFull(3)
        for c in range(3):
            _up(s, c, F.F_HEAT_OLD, old[c])
            _up(s, c, F.F_HEAT_SRC, src[c])
        stats = s.heatStepMulti(scheme, dt, zeroPhi=True)
        _reaches(s, 3, expected_K(s, lay), 0)
        for c in range(3):
            assert stats[c]["iters"] > 0
            _same(_down(s, c, F.F_PHI, grids), seq[c][0], "scheme %d, phi of component %d" % (scheme, c))
            for k in STAT_KEYS:
                assert stats[c][k] == seq[c][1][k], (scheme, c, k)
    finally:
        s.undefine()


# ---- 5. metric refresh ----------------------------------------------------------------------------------------------------------------
def test_metric_refresh_with_three_components(oracle):
    """the sheared map with other amplitudes written into a three-component handle: the components' uploaded fields survive,
    the batched depths are decided again, and one cycle is a freshly defined handle's with the new metric"""
    from somar_amd import api as F
    so, lay = oracle, LAYOUTS["dirichlet-deep"]
    prob = problem(so, lay)
    prob2 = problem(so, lay, amp=(0.1, 0.3, 0.2))
    grids = prob[1]
    res = [so.random_field(grids, 5 + c, (0, 0, 0), prob[0].box) for c in range(3)]
    s = handle(lay, prob)
    try:
        s.setComponentsFull(3)
        K = expected_K(s, lay)
        for c in range(3):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        launches = _reaches(s, 3, K, 0)
        first = [_down(s, c, F.F_CORR, grids) for c in range(3)]
        with s.metricUpdate():
            _set_metric(s, prob2)
        assert s.getComponents() == (3, K, launches)
        for c in range(3):
            _same(_down(s, c, F.F_RES, grids), [np.asfortranarray(f.a[..., 0]) for f in res[c].fabs], "F_RES of component %d" % c)
            _same(_down(s, c, F.F_CORR, grids), first[c], "F_CORR of component %d across the refresh" % c)
        s.vcycleMulti(True)
        _reaches(s, 3, K, launches)
        got = [_down(s, c, F.F_CORR, grids) for c in range(3)]
    finally:
        s.undefine()
    fresh = handle(lay, prob2)
    try:
        for c in range(3):
            upload(fresh, F.F_RES, res[c])
            fresh.vcycleFromZero(F.F_CORR, F.F_RES)
            want = download_valid(fresh, F.F_CORR, grids)
            _same(got[c], want, "component %d after the refresh vs a fresh handle" % c)
            assert any(not np.array_equal(x, y) for x, y in zip(want, first[c]))   # (the two metrics do differ)
    finally:
        fresh.undefine()


# ---- 6. SpaceDim 2 --------------------------------------------------------------------------------------------------------------------
def test_2d_handle_accepts_three_components_and_batches_nothing(oracle):
    """the 9-point handle: no depth marches, K == 0, the capability is the shared metric alone"""
    from somar_amd import AMRPressureSolver
    from somar_amd import api as F
    so = oracle
    n, bs, per, L = (32, 32), 16, (False, False), (2.0, 1.0)
    dom = so.Domain(so.Box((0, 0, 0), (n[0] - 1, n[1] - 1, 0)), (per[0], per[1], False))
    grids = so.split_domain(dom.box, (bs, bs, 1))
    dx = (L[0] / n[0], L[1] / n[1], 1.0)
    Jgup, Jinv = so.make_full_metric_2d(grids, dx, L, dom)
    rhs = [so.random_field(grids, 11 + c, (0, 0, 0), dom.box) for c in range(3)]
    s = AMRPressureSolver()
    s.setSpaceDim(2)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=ALPHA, beta=BETA)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricFull(q, np.asfortranarray(Jgup[gi][0].a), np.asfortranarray(Jgup[gi][1].a), None,
                        np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    try:
        seq = []
        for c in range(3):
            upload(s, F.F_RHS, rhs[c])
            st = s.solveResident(zeroPhi=True)
            seq.append((download_valid(s, F.F_PHI, grids), dict(st)))
        s.setComponentsFull(3)
        assert s.getComponents() == (3, 0, 0)
        for c in range(3):
            _up(s, c, F.F_RHS, rhs[c])
        stats = s.solveMulti(zeroPhi=True)
        assert s.getComponents() == (3, 0, 0)
        for c in range(3):
            assert stats[c]["iters"] > 0
            _same(_down(s, c, F.F_PHI, grids), seq[c][0], "phi of component %d" % c)
            for k in STAT_KEYS:
                assert stats[c][k] == seq[c][1][k], (c, k)
    finally:
        s.undefine()


# ---- 7. the fused red+black 19-point sweep stays single-field ----------------------------------------------------------------------------
def test_depths_with_the_fused_19_point_sweep_are_not_batched(oracle, monkeypatch):
    from somar_amd import api as F
    monkeypatch.setenv("SOMAR_FUSED19_MIN_BOX", "0")
    so, lay = oracle, LAYOUTS["dirichlet-deep"]   # boxes of 16^3, then 8^3: both depths of more than SMALL cells take the fused sweep
    prob, res, seq, ora, _ = _cycle_refs(so, lay)   # (the references ran the two-pass kernels: the same bits, tests/test_gpu_full.py)
    grids = prob[1]
    s = handle(lay, prob)
    try:
        s.setComponentsFull(3)
        assert s.getComponents() == (3, 0, 0)
        swept = s.fused19Sweeps()
        for c in range(3):
            _up(s, c, F.F_RES, res[c])
        s.vcycleMulti(True)
        assert s.getComponents() == (3, 0, 0) and s.fused19Sweeps() > swept
        for c in range(3):
            _same(_down(s, c, F.F_CORR, grids), seq[c], "component %d vs the single-field cycle" % c)
    finally:
        s.undefine()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def _raises(fn, *words):
    from somar_amd import SomarError
    with pytest.raises(SomarError) as e:
        fn()
    msg = str(e.value)
    for w in words:
        assert w in msg, msg


def _still_cycles(s, grids, res):
    from somar_amd import api as F
    upload(s, F.F_RES, res)
    s.vcycleFromZero(F.F_CORR, F.F_RES)
    got = download_valid(s, F.F_CORR, grids)
    assert all(np.all(np.isfinite(g)) and float(np.max(np.abs(g))) > 0.0 for g in got)


def test_refusals(oracle):
    from somar_amd import AMRPressureSolver
    so, lay = oracle, LAYOUTS["seams"]
    prob = problem(so, lay)
    dom, grids, dx = prob[0], prob[1], prob[2]
    res = so.random_field(grids, 91, (0, 0, 0), dom.box)
    # a diagonal-metric handle: the message names the call that serves it
    diag = so.make_diagonal_metric(grids, dx, lay.L, 3, "stretched", domain=dom)
    s = AMRPressureSolver()
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=ALPHA, beta=BETA)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricOrtho(q, *[np.asfortranarray(diag[0][gi][d].a[..., d]) for d in range(3)], np.asfortranarray(diag[1][gi].a[..., 0]))
    s.finalize()
    try:
        _raises(lambda: s.setComponentsFull(2), "somar_solver_set_components")
        assert s.getComponents()[:2] == (1, 0)
        _still_cycles(s, grids, res)
    finally:
        s.undefine()
    # the 7-point call's reasons, in its words
    for kw, word in (({"relax": 0}, "relax_mode other than LevelGSRB"), ({"relax": 3}, "relax_mode other than LevelGSRB"),
                     ({"num_mg": 2}, "num_mg != 1")):
        s = handle(lay, prob, **kw)
        try:
            _raises(lambda: s.setComponentsFull(2), word)
            assert s.getComponents()[:2] == (1, 0)
            s.setComponentsFull(1)   # one component is always accepted
            _still_cycles(s, grids, res)
        finally:
            s.undefine()
    s = handle(lay, prob)
    try:
        _raises(lambda: s.setComponentsFull(5), "1 to 4")
        _raises(lambda: s.setComponentsFull(0), "1 to 4")
        _raises(lambda: s.setComponents(2), "non-diagonal")
        _still_cycles(s, grids, res)
        s.setComponentsFull(2)
        _raises(lambda: s.setCompOp(1, [D] * 6, [0.0] * 6, 1.0, -0.02), "non-diagonal")
        _raises(lambda: s.setComponents(2), "non-diagonal")   # its present error, whichever call created the components
        assert s.getComponents()[:2] == (2, expected_K(s, lay))
        with s.metricUpdate():
            _raises(lambda: s.setComponentsFull(3), "metric update")
        assert s.getComponents()[0] == 2
        _still_cycles(s, grids, res)
        s.setComponents(1)   # ... and still releases them
        assert s.getComponents()[:2] == (1, 0)
        _still_cycles(s, grids, res)
    finally:
        s.undefine()
