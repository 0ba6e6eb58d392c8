"""Several components on one operator (somar_solver_set_components): the N-field sweep, residual + restriction and residual
kernels (multi_march.hip) and the lock-step solve, against the single-field path of the SAME handle, bit for bit -- the
specification of solveMulti is that it leaves every component as successive single-field calls would -- and, for one component
other than 0, against the oracle's one_cycle, bit for bit, which is the standard the parity tests hold the single-field
kernels to.

Layouts: the ones tests/test_gpu_mixed_kernels.py reasons about (the smallest at which the marching kernels can go wrong),
here with a Helmholtz operator (alpha = 1, beta = -0.01: no null space, so every large depth is batched): the 128-wide box
with narrow (124 + 4, 60 + 4) and equal columns in the level's own tables -- the N-field launches bring class-0 tables of
their own, the odd component of a 2 + 1 restriction takes the level's -- and with six Dirichlet sides; the ragged four-box
layout, periodic in x and y; the semicoarsened layout with ratios (1, 2, 2) then (2, 2, 2).

Layouts chosen for the N-field path itself, where it differs from the single-field one:
  * extra-wide, extra-wide-dirichlet (256 x 24 x 24, one box; each also as *-equal-tables with SOMAR_NO_NARROW_TILES=1): the
    N-field launches of depth 0 run three class-0 columns 86 / 86 / 84 of their own table, the last one cut by the box and not
    by the tile's width, while the level's own sweep table -- which the folded-prolongation sweep and the odd component of a
    2 + 1 restriction take -- holds tall class-1 tiles (default) or the same equal columns (switch).  One V-cycle mixes the
    two tilings of the same cells.  As in tests/test_gpu_tall_tiles.py the library exports no tile table: the default run
    asserts the tall rule's inputs (assert_tall_rule), and tests/test_march_plan.py pins the N-field tables on the CPU.
    Four batched depths, ratios (2, 1, 1) x 3 then (2, 2, 2).
  * wide-mixed-sides: the 128-wide box with one Dirichlet and one Neumann side in every direction -- the boundary predicates
    the N-field kernels restate (P.neum || (DIRI && P.diri) per side; the Neumann edge flags of the residual).
  * ragged-mixed-sides: the four ragged boxes with Dirichlet and Neumann sides that run across the box seams in x and y, where
    the tests on the global index (g < P.dom_lo) decide and the local one does not.
  * ragged-periodic-dirichlet-z: periodic seams in x and y with a Dirichlet direction (DIRI instantiations, periodic wrap).
  * ratio-212, ratio-221, ratio-112: the restriction ratios (2, 1, 2), (2, 2, 1) and (1, 1, 2), whose leader / hand-over /
    first / last logic in accumulate() branches on each direction separately and had run only as (2, 1, 1), (2, 2, 2) and
    (1, 2, 2).

What the valid region cannot show, and what stands in for it:
  * the cut of extra-wide's last column by the box: uncut, the sweep stores into the ghost columns 256 and 257, which every
    reader refills or ignores.  test_vcycle_multi_leaves_the_ghost_cells_as_the_single_field_cycle compares the ghost layer.
  * the `P.neum ||` / `DIRI && P.diri` terms of the sweep's ring predicate (comp_ij): they keep the red pass from updating a
    ghost cell beyond a physical side.  gsrb_point never uses that cell's value -- a Neumann face contributes no flux, a
    Dirichlet face's ghost is -own -- and the ring lives in LDS only, so with one term removed every field keeps every bit
    (tried: all of this file passes).  What a wrong side or a local index in place of the global one does change is the
    residual's Neumann flags and the classification inside gsrb_point, and there the mixed-sides layouts fail while the
    symmetric ones pass (tried with the x-low flag taken from the x-high side).

Every case first proves it reaches its target: batched_depths equals the expected K, batched_launches grew, the MG ratios are
the oracle's and begin with the ratios the layout is there for, and the boxes of every batched depth have the stated widths.
A case that silently fell back to the single-field path, or whose hierarchy coarsens otherwise, fails instead of passing
vacuously.

One refusal of the list cannot be reached from a one-level Python handle and is held by tests/test_multi_exports.py on the
text of multi_refusal: coarse-fine faces exist only on the levels of a hierarchy, which are refused as such first."""
import numpy as np
import pytest

from tests.helpers import download_valid, make_problem, upload
from tests.test_gpu_mixed_kernels import (RAGGED_BOXES, RAGGED_N, WIDE_BOX, WIDE_N, WIDE_RATIOS, Case, gpu_solver, oracle_cycle,
                                          problem, set_env)
from tests.test_gpu_tall_tiles import assert_tall_rule

pytestmark = pytest.mark.gpu

D, N = 1, 0
ALPHA, BETA = 1.0, -0.01
BC_VALUES = [0.25, -0.5, 0.75, 0.1, -0.3, 0.6]


def _case(name, n, boxes, periodic, L, bc, narrow, K, variant="stretched", alpha=ALPHA, beta=BETA, widths=None, ratios=None,
          tables=None, ref=None):
    """widths: the sorted box widths of every batched depth; ratios: the MG ratios the hierarchy must begin with; tables: None,
    or "tall" / "equal" -- the level's own sweep table of a depth wider than 128 (SOMAR_NO_NARROW_TILES unset / 1); ref: the
    layout whose references (_cycle_refs) serve this one -- the same problem under the other table, the same bits"""
    c = Case(name, n, boxes, variant, periodic, L, bc, alpha, beta, narrow, K, widths, ratios, None)
    c.tables, c.ref = tables, ref or name
    return c


WIDE_WIDTHS = [[128], [64], [32]]
RAGGED_WIDTHS = [[32, 32, 48, 48], [16, 16, 24, 24]]
XWIDE_N = (256, 24, 24)                       # 147456 cells; 128 x 24 x 24, 64 x 24 x 24, 32 x 24 x 24, then 16 x 12 x 12 replayed
XWIDE_BOX = [((0, 0, 0), (255, 23, 23))]
XWIDE_WIDTHS = [[256], [128], [64], [32]]
XWIDE_RATIOS = [(2, 1, 1)] * 3 + [(2, 2, 2)]
LAYOUTS = {c.name: c for c in [
    _case("wide-narrow", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), None, "1", 3, widths=WIDE_WIDTHS, ratios=WIDE_RATIOS),
    _case("wide-equal", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), None, "0", 3, widths=WIDE_WIDTHS, ratios=WIDE_RATIOS),
    _case("wide-dirichlet", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), [D] * 6, None, 3, widths=WIDE_WIDTHS,
          ratios=WIDE_RATIOS),
    _case("ragged", RAGGED_N, RAGGED_BOXES, (True, True, False), (1.25, 1.0, 0.5), None, None, 2, widths=RAGGED_WIDTHS,
          ratios=[(2, 2, 2)] * 2),
    _case("anisotropic", (64, 32, 16), 32, (False, True, False), (4.0, 1.0, 0.5), None, None, 2, widths=[[32, 32]] * 2,
          ratios=[(1, 2, 2), (2, 2, 2)]),
    # ---- the N-field path's own corners (module docstring) ----
    _case("extra-wide", XWIDE_N, XWIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), None, None, 4, widths=XWIDE_WIDTHS,
          ratios=XWIDE_RATIOS, tables="tall"),
    _case("extra-wide-equal-tables", XWIDE_N, XWIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), None, None, 4, widths=XWIDE_WIDTHS,
          ratios=XWIDE_RATIOS, tables="equal", ref="extra-wide"),
    _case("extra-wide-dirichlet", XWIDE_N, XWIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), [D] * 6, None, 4, widths=XWIDE_WIDTHS,
          ratios=XWIDE_RATIOS, tables="tall"),
    _case("extra-wide-dirichlet-equal-tables", XWIDE_N, XWIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), [D] * 6, None, 4,
          widths=XWIDE_WIDTHS, ratios=XWIDE_RATIOS, tables="equal", ref="extra-wide-dirichlet"),
    _case("wide-mixed-sides", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), [D, N, N, D, D, N], None, 3, widths=WIDE_WIDTHS,
          ratios=WIDE_RATIOS),
    _case("ragged-mixed-sides", RAGGED_N, RAGGED_BOXES, (False,) * 3, (1.25, 1.0, 0.5), [N, D, D, N, D, D], None, 2,
          widths=RAGGED_WIDTHS, ratios=[(2, 2, 2)] * 2),
    _case("ragged-periodic-dirichlet-z", RAGGED_N, RAGGED_BOXES, (True, True, False), (1.25, 1.0, 0.5), [N, N, N, N, D, D], None,
          2, widths=RAGGED_WIDTHS, ratios=[(2, 2, 2)] * 2),
    # 64 x 16 x 64 in four boxes 32 x 16 x 32: dx = 1/64, 1/16, 1/64 -> (2, 1, 2) twice, then 16^3 (4096 cells: replayed)
    _case("ratio-212", (64, 16, 64), 32, (False,) * 3, (1.0, 1.0, 1.0), None, None, 2, widths=[[32] * 4, [16] * 4],
          ratios=[(2, 1, 2), (2, 1, 2)]),
    # 64 x 64 x 16 in four boxes 32 x 32 x 16: dx = 1/64, 1/64, 1/32 -> (2, 2, 1), then (2, 2, 2) to 16 x 16 x 8 (replayed)
    _case("ratio-221", (64, 64, 16), 32, (False,) * 3, (1.0, 1.0, 0.5), None, None, 2, widths=[[32] * 4, [16] * 4],
          ratios=[(2, 2, 1), (2, 2, 2)]),
    # 32 x 32 x 64 in two boxes of 32^3: dx = 1/32, 1/32, 1/64 -> (1, 1, 2), then (2, 2, 2) to 16^3 (replayed)
    _case("ratio-112", (32, 32, 64), 32, (False,) * 3, (1.0, 1.0, 1.0), None, None, 2, widths=[[32] * 2, [32] * 2],
          ratios=[(1, 1, 2), (2, 2, 2)]),
]}


@pytest.fixture(autouse=True)
def _large_level_kernels(monkeypatch):
    set_env(monkeypatch.setenv)
    for k in ("SOMAR_NARROW_7PT", "SOMAR_NO_NARROW_TILES", "SOMAR_FUSED_ROWS", "SOMAR_ORDERED_REDUCE_MAX"):
        monkeypatch.delenv(k, raising=False)


def _narrow_env(monkeypatch, case):
    if case.narrow is not None:
        monkeypatch.setenv("SOMAR_NARROW_7PT", case.narrow)
    if case.tables == "equal":
        monkeypatch.setenv("SOMAR_NO_NARROW_TILES", "1")


def _up(s, comp, field, ld):
    for p in range(s.num_local_patches):
        _, _, gi = s.patch_box(p)
        s.uploadComp(comp, field, p, np.asfortranarray(ld[gi].a[..., 0]), ld.ghost)


def _down(s, comp, field, grids):
    out = [None] * len(grids)
    for p in range(s.num_local_patches):
        _, _, gi = s.patch_box(p)
        out[gi] = s.downloadComp(comp, field, p, (0, 0, 0))
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


def _reaches_layout(s, case, K, oracle_ratios):
    """the hierarchy is the one the layout is there for: the oracle's MG ratios, beginning with the case's; the box widths of
    every batched depth; where the level's own sweep table matters, the inputs of the tall rule (the table itself is not
    exported: tests/test_gpu_tall_tiles.py says what that leaves open, tests/test_march_plan.py pins the tables on the CPU)"""
    assert s.mgRefRatios() == oracle_ratios, (s.mgRefRatios(), oracle_ratios)
    assert s.mgRefRatios()[:len(case.ratios)] == case.ratios, s.mgRefRatios()
    for d in range(K):
        widths = sorted(s.patch_box(q, d)[1][0] - s.patch_box(q, d)[0][0] + 1 for q in range(s.num_local_patches))
        assert widths == case.widths[d], (d, widths)
    if case.tables == "tall":
        assert_tall_rule(s, None)
    elif case.tables == "equal":
        assert s.tuning("NO_NARROW_TILES") == 1 and s.metricUniform(0) is None


# ---- 1. the V-cycle kernels -------------------------------------------------------------------------------------------------
_CYCLE_REFS = {}


def _cycle_refs(so, case, sweeps):
    """per component seed: the residual field and its single-field V-cycle from zero on a handle of one component; for
    component 1 the oracle's one_cycle too.  Computed once per (layout, sweeps) and left unchanged."""
    from somar_amd import api as F
    key = (case.ref, sweeps)
    if key not in _CYCLE_REFS:
        prob = problem(so, case)
        dom, grids = prob[0], prob[1]
        res = [so.random_field(grids, 5 + c, (0, 0, 0), dom.box) for c in range(4)]
        s = gpu_solver(case, prob, sweeps=sweeps)
        try:
            assert s.getComponents()[:2] == (1, 0)
            seq = []
            for c in range(4):
                upload(s, F.F_RES, res[c])
                s.vcycleFromZero(F.F_CORR, F.F_RES)
                seq.append(download_valid(s, F.F_CORR, grids))
            assert s.getComponents()[2] == 0   # the single-field path issues no N-field launch
        finally:
            s.undefine()
        ora, oratios = oracle_cycle(so, case, prob, res[1], sweeps)
        _CYCLE_REFS[key] = (prob, res, seq, ora, oratios)
    return _CYCLE_REFS[key]


@pytest.mark.parametrize("ncomp", [2, 3, 4])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_vcycle_multi_is_the_single_field_cycle_per_component(oracle, monkeypatch, name, ncomp):
    from somar_amd import api as F
    so, case = oracle, LAYOUTS[name]
    _narrow_env(monkeypatch, case)
    # K = 1 with one sweep per side: one sweep from zero on two or three fields (four: 2 + 2), one residual + restriction on
    # two (three: 2 + 1 with the level's own table), the folded prolongation sweep field by field; then the full K with 2/2/2
    # sweeps: plain two-field sweeps too (three: 2 + 1), and the batched depths below 0
    for sweeps, full_K in ((1, False), (2, True)):
        prob, res, seq, ora, oratios = _cycle_refs(so, case, sweeps)
        grids = prob[1]
        s = gpu_solver(case, prob, sweeps=sweeps)
        try:
            K = case.K if full_K else 1
            s.setComponents(ncomp, 0 if full_K else s.levelInfo(0)["cells"])   # depth 0 alone reaches min_cells
            _reaches_layout(s, case, K, oratios)
            for c in range(ncomp):
                _up(s, c, F.F_RES, res[c])
            s.vcycleMulti(True)
            _reaches(s, ncomp, K, 0)
            got = [_down(s, c, F.F_CORR, grids) for c in range(ncomp)]
        finally:
            s.undefine()
        for c in range(ncomp):
            assert all(float(np.max(np.abs(g))) > 0.0 for g in got[c])
            _same(got[c], seq[c], "%s K=%d %d/%d/%d component %d of %d vs the single-field cycle" % (
                name, K, sweeps, sweeps, sweeps, c, ncomp))
        _same(got[1], ora, "%s K=%d component 1 of %d vs the oracle's one_cycle" % (name, K, ncomp))


GHOST_MARK = 7.5   # what the caller leaves in the ghost cells of a given correction


def _given_correction(so, case, ghost=(0, 0, 0)):
    """ghost: how much of the ghost layer is compared too.  The caller's ghost cells hold GHOST_MARK + the component."""
    from somar_amd import api as F
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    res = [so.random_field(grids, 21 + c, (0, 0, 0), dom.box) for c in range(3)]
    cor = [so.random_field(grids, 31 + c, (1, 1, 1), dom.box) for c in range(3)]
    for c in range(3):
        for g, f in zip(grids, cor[c].fabs):
            valid = np.array(f.view(g))
            f.a[...] = GHOST_MARK + c
            f.view(g)[...] = valid
    s = gpu_solver(case, prob)
    try:
        seq = []
        for c in range(3):
            upload(s, F.F_RES, res[c])
            upload(s, F.F_CORR, cor[c])
            s.vcycle(F.F_CORR, F.F_RES)
            seq.append([s.download(F.F_CORR, q, ghost) for q in range(s.num_local_patches)])
        s.setComponents(3)
        for c in range(3):
            _up(s, c, F.F_RES, res[c])
            _up(s, c, F.F_CORR, cor[c])
        s.vcycleMulti(False)
        _reaches(s, 3, case.K, 0)
        got = [[s.downloadComp(c, F.F_CORR, q, ghost) for q in range(s.num_local_patches)] for c in range(3)]
        for c in range(3):
            _same(got[c], seq[c], "%s, component %d" % (case.name, c))
        return got
    finally:
        s.undefine()


def test_vcycle_multi_on_a_given_correction(oracle):
    """from_zero = False: the first pre-smoothing sweep reads the correction (plain sweeps on depth 0), as somar_vcycle"""
    _given_correction(oracle, LAYOUTS["wide-dirichlet"])


def test_vcycle_multi_on_a_given_correction_with_mixed_sides(oracle):
    """the same with one Dirichlet and one Neumann side per direction: nothing fills the given correction's ghost cells on the
    Neumann sides, they hold the caller's mark, which the sweeps must not read"""
    _given_correction(oracle, LAYOUTS["wide-mixed-sides"])


def test_vcycle_multi_leaves_the_ghost_cells_as_the_single_field_cycle(oracle):
    """extra-wide, every side Neumann, the ghost layer compared too.  No exchange and no boundary condition writes the ghost
    cells of this box, and an even number of sweeps per side (2/2/2) ends in the caller's array: the single-field cycle leaves
    them as the caller uploaded them, and so must the N-field sweeps.  This is what the cut of the last of the three columns by
    the box (l < n0; the tile's width 86 reaches two cells past it) is for: without it the sweep stores into the ghost columns
    256 and 257, which no valid cell of a cycle ever reads back -- the valid region alone cannot show it."""
    case = LAYOUTS["extra-wide"]
    got = _given_correction(oracle, case, ghost=(1, 1, 1))
    for c in range(3):
        (a,) = got[c]
        assert a.shape == tuple(n + 2 for n in case.n)
        for face in (a[0], a[-1], a[:, 0], a[:, -1], a[:, :, 0], a[:, :, -1]):
            np.testing.assert_array_equal(face, GHOST_MARK + c)


# ---- 2. solves ----------------------------------------------------------------------------------------------------------------
STAT_KEYS = ("iters", "exitStatus", "status", "bottom_iters", "bottom_exit", "initial_rnorm", "final_rnorm", "history")
# The solves stop on the ABSOLUTE residual norm (norm_thresh) or on imax; eps is out of reach.  A V-cycle of these cases
# contracts the residual by 0.2 - 0.3 (measured), and certainly by a factor between 0.05 and 0.5: the small smooth right-hand
# side, 30 NORM_THRESH in the max norm, then falls below NORM_THRESH within 2 to 5 cycles, while the random one, of order one,
# is 12 decades away and runs into IMAX.
IMAX, NORM_THRESH, EPS = 8, 1e-12, 1e-30


def _smooth_field(so, grids, dom, n, amplitude):
    f = so.LevelData(grids, 1, (0, 0, 0))
    for g, fab in zip(grids, f.fabs):
        i, j, k = np.meshgrid(*[np.arange(g.lo[d], g.hi[d] + 1) for d in range(3)], indexing="ij")
        fab.view(g)[..., 0] = amplitude * (np.cos(np.pi * (i + 0.5) / n[0]) * np.cos(np.pi * (j + 0.5) / n[1]) *
                                           np.cos(np.pi * (k + 0.5) / n[2]))
    return f


def _solve_rhs(so, case, prob):
    """a small smooth rhs (few cycles: goNorm), a rhs identically zero (no cycle; not first, so that the bottom counts it
    reports are the component's before it on either path) and a random one that IMAX stops (goIter): the active set shrinks
    twice"""
    dom, grids = prob[0], prob[1]
    zero = so.LevelData(grids, 1, (0, 0, 0))
    return [_smooth_field(so, grids, dom, case.n, 30 * NORM_THRESH), zero, so.random_field(grids, 11, (0, 0, 0), dom.box)]


def _solver(case, prob, eps, imax, bc_values=None, norm_thresh=None):
    """gpu_solver of tests/test_gpu_mixed_kernels.py (2/2/2 sweeps), with Dirichlet values"""
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv = prob
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh if norm_thresh is None else norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=case.alpha, beta=case.beta,
             bc_type=case.bc)
    if bc_values is not None:
        s.setBCValues(bc_values)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                         np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return s


def _solve_both_ways(so, case, zero_phi, force_homogeneous, bc_values=None, expect_K=None, face_values=None, phi_out=None):
    """face_values: {(dir, side): plane} for setBCFaceValues; phi_out: a list that receives every component's phi"""
    from somar_amd import api as F
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    rhs = _solve_rhs(so, case, prob)
    guess = [so.random_field(grids, 51 + c, (1, 1, 1), dom.box) for c in range(3)]
    s = _solver(case, prob, EPS, IMAX, bc_values, NORM_THRESH)
    try:
        for (d, side), plane in sorted((face_values or {}).items()):
            s.setBCFaceValues(d, side, plane)
        seq = []
        for c in range(3):
            upload(s, F.F_RHS, rhs[c])
            if not zero_phi:
                upload(s, F.F_PHI, guess[c])
            st = s.solveResident(zeroPhi=zero_phi, forceHomogeneous=force_homogeneous)
            seq.append((download_valid(s, F.F_PHI, grids), dict(st), [float(v) for v in F.last_history()]))
        s.setComponents(3)
        for c in range(3):
            _up(s, c, F.F_RHS, rhs[c])
            if not zero_phi:
                _up(s, c, F.F_PHI, guess[c])
        stats = s.solveMulti(zeroPhi=zero_phi, forceHomogeneous=force_homogeneous)
        K = case.K if expect_K is None else expect_K
        if K > 0:
            _reaches(s, 3, K, 0)
        else:
            assert s.getComponents() == (3, 0, 0)
        for c in range(3):
            print("%s component %d: %d V-cycles, exit %d, bottom %d/%d, final/initial %.3e" % (
                case.name, c, stats[c]["iters"], stats[c]["exitStatus"], stats[c]["bottom_iters"], stats[c]["bottom_exit"],
                stats[c]["final_rnorm"] / max(stats[c]["initial_rnorm"], 1e-300)))
            _same(_down(s, c, F.F_PHI, grids), seq[c][0], "phi of component %d" % c)
            for k in STAT_KEYS:
                assert stats[c][k] == seq[c][1][k], (c, k, stats[c][k], seq[c][1][k])
            assert s.compHistory(c) == seq[c][2], c
        if phi_out is not None:
            phi_out.extend(seq[c][0] for c in range(3))
    finally:
        s.undefine()
    return stats


def _assert_active_set_shrinks(stats):
    a, z, r = stats[0]["iters"], stats[1]["iters"], stats[2]["iters"]
    assert z == 0 and 0 < a < r == IMAX, (a, z, r)
    assert stats[0]["exitStatus"] == 8 and stats[1]["exitStatus"] & 8 and stats[2]["exitStatus"] == 2, stats


@pytest.mark.parametrize("zero_phi", [True, False])
@pytest.mark.parametrize("name", ["wide-narrow", "ragged", "extra-wide", "ragged-mixed-sides"])
def test_solve_multi_is_three_solves(oracle, monkeypatch, name, zero_phi):
    """(ragged-mixed-sides: with constant values on its Dirichlet sides -- those of the Neumann sides are ignored -- so the
    right-hand side identically zero is no longer a solve without a cycle, and the active set is not asserted to shrink)"""
    case = LAYOUTS[name]
    _narrow_env(monkeypatch, case)
    values = BC_VALUES if case.bc is not None else None
    stats = _solve_both_ways(oracle, case, zero_phi, False, bc_values=values)
    if zero_phi and values is None:
        _assert_active_set_shrinks(stats)


@pytest.mark.parametrize("force_homogeneous", [False, True])
def test_solve_multi_with_dirichlet_values(oracle, force_homogeneous):
    stats = _solve_both_ways(oracle, LAYOUTS["wide-dirichlet"], True, force_homogeneous, bc_values=BC_VALUES)
    if force_homogeneous:
        _assert_active_set_shrinks(stats)


def test_component_without_a_cycle_first_reports_the_counts_before_the_call(oracle):
    """A solve that runs no cycle reports the bottom solver's counts as the solve before it left them.  With the component
    that runs none FIRST, those are the counts before the call -- not the last cycle of a component that, solved one after
    the other, would come later.  Two fresh handles, so both paths start from the same counts (none: 0 / 0)."""
    from somar_amd import api as F
    so, case = oracle, LAYOUTS["ragged"]
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    smooth, zero, rand = _solve_rhs(so, case, prob)
    rhs = [zero, rand, zero, smooth]   # no cycle first; and one between two that cycle
    a = _solver(case, prob, EPS, IMAX, None, NORM_THRESH)
    try:
        seq = []
        for c in range(4):
            upload(a, F.F_RHS, rhs[c])
            seq.append(dict(a.solveResident(zeroPhi=True)))
    finally:
        a.undefine()
    b = _solver(case, prob, EPS, IMAX, None, NORM_THRESH)
    try:
        b.setComponents(4)
        for c in range(4):
            _up(b, c, F.F_RHS, rhs[c])
        stats = b.solveMulti(zeroPhi=True)
        _reaches(b, 4, case.K, 0)
        # a second call on the same handle starts from the counts the first one left: those of the last component that cycled
        again = b.solveMulti(zeroPhi=True)
    finally:
        b.undefine()
    assert [x["iters"] for x in seq] == [0, IMAX, 0, seq[3]["iters"]] and 0 < seq[3]["iters"] < IMAX, seq
    assert (seq[0]["bottom_iters"], seq[0]["bottom_exit"]) == (0, 0) and seq[1]["bottom_iters"] > 0, seq
    assert (seq[2]["bottom_iters"], seq[2]["bottom_exit"]) == (seq[1]["bottom_iters"], seq[1]["bottom_exit"])
    for c in range(4):
        for k in STAT_KEYS:
            assert stats[c][k] == seq[c][k], (c, k, stats[c][k], seq[c][k])
    assert (again[0]["bottom_iters"], again[0]["bottom_exit"]) == (seq[3]["bottom_iters"], seq[3]["bottom_exit"])
    for c in range(1, 4):
        assert (again[c]["bottom_iters"], again[c]["bottom_exit"]) == (seq[c]["bottom_iters"], seq[c]["bottom_exit"]), c


def test_solve_multi_without_graphs(oracle, monkeypatch):
    """SOMAR_GRAPH_CELLS = 0: no graph-replayed legs, so the batched depths end where the serial-order sums begin"""
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", "0")
    case = LAYOUTS["wide-equal"]
    _narrow_env(monkeypatch, case)
    # 128x48x48, 64x48x48, 32x24x24, 16x12x12 (2304 cells: serial-order sums, not batched)
    _assert_active_set_shrinks(_solve_both_ways(oracle, case, True, False, expect_K=3))


# ---- 3. heat steps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_heat_step_multi_is_three_heat_steps(oracle, scheme):
    from somar_amd import api as F
    so = oracle
    case = _case("wide-dirichlet-heat", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), [D] * 6, None, 3, alpha=1.0, beta=1.0)
    prob = problem(so, case)
    dom, grids = prob[0], prob[1]
    old = [so.random_field(grids, 61 + c, (1, 1, 1), dom.box) for c in range(3)]
    src = [so.random_field(grids, 71 + c, (0, 0, 0), dom.box) for c in range(3)]
    dt = 0.01   # (I - dt L): the Helmholtz operator of the V-cycle cases
    s = _solver(case, prob, 1e-8, 20, BC_VALUES)   # (the apply_op stages take the inhomogeneous values)
    try:
        seq = []
        for c in range(3):
            upload(s, F.F_HEAT_OLD, old[c])
            upload(s, F.F_HEAT_SRC, src[c])
            st = s.heatStep(scheme, dt, zeroPhi=True)
            seq.append((download_valid(s, F.F_PHI, grids), dict(st)))
        s.setComponents(3)
        for c in range(3):
            _up(s, c, F.F_HEAT_OLD, old[c])
            _up(s, c, F.F_HEAT_SRC, src[c])
        stats = s.heatStepMulti(scheme, dt, zeroPhi=True)
        _reaches(s, 3, case.K, 0)
        for c in range(3):
            assert stats[c]["iters"] > 0
            _same(_down(s, c, F.F_PHI, grids), seq[c][0], "scheme %d, phi of component %d" % (scheme, c))
            for k in STAT_KEYS:
                assert stats[c][k] == seq[c][1][k], (scheme, c, k)
    finally:
        s.undefine()


# ---- 4. K = 0: nothing batched, the calls are loops over the single-field ones -------------------------------------------------
FALLBACKS = {c.name: c for c in [
    _case("cartesian", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), None, None, 0, variant="cartesian"),       # uniform metric
    _case("poisson-neumann", WIDE_N, WIDE_BOX, (False,) * 3, (1.0, 1.0, 1.0), None, None, 0, alpha=0.0, beta=1.0),  # zero-average depths
    _case("small", (16, 16, 16), 16, (False,) * 3, (1.0, 1.0, 1.0), None, None, 0),                                # nothing large
]}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallbacks_accept_three_components(oracle, name):
    so, case = oracle, FALLBACKS[name]
    if case.null_space:
        # a compatible right-hand side per component
        from somar_amd import api as F
        prob = problem(so, case)
        dom, grids, Jinv = prob[0], prob[1], prob[4]
        rhs = [so.random_field(grids, 81 + c, (0, 0, 0), dom.box) for c in range(3)]
        for r in rhs:
            so.remove_weighted_mean(r, Jinv)
        s = gpu_solver(case, prob, eps=1e-8, imax=IMAX)
        try:
            assert s.zeroAvg(0)
            seq = []
            for c in range(3):
                upload(s, F.F_RHS, rhs[c])
                st = s.solveResident(zeroPhi=True)
                seq.append((download_valid(s, F.F_PHI, grids), dict(st)))
            s.setComponents(3)
            for c in range(3):
                _up(s, c, F.F_RHS, rhs[c])
            stats = s.solveMulti(zeroPhi=True)
            assert s.getComponents() == (3, 0, 0)
            for c in range(3):
                _same(_down(s, c, F.F_PHI, grids), seq[c][0], "phi of component %d" % c)
                for k in STAT_KEYS:
                    assert stats[c][k] == seq[c][1][k], (c, k)
        finally:
            s.undefine()
        return
    _solve_both_ways(so, case, True, False, expect_K=0)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def _raises(fn, *words):
    from somar_amd import SomarError
    with pytest.raises(SomarError) as e:
        fn()
    msg = str(e.value)
    for w in words:
        assert w in msg, msg


def _small(so, relaxMode=1, numMG=1, full=False):
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 32, 32), 16, "stretched")
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, relaxMode, numMG, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=ALPHA, beta=BETA)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        if full:
            jg = []
            for d in range(3):
                a = np.zeros(Jgup[gi][d].a.shape[:3] + (3,), order="F")
                a[..., d] = Jgup[gi][d].a[..., d]
                jg.append(a)
            s.setMetricFull(q, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
        else:
            s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                             np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    rhs = so.random_field(grids, 91, (0, 0, 0), dom.box)
    return s, grids, rhs


def _still_solves(s, grids, rhs):
    from somar_amd import api as F
    upload(s, F.F_RHS, rhs)
    st = s.solveResident(zeroPhi=True)
    assert st["iters"] > 0 and st["final_rnorm"] < st["initial_rnorm"]


def _still_cycles(s, grids, rhs):
    """(a Jacobi or line-relaxed handle: one V-cycle; whether its solve converges is not this test's business)"""
    from somar_amd import api as F
    upload(s, F.F_RES, rhs)
    s.vcycleFromZero(F.F_CORR, F.F_RES)
    got = download_valid(s, F.F_CORR, grids)
    assert all(np.all(np.isfinite(g)) and float(np.max(np.abs(g))) > 0.0 for g in got)


def test_refusals(oracle):
    so = oracle
    for kw, word in (({"relaxMode": 0}, "relax_mode"), ({"relaxMode": 3}, "relax_mode"), ({"numMG": 2}, "num_mg"),
                     ({"full": True}, "non-diagonal")):
        s, grids, rhs = _small(so, **kw)
        try:
            _raises(lambda: s.setComponents(2), word)
            assert s.getComponents()[:2] == (1, 0)
            s.setComponents(1)   # one component is always accepted
            _still_cycles(s, grids, rhs)
        finally:
            s.undefine()
    # the two call orders with mixed precision
    s, grids, rhs = _small(so)
    try:
        _raises(lambda: s.setComponents(5), "1 to 4")
        _raises(lambda: s.setComponents(0), "1 to 4")
        s.setComponents(2)
        _raises(lambda: s.setPrecision(1), "more than one component")
        s.setComponents(1)
        s.setPrecision(1)
        _raises(lambda: s.setComponents(2), "set_precision")
        _still_solves(s, grids, rhs)
        s.setPrecision(0)
        s.setComponents(2)
        with s.metricUpdate():
            _raises(lambda: s.setComponents(3), "metric update")
        assert s.getComponents()[0] == 2
    finally:
        s.undefine()
    # a level of an AMR hierarchy with two levels (the fine one has the coarse-fine faces)
    from somar_amd import AMRPressureSolver
    h = AMRPressureSolver()
    h.defineAMR((0, 0, 0), (15, 15, 15), (False, False, False), (1 / 16.0,) * 3, [(2, 2, 2)],
                [[((0, 0, 0), (15, 15, 15))], [((8, 8, 8), (23, 23, 23))]])
    try:
        for lv in h.levels:
            _raises(lambda: lv.setComponents(2), "AMR")
    finally:
        h.undefine()
    # the handles of a leptic solver
    from somar_amd.api import LevelLepticSolver
    lep = LevelLepticSolver()
    lep.define((0, 0, 0), (15, 15, 7), (False, False, False), (1 / 16.0, 1 / 16.0, 1 / 16.0), [((0, 0, 0), (15, 15, 7))])
    try:
        _raises(lambda: lep.level.setComponents(2), "leptic")
    finally:
        lep.undefine()


def _worker_two_ranks(rank, nranks, name, q, slots, barrier):
    import traceback
    try:
        from tests import test_gpu_mixed_multirank as M
        M._setup_env("replicated")
        from oracle import somar_oracle as so
        from somar_amd import api as F
        comm = F.comm_create_shm(name, rank, nranks)
        case = M._case("neumann")
        prob = make_problem(so, case[1], case[2], "stretched", case[3], (1.0, 1.0, 1.0))
        dom, grids, dx, Jgup, Jinv = prob
        owner = [i % nranks for i in range(len(grids))]
        s = M._solver(case, prob, owner, comm)
        _raises(lambda: s.setComponents(2), "more than one rank")
        assert s.getComponents()[:2] == (1, 0)
        s.setComponents(1)
        st = M._solve(s, grids, M._rhs(so, case, dom, grids, Jinv, seed=11))[1]   # (collective: both ranks solve)
        assert st["exitStatus"] & 1
        s.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok", []))
    except Exception:
        q.put((rank, traceback.format_exc(), []))


def test_refused_on_more_than_one_rank():
    from tests.test_gpu_mixed_multirank import _run
    _run(_worker_two_ranks, 2)


# ---- 6. memory ------------------------------------------------------------------------------------------------------------------
def test_components_hold_and_release_device_memory(oracle):
    from somar_amd import api as F
    so, case = oracle, LAYOUTS["anisotropic"]
    prob = problem(so, case)
    base = F.device_bytes_live()
    s = gpu_solver(case, prob)
    try:
        one = F.device_bytes_live()
        assert one > base
        s.setComponents(3)
        assert s.getComponents()[:2] == (3, case.K)
        three = F.device_bytes_live()
        elems = s.levelInfo(0)["field_elems"]
        assert three - one >= 2 * 5 * 8 * elems   # two more components: five depth-0 fields each, at least
        s.setComponents(1)
        assert F.device_bytes_live() == one
        s.setComponents(3)
        assert F.device_bytes_live() == three
        s.setComponents(3)
        assert F.device_bytes_live() == three
    finally:
        s.undefine()
    assert F.device_bytes_live() == base
