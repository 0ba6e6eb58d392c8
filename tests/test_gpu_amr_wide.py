"""AMR levels as wide as the bench hierarchies' (C3 / C4: 128-wide boxes, C5: 64-wide) on the GPU vs oracle/somar_amr.py.

What only a wide REFINED level reaches: a class-0 tile column plus a 4-wide class-4 remainder (128 -> 124 + 4) and a class-1
column plus the remainder (64 -> 60 + 4) in the marching tile tables, with the x-low coarse-fine face in lane 0 of the first
column and the x-high one inside the class-4 column; the coarse-fine ghosts made inside the fused sweep; residual +
restriction in one marching pass; the ring-only coarse-fine gather and the register-face fluxes on those columns.  The other
AMR parity modules stop at 32-wide boxes (one class-1 column, equal columns or two class-4 columns).  The lean interior-tile
body of the uniform-metric fused sweep never runs here (every box spans the periodic y extent, and every tile column touches
a coarse-fine x face or is class 4): what these cases show of it is that its per-tile test does not wrongly answer "interior"
next to a coarse-fine face; the body itself is covered on single levels (test_gpu_parity.py, test_gpu_uniform_metric.py).

The hierarchies are the smallest with such levels, thin in y and z:
  A   base 96 x 8 x 8 (one class-0 column of a width in (76, 124)), level 1 one 128-wide box, level 2 one 64-wide box;
      Cartesian (uniform-metric kernels, narrow classes by default) and stretched with SOMAR_NARROW_7PT = 1 and = 0
  A2  A's first two levels, level 1 cut into two 64-wide boxes: a fine-fine seam between a class-4 column and lane 0
  C   refinement by (4, 1, 1) onto one 128-wide box: the mini V-cycle runs on a 128- and a 64-wide depth
  D   A with the sheared non-diagonal metric: the 19-point kernels on their direct / march / fused paths

Every case first checks what it is for (assert_reaches_target): from the library, the box widths of every level and MG depth,
MG ratios equal to the oracle's and to the lists written here, and the uniform-metric flag that decides the tiling; from
helpers.march_columns, a restatement of Level::build_march_tiles' rule (the library exports no tile table), the columns a
box of each such width gets.  The 19-point fused cases also assert that the fused-sweep counter rose on every level; the
library has no such counter for the 7-point fused sweep, so that the "fused" cases execute its class-4 and class-1 bodies
and its in-kernel x-high ghost is not asserted here.  Then the operations of test_gpu_amr.py:
quadratic CF interpolation, refluxed composite residual and whole AMR V-cycles bit for bit (SOMAR_ORDERED_REDUCE_MAX raised
over every level, so each sum runs in the reference's serial order), the mini V-cycle bit for bit, composite solves with
the oracle's iterations, exit status and history (1e-12 for 7-point with ordered sums, 1e-8 for 19-point), and one V-cycle
with the default ordered-sum limit held to 1e-12 of the correction's scale per box (the base level's 6144 cells are then
tree-summed)."""
import numpy as np
import pytest

from helpers import (download_valid, make_amr_levels, make_full_amr_levels, make_gpu_amr, march_columns, max_rel_diff, upload,
                     valid_of)

pytestmark = pytest.mark.gpu

ORDERED_DEFAULT = 4096      # PressureSolver::ordered_max_cells_
ORDERED_ALL = "1000000"     # above every level here: serial-order sums everywhere
HUGE = "1000000000000"

# the columns [(width, lane class)] of a box, by width: narrow lane classes, and equal columns (SOMAR_NARROW_7PT = 0).  16: four
# class-4 columns would cost a whole workgroup-march, more than 0.85 of the one equal column
NARROW_COLS = {128: [(124, 0), (4, 4)], 96: [(96, 0)], 64: [(60, 1), (4, 4)], 48: [(48, 1)], 32: [(32, 1)], 24: [(24, 1)],
               16: [(16, 0)], 8: [(4, 4), (4, 4)]}
EQUAL_COLS = {128: [(64, 0), (64, 0)], 96: [(96, 0)], 64: [(64, 0)], 48: [(48, 0)], 32: [(32, 0)], 24: [(24, 0)],
              16: [(16, 0)], 8: [(8, 0)]}


class Hier:
    """a hierarchy and what it is for.  widths[l]: the box widths of AMR level l; mg[l]: its MG ratios (the oracle's, written
    out); variant: "cartesian" / "stretched" (7-point) or "full" (sheared, 19-point); narrow: SOMAR_NARROW_7PT or None"""

    def __init__(self, name, n, L, ratios, boxes, widths, mg, variant="cartesian", narrow=None):
        self.name, self.n, self.L, self.ratios, self.boxes = name, n, L, ratios, boxes
        self.widths, self.mg, self.variant, self.narrow = widths, mg, variant, narrow
        self.periodic = (False, True, False)

    @property
    def full(self):
        return self.variant == "full"

    @property
    def layout(self):
        return repr((self.n, self.L, self.ratios, self.boxes, self.variant))   # the oracle does not see `narrow`

    def __repr__(self):
        return self.name


A_BOXES = [[((32, 0, 0), (159, 15, 7))], [((160, 0, 0), (223, 31, 7))]]
A_MG = [[(2, 1, 2)], [(2, 1, 1), (2, 2, 2)], [(2, 2, 1), (2, 1, 1), (2, 2, 2)]]
A_ARGS = ((96, 8, 8), (6.0, 1.0, 0.5), [(2, 2, 1), (2, 2, 1)], A_BOXES, [[96], [128], [64]], A_MG)
A_CART = Hier("A-cartesian", *A_ARGS)
A_NARROW = Hier("A-stretched-narrow", *A_ARGS, variant="stretched", narrow="1")
A_EQUAL = Hier("A-stretched-equal", *A_ARGS, variant="stretched", narrow="0")
A2 = Hier("A2-cartesian", (96, 8, 8), (6.0, 1.0, 0.5), [(2, 2, 1)], [[((32, 0, 0), (95, 15, 7)), ((96, 0, 0), (159, 15, 7))]],
          [[96], [64, 64]], A_MG[:2])
C = Hier("C-cartesian", (48, 8, 8), (6.0, 1.0, 1.0), [(4, 1, 1)], [[((32, 0, 0), (159, 7, 7))]], [[48], [128]],
         [[(2, 2, 2)], [(2, 1, 1), (2, 1, 1), (2, 2, 2)]])
D = Hier("D-sheared", *A_ARGS, variant="full")
SEVEN_POINT = [A_CART, A_NARROW, A_EQUAL, A2, C]


@pytest.fixture(scope="module")
def am(oracle):
    from oracle import somar_amr
    return somar_amr


@pytest.fixture(scope="module")
def F():
    from somar_amd import api
    return api


# (SOMAR_FUSED_MIN_CELLS, SOMAR_MARCH_MIN_CELLS, SOMAR_FUSED19_MIN_BOX); None: unset
KERNELS = {"twopass": (HUGE, None, None), "fused": ("0", None, None),                                   # 7-point
           "direct": (None, HUGE, "-1"), "march": (None, "0", "-1"), "fused19": (None, "0", "0")}      # 19-point


def set_env(monkeypatch, h, kernels, ordered=ORDERED_ALL, uniform=True):
    """the knobs read at solver creation.  7-point: test_gpu_amr.py's sweep_kernel -- "fused" puts the fused red+black sweep
    and, with it, the marching operator / residual kernels on every level; 19-point: the three paths of test_gpu_amr_full.py's
    fixture"""
    fused, march, fused19 = KERNELS[kernels]
    for name, value in (("SOMAR_FUSED_MIN_CELLS", fused), ("SOMAR_MARCH_MIN_CELLS", march), ("SOMAR_FUSED19_MIN_BOX", fused19),
                        ("SOMAR_NARROW_7PT", h.narrow), ("SOMAR_ORDERED_REDUCE_MAX", ordered),
                        ("SOMAR_NO_UNIFORM", None if uniform else "1")):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


# (hierarchy, kernels) of every operation: 7-point on both sweep / residual kernel families, 19-point on its three paths
PATHS = [(h, k) for h in SEVEN_POINT for k in ("twopass", "fused")] + [(D, k) for k in ("direct", "march", "fused19")]
IDS = ["%s-%s" % hk for hk in PATHS]


SOLVE_PATHS = [hk for hk in PATHS if hk[0] in (A_CART, D)]


def make_levels(so, am, h):
    fb = [[so.Box(lo, hi) for lo, hi in lev] for lev in h.boxes]
    if h.full:
        return make_full_amr_levels(so, am, h.n, h.L, h.periodic, h.ratios, fb, cbox=h.n)
    return make_amr_levels(so, am, h.n, h.L, h.periodic, h.ratios, fb, variant=h.variant, cbox=h.n)


_COMPOSITES = {}   # layout -> (levels, AMRComposite): the oracle's hierarchy, built once and only looked at


def fresh_composite(so, am, h, levels):
    """every oracle computation gets a solver of its own (a solve leaves its convergence metrics in the bottom solver)"""
    return am.AMRComposite(levels, h.ratios, so.BCHolder(), so.BiCGStab(), isDiagonal=not h.full)


def oracle_hierarchy(so, am, h):
    if h.layout not in _COMPOSITES:
        levels = make_levels(so, am, h)
        _COMPOSITES[h.layout] = (levels, fresh_composite(so, am, h, levels))
    return _COMPOSITES[h.layout]


def gpu_hierarchy(levels, h, **kw):
    return make_gpu_amr(levels, h.ratios, full=h.full, **kw)


def assert_reaches_target(gpu, comp, h, uniform=True):
    """box widths of every level and MG depth, MG ratios and uniform-metric flag as the library reports them, and the tile
    columns the restated rule gives boxes of those widths: a case that no longer reaches the wide-box paths fails here"""
    assert len(gpu.levels) == len(h.widths)
    for l, v in enumerate(gpu.levels):
        oracle_ratios = [tuple(r) for r in comp.mg[l].mgRefRatios]
        assert v.mgRefRatios() == oracle_ratios == h.mg[l], (l, v.mgRefRatios(), oracle_ratios)
        assert v.depth() == len(h.mg[l]) + 1
        want = list(h.widths[l])
        for d in range(v.depth()):
            boxes = [v.patch_box(q, d) for q in range(v.num_local_patches)]
            assert sorted(hi[0] - lo[0] + 1 for lo, hi, _ in boxes) == want, (l, d, boxes)
            is_uniform = v.metricUniform(d) is not None
            assert is_uniform == (h.variant == "cartesian" and uniform), (l, d)
            # finalize's choice (solver.cpp): SOMAR_NARROW_7PT forces it, else narrow classes where the metric is uniform; the
            # 19-point tables always use the classes
            narrow = True if h.full else (h.narrow == "1" if h.narrow is not None else is_uniform)
            for w in set(want):
                assert march_columns(w, narrow) == (NARROW_COLS if narrow else EQUAL_COLS)[w], (l, d, w)
            if d < len(h.mg[l]):
                assert all(w % h.mg[l][d][0] == 0 for w in want)
                want = [w // h.mg[l][d][0] for w in want]


def assert_boxes_equal(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg="%s, box %d" % (what, i))


# ---- 1. quadratic CF interpolation ---------------------------------------------------------------------------------------
_ORACLE_INTERP = {}


@pytest.mark.parametrize("h", [A_CART, A2, C, D], ids=repr)
def test_cf_interpolation_bit_exact(oracle, am, F, monkeypatch, h):
    """every coarse-fine ghost cell of every refined level: the x-low face of a 128-wide box, and its x-high face (the
    interpolation does not depend on the sweep / residual kernel family)"""
    kernels = "march" if h.full else "fused"
    so = oracle
    levels, comp = oracle_hierarchy(so, am, h)
    if h.layout not in _ORACLE_INTERP:
        phi = [so.random_field(L.grids, 5 + l, (1, 1, 1), L.domain.box) for l, L in enumerate(levels)]
        src = [[np.array(f.a[..., 0]) for f in p.fabs] for p in phi]
        own = fresh_composite(so, am, h, levels)
        for l in range(1, len(levels)):
            own.interp_cf_ghosts(l, phi[l], phi[l - 1])
        _ORACLE_INTERP[h.layout] = (phi, src)
    phi, src = _ORACLE_INTERP[h.layout]
    set_env(monkeypatch, h, kernels)
    gpu = gpu_hierarchy(levels, h)
    try:
        assert_reaches_target(gpu, comp, h)
        for l, v in enumerate(gpu.levels):
            for q in range(v.num_local_patches):
                _, _, gi = v.patch_box(q)
                v.upload(F.F_PHI, q, np.asfortranarray(src[l][gi]), phi[l].ghost)    # as it was before the interpolation
        for l in range(1, len(levels)):
            gpu.interpCF(l)
            v = gpu.levels[l]
            got = {v.patch_box(q)[2]: v.download(F.F_PHI, q, phi[l].ghost) for q in range(v.num_local_patches)}
            ncf, sides = 0, set()
            for (i, d, s), (gb, m) in comp.ops[l].cf.ivs.items():
                if m is None:
                    continue
                want = phi[l][i].view(gb)[..., 0]
                have = got[i][gb.slices(phi[l][i].box.lo)]
                np.testing.assert_array_equal(have[m], want[m], err_msg="level %d box %d dir %d side %s" % (l, i, d, s))
                ncf += int(m.sum())
                sides.add((d, s))
            assert ncf > 0 and len([x for x in sides if x[0] == 0]) == 2, (l, sides)    # both x sides are coarse-fine
    finally:
        gpu.undefine()


# ---- 2. refluxed composite residual ------------------------------------------------------------------------------------
_ORACLE_RESID = {}


@pytest.mark.parametrize("h,kernels", PATHS, ids=IDS)
def test_composite_residual_bit_exact(oracle, am, F, monkeypatch, h, kernels):
    so = oracle
    levels, comp = oracle_hierarchy(so, am, h)
    lmax = len(levels) - 1
    if h.layout not in _ORACLE_RESID:
        phi = [so.random_field(L.grids, 5 + l, (1, 1, 1), L.domain.box) for l, L in enumerate(levels)]
        rhs = [so.random_field(L.grids, 50 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
        src = [[np.array(f.a[..., 0]) for f in p.fabs] for p in phi]
        res = [so.LevelData(L.grids, 1) for L in levels]
        own = fresh_composite(so, am, h, levels)
        own.init(phi, rhs, lmax, 0)
        own.compute_amr_residual(res, phi, rhs, lmax, 0, True)     # zeroes the covered cells
        _ORACLE_RESID[h.layout] = (phi, src, rhs, [[np.array(x) for x in valid_of(r)] for r in res])
    phi, src, rhs, want = _ORACLE_RESID[h.layout]
    set_env(monkeypatch, h, kernels)
    gpu = gpu_hierarchy(levels, h)
    try:
        assert_reaches_target(gpu, comp, h)
        for l, v in enumerate(gpu.levels):
            for q in range(v.num_local_patches):
                _, _, gi = v.patch_box(q)
                v.upload(F.F_PHI, q, np.asfortranarray(src[l][gi]), phi[l].ghost)
            upload(v, F.F_RHS, rhs[l])
        for ilev in range(lmax + 1):
            gpu.residualLevel(lmax, 0, ilev)
            if ilev != lmax:
                gpu.zeroCovered(ilev, F.F_RES)
            assert_boxes_equal(download_valid(gpu.levels[ilev], F.F_RES, levels[ilev].grids), want[ilev],
                               "composite residual, level %d" % ilev)
    finally:
        gpu.undefine()


# ---- 3. one AMR V-cycle from zero ------------------------------------------------------------------------------------------
_ORACLE_CYCLES = {}   # (layout, numMG) -> the oracle's AMRVCycle, shared by the kernel paths and the tilings


def oracle_cycle(so, am, h, numMG=1):
    key = (h.layout, numMG)
    if key not in _ORACLE_CYCLES:
        levels, _ = oracle_hierarchy(so, am, h)
        lmax = len(levels) - 1
        comp = fresh_composite(so, am, h, levels)
        comp.numMG = numMG
        phi = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        res = [so.random_field(L.grids, 70 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
        for l in range(lmax):
            comp.zero_covered(l, res[l])
        comp.init(phi, res, lmax, 0)
        comp.set_bottom_solver(lmax, 0)
        corr = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.amr_vcycle(corr, res, lmax, lmax, 0)
        _ORACLE_CYCLES[key] = (res, [[np.array(x) for x in valid_of(c)] for c in corr])
    return _ORACLE_CYCLES[key]


def fused19_sweeps(gpu):
    return [v.fused19Sweeps() for v in gpu.levels]


def assert_fused19_ran(gpu, kernels, before):
    """since `before`, the fused red+black 19-point sweep ran on every level (all boxes here are at least 8 cells in every
    direction and even in x), and only where it was asked for"""
    for l, (n, n0) in enumerate(zip(fused19_sweeps(gpu), before)):
        assert (n > n0) == (kernels == "fused19"), (l, kernels, n0, n)


def gpu_cycle(F, levels, comp, h, res, numMG=None, uniform=True, kernels=None):
    gpu = gpu_hierarchy(levels, h, numMG=numMG)
    try:
        assert_reaches_target(gpu, comp, h, uniform)
        before = fused19_sweeps(gpu)
        lmax = len(levels) - 1
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RES, res[l])
            v.setVal(F.F_CORR, 0.0)
        gpu.vcycleAMR(lmax, 0)
        assert_fused19_ran(gpu, kernels, before)
        cells = [[v.levelInfo(d)["cells"] for d in range(v.depth())] for v in gpu.levels]
        return [download_valid(gpu.levels[l], F.F_CORR, levels[l].grids) for l in range(lmax + 1)], cells
    finally:
        gpu.undefine()


@pytest.mark.parametrize("h,kernels", PATHS, ids=IDS)
def test_amr_vcycle_bit_exact(oracle, am, F, monkeypatch, h, kernels):
    """smoothing (the coarse-fine ghosts of the black pass made inside the fused sweep), refluxed residual, residual +
    restriction in one pass, the base level's cycle, prolongation folded into the first up-sweep: the oracle's bits in every
    box of every level.  The Cartesian hierarchies also against their streaming twin (SOMAR_NO_UNIFORM = 1: the kernels that
    read the metric arrays, on equal columns)."""
    so = oracle
    levels, comp = oracle_hierarchy(so, am, h)
    res, want = oracle_cycle(so, am, h)
    set_env(monkeypatch, h, kernels)
    got, _ = gpu_cycle(F, levels, comp, h, res, kernels=kernels)
    for l in range(len(levels)):
        assert_boxes_equal(got[l], want[l], "AMR V-cycle, level %d" % l)
    if h.variant == "cartesian":
        set_env(monkeypatch, h, kernels, uniform=False)
        twin, _ = gpu_cycle(F, levels, comp, h, res, uniform=False)
        for l in range(len(levels)):
            assert_boxes_equal(twin[l], got[l], "streaming twin, level %d" % l)


@pytest.mark.parametrize("kernels", ["twopass", "fused"])
def test_amr_w_cycle_bit_exact(oracle, am, F, monkeypatch, kernels):
    """numMG = 2 on A: every level is visited twice per visit of the finer one, the second time from a non-zero correction"""
    so = oracle
    h = A_CART
    levels, comp = oracle_hierarchy(so, am, h)
    res, want = oracle_cycle(so, am, h, numMG=2)
    set_env(monkeypatch, h, kernels)
    got, _ = gpu_cycle(F, levels, comp, h, res, numMG=2)
    for l in range(len(levels)):
        assert_boxes_equal(got[l], want[l], "AMR W-cycle, level %d" % l)
    assert any(not np.array_equal(a, b) for a, b in zip(want[0], oracle_cycle(so, am, h)[1][0]))   # not the V-cycle again


@pytest.mark.parametrize("kernels", ["twopass", "fused"])
def test_amr_vcycle_default_reduction(oracle, am, F, monkeypatch, kernels):
    """the default ordered-sum limit: the base level's 6144 cells are above it, so its mean removal and BiCGStab scalars are
    tree sums (and the fused path may fold the prolongation into the up-sweep): round-off, 1e-12 of the correction's scale
    per box (test_gpu_wcycle.py's tree-sum bound)"""
    so = oracle
    h = A_CART
    levels, comp = oracle_hierarchy(so, am, h)
    res, want = oracle_cycle(so, am, h)
    set_env(monkeypatch, h, kernels, ordered=None)
    got, cells = gpu_cycle(F, levels, comp, h, res)
    assert cells[0][0] > ORDERED_DEFAULT, cells
    scale = max(float(np.abs(w).max()) for lev in want for w in lev)
    for l in range(len(levels)):
        for i, (g, w) in enumerate(zip(got[l], want[l])):
            print("%s %s level %d box %d: max|c - c_oracle| / scale = %.3e" % (h, kernels, l, i, np.abs(g - w).max() / scale))
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * scale, err_msg="level %d box %d" % (l, i))


# ---- 4. the mini V-cycle of a level refined by 4 ---------------------------------------------------------------------------
_ORACLE_MINI = {}


@pytest.mark.parametrize("kernels", ["twopass", "fused"])
def test_mini_vcycle_bit_exact(oracle, am, F, monkeypatch, kernels):
    """MappedAMRMultiGrid::relax on C's fine level: a V-cycle over the forced (2, 1, 1) depth, 128 and 64 cells wide, whose
    bottom is smoothed and then zeroed by the NoOpSolver (test_gpu_amr.py::test_mini_vcycle_bit_exact)"""
    so = oracle
    h = C
    levels, comp = oracle_hierarchy(so, am, h)
    L = levels[1]
    assert comp.mg[1].maxForcedDepth == 1 and comp.mg[1].mgRefRatios[0] == (2, 1, 1)
    if h.layout not in _ORACLE_MINI:
        res = so.random_field(L.grids, 70, (0, 0, 0), L.domain.box)
        corr = so.random_field(L.grids, 71, (1, 1, 1), L.domain.box)
        start = [np.array(f.a[..., 0]) for f in corr.fabs]
        zero = [so.LevelData(X.grids, 1, (1, 1, 1)) for X in levels]
        zres = [so.LevelData(X.grids, 1, (0, 0, 0)) for X in levels]
        own = fresh_composite(so, am, h, levels)
        own.init(zero, zres, 1, 0)
        own.set_bottom_solver(1, 0)
        own.relax(1, corr, res, 2)
        _ORACLE_MINI[h.layout] = (res, corr.ghost, start, [np.array(x) for x in valid_of(corr)])
    res, ghost, start, want = _ORACLE_MINI[h.layout]
    set_env(monkeypatch, h, kernels)
    gpu = gpu_hierarchy(levels, h)
    try:
        assert_reaches_target(gpu, comp, h)
        v = gpu.levels[1]
        upload(v, F.F_RES, res)
        for q in range(v.num_local_patches):
            _, _, gi = v.patch_box(q)
            v.upload(F.F_CORR, q, np.asfortranarray(start[gi]), ghost)
        v.miniVCycle(F.F_CORR, F.F_RES)
        assert_boxes_equal(download_valid(v, F.F_CORR, L.grids), want, "mini V-cycle")
    finally:
        gpu.undefine()


# ---- 5. composite solves ---------------------------------------------------------------------------------------------------
_ORACLE_SOLVES = {}


@pytest.mark.parametrize("h,kernels", SOLVE_PATHS, ids=["%s-%s" % hk for hk in SOLVE_PATHS])
def test_composite_solve_history_matches(oracle, am, F, monkeypatch, h, kernels):
    """a compatible right-hand side (rhs = L_composite[random phi]): the oracle's V-cycles, exit status and residual history
    (test_gpu_amr.py's rtol 1e-12 for 7-point with ordered sums, test_gpu_amr_full.py's 1e-8 for 19-point)"""
    so = oracle
    levels, comp = oracle_hierarchy(so, am, h)
    lmax = len(levels) - 1
    if h.layout not in _ORACLE_SOLVES:
        phi = [so.random_field(L.grids, 5 + l, (1, 1, 1), L.domain.box) for l, L in enumerate(levels)]
        zero = [so.LevelData(L.grids, 1) for L in levels]
        rhs = [so.LevelData(L.grids, 1) for L in levels]
        own = fresh_composite(so, am, h, levels)
        own.init(phi, zero, lmax, 0)
        own.compute_amr_residual(rhs, phi, zero, lmax, 0, True)
        for r in rhs:
            so.ld_scale(r, -1.0)
        sol = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        own.solve(sol, rhs, lmax, 0)
        _ORACLE_SOLVES[h.layout] = {"rhs": rhs, "sol": [[np.array(x) for x in valid_of(s_)] for s_ in sol],
                                    "iters": own.iters, "exitStatus": own.exitStatus, "history": list(own.history)}
    o = _ORACLE_SOLVES[h.layout]
    set_env(monkeypatch, h, kernels)
    gpu = gpu_hierarchy(levels, h)
    try:
        assert_reaches_target(gpu, comp, h)
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RHS, o["rhs"][l])
        before = fused19_sweeps(gpu)
        st = gpu.solveAMR(lmax, 0)
        assert_fused19_ran(gpu, kernels, before)
        assert st["iters"] == o["iters"] and st["exitStatus"] == o["exitStatus"], (st, o["iters"], o["exitStatus"])
        assert o["iters"] >= 2
        np.testing.assert_allclose(st["history"], o["history"], rtol=1e-8 if h.full else 1e-12, atol=0.0)
        if not h.full:
            for l in range(lmax + 1):
                assert max_rel_diff(download_valid(gpu.levels[l], F.F_PHI, levels[l].grids), o["sol"][l]) < 1e-8
    finally:
        gpu.undefine()
