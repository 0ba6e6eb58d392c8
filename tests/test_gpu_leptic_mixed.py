"""The leptic level solver on a level that MIXES Neumann-Neumann (spanning) columns with columns ended by a coarse-fine
interface: a fine level refined by (2, 2, 2) whose boxes partly span the water column and partly stop half way up (or
start half way down) under the coarse level -- the reference's m_flatDI / m_flatDIComplement (LevelLepticSolver.cpp:318-333,
:1203, :1019-1021, :1504), against the oracle's restatement (oracle/somar_leptic.py).

The level solve alone stalls on such a level (the horizontal correction reaches the spanning boxes only) and the
full-multigrid fallback blows up there, in the oracle as well: every case below uses a max_order at which the oracle ends
with usedFullSolver == False, and asserts it."""
import functools

import numpy as np
import pytest

from oracle import somar_amr as sa
from oracle import somar_leptic as sl
from oracle import somar_oracle as so
from tests.helpers import download_valid, make_amr_levels, make_gpu_amr, upload, valid_of

pytestmark = pytest.mark.gpu

H = 0.005
N, RATIOS = (16, 16, 8), [(2, 2, 2)]
NN, N_CF, CF_N = (sl.VBC_NEUM, sl.VBC_NEUM), (sl.VBC_NEUM, sl.VBC_CF), (sl.VBC_CF, sl.VBC_NEUM)
LAYOUTS = {
    # one spanning box, one (Neumann, CF) box
    "A": [so.Box((8, 8, 0), (15, 23, 15)), so.Box((16, 8, 0), (23, 23, 7))],
    # the complement is (CF, Neumann)
    "B": [so.Box((8, 8, 0), (15, 23, 15)), so.Box((16, 8, 8), (23, 23, 15))],
    # the spanning boxes are patches 0 and 3 (flat patches 0 and 1): an identity patch map fails here; both complement kinds
    "C": [so.Box((8, 8, 0), (15, 15, 15)), so.Box((16, 8, 0), (23, 15, 7)), so.Box((8, 16, 8), (15, 23, 15)),
          so.Box((16, 16, 0), (23, 23, 15))],
    # A with the complement first
    "A_swapped": [so.Box((16, 8, 0), (23, 23, 7)), so.Box((8, 8, 0), (15, 23, 15))],
}
KINDS = {"A": [NN, N_CF], "B": [NN, CF_N], "C": [NN, N_CF, CF_N, NN], "A_swapped": [N_CF, NN]}


@functools.lru_cache(maxsize=None)
def _levels(layout):
    return make_amr_levels(so, sa, N, (1.0, 1.0, H), (False, False, False), RATIOS, [LAYOUTS[layout]], cbox=(8, 8, 8))


def _oracle(levels, maxOrder, fixed=False, iters=2):
    amr = sl.AMRLepticSolver(levels, RATIOS, so.BCHolder(), leptic=dict(maxOrder=maxOrder, domainHeight=H),
                             baseFromRestricted=fixed)
    amr.iterMax = iters
    return amr


def _gpu(levels, maxOrder, fixed=False, full=False, iters=2):
    from somar_amd import api as F
    gpu = make_gpu_amr(levels, RATIOS, full=full, imax=iters)
    try:
        lp = F.LepticParams()
        F._ck(F.lib().somar_leptic_params_default(lp))
        lp.max_order, lp.domain_height = maxOrder, H
        gpu.enableLeptic(lp, baseFromRestricted=fixed)
    except Exception:
        gpu.undefine()
        raise
    return gpu


def _compatible_rhs(amr, levels, lmax):
    phi = [so.random_field(Lv.grids, 5 + l, (1, 1, 1), Lv.domain.box) for l, Lv in enumerate(levels)]
    zero = [so.LevelData(Lv.grids, 1) for Lv in levels]
    rhs = [so.LevelData(Lv.grids, 1) for Lv in levels]
    amr.init(phi, zero, lmax, 0)
    amr.compute_amr_residual(rhs, phi, zero, lmax, 0, True)
    for r in rhs:
        so.ld_scale(r, -1.0)
    return rhs


def _rhs1(levels):
    return so.random_field(levels[1].grids, 9, domainBox=levels[1].domain.box)


@functools.lru_cache(maxsize=None)
def _oracle_fine_alone(layout, maxOrder, iters):
    """the oracle's l_base = l_max = 1 solve, computed once per case and shared (read only)"""
    levels = _levels(layout)
    amr = _oracle(levels, maxOrder, iters=iters)
    phi = [so.LevelData(Lv.grids, 1, (1, 1, 1)) for Lv in levels]
    amr.solve(phi, [None, _rhs1(levels)], 1, 1)
    lep = amr.leptic[1]
    assert lep.vertBCTypes == KINDS[layout] and lep.doHorizSolve
    assert lep.flatDI == [i for i, t in enumerate(KINDS[layout]) if t == NN]
    return amr, phi


def _gpu_fine_alone(gpu, levels):
    from somar_amd import api as F
    upload(gpu.levels[1], F.F_RHS, _rhs1(levels))
    gpu.levels[0].setVal(F.F_PHI, 0.0)
    st = gpu.solveAMRLeptic(1, 1)
    return st, gpu.lepticStats(1), download_valid(gpu.levels[1], F.F_PHI, levels[1].grids)


# the orders at which the oracle does not reach its fallback (A 3, B 2 and C 3 do, and the oracle raises there)
@pytest.mark.parametrize("layout,maxOrder", [("A", 1), ("A", 2), ("B", 1), ("B", 3), ("C", 1), ("C", 2), ("A_swapped", 1),
                                             ("A_swapped", 2)])
def test_fine_level_alone_mixed_columns(layout, maxOrder):
    """l_base = l_max = 1 with a zero coarse phi, iterMax = 2: two LevelLepticSolver::solve calls on the mixed level.  The
    level's statistics are those of its LAST solve, so the same hierarchy is also run with iterMax = 1: the first solve is
    the one whose residual jumps at order 0 (1.737 -> 7.06 in the oracle), when the horizontal correction has lifted the
    spanning boxes only and left a step across the fine-fine face -- a path that skips the horizontal part shows no jump."""
    levels = _levels(layout)
    for iters in (1, 2):
        amr, phi = _oracle_fine_alone(layout, maxOrder, iters)
        lep = amr.leptic[1]
        assert lep.usedFullSolver is False
        gpu = _gpu(levels, maxOrder, iters=iters)
        try:
            st, ls, got = _gpu_fine_alone(gpu, levels)
            print("iterMax", iters, "history", st["history"], amr.history, "resNorms", ls["resNorms"], lep.resNorms)
            assert st["iters"] == amr.iters == iters and st["exitStatus"] == amr.exitStatus
            assert ls["exitStatus"] == lep.exitStatus and ls["horizSolves"] == lep.horizSolves == 1
            assert ls["usedFullSolver"] == 0
            np.testing.assert_allclose(st["history"], amr.history, rtol=0, atol=1e-10 * amr.history[0])
            np.testing.assert_allclose(ls["resNorms"], lep.resNorms, rtol=0, atol=1e-10 * lep.resNorms[0])
            if iters == 1:
                assert ls["resNorms"][1] > ls["resNorms"][0]
            want = valid_of(phi[1])
            scale = max(float(np.max(np.abs(w))) for w in want)
            for g_, w_ in zip(got, want):
                np.testing.assert_allclose(g_, w_, rtol=0, atol=1e-9 * scale)
        finally:
            gpu.undefine()


def test_two_level_composite_solve_mixed_columns():
    """l_base = 0, l_max = 1, the base level fed the restricted residual: the mixed level solve as the smoother of the
    composite cycle, where it works (the oracle contracts 7.7e7 -> 6.9e4 -> 1.4e4).  Layout A only: the oracle's leg takes
    eight seconds per layout, and layout C's patch map is covered by the one-level cases above."""
    from somar_amd import api as F
    levels = _levels("A")
    amr = _oracle(levels, 2, fixed=True)
    rhs = _compatible_rhs(amr, levels, 1)
    sol = [so.LevelData(Lv.grids, 1, (1, 1, 1)) for Lv in levels]
    amr.solve(sol, rhs, 1, 0)
    assert all(lep.usedFullSolver is False for lep in amr.leptic)
    gpu = _gpu(levels, 2, fixed=True)
    try:
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_RHS, rhs[l])
        st = gpu.solveAMRLeptic(1, 0)
        h = np.array(amr.history)
        print("history", st["history"], h)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        np.testing.assert_allclose(st["history"], h, rtol=0, atol=1e-9 * h[0])
        for l in (0, 1):
            ls, lep = gpu.lepticStats(l), amr.leptic[l]
            assert ls["exitStatus"] == lep.exitStatus and ls["horizSolves"] == lep.horizSolves
            assert ls["usedFullSolver"] == 0
            np.testing.assert_allclose(ls["resNorms"], lep.resNorms, rtol=0, atol=1e-9 * lep.resNorms[0])
            want = valid_of(sol[l])
            scale = max(float(np.max(np.abs(w))) for w in want)
            for g_, w_ in zip(download_valid(gpu.levels[l], F.F_PHI, levels[l].grids), want):
                np.testing.assert_allclose(g_, w_, rtol=0, atol=1e-7 * scale)
        assert gpu.lepticStats(1)["horizSolves"] == 1
    finally:
        gpu.undefine()


def test_pieces_of_one_level_solve_layout_c():
    """one level solve on layout C against the oracle's lep.last: the flat solver holds the two spanning boxes (patches 0 and
    3 of the level are its patches 0 and 1), its right-hand side and solution are those of the first order (a diagonal
    metric solves the flat problem at order 0 only), and the J-scaled operator's phi is the last order's vertPhi"""
    from somar_amd import api as F
    levels = _levels("C")
    amr, _ = _oracle_fine_alone("C", 2, 1)
    lep = amr.leptic[1]
    last = lep.last
    gpu = _gpu(levels, 2, iters=1)
    try:
        _gpu_fine_alone(gpu, levels)
        flat = gpu.lepticPart(1, 2)
        assert flat.num_local_patches == len(lep.horizGrids) == 2
        for p_ in range(2):
            lo, hi, gi = flat.patch_box(p_)
            assert (tuple(lo), tuple(hi)) == (tuple(lep.horizGrids[gi].lo), tuple(lep.horizGrids[gi].hi))
        for field, name in ((F.F_RHS, "horizRhs"), (F.F_PHI, "horizPhi")):
            want = valid_of(last[name])
            scale = max(float(np.max(np.abs(w))) for w in want)
            assert scale > 0.0
            for g_, w_ in zip(download_valid(flat, field, lep.horizGrids), want):
                np.testing.assert_allclose(np.reshape(g_, w_.shape, order="F"), w_, rtol=0, atol=1e-10 * scale, err_msg=name)
        # vertPhi carries the extruded horizPhi: the tolerance of phi in the one-level cases
        want = valid_of(last["vertPhi"])
        scale = max(float(np.max(np.abs(w))) for w in want)
        for g_, w_ in zip(download_valid(gpu.lepticPart(1, 1), F.F_PHI, levels[1].grids), want):
            np.testing.assert_allclose(g_, w_, rtol=0, atol=1e-9 * scale)
    finally:
        gpu.undefine()


def test_failed_fallback_on_a_mixed_level_is_an_error():
    """layout A at max_order 3 hangs at its last order and hands over to the full multigrid, which fails on a mixed level
    (the oracle raises there: MappedAMRMultiGrid's kaboom / "solver blew up", the two non-zero statuses): an error, not a
    correction"""
    from somar_amd import SomarError
    levels = _levels("A")
    gpu = _gpu(levels, 3, iters=1)
    try:
        with pytest.raises(SomarError, match="full-multigrid fallback failed"):
            _gpu_fine_alone(gpu, levels)
    finally:
        gpu.undefine()


def _set_metric(gpu, levels):
    for Lv, v in zip(levels, gpu.levels):
        for p_ in range(v.num_local_patches):
            _, _, gi = v.patch_box(p_)
            jg = [np.asfortranarray(Lv.Jgup[gi][d].a[..., d]) for d in range(3)]
            v.setMetricOrtho(p_, jg[0], jg[1], jg[2], np.asfortranarray(Lv.Jinv[gi].a[..., 0]))


def test_metric_refresh_to_another_metric_on_a_mixed_level():
    """a hierarchy refreshed to another metric equals one built with it: the flat problem's vertical averages are rewritten
    through the patch map (layout C: an identity map would average the wrong boxes)"""
    levels = _levels("C")
    # the same hierarchy (domains, boxes, spacings) with the stretched map of another period
    other = [sa.AMRLevel(Lv.domain, Lv.grids, Lv.dx, *so.make_diagonal_metric(Lv.grids, Lv.dx, (0.9, 1.1, H), 3, "stretched",
                                                                              domain=Lv.domain)) for Lv in levels]
    a, b = _gpu(levels, 2), None
    try:
        b = _gpu(other, 2)
        first = _gpu_fine_alone(a, levels)
        with a.metricUpdate():
            _set_metric(a, other)
        sta, lsa, phia = _gpu_fine_alone(a, levels)
        stb, lsb, phib = _gpu_fine_alone(b, levels)
        assert first[1]["resNorms"] != lsb["resNorms"]   # the two metrics do differ
        assert sta["iters"] == stb["iters"] and sta["exitStatus"] == stb["exitStatus"]
        np.testing.assert_array_equal(sta["history"], stb["history"])
        assert lsa == lsb and lsa["horizSolves"] == 1
        for x, y in zip(phia, phib):
            np.testing.assert_array_equal(x, y)
    finally:
        a.undefine()
        if b is not None:
            b.undefine()


def test_metric_refresh_on_a_mixed_level():
    """a metric update that rewrites the same metric: the J-scaled operator's copy and the flat problem's vertical averages
    (through the patch map) come out as before, and so does the next solve, bit for bit"""
    levels = _levels("A")
    gpu = _gpu(levels, 2)
    try:
        st0, ls0, phi0 = _gpu_fine_alone(gpu, levels)
        with gpu.metricUpdate():
            _set_metric(gpu, levels)
        st1, ls1, phi1 = _gpu_fine_alone(gpu, levels)
        assert st1["iters"] == st0["iters"] and st1["exitStatus"] == st0["exitStatus"]
        np.testing.assert_array_equal(st1["history"], st0["history"])
        for k in ("exitStatus", "orders", "horizSolves", "usedFullSolver"):
            assert ls1[k] == ls0[k]
        np.testing.assert_array_equal(ls1["resNorms"], ls0["resNorms"])
        assert ls1["horizSolves"] == 1
        for a, b in zip(phi1, phi0):
            np.testing.assert_array_equal(a, b)
    finally:
        gpu.undefine()


def test_mixed_columns_with_a_non_diagonal_metric_are_refused():
    """the oracle restates mixed layouts for diagonal metrics only (levelVertHorizGradient would hand the complement's
    Neumann ends non-zero boundary data)"""
    from somar_amd import SomarError
    L = (32.0, 32.0, 1.0)
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in N)), (False, False, False))
    dx = tuple(L[d] / N[d] for d in range(3))
    levels = []
    for l, g in enumerate([so.split_domain(dom.box, (8, 8, 8)), list(LAYOUTS["A"])]):
        if l > 0:
            dom = dom.refine(RATIOS[l - 1])
            dx = tuple(a / b for a, b in zip(dx, RATIOS[l - 1]))
        Jgup, Jinv = so.make_terrain_metric(g, dx, L, dom)
        levels.append(sa.AMRLevel(dom, g, dx, Jgup, Jinv))
    with pytest.raises(SomarError, match="non-diagonal metric"):
        _gpu(levels, 2, full=True).undefine()
