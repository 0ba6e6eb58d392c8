"""Every device allocation of the library is released with the object that made it (csrc/devbuf.h).  The library keeps an
exact count of the bytes it holds (somar_device_bytes_live): each case reads it, builds and runs something, checks the
count is larger while the object lives, destroys the object and requires the first reading back, to the byte.  What a case
computes is checked elsewhere; here only the count matters."""
import numpy as np
import pytest

from helpers import make_amr_levels, make_gpu_amr, make_gpu_solver, make_problem, smooth_cc_velocity, upload

pytestmark = pytest.mark.gpu

WALLS = (False, False, False)


@pytest.fixture
def live():
    """-> check(obj): the count is above the case's first reading now, and back at it once obj is undefined"""
    from somar_amd import api as F
    before = F.device_bytes_live()

    def check(*objs):
        assert F.device_bytes_live() > before
        for o in objs:
            o.undefine()
        assert F.device_bytes_live() == before

    yield check
    assert F.device_bytes_live() == before   # also where a case undefined everything itself


def _solve(so, s, dom, grids, Jinv, seed=3):
    from somar_amd import api as F
    rhs = so.random_field(grids, seed, domainBox=dom.box)
    so.remove_weighted_mean(rhs, Jinv)
    upload(s, F.F_RHS, rhs)
    return s.solveResident()


def _full_solver(so, n, bs, per, L):
    from somar_amd import AMRPressureSolver
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), per)
    grids = so.split_domain(dom.box, bs)
    dx = tuple(L[d] / n[d] for d in range(3))
    Jgup, Jinv = so.make_full_metric(grids, dx, L, dom)
    s = AMRPressureSolver()
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricFull(q, *[np.asfortranarray(Jgup[gi][d].a) for d in range(3)], np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return s, dom, grids, Jinv


def _set_ortho_metric(s, Jgup, Jinv, scale=1.0):
    for p in range(s.num_local_patches):
        _, _, gi = s.patch_box(p)
        jg = [np.asfortranarray(scale * Jgup[gi][d].a[..., d]) for d in range(3)]
        s.setMetricOrtho(p, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))


@pytest.mark.parametrize("boxsz", [8, 16])
def test_level_solve(oracle, live, boxsz):
    """a) 7-point solve with the defaults; b) one 16^3 box: the workgroup-local box bottom solve and its tables"""
    so = oracle
    dom, grids, dx, Jgup, Jinv = make_problem(so, (16, 16, 16), boxsz)
    s = make_gpu_solver(dom, grids, dx, Jgup, Jinv)
    st = _solve(so, s, dom, grids, Jinv)
    assert st["iters"] > 0
    if boxsz == 16:
        assert s.bottomKind() == 2
    live(s)


@pytest.mark.parametrize("case", [((16, 16, 16), 8, (True, True, True), (1.0, 1.0, 1.0)),
                                  ((32, 16, 8), (16, 8, 8), WALLS, (2.0, 1.0, 0.5))])
def test_non_diagonal_metric_solve(oracle, live, case, monkeypatch):
    """c) the ghost programs, the cross planes of every depth and the compiled box programs of the 19-point bottom solve
    (sizes of test_gpu_box_bottom.py's FULL_CASES)"""
    monkeypatch.setenv("SOMAR_BOX_BOTTOM", "1")
    s, dom, grids, Jinv = _full_solver(oracle, *case)
    _solve(oracle, s, dom, grids, Jinv)
    assert s.bottomKind() == 2
    live(s)


def test_dirichlet_face_values_set_cleared_set(oracle, live):
    """d) op lists and the face-value buffer"""
    so = oracle
    dom, grids, dx, Jgup, Jinv = make_problem(so, (16, 16, 16), 8)
    s = make_gpu_solver(dom, grids, dx, Jgup, Jinv, bc_type=[1, 1, 0, 0, 1, 0], bc_values=[0.3, -0.2, 0.0, 0.0, 0.1, 0.0])
    plane = np.linspace(-1.0, 1.0, 256).reshape(16, 16)
    for values in (plane, None, 2.0 * plane):
        s.setBCFaceValues(0, 1, values)
        _solve(so, s, dom, grids, Jinv)
    live(s)


def test_precision_on_off_on(oracle, live, monkeypatch):
    """e) the fp32 fields and metric copies"""
    so = oracle
    monkeypatch.setenv("SOMAR_FUSED_MIN_CELLS", "0")
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", "0")
    dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 32, 32), 16)
    s = make_gpu_solver(dom, grids, dx, Jgup, Jinv)
    s.setPrecision(1, 1)
    assert s.precision()[1] > 0
    _solve(so, s, dom, grids, Jinv)
    s.setPrecision(0)
    s.setPrecision(1, 1)
    _solve(so, s, dom, grids, Jinv)
    live(s)


def test_metric_update_twice(oracle, live):
    """f) the refresh's work items and min / max tables"""
    so = oracle
    dom, grids, dx, Jgup, Jinv = make_problem(so, (16, 16, 16), 8)
    s = make_gpu_solver(dom, grids, dx, Jgup, Jinv)
    for scale in (1.5, 0.5):
        with s.metricUpdate():
            _set_ortho_metric(s, Jgup, Jinv, scale)
        _solve(so, s, dom, grids, Jinv)
    live(s)


def test_lazily_allocated_fields(oracle, live):
    """g) MAC and cell-centred projection, multByJ / divByJ and one heat step of each scheme on one solver"""
    from somar_amd import api as F
    so = oracle
    dom, grids, dx, Jgup, Jinv = make_problem(so, (16, 16, 16), 8)
    s = make_gpu_solver(dom, grids, dx, Jgup, Jinv, alpha=1.0, beta=1e-2)
    rng = np.random.default_rng(9)
    ghost = (1, 1, 1)
    cc = smooth_cc_velocity(so, dom, grids, ghost)
    gi_of = [s.patch_box(p)[2] for p in range(s.num_local_patches)]
    mac = [[np.asfortranarray(rng.uniform(-1, 1, tuple(n + (a == d) for a, n in enumerate(grids[gi].size()))))
            for gi in gi_of] for d in range(3)]
    for p, gi in enumerate(gi_of):
        J = np.asfortranarray(rng.uniform(0.5, 2.0, cc[gi].a.shape[:3]))
        s.uploadCCVel(p, cc[gi].a, ghost)
        s.setCCJ(p, J, np.asfortranarray(1.0 / J), ghost)
        for d in range(3):
            Jf = np.asfortranarray(rng.uniform(0.5, 2.0, mac[d][p].shape))
            s.uploadVel(d, p, mac[d][p])
            s.setFaceJ(d, p, Jf, np.asfortranarray(1.0 / Jf))
    for centring in (0, 1):
        s.multByJ(centring)
        s.divByJ(centring)
    s.setAlphaAndBeta(0.0, 1.0)
    s.levelProject(mac, 0.5)
    s.levelProjectCC([cc[gi].a.copy(order="F") for gi in gi_of], ghost, 0.5)
    upload(s, F.F_HEAT_OLD, so.random_field(grids, 3, (1, 1, 1), dom.box))
    upload(s, F.F_HEAT_SRC, so.random_field(grids, 4, (0, 0, 0), dom.box))
    for scheme in (0, 1, 2):
        s.heatStep(scheme, 0.2)
    live(s)


@pytest.mark.parametrize("leptic", [False, True])
def test_two_level_hierarchy(oracle, live, leptic):
    """h) links, flux registers and CF tables of a two-level hierarchy: one AMR V-cycle, resp. one leptic composite solve"""
    from oracle import somar_amr as am
    from somar_amd import api as F
    so = oracle
    ratios = [(2, 2, 1)]
    fine = [[so.Box((16, 16, 0), (31, 47, 7)), so.Box((32, 16, 0), (47, 47, 7))]]
    levels = make_amr_levels(so, am, (32, 32, 8), (1.0, 1.0, 0.005), WALLS, ratios, fine, cbox=(16, 16, 8))
    gpu = make_gpu_amr(levels, ratios, imax=2)
    for l, v in enumerate(gpu.levels):
        upload(v, F.F_RES, so.random_field(levels[l].grids, 70 + l, (0, 0, 0), levels[l].domain.box))
        upload(v, F.F_RHS, so.random_field(levels[l].grids, 80 + l, (0, 0, 0), levels[l].domain.box))
        v.setVal(F.F_CORR, 0.0)
    if leptic:
        lp = F.LepticParams()
        F._ck(F.lib().somar_leptic_params_default(lp))
        lp.max_order, lp.domain_height = 2, 0.005
        gpu.enableLeptic(lp)
        gpu.solveAMRLeptic(1, 0)
    else:
        gpu.vcycleAMR(1, 0)
    live(gpu)


def test_stand_alone_leptic_solver(oracle, live):
    """i) LepticSolver's fields, tables and its three level solvers"""
    from somar_amd import LevelLepticSolver
    from somar_amd import api as F
    so = oracle
    H = 0.005
    dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 32, 8), (16, 16, 8), L=(1.0, 1.0, H))
    s = LevelLepticSolver()
    s.params.max_order, s.params.domain_height = 2, H
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
    _set_ortho_metric(s.level, Jgup, Jinv)
    s.finalize()
    rhs = so.random_field(grids, 3, domainBox=dom.box)
    so.remove_weighted_mean(rhs, Jinv)
    upload(s.level, F.F_RHS, rhs)
    s.solve()
    live(s)


def test_defined_but_never_finalized(oracle, live):
    """j) the level's tables and metric planes alone"""
    from somar_amd import AMRPressureSolver
    so = oracle
    dom, grids, dx, Jgup, Jinv = make_problem(so, (16, 16, 16), 8)
    s = AMRPressureSolver()
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
    _set_ortho_metric(s, Jgup, Jinv)
    live(s)


def test_kernel_hooks_release_their_temporaries(live):
    """k) one call of every hook that allocates on the device; each returns with the count where it was"""
    from somar_amd import api as F
    before = F.device_bytes_live()
    rng = np.random.default_rng(5)
    lo, n = (3, -2, 5), (20, 13, 9)
    hi = tuple(a + b - 1 for a, b in zip(lo, n))
    faces = [tuple(a + (d == q) for q, a in enumerate(n)) for d in range(3)]
    jinv = np.asfortranarray(rng.uniform(0.5, 1.5, n))
    dx = (0.1, 0.07, 0.2)
    region = ((lo[0] + 2, lo[1], lo[2] + 1), (hi[0], hi[1] - 3, hi[2]))
    calls = []
    phi = np.asfortranarray(rng.uniform(-1, 1, tuple(a + 2 for a in n)))
    jg = [np.asfortranarray(rng.uniform(0.5, 1.5, f)) for f in faces]
    calls.append(lambda: F.k_gsrbiter3dortho(phi, tuple(a - 1 for a in lo), np.asfortranarray(rng.uniform(-1, 1, n)), lo, jg,
                                             [lo, lo, lo], jinv, lo, np.asfortranarray(rng.uniform(1, 2, n)), lo, region, dx,
                                             0.3, 1.7, 0))
    jg3 = [np.asfortranarray(rng.uniform(0.5, 1.5, f + (3,))) for f in faces]
    calls.append(lambda: F.k_fillmappedlapdiag3d(np.zeros(n, order="F"), lo, jg3, [lo, lo, lo], jinv, lo, region, dx))
    r, cbox = (2, 1, 2), ((2, -1, 3), (9, 6, 6))
    flo = tuple(a * q for a, q in zip(cbox[0], r))
    fn = tuple((h - a + 1) * q for a, h, q in zip(cbox[0], cbox[1], r))
    cn = tuple(h - a + 1 for a, h in zip(cbox[0], cbox[1]))
    fine, fjinv = np.asfortranarray(rng.uniform(-1, 1, fn + (2,))), np.asfortranarray(rng.uniform(0.5, 1.5, fn))
    calls.append(lambda: F.k_mappedaverage2(np.zeros(cn + (2,), order="F"), cbox[0], fine, flo, fjinv, flo, cbox, r))
    one = np.ones(1000)
    calls.append(lambda: F.altered_jgup(one, one, one, one, one, 0.37, 0.13))
    dxdxi = rng.uniform(0.5, 1.5, (1000, 3, 3)) + 2.0 * np.eye(3)
    calls.append(lambda: F.jgup_from_dxdxi(dxdxi, np.linalg.det(dxdxi), 1))
    calls.append(lambda: F.stream_probe(2, cells=1 << 16, reps=1))
    for call in calls:
        call()
        assert F.device_bytes_live() == before
