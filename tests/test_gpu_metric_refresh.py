"""Metric refresh of a finalized solver (somar_solver_metric_update_begin / _end, somar_amr_metric_update_begin / _end).

Every case compares solver A -- created with metric M1, finalized, run once (so that graphs exist), then refreshed to M2 --
with solver B, created with M2 from the start.  Everything finalize derives from the metric must come out the same bits:
every metric array of every MG depth (somar_solver_metric_download), the uniform / zero-plane / null-space flags, and the
solves that follow (phi, residual history, iteration count, exit status)."""
import multiprocessing as mp
import os
import traceback
import uuid

import numpy as np
import pytest

from oracle import somar_amr as sa
from oracle import somar_oracle as so
from tests.helpers import download_valid, make_amr_levels, make_gpu_amr, upload

pytestmark = pytest.mark.gpu

N, BOX = (32, 32, 16), (16, 16, 16)
L1, L2 = (1.0, 1.0, 0.5), (0.7, 1.3, 0.45)


def _solver(dom, grids, dx, ndim=3, alpha=0.0, beta=1.0, bc_type=None):
    from somar_amd import AMRPressureSolver
    s = AMRPressureSolver()
    s.setSpaceDim(ndim)
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=alpha, beta=beta,
             bc_type=bc_type)
    return s


def _ortho(s, Jgup, Jinv, ndim=3):
    for p in range(s.num_local_patches):
        _, _, gi = s.patch_box(p)
        jg = [np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(ndim)] + [None] * (3 - ndim)
        s.setMetricOrtho(p, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))


def _full(s, Jgup, Jinv, ndim=3):
    for p in range(s.num_local_patches):
        _, _, gi = s.patch_box(p)
        jg = [np.asfortranarray(Jgup[gi][d].a) for d in range(ndim)] + [None] * (3 - ndim)
        s.setMetricFull(p, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))


def _which(full, ndim):
    w = list(range(ndim)) + [3, 4]
    if full:
        w += [16 + 3 * a + b for a in range(ndim) for b in range(ndim) if a != b]
    return w


def _state(s, full=False, ndim=3):
    """every metric array of every depth and patch, and the per-depth flags"""
    out = {"depth": s.depth(), "ratios": s.mgRefRatios()}
    for d in range(s.depth()):
        out[("zeroAvg", d)] = s.zeroAvg(d)
        out[("uniform", d)] = s.metricUniform(d)
        for p in range(_npatches(s, d)):
            for w in _which(full, ndim):
                out[(d, p, w)] = s.metricDownload(d, w, p)
    return out


def _npatches(s, d):
    # patch_box refuses past the last local patch
    from somar_amd.api import SomarError
    n = 0
    while True:
        try:
            s.patch_box(n, d)
        except SomarError:
            return n
        n += 1


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=str(k))
        else:
            assert a[k] == b[k], k


def _solve(s, grids, dom, seed=5):
    from somar_amd.api import F_PHI, F_RHS
    rhs = so.random_field(grids, seed, domainBox=dom.box)
    upload(s, F_RHS, rhs)
    st = s.solveResident(True, False)
    return st, download_valid(s, F_PHI, grids)


def _assert_same_solve(a, b):
    (sa_, pa), (sb, pb) = a, b
    for k in ("iters", "exitStatus", "status", "history", "final_rnorm"):
        assert sa_[k] == sb[k], k
    for x, y in zip(pa, pb):
        np.testing.assert_array_equal(x, y)


def _problem(n=N, box=BOX, periodic=(False, True, False)):
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), periodic)
    grids = so.split_domain(dom.box, box)
    dx = tuple(L1[d] / n[d] for d in range(3))
    return dom, grids, dx


@pytest.mark.parametrize("graphs", [True, False])
def test_diagonal_3d_refresh_equals_fresh_solver(graphs, monkeypatch):
    if not graphs:
        monkeypatch.setenv("SOMAR_GRAPH_CELLS", "0")
    dom, grids, dx = _problem()
    M1 = so.make_diagonal_metric(grids, dx, L1, 3, "stretched", domain=dom)
    M2 = so.make_diagonal_metric(grids, dx, L2, 3, "stretched", domain=dom)
    a = _solver(dom, grids, dx)
    b = _solver(dom, grids, dx)
    try:
        _ortho(a, *M1)
        a.finalize()
        before = _state(a)
        _solve(a, grids, dom, 3)
        _solve(a, grids, dom, 4)   # a second solve replays the captured graphs
        with a.metricUpdate():
            _ortho(a, *M2)
        _ortho(b, *M2)
        b.finalize()
        sa_, sb = _state(a), _state(b)
        assert any(not np.array_equal(before[k], sa_[k]) for k in sa_ if isinstance(k, tuple) and isinstance(k[0], int)
                   and k[0] > 0)
        _assert_same_state(sa_, sb)
        _assert_same_solve(_solve(a, grids, dom), _solve(b, grids, dom))
        _assert_same_solve(_solve(a, grids, dom, 6), _solve(b, grids, dom, 6))
    finally:
        a.undefine()
        b.undefine()


def test_idempotent_refresh_to_the_same_metric():
    dom, grids, dx = _problem()
    M1 = so.make_diagonal_metric(grids, dx, L1, 3, "stretched", domain=dom)
    a = _solver(dom, grids, dx)
    try:
        _ortho(a, *M1)
        a.finalize()
        s0 = _state(a)
        r0 = _solve(a, grids, dom)
        with a.metricUpdate():
            _ortho(a, *M1)
        _assert_same_state(_state(a), s0)
        _assert_same_solve(_solve(a, grids, dom), r0)
    finally:
        a.undefine()


def test_uniform_flag_transitions():
    """Cartesian -> stretched -> Cartesian with other constants: flags, constants, tiles and solves follow"""
    dom, grids, dx = _problem(n=(64, 64, 64), box=(32, 32, 32), periodic=(False, False, False))
    c1, c3 = (1.0, 1.0, 1.0, 1.0), (2.0, 0.5, 1.5, 0.25)
    M2 = so.make_diagonal_metric(grids, dx, L2, 3, "stretched", domain=dom)
    a = _solver(dom, grids, dx)
    try:
        a.setMetricUniform(*c1)
        a.finalize()
        assert a.metricUniform(0) == c1
        _solve(a, grids, dom)
        for step, produce in enumerate([lambda s: _ortho(s, *M2), lambda s: s.setMetricUniform(*c3)]):
            with a.metricUpdate():
                produce(a)
            b = _solver(dom, grids, dx)
            try:
                produce(b)
                b.finalize()
                if step == 0:
                    assert a.metricUniform(0) is None
                else:
                    assert a.metricUniform(0) == c3 and a.metricUniform(a.depth() - 1) == c3
                _assert_same_state(_state(a), _state(b))
                _assert_same_solve(_solve(a, grids, dom), _solve(b, grids, dom))
            finally:
                b.undefine()
    finally:
        a.undefine()


def _bathy_depth(n, dx, d0):
    dlo, dn = (-1, -1), (n[0] + 4, n[1] + 4)
    x = (np.arange(dlo[0], dlo[0] + dn[0]) * dx[0])[:, None]
    y = (np.arange(dlo[1], dlo[1] + dn[1]) * dx[1])[None, :]
    return d0 + 0.02 * x - 0.03 * y + 0.25 * np.exp(-((x - 1.7) ** 2 + (y - 0.9) ** 2) / 0.5), dlo


@pytest.mark.parametrize("kind", ["bathymetric", "twisted"])
def test_non_diagonal_map_refresh(kind):
    from somar_amd import api as F
    n, L = (32, 32, 16), (3.0, 2.0, 1.0)
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), (False, False, False))
    grids = so.split_domain(dom.box, (16, 16, 16))
    dx = tuple(L[d] / n[d] for d in range(3))
    if kind == "bathymetric":
        (d1, dlo), (d2, _) = _bathy_depth(n, dx, 0.15), _bathy_depth(n, dx, 0.3)
        m1 = lambda s: s.setMetricMap(F.MAP_BATHYMETRIC, L, d1, dlo)   # noqa: E731
        m2 = lambda s: s.setMetricMap(F.MAP_BATHYMETRIC, L, d2, dlo)   # noqa: E731
    else:
        m1 = lambda s: s.setMetricMap(F.MAP_TWISTED, (0.05, 0.04, 0.03))   # noqa: E731
        m2 = lambda s: s.setMetricMap(F.MAP_TWISTED, (0.02, 0.06, 0.01))   # noqa: E731
    a = _solver(dom, grids, dx)
    b = _solver(dom, grids, dx)
    try:
        m1(a)
        a.finalize()
        _solve(a, grids, dom)
        with a.metricUpdate():
            m2(a)
        m2(b)
        b.finalize()
        sa_, sb = _state(a, True), _state(b, True)
        _assert_same_state(sa_, sb)
        _assert_same_solve(_solve(a, grids, dom), _solve(b, grids, dom))
    finally:
        a.undefine()
        b.undefine()


def test_full_2d_refresh():
    n, L = (32, 32, 1), (64.0, 64.0, 1.0)
    dom = so.Domain(so.Box((0, 0, 0), (n[0] - 1, n[1] - 1, 0)), (False, False, False))
    grids = so.split_domain(dom.box, (16, 16, 1))
    dx = (L[0] / n[0], L[1] / n[1], 1.0)
    M1 = so.make_full_metric_2d(grids, dx, L[:2], dom)
    M2 = so.make_full_metric_2d(grids, dx, (48.0, 80.0), dom)
    a = _solver(dom, grids, dx, ndim=2)
    b = _solver(dom, grids, dx, ndim=2)
    try:
        _full(a, *M1, ndim=2)
        a.finalize()
        _solve(a, grids, dom)
        with a.metricUpdate():
            _full(a, *M2, ndim=2)
        _full(b, *M2, ndim=2)
        b.finalize()
        _assert_same_state(_state(a, True, 2), _state(b, True, 2))
        _assert_same_solve(_solve(a, grids, dom), _solve(b, grids, dom))
    finally:
        a.undefine()
        b.undefine()


def test_heat_step_after_refresh():
    """a TGA step (scheme 2) after a refresh of a solver whose coefficients set_alpha_beta changed"""
    from somar_amd.api import F_HEAT_OLD, F_HEAT_SRC, F_PHI
    dom, grids, dx = _problem(periodic=(False, False, False))
    M1 = so.make_diagonal_metric(grids, dx, L1, 3, "stretched", domain=dom)
    M2 = so.make_diagonal_metric(grids, dx, L2, 3, "stretched", domain=dom)
    bc = [1] * 6
    dt, nu = 0.01, 0.3

    def step(s):
        upload(s, F_HEAT_OLD, so.random_field(grids, 8, domainBox=dom.box))
        upload(s, F_HEAT_SRC, so.random_field(grids, 9, domainBox=dom.box))
        st = s.heatStep(2, dt)
        return st, download_valid(s, F_PHI, grids)

    a = _solver(dom, grids, dx, alpha=1.0, beta=nu, bc_type=bc)
    b = _solver(dom, grids, dx, alpha=1.0, beta=nu, bc_type=bc)
    try:
        _ortho(a, *M1)
        a.finalize()
        step(a)
        step(a)
        a.setAlphaAndBeta(1.0, dt * nu)
        with a.metricUpdate():
            _ortho(a, *M2)
        _ortho(b, *M2)
        b.finalize()
        b.setAlphaAndBeta(1.0, dt * nu)
        _assert_same_state(_state(a), _state(b))
        _assert_same_solve(step(a), step(b))
    finally:
        a.undefine()
        b.undefine()


def _remetric(levels, L):
    """the same hierarchy (domains, boxes, spacings) with the stretched map of period L"""
    return [sa.AMRLevel(Lv.domain, Lv.grids, Lv.dx, *so.make_diagonal_metric(Lv.grids, Lv.dx, L, 3, "stretched",
                                                                              domain=Lv.domain)) for Lv in levels]


def _amr_state(s, full=False):
    return [_state(v, full) for v in s.levels]


def _amr_solve(s, levels, seed=11):
    from somar_amd.api import F_PHI, F_RHS
    for l, (Lv, v) in enumerate(zip(levels, s.levels)):
        rhs = so.random_field(Lv.grids, seed + l, domainBox=Lv.domain.box)
        upload(v, F_RHS, rhs)
        upload(v, F_PHI, so.LevelData(Lv.grids, 1))
    st = s.solveAMR(len(levels) - 1, 0)
    return st, [download_valid(v, F_PHI, Lv.grids) for Lv, v in zip(levels, s.levels)]


def _amr_tga(s, levels, dt=0.02):
    from somar_amd.api import F_HEAT_OLD, F_HEAT_SRC, F_PHI
    for l, (Lv, v) in enumerate(zip(levels, s.levels)):
        upload(v, F_HEAT_OLD, so.random_field(Lv.grids, 21 + l, domainBox=Lv.domain.box))
        upload(v, F_HEAT_SRC, so.random_field(Lv.grids, 31 + l, domainBox=Lv.domain.box))
        upload(v, F_PHI, so.LevelData(Lv.grids, 1))
    st = s.tgaStepAMR(len(levels) - 1, 0, dt)
    s.setAlphaAndBetaAMR(1.0, 1.0)   # back to the coefficients the hierarchy was created with
    return st, [download_valid(v, F_PHI, Lv.grids) for Lv, v in zip(levels, s.levels)]


def _same_amr(a, b):
    (sa_, pa), (sb, pb) = a, b
    for k in ("iters", "exitStatus", "history"):
        assert sa_[k] == sb[k], k
    for la, lb in zip(pa, pb):
        for x, y in zip(la, lb):
            np.testing.assert_array_equal(x, y)


def test_amr_refresh():
    """three levels, ratios (2, 2, 1) and (4, 1, 1) (forced MG depths, mini V-cycles): level 1 alone, then every level"""
    n, ratios = (16, 16, 8), [(2, 2, 1), (4, 1, 1)]
    fine = [[so.Box((8, 8, 0), (23, 23, 7))], [so.Box((40, 12, 0), (71, 19, 7))]]
    P = (True, False, False)
    M1 = make_amr_levels(so, sa, n, (2.0, 1.0, 0.5), P, ratios, fine)
    M2 = _remetric(M1, (1.6, 1.3, 0.4))
    a = make_gpu_amr(M1, ratios)
    try:
        _amr_solve(a, M1)
        # level 1 only, then every level
        for written in ([1], [0, 1, 2]):
            want = [M2[l] if l in written or l == 1 else M1[l] for l in range(3)]
            with a.metricUpdate():
                for l in written:
                    _ortho(a.levels[l], M2[l].Jgup, M2[l].Jinv)
            b = make_gpu_amr(want, ratios)
            try:
                for sa_, sb in zip(_amr_state(a), _amr_state(b)):
                    _assert_same_state(sa_, sb)
                _same_amr(_amr_solve(a, want), _amr_solve(b, want))
                _same_amr(_amr_tga(a, want), _amr_tga(b, want))
            finally:
                b.undefine()
    finally:
        a.undefine()


def test_amr_leptic_attachment_refresh():
    from somar_amd import api as F
    N_, ratios = (32, 32, 8), [(2, 2, 1)]
    fine = [[so.Box((16, 16, 0), (31, 47, 7)), so.Box((32, 16, 0), (47, 47, 7))]]
    P = (False, False, False)
    M1 = make_amr_levels(so, sa, N_, (1.0, 1.0, 0.005), P, ratios, fine, cbox=(16, 16, 8))
    M2 = _remetric(M1, (0.9, 1.1, 0.005))

    def gpu(levels):
        s = make_gpu_amr(levels, ratios, imax=4)
        lp = F.LepticParams()
        F._ck(F.lib().somar_leptic_params_default(lp))
        lp.domain_height = 0.005
        s.enableLeptic(lp)
        return s

    def run(s, levels):
        for l, (Lv, v) in enumerate(zip(levels, s.levels)):
            upload(v, F.F_RHS, so.random_field(Lv.grids, 40 + l, domainBox=Lv.domain.box))
            upload(v, F.F_PHI, so.LevelData(Lv.grids, 1))
        st = s.solveAMRLeptic(1, 0)
        return st, [download_valid(v, F.F_PHI, Lv.grids) for Lv, v in zip(levels, s.levels)]

    a = gpu(M1)
    b = gpu(M2)
    try:
        run(a, M1)
        with a.metricUpdate():
            for l in range(2):
                _ortho(a.levels[l], M2[l].Jgup, M2[l].Jinv)
        _same_amr(run(a, M2), run(b, M2))
    finally:
        a.undefine()
        b.undefine()


def test_leptic_handle_refresh():
    from somar_amd import api as F
    from somar_amd.api import LevelLepticSolver
    n, Lz = (32, 32, 8), 0.005
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), (False, False, False))
    grids = so.split_domain(dom.box, (16, 16, 8))
    dx = (1.0 / n[0], 1.0 / n[1], Lz / n[2])
    M1 = so.make_diagonal_metric(grids, dx, (1.0, 1.0, Lz), 3, "stretched", domain=dom)
    M2 = so.make_diagonal_metric(grids, dx, (0.8, 1.3, Lz), 3, "stretched", domain=dom)

    def make(M):
        s = LevelLepticSolver()
        s.params.domain_height = Lz
        s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
        _ortho(s.level, *M)
        s.finalize()
        return s

    def run(s):
        upload(s.level, F.F_RHS, so.random_field(grids, 50, domainBox=dom.box))
        upload(s.level, F.F_PHI, so.LevelData(grids, 1))
        st = s.solve(False)
        return st, download_valid(s.level, F.F_PHI, grids)

    a, b = make(M1), make(M2)
    try:
        run(a)
        with a.level.metricUpdate():
            _ortho(a.level, *M2)
        (sa_, pa), (sb, pb) = run(a), run(b)
        assert sa_ == sb
        for x, y in zip(pa, pb):
            np.testing.assert_array_equal(x, y)
    finally:
        a.undefine()
        b.undefine()


def test_refusals():
    from somar_amd.api import F_PHI, F_RHS, SomarError
    dom, grids, dx = _problem()
    M1 = so.make_diagonal_metric(grids, dx, L1, 3, "stretched", domain=dom)
    a = _solver(dom, grids, dx)
    try:
        with pytest.raises(SomarError, match="not finalized"):
            with a.metricUpdate():
                pass
        _ortho(a, *M1)
        a.finalize()
        with pytest.raises(SomarError, match="after finalize"):
            _ortho(a, *M1)
        with pytest.raises(SomarError, match="without metric_update_begin"):
            from somar_amd import api as F
            F._ck(F.lib().somar_solver_metric_update_end(a._h))
        with a.metricUpdate():
            with pytest.raises(SomarError, match="already open"):
                with a.metricUpdate():
                    pass
            with pytest.raises(SomarError, match="while a metric update is open"):
                a.solveResident(True, False)
            with pytest.raises(SomarError, match="while a metric update is open"):
                a.heatStep(0, 0.1)
            with pytest.raises(SomarError, match="finalized with a diagonal metric"):
                a.setMetricMap(2 + 1, (0.05, 0.04, 0.03))
            _ortho(a, *M1)
        upload(a, F_RHS, so.random_field(grids, 5, domainBox=dom.box))
        a.solveResident(True, False)
        assert len(download_valid(a, F_PHI, grids)) == len(grids)
    finally:
        a.undefine()
    n, L = (32, 32, 16), (3.0, 2.0, 1.0)
    dom = so.Domain(so.Box((0, 0, 0), tuple(x - 1 for x in n)), (False, False, False))
    grids = so.split_domain(dom.box, (16, 16, 16))
    b = _solver(dom, grids, tuple(L[d] / n[d] for d in range(3)))
    try:
        b.setMetricMap(3, (0.05, 0.04, 0.03))
        b.finalize()
        with b.metricUpdate():
            with pytest.raises(SomarError, match="non-diagonal metric"):
                b.setMetricUniform(1.0, 1.0, 1.0, 1.0)
            b.setMetricMap(3, (0.05, 0.04, 0.03))
    finally:
        b.undefine()
    # a level of a hierarchy goes through the hierarchy's pair
    ratios, fine = [(2, 2, 1)], [[so.Box((8, 8, 0), (23, 23, 15))]]
    M = make_amr_levels(so, sa, (16, 16, 16), (1.0, 1.0, 1.0), (False, False, False), ratios, fine, cbox=8)
    h = make_gpu_amr(M, ratios)
    try:
        with pytest.raises(SomarError, match="goes through the hierarchy"):
            with h.levels[1].metricUpdate():
                pass
        with h.metricUpdate():
            with pytest.raises(SomarError, match="while a metric update is open"):
                _amr_solve(h, M)
    finally:
        h.undefine()


# ---- two ranks over the shared-memory transport on one GPU: the agglomerated tail is refreshed too ------------------------
def _rank(rank, nranks, name, q):
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, os.path.dirname(here))
        from somar_amd import api as F
        comm = F.comm_create_shm(name, rank, nranks) if nranks > 1 else None
        dom = so.Domain(so.Box((0, 0, 0), (31, 31, 31)), (False, True, False))
        grids = so.split_domain(dom.box, 16)
        dx = (2.0 / 32, 1.0 / 32, 1.0 / 32)
        owner = [i % nranks for i in range(len(grids))]
        M1 = so.make_diagonal_metric(grids, dx, (2.0, 1.0, 1.0), 3, "stretched", domain=dom)
        M2 = so.make_diagonal_metric(grids, dx, (1.7, 1.2, 0.9), 3, "stretched", domain=dom)

        def make(M):
            from somar_amd import AMRPressureSolver
            s = AMRPressureSolver()
            s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], owner=owner, comm=comm)
            _ortho(s, *M)
            s.finalize()
            return s

        def run(s):
            rhs = so.random_field(grids, 5, domainBox=dom.box)
            so.remove_weighted_mean(rhs, M2[1])   # a compatible right-hand side (Neumann / periodic)
            for p in range(s.num_local_patches):
                _, _, gi = s.patch_box(p)
                s.upload(F.F_RHS, p, np.asfortranarray(rhs[gi].a[..., 0]), rhs.ghost)
            st = s.solveResident(True, False)
            phi = {}
            for p in range(s.num_local_patches):
                _, _, gi = s.patch_box(p)
                phi[gi] = s.download(F.F_PHI, p, (0, 0, 0))
            return st, phi

        a, b = make(M1), make(M2)
        run(a)
        with a.metricUpdate():
            _ortho(a, *M2)
        (sa_, pa), (sb, pb) = run(a), run(b)
        assert sa_["iters"] == sb["iters"] and sa_["history"] == sb["history"]
        for gi in pa:
            np.testing.assert_array_equal(pa[gi], pb[gi])
        q.put((rank, "ok", sa_["iters"], sa_["history"], {gi: v for gi, v in pa.items()}))
        a.undefine()
        b.undefine()
        if comm is not None:
            F.comm_destroy(comm)
    except Exception:
        q.put((rank, traceback.format_exc(), None, None, None))


def test_sharded_refresh_matches_fresh_and_one_rank():
    ctx = mp.get_context("spawn")
    results = {}
    for nranks in (1, 2):
        q = ctx.Queue()
        name = "/somar_mr_" + uuid.uuid4().hex[:12]
        procs = [ctx.Process(target=_rank, args=(r, nranks, name, q)) for r in range(nranks)]
        for p in procs:
            p.start()
        got = [q.get(timeout=600) for _ in procs]
        for p in procs:
            p.join(60)
        for r, status, *_ in got:
            assert status == "ok", "rank %d:\n%s" % (r, status)
        results[nranks] = got
    one = results[1][0]
    for _, _, iters, hist, phi in results[2]:
        assert iters == one[2]
        # to 1e-10 of the initial residual / of the solution's scale: the two layouts add the large levels' sums in another order
        np.testing.assert_allclose(hist, one[3], rtol=0, atol=1e-10 * one[3][0])
        scale = max(float(np.max(np.abs(v))) for v in one[4].values())
        for gi, v in phi.items():
            np.testing.assert_allclose(v, one[4][gi], rtol=0, atol=1e-10 * scale)
