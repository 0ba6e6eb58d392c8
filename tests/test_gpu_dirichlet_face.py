"""Position-dependent Dirichlet values on the GPU (somar_solver_set_bc_face_values: GHOST_DIRI_FACE ops of both operator
families) against the constant path, the oracle patched with the same planes (tests/diri_face.py), and an analytic
solution."""
import multiprocessing as mp
import os
import traceback
import uuid

import numpy as np
import pytest

from diri_face import patch, step_plane
from helpers import download_valid, make_problem, max_rel_diff, upload, valid_of

pytestmark = pytest.mark.gpu
D, N = 1, 0

CASES = [   # the shapes of test_gpu_dirichlet.py: n, box, periodic, bc types, alpha, beta
    ((16, 16, 8), 8, (False, False, False), [(D, D), (N, N), (N, D)], 0.0, 1.0),
    ((16, 16, 8), 8, (False, True, False), [(D, N), (N, N), (D, D)], 0.0, 1.0),
    ((32, 16, 16), (16, 8, 8), (False, False, False), [(D, D), (D, D), (D, D)], 1.0, -1e-3),
]
VALS = [(0.5, -1.0), (0.75, 2.0), (0.25, -1.5)]   # constants of the Dirichlet sides


def _vals(types, vals=VALS):
    """vals on the Dirichlet sides, 0 on the Neumann ones (the GPU takes homogeneous Neumann sides only)"""
    return [[vals[d][s] if types[d][s] == D else 0.0 for s in (0, 1)] for d in range(3)]


@pytest.fixture(params=["direct", "march", "fused"])
def kernel_path(request, monkeypatch):
    """the three kernel paths of test_gpu_dirichlet.py"""
    if request.param == "march":
        monkeypatch.setenv("SOMAR_MARCH_MIN_CELLS", "0")
    elif request.param == "fused":
        monkeypatch.setenv("SOMAR_FUSED_MIN_CELLS", "0")
    return request.param


def _sides(types, ndim=3):
    return [(d, s) for d in range(ndim) for s in (0, 1) if types[d][s] == D]


def _planes(dom, dx, types, ndim=3, L0=1.0):
    return {(d, s): step_plane(dom.box, dx, d, s, L0=L0, amp=0.25 + 0.1 * d, hot=1.0 - s, cold=-0.5 + 0.2 * d)
            for d, s in _sides(types, ndim)}


def _sheared(so):
    n, L = (16, 16, 8), (2.0, 1.0, 0.5)
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), (False, False, False))
    grids = so.split_domain(dom.box, 8)
    dx = tuple(L[d] / n[d] for d in range(3))
    Jgup, Jinv = so.make_full_metric(grids, dx, L, dom)
    return dom, grids, dx, Jgup, Jinv


def _problem(so, which):
    """-> dom, grids, dx, Jgup, Jinv, types, alpha, beta, full, ndim"""
    if which == "sheared":   # test_dirichlet_sides_with_a_nondiagonal_metric
        return _sheared(so) + ([(D, D), (N, D), (D, N)], 1.0, -0.02, True, 3)
    if which == "2d":
        n, L = (32, 24), (1.0, 1.5)
        dom = so.Domain(so.Box((0, 0, 0), (n[0] - 1, n[1] - 1, 0)), (False, False, False))
        grids = so.split_domain(dom.box, (16, 12, 1))
        dx = (L[0] / n[0], L[1] / n[1], 1.0)
        Jgup, Jinv = so.make_diagonal_metric(grids, dx, L + (1.0,), 2, "stretched", domain=dom)
        return dom, grids, dx, Jgup, Jinv, [(D, N), (N, D), (N, N)], 0.0, 1.0, False, 2
    n, bs, per, types, alpha, beta = CASES[which]
    dom, grids, dx, Jgup, Jinv = make_problem(so, n, bs, "stretched", per, (1.0, 1.0, 0.5))
    return dom, grids, dx, Jgup, Jinv, types, alpha, beta, False, 3


def _oracle(so, prob, planes, vals=VALS):
    dom, grids, dx, Jgup, Jinv, types, alpha, beta, full, ndim = prob
    bc = so.BCHolder([list(t) for t in types], _vals(types, vals))
    for (d, s), pl in planes.items():
        bc.values[d][s] = pl
    fac = so.Factory(dom, grids, dx, bc, Jgup, Jinv, alpha=alpha, beta=beta, isDiagonal=not full, ndim=ndim)
    return so.AMRMultiGrid(fac, so.BiCGStab())


def _gpu(prob, planes, owner=None, comm=None, eps=None, imax=None, vals=VALS):
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv, types, alpha, beta, full, ndim = prob
    s = AMRPressureSolver()
    s.setSpaceDim(ndim)
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax if imax is None else imax, p.eps if eps is None else eps, -1,
                         p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang, p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], owner=owner, alpha=alpha,
             beta=beta, comm=comm, bc_type=[t for pair in types for t in pair])
    s.setBCValues([v for pair in vals for v in pair])
    for (d, side), pl in planes.items():
        s.setBCFaceValues(d, side, pl)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        if full:
            s.setMetricFull(q, *[np.asfortranarray(Jgup[gi][d].a) for d in range(3)], np.asfortranarray(Jinv[gi].a[..., 0]))
        else:
            jg = [np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(ndim)] + [None] * (3 - ndim)
            s.setMetricOrtho(q, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return s


def _solve_gpu(s, grids, rhs, ndim=3):
    """inhomogeneous solve from zero; -> stats, valid phi per local patch"""
    gb, gx = [], []
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        gb.append(np.asfortranarray(rhs[gi].a[..., 0]))
        gx.append(np.zeros(tuple(n + 2 for n in grids[gi].size()[:ndim]) + (1,) * (3 - ndim), order="F"))
    st = s.solve(gx, gb, 0, 0, True, False, phi_ghost=(1, 1, 1) if ndim == 3 else (1, 1, 0))
    return st, [a[1:-1, 1:-1, 1:-1] if ndim == 3 else a[1:-1, 1:-1, :] for a in gx]


def _pieces(s, so, grids, dom, phi, rhs):
    """GPU residual_bc / apply_op_bc with homogeneous = 0 on the resident phi / rhs"""
    from somar_amd import api as F
    upload(s, F.F_PHI, phi)
    upload(s, F.F_RHS, rhs)
    s.residualBC(F.F_RES, F.F_PHI, F.F_RHS, False)
    r = download_valid(s, F.F_RES, grids)
    s.applyOpBC(F.F_RES, F.F_PHI, False)
    a = download_valid(s, F.F_RES, grids)
    return r, a


def _fields(so, grids, dom, ndim=3):
    return so.random_field(grids, 7, (1, 1, 1) if ndim == 3 else (1, 1, 0), dom.box), so.random_field(grids, 8, (0, 0, 0), dom.box)


# ---- 1. a constant plane is the constant path, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("which", [0, "sheared"])
def test_constant_plane_is_the_constant_path_bit_for_bit(oracle, kernel_path, which):
    so = oracle
    prob = _problem(so, which)
    dom, grids = prob[0], prob[1]
    const = {(d, s): np.full([dom.box.size()[q] for q in range(3) if q != d], VALS[d][s], order="F")
             for d, s in _sides(prob[5])}
    a, b = _gpu(prob, {}), _gpu(prob, const)
    try:
        phi, rhs = _fields(so, grids, dom)
        ra, aa = _pieces(a, so, grids, dom, phi, rhs)
        rb, ab = _pieces(b, so, grids, dom, phi, rhs)
        for x, y in zip(ra + aa, rb + ab):
            np.testing.assert_array_equal(x, y)
        st_a, xa = _solve_gpu(a, grids, rhs)
        st_b, xb = _solve_gpu(b, grids, rhs)
        assert (st_a["iters"], st_a["exitStatus"]) == (st_b["iters"], st_b["exitStatus"])
        np.testing.assert_array_equal(st_a["history"], st_b["history"])
        for x, y in zip(xa, xb):
            np.testing.assert_array_equal(x, y)
    finally:
        a.undefine()
        b.undefine()


# ---- 2. varying planes against the patched oracle ------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2, "sheared", "2d"])
def test_varying_plane_matches_the_patched_oracle(oracle, monkeypatch, which):
    so = oracle
    patch(monkeypatch, so)
    prob = _problem(so, which)
    dom, grids, dx, ndim = prob[0], prob[1], prob[2], prob[9]
    planes = _planes(dom, dx, prob[5], ndim)
    amr = _oracle(so, prob, planes)
    gpu = _gpu(prob, planes)
    try:
        phi, rhs = _fields(so, grids, dom, ndim)
        r, a = _pieces(gpu, so, grids, dom, phi, rhs)
        res, lhs = so.LevelData(grids, 1), so.LevelData(grids, 1)
        amr.op.residual(res, phi, rhs, False)
        amr.op.apply_op(lhs, phi, False)
        for x, y in zip(r, valid_of(res)):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a, valid_of(lhs)):
            np.testing.assert_array_equal(x, y)
        x = so.LevelData(grids, 1, (1, 1, 1) if ndim == 3 else (1, 1, 0))
        amr.solve(x, rhs, zeroPhi=True, forceHomogeneous=False)
        st, got = _solve_gpu(gpu, grids, rhs, ndim)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-13 * amr.history[0])
        assert max_rel_diff(got, valid_of(x)) < 1e-8
    finally:
        gpu.undefine()


# ---- 3. heat integrators ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_heat_step_with_a_varying_top(oracle, monkeypatch, scheme):
    from somar_amd import api as F
    so = oracle
    patch(monkeypatch, so)
    dom, grids, dx, Jgup, Jinv = make_problem(so, (16, 16, 8), 8, "stretched", (False, True, False), (1.0, 1.0, 0.5))
    prob = (dom, grids, dx, Jgup, Jinv, [(D, D), (N, N), (N, D)], 1.0, 5e-2, False, 3)
    planes = {(2, 1): step_plane(dom.box, dx, 2, 1)}
    amr = _oracle(so, prob, planes)
    gpu = _gpu(prob, planes)
    try:
        dt = 0.2
        old = so.random_field(grids, 3, (1, 1, 1), dom.box)
        src = so.random_field(grids, 4, (0, 0, 0), dom.box)
        upload(gpu, F.F_HEAT_OLD, old)
        upload(gpu, F.F_HEAT_SRC, src)
        new = so.LevelData(grids, 1, (1, 1, 1))
        [so.level_backward_euler, so.level_crank_nicolson, so.level_tga][scheme](amr, new, old, src, dt)
        st = gpu.heatStep(scheme, dt)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-13 * amr.history[0])
        assert max_rel_diff(download_valid(gpu, F.F_PHI, grids), valid_of(new)) < 1e-10
    finally:
        gpu.undefine()


@pytest.mark.parametrize("scheme", [0, 2])
def test_amr_heat_step_on_the_fine_level_with_a_varying_top(monkeypatch, scheme):
    from oracle import somar_amr as sa
    from oracle import somar_oracle as so
    from somar_amd import AMRPressureSolver
    from somar_amd import api as F
    from helpers import make_amr_levels
    patch(monkeypatch, so)
    ratios = [(2, 2, 2)]
    fine = [[so.Box((8, 8, 4), (23, 15, 15)), so.Box((8, 16, 4), (23, 23, 15))]]
    types, nu = [(D, D), (D, N), (N, D)], 0.05
    levels = make_amr_levels(so, sa, (16, 16, 8), (1.0, 1.0, 0.5), (False, False, False), ratios, fine, cbox=8)
    planes = [step_plane(L.domain.box, L.dx, 2, 1) for L in levels]
    bc = so.BCHolder([list(t) for t in types], _vals(types))
    bc.values[2][1] = {tuple(L.domain.box.size()): pl for L, pl in zip(levels, planes)}
    comp = sa.AMRComposite(levels, ratios, bc, so.BiCGStab(), alpha=1.0, beta=nu)
    s = AMRPressureSolver()
    L0 = levels[0]
    s.defineAMR(L0.domain.box.lo, L0.domain.box.hi, L0.domain.periodic, L0.dx, ratios,
                [[(g.lo, g.hi) for g in L.grids] for L in levels], alpha=1.0, beta=nu, bc_type=[t for q in types for t in q])
    for L, v, pl in zip(levels, s.levels, planes):
        v.setBCValues([x for q in VALS for x in q])
        v.setBCFaceValues(2, 1, pl)
        for p_ in range(v.num_local_patches):
            _, _, gi = v.patch_box(p_)
            jg = [np.asfortranarray(L.Jgup[gi][d].a[..., d]) for d in range(3)]
            v.setMetricOrtho(p_, jg[0], jg[1], jg[2], np.asfortranarray(L.Jinv[gi].a[..., 0]))
    s.finalize()
    try:
        l, dt = 1, 0.2
        g1, g0 = levels[1].grids, levels[0].grids
        old = so.random_field(g1, 3, (1, 1, 1), levels[1].domain.box)
        src = so.random_field(g1, 4, (0, 0, 0), levels[1].domain.box)
        cold = so.random_field(g0, 5, (1, 1, 1), levels[0].domain.box)
        cnew = so.random_field(g0, 6, (1, 1, 1), levels[0].domain.box)
        new = so.LevelData(g1, 1, (1, 1, 1))
        flux = so.FluxData(g1, 1)
        times = dict(oldTime=0.25, crseOldTime=0.0, crseNewTime=1.0)
        sa.amr_level_heat(comp, l, scheme, new, old, src, cold, cnew, dt=dt, zeroPhi=True, flux=flux, **times)
        upload(s.levels[1], F.F_HEAT_OLD, old)
        upload(s.levels[1], F.F_HEAT_SRC, src)
        upload(s.levels[0], F.F_HEAT_OLD, cold)
        upload(s.levels[0], F.F_PHI, cnew)
        st = s.heatStepAMR(l, scheme, dt, True, **times)
        assert st["iters"] == comp.iters and st["exitStatus"] == comp.exitStatus
        np.testing.assert_allclose(st["history"], comp.history, rtol=1e-10, atol=1e-13 * comp.history[0])
        assert max_rel_diff(download_valid(s.levels[1], F.F_PHI, g1), valid_of(new)) < 1e-10
        # heatFlux on the z faces inside the domain (test_gpu_amr_heat.py's comparison)
        v = s.levels[1]
        top = levels[1].domain.box.hi[2]
        for q in range(v.num_local_patches):
            lo, hi, gi = v.patch_box(q)
            got, want = v.heatFlux(2, q), flux[gi][2].a[..., 0]
            b = got.shape[2] - (1 if hi[2] == top else 0)
            scale = float(np.max(np.abs(want))) or 1.0
            np.testing.assert_allclose(got[:, :, :b], want[:, :, :b], rtol=0, atol=1e-9 * scale)
    finally:
        s.undefine()


# ---- 4. AMR composite solve ------------------------------------------------------------------------------------------
def test_amr_composite_solve_with_a_plane_per_level(oracle, monkeypatch):
    from oracle import somar_amr as am
    from somar_amd import AMRPressureSolver
    from somar_amd import api as F
    from helpers import make_amr_levels
    so = oracle
    patch(monkeypatch, so)
    types = [(D, D), (N, N), (N, D)]
    ratios = [(2, 2, 1)]
    fb = [[so.Box((8, 8, 0), (23, 23, 7))]]
    levels = make_amr_levels(so, am, (16, 16, 8), (2.0, 1.0, 0.5), (False, False, False), ratios, fb)
    bc = so.BCHolder([list(t) for t in types], _vals(types))
    planes = [{(d, s): step_plane(L.domain.box, L.dx, d, s, L0=2.0 if d else 1.0, hot=1.0 - s) for d, s in _sides(types)}
              for L in levels]
    for d, s in _sides(types):
        bc.values[d][s] = {tuple(L.domain.box.size()): pl[(d, s)] for L, pl in zip(levels, planes)}
    comp = am.AMRComposite(levels, ratios, bc, so.BiCGStab())
    s = AMRPressureSolver()
    L0 = levels[0]
    s.defineAMR(L0.domain.box.lo, L0.domain.box.hi, L0.domain.periodic, L0.dx, ratios,
                [[(g.lo, g.hi) for g in L.grids] for L in levels], bc_type=[t for pair in types for t in pair])
    for L, v, pl in zip(levels, s.levels, planes):
        v.setBCValues([x for pair in VALS for x in pair])
        for (d, side), p_ in pl.items():
            v.setBCFaceValues(d, side, p_)
        for p_ in range(v.num_local_patches):
            _, _, gi = v.patch_box(p_)
            jg = [np.asfortranarray(L.Jgup[gi][d].a[..., d]) for d in range(3)]
            v.setMetricOrtho(p_, jg[0], jg[1], jg[2], np.asfortranarray(L.Jinv[gi].a[..., 0]))
    s.finalize()
    try:
        rhs = [so.random_field(L.grids, 50 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
        comp.zero_covered(0, rhs[0])
        sol = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.solve(sol, rhs, 1, 0, forceHomogeneous=False)
        for l, v in enumerate(s.levels):
            upload(v, F.F_RHS, rhs[l])
        st = s.solveAMR(1, 0, zeroPhi=True, forceHomogeneous=False)
        assert st["iters"] == comp.iters and st["exitStatus"] == comp.exitStatus
        np.testing.assert_allclose(st["history"], comp.history, rtol=1e-10, atol=0.0)
        for l in (0, 1):
            assert max_rel_diff(download_valid(s.levels[l], F.F_PHI, levels[l].grids), valid_of(sol[l])) < 1e-8
    finally:
        s.undefine()


# ---- 5. new values after finalize ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, "sheared"])
def test_update_after_finalize_and_back_to_constants(oracle, which):
    so = oracle
    prob = _problem(so, which)
    dom, grids, dx = prob[0], prob[1], prob[2]
    pa = _planes(dom, dx, prob[5])
    pb = {k: np.asfortranarray(-0.5 * v + 0.125) for k, v in pa.items()}
    s, fresh, const = _gpu(prob, pa), _gpu(prob, pb), _gpu(prob, {})
    try:
        _, rhs = _fields(so, grids, dom)
        st0, x0 = _solve_gpu(s, grids, rhs)
        for (d, side), pl in pb.items():
            s.setBCFaceValues(d, side, pl)
        st1, x1 = _solve_gpu(s, grids, rhs)
        stf, xf = _solve_gpu(fresh, grids, rhs)
        assert st1["history"] != st0["history"]
        assert (st1["iters"], st1["exitStatus"]) == (stf["iters"], stf["exitStatus"])
        np.testing.assert_array_equal(st1["history"], stf["history"])
        for a, b in zip(x1, xf):
            np.testing.assert_array_equal(a, b)
        for d, side in pb:
            s.setBCFaceValues(d, side, None)
        st2, x2 = _solve_gpu(s, grids, rhs)
        stc, xc = _solve_gpu(const, grids, rhs)
        assert (st2["iters"], st2["exitStatus"]) == (stc["iters"], stc["exitStatus"])
        np.testing.assert_array_equal(st2["history"], stc["history"])
        for a, b in zip(x2, xc):
            np.testing.assert_array_equal(a, b)
    finally:
        for q in (s, fresh, const):
            q.undefine()


# ---- 6. analytic anchor --------------------------------------------------------------------------------------------
def test_second_order_convergence_to_an_analytic_solution(oracle):
    """u = cos(pi x) sinh(pi z) / sinh(pi) on [0,1]^3 solves Laplace's equation with homogeneous Neumann x and y sides,
    u = 0 at the bottom and u = cos(pi x) on the top: the top is a face-valued side"""
    so = oracle
    errs = []
    for n in (16, 32, 64):
        dom = so.Domain(so.Box((0, 0, 0), (n - 1, 3, n - 1)), (False, False, False))
        grids = so.split_domain(dom.box, (16, 4, 16))
        dx = (1.0 / n, 0.25, 1.0 / n)
        Jgup, Jinv = so.make_diagonal_metric(grids, dx, (1.0, 1.0, 1.0), 3, "cartesian", domain=dom)
        prob = (dom, grids, dx, Jgup, Jinv, [(N, N), (N, N), (D, D)], 0.0, 1.0, False, 3)
        xf = (np.arange(n) + 0.5) / n
        top = np.asfortranarray(np.repeat(np.cos(np.pi * xf)[:, None], 4, axis=1))
        s = _gpu(prob, {(2, 1): top}, eps=1e-12, imax=60, vals=[(0.0, 0.0)] * 3)
        try:
            rhs = so.LevelData(grids, 1)
            st, x = _solve_gpu(s, grids, rhs)
            assert st["history"][-1] <= 1e-12 * st["history"][0], st
            err = 0.0
            for q in range(s.num_local_patches):
                _, _, gi = s.patch_box(q)
                g = grids[gi]
                xc = (np.arange(g.lo[0], g.hi[0] + 1) + 0.5) / n
                zc = (np.arange(g.lo[2], g.hi[2] + 1) + 0.5) / n
                u = np.cos(np.pi * xc)[:, None, None] * np.sinh(np.pi * zc)[None, None, :] / np.sinh(np.pi)
                err = max(err, float(np.max(np.abs(x[q] - u))))
            errs.append(err)
        finally:
            s.undefine()
    assert errs[0] / errs[1] >= 3.5 and errs[1] / errs[2] >= 3.5, errs


# ---- 7. two ranks on one GPU ---------------------------------------------------------------------------------------
def _worker(rank, nranks, name, q):
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, here)
        sys.path.insert(0, os.path.dirname(here))
        from oracle import somar_oracle as so
        from somar_amd import api as F
        import diri_face
        from helpers import download_valid, make_problem, upload, valid_of
        diri_face.install(so)
        comm = F.comm_create_shm(name, rank, nranks)
        dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 32, 16), 16, "stretched", (False, False, False), (1.0, 1.0, 0.5))
        owner = [i % nranks for i in range(len(grids))]
        types = [(N, N), (D, N), (N, D)]
        prob = (dom, grids, dx, Jgup, Jinv, types, 0.0, 1.0, False, 3)
        planes = {(1, 0): diri_face.step_plane(dom.box, dx, 1, 0), (2, 1): diri_face.step_plane(dom.box, dx, 2, 1)}
        top = [i for i, g in enumerate(grids) if g.hi[2] == dom.box.hi[2]]
        assert {owner[i] for i in top} == set(range(nranks)), "the face-valued top must be split across the ranks"
        amr = _oracle(so, prob, planes)
        gpu = _gpu(prob, planes, owner=owner, comm=comm)
        phi, rhs = so.random_field(grids, 7, (1, 1, 1), dom.box), so.random_field(grids, 8, (0, 0, 0), dom.box)
        upload(gpu, F.F_PHI, phi)
        upload(gpu, F.F_RHS, rhs)
        gpu.residualBC(F.F_RES, F.F_PHI, F.F_RHS, False)
        res = so.LevelData(grids, 1)
        amr.op.residual(res, phi, rhs, False)
        n = 0
        for g, w in zip(download_valid(gpu, F.F_RES, grids), valid_of(res)):
            if g is not None:
                np.testing.assert_array_equal(g, w)
                n += 1
        assert n > 0
        x = so.LevelData(grids, 1, (1, 1, 1))
        amr.solve(x, rhs, zeroPhi=True, forceHomogeneous=False)
        st, _ = _solve_gpu(gpu, grids, rhs)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-13 * amr.history[0])
        gpu.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_two_ranks_sharing_one_gpu():
    nranks = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/somar_%s" % uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=_worker, args=(r, nranks, name, q)) for r in range(nranks)]
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


# ---- 8. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    from somar_amd import LevelLepticSolver, SomarError
    from somar_amd import api as F
    so = oracle
    prob = _problem(so, 1)   # x: (D, N), y periodic, z: (D, D)
    dom = prob[0]
    plane = np.zeros((dom.box.size()[1], dom.box.size()[2]), order="F")
    s = _gpu(prob, {})
    try:
        with pytest.raises(SomarError, match="not a Dirichlet side"):
            s.setBCFaceValues(0, 1, plane)
        with pytest.raises(SomarError, match="periodic"):
            s.setBCFaceValues(1, 0, plane)
        for d, side in ((3, 0), (-1, 0), (0, 2), (0, -1)):
            assert F.lib().somar_solver_set_bc_face_values(s._h, d, side, None) != 0
            assert b"dir must be" in F.lib().somar_last_error()
    finally:
        s.undefine()
    # leptic: refused whichever order the calls come in
    n, dx = (16, 16, 8), (1.0 / 16, 1.0 / 16, 0.005 / 8)
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), (False, False, False))
    grids = so.split_domain(dom.box, (16, 16, 8))
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, (1.0, 1.0, 0.005), 3, "stretched", domain=dom)
    top = np.ones((n[0], n[1]), order="F")
    for before in (True, False):
        lep = LevelLepticSolver()
        lep.params.max_order = 2
        lep.params.domain_height = 0.005
        lep.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], bc_type=[N, N, N, N, N, D])
        try:
            lv = lep.level
            if before:
                lv.setBCFaceValues(2, 1, top)
            for p_ in range(lv.num_local_patches):
                _, _, gi = lv.patch_box(p_)
                jg = [np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)]
                lv.setMetricOrtho(p_, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
            lep.finalize()
            if not before:
                lv.setBCFaceValues(2, 1, top)
            with pytest.raises(SomarError, match="leptic path does not read them"):
                lep.solve()
        finally:
            lep.undefine()
