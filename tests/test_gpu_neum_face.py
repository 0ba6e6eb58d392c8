"""Position-dependent Neumann values on a diagonal metric on the GPU (somar_solver_set_neum_face_values: GHOST_NEUM_FACE
ghosts, the planes' values as the boundary fluxes of the inhomogeneous operator) against the oracle wrapped with the same
planes (tests/neum_face.py), through the C ABI.  Planes are smooth plus a step (diri_face.step_plane)."""
import multiprocessing as mp
import os
import traceback
import uuid

import numpy as np
import pytest

from helpers import download_valid, make_amr_levels, make_problem, max_rel_diff, upload, valid_of
from neum_face import patch, step_plane, transverse

pytestmark = pytest.mark.gpu
D, N = 1, 0
DVAL = 0.75                                    # the constant of every Dirichlet side
TYPES = [(N, N), (N, D), (N, N)]               # x and z Neumann, the high y side Dirichlet
SIDES = [(0, 0), (2, 1)]                       # face-valued: one low and one high side of different directions
G3, G2 = (1, 1, 1), (1, 1, 0)


def _problem(so, which):
    """-> dom, grids, dx, Jgup, Jinv, types, alpha, beta, ndim, face-valued sides"""
    if which == "2d":
        n, L = (32, 16), (1.0, 1.5)
        dom = so.Domain(so.Box((0, 0, 0), (n[0] - 1, n[1] - 1, 0)), (False, False, False))
        grids = so.split_domain(dom.box, (16, 16, 1))
        dx = (L[0] / n[0], L[1] / n[1], 1.0)
        Jgup, Jinv = so.make_diagonal_metric(grids, dx, L + (1.0,), 2, "stretched", domain=dom)
        return dom, grids, dx, Jgup, Jinv, [(N, D), (N, N), (N, N)], 0.0, 1.0, 2, [(0, 0), (1, 1)]
    types, alpha, beta, per = TYPES, 0.0, 1.0, (False, False, False)
    if which == "helmholtz":
        alpha, beta = 1.0, -0.05
    elif which == "allneum":
        types = [(N, N)] * 3
    elif which == "allneum-helmholtz":
        types, alpha, beta = [(N, N)] * 3, 1.0, -0.05
    elif which == "periodic":
        types, per = [(N, N), (N, N), (N, D)], (False, True, False)
    variant = "cartesian" if which == "uniform" else "stretched"
    # 32 x 16 x 16 in two boxes split in x
    dom, grids, dx, Jgup, Jinv = make_problem(so, (32, 16, 16), 16, variant, per, (2.0, 1.0, 0.5))
    assert len(grids) == 2
    sides = [(0, 0), (2, 0)] if which == "periodic" else SIDES
    return dom, grids, dx, Jgup, Jinv, types, alpha, beta, 3, sides


def _planes(dom, dx, sides, scale=1.0):
    return {(d, s): np.asfortranarray(scale * step_plane(dom.box, dx, d, s, L0=2.0 if d else 1.0, amp=0.25 + 0.1 * d,
                                                         hot=1.0 - s, cold=-0.5 + 0.2 * d)) for d, s in sides}


def _bc(so, types, planes):
    bc = so.BCHolder([list(t) for t in types], [[DVAL if t == D else 0.0 for t in pair] for pair in types])
    for (d, s), pl in planes.items():
        bc.values[d][s] = pl
    return bc


def _oracle(so, prob, planes):
    dom, grids, dx, Jgup, Jinv, types, alpha, beta, ndim, _ = prob
    fac = so.Factory(dom, grids, dx, _bc(so, types, planes), Jgup, Jinv, alpha=alpha, beta=beta, isDiagonal=True, ndim=ndim)
    return so.AMRMultiGrid(fac, so.BiCGStab())


def _gpu(prob, planes, owner=None, comm=None):
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv, types, alpha, beta, ndim, _ = prob
    s = AMRPressureSolver()
    s.setSpaceDim(ndim)
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], owner=owner, alpha=alpha,
             beta=beta, comm=comm, bc_type=[t for pair in types for t in pair])
    s.setBCValues([DVAL if t == D else 0.0 for pair in types for t in pair])
    for (d, side), pl in planes.items():
        s.setNeumFaceValues(d, side, pl)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        jg = [np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(ndim)] + [None] * (3 - ndim)
        s.setMetricOrtho(q, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return s


def _fields(so, grids, dom, ndim=3):
    return so.random_field(grids, 7, G3 if ndim == 3 else G2, dom.box), so.random_field(grids, 8, (0, 0, 0), dom.box)


def _pieces(s, grids, phi, rhs, homogeneous):
    """GPU residual_bc / apply_op_bc on the resident phi / rhs -> residual, L(phi), phi with its ghosts afterwards"""
    from somar_amd import api as F
    upload(s, F.F_PHI, phi)
    upload(s, F.F_RHS, rhs)
    s.residualBC(F.F_RES, F.F_PHI, F.F_RHS, homogeneous)
    r = download_valid(s, F.F_RES, grids)
    s.applyOpBC(F.F_RES, F.F_PHI, homogeneous)
    a = download_valid(s, F.F_RES, grids)
    ghosted = [None] * len(grids)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        ghosted[gi] = s.download(F.F_PHI, q, phi.ghost)
    return r, a, ghosted


def _host_arrays(s, grids, rhs, ndim=3):
    gb, gx = [], []
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        gb.append(np.asfortranarray(rhs[gi].a[..., 0]))
        gx.append(np.zeros(tuple(n + 2 for n in grids[gi].size()[:ndim]) + (1,) * (3 - ndim), order="F"))
    return gx, gb


def _solve_gpu(s, grids, rhs, ndim=3):
    """inhomogeneous solve from zero through _host; -> stats, valid phi per local patch"""
    gx, gb = _host_arrays(s, grids, rhs, ndim)
    st = s.solve(gx, gb, 0, 0, True, False, phi_ghost=G3 if ndim == 3 else G2)
    return dict(st), [a[1:-1, 1:-1, 1:-1] if ndim == 3 else a[1:-1, 1:-1, :] for a in gx]


def _same_solve(a, b):
    (sa_, xa), (sb_, xb) = a, b
    assert (sa_["iters"], sa_["exitStatus"]) == (sb_["iters"], sb_["exitStatus"])
    np.testing.assert_array_equal(sa_["history"], sb_["history"])
    for x, y in zip(xa, xb):
        np.testing.assert_array_equal(x, y)


@pytest.fixture
def kernel_path(request, monkeypatch):
    if request.param == "march":   # the k-marching operator instead of the direct-load one
        monkeypatch.setenv("SOMAR_MARCH_MIN_CELLS", "0")
    return request.param


# ---- 1. the operator, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,kernel_path", [("3d", "direct"), ("3d", "march"), ("2d", "direct"), ("uniform", "direct"),
                                               ("uniform", "march")], indirect=["kernel_path"])
def test_operator_is_the_wrapped_oracle_bit_for_bit(oracle, monkeypatch, which, kernel_path):
    so = oracle
    patch(monkeypatch, so)
    prob = _problem(so, which)
    dom, grids, dx, ndim, sides = prob[0], prob[1], prob[2], prob[8], prob[9]
    planes = _planes(dom, dx, sides)
    amr = _oracle(so, prob, planes)
    gpu, plain = _gpu(prob, planes), _gpu(prob, {})
    try:
        if which == "uniform":
            assert gpu.metricUniform(0) is not None   # the ghost op takes its coefficient from StencilParams::uc
        phi, rhs = _fields(so, grids, dom, ndim)
        r, a, ghosted = _pieces(gpu, grids, phi, rhs, False)
        res, lhs = so.LevelData(grids, 1), so.LevelData(grids, 1)
        amr.op.residual(res, phi, rhs, False)
        amr.op.apply_op(lhs, phi, False)   # (leaves the ghosts of bc_set_ghosts in phi)
        for x, y in zip(r, valid_of(res)):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a, valid_of(lhs)):
            np.testing.assert_array_equal(x, y)
        nlayers = 0
        for gi, g in enumerate(grids):   # the ghost layers EllipticNeumBCGhostClass wrote
            for d, s in sides:
                if (g.lo[d] if s == 0 else g.hi[d]) != (dom.box.lo[d] if s == 0 else dom.box.hi[d]):
                    continue
                want = phi[gi].view(g.adjCell(d, s, 1))[..., 0]
                sl = [slice(1, -1) if q < ndim else slice(None) for q in range(3)]
                sl[d] = slice(-1, None) if s else slice(0, 1)
                np.testing.assert_array_equal(ghosted[gi][tuple(sl)], want)
                nlayers += 1
        assert nlayers >= len(sides)
        # the values moved the result, and only the homogeneous switch takes them out again
        r0, a0, _ = _pieces(plain, grids, phi, rhs, False)
        assert any(np.any(x != y) for x, y in zip(a, a0))
        rh, ah, _ = _pieces(gpu, grids, phi, rhs, True)
        rp, ap, _ = _pieces(plain, grids, phi, rhs, True)
        for x, y in zip(rh + ah, rp + ap):
            np.testing.assert_array_equal(x, y)
    finally:
        gpu.undefine()
        plain.undefine()


# ---- 2. full solves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["helmholtz", "allneum"])
def test_solve_matches_the_wrapped_oracle_resident_host_and_dev(oracle, monkeypatch, which):
    import torch
    from somar_amd import api as F
    so = oracle
    patch(monkeypatch, so)
    prob = _problem(so, which)
    dom, grids, dx, sides = prob[0], prob[1], prob[2], prob[9]
    planes = _planes(dom, dx, sides)
    amr = _oracle(so, prob, planes)
    gpu = _gpu(prob, planes)
    try:
        if which == "allneum":
            # all-Neumann Poisson: the right-hand side is the oracle's own inhomogeneous L(phi*), compatible by construction
            star = so.random_field(grids, 21, G3, dom.box)
            rhs = so.LevelData(grids, 1)
            amr.op.apply_op(rhs, star, False)
        else:
            rhs = so.random_field(grids, 8, (0, 0, 0), dom.box)
        x = so.LevelData(grids, 1, G3)
        amr.solve(x, rhs, zeroPhi=True, forceHomogeneous=False)
        upload(gpu, F.F_RHS, rhs)
        st = dict(gpu.solveResident(True, False))
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-13 * amr.history[0])
        resident = (st, download_valid(gpu, F.F_PHI, grids))
        if which == "allneum":   # phi is defined up to a constant there: compare with the means taken out
            w = [1.0 / j.view(g)[..., 0] for g, j in zip(grids, prob[4].fabs)]
            mean = lambda f: sum(float(np.sum(a * b)) for a, b in zip(f, w)) / sum(float(np.sum(b)) for b in w)
            got, want = resident[1], valid_of(x)
            mg, mw = mean(got), mean(want)
            assert max_rel_diff([a - mg for a in got], [a - mw for a in want]) < 1e-8
        else:
            assert max_rel_diff(resident[1], valid_of(x)) < 1e-8
        _same_solve(_solve_gpu(gpu, grids, rhs), resident)
        gx, gb = _host_arrays(gpu, grids, rhs)
        dphi = [torch.from_numpy(np.ravel(a, order="F").copy()).cuda() for a in gx]
        drhs = [torch.from_numpy(np.ravel(a, order="F").copy()).cuda() for a in gb]
        st_d = dict(gpu.solveDev(dphi, drhs, True, False))
        xd = [t.cpu().numpy().reshape(a.shape, order="F")[1:-1, 1:-1, 1:-1] for t, a in zip(dphi, gx)]
        _same_solve((st_d, xd), resident)
    finally:
        gpu.undefine()


# ---- 3. new values after finalize ---------------------------------------------------------------------------------------
def test_refresh_after_finalize_and_back_to_zero_neumann(oracle):
    from somar_amd import api as F
    so = oracle
    prob = _problem(so, "helmholtz")
    dom, grids, dx, sides = prob[0], prob[1], prob[2], prob[9]
    pa = _planes(dom, dx, sides)
    pb = {k: np.asfortranarray(-0.5 * v + 0.125) for k, v in pa.items()}
    s, fresh, plain = _gpu(prob, pa), _gpu(prob, pb), _gpu(prob, {})
    try:
        _, rhs = _fields(so, grids, dom)
        first = _solve_gpu(s, grids, rhs)
        live = F.device_bytes_live()
        for (d, side), pl in pb.items():
            s.setNeumFaceValues(d, side, pl)
        assert F.device_bytes_live() == live   # only copies: no buffer was made or resized
        second = _solve_gpu(s, grids, rhs)
        assert second[0]["history"] != first[0]["history"]
        _same_solve(second, _solve_gpu(fresh, grids, rhs))
        for d, side in pb:
            s.setNeumFaceValues(d, side, None)
        assert F.device_bytes_live() == live
        _same_solve(_solve_gpu(s, grids, rhs), _solve_gpu(plain, grids, rhs))
        # a plane set for the first time after finalize
        for (d, side), pl in pb.items():
            plain.setNeumFaceValues(d, side, pl)
        _same_solve(_solve_gpu(plain, grids, rhs), second)
    finally:
        for q in (s, fresh, plain):
            q.undefine()


@pytest.mark.parametrize("min_cells", [0, 1 << 40])   # every depth batched / none
def test_components_under_the_solvers_own_sides_take_the_planes(oracle, monkeypatch, min_cells):
    """the planes belong to the solver's own sides: solveMulti leaves each component as a single-field solve would"""
    from somar_amd import api as F
    so = oracle
    monkeypatch.setenv("SOMAR_MARCH_MIN_CELLS", "0")   # the batched kernels are the marching ones
    monkeypatch.setenv("SOMAR_FUSED_MIN_CELLS", "0")
    prob = _problem(so, "allneum-helmholtz")
    dom, grids, dx, sides = prob[0], prob[1], prob[2], prob[9]
    s = _gpu(prob, _planes(dom, dx, sides))
    try:
        rhs = [so.random_field(grids, 8 + c, (0, 0, 0), dom.box) for c in range(2)]
        seq = []
        for c in range(2):
            upload(s, F.F_RHS, rhs[c])
            st = dict(s.solveResident(True, False))
            seq.append((st, download_valid(s, F.F_PHI, grids)))
        s.setComponents(2, min_cells)
        for c in range(2):
            for q in range(s.num_local_patches):
                _, _, gi = s.patch_box(q)
                s.uploadComp(c, F.F_RHS, q, np.asfortranarray(rhs[c][gi].a[..., 0]), (0, 0, 0))
        stats = s.solveMulti(zeroPhi=True, forceHomogeneous=False)
        for c in range(2):
            assert (stats[c]["iters"], stats[c]["exitStatus"]) == (seq[c][0]["iters"], seq[c][0]["exitStatus"])
            assert s.compHistory(c) == seq[c][0]["history"]
            for q in range(s.num_local_patches):
                _, _, gi = s.patch_box(q)
                np.testing.assert_array_equal(s.downloadComp(c, F.F_PHI, q, (0, 0, 0)), seq[c][1][gi])
    finally:
        s.undefine()


# ---- 4. AMR -------------------------------------------------------------------------------------------------------------
AMR_RATIOS = [(2, 2, 1)]


def _amr(so, sa, alpha=0.0, beta=1.0, cbox=8):
    """two levels, ratio (2,2,1), base 16^3, one 16 x 16 x 16 fine box that touches the face-valued low x side and (as the
    ratio in z is 1) the face-valued top; each level has its own planes at its own resolution"""
    from somar_amd import AMRPressureSolver
    fine = [[so.Box((0, 8, 0), (15, 23, 15))]]
    levels = make_amr_levels(so, sa, (16, 16, 16), (2.0, 1.0, 0.5), (False, False, False), AMR_RATIOS, fine, cbox=cbox)
    planes =[_planes(L.domain, L.dx, SIDES) for L in levels]
    bc = _bc(so, TYPES, {})
    for d, s in SIDES:
        bc.values[d][s] = {tuple(L.domain.box.size()): pl[(d, s)] for L, pl in zip(levels, planes)}
    comp = sa.AMRComposite(levels, AMR_RATIOS, bc, so.BiCGStab(), alpha=alpha, beta=beta)
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    L0 = levels[0]
    s.defineAMR(L0.domain.box.lo, L0.domain.box.hi, L0.domain.periodic, L0.dx, AMR_RATIOS,
                [[(g.lo, g.hi) for g in L.grids] for L in levels], alpha=alpha, beta=beta,
                bc_type=[t for pair in TYPES for t in pair])
    for L, v, pl in zip(levels, s.levels, planes):
        v.setBCValues([DVAL if t == D else 0.0 for pair in TYPES for t in pair])
        for (d, side), p_ in pl.items():
            v.setNeumFaceValues(d, side, p_)
        for q in range(v.num_local_patches):
            _, _, gi = v.patch_box(q)
            jg = [np.asfortranarray(L.Jgup[gi][d].a[..., d]) for d in range(3)]
            v.setMetricOrtho(q, jg[0], jg[1], jg[2], np.asfortranarray(L.Jinv[gi].a[..., 0]))
    s.finalize()
    return levels, planes, comp, s


def test_amr_composite_solve_and_level_residuals(monkeypatch):
    from oracle import somar_amr as sa
    from oracle import somar_oracle as so
    from somar_amd import api as F
    patch(monkeypatch, so)
    levels, planes, comp, s = _amr(so, sa)
    try:
        rhs = [so.random_field(L.grids, 50 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
        comp.zero_covered(0, rhs[0])
        sol = [so.LevelData(L.grids, 1, G3) for L in levels]
        comp.solve(sol, rhs, 1, 0, forceHomogeneous=False)
        for l, v in enumerate(s.levels):
            upload(v, F.F_RHS, rhs[l])
        st = s.solveAMR(1, 0, zeroPhi=True, forceHomogeneous=False)
        assert st["iters"] == comp.iters and st["exitStatus"] == comp.exitStatus
        np.testing.assert_allclose(st["history"], comp.history, rtol=1e-10, atol=0.0)
        for l in (0, 1):
            assert max_rel_diff(download_valid(s.levels[l], F.F_PHI, levels[l].grids), valid_of(sol[l])) < 1e-8
        # somar_amr_residual_level takes the physical boundary values as zero (as it does Dirichlet ones): with planes set
        # it is the oracle's homogeneous composite residual, bit for bit
        phis = [so.random_field(L.grids, 5 + l, G3, L.domain.box) for l, L in enumerate(levels)]
        ress = [so.LevelData(L.grids, 1) for L in levels]
        comp.init(phis, rhs, 1, 0)
        for l, v in enumerate(s.levels):
            upload(v, F.F_PHI, phis[l])
        comp.compute_amr_residual(ress, phis, rhs, 1, 0, True)
        for ilev in (0, 1):
            s.residualLevel(1, 0, ilev)
            if ilev == 0:
                s.zeroCovered(0, F.F_RES)
            for g, w in zip(download_valid(s.levels[ilev], F.F_RES, levels[ilev].grids), valid_of(ress[ilev])):
                np.testing.assert_array_equal(g, w)
    finally:
        s.undefine()


# ---- 5. heat ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_heat_step_on_a_level(oracle, monkeypatch, scheme):
    """tolerances: tests/test_gpu_heat.py's for the same schemes"""
    from somar_amd import api as F
    so = oracle
    patch(monkeypatch, so)
    dom, grids, dx, Jgup, Jinv = make_problem(so, (16, 16, 16), 8, "stretched", (False, False, False), (2.0, 1.0, 0.5))
    prob = (dom, grids, dx, Jgup, Jinv, TYPES, 1.0, 5e-2, 3, SIDES)
    planes = _planes(dom, dx, SIDES)
    amr = _oracle(so, prob, planes)
    gpu = _gpu(prob, planes)
    try:
        dt = 0.2
        old = so.random_field(grids, 3, G3, dom.box)
        src = so.random_field(grids, 4, (0, 0, 0), dom.box)
        upload(gpu, F.F_HEAT_OLD, old)
        upload(gpu, F.F_HEAT_SRC, src)
        new = so.LevelData(grids, 1, G3)
        [so.level_backward_euler, so.level_crank_nicolson, so.level_tga][scheme](amr, new, old, src, dt)
        st = gpu.heatStep(scheme, dt)
        assert st["iters"] == amr.iters and st["exitStatus"] == amr.exitStatus
        np.testing.assert_allclose(st["history"], amr.history, rtol=1e-10, atol=1e-13 * amr.history[0])
        assert max_rel_diff(download_valid(gpu, F.F_PHI, grids), valid_of(new)) < 1e-9
    finally:
        gpu.undefine()


def test_amr_heat_flux_boundary_faces_are_the_planes(monkeypatch):
    """somar_amr_heat_step accumulates the flux somar_heat_flux_download returns: on a face-valued Neumann side its boundary
    faces are the plane's values themselves (EllipticNeumBCFluxClass)"""
    from oracle import somar_amr as sa
    from oracle import somar_oracle as so
    from somar_amd import api as F
    patch(monkeypatch, so)
    levels, planes, comp, s = _amr(so, sa, alpha=1.0, beta=0.05)
    try:
        l, dt = 1, 0.2
        g1, g0 = levels[1].grids, levels[0].grids
        old = so.random_field(g1, 3, G3, levels[1].domain.box)
        src = so.random_field(g1, 4, (0, 0, 0), levels[1].domain.box)
        cold = so.random_field(g0, 5, G3, levels[0].domain.box)
        cnew = so.random_field(g0, 6, G3, levels[0].domain.box)
        new = so.LevelData(g1, 1, G3)
        times = dict(oldTime=0.25, crseOldTime=0.0, crseNewTime=1.0)
        sa.amr_level_heat(comp, l, 0, new, old, src, cold, cnew, dt=dt, zeroPhi=True, **times)
        upload(s.levels[1], F.F_HEAT_OLD, old)
        upload(s.levels[1], F.F_HEAT_SRC, src)
        upload(s.levels[0], F.F_HEAT_OLD, cold)
        upload(s.levels[0], F.F_PHI, cnew)
        st = s.heatStepAMR(l, 0, dt, True, **times)
        assert st["iters"] == comp.iters and st["exitStatus"] == comp.exitStatus
        np.testing.assert_allclose(st["history"], comp.history, rtol=1e-10, atol=1e-13 * comp.history[0])
        assert max_rel_diff(download_valid(s.levels[1], F.F_PHI, g1), valid_of(new)) < 1e-9
        v, dom = s.levels[1], levels[1].domain.box
        nfaces = 0
        for q in range(v.num_local_patches):
            lo, hi, _ = v.patch_box(q)
            for d, side in SIDES:
                if (lo[d] if side == 0 else hi[d]) != (dom.lo[d] if side == 0 else dom.hi[d]):
                    continue
                t0, t1 = transverse(d)
                want = planes[1][(d, side)][lo[t0] - dom.lo[t0]:hi[t0] - dom.lo[t0] + 1, lo[t1] - dom.lo[t1]:hi[t1] - dom.lo[t1] + 1]
                got = np.take(v.heatFlux(d, q), -1 if side else 0, axis=d)
                np.testing.assert_array_equal(got, want)
                nfaces += 1
        assert nfaces == len(SIDES)
    finally:
        s.undefine()


def test_composite_tga_step(monkeypatch):
    """tolerances: tests/test_gpu_amr_tga.py's"""
    from oracle import somar_amr as sa
    from oracle import somar_oracle as so
    from somar_amd import api as F
    patch(monkeypatch, so)
    levels, planes, comp, s = _amr(so, sa, alpha=1.0, beta=0.05)
    try:
        dt = 0.2
        old = [so.random_field(L.grids, 3 + l, G3, L.domain.box) for l, L in enumerate(levels)]
        src = [so.random_field(L.grids, 13 + l, G3, L.domain.box) for l, L in enumerate(levels)]
        new = [so.random_field(L.grids, 23 + l, G3, L.domain.box) for l, L in enumerate(levels)]
        for l in range(2):
            upload(s.levels[l], F.F_HEAT_OLD, old[l])
            upload(s.levels[l], F.F_HEAT_SRC, src[l])
            upload(s.levels[l], F.F_PHI, new[l])
        sa.amr_tga_one_step(comp, new, old, src, dt, 0, 1)
        st = s.tgaStepAMR(1, 0, dt)
        assert st["iters"] == comp.iters and st["exitStatus"] == comp.exitStatus
        np.testing.assert_allclose(st["history"], comp.history, rtol=1e-10, atol=1e-13 * comp.history[0])
        got0 = so.LevelData(levels[0].grids, 1, G3)
        for g, fab, a in zip(levels[0].grids, got0.fabs, download_valid(s.levels[0], F.F_PHI, levels[0].grids)):
            fab.view(g)[..., 0] = a
        want0 = so.ld_create(new[0])
        so.ld_assign(want0, new[0])
        comp.zero_covered(0, got0)   # a composite solve leaves nothing meaningful under the fine level
        comp.zero_covered(0, want0)
        got = valid_of(got0) + download_valid(s.levels[1], F.F_PHI, levels[1].grids)
        assert max_rel_diff(got, valid_of(want0) + valid_of(new[1])) < 1e-9
    finally:
        s.undefine()


# ---- 6. two ranks on one GPU --------------------------------------------------------------------------------------------
def _worker(rank, nranks, name, q):
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, here)
        sys.path.insert(0, os.path.dirname(here))
        from oracle import somar_oracle as so
        from somar_amd import api as F
        comm = F.comm_create_shm(name, rank, nranks)
        prob = _problem(so, "helmholtz")
        dom, grids, dx, sides = prob[0], prob[1], prob[2], prob[9]
        planes = _planes(dom, dx, sides)
        _, rhs = _fields(so, grids, dom)
        one = _gpu(prob, planes)
        st1, _ = _solve_gpu(one, grids, rhs)
        one.undefine()
        gpu = _gpu(prob, planes, owner=[i % nranks for i in range(len(grids))], comm=comm)
        assert gpu.num_local_patches == 1   # the two-box level, one box per rank: each keeps its own slices of the planes
        st, _ = _solve_gpu(gpu, grids, rhs)
        assert (st["iters"], st["exitStatus"]) == (st1["iters"], st1["exitStatus"])
        np.testing.assert_allclose(st["history"], st1["history"], rtol=1e-10, atol=1e-13 * st1["history"][0])
        gpu.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_two_ranks_match_the_one_rank_run():
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


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def _refused(s, d, side, values, match):
    from somar_amd import api as F
    ptr = None if values is None else F._dp(values)
    assert F.lib().somar_solver_set_neum_face_values(s._h, d, side, ptr) != 0
    assert match.encode() in F.lib().somar_last_error(), F.lib().somar_last_error()


def test_refused_sides_leave_the_solver_as_it_was(oracle):
    so = oracle
    prob = _problem(so, "periodic")   # x (N, N), y periodic, z (N, D)
    dom, grids, dx = prob[0], prob[1], prob[2]
    planes = _planes(dom, dx, prob[9])
    s, fresh = _gpu(prob, planes), _gpu(prob, planes)
    try:
        pl = np.ones((32, 16), order="F")
        _refused(s, 2, 1, pl, "not a Neumann side")
        _refused(s, 1, 0, np.ones((32, 16), order="F"), "periodic")
        for d, side in ((3, 0), (-1, 0), (0, 2), (0, -1)):
            _refused(s, d, side, None, "dir must be")
        _, rhs = _fields(so, grids, dom)
        _same_solve(_solve_gpu(s, grids, rhs), _solve_gpu(fresh, grids, rhs))
    finally:
        s.undefine()
        fresh.undefine()
    prob = _problem(so, "2d")
    dom, grids, dx = prob[0], prob[1], prob[2]
    planes = _planes(dom, dx, prob[9])
    s, fresh = _gpu(prob, planes), _gpu(prob, planes)
    try:
        _refused(s, 2, 0, np.ones((32, 16), order="F"), "inactive")
        _, rhs = _fields(so, grids, dom, 2)
        _same_solve(_solve_gpu(s, grids, rhs, 2), _solve_gpu(fresh, grids, rhs, 2))
    finally:
        s.undefine()
        fresh.undefine()


def _sheared(so, neum_plane_first=False, full=True):
    """16 x 16 x 8, all sides Neumann but the top; -> solver, grids, dom (test_gpu_dirichlet_face.py's sheared metric)"""
    from somar_amd import AMRPressureSolver, SomarError
    n, L = (16, 16, 8), (2.0, 1.0, 0.5)
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), (False, False, False))
    grids = so.split_domain(dom.box, 8)
    dx = tuple(L[d] / n[d] for d in range(3))
    Jgup, Jinv = so.make_full_metric(grids, dx, L, dom)
    Jd, Jdi = so.make_diagonal_metric(grids, dx, L, 3, "stretched", domain=dom)
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=1.0, beta=-0.02,
             bc_type=[N, N, N, N, N, D])
    s.setBCValues([0, 0, 0, 0, 0, DVAL])
    plane = step_plane(dom.box, dx, 0, 0)
    if neum_plane_first:
        s.setNeumFaceValues(0, 0, plane)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        full_args = [np.asfortranarray(Jgup[gi][d].a) for d in range(3)] + [np.asfortranarray(Jinv[gi].a[..., 0])]
        if neum_plane_first:   # refused: the solver keeps its diagonal metric and its plane
            with pytest.raises(SomarError, match="diagonal metric only"):
                s.setMetricFull(q, *full_args)
        if full and not neum_plane_first:
            s.setMetricFull(q, *full_args)
        else:
            jg = [np.asfortranarray(Jd[gi][d].a[..., d]) for d in range(3)]
            s.setMetricOrtho(q, jg[0], jg[1], jg[2], np.asfortranarray(Jdi[gi].a[..., 0]))
    s.finalize()
    return s, grids, dom, plane


def test_a_nondiagonal_metric_and_face_valued_neumann_sides_refuse_each_other(oracle):
    so = oracle
    # a full-metric handle refuses the plane ...
    s, grids, dom, plane = _sheared(so)
    fresh = _sheared(so)[0]
    try:
        _refused(s, 0, 0, plane, "non-diagonal metric")
        _, rhs = _fields(so, grids, dom)
        _same_solve(_solve_gpu(s, grids, rhs), _solve_gpu(fresh, grids, rhs))
    finally:
        s.undefine()
        fresh.undefine()
    # ... and a handle with a plane refuses the full metric, staying the diagonal solver with that plane
    s, grids, dom, plane = _sheared(so, neum_plane_first=True)
    fresh = _sheared(so, full=False)[0]
    try:
        fresh.setNeumFaceValues(0, 0, plane)
        _, rhs = _fields(so, grids, dom)
        _same_solve(_solve_gpu(s, grids, rhs), _solve_gpu(fresh, grids, rhs))
    finally:
        s.undefine()
        fresh.undefine()


def test_leptic_solvers_refuse_a_level_with_a_plane(oracle, monkeypatch):
    from oracle import somar_amr as sa
    from somar_amd import LevelLepticSolver, SomarError
    from somar_amd import api as F
    so = oracle
    patch(monkeypatch, so)   # (_amr builds the oracle's composite too, whose probes meet the planes)
    n, dx = (16, 16, 8), (1.0 / 16, 1.0 / 16, 0.005 / 8)
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), (False, False, False))
    grids = so.split_domain(dom.box, (16, 16, 8))
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, (1.0, 1.0, 0.005), 3, "stretched", domain=dom)
    bottom = np.ones((n[0], n[1]), order="F")
    rhs = so.random_field(grids, 8, (0, 0, 0), dom.box)

    def make(plane_before):
        lep = LevelLepticSolver()
        lep.params.max_order = 2
        lep.params.domain_height = 0.005
        lep.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], bc_type=[N, N, N, N, N, D])
        lv = lep.level
        if plane_before:
            lv.setNeumFaceValues(2, 0, bottom)
        for p_ in range(lv.num_local_patches):
            _, _, gi = lv.patch_box(p_)
            jg = [np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)]
            lv.setMetricOrtho(p_, jg[0], jg[1], jg[2], np.asfortranarray(Jinv[gi].a[..., 0]))
        lep.finalize()
        return lep

    def run(lep):
        lep.level.setVal(F.F_PHI, 0.0)
        upload(lep.level, F.F_RHS, rhs)
        st = lep.solve()
        return st["resNorms"], download_valid(lep.level, F.F_PHI, grids)

    fresh = make(False)
    try:
        want = run(fresh)
    finally:
        fresh.undefine()
    for before in (True, False):
        lep = make(before)
        try:
            if not before:
                lep.level.setNeumFaceValues(2, 0, bottom)
            with pytest.raises(SomarError, match="leptic path does not read them"):
                lep.solve()
            lep.level.setNeumFaceValues(2, 0, None)   # without the plane it is the solver it was
            got = run(lep)
            assert got[0] == want[0]
            for a, b in zip(got[1], want[1]):
                np.testing.assert_array_equal(a, b)
        finally:
            lep.undefine()
    # the AMR leptic solve (base boxes spanning the vertical, as the leptic solver wants its columns)
    levels, planes, comp, s = _amr(so, sa, cbox=(8, 8, 16))
    try:
        s.enableLeptic()
        with pytest.raises(SomarError, match="leptic path does not read them"):
            s.solveAMRLeptic(1, 0)
    finally:
        s.undefine()
