"""The oracle with position-dependent Dirichlet values (tests/diri_face.py patches somar_oracle.set_side_diri_bc), checked
on its own before the GPU is compared with it: a constant plane reproduces the constant path bit for bit, and on a
stretched diagonal metric the values move the residual only on the boundary layer, by the amount the 7-point operator
L = beta Jinv sum_a (F_{i+e_a} - F_i) / dx_a with ghost = (-first valid) + 2 g predicts."""
import numpy as np

from diri_face import patch, step_plane
from helpers import make_problem, valid_of

D, N = 1, 0


def _op(so, types, values, alpha=0.0, beta=1.0):
    dom, grids, dx, Jgup, Jinv = make_problem(so, (16, 16, 8), 8, "stretched", (False, False, False), (1.0, 1.0, 0.5))
    bc = so.BCHolder([list(t) for t in types], [list(v) for v in values])
    fac = so.Factory(dom, grids, dx, bc, Jgup, Jinv, alpha=alpha, beta=beta)
    return dom, grids, dx, Jgup, Jinv, bc, so.AMRMultiGrid(fac, so.BiCGStab())


def test_constant_plane_reproduces_the_constant_path(oracle, monkeypatch):
    so = oracle
    patch(monkeypatch, so)
    types = [(D, D), (N, N), (N, D)]
    vals = [(0.7, -0.4), (0.0, 0.0), (0.0, 1.3)]
    dom, grids, dx, _, _, bc, amr = _op(so, types, vals, alpha=1.0, beta=-0.05)
    _, _, _, _, _, bcp, amrp = _op(so, types, vals, alpha=1.0, beta=-0.05)
    for d, s in ((0, 0), (0, 1), (2, 1)):
        shape = [dom.box.size()[q] for q in range(3) if q != d]
        bcp.values[d][s] = np.full(shape, vals[d][s], order="F")
    phi = so.random_field(grids, 5, (1, 1, 1), dom.box)
    rhs = so.random_field(grids, 6, (0, 0, 0), dom.box)
    for homog in (False, True):
        a, b = so.LevelData(grids, 1), so.LevelData(grids, 1)
        amr.op.residual(a, phi, rhs, homog)
        amrp.op.residual(b, phi, rhs, homog)
        for x, y in zip(valid_of(a), valid_of(b)):
            np.testing.assert_array_equal(x, y)
        amr.op.apply_op(a, phi, homog)
        amrp.op.apply_op(b, phi, homog)
        for x, y in zip(valid_of(a), valid_of(b)):
            np.testing.assert_array_equal(x, y)


def test_values_enter_the_boundary_layer_as_the_stencil_predicts(oracle, monkeypatch):
    so = oracle
    patch(monkeypatch, so)
    beta = 0.7
    types = [(N, N), (N, N), (N, D)]
    dom, grids, dx, Jgup, Jinv, bc, amr = _op(so, types, [(0.0, 0.0)] * 3, alpha=0.0, beta=beta)
    plane = step_plane(dom.box, dx, 2, 1)
    assert np.ptp(plane) > 1.0
    phi = so.random_field(grids, 5, (1, 1, 1), dom.box)
    rhs = so.random_field(grids, 6, (0, 0, 0), dom.box)
    r0, r1 = so.LevelData(grids, 1), so.LevelData(grids, 1)
    bc.values[2][1] = np.zeros_like(plane)
    amr.op.residual(r0, phi, rhs, False)
    bc.values[2][1] = plane
    amr.op.residual(r1, phi, rhs, False)
    top = dom.box.hi[2]
    nlayer = 0
    for gi, g in enumerate(grids):
        diff = r1[gi].view(g)[..., 0] - r0[gi].view(g)[..., 0]
        if g.hi[2] != top:
            np.testing.assert_array_equal(diff, 0.0)
            continue
        face = so.Box((g.lo[0], g.lo[1], top + 1), (g.hi[0], g.hi[1], top + 1))
        cells = so.Box((g.lo[0], g.lo[1], top), (g.hi[0], g.hi[1], top))
        jg = Jgup[gi][2].view(face)[..., 0, 2]
        jinv = Jinv[gi].view(cells)[..., 0, 0]
        gv = plane[g.lo[0]:g.hi[0] + 1, g.lo[1]:g.hi[1] + 1]
        want = -beta * jinv * jg * 2.0 * gv / dx[2] ** 2
        np.testing.assert_allclose(diff[..., -1], want, rtol=1e-13, atol=0.0)
        np.testing.assert_array_equal(diff[..., :-1], 0.0)
        nlayer += 1
    assert nlayer > 0
