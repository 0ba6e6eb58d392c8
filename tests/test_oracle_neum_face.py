"""The oracle with position-dependent Neumann values (tests/neum_face.py wraps somar_oracle.bc_set_ghosts and
bc_set_fluxes), anchored without the oracle's own arithmetic before the GPU is compared with it:
 1. on a Cartesian metric a linear field with the planes J g^{dd} dphi/dxi_d on all six sides is annihilated by the
    inhomogeneous operator at every cell, boundary cells included -- and is not with the planes negated (the sign on
    both sides);
 2. on a stretched diagonal metric the ghost the wrap writes, differenced back, is the plane;
 3. a plane of zeros is the unwrapped oracle, bit for bit."""
import numpy as np

from helpers import make_problem, valid_of
from neum_face import patch, step_plane, transverse

D, N = 1, 0


def _op(so, variant, types, n=(16, 12, 8), L=(1.0, 1.5, 0.5), alpha=0.0, beta=1.0):
    dom, grids, dx, Jgup, Jinv = make_problem(so, n, (8, 6, 4), variant, (False, False, False), L)
    bc = so.BCHolder([list(t) for t in types], [[0.0, 0.0] for _ in range(3)])
    fac = so.Factory(dom, grids, dx, bc, Jgup, Jinv, alpha=alpha, beta=beta)
    return dom, grids, dx, Jgup, Jinv, bc, so.AMRMultiGrid(fac, so.BiCGStab())


def test_linear_field_on_a_cartesian_metric_pins_the_sign_on_both_sides(oracle, monkeypatch):
    so = oracle
    patch(monkeypatch, so)
    dom, grids, dx, Jgup, Jinv, bc, amr = _op(so, "cartesian", [(N, N)] * 3)
    for gi in range(len(grids)):   # the anchor below is written for an all-ones metric: say so
        for d in range(3):
            np.testing.assert_array_equal(Jgup[gi][d].a[..., d], 1.0)
        np.testing.assert_array_equal(Jinv[gi].a, 1.0)
    coef = (0.75, -1.25, 2.0)
    phi = so.LevelData(grids, 1, (1, 1, 1))
    for f in phi.fabs:
        I = np.meshgrid(*[np.arange(f.box.lo[a], f.box.hi[a] + 1) for a in range(3)], indexing="ij")
        f.a[..., 0] = sum(coef[a] * (I[a] + 0.5) * dx[a] for a in range(3))
    for f in phi.fabs:   # the physical ghosts are the operator's to fill: spoil what the formula put there
        inside = f.view(f.box & dom.box).copy()
        f.a[...] = 1.0e30
        f.view(f.box & dom.box)[...] = inside
    amax = max(float(np.max(np.abs(v))) for v in valid_of(phi))
    bound = 1e-12 * amax / min(dx) ** 2
    for sign, small in ((1.0, True), (-1.0, False)):
        for d in range(3):
            t0, t1 = transverse(d)
            shape = (dom.box.size()[t0], dom.box.size()[t1])
            for s in (0, 1):
                # J g^{dd} dphi/dxi_d = 1 * coef[d], the same on the low and the high side
                bc.values[d][s] = np.full(shape, sign * coef[d], order="F")
        lhs = so.LevelData(grids, 1)
        amr.op.apply_op(lhs, phi, False)
        worst = max(float(np.max(np.abs(v))) for v in valid_of(lhs))
        if small:
            assert worst <= bound, (worst, bound)
        else:
            assert worst > 1e3 * bound, (worst, bound)


def test_ghost_differenced_back_is_the_plane_on_a_stretched_metric(oracle, monkeypatch):
    so = oracle
    patch(monkeypatch, so)
    dom, grids, dx, Jgup, Jinv, bc, amr = _op(so, "stretched", [(N, N), (D, N), (N, N)])
    sides = [(0, 0), (0, 1), (1, 1), (2, 0), (2, 1)]
    planes = {(d, s): step_plane(dom.box, dx, d, s, amp=0.25 + 0.1 * d, hot=1.0 - s) for d, s in sides}
    for (d, s), pl in planes.items():
        bc.values[d][s] = pl
    phi = so.random_field(grids, 5, (1, 1, 1), dom.box)
    nchecked = 0
    for gi, g in enumerate(grids):
        f = phi[gi]
        so.bc_set_ghosts(bc, f, None, g, dom, dx, Jgup[gi], False, True, 3)
        for (d, s), pl in planes.items():
            if (g.lo[d] if s == 0 else g.hi[d]) != (dom.box.lo[d] if s == 0 else dom.box.hi[d]):
                continue
            ghost = g.adjCell(d, s, 1)
            sh = [0, 0, 0]
            sh[d] = -1 if s else 1
            near = ghost.shift(sh)
            sgn = 1.0 if s else -1.0
            jg = Jgup[gi][d].view(ghost if s else near)[..., d]
            t0, t1 = transverse(d)
            want = np.expand_dims(pl[g.lo[t0]:g.hi[t0] + 1, g.lo[t1]:g.hi[t1] + 1], d)
            gv, nv = f.view(ghost)[..., 0], f.view(near)[..., 0]
            got = jg * (gv - nv) / (sgn * dx[d])
            # ghost = near + t is rounded to half an ulp of |ghost|; the difference ghost - near is then exact or rounded
            # again the same way: in all a few ulp of max(|ghost|, |near|), scaled as t is into the plane's units
            eps = np.finfo(float).eps
            tol = 4 * eps * (np.abs(want) + np.abs(jg) * np.maximum(np.abs(gv), np.abs(nv)) / dx[d])
            assert np.all(np.abs(got - want) <= tol)
            nchecked += 1
    assert nchecked >= len(sides)


def test_plane_of_zeros_is_the_unwrapped_oracle_bit_for_bit(oracle, monkeypatch):
    so = oracle
    types = [(N, N), (D, N), (N, N)]
    dom, grids, dx, Jgup, Jinv, bc, amr = _op(so, "stretched", types, alpha=1.0, beta=-0.05)
    phi = so.random_field(grids, 5, (1, 1, 1), dom.box)
    rhs = so.random_field(grids, 6, (0, 0, 0), dom.box)
    plain = {}
    for homog in (False, True):
        a, b = so.LevelData(grids, 1), so.LevelData(grids, 1)
        amr.op.residual(a, phi, rhs, homog)
        amr.op.apply_op(b, phi, homog)
        plain[homog] = [v.copy() for v in valid_of(a) + valid_of(b)]
    patch(monkeypatch, so)
    for d, s in ((0, 0), (1, 1), (2, 1)):
        t0, t1 = transverse(d)
        bc.values[d][s] = np.zeros((dom.box.size()[t0], dom.box.size()[t1]), order="F")
    for homog in (False, True):
        a, b = so.LevelData(grids, 1), so.LevelData(grids, 1)
        amr.op.residual(a, phi, rhs, homog)
        amr.op.apply_op(b, phi, homog)
        for x, y in zip(valid_of(a) + valid_of(b), plain[homog]):
            np.testing.assert_array_equal(x, y)
