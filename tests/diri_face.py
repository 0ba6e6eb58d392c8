"""Position-dependent Dirichlet values (EllipticDiriBCGhostClass, BCInterface/EllipticBCUtils.cpp:548-646) for the
oracle, without touching oracle/: every Dirichlet ghost of the oracle goes through the module-level
somar_oracle.set_side_diri_bc, so a test replaces that function with one that also takes a numpy face plane as the
side's value (BCHolder.values[d][side]; a hierarchy's levels share one BCHolder, so there the value is a dict from
the size of a level's domain box to that level's plane).  Scalars still go to the original function.

A plane covers the whole domain box's faces of one side, indexed [t0, t1] by the two transverse directions in
increasing order -- the layout of somar_solver_set_bc_face_values."""
import numpy as np


def transverse(d):
    return [q for q in range(3) if q != d]


def face_positions(dom_box, dx, d, side):
    """(pos[t0], pos[t1]) of every boundary face of side (d, side), the reference functor's pos (EllipticBCUtils.cpp:
    595-626): transverse cell centres (fc + 0.5) dx"""
    t0, t1 = transverse(d)
    x0 = (np.arange(dom_box.lo[t0], dom_box.hi[t0] + 1) + 0.5) * dx[t0]
    x1 = (np.arange(dom_box.lo[t1], dom_box.hi[t1] + 1) + 0.5) * dx[t1]
    return np.meshgrid(x0, x1, indexing="ij")


def step_plane(dom_box, dx, d, side, L0=1.0, amp=0.25, hot=1.0, cold=-0.5):
    """a smooth function plus a hot / cold step along the first transverse direction, in the spirit of
    HorizConvBCUtil's topBCValueFunc (BCutil/HorizConvBCUtil.cpp:33-66)"""
    p0, p1 = face_positions(dom_box, dx, d, side)
    step = np.where(p0 < 0.4 * L0, hot, cold)
    return np.asfortranarray(step + amp * np.sin(2.0 * np.pi * p0 / L0 + 0.3) * np.cos(np.pi * p1 + 0.1))


def install(so):
    """replace so.set_side_diri_bc; returns the function that puts the original back"""
    orig = so.set_side_diri_bc

    def set_side_diri_bc(state, valid, domain, value, d, side, homogeneous, order):
        if not isinstance(value, (np.ndarray, dict)):
            return orig(state, valid, domain, value, d, side, homogeneous, order)
        assert order == 1
        if domain.periodic[d]:
            return
        vend = valid.lo[d] if side == 0 else valid.hi[d]
        dend = domain.box.lo[d] if side == 0 else domain.box.hi[d]
        if vend != dend:
            return
        ghost = valid.adjCell(d, side, 1) & state.box
        if ghost.isEmpty():
            return
        sh = [0, 0, 0]
        sh[d] = -1 if side else 1
        gv = state.view(ghost)
        sv = state.view(ghost.shift(sh))
        if homogeneous:
            gv[...] = -sv
            return
        if isinstance(value, dict):   # AMR: one plane per level, keyed by the size of that level's domain box
            value = value[tuple(domain.box.size())]
        t0, t1 = transverse(d)
        lo = domain.box.lo
        g = value[ghost.lo[t0] - lo[t0]:ghost.hi[t0] - lo[t0] + 1, ghost.lo[t1] - lo[t1]:ghost.hi[t1] - lo[t1] + 1]
        g = np.expand_dims(g, d)[..., None]
        # EllipticBCUtils.cpp:611-630: copy, negate, then += 2 g
        gv[...] = (-sv) + 2.0 * g

    so.set_side_diri_bc = set_side_diri_bc

    def restore():
        so.set_side_diri_bc = orig
    return restore


def patch(monkeypatch, so):
    """install() for the length of one test"""
    orig = so.set_side_diri_bc
    install(so)
    patched = so.set_side_diri_bc
    so.set_side_diri_bc = orig
    monkeypatch.setattr(so, "set_side_diri_bc", patched)
