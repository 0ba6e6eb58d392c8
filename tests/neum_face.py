"""Position-dependent Neumann values on a diagonal metric (EllipticNeumBCGhostClass / EllipticNeumBCFluxClass,
BCInterface/EllipticBCUtils.cpp:696-947) for the oracle, without touching oracle/.  set_side_neum_bc is not handed
`homogeneous`, so the extension sits one level up: a test replaces the module-level somar_oracle.bc_set_ghosts and
somar_oracle.bc_set_fluxes (every oracle module calls them through the module).  A Neumann side whose
BCHolder.values[d][side] is a numpy plane -- for hierarchies, whose levels share one BCHolder, a dict from the size of a
level's domain box to that level's plane -- goes to the original as 0.0; then, unless homogeneous, its ghost layer becomes
near + ((sgn dx) g) / Jg^{dd}(boundary face) (:842-843, the cross term being zero on a diagonal metric) and its boundary
faces become g.  Scalars go to the original unchanged.

g = J g^{dd} dphi/dxi_d at the face on BOTH sides (not the outward-normal flux).  A plane has the layout of
somar_solver_set_neum_face_values, which is that of diri_face.py's planes."""
import numpy as np

from diri_face import face_positions, step_plane, transverse   # noqa: F401  (the planes are laid out alike)

BC_NEUM = 0


def _planes_of(bc, ndim):
    return [(d, s) for d in range(ndim) for s in (0, 1)
            if bc.types[d][s] == BC_NEUM and isinstance(bc.values[d][s], (np.ndarray, dict))]


class _Zeroed:
    """the BCHolder as the original functions see it: face-valued Neumann sides carry 0.0"""

    def __init__(self, bc, sides):
        self.types = bc.types
        self.values = [list(v) for v in bc.values]
        for d, s in sides:
            self.values[d][s] = 0.0
        self._bc = bc

    def __getattr__(self, name):
        return getattr(self._bc, name)


def _plane(value, domain, region, d):
    """the plane's values over `region` (one cell or face thick along d), shaped like a view of that region"""
    if isinstance(value, dict):   # AMR: one plane per level, keyed by the size of that level's domain box
        value = value[tuple(domain.box.size())]
    t0, t1 = transverse(d)
    lo = domain.box.lo
    g = value[region.lo[t0] - lo[t0]:region.hi[t0] - lo[t0] + 1, region.lo[t1] - lo[t1]:region.hi[t1] - lo[t1] + 1]
    return np.expand_dims(g, d)[..., None]


def _touches(valid, domain, d, side):
    if domain.periodic[d]:
        return False
    return (valid.lo[d] if side == 0 else valid.hi[d]) == (domain.box.lo[d] if side == 0 else domain.box.hi[d])


def install(so):
    """replace so.bc_set_ghosts and so.bc_set_fluxes; returns the function that puts the originals back"""
    orig_ghosts, orig_fluxes = so.bc_set_ghosts, so.bc_set_fluxes

    def bc_set_ghosts(bc, state, extrap, valid, domain, dx, Jgup, homogeneous, is_diagonal, ndim=3):
        sides = _planes_of(bc, ndim)
        if not sides:
            return orig_ghosts(bc, state, extrap, valid, domain, dx, Jgup, homogeneous, is_diagonal, ndim)
        assert is_diagonal, "face-valued Neumann sides are defined on a diagonal metric only"
        orig_ghosts(_Zeroed(bc, sides), state, extrap, valid, domain, dx, Jgup, homogeneous, is_diagonal, ndim)
        if homogeneous:
            return
        for d, side in sides:
            if not _touches(valid, domain, d, side):
                continue
            ghost = valid.adjCell(d, side, 1) & state.box
            if ghost.isEmpty():
                continue
            sgn = 1.0 if side else -1.0
            sh = [0, 0, 0]
            sh[d] = -1 if side else 1
            near = ghost.shift(sh)
            face = ghost if side else near   # face i is the low face of cell i: the boundary face of either side
            g = _plane(bc.values[d][side], domain, ghost, d)
            jg = Jgup[d].view(face, slice(d, d + 1))
            state.view(ghost)[...] = state.view(near) + ((sgn * dx[d]) * g) / jg

    def bc_set_fluxes(bc, flux, valid, domain, homogeneous, ndim=3):
        sides = _planes_of(bc, ndim)
        if not sides:
            return orig_fluxes(bc, flux, valid, domain, homogeneous, ndim)
        orig_fluxes(_Zeroed(bc, sides), flux, valid, domain, homogeneous, ndim)
        if homogeneous:
            return
        for d, side in sides:
            if not _touches(valid, domain, d, side):
                continue
            fb = valid.faces(d)
            lo, hi = list(fb.lo), list(fb.hi)
            if side == 0:
                hi[d] = lo[d]
            else:
                lo[d] = hi[d]
            region = so.Box(lo, hi)
            flux[d].view(region)[...] = _plane(bc.values[d][side], domain, region, d)

    so.bc_set_ghosts, so.bc_set_fluxes = bc_set_ghosts, bc_set_fluxes

    def restore():
        so.bc_set_ghosts, so.bc_set_fluxes = orig_ghosts, orig_fluxes
    return restore


def patch(monkeypatch, so):
    """install() for the length of one test"""
    restore = install(so)
    patched = so.bc_set_ghosts, so.bc_set_fluxes
    restore()
    monkeypatch.setattr(so, "bc_set_ghosts", patched[0])
    monkeypatch.setattr(so, "bc_set_fluxes", patched[1])
