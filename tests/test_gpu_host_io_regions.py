"""The host side of the caller-array boundary, region by region: what a host call moves, what it leaves alone, and the
rules it shares with the device-pointer calls.  test_gpu_device_io.py shows that host and device transfers agree; these
tests pin the host regions themselves, so that the two cannot drift together.

Layouts are test_gpu_device_io.py's: "unequal" (44 x 24 x 10 in six boxes of i-width 12 / 20 / 12), "flat2d" (the same, one
cell thick, space_dim 2) and "deep" (48 x 16 x 8, the one with a multigrid depth 1).  A copy has no tolerance, and the
arithmetic checked here (a face average, a product, a divergence of stored faces) is restated in numpy in the kernels'
operation order: every comparison is assert_array_equal."""
import ctypes as C

import numpy as np
import pytest
from test_gpu_device_io import LAYOUTS, SENTINEL, _same_stats, _shape, _solver, _values

pytestmark = pytest.mark.gpu

RHS_SENTINEL, PHI_SENTINEL = 3.0e30, -5.0e29


def _inner(ghost, shape):
    """the valid cells of an array over valid.grow(ghost)"""
    return tuple(slice(g, n - g) for g, n in zip(ghost, shape))


def _wrap(valid, ghost, fill):
    a = np.full(tuple(n + 2 * g for n, g in zip(valid.shape, ghost)), fill, order="F")
    a[_inner(ghost, a.shape)] = valid
    return a


def _rhs_and_start(s, seed):
    rng = np.random.default_rng(seed)
    rhs = [rng.standard_normal(_shape(s, p)) for p in range(s.num_local_patches)]
    mean = sum(a.sum() for a in rhs) / sum(a.size for a in rhs)
    rhs = [np.asfortranarray(a - mean) for a in rhs]
    start = [np.asfortranarray(0.01 * rng.standard_normal(a.shape)) for a in rhs]
    return rhs, start


# ---- regions the host calls have always moved (these pass before and after the two paths were folded into one) ----------

def test_solve_on_host_arrays_uploads_valid_cells_only():
    """rhs on valid.grow(3) -- wider than the device frame, which is fine: only its valid cells move -- and phi on
    valid.grow((2, 0, 1)) from a given start.  The ghosts of both hold sentinels; the twin gets the same valid cells in an
    rhs without ghosts and a phi whose ghosts are zero.  Equal results and stats: no ghost cell was uploaded."""
    n, boxes, ndim = LAYOUTS["unequal"]
    s, twin = (_solver(n, boxes, ndim) for _ in range(2))   # the same life for both
    pg, rg = (2, 0, 1), (3, 3, 3)
    try:
        rhs, start = _rhs_and_start(s, 7)
        phi_a = [_wrap(a, pg, PHI_SENTINEL) for a in start]
        phi_b = [_wrap(a, pg, 0.0) for a in start]
        rhs_a = [_wrap(a, rg, RHS_SENTINEL) for a in rhs]
        st_a = dict(s.solve(phi_a, rhs_a, 0, 0, False, False, phi_ghost=pg, rhs_ghost=rg))
        st_b = dict(twin.solve(phi_b, rhs, 0, 0, False, False, phi_ghost=pg, rhs_ghost=(0, 0, 0)))
        _same_stats(st_a, st_b)
        for p in range(s.num_local_patches):
            assert phi_a[p][_inner(pg, phi_a[p].shape)].any()
            assert np.all(np.abs(phi_a[p]) < 1e20)   # neither sentinel came back: phi is written ghosts and all
            np.testing.assert_array_equal(phi_a[p], phi_b[p])
            np.testing.assert_array_equal(rhs_a[p], _wrap(rhs[p], rg, RHS_SENTINEL))   # rhs is read only
    finally:
        s.undefine()
        twin.undefine()


@pytest.mark.parametrize("layout,ghost", [("unequal", (2, 2, 2)), ("flat2d", (2, 2, 0))])
def test_cell_centred_velocity_with_two_ghost_layers(layout, ghost):
    """Distinct values in both ghost layers of the caller's array.  CellToEdge (divergenceCC) averages each cell with its
    neighbour into the resident MAC velocity, so the faces on a box's two ends in direction d show the first ghost layer in
    d, taken from the right place of an array with a wider ghost, and the divergence of those faces is restated on one box.
    (No call reads the resident array's second frame layer back, so that the second ghost layer stays behind is not
    observable here.)  The way down writes the valid cells only: both ghost layers of the caller's array keep 99."""
    from somar_amd import api as F
    n, boxes, ndim = LAYOUTS[layout]
    s = _solver(n, boxes, ndim)
    try:
        npatch = s.num_local_patches
        src = [_values(_shape(s, p, ghost) + (ndim,), p + 1) for p in range(npatch)]
        for p in range(npatch):
            s.uploadCCVel(p, src[p], ghost)
        dt = 0.5
        s.divergenceCC(F.F_RHS, dt, wall=False)
        for p in range(npatch):
            faces = []
            for d in range(ndim):
                sl = list(_inner(ghost, src[p].shape[:3]))
                sl[d] = slice(ghost[d] - 1, src[p].shape[d] - ghost[d] + 1)   # the valid cells and one ghost on either end
                c = src[p][tuple(sl) + (d,)]
                hi, lo = [slice(None)] * 3, [slice(None)] * 3
                hi[d], lo[d] = slice(1, None), slice(None, -1)
                faces.append(0.5 * (c[tuple(hi)] + c[tuple(lo)]))
                np.testing.assert_array_equal(s.downloadVel(d, p), faces[d])
            if p == 0:   # k_div_mac on the stored faces, Jinv = 1: ((du0) / dx0 + (du1) / dx1 + (du2) / dx2) / dt
                div = 0.0
                for d in range(3):
                    dxinv = 1.0 / (1.0 / n[d])
                    if d < ndim:
                        hi, lo = [slice(None)] * 3, [slice(None)] * 3
                        hi[d], lo[d] = slice(1, None), slice(None, -1)
                        term = (faces[d][tuple(hi)] - faces[d][tuple(lo)]) * dxinv
                    else:
                        term = 0.0 * dxinv
                    div = term if d == 0 else div + term
                np.testing.assert_array_equal(s.download(F.F_RHS, p, (0, 0, 0)), 1.0 * div / dt)
        for p in range(npatch):
            got = np.full_like(src[p], 99.0)
            s.downloadCCVel(p, got, ghost)
            want = np.full_like(src[p], 99.0)
            inner = _inner(ghost, src[p].shape[:3])
            want[inner] = src[p][inner]
            np.testing.assert_array_equal(got, want)   # the valid cells; every ghost keeps 99
    finally:
        s.undefine()


def test_j_scales_cell_centred_and_on_faces():
    """setCCJ with two ghost layers in the caller's arrays, setFaceJ on the face boxes: multByJ multiplies the resident
    velocities by exactly what was uploaded, on every valid cell resp. every face, the hi-side face of every box included"""
    n, boxes, ndim = LAYOUTS["unequal"]
    s = _solver(n, boxes, ndim)
    ghost = (2, 2, 2)
    try:
        npatch = s.num_local_patches
        rng = np.random.default_rng(11)
        vel = [np.asfortranarray(rng.standard_normal(_shape(s, p, ghost) + (ndim,))) for p in range(npatch)]
        J = [1.0 + 1e-4 * _values(_shape(s, p, ghost), p + 1) for p in range(npatch)]
        for p in range(npatch):
            s.setCCJ(p, J[p], np.asfortranarray(1.0 / J[p]), ghost)
            s.uploadCCVel(p, vel[p], ghost)
        s.multByJ(1)
        for p in range(npatch):
            got = np.full_like(vel[p], 99.0)
            s.downloadCCVel(p, got, ghost)
            inner = _inner(ghost, J[p].shape)
            for c in range(ndim):
                np.testing.assert_array_equal(got[inner + (c,)], vel[p][inner + (c,)] * J[p][inner])
        u = [[np.asfortranarray(rng.standard_normal(_shape(s, p, face=d))) for p in range(npatch)] for d in range(3)]
        Jf = [[2.0 + 1e-4 * _values(_shape(s, p, face=d), 10 * d + p + 1) for p in range(npatch)] for d in range(3)]
        for d in range(3):
            for p in range(npatch):
                s.setFaceJ(d, p, Jf[d][p], np.asfortranarray(1.0 / Jf[d][p]))
                s.uploadVel(d, p, u[d][p])
        s.multByJ(0)
        for d in range(3):
            for p in range(npatch):
                np.testing.assert_array_equal(s.downloadVel(d, p), u[d][p] * Jf[d][p])
    finally:
        s.undefine()


def test_heat_flux_is_a_face_array():
    """heatFlux(d, p) fills faces(valid, d), the +1 face included: a fresh accumulator is all zeros, and the caller's
    array, handed over full of a sentinel, comes back with none left"""
    from somar_amd import api as F
    n, boxes, ndim = LAYOUTS["unequal"]
    s = _solver(n, boxes, ndim)
    try:
        for d in range(3):
            for p in range(s.num_local_patches):
                shape = _shape(s, p, face=d)
                assert s.heatFlux(d, p).shape == shape
                out = np.full(shape, SENTINEL, order="F")
                F._ck(F.lib().somar_heat_flux_download(s._h, d, p, F._dp(out)))
                np.testing.assert_array_equal(out, np.zeros(shape))
    finally:
        s.undefine()


def test_metric_download_returns_what_set_metric_ortho_uploaded():
    """J g^{aa} on faces(valid, a) (which 0 .. 2) and J^{-1} on the valid cells (which 3) at depth 0 of "deep"; the values
    are a function of the global face / cell index, so they are distinct in every box and agree on shared faces"""
    from somar_amd import AMRPressureSolver
    n, boxes, ndim = LAYOUTS["deep"]
    s = AMRPressureSolver()
    s.setSpaceDim(ndim)
    s.define((0, 0, 0), tuple(a - 1 for a in n), (False, False, False), tuple(1.0 / a for a in n), boxes)

    def metric(p, which):
        lo, hi, _ = s.patch_box(p)
        ax = [np.arange(lo[a], hi[a] + 1 + (1 if a == which else 0)) for a in range(3)]
        I, J, K = np.meshgrid(*ax, indexing="ij")
        return np.asfortranarray(1.0 + 0.25 * which + 1e-5 * (I + 64.0 * J + 4096.0 * K))

    try:
        for p in range(s.num_local_patches):
            s.setMetricOrtho(p, *[metric(p, w) for w in range(4)])
        s.finalize()
        assert s.depth() >= 2
        for p in range(s.num_local_patches):
            for w in range(4):
                got = s.metricDownload(0, w, p)
                assert got.shape == _shape(s, p, face=w if w < 3 else None)
                np.testing.assert_array_equal(got, metric(p, w))
    finally:
        s.undefine()


# ---- the rules both paths follow since they are one path ------------------------------------------------------------------

def _all_sentinel(s, fields):
    for f in fields:
        for p in range(s.num_local_patches):
            assert np.all(s.download(f, p, (2, 2, 2)) == SENTINEL)


def test_solve_refuses_a_wide_phi_ghost_before_anything_moves():
    from somar_amd import SomarError
    from somar_amd import api as F
    n, boxes, ndim = LAYOUTS["unequal"]
    s = _solver(n, boxes, ndim)
    g = (3, 3, 3)
    try:
        rhs, start = _rhs_and_start(s, 8)
        for f in (F.F_PHI, F.F_RHS):
            s.setVal(f, SENTINEL)
        phi = [_wrap(a, g, 0.0) for a in start]
        with pytest.raises(SomarError, match="ghost wider"):
            s.solve(phi, rhs, 0, 0, False, False, phi_ghost=g)
        _all_sentinel(s, (F.F_PHI, F.F_RHS))   # nothing was uploaded, nothing was solved
        for p in range(s.num_local_patches):
            np.testing.assert_array_equal(phi[p], _wrap(start[p], g, 0.0))
    finally:
        s.undefine()


def test_amr_solve_refuses_a_wide_phi_ghost_before_anything_moves(oracle):
    """the two-level hierarchy of test_gpu_device_io.py's AMR twin test"""
    from helpers import make_amr_levels, make_gpu_amr
    from oracle import somar_amr as am
    from somar_amd import SomarError
    from somar_amd import api as F
    so = oracle
    ratios = [(2, 2, 2)]
    levels = make_amr_levels(so, am, (16, 16, 8), (2.0, 1.0, 0.5), (False, False, False), ratios,
                             [[so.Box((8, 8, 4), (23, 23, 11))]])
    gpu = make_gpu_amr(levels, ratios)
    g = (3, 3, 3)
    try:
        for v in gpu.levels:
            for f in (F.F_PHI, F.F_RHS):
                v.setVal(f, SENTINEL)
        phi = [[np.zeros(_shape(v, p, g), order="F") for p in range(v.num_local_patches)] for v in gpu.levels]
        rhs = [[np.ones(_shape(v, p), order="F") for p in range(v.num_local_patches)] for v in gpu.levels]
        with pytest.raises(SomarError, match="ghost wider"):
            gpu.solveAMRHost(phi, rhs, 0, 1, False, False, phi_ghost=g)
        for v in gpu.levels:
            _all_sentinel(v, (F.F_PHI, F.F_RHS))
    finally:
        gpu.undefine()


def test_none_entry_skips_its_patch_in_the_host_tables():
    """the host mirror of test_null_entry_skips_its_patch: a skipped patch keeps its resident values -- here put there
    beforehand by the per-patch calls -- so the call computes what the twin computes from full tables, and writes every
    array it was given"""
    from somar_amd import api as F
    n, boxes, ndim = LAYOUTS["unequal"]
    s, twin = (_solver(n, boxes, ndim) for _ in range(2))
    try:
        npatch = s.num_local_patches
        rhs, start = _rhs_and_start(s, 9)
        full = [_wrap(a, (1, 1, 1), 0.0) for a in start]
        st_t = dict(twin.solve(full, rhs, 0, 0, False, False))
        s.upload(F.F_RHS, 4, rhs[4], (0, 0, 0))
        s.upload(F.F_PHI, 1, start[1], (0, 0, 0))
        phi = [None if p == 1 else _wrap(start[p], (1, 1, 1), 0.0) for p in range(npatch)]
        st_s = dict(s.solve(phi, [None if p == 4 else rhs[p] for p in range(npatch)], 0, 0, False, False))
        _same_stats(st_s, st_t)
        for p in range(npatch):
            assert full[p].any()
            np.testing.assert_array_equal(s.download(F.F_PHI, p, (1, 1, 1)) if p == 1 else phi[p], full[p])

        rng = np.random.default_rng(10)
        vel = [[np.asfortranarray(rng.standard_normal(_shape(s, p, face=d))) for p in range(npatch)] for d in range(3)]
        want = [[a.copy(order="F") for a in vel[d]] for d in range(3)]
        st_t = dict(twin.levelProject(want, 0.5))
        skipped = [(0, 2), (2, 5)]
        for d, p in skipped:
            s.uploadVel(d, p, vel[d][p])
        got = [[None if (d, p) in skipped else vel[d][p].copy(order="F") for p in range(npatch)] for d in range(3)]
        st_s = dict(s.levelProject(got, 0.5))
        _same_stats(st_s, st_t)
        for d in range(3):
            for p in range(npatch):
                assert not np.array_equal(want[d][p], vel[d][p])
                np.testing.assert_array_equal(s.downloadVel(d, p) if (d, p) in skipped else got[d][p], want[d][p])
    finally:
        s.undefine()
        twin.undefine()


def test_field_download_checks_the_patch_index():
    from somar_amd import api as F
    n, boxes, ndim = LAYOUTS["unequal"]
    s = _solver(n, boxes, ndim)
    try:
        src = _values(_shape(s, 2), 3)
        s.upload(F.F_PHI, 2, src, (0, 0, 0))
        out = np.full(_shape(s, 0), SENTINEL, order="F")
        g0 = (C.c_int * 3)(0, 0, 0)
        for bad in (-1, s.num_local_patches):
            assert F.lib().somar_field_download(s._h, F.F_PHI, bad, F._dp(out), g0) != 0
            assert b"patch" in F.lib().somar_last_error()
            assert np.all(out == SENTINEL)
        np.testing.assert_array_equal(s.download(F.F_PHI, 2, (0, 0, 0)), src)   # a good call afterwards still works
    finally:
        s.undefine()
