"""The volume-discrepancy correction (AMRNavierStokes::computeVDCorrection, NavierStokes/AMRNavierStokesSync.cpp:850-1060) on
the GPU against a reference COMPOSED here from oracle functions: AMRComposite.solve, QuadCFInterp.coarse_fine_interp,
CFRegion.extrapolate_cf_ev, level_gradient_mac, orc_unmappedaverageface (MappedCoarseAverageF.ChF:182-237) and
compute_amr_operator.

The face copy onto the coarse level (MappedCoarseAverage.cpp:400-520, m_coarsenedFineData->copyTo(a_coarseData)) is restated
in _average_down_ref with the library's documented rule: where several coarsened fine boxes (or periodic images) supply one
coarse face, the box later in layout order wins, periodic images last.  The rule is UNPINNED against the reference (Chombo's
Copier is not part of it); the tests show that it cannot matter with a diagonal metric (both candidates hold the same bits)
and that layout f does exercise it.

Layouts (base level 16 x 16 x 8 in boxes of 8, lengths (2.0, 1.0, 0.5)): the smallest at which each piece can go wrong --
a interior box; b the coarsened boxes start at the boundary between two coarse boxes (the coarse box WITHOUT a fine cell
receives its high face) and two fine boxes share faces; c periodic, coarse face 0 is also face 16 of the last box, ratio 1
in z; d three levels (l_base 0 and 1); e ratio (4, 1, 1): four fine faces per coarse x-face, one per y / z-face; f layout b
with the non-diagonal metric; g a 2-D hierarchy.

The error return "l_base > 0 needs level l_base - 1" cannot be produced through the interface: a hierarchy's levels are
contiguous from 0, so every valid level range has that level; the other three error returns are tested."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_amr_levels, make_full_amr_levels, make_gpu_amr, max_rel_diff, upload

pytestmark = pytest.mark.gpu

N3, L3 = (16, 16, 8), (2.0, 1.0, 0.5)
LAYOUTS = {
    "a": dict(periodic=(False, False, False), ratios=[(2, 2, 2)], boxes=[[((8, 8, 4), (23, 23, 11))]]),
    "b": dict(periodic=(False, False, False), ratios=[(2, 2, 2)],
              boxes=[[((16, 0, 0), (31, 15, 15)), ((16, 16, 0), (31, 31, 15))]]),
    "c": dict(periodic=(True, False, False), ratios=[(2, 2, 1)], boxes=[[((0, 8, 0), (15, 23, 7)), ((24, 8, 0), (31, 23, 7))]]),
    "d": dict(periodic=(False, True, False), ratios=[(2, 2, 1), (2, 2, 1)],
              boxes=[[((8, 0, 0), (23, 31, 7))], [((24, 0, 0), (39, 63, 7))]]),
    "e": dict(periodic=(False, False, False), ratios=[(4, 1, 1)], boxes=[[((16, 4, 0), (47, 11, 7))]]),
    "f": dict(periodic=(False, False, False), ratios=[(2, 2, 2)],
              boxes=[[((16, 0, 0), (31, 15, 15)), ((16, 16, 0), (31, 31, 15))]], full=True),
    "g": dict(periodic=(False, False, False), ratios=[(2, 2, 1)], boxes=[[((8, 8, 0), (15, 23, 0)), ((16, 8, 0), (23, 23, 0))]],
              ndim=2),
}
MULT = 0.3 / 0.07   # etaLambda / dt: not a power of two
POISON = -7.25


@pytest.fixture(scope="module")
def am(oracle):
    from oracle import somar_amr
    return somar_amr


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _setup(so, am, name):
    lay = LAYOUTS[name]
    full, ndim = lay.get("full", False), lay.get("ndim", 3)
    fb = [[so.Box(lo, hi) for lo, hi in lev] for lev in lay["boxes"]]
    n, L, cbox = (N3, L3, 8) if ndim == 3 else ((16, 16, 1), (2.0, 1.0, 1.0), (8, 8, 1))
    if full:
        levels = make_full_amr_levels(so, am, n, L, lay["periodic"], lay["ratios"], fb, cbox=cbox, ndim=ndim)
    else:
        levels = make_amr_levels(so, am, n, L, lay["periodic"], lay["ratios"], fb, cbox=cbox, ndim=ndim)
    comp = am.AMRComposite(levels, lay["ratios"], so.BCHolder(), so.BiCGStab(), ndim=ndim, isDiagonal=not full)
    gpu = make_gpu_amr(levels, lay["ratios"], ndim=ndim, full=full)
    return levels, comp, gpu


# ---- the composed reference ---------------------------------------------------------------------------------------
def _shifts(so, domain):
    """the unshifted image first, then the periodic images in (x, y, z) lexicographic order of (-n, 0, +n)"""
    return [(0, 0, 0)] + [s for s in so.periodic_shifts(domain) if s != (0, 0, 0)]


def _covered_faces(so, levels, ratios, l, d):
    """the stated set: per coarse box, the mask over faces(box, d) of the faces that are faces of a coarsened box of level
    l + 1 or of a periodic image of one"""
    cfb = [g.coarsen(ratios[l]) for g in levels[l + 1].grids]
    out = []
    for g in levels[l].grids:
        gf = g.faces(d)
        m = np.zeros(gf.size(), dtype=bool)
        for sh in _shifts(so, levels[l].domain):
            for cb in cfb:
                r = gf & cb.faces(d).shift(sh)
                if not r.isEmpty():
                    m[r.slices(gf.lo)] = True
        out.append(m)
    return out


def _average_down_ref(so, levels, ratios, l, crse, fine, nd):
    """MappedCoarseAverageFace::averageToCoarse(crse, fine): UNMAPPEDAVERAGEFACE per fine box and direction onto
    faces(coarsen(fineBox), d), then the copy onto the valid faces of the coarse level, candidates applied in ascending
    priority (layout order, periodic images last) so that the later box wins.  crse / fine: per box, per direction Fabs over
    faces(box, d).  -> the number of faces where a later candidate overwrote DIFFERENT bits."""
    r = ratios[l]
    cfb = [g.coarsen(r) for g in levels[l + 1].grids]
    avg = [[so.Fab(cb.faces(d), 1, np.nan) for d in range(nd)] for cb in cfb]
    for i, cb in enumerate(cfb):
        for d in range(nd):
            lo, hi = so._b(cb.faces(d))
            so.lib().orc_unmappedaverageface(*avg[i][d].fra(), *fine[i][d].fran(), lo, hi, d, so._ivc(r))
    differ = 0
    for j, g in enumerate(levels[l].grids):
        for d in range(nd):
            gf = g.faces(d)
            written = np.zeros(gf.size(), dtype=bool)
            for sh in _shifts(so, levels[l].domain):
                for i, cb in enumerate(cfb):
                    reg = gf & cb.faces(d).shift(sh)
                    if reg.isEmpty():
                        continue
                    src = avg[i][d].view(reg.shift([-s for s in sh]), 0)
                    dst = crse[j][d].view(reg, 0)
                    w = written[reg.slices(gf.lo)]
                    differ += int(np.count_nonzero(w & (dst != src)))
                    dst[...] = src
                    written[reg.slices(gf.lo)] = True
    return differ


def _gradient_ref(so, comp, levels, ratios, phi, l_max, l_base):
    """the gradient loop, AMRNavierStokesSync.cpp:1001-1044 -> (grad[l][box][d] Fabs, faces where the rule mattered)"""
    nd = comp.ndim
    grad = [None] * len(levels)
    differ = 0
    for l in range(l_max, l_base - 1, -1):
        L, op = levels[l], comp.ops[l]
        so.exchange(phi[l], L.domain, phi[l].ghost)               # the BC pass's exchange, :984-988
        if l > 0:                                                 # levelGradientMAC, Gradient.cpp:104-114
            op.quad.coarse_fine_interp(phi[l], phi[l - 1])
            if not op.isDiagonal:
                op.cf.extrapolate_cf_ev(phi[l], 2, op.activeDirs)
        g = so.FluxData(L.grids, 1, nd)
        so.level_gradient_mac(g, phi[l], L.grids, L.domain, L.Jgup, L.dx, nd, op=op)
        grad[l] = g.fabs
        if l < l_max:
            differ += _average_down_ref(so, levels, ratios, l, grad[l], grad[l + 1], nd)
    return grad, differ


def _download_grad(gpu, l, nd):
    """-> [box][d] arrays over faces(box, d)"""
    v = gpu.levels[l]
    out = [None] * v.num_local_patches
    for p in range(v.num_local_patches):
        out[v.patch_box(p)[2]] = [v.downloadVel(d, p) for d in range(nd)]
    return out


def _upload_grad(gpu, l, fabs, nd):
    v = gpu.levels[l]
    for p in range(v.num_local_patches):
        gi = v.patch_box(p)[2]
        for d in range(nd):
            v.uploadVel(d, p, np.asfortranarray(fabs[gi][d].a[..., 0]))


def _random_faces(so, grids, nd, seed):
    rng = np.random.default_rng(seed)
    out = [[so.Fab(g.faces(d), 1) for d in range(nd)] for g in grids]
    for row in out:
        for f in row:
            f.a[...] = rng.uniform(-1.0, 1.0, f.a.shape)
    return out


def _poison_faces(so, grids, nd):
    """distinct negative values per face: a face written from the wrong place shows"""
    out = [[so.Fab(g.faces(d), 1) for d in range(nd)] for g in grids]
    for i, row in enumerate(out):
        for d, f in enumerate(row):
            f.a[...] = POISON - (np.arange(f.a.size, dtype=np.float64).reshape(f.a.shape, order="F") + 1000.0 * (3 * i + d))
    return out


# ---- 1. the right-hand side -------------------------------------------------------------------------------------------
def test_vd_rhs_is_lambda_minus_one_times_mult_bit_for_bit(oracle, am):
    from somar_amd import api as F
    so = oracle
    levels, comp, gpu = _setup(so, am, "a")
    try:
        assert np.log2(MULT) != np.round(np.log2(MULT))
        for l, L in enumerate(levels):
            lam = so.random_field(L.grids, 40 + l, (0, 0, 0), L.domain.box)
            for f in lam.fabs:
                f.a[...] = 1.0 + 1e-3 * f.a
            upload(gpu.levels[l], F.F_RHS, lam)
            gpu.vdRhs(l, MULT)
            v = gpu.levels[l]
            for p in range(v.num_local_patches):
                gi = v.patch_box(p)[2]
                np.testing.assert_array_equal(v.download(F.F_RHS, p, (0, 0, 0)), (lam[gi].a[..., 0] - 1.0) * MULT)
    finally:
        gpu.undefine()


# ---- 2. the gradient loop given the same eLambda ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_gradient_loop_bit_exact(oracle, am, name):
    from somar_amd import api as F
    so = oracle
    levels, comp, gpu = _setup(so, am, name)
    try:
        nd, lmax, ratios = comp.ndim, len(levels) - 1, comp.refRatios
        phi = [so.random_field(L.grids, 5 + l, (1, 1, 1), L.domain.box) for l, L in enumerate(levels)]
        for l, v in enumerate(gpu.levels):
            upload(v, F.F_PHI, phi[l])
        want, differ = _gradient_ref(so, comp, levels, ratios, phi, lmax, 0)
        if LAYOUTS[name].get("full"):
            # the layout has to exercise the later-box-wins rule: the two fine boxes hold different bits on shared faces
            print("faces where the two candidates differ:", differ)
            assert differ > 0
        else:
            assert differ == 0   # diagonal metric: both candidates of every shared face are equal, the rule cannot matter
        gpu.compGradientMAC(lmax, 0)
        for l in range(lmax + 1):
            got = _download_grad(gpu, l, nd)
            for i in range(len(levels[l].grids)):
                for d in range(nd):
                    np.testing.assert_array_equal(got[i][d], want[l][i][d].a[..., 0], err_msg="level %d box %d dir %d" % (l, i, d))
    finally:
        gpu.undefine()


# ---- 3. the face average alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_average_down_faces_from_poisoned_coarse_arrays(oracle, am, name):
    so = oracle
    levels, comp, gpu = _setup(so, am, name)
    try:
        nd, lmax, ratios = comp.ndim, len(levels) - 1, comp.refRatios
        for l in range(lmax):
            fine = _random_faces(so, levels[l + 1].grids, nd, 70 + l)
            crse = _poison_faces(so, levels[l].grids, nd)
            poison = [[f.a[..., 0].copy() for f in row] for row in crse]
            _upload_grad(gpu, l + 1, fine, nd)
            _upload_grad(gpu, l, crse, nd)
            gpu.averageDownFaces(l)
            # independent fine values on shared faces: the rule decides, and the reference applies it
            _average_down_ref(so, levels, ratios, l, crse, fine, nd)
            got = _download_grad(gpu, l, nd)
            for d in range(nd):
                stated = _covered_faces(so, levels, ratios, l, d)
                for i in range(len(levels[l].grids)):
                    at = "level %d box %d dir %d" % (l, i, d)
                    np.testing.assert_array_equal(got[i][d] != poison[i][d], stated[i], err_msg=at)
                    np.testing.assert_array_equal(got[i][d], crse[i][d].a[..., 0], err_msg=at)
            # the fine arrays are read only
            back = _download_grad(gpu, l + 1, nd)
            for i in range(len(levels[l + 1].grids)):
                for d in range(nd):
                    np.testing.assert_array_equal(back[i][d], fine[i][d].a[..., 0])
        if name == "b":
            # coarse face x = 8 is the low side of the coarsened fine boxes: the coarse boxes [0..7] hold no fine cell and must
            # still receive it as their high face
            stated = _covered_faces(so, levels, ratios, 0, 0)
            hit = [i for i, g in enumerate(levels[0].grids) if g.hi[0] == 7 and stated[i][-1].any()]
            assert hit and all(stated[i][-1].all() and not stated[i][:-1].any() for i in hit)
        if name == "c":
            # periodic: coarse face 0 is also the high face 16 of the last coarse box
            stated = _covered_faces(so, levels, ratios, 0, 0)
            assert any(g.hi[0] == 15 and stated[i][-1].any() for i, g in enumerate(levels[0].grids))
    finally:
        gpu.undefine()


# ---- 4. the whole call ----------------------------------------------------------------------------------------------------------
def _compatible_lambda(so, am, comp, levels, lmax, lbase):
    """lambda = 1 + L(random phi) / mult: (lambda - 1) * mult is then in the range of the composite operator"""
    phi0 = [so.random_field(L.grids, 20 + l, (1, 1, 1), L.domain.box) for l, L in enumerate(levels)]
    for l in range(lbase):
        so.ld_set(phi0[l], 0.0)   # the call zeroes level l_base - 1
    lph = [so.LevelData(L.grids, 1) for L in levels]
    am.compute_amr_operator(comp, lph, phi0, lmax, lbase, False)
    lam = [so.LevelData(L.grids, 1) for L in levels]
    for l in range(lbase, lmax + 1):
        for a, b in zip(lam[l].fabs, lph[l].fabs):
            a.a[...] = 1.0 + b.a / MULT
    return lam


@pytest.mark.parametrize("name,lbase", [("a", 0), ("c", 0), ("d", 0), ("d", 1), ("f", 0)])
def test_vd_correction_matches(oracle, am, name, lbase):
    from somar_amd import api as F
    so = oracle
    levels, comp, gpu = _setup(so, am, name)
    try:
        full = LAYOUTS[name].get("full", False)
        nd, lmax, ratios = comp.ndim, len(levels) - 1, comp.refRatios
        lam = _compatible_lambda(so, am, comp, levels, lmax, lbase)
        # the reference: rhs = (lambda - 1) * mult, eLambda = 0 on l_base - 1 .. l_max, solve, gradient loop
        rhs = [so.LevelData(L.grids, 1) for L in levels]
        for l in range(lbase, lmax + 1):
            for a, b in zip(rhs[l].fabs, lam[l].fabs):
                a.a[...] = (b.a - 1.0) * MULT
        phi = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
        comp.solve(phi, rhs, lmax, lbase, zeroPhi=False)
        want, _ = _gradient_ref(so, comp, levels, ratios, phi, lmax, lbase)
        # the library
        for l in range(lbase, lmax + 1):
            upload(gpu.levels[l], F.F_RHS, lam[l])
        for l, v in enumerate(gpu.levels):
            v.setVal(F.F_PHI, 3.5)   # the call must zero l_base - 1 .. l_max itself
        poison = None
        if lbase > 0:
            poison = _poison_faces(so, levels[0].grids, nd)
            _upload_grad(gpu, 0, poison, nd)
        st = gpu.vdCorrection(lmax, lbase, MULT)
        print("iters", st["iters"], comp.iters, "exit", st["exitStatus"], comp.exitStatus)
        assert st["iters"] > 0
        assert st["iters"] == comp.iters and st["exitStatus"] == comp.exitStatus
        tol = 1e-9 if full else 1e-10
        np.testing.assert_allclose(st["history"], comp.history, rtol=tol, atol=tol * comp.history[0])
        for l in range(lbase, lmax + 1):
            got = _download_grad(gpu, l, nd)
            for d in range(nd):
                assert max(float(np.max(np.abs(w[d].a))) for w in want[l]) > 0.0
                diff = max_rel_diff([g[d] for g in got], [w[d].a[..., 0] for w in want[l]])
                print("level %d dir %d max_rel_diff %.3e" % (l, d, diff))
                assert diff < (1e-7 if full else 1e-8), (l, d)
        if lbase > 0:
            v = gpu.levels[0]
            for p in range(v.num_local_patches):
                assert not v.download(F.F_PHI, p, (0, 0, 0)).any()   # level l_base - 1: eLambda zeroed
            got = _download_grad(gpu, 0, nd)
            for i in range(len(levels[0].grids)):
                for d in range(nd):
                    np.testing.assert_array_equal(got[i][d], poison[i][d].a[..., 0])   # its MAC arrays untouched
    finally:
        gpu.undefine()


# ---- 5. caller arrays in host and device memory ------------------------------------------------------------------------------
def _to_dev(torch, a):
    return torch.from_numpy(np.ravel(a, order="F").copy()).cuda()


def _to_host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def test_host_and_device_calls_equal_the_resident_call(oracle, am, torch):
    from somar_amd import api as F
    from somar_amd import lib
    so = oracle
    levels, comp, gpu = _setup(so, am, "b")
    try:
        nd, lmax = comp.ndim, len(levels) - 1
        lam_ld = _compatible_lambda(so, am, comp, levels, lmax, 0)
        eg = (1, 1, 1)
        # the resident call followed by downloads
        for l in range(lmax + 1):
            upload(gpu.levels[l], F.F_RHS, lam_ld[l])
        st_r = dict(gpu.vdCorrection(lmax, 0, MULT))
        want_e, want_g = [], []
        for l, v in enumerate(gpu.levels):
            want_e.append([v.download(F.F_PHI, p, eg) for p in range(v.num_local_patches)])
            want_g.append([[v.downloadVel(d, p) for p in range(v.num_local_patches)] for d in range(nd)])
        # per level, per local patch host arrays
        lam = [[np.asfortranarray(lam_ld[l][v.patch_box(p)[2]].a[..., 0]) for p in range(v.num_local_patches)]
               for l, v in enumerate(gpu.levels)]
        lam0 = [[a.copy() for a in row] for row in lam]

        def outputs():
            e = [[np.full(a.shape, POISON, order="F") for a in row] for row in want_e]
            g = [[[np.full(a.shape, POISON, order="F") for a in want_g[l][d]] for l in range(lmax + 1)] for d in range(nd)]
            return e, g

        def scramble():
            for v in gpu.levels:
                v.setVal(F.F_PHI, 1.5)
                v.setVal(F.F_RHS, 2.5)

        scramble()
        e_h, g_h = outputs()
        st_h = dict(gpu.vdCorrectionHost(lam, e_h, g_h, lmax, 0, MULT, elambda_ghost=eg))
        scramble()
        d_lam = [[_to_dev(torch, a) for a in row] for row in lam]
        e0, g0 = outputs()
        d_e = [[_to_dev(torch, a) for a in row] for row in e0]
        d_g = [[[_to_dev(torch, a) for a in lev] for lev in g0[d]] for d in range(nd)]
        st_d = dict(gpu.vdCorrectionDev(d_lam, d_e, d_g, lmax, 0, MULT, elambda_ghost=eg))
        for st in (st_h, st_d):
            assert st["iters"] == st_r["iters"] > 0 and st["exitStatus"] == st_r["exitStatus"]
            np.testing.assert_array_equal(st["history"], st_r["history"])
        for l in range(lmax + 1):
            for p in range(len(lam[l])):
                np.testing.assert_array_equal(lam[l][p], lam0[l][p])                                  # read-only
                np.testing.assert_array_equal(_to_host(d_lam[l][p], lam0[l][p].shape), lam0[l][p])
                np.testing.assert_array_equal(e_h[l][p], want_e[l][p])
                np.testing.assert_array_equal(_to_host(d_e[l][p], want_e[l][p].shape), want_e[l][p])
                for d in range(nd):
                    np.testing.assert_array_equal(g_h[d][l][p], want_g[l][d][p])
                    np.testing.assert_array_equal(_to_host(d_g[d][l][p], want_g[l][d][p].shape), want_g[l][d][p])
        # a host pointer handed to _dev (the LAST lambda entry, after valid ones) is refused before anything moved
        for v in gpu.levels:
            v.setVal(F.F_PHI, POISON)
            v.setVal(F.F_RHS, POISON)
        for row in d_e:
            for t in row:
                t.fill_(POISON)
        for dd in d_g:
            for row in dd:
                for t in row:
                    t.fill_(POISON)
        nl = lmax + 1
        keep = []

        def table(rows_of_ptrs):
            rows = (C.POINTER(C.c_void_p) * nl)()
            for l, ptrs in enumerate(rows_of_ptrs):
                row = (C.c_void_p * len(ptrs))(*ptrs)
                keep.append(row)
                rows[l] = C.cast(row, C.POINTER(C.c_void_p))
            return rows

        lam_ptrs = [[t.data_ptr() for t in row] for row in d_lam]
        lam_ptrs[-1][-1] = lam[-1][-1].ctypes.data
        g3 = [table([[t.data_ptr() for t in row] for row in d_g[d]]) for d in range(nd)]
        gh, ge = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(*eg)
        stc = F.Stats()
        torch.cuda.synchronize()
        rc = lib().somar_amr_vd_correction_dev(gpu._amr, table(lam_ptrs), gh, table([[t.data_ptr() for t in row] for row in d_e]),
                                               ge, g3[0], g3[1], g3[2], lmax, 0, MULT, C.byref(stc))
        assert rc != 0
        msg = lib().somar_last_error().decode()
        assert "not a device pointer" in msg and "lambda" in msg, msg
        for l, v in enumerate(gpu.levels):
            for p in range(v.num_local_patches):
                assert np.all(v.download(F.F_PHI, p, (0, 0, 0)) == POISON) and np.all(v.download(F.F_RHS, p, (0, 0, 0)) == POISON)
                assert bool((d_e[l][p] == POISON).all())
                for d in range(nd):
                    assert bool((d_g[d][l][p] == POISON).all())
    finally:
        gpu.undefine()


# ---- 6. error returns -------------------------------------------------------------------------------------------------------
def test_error_returns(oracle, am):
    from somar_amd import AMRPressureSolver, SomarError
    so = oracle
    levels, comp, gpu = _setup(so, am, "a")
    try:
        for bad in (0.0, float("inf"), float("nan")):
            with pytest.raises(SomarError, match="lambda_mult"):
                gpu.vdCorrection(1, 0, bad)
            with pytest.raises(SomarError, match="lambda_mult"):
                gpu.vdRhs(0, bad)
        for lmax, lbase in ((2, 0), (0, 1), (1, -1)):
            with pytest.raises(SomarError, match="level range"):
                gpu.vdCorrection(lmax, lbase, MULT)
            with pytest.raises(SomarError, match="level range"):
                gpu.compGradientMAC(lmax, lbase)
        with pytest.raises(SomarError, match="level range"):
            gpu.vdRhs(2, MULT)
        with pytest.raises(SomarError, match="level range"):
            gpu.averageDownFaces(1)
    finally:
        gpu.undefine()
    raw = AMRPressureSolver()
    L0 = levels[0]
    raw.defineAMR(L0.domain.box.lo, L0.domain.box.hi, L0.domain.periodic, L0.dx, LAYOUTS["a"]["ratios"],
                  [[(g.lo, g.hi) for g in L.grids] for L in levels])
    try:
        with pytest.raises(SomarError, match="finalized"):
            raw.vdCorrection(1, 0, MULT)
        with pytest.raises(SomarError, match="finalized"):
            raw.compGradientMAC(1, 0)
        with pytest.raises(SomarError, match="finalized"):
            raw.averageDownFaces(0)
        with pytest.raises(SomarError, match="finalized"):
            raw.vdRhs(0, MULT)
    finally:
        raw.undefine()
