"""An anchor for the oracle that shares NO code with it.

The reference ships no fixtures for the pressure path, so `oracle/` is pinned by known-answer tests only ("parity
unpinned") -- and every GPU parity test compares against that oracle.  A shared misreading of the reference's
ORCHESTRATION (coarse-metric averaging, J-weighted restriction, the mean removal, the cycle's order) would pass all of them.
This file restates the same mathematics a second time, as linear algebra with scipy.sparse / numpy array slicing, written
from the formulas of SURVEY.md 0.3 and Appendix B and from the reference sources cited below -- not from oracle/ -- and
checks the oracle against it:

  * the 7-point operator assembled as a sparse matrix from the metric ARRAYS (Neumann walls = zero boundary flux, periodic wrap)
    equals the oracle's applyOp to rounding; lapDiag equals FILLMAPPEDLAPDIAG's expression and, away from Neumann walls, the
    matrix diagonal (MappedAMRPoissonOpF.ChF:266-271; quirk Q3);
  * the 19-point operator written with array slices (fluxes with cross terms from an extrapolated copy, order 2,
    MappedAMRPoissonOpF.ChF:404-421, MappedAMRPoissonOp.cpp:2244-2270) equals the oracle's on a sheared and on a
    terrain-following metric;
  * one LevelGSRB sweep = (I - P_black D^-1 A)(I - P_red D^-1 A) with D the matrix diagonal (GSRBF.ChF:389-429, 616-698);
  * a whole V-cycle built from formulas -- coarse metric by arithmetic face / harmonic cell averages
    (MappedAMRPoissonOpFactory.cpp:1176-1185), residual restricted with J weighting (MappedCoarseAverageF.ChF:153-162),
    piecewise-constant prolongation followed by the removal of the J-weighted mean (ProlongationStrategyF.ChF:135-156,
    ProlongationStrategy.cpp:160-163), the order of MappedMultiGrid<T>::cycle (MappedMultiGrid.H:555-653), an exact bottom
    solve -- reproduces the oracle's V-cycle to 1e-9;
  * its asymptotic contraction factor (power iteration on the error propagator) reproduces what DESIGN.md 4 reports for the
    oracle: 0.43 per 2/2/2 V-cycle on the stretched metric at 32^3, 0.07 on the Cartesian one -- the stall of the headline
    workload is a property of this algorithm as written down twice, not of one restatement.

Parity with SOMAR itself stays unpinned: both restatements are readings of the same sources."""
import numpy as np
import pytest
import scipy.sparse as sp


# ----------------------------------------------------------------------------------------------------------------
# independent pieces: everything below works on plain numpy arrays indexed [i, j, k]
# ----------------------------------------------------------------------------------------------------------------
def assemble_7pt(jg, jinv, dx, periodic):
    """L[phi]_i = Jinv_i sum_a (F^a_{i+e_a} - F^a_i) / dx_a,  F^a_i = Jg^aa_i (phi_i - phi_{i-e_a}) / dx_a  (face i is the low
    face of cell i), F = 0 on non-periodic domain faces.  jg[a]: faces array, one longer than the cells along a."""
    n = jinv.shape
    N = int(np.prod(n))
    idx = np.arange(N).reshape(n)
    rows, cols, vals = [], [], []
    for a in range(3):
        for side in (0, 1):     # the low / high face of every cell
            face = jg[a][tuple(slice(side, side + n[d]) if d == a else slice(None) for d in range(3))]
            nb = np.roll(idx, 1 - 2 * side, axis=a)            # cell on the other side of that face
            w = jinv * face / (dx[a] * dx[a])
            if not periodic[a]:                                # zero flux through the wall: the face drops out
                sl = tuple((0 if side == 0 else n[a] - 1) if d == a else slice(None) for d in range(3))
                w = w.copy()
                w[sl] = 0.0
            rows += [idx.ravel(), idx.ravel()]
            cols += [nb.ravel(), idx.ravel()]
            vals += [w.ravel(), -w.ravel()]
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    A.sum_duplicates()
    return A


def lapdiag_formula(jg, jinv, dx):
    n = jinv.shape
    s = 0.0
    for a in range(3):
        lo = jg[a][tuple(slice(0, n[d]) if d == a else slice(None) for d in range(3))]
        hi = jg[a][tuple(slice(1, n[d] + 1) if d == a else slice(None) for d in range(3))]
        s = s + (hi + lo) / (dx[a] * dx[a])
    return -jinv * s


def apply_19pt(phi, jgf, jinv, dx, periodic, smoother=False):
    """the 19-point operator by array slices.  jgf[a][..., b] = J g^{ab} on a-faces.  psi = phi with one ghost layer:
    periodic wrap, or the quadratic extrapolation 3 (p1 - p2) + p3 beyond a wall.
    smoother: the cross terms see the SMOOTHER's copy instead (RelaxationMethod::fillGhostsAndExtrapolate,
    RelaxationMethod.cpp:376-435): linear extrapolation 2 p1 - p2 beyond EVERY face of the domain
    box, a periodic one included, direction after direction; the normal differences keep the periodic images."""
    n = phi.shape
    psi = np.zeros(tuple(m + 2 for m in n))
    psi[1:-1, 1:-1, 1:-1] = phi
    for d in range(3):
        def sl(i):
            return tuple(i if e == d else slice(None) for e in range(3))
        if periodic[d]:
            psi[sl(0)] = psi[sl(n[d])]
            psi[sl(n[d] + 1)] = psi[sl(1)]
        else:
            psi[sl(0)] = 3.0 * (psi[sl(1)] - psi[sl(2)]) + psi[sl(3)]
            psi[sl(n[d] + 1)] = 3.0 * (psi[sl(n[d])] - psi[sl(n[d] - 1)]) + psi[sl(n[d] - 2)]
    ext = psi
    if smoother:
        ext = np.zeros_like(psi)
        ext[1:-1, 1:-1, 1:-1] = phi
        for d in range(3):
            def sl(i):
                return tuple(i if e == d else slice(None) for e in range(3))
            ext[sl(0)] = 2.0 * ext[sl(1)] - ext[sl(2)]
            ext[sl(n[d] + 1)] = 2.0 * ext[sl(n[d])] - ext[sl(n[d] - 1)]

    out = np.zeros(n)
    for a in range(3):
        # faces 0 .. n_a along a; the face's high cell has padded index f + 1, its low cell f
        def at(cell_side, shift_dir=None, shift=0, src=psi):
            ix = []
            for e in range(3):
                if e == a:
                    ix.append(slice(cell_side, cell_side + n[a] + 1))
                elif e == shift_dir:
                    ix.append(slice(1 + shift, 1 + shift + n[e]))
                else:
                    ix.append(slice(1, 1 + n[e]))
            return src[tuple(ix)]
        F = jgf[a][..., a] * (at(1) - at(0)) / dx[a]
        for b in range(3):
            if b == a:
                continue
            F = F + jgf[a][..., b] / (4.0 * dx[b]) * (at(1, b, 1, ext) - at(1, b, -1, ext) + at(0, b, 1, ext) - at(0, b, -1, ext))
        if not periodic[a]:
            F[tuple(0 if e == a else slice(None) for e in range(3))] = 0.0
            F[tuple(n[a] if e == a else slice(None) for e in range(3))] = 0.0
        hi = F[tuple(slice(1, n[a] + 1) if e == a else slice(None) for e in range(3))]
        lo = F[tuple(slice(0, n[a]) if e == a else slice(None) for e in range(3))]
        out = out + (hi - lo) / dx[a]
    return jinv * out


def coarsen_metric(jg, jinv, r):
    """coarse J g^aa on a face = arithmetic mean of the fine faces it covers; coarse Jinv = harmonic mean of the children's"""
    n = jinv.shape
    nc = tuple(n[d] // r[d] for d in range(3))
    cj = []
    for a in range(3):
        f = jg[a][tuple(slice(None, None, r[d]) if d == a else slice(None) for d in range(3))]   # fine faces on coarse planes
        shp = []
        for d in range(3):
            shp += [f.shape[d], 1] if d == a else [nc[d], r[d]]
        cj.append(f.reshape(shp).mean(axis=(1, 3, 5)))
    inv = (1.0 / jinv).reshape(nc[0], r[0], nc[1], r[1], nc[2], r[2]).mean(axis=(1, 3, 5))
    return cj, 1.0 / inv


def transfer_matrices(jinv, r):
    """R: J-weighted mean of the children; P: every child takes its parent's value"""
    n = jinv.shape
    nc = tuple(n[d] // r[d] for d in range(3))
    fine = np.arange(int(np.prod(n))).reshape(n)
    I, J, K = np.meshgrid(*[np.arange(m) for m in n], indexing="ij")
    parent = ((I // r[0]) * nc[1] + (J // r[1])) * nc[2] + (K // r[2])
    P = sp.csr_matrix((np.ones(fine.size), (fine.ravel(), parent.ravel())), shape=(fine.size, int(np.prod(nc))))
    w = (1.0 / jinv).ravel()
    wsum = P.T @ w
    R = sp.diags(1.0 / wsum) @ P.T @ sp.diags(w)
    return R.tocsr(), P


def mg_ratio(dx, n, minbox=4):
    """the factory's rule (MappedAMRPoissonOpFactory.cpp:476-496) for ONE box covering the domain: coarsen the directions whose
    spacing is at most half the largest, all of them if none is; None when a direction would drop below minbox cells"""
    mx = max(dx)
    r = [2 if dx[d] <= mx / 2.0 else 1 for d in range(3)]
    if r == [1, 1, 1]:
        r = [2, 2, 2]
    if any(n[d] % r[d] or n[d] // r[d] < minbox for d in range(3)):
        return None
    return tuple(r)


class Depth:
    pass


def build_hierarchy(jg, jinv, dx, periodic):
    levels = []
    while True:
        L = Depth()
        L.jg, L.jinv, L.dx, L.n = jg, jinv, dx, jinv.shape
        L.A = assemble_7pt(jg, jinv, dx, periodic)
        L.Dinv = 1.0 / L.A.diagonal()
        I, J, K = np.meshgrid(*[np.arange(m) for m in L.n], indexing="ij")
        L.red = ((I + J + K) % 2 == 0).ravel()
        L.w = (1.0 / jinv).ravel()                     # dvol up to the constant dxProduct
        levels.append(L)
        r = mg_ratio(dx, L.n)
        if r is None:
            break
        L.r = r
        L.R, L.P = transfer_matrices(jinv, r)
        jg, jinv = coarsen_metric(jg, jinv, r)
        dx = tuple(dx[d] * r[d] for d in range(3))
    return levels


def sweep(L, e, rhs, count):
    for _ in range(count):
        for colour in (L.red, ~L.red):
            res = rhs - L.A @ e
            e = e + np.where(colour, L.Dinv * res, 0.0)
    return e


def vcycle(levels, d, e, rhs, pre=2, post=2, bottom=2, singular=True, cycles=1):
    """cycles = 1: a V-cycle; cycles = 2: a W-cycle (and so on)"""
    L = levels[d]
    if d == len(levels) - 1:
        e = sweep(L, e, rhs, bottom)
        # exact bottom solve started from e: e + the minimum-norm correction of what is left
        M = L.A.toarray()
        e = e + np.linalg.lstsq(M, rhs - M @ e, rcond=None)[0]
        return e
    e = sweep(L, e, rhs, pre)
    rc = L.R @ (rhs - L.A @ e)
    # the coarse correction is zeroed once; every further recursion continues from the previous one's result
    ec = np.zeros(rc.size)
    for _ in range(cycles):
        ec = vcycle(levels, d + 1, ec, rc, pre, post, bottom, singular, cycles)
    e = e + L.P @ ec
    if singular:
        e = e - np.dot(L.w, e) / L.w.sum()
    return sweep(L, e, rhs, post)


# ----------------------------------------------------------------------------------------------------------------
# glue to the oracle's containers (data in, data out -- no arithmetic)
# ----------------------------------------------------------------------------------------------------------------
def _one_box(so, n, periodic, L):
    dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), periodic)
    grids = so.split_domain(dom.box, max(n))
    assert len(grids) == 1
    dx = tuple(L[d] / n[d] for d in range(3))
    return dom, grids, dx


def _diag_arrays(Jgup, Jinv):
    return [np.array(Jgup[0][d].a[..., d]) for d in range(3)], np.array(Jinv[0].a[..., 0])


def valid_of_one(ld):
    return ld[0].view(ld.grids[0])[..., 0]


def _field(so, grids, arr, ghost=(1, 1, 1)):
    ld = so.LevelData(grids, 1, ghost)
    ld[0].view(grids[0])[..., 0] = arr
    return ld


CASES_7 = [
    ((16, 16, 16), (False, False, False), (1.0, 1.0, 1.0), "stretched"),
    ((16, 12, 8), (False, True, False), (2.0, 1.0, 0.5), "stretched"),
    ((8, 8, 16), (True, True, True), (1.0, 1.0, 3.0), "stretched"),
    ((16, 16, 16), (False, False, False), (1.0, 1.0, 1.0), "cartesian"),
]


@pytest.mark.parametrize("case", CASES_7)
def test_seven_point_operator_and_lapdiag_equal_the_assembled_matrix(oracle, case):
    so = oracle
    n, per, L, variant = case
    dom, grids, dx = _one_box(so, n, per, L)
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, L, 3, variant, domain=dom)
    jg, jinv = _diag_arrays(Jgup, Jinv)
    A = assemble_7pt(jg, jinv, dx, per)
    op = so.Factory(dom, grids, dx, so.BCHolder(), Jgup, Jinv, maxDepth=0).mg_new_op(0, None)
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, n)
    out = so.LevelData(grids, 1)
    op.apply_op(out, _field(so, grids, x), True)
    got = out[0].view(grids[0])[..., 0]
    want = (A @ x.ravel()).reshape(n)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # the operator annihilates constants and its J-weighted column sums vanish (conservation)
    assert np.abs(A @ np.ones(A.shape[0])).max() <= 1e-10 * np.abs(A.diagonal()).max()
    assert np.abs((1.0 / jinv).ravel() @ A).max() <= 1e-10 * np.abs(A.diagonal()).max()
    lap = op.lapDiag[0].view(grids[0])[..., 0]
    np.testing.assert_allclose(lap, lapdiag_formula(jg, jinv, dx), rtol=1e-14, atol=0)
    inner = tuple(slice(None) if per[d] else slice(1, -1) for d in range(3))
    np.testing.assert_allclose(lap[inner], A.diagonal().reshape(n)[inner], rtol=1e-13, atol=0)


@pytest.mark.parametrize("case", CASES_7[:3])
def test_level_gsrb_is_the_two_colour_gauss_seidel_of_that_matrix(oracle, case):
    so = oracle
    n, per, L, variant = case
    dom, grids, dx = _one_box(so, n, per, L)
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, L, 3, variant, domain=dom)
    jg, jinv = _diag_arrays(Jgup, Jinv)
    lv = build_hierarchy(jg, jinv, dx, per)[0]
    op = so.Factory(dom, grids, dx, so.BCHolder(), Jgup, Jinv, maxDepth=0).mg_new_op(0, None)
    rng = np.random.default_rng(11)
    e0, rhs = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    phi = _field(so, grids, e0)
    op.relax(phi, _field(so, grids, rhs, (0, 0, 0)), 2)
    got = phi[0].view(grids[0])[..., 0]
    want = sweep(lv, e0.ravel(), rhs.ravel(), 2).reshape(n)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_restated_bicgstab_solves_the_assembled_system(oracle):
    """Chombo 3.1's BiCGStabSolver is EXTERNAL to the reference tree and restated from its published algorithm (oracle
    BiCGStab, GPU bottom solvers).  Independent check of WHAT it solves: on a stretched 8 x 8 x 8 Neumann box (singular operator,
    right-hand side made compatible with the J-weighted null vector) its answer must satisfy the scipy-assembled system, and
    agree with scipy's direct least-squares solution up to the constant the null space leaves free."""
    import scipy.sparse.linalg as spla
    so = oracle
    n, per, L = (8, 8, 8), (False, False, False), (1.0, 2.0, 0.5)
    dom, grids, dx = _one_box(so, n, per, L)
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, L, 3, "stretched", domain=dom)
    jg, jinv = _diag_arrays(Jgup, Jinv)
    A = assemble_7pt(jg, jinv, dx, per)
    op = so.Factory(dom, grids, dx, so.BCHolder(), Jgup, Jinv, maxDepth=0).mg_new_op(0, None)
    rng = np.random.default_rng(31)
    b = rng.uniform(-1, 1, n)
    w = 1.0 / jinv                                   # left null vector of A: J (conservation)
    b = b - (w * b).sum() / w.sum()
    solver = so.BiCGStab(imax=400, eps=1e-12)
    solver.define(op, True)
    phi = _field(so, grids, np.zeros(n))
    solver.solve(phi, _field(so, grids, b, ghost=(0, 0, 0)))
    x = phi[0].view(grids[0])[..., 0].ravel()
    assert np.abs(A @ x - b.ravel()).max() <= 1e-8 * np.abs(b).max()
    ref = spla.lsqr(A, b.ravel(), atol=1e-14, btol=1e-14, iter_lim=20000)[0]
    d = (x - x.mean()) - (ref - ref.mean())
    assert np.abs(d).max() <= 1e-6 * np.abs(ref - ref.mean()).max()


@pytest.mark.parametrize("mode", [-1, 0, 1])
@pytest.mark.parametrize("iters", [0, 1, 3])
def test_restated_bicgstab_solves_the_assembled_system_with_every_preconditioner(oracle, mode, iters):
    """preCond's modes (None / DiagRelax / DiagLineRelax) and iteration counts change BiCGStab's iterates, not its answer:
    each must satisfy the same scipy-assembled system"""
    so = oracle
    n, per, L = (8, 8, 8), (False, False, False), (1.0, 2.0, 0.5)
    dom, grids, dx = _one_box(so, n, per, L)
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, L, 3, "stretched", domain=dom)
    jg, jinv = _diag_arrays(Jgup, Jinv)
    A = assemble_7pt(jg, jinv, dx, per)
    op = so.Factory(dom, grids, dx, so.BCHolder(), Jgup, Jinv, maxDepth=0, precondIters=iters,
                    precondMode=mode).mg_new_op(0, None)
    rng = np.random.default_rng(31)
    b = rng.uniform(-1, 1, n)
    w = 1.0 / jinv
    b = b - (w * b).sum() / w.sum()
    solver = so.BiCGStab(imax=400, eps=1e-12)
    solver.define(op, True)
    phi = _field(so, grids, np.zeros(n))
    solver.solve(phi, _field(so, grids, b, ghost=(0, 0, 0)))
    x = phi[0].view(grids[0])[..., 0].ravel()
    assert np.abs(A @ x - b.ravel()).max() <= 1e-8 * np.abs(b).max()


def _full_arrays(Jg, Ji):
    return [np.array(Jg[0][d].a) for d in range(3)], np.array(Ji[0].a[..., 0])


@pytest.mark.parametrize("per", [(False, False, False), (False, True, False)])
@pytest.mark.parametrize("metric", ["sheared", "terrain"])
def test_nineteen_point_operator_equals_the_sliced_formula(oracle, per, metric):
    so = oracle
    n, L = (16, 12, 8), (2.0, 1.0, 0.5)
    dom, grids, dx = _one_box(so, n, per, L)
    if metric == "sheared":
        Jg, Ji = so.make_full_metric(grids, dx, L, dom)
    else:
        from somar_amd import synthetic
        jgs, jv = synthetic.terrain_metric((0, 0, 0), tuple(a - 1 for a in n), dx, L)
        Jg, Ji = so.FluxData(grids, 3, 3), so.LevelData(grids, 1, (0, 0, 0), 1.0)
        for d in range(3):
            Jg[0][d].a[...] = jgs[d]
        Ji[0].a[..., 0] = jv
    jgf, jinv = _full_arrays(Jg, Ji)
    op = so.Factory(dom, grids, dx, so.BCHolder(), Jg, Ji, isDiagonal=False, maxDepth=0).mg_new_op(0, None)
    rng = np.random.default_rng(19)
    x = rng.uniform(-1, 1, n)
    out = so.LevelData(grids, 1)
    op.apply_op(out, _field(so, grids, x), True)
    got = out[0].view(grids[0])[..., 0]
    want = apply_19pt(x, jgf, jinv, dx, per)
    # Where a Neumann wall meets a periodic seam (or, on a multi-box layout, a box edge) the reference is NOT this formula:
    # setSideNeumBC's ExtrapolateFaceAndCopy (EllipticBCUtils.cpp:196, ExtrapolationUtils.cpp:136-152) extrapolates the wall's
    # ghost slab AND the first valid slab sideways into the tangential ghosts of the shared `extrap` copy, overwriting the
    # periodic images there ("Known reference behaviour reproduced").  The oracle follows the reference; the
    # deviation must be confined to the two cell layers next to a wall, in the rows / columns that touch a seam.
    junction = np.zeros(n, dtype=bool)
    I = np.meshgrid(*[np.arange(m) for m in n], indexing="ij")
    for a in range(3):
        if per[a]:
            continue
        near_wall = (I[a] <= 1) | (I[a] >= n[a] - 2)
        for b in range(3):
            if b != a and per[b]:
                junction |= near_wall & ((I[b] == 0) | (I[b] == n[b] - 1))
    tol = 1e-13 * np.abs(want).max()
    assert np.abs(got - want)[~junction].max() <= tol
    if junction.any():
        assert np.abs(got - want)[junction].max() > 1e-3 * np.abs(want).max()   # the quirk is there, and only there
    lap = op.lapDiag[0].view(grids[0])[..., 0]
    np.testing.assert_allclose(lap, lapdiag_formula([jgf[a][..., a] for a in range(3)], jinv, dx), rtol=1e-14, atol=0)


def test_nineteen_point_level_gsrb_is_a_coloured_jacobi_step_on_the_pre_pass_field(oracle):
    """LevelGSRB with a non-diagonal metric (GSRBITER3D, GSRBF.ChF:36-282): a colour pass takes EVERY neighbour -- the six
    of the other colour and the twelve diagonal ones of its own colour, which the reference reads from the snapshot
    `extrap` -- at its value before the pass.  As a formula: phi += mask_colour * (rhs - L~[phi]) / (alpha + beta lapDiag), with L~ the
    sliced 19-point operator above whose cross terms see the smoother's linearly extrapolated copy (apply_19pt(smoother=True)).
    Fully periodic box (no wall forms), sheared metric, two sweeps."""
    so = oracle
    n, L, per = (12, 8, 8), (2.0, 1.0, 0.5), (True, True, True)
    dom, grids, dx = _one_box(so, n, per, L)
    Jg, Ji = so.make_full_metric(grids, dx, L, dom)
    jgf, jinv = _full_arrays(Jg, Ji)
    op = so.Factory(dom, grids, dx, so.BCHolder(), Jg, Ji, isDiagonal=False, maxDepth=0).mg_new_op(0, None)
    rng = np.random.default_rng(23)
    x, b = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    phi = _field(so, grids, x)
    rhs = _field(so, grids, b, ghost=(0, 0, 0))
    op.relax(phi, rhs, 2)
    got = phi[0].view(grids[0])[..., 0]
    diag = lapdiag_formula([jgf[a][..., a] for a in range(3)], jinv, dx)       # alpha = 0, beta = 1
    I = np.meshgrid(*[np.arange(m) for m in n], indexing="ij")
    want = x.copy()
    for _ in range(2):
        for colour in (0, 1):
            mask = ((I[0] + I[1] + I[2] + colour) % 2) == 0
            want = want + mask * (b - apply_19pt(want, jgf, jinv, dx, per, smoother=True)) / diag
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("variant", ["stretched", "cartesian"])
def test_whole_vcycle_equals_the_cycle_built_from_formulas(oracle, variant):
    so = oracle
    n, per, L = (16, 16, 16), (False, False, False), (1.0, 1.0, 1.0)
    dom, grids, dx = _one_box(so, n, per, L)
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, L, 3, variant, domain=dom)
    jg, jinv = _diag_arrays(Jgup, Jinv)
    levels = build_hierarchy(jg, jinv, dx, per)
    fac = so.Factory(dom, grids, dx, so.BCHolder(), Jgup, Jinv)
    amr = so.AMRMultiGrid(fac, so.BiCGStab(eps=1e-14, reps=1e-14))
    assert amr.mg.depth == len(levels) == 3
    assert [tuple(r) for r in amr.mg.mgRefRatios] == [lv.r for lv in levels[:-1]]
    # the coarse metrics of both hierarchies
    for d, lv in enumerate(levels):
        o = amr.mg.ops[d]
        for a in range(3):
            np.testing.assert_allclose(o.Jgup[0][a].a[..., a], lv.jg[a], rtol=1e-14, atol=0)
        np.testing.assert_allclose(o.Jinv[0].a[..., 0], lv.jinv, rtol=1e-14, atol=0)
        assert o.zeroAvg
    rng = np.random.default_rng(23)
    res = rng.uniform(-1, 1, n)
    res -= (res / jinv).sum() / (1.0 / jinv).sum()          # in the range of the singular Neumann operator
    corr = so.LevelData(grids, 1, (1, 1, 1))
    resld = _field(so, grids, res, (0, 0, 0))
    amr.mg.init(corr, resld)
    amr.mg.bottomSolver = so.BiCGStab(eps=1e-14, reps=1e-14)
    amr.mg.bottomSolver.define(amr.mg.ops[-1], True)
    amr.mg.one_cycle(corr, resld)
    got = corr[0].view(grids[0])[..., 0]
    want = vcycle(levels, 0, np.zeros(res.size), res.ravel()).reshape(n)
    # both corrections are defined up to a constant only at the bottom; the mean removal on the way up fixes it
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("variant", ["stretched", "cartesian"])
@pytest.mark.parametrize("cycles", [2, 3])
def test_whole_w_cycle_equals_the_cycle_built_from_formulas(oracle, variant, cycles):
    """numMG = m_cycle > 1 (MappedMultiGrid.H:628-633): the coarser correction is set to zero ONCE, then `cycles` recursive
    calls each start from the previous call's result.  Depth 1 of this 3-depth hierarchy is entered `cycles` times, the bottom
    `cycles`**2 times -- all but the first of them from a non-zero correction."""
    so = oracle
    n, per, L = (16, 16, 16), (False, False, False), (1.0, 1.0, 1.0)
    dom, grids, dx = _one_box(so, n, per, L)
    Jgup, Jinv = so.make_diagonal_metric(grids, dx, L, 3, variant, domain=dom)
    jg, jinv = _diag_arrays(Jgup, Jinv)
    levels = build_hierarchy(jg, jinv, dx, per)
    fac = so.Factory(dom, grids, dx, so.BCHolder(), Jgup, Jinv)
    amr = so.AMRMultiGrid(fac, so.BiCGStab(eps=1e-14, reps=1e-14))
    assert amr.mg.depth == len(levels) == 3     # an intermediate depth that is revisited
    amr.mg.cycle_type = cycles
    entries = []
    inner = amr.mg.cycle

    def counting(depth, correction, residual):
        entries.append((depth, float(np.abs(valid_of_one(correction)).max())))
        return inner(depth, correction, residual)

    amr.mg.cycle = counting
    rng = np.random.default_rng(29)
    res = rng.uniform(-1, 1, n)
    res -= (res / jinv).sum() / (1.0 / jinv).sum()
    corr = so.LevelData(grids, 1, (1, 1, 1))
    resld = _field(so, grids, res, (0, 0, 0))
    amr.mg.init(corr, resld)
    amr.mg.bottomSolver = so.BiCGStab(eps=1e-14, reps=1e-14)
    amr.mg.bottomSolver.define(amr.mg.ops[-1], True)
    amr.mg.one_cycle(corr, resld)
    assert [d for d, _ in entries] == [0] + ([1] + [2] * cycles) * cycles
    # every revisit of a depth within one parent visit starts from the previous visit's (non-zero) result
    firsts = {i for i, (d, _) in enumerate(entries) if i == 0 or entries[i - 1][0] < d}
    for i, (d, m) in enumerate(entries):
        assert (m == 0.0) == (i in firsts), (i, d, m)
    got = corr[0].view(grids[0])[..., 0]
    want = vcycle(levels, 0, np.zeros(res.size), res.ravel(), cycles=cycles).reshape(n)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # and it is not the V-cycle
    v = vcycle(levels, 0, np.zeros(res.size), res.ravel()).reshape(n)
    assert np.abs(v - want).max() > 1e-3 * np.abs(want).max()


@pytest.mark.parametrize("variant,lo,hi", [("stretched", 0.42, 0.44), ("cartesian", 0.064, 0.074)])
def test_asymptotic_contraction_of_the_formula_cycle_matches_the_oracles(variant, lo, hi):
    """power iteration on  e -> e - V(A e)  at 32^3 (2/2/2 sweeps): profiles/r02_v4_c2_oracle_contraction_vs_h.json reports the
    ORACLE's residual ratios settling at 0.428-0.436 (stretched) and 0.065-0.069, still creeping up, (Cartesian) per cycle; this
    cycle gives 0.4295 and 0.0692"""
    n, per, L = (32, 32, 32), (False, False, False), (1.0, 1.0, 1.0)
    dx = tuple(L[d] / n[d] for d in range(3))
    if variant == "cartesian":
        jg = [np.ones(tuple(n[d] + (d == a) for d in range(3))) for a in range(3)]
        jinv = np.ones(n)
    else:   # the separable stretch of BASELINE C2 (ii): s_a = 1 + 0.3 sin(2 pi x_a / L_a + a), written out here once more
        def s(a, x):
            return 1.0 + 0.3 * np.sin(2.0 * np.pi * x / L[a] + a)
        cc = [(np.arange(n[d]) + 0.5) * dx[d] for d in range(3)]
        fc = [np.arange(n[d] + 1) * dx[d] for d in range(3)]
        jg = []
        for a in range(3):
            sv = [s(d, fc[d] if d == a else cc[d]) for d in range(3)]
            S = np.meshgrid(*sv, indexing="ij")
            others = [S[d] for d in range(3) if d != a]
            jg.append(others[0] * others[1] / S[a])
        S = np.meshgrid(*[s(d, cc[d]) for d in range(3)], indexing="ij")
        jinv = 1.0 / (S[0] * S[1] * S[2])
    levels = build_hierarchy(jg, jinv, dx, per)
    assert len(levels) == 4
    A, w = levels[0].A, levels[0].w
    rng = np.random.default_rng(5)
    e = rng.uniform(-1, 1, A.shape[0])
    ratios = []
    for it in range(25):
        # error e of an iterate, residual -A e; one V-cycle on the residual equation from a zero correction: e <- e - V(A e)
        e = e - np.dot(w, e) / w.sum()
        e = e / np.abs(A @ e).max()
        e = e - vcycle(levels, 0, np.zeros(e.size), A @ e)
        ratios.append(np.abs(A @ e).max())       # against 1 before the cycle
    tail = np.array(ratios[-6:])
    assert lo < tail.mean() < hi, ratios
