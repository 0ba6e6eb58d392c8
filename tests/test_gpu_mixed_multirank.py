"""The opt-in fp32 multigrid cycle (somar_solver_set_precision mode 1) on levels SHARDED over ranks: 2 and 4 processes on the
one GPU of the test box over the shared-memory transport, as tests/test_gpu_multirank.py runs the fp64 path.  The fp32 depths
exchange their ghost cells in fp32 messages (4 bytes per value); the sums, the seam, the replicated tail and the serial-order
depths stay fp64.

Cases: single level, 2/2/2 LevelGSRB V-cycles, a 64^3 grid of 32^3 boxes dealt round-robin to the ranks -- depths 64^3, 32^3,
16^3, ... -- in two tail modes:
  tail "replicated": SOMAR_AGGLOM_CELLS = 4096, depth 2 (16^3) is the landing layout of the replicated tail;
  tail "sharded":    SOMAR_AGGLOM_CELLS = 0, every depth is sharded and depth 2 is a serial-order depth.
Either way depths 0 and 1 run in fp32 (K = 2).  With the default SOMAR_AGGLOM_CELLS depth 1 is the landing layout and K = 1.

Every worker builds the oracle problem itself and checks ITS boxes:
  1. mode 1 is accepted, (1, K) is the same on every rank and follows from the depths' cell counts and the thresholds; mode 0
     after mode 1 restores the sharded fp64 solve bit for bit;
  2. one V-cycle from zero against the ORACLE's fp64 one_cycle of the whole problem, per owned box:
     0 < max|c32 - c_oracle| / max|c_oracle| <= 1e-6 (BOUND of tests/test_gpu_mixed_kernels.py for full-K 2/2/2 cycles);
  3. (test_overlap_is_only_scheduling) the exchange / compute overlap of the fp32 sweeps changes no bit;
  4. full solves against the same sharded solver in mode 0, the criteria of test_gpu_mixed_precision's
     test_full_solves_reach_fp64_tolerances, and two mixed solves in a row are bit-identical;
  5. bytes on the wire of one V-cycle: fp64(mode 1) + 2 * fp32(mode 1) == fp64(mode 0), fp32(mode 0) == 0 < fp32(mode 1); with
     every depth sharded the bottom solver's own exchanges (their number follows its iteration count) are taken off both sides;
  6. (test_ranks_that_disagree_raise) ranks that call setPrecision with different arguments all get an error that names the
     collective rule, and the solver goes on in mode 0."""
import multiprocessing as mp
import os
import traceback
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUND = 1e-6               # tests/test_gpu_mixed_kernels.py: full-K 2/2/2 cycles, about 17 fp32 unit roundoffs
ORDERED_MAX_CELLS = 4096   # levels of at most this many cells add their sums in the serial order and stay fp64 (solver.h)
DEFAULT_AGGLOM_CELLS = 2097152
TAILS = {"replicated": 4096, "sharded": 0, "default": None}

D, N = 1, 0
# (name, n, box, periodic, bc types per side, bc values, alpha, beta), the layout of test_gpu_mixed_precision.CASES
CASES = {
    "neumann": ("neumann", (64, 64, 64), 32, (False, False, False), None, None, 0.0, 1.0),
    "periodic-y": ("periodic-y", (64, 64, 64), 32, (False, True, False), None, None, 0.0, 1.0),
    "dirichlet": ("dirichlet", (64, 64, 64), 32, (False, False, False), [D] * 6, [0.25, -0.5, 0.75, 0.1, -0.3, 0.6], 0.0, 1.0),
}


def _case(name):
    if name == "helmholtz":
        from tests.test_gpu_mixed_precision import CASES as ONE_RANK_CASES
        return [c for c in ONE_RANK_CASES if c[0] == "helmholtz"][0]
    return CASES[name]


def _setup_env(tail):
    os.environ["SOMAR_FUSED_MIN_CELLS"] = "0"
    os.environ["SOMAR_MARCH_MIN_CELLS"] = "0"
    if TAILS[tail] is None:
        os.environ.pop("SOMAR_AGGLOM_CELLS", None)
    else:
        os.environ["SOMAR_AGGLOM_CELLS"] = str(TAILS[tail])
    for k in ("SOMAR_NO_OVERLAP", "SOMAR_NARROW_7PT"):
        os.environ.pop(k, None)
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (here, root):
        if p not in sys.path:
            sys.path.insert(0, p)


def _solver(case, prob, owner, comm, eps=1e-10, imax=100):
    """the sharded handle: 2/2/2 LevelGSRB V-cycles, this rank's boxes only"""
    from somar_amd import AMRPressureSolver
    types, values, alpha, beta = case[4:8]
    dom, grids, dx, Jgup, Jinv = prob
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], owner=owner, alpha=alpha, beta=beta,
             comm=comm, bc_type=types)
    if values is not None:
        s.setBCValues(values)
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                         np.asfortranarray(Jinv[gi].a[..., 0]))
    s.finalize()
    return s


def _expected_K(s, agglom_cells, min_cells=0):
    """mp_setup's rule restated from the depths' cell counts: depth d runs in fp32 while it lies above the landing layout of
    the replicated tail (the first depth >= 1 with at most agglom_cells cells), is no serial-order level, has at least
    min_cells cells and has a coarser depth (SOMAR_FUSED_MIN_CELLS = SOMAR_MARCH_MIN_CELLS = 0 here)"""
    cells = [s.levelInfo(d)["cells"] for d in range(s.depth())]
    land = next((d for d in range(1, len(cells)) if cells[d] <= agglom_cells), len(cells) - 1)
    K = 0
    for d in range(land):
        if cells[d] <= ORDERED_MAX_CELLS or cells[d] < min_cells:
            break
        K = d + 1
    return K, cells


def _oracle_cycle(so, case, prob, res):
    """the oracle's fp64 MultiGrid::one_cycle from zero on the WHOLE problem (homogeneous), 2/2/2 sweeps"""
    dom, grids, dx, Jgup, Jinv = prob
    bc = so.BCHolder() if case[4] is None else so.BCHolder([[case[4][2 * d], case[4][2 * d + 1]] for d in range(3)], None)
    fac = so.Factory(dom, grids, dx, bc, Jgup, Jinv, alpha=case[6], beta=case[7])
    amr = so.AMRMultiGrid(fac, so.BiCGStab())
    amr.pre = amr.post = amr.bottom = 2
    amr.mg.pre = amr.mg.post = amr.mg.bottom = 2
    corr = so.LevelData(grids, 1, (1, 1, 1))
    amr.mg.init(corr, res)
    amr.mg.bottomSolver = so.BiCGStab()
    amr.mg.bottomSolver.define(amr.mg.ops[-1], True)
    amr.mg.one_cycle(corr, res)
    return [f.view(g)[..., 0] for g, f in zip(corr.grids, corr.fabs)]


def _rhs(so, case, dom, grids, Jinv, seed):
    rhs = so.random_field(grids, seed, (0, 0, 0), dom.box)
    if case[4] is None and case[6] == 0.0:
        so.remove_weighted_mean(rhs, Jinv)   # Neumann / periodic Poisson: a compatible right-hand side
    return rhs


def _solve(s, grids, rhs):
    from somar_amd import api as F
    from helpers import download_valid, upload
    upload(s, F.F_RHS, rhs)
    st = s.solveResident(zeroPhi=True)
    return download_valid(s, F.F_PHI, grids), st


def _assert_same_solve(a, b, what):
    (pa, sa), (pb, sb) = a, b
    assert (sa["iters"], sa["exitStatus"]) == (sb["iters"], sb["exitStatus"]), what
    assert sa["history"] == sb["history"], what
    n = 0
    for x, y in zip(pa, pb):
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg=what)
            n += 1
    assert n > 0, "rank owns no box"


class _Gather:
    """sums over the ranks through shared memory: every rank deposits its values, a barrier (with a time limit) separates the
    writes from the reads"""

    def __init__(self, rank, nranks, slots, barrier):
        self.rank, self.nranks, self.slots, self.barrier = rank, nranks, slots, barrier

    def sum(self, values):
        n = len(values)
        self.barrier.wait(timeout=200)
        for i, v in enumerate(values):
            self.slots[self.rank * 8 + i] = v
        self.barrier.wait(timeout=200)
        return [sum(self.slots[r * 8 + i] for r in range(self.nranks)) for i in range(n)]


def _worker_cases(rank, nranks, name, casename, tail, q, slots, barrier):
    lines = []   # the measured figures, printed by the parent (also when an assertion fails)
    try:
        _setup_env(tail)
        from oracle import somar_oracle as so
        from somar_amd import api as F
        from helpers import download_valid, make_problem, upload
        case = _case(casename)
        gather = _Gather(rank, nranks, slots, barrier)
        comm = F.comm_create_shm(name, rank, nranks)
        prob = make_problem(so, case[1], case[2], "stretched", case[3], (1.0, 1.0, 1.0))
        dom, grids, dx, Jgup, Jinv = prob
        owner = [i % nranks for i in range(len(grids))]
        null_space = case[4] is None and case[6] == 0.0
        agglom = DEFAULT_AGGLOM_CELLS if TAILS[tail] is None else TAILS[tail]

        def solves_agree(eps, s64, s32):
            lines.append("rank %d %s/%s eps %g: iterations fp64 %d mixed %d, final / initial %.3e / %.3e" % (
                rank, casename, tail, eps, s64["iters"], s32["iters"], s64["final_rnorm"] / s64["initial_rnorm"],
                s32["final_rnorm"] / s32["initial_rnorm"]))
            assert s32["exitStatus"] & 1 and s64["exitStatus"] & 1, (s32, s64)   # converged: the residual test ended it
            assert s32["final_rnorm"] <= eps * s32["initial_rnorm"]
            if eps == 1e-10:
                assert s32["iters"] <= s64["iters"] + 1
            else:
                assert s32["iters"] == s64["iters"]

        rhs = _rhs(so, case, dom, grids, Jinv, seed=11)
        res = _rhs(so, case, dom, grids, Jinv, seed=5)

        # ======== a fresh handle (eps 1e-6): the split, one cycle against the oracle, the bytes, then the 1e-6 solves ========
        # (the cycles come before any solve: a solve leaves its convergence metric to the bottom solver, and the oracle's
        # one_cycle has a fresh bottom solver -- as in tests/test_gpu_mixed_kernels.py)
        s = _solver(case, prob, owner, comm, eps=1e-6)
        assert s.num_local_patches == len(grids) // nranks
        assert s.precision() == (0, 0)

        # ---- 1. accepted, the same split on every rank ----
        s.setPrecision(1)   # (refused with "more than one rank" before the fp32 halo exchange existed)
        K, cells = _expected_K(s, agglom)
        assert cells[:3] == [64 ** 3, 32 ** 3, 16 ** 3], cells
        assert K == (1 if tail == "default" else 2), (K, cells)
        assert s.precision() == (1, K), (s.precision(), K)
        ks = gather.sum([float(s.precision()[1])] + [float(s.precision()[1] == k) for k in range(4)])
        assert ks[0] == K * nranks and ks[1 + K] == nranks, ks   # every rank reports this K

        # ---- 5. bytes on the wire of one V-cycle, mode 1 and mode 0 on the same handle ----
        upload(s, F.F_RES, res)
        depths = s.depth()

        def cycle_bytes():
            """(fp64, fp32) bytes of one V-cycle from zero: in all, and per depth"""
            b0 = [s.exchangeBytes()] + [s.exchangeBytes(d) for d in range(depths)]
            s.vcycleFromZero(F.F_CORR, F.F_RES)
            b1 = [s.exchangeBytes()] + [s.exchangeBytes(d) for d in range(depths)]
            diff = [(y[0] - x[0], y[1] - x[1]) for x, y in zip(b0, b1)]
            assert diff[0] == (sum(v[0] for v in diff[1:]), sum(v[1] for v in diff[1:])), diff   # the depths add up
            return diff[0], diff[1:]

        mixed_bytes, mixed_depth = cycle_bytes()
        c32 = download_valid(s, F.F_CORR, grids)
        s.setPrecision(0)
        assert s.precision() == (0, 0)
        upload(s, F.F_RES, res)
        fp64_bytes, fp64_depth = cycle_bytes()
        lines.append("rank %d %s/%s/%d ranks: bytes per V-cycle fp64 mode %s, mixed mode %s; per depth fp64 mode %s, mixed mode %s" % (
            rank, casename, tail, nranks, fp64_bytes, mixed_bytes, fp64_depth, mixed_depth))
        assert mixed_bytes[1] > 0, mixed_bytes
        assert fp64_bytes[1] == 0, fp64_bytes
        if tail == "sharded":
            # Both paths issue the same exchanges but for ONE term (mixed precision): with every depth sharded the
            # BiCGStab bottom solver exchanges ghosts between the ranks, once per operator application, and how often it
            # iterates follows its right-hand side -- which differs by the fp32 cycle's rounding.  Those exchanges are all of
            # the last depth's; the identity holds exactly with that depth's bytes taken off both sides, and depth by depth.
            last = depths - 1
            assert K < last
            assert (mixed_bytes[0] - mixed_depth[last][0]) + 2 * mixed_bytes[1] == fp64_bytes[0] - fp64_depth[last][0], (
                mixed_bytes, fp64_bytes, mixed_depth, fp64_depth)
            for d in range(last):
                assert mixed_depth[d][0] + 2 * mixed_depth[d][1] == fp64_depth[d][0], (d, mixed_depth, fp64_depth)
            assert mixed_depth[last][1] == 0
        else:
            assert mixed_bytes[0] + 2 * mixed_bytes[1] == fp64_bytes[0], (mixed_bytes, fp64_bytes)
        for d in range(depths):   # fp32 messages on the fp32 depths, and only there
            assert (mixed_depth[d][1] > 0) == (d < K) and (d >= K or mixed_depth[d][0] == 0), (d, K, mixed_depth)

        # ---- 2. that one cycle against the oracle, per owned box ----
        want = _oracle_cycle(so, case, prob, res)
        errs = {gi: float(np.max(np.abs(g - w)) / np.max(np.abs(w))) for gi, (g, w) in enumerate(zip(c32, want))
                if g is not None}
        lines.append("rank %d %s/%s/%d ranks: per-box max|c32 - c_oracle| / max|c_oracle| = %s" % (
            rank, casename, tail, nranks, " ".join("%d:%.2e" % kv for kv in sorted(errs.items()))))
        assert len(errs) >= 1, "rank checked no box"
        assert all(0.0 < e <= BOUND for e in errs.values()), errs

        # ---- 4. full solves, eps 1e-6 ----
        p64, s64 = _solve(s, grids, rhs)
        s.setPrecision(1)
        assert s.precision() == (1, K)
        p32, s32 = _solve(s, grids, rhs)
        solves_agree(1e-6, s64, s32)
        s.undefine()

        # ======== a second handle (eps 1e-10): full solves, determinism, and mode 0 after mode 1 ========
        s = _solver(case, prob, owner, comm, eps=1e-10)
        ref = _solve(s, grids, rhs)   # the sharded fp64 solve of a handle that has never been in mode 1
        s.setPrecision(1)
        assert s.precision() == (1, K)
        m1 = _solve(s, grids, rhs)
        m2 = _solve(s, grids, rhs)
        _assert_same_solve(m1, m2, "two mixed solves in a row")
        assert m1[1]["history"] != ref[1]["history"]   # the fp32 cycle does run
        solves_agree(1e-10, ref[1], m1[1])
        a = np.concatenate([x.ravel() for x in m1[0] if x is not None])
        b = np.concatenate([x.ravel() for x in ref[0] if x is not None])
        tot = gather.sum([float(a.sum()), float(b.sum()), float(a.size)])   # (every rank takes part, null space or not)
        if null_space:   # the mean over ALL boxes, not over this rank's
            a, b = a - tot[0] / tot[2], b - tot[1] / tot[2]
        err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
        lines.append("rank %d %s/%s: |phi32 - phi64| / |phi64| = %.3e" % (rank, casename, tail, err))
        assert err <= 1e-8, err

        # ---- 1. mode 0 after mode 1: the sharded fp64 solve, bit for bit ----
        s.setPrecision(0)
        assert s.precision() == (0, 0)
        _assert_same_solve(_solve(s, grids, rhs), ref, "mode 0 after mode 1")
        s.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok", lines))
    except Exception:
        q.put((rank, traceback.format_exc(), lines))


def _worker_overlap(rank, nranks, name, q, slots, barrier):
    try:
        _setup_env("replicated")
        from oracle import somar_oracle as so
        from somar_amd import api as F
        from helpers import download_valid, make_problem, upload
        comm = F.comm_create_shm(name, rank, nranks)
        # the layout of test_gpu_multirank.py: one box per rank, with tiles that read no remote ghost cell
        case = ("overlap", (64, 64 * nranks, 32), (64, 64, 32), (False, True, False), None, None, 0.0, 1.0)
        prob = make_problem(so, case[1], case[2], "stretched", case[3], (2.0, 1.0, 1.0))
        dom, grids, dx, Jgup, Jinv = prob
        assert len(grids) == nranks
        owner = list(range(nranks))
        res = _rhs(so, case, dom, grids, Jinv, seed=5)
        got = {}
        for overlap, narrow in ((True, False), (False, False), (True, True)):
            if overlap:
                os.environ.pop("SOMAR_NO_OVERLAP", None)
            else:
                os.environ["SOMAR_NO_OVERLAP"] = "1"
            if narrow:
                os.environ["SOMAR_NARROW_7PT"] = "1"
            else:
                os.environ.pop("SOMAR_NARROW_7PT", None)
            s = _solver(case, prob, owner, comm)
            s.setPrecision(1)
            K, cells = _expected_K(s, TAILS["replicated"])
            assert K >= 2 and s.precision() == (1, K), (s.precision(), K, cells)   # (this metric semicoarsens: more depths)
            upload(s, F.F_RES, res)
            n0 = s.counters()["overlapped_sweeps"]
            s.vcycleFromZero(F.F_CORR, F.F_RES)
            n1 = s.counters()["overlapped_sweeps"]
            assert (n1 - n0 > 0) == overlap, (overlap, narrow, n0, n1)
            got[(overlap, narrow)] = ([x for x in download_valid(s, F.F_CORR, grids) if x is not None], n1 - n0)
            s.undefine()
        first = got[(True, False)][0]
        assert len(first) == 1 and float(np.max(np.abs(first[0]))) > 0.0
        for key, (c, _) in got.items():
            for x, y in zip(c, first):
                np.testing.assert_array_equal(x, y, err_msg="overlap, narrow = %r" % (key,))
        F.comm_destroy(comm)
        q.put((rank, "ok", ["rank %d: overlapped sweeps per mixed V-cycle %s" % (rank, {k: v[1] for k, v in got.items()})]))
    except Exception:
        q.put((rank, traceback.format_exc(), []))


def _worker_disagree(rank, nranks, name, q, slots, barrier):
    try:
        _setup_env("replicated")
        from oracle import somar_oracle as so
        from somar_amd import SomarError
        from somar_amd import api as F
        from helpers import make_problem
        comm = F.comm_create_shm(name, rank, nranks)
        case = _case("neumann")
        prob = make_problem(so, case[1], case[2], "stretched", case[3], (1.0, 1.0, 1.0))
        dom, grids, dx, Jgup, Jinv = prob
        owner = [i % nranks for i in range(len(grids))]
        s = _solver(case, prob, owner, comm)
        rhs = _rhs(so, case, dom, grids, Jinv, seed=11)
        ref = _solve(s, grids, rhs)
        c1 = s.levelInfo(1)["cells"]
        assert _expected_K(s, TAILS["replicated"])[0] == 2 and _expected_K(s, TAILS["replicated"], c1 + 1)[0] == 1
        # BOTH ranks make the call, so the collective completes; their arguments give K = 2 and K = 1
        with pytest.raises(SomarError, match="every rank"):
            if rank == 0:
                s.setPrecision(1)
            else:
                s.setPrecision(1, c1 + 1)
        assert s.precision() == (0, 0)
        _assert_same_solve(_solve(s, grids, rhs), ref, "mode 0 after the refused call")
        # ... and the same call made alike on every rank is accepted afterwards
        s.setPrecision(1, c1 + 1)
        assert s.precision() == (1, 1)
        st = _solve(s, grids, rhs)[1]
        assert st["exitStatus"] & 1 and st["final_rnorm"] <= 1e-10 * st["initial_rnorm"]
        s.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok", []))
    except Exception:
        q.put((rank, traceback.format_exc(), []))


def _run(target, nranks, *args):
    assert nranks <= 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    slots = ctx.Array("d", 8 * nranks)
    barrier = ctx.Barrier(nranks)
    name = "/somar_%s" % uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=target, args=(r, nranks, name) + args + (q, slots, barrier)) for r in range(nranks)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in procs:
            rank, msg, lines = q.get(timeout=300)
            out[rank] = msg
            for ln in lines:
                print(ln)
            if msg != "ok":
                break   # the peers of a failed rank wait for it in vain: do not wait for them
    finally:
        for p in procs:
            p.join(timeout=10 if all(m == "ok" for m in out.values()) and len(out) == nranks else 0.5)
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert out == {r: "ok" for r in range(nranks)}, "\n".join("rank %d: %s" % kv for kv in sorted(out.items()))


@pytest.mark.parametrize("casename,nranks,tail", [
    ("neumann", 2, "replicated"), ("neumann", 2, "sharded"),
    ("periodic-y", 2, "replicated"), ("periodic-y", 2, "sharded"),
    ("dirichlet", 2, "replicated"), ("dirichlet", 2, "sharded"),
    ("helmholtz", 2, "replicated"), ("helmholtz", 2, "sharded"),
    ("neumann", 4, "replicated"), ("neumann", 4, "sharded"),
    ("neumann", 2, "default"),
])
def test_sharded_mixed_cycle(casename, nranks, tail):
    _run(_worker_cases, nranks, casename, tail)


def test_overlap_is_only_scheduling():
    _run(_worker_overlap, 2)


def test_ranks_that_disagree_raise():
    _run(_worker_disagree, 2)
