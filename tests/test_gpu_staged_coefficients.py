"""Staged coefficients of the fused 7-point sweep (somar_amd/csrc/gsrb_fused.hip): the fp64, streamed-metric,
16-row instantiations of k_gsrb_fused fetch the six coefficient pairs of a plane one step ahead with loads that write LDS
directly, and phi a plane further ahead in registers.  The arithmetic is untouched -- the same values reach the same
expressions -- so no field may move by a bit: every case runs in fresh solvers with the staged form (default) and with
SOMAR_NO_STAGED_COEF=1 (the loads into registers, as before) and compares the two with array_equal; and it is held against the
oracle as tests/test_gpu_tall_tiles.py does, whose cases, problem set-up and oracle cycle this file shares (one oracle cycle per
case, computed once): bit for bit where every sum runs in the reference's serial order (sweep modes 1, 0, 2), to the project's
tree-sum tolerance (1e-12 of the correction's scale) where depth 0 folds prolongation and a tree-summed mean into its first
up-sweep (modes 1, 0 and 4, or 3 with Dirichlet sides).  Modes 3 and 4 themselves are not staged (they would spill, see the
resource table in profiles/r14_staged_coefficients.md): there the pair checks that the switch leaves them alone.

Shapes, the smallest that reach each risk (SOMAR_FUSED_MIN_CELLS=0 and SOMAR_STAGED_MIN_CELLS=0 -- by default only levels of
at least 4194304 cells take the staged form --, stretched metric everywhere):
  * class-0 body: one 40 x 24 x 8 box, two depths.  march_plan.h cuts 8 planes into two k-chunks of 4 (its shortest chunk), so
    the prologue's staging runs once per chunk and a chunk's last step stages nothing;
  * tall class-1 body: 136 x 40 x 16 and 136 x 28 x 16 -- partial last tile rows and columns, predicates off inside a wave;
  * a 136 x 28 x 8 box that is its own periodic neighbour in x and y;
  * Dirichlet sides + Helmholtz (the DIRI instantiations; the folded sweep is mode 3);
  * two boxes at different offsets in one level (the safe address is per patch);
  * mixed lane classes (SOMAR_NARROW_7PT=1: boxes 152 and 64 wide give classes 0 + 1 and 1 + 4): of the mixed-class kernels
    only the sweep from zero (mode 1) is staged;
  * an AMR fine level with coarse-fine faces on both x sides; two ranks over the shared-memory transport with the exchange
    overlapped (own / remote tile split); the fp32 cycle, which has no staged form.

What cannot be shown here: which of the two forms ran.  The bits agree by design and the library exports no launch counter for
the sweep; each case asserts what the solver holds for the switch, and the evidence that the staged kernels run (kernel names,
LDS size, times) is the trace in profiles/r14_staged_coefficients.md."""
import multiprocessing as mp
import os
import traceback
import uuid

import numpy as np
import pytest

from tests.helpers import download_valid, make_amr_levels, make_gpu_amr, upload, valid_of
from test_gpu_tall_tiles import (AMR_BOXES, AMR_L, AMR_N, AMR_RATIOS, HELMHOLTZ, ONE_BOX, ONE_ROW, ORDERED_ALL, SWEEPS,
                                 TREE_SUM_TOL, Case, _ranks_problem, _relax_and_restrict, assert_same, gpu_solver,
                                 oracle_cycle)

pytestmark = pytest.mark.gpu

FORMS = (("staged", None), ("registers", "1"))   # SOMAR_NO_STAGED_COEF
L3 = (2.0, 1.0, 0.5)
CLASS0 = Case("class0-40x24x8", (40, 24, 8), None, (False,) * 3, L3)
SELF_PERIODIC = Case("self-periodic-xy", (136, 28, 8), None, (True, True, False), L3)
TWO_BOXES = Case("two-boxes", (40, 48, 8), [((0, 0, 0), (39, 23, 7)), ((0, 24, 0), (39, 47, 7))], (False,) * 3, L3)
MIXED_01 = Case("mixed-classes-152", (152, 24, 8), None, (False,) * 3, L3)
MIXED_14 = Case("mixed-classes-64", (64, 24, 8), None, (False,) * 3, L3)
NARROW = {MIXED_01.name: "1", MIXED_14.name: "1"}   # SOMAR_NARROW_7PT of a case (unset otherwise)
SWITCHES = ("SOMAR_NARROW_7PT", "SOMAR_NO_NARROW_TILES", "SOMAR_FUSED_ROWS", "SOMAR_ORDERED_REDUCE_MAX", "SOMAR_NO_STAGED_COEF",
            "SOMAR_NO_UNIFORM")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("SOMAR_FUSED_MIN_CELLS", "0")
    monkeypatch.setenv("SOMAR_MARCH_MIN_CELLS", "0")
    monkeypatch.setenv("SOMAR_STAGED_MIN_CELLS", "0")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def set_env(monkeypatch, **kw):
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv("SOMAR_" + k, raising=False)
        else:
            monkeypatch.setenv("SOMAR_" + k, v)


def assert_switch(s, no_staged, depth=0):
    """what decides the staged form, as the solver reports it: the switch, 16-row kernels, a streamed (not uniform) metric"""
    assert s.tuning("NO_STAGED_COEF") == (1 if no_staged else 0) and s.tuning("STAGED_MIN_CELLS") == 0
    assert s.tuning("FUSED_ROWS") == 16 and s.tuning("FUSED_MIN_CELLS") == 0
    assert s.metricUniform(depth) is None


def gpu_cycle(case, prob, res, no_staged, fold, fp32=False):
    """one V-cycle from zero, 2/2/2.  fold: whether depth 0 is on the folded-prolongation path (its inputs are asserted)"""
    from somar_amd import api as F
    s = gpu_solver(case, prob)
    try:
        assert_switch(s, no_staged)
        cells = [s.levelInfo(d)["cells"] for d in range(s.depth())]
        limit = s.tuning("ORDERED_REDUCE_MAX")
        assert len(cells) >= 2 and all(c <= limit for c in cells[1:]), (cells, limit)
        assert (cells[0] > limit) == fold and s.tuning("NO_FOLD_PROLONG") == 0, (cells, limit)
        if fp32:
            s.setPrecision(1)
            assert s.precision()[0] == 1 and s.precision()[1] >= 1, s.precision()
        upload(s, F.F_RES, res)
        s.vcycleFromZero(F.F_CORR, F.F_RES)
        return download_valid(s, F.F_CORR, prob[1])
    finally:
        s.undefine()


def below_top(case):
    """a sum limit between depth 0 and every coarser depth (each at most half of it)"""
    return str(int(np.prod(case.n)) - 1)


@pytest.mark.parametrize("case", [CLASS0, ONE_BOX, ONE_ROW, SELF_PERIODIC, HELMHOLTZ, TWO_BOXES, MIXED_01, MIXED_14], ids=repr)
def test_vcycle_same_bits_staged_or_not_and_against_the_oracle(oracle, monkeypatch, case):
    prob, res, want = oracle_cycle(oracle, case)
    scale = max(float(np.abs(w).max()) for w in want)
    for ordered, fold in ((ORDERED_ALL, False), (below_top(case), True)):
        got = {}
        for label, no_staged in FORMS:
            set_env(monkeypatch, NO_STAGED_COEF=no_staged, ORDERED_REDUCE_MAX=ordered, NARROW_7PT=NARROW.get(case.name))
            got[label] = gpu_cycle(case, prob, res, no_staged, fold)
        assert_same(got["staged"], got["registers"], "%s, sum limit %s: staged against register loads" % (case, ordered))
        if not fold:
            assert_same(got["staged"], want, "%s: staged coefficients against the oracle, serial-order sums" % case)
        else:
            for i, (g, w) in enumerate(zip(got["staged"], want)):
                print("%s box %d, depth 0 folded (mode %s): max|c - c_oracle| / scale = %.3e" % (
                    case, i, "3" if case.bc else "4", np.abs(g - w).max() / scale))
                np.testing.assert_allclose(g, w, rtol=0, atol=TREE_SUM_TOL * scale, err_msg="%s box %d" % (case, i))


def test_fp32_cycle_is_left_alone(oracle, monkeypatch):
    """the float instantiations have no staged form (a float pair is 8 bytes, not a width the load has): the opt-in fp32 cycle on
    depth 0 -- above the sum limit and outside graph replay, as tests/test_gpu_tall_tiles.py sets it up -- gives the same bits
    with the switch either way.  Its distance from the fp64 oracle is printed, not bounded (see that file)."""
    case = ONE_BOX
    prob, res, want = oracle_cycle(oracle, case)
    monkeypatch.setenv("SOMAR_GRAPH_CELLS", "4096")
    got = {}
    for label, no_staged in FORMS:
        set_env(monkeypatch, NO_STAGED_COEF=no_staged, ORDERED_REDUCE_MAX=below_top(case))
        got[label] = gpu_cycle(case, prob, res, no_staged, True, fp32=True)
    assert_same(got["staged"], got["registers"], "fp32 cycle: switch off against switch on")
    err = max(float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got["staged"], want))
    print("fp32 cycle: max|c32 - c_oracle| / max|c_oracle| = %.3e" % err)


def test_amr_vcycle_bit_exact_staged_or_not(oracle, monkeypatch):
    """one AMR V-cycle from zero on the hierarchy of tests/test_gpu_tall_tiles.py: a refined level of one 136-wide box with
    coarse-fine faces on both x sides, whose ghosts of the black pass are made inside the sweep"""
    from oracle import somar_amr as am
    from somar_amd import api as F
    so = oracle
    fb = [[so.Box(lo, hi) for lo, hi in lev] for lev in AMR_BOXES]
    levels = make_amr_levels(so, am, AMR_N, AMR_L, (False, True, False), AMR_RATIOS, fb, variant="stretched", cbox=AMR_N)
    comp = am.AMRComposite(levels, AMR_RATIOS, so.BCHolder(), so.BiCGStab(), isDiagonal=True)
    phi = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
    res = [so.random_field(L.grids, 70 + l, (0, 0, 0), L.domain.box) for l, L in enumerate(levels)]
    comp.zero_covered(0, res[0])
    comp.init(phi, res, 1, 0)
    comp.set_bottom_solver(1, 0)
    corr = [so.LevelData(L.grids, 1, (1, 1, 1)) for L in levels]
    comp.amr_vcycle(corr, res, 1, 1, 0)
    want = [[np.array(x) for x in valid_of(c)] for c in corr]
    got = {}
    for label, no_staged in FORMS:
        set_env(monkeypatch, NO_STAGED_COEF=no_staged, ORDERED_REDUCE_MAX=ORDERED_ALL)
        gpu = make_gpu_amr(levels, AMR_RATIOS)
        try:
            for v in gpu.levels:
                assert_switch(v, no_staged)
            for l, v in enumerate(gpu.levels):
                upload(v, F.F_RES, res[l])
                v.setVal(F.F_CORR, 0.0)
            gpu.vcycleAMR(1, 0)
            got[label] = [download_valid(gpu.levels[l], F.F_CORR, levels[l].grids) for l in range(2)]
        finally:
            gpu.undefine()
    for l in range(2):
        assert_same(got["staged"][l], got["registers"][l], "AMR V-cycle level %d: staged against register loads" % l)
        assert_same(got["staged"][l], want[l], "AMR V-cycle level %d against the oracle" % l)


def _worker(rank, nranks, name, path, q):
    try:
        os.environ["SOMAR_FUSED_MIN_CELLS"] = "0"
        os.environ["SOMAR_MARCH_MIN_CELLS"] = "0"
        os.environ["SOMAR_STAGED_MIN_CELLS"] = "0"
        for k in SWITCHES + ("SOMAR_NO_OVERLAP",):
            os.environ.pop(k, None)
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, os.path.dirname(here))
        from oracle import somar_oracle as so
        from somar_amd import api as F
        from tests.helpers import make_gpu_solver
        want = np.load(path)
        comm = F.comm_create_shm(name, rank, nranks)
        dom, grids, dx, Jgup, Jinv = _ranks_problem(so)
        assert len(grids) == nranks
        for label, no_staged in FORMS:
            if no_staged is None:
                os.environ.pop("SOMAR_NO_STAGED_COEF", None)
            else:
                os.environ["SOMAR_NO_STAGED_COEF"] = no_staged
            gpu = make_gpu_solver(dom, grids, dx, Jgup, Jinv, owner=list(range(nranks)), comm=comm)
            try:
                assert_switch(gpu, no_staged)
                got = _relax_and_restrict(so, F, gpu, grids, dom)
                assert gpu.counters()["overlapped_sweeps"] >= SWEEPS, gpu.counters()
                mine = [(gi, g) for gi, g in enumerate(got) if g is not None]
                assert len(mine) == 1
                for gi, g in mine:
                    np.testing.assert_array_equal(g, want["box%d" % gi], err_msg="%s, box %d" % (label, gi))
            finally:
                gpu.undefine()
        F.comm_destroy(comm)
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_two_ranks_match_one_process(oracle, monkeypatch, tmp_path):
    """three fused sweeps (plain, mode 0) on the level of tests/test_gpu_tall_tiles.py sharded over two ranks, the exchange
    travelling under the tiles that read no remote cell: staged or not, the bits of the one-process run, which is the oracle's
    relax"""
    from somar_amd import api as F
    from tests.helpers import make_gpu_solver, make_oracle_solver
    so = oracle
    dom, grids, dx, Jgup, Jinv = _ranks_problem(so)
    gpu = make_gpu_solver(dom, grids, dx, Jgup, Jinv)
    try:
        assert_switch(gpu, None)
        one = _relax_and_restrict(so, F, gpu, grids, dom)
    finally:
        gpu.undefine()
    phi = so.random_field(grids, 13, (1, 1, 1), dom.box)
    rhs = so.random_field(grids, 14, (0, 0, 0), dom.box)
    make_oracle_solver(so, dom, grids, dx, Jgup, Jinv).mg.ops[0].relax(phi, rhs, SWEEPS)
    assert_same(one, valid_of(phi), "one process against the oracle's relax")
    path = str(tmp_path / "one_process.npz")
    np.savez(path, **{"box%d" % i: a for i, a in enumerate(one)})
    nranks = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/somar_%s" % uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=_worker, args=(r, nranks, name, path, q)) for r in range(nranks)]
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
