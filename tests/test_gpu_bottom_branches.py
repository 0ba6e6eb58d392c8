"""Every way out of the BiCGStab loop, and the restart, on the three one-launch bottom solvers that test_gpu_bottom_local.py
does not reach: k_tiny_bicgstab (kind 1), the multi-box k_box_bicgstab with 1, 2 and 4 cells per thread (kind 2) and its
19-point variant (kind 2, FULL) -- against the oracle's restatement of Chombo's BiCGStabSolver and against the launch-by-launch
path PressureSolver::bottom_solve (kind 0).

Serial-order sums everywhere (SOMAR_ORDERED_REDUCE_MAX covers every level), so the three sides agree BIT FOR BIT: iteration
count, exit code, solution, and a second solve on the same handle from that answer (a non-zero guess; kernel against launch
path).  Each case also asserts ON THE ORACLE that the branch it is named after is taken -- exit code, restarts counted as the
solver's calls of op.residual minus one, iters == imax, the skipped second half-step counted as calls of op.apply_op -- so a
drift of the inputs cannot turn a case into a plain converging solve.

Branches: exit 3 with and without a restart before it; a restart followed by convergence (the only case that shows the
state after the reset is right); the iteration limit; the `small` branch; the `reps` guard with the second half-step skipped;
exit 2 (rho == 0 exactly) and the loop never entered; normType 0 / 1 / 2; a Helmholtz operator.  Then whole solves, where
AMRMultiGrid's convergence metric replaces the bottom solver's initial norm, with bottom solves that leave through -1 / 3
on the first cycles; and graph-replayed cycles whose bottom kernel leaves through its early return while the host collects
(iterations, exit code) only after the up leg is enqueued.

Oracle results are computed once per module and shared; the launch path's are shared by the targets on the same level."""
import numpy as np
import pytest

from helpers import download_valid, make_problem, upload, valid_of

pytestmark = pytest.mark.gpu

ORDERED_ALL = "1000000"
SWITCHES = ("SOMAR_BOX_BOTTOM", "SOMAR_FUSED_BOTTOM_MAX_CELLS", "SOMAR_BOX_BOTTOM_MIN_CELLS", "SOMAR_GRAPH_CELLS",
            "SOMAR_BOTTOM_ASYNC", "SOMAR_ORDERED_REDUCE_MAX")
LAUNCH_ENV = dict(SOMAR_BOX_BOTTOM="0", SOMAR_FUSED_BOTTOM_MAX_CELLS="0")
TINY_ENV = dict(SOMAR_BOX_BOTTOM="0")
BOX_ENV = dict(SOMAR_FUSED_BOTTOM_MAX_CELLS="0", SOMAR_BOX_BOTTOM="1", SOMAR_BOX_BOTTOM_MIN_CELLS="1")
FULL_ENV = dict(SOMAR_BOX_BOTTOM="1")
KIND_ENV = {0: LAUNCH_ENV, 1: TINY_ENV, 2: BOX_ENV}

# level -> (n, boxsz, variant, periodic, L, maxDepth, alpha, beta, 19-point); the bottom level is the one under test
LEVELS = {
    "32^3": ((32, 32, 32), 16, "stretched", (False, False, False), (1.0, 1.0, 1.0), -1, 0.0, 1.0, False),
    "32^3-helmholtz": ((32, 32, 32), 16, "stretched", (False, True, False), (1.0, 1.0, 1.0), -1, 1.0, -0.05, False),
    "36x20x12": ((36, 20, 12), (12, 20, 4), "stretched", (False, False, True), (1.0, 1.0, 3.0), 0, 0.0, 1.0, False),
    "32x32x16": ((32, 32, 16), (16, 16, 8), "cartesian", (False, True, False), (1.0, 1.0, 1.0), 0, 0.0, 1.0, False),
    "sheared": ((16, 16, 8), 8, "sheared", (False, True, False), (2.0, 1.0, 0.5), -1, 0.0, 1.0, True),
    "16^3-two-deep": ((16, 16, 16), 8, "stretched", (False, False, False), (1.0, 1.0, 1.0), 2, 0.0, 1.0, False),
}
# target -> (level, boxes and cells per box of the bottom level, environment, bottomKind()): the smallest levels that select
# the single-workgroup kernel, the multi-box kernel with 1 (64-thread workgroups), 2 and 4 cells per thread, the 19-point one
TARGETS = {
    "T": ("32^3", 8, 64, TINY_ENV, 1),
    "B1": ("32^3", 8, 64, BOX_ENV, 2),
    "B2": ("36x20x12", 9, 960, BOX_ENV, 2),
    "B4": ("32x32x16", 8, 2048, BOX_ENV, 2),
    "F": ("sheared", 4, 128, FULL_ENV, 2),
    "T-helmholtz": ("32^3-helmholtz", 8, 64, TINY_ENV, 1),
    "B1-helmholtz": ("32^3-helmholtz", 8, 64, BOX_ENV, 2),
}
ALL = ("T", "B1", "B2", "B4", "F")


@pytest.fixture(scope="module")
def F():
    from somar_amd import api
    return api


def _key(params):
    return tuple(sorted(params.items()))


# ---- the oracle's side: built once per level -----------------------------------------------------------------------------------
_LEVEL, _RHS, _ORACLE, _LAUNCH = {}, {}, {}, {}


def _level(so, name):
    """-> (problem, the oracle's AMRMultiGrid on it): the bottom operator is amr.mg.ops[-1]"""
    if name not in _LEVEL:
        n, boxsz, variant, periodic, L, maxDepth, alpha, beta, full = LEVELS[name]
        if full:
            dom = so.Domain(so.Box((0, 0, 0), tuple(a - 1 for a in n)), periodic)
            grids = so.split_domain(dom.box, boxsz)
            dx = tuple(L[d] / n[d] for d in range(3))
            Jgup, Jinv = so.make_full_metric(grids, dx, L, dom)
            prob = (dom, grids, dx, Jgup, Jinv)
        else:
            prob = make_problem(so, n, boxsz, variant, periodic, L)
        fac = so.Factory(prob[0], prob[1], prob[2], so.BCHolder(), prob[3], prob[4], alpha=alpha, beta=beta,
                         isDiagonal=not full, maxDepth=maxDepth)
        _LEVEL[name] = (prob, so.AMRMultiGrid(fac, so.BiCGStab()))
    return _LEVEL[name]


def _bottom_rhs(so, name, kind):
    """"random": random_field seed 91, its weighted mean removed where the operator has a null space (on the 19-point level:
    the operator applied to such a field, so that it is in the range -- with the other one the deck defaults stagnate);
    "tiny": that times 1e-170, whose norm is positive while every product of two of its values underflows to zero;
    "zero": all zero"""
    if (name, kind) not in _RHS:
        opb = _level(so, name)[1].mg.ops[-1]
        if LEVELS[name][8]:
            rhs = so.LevelData(opb.grids, 1)
            opb.apply_op(rhs, so.random_field(opb.grids, 91, (1, 1, 1), opb.domain.box), True)
        else:
            rhs = so.random_field(opb.grids, 91, (0, 0, 0), opb.domain.box)
            if LEVELS[name][6] == 0.0:
                so.remove_weighted_mean(rhs, opb.Jinv)
        if kind == "tiny":
            so.ld_scale(rhs, 1e-170)
        elif kind == "zero":
            so.ld_set(rhs, 0.0)
        _RHS[(name, kind)] = rhs
    return _RHS[(name, kind)]


class _Counted:
    """counts the calls of one method of an operator while a solver runs"""

    def __init__(self, op, *names):
        self.op, self.names, self.calls = op, names, {}

    def __enter__(self):
        for name in self.names:
            self.calls[name] = 0
            setattr(self.op, name, self._wrap(name, getattr(self.op, name)))
        return self.calls

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.calls[name] += 1
            return fn(*a, **kw)
        return counted

    def __exit__(self, *exc):
        for name in self.names:
            delattr(self.op, name)     # the instance attribute goes, the class's method is back


def _oracle_bottom(so, name, params, rhs_kind="random"):
    """-> dict(iters, exit, sol, restarts, applies) of so.BiCGStab(**params) on the level's bottom, from a zero guess"""
    key = (name, _key(params), rhs_kind)
    if key not in _ORACLE:
        opb = _level(so, name)[1].mg.ops[-1]
        rhs = _bottom_rhs(so, name, rhs_kind)
        bs = so.BiCGStab(**params)
        bs.define(opb, True)
        phi = so.LevelData(opb.grids, 1, (1, 1, 1))
        with _Counted(opb, "residual", "apply_op") as calls:
            bs.solve(phi, rhs)
        _ORACLE[key] = dict(iters=bs.iters, exit=bs.exitStatus, sol=[a.copy() for a in valid_of(phi)],
                            restarts=calls["residual"] - 1, applies=calls["apply_op"])
    return _ORACLE[key]


# ---- the GPU's side -------------------------------------------------------------------------------------------------------------
def _gpu(so, name, env, params, monkeypatch):
    """a solver on the level created under `env` + serial-order sums (the switches are read at construction; every other
    bottom switch at its default), with the BiCGStab parameters of `params` where they differ from the deck's"""
    from somar_amd import AMRPressureSolver
    for sw in SWITCHES:
        monkeypatch.delenv(sw, raising=False)
    monkeypatch.setenv("SOMAR_ORDERED_REDUCE_MAX", ORDERED_ALL)
    for sw, v in env.items():
        monkeypatch.setenv(sw, v)
    (dom, grids, dx, Jgup, Jinv), _ = _level(so, name)
    maxDepth, alpha, beta, full = LEVELS[name][5:]
    s = AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, p.imax, p.eps, maxDepth, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    b = params
    s.setBottomParameters(b.get("imax", p.bottom_imax), b.get("numRestarts", p.bottom_num_restarts), p.bottom_eps,
                          b.get("reps", p.bottom_reps), b.get("hang", p.bottom_hang), b.get("small", p.bottom_small),
                          b.get("normType", p.bottom_norm_type), 0)
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids], alpha=alpha, beta=beta)
    try:
        for q in range(s.num_local_patches):
            _, _, gi = s.patch_box(q)
            if full:
                s.setMetricFull(q, *[np.asfortranarray(Jgup[gi][d].a) for d in range(3)], np.asfortranarray(Jinv[gi].a[..., 0]))
            else:
                s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)],
                                 np.asfortranarray(Jinv[gi].a[..., 0]))
        s.finalize()
    except Exception:
        s.undefine()
        raise
    return s


def _bottom_fields(F, D):
    return (F.FIELD(D - 1, F.F_CORR), F.FIELD(D - 1, F.F_RES)) if D > 1 else (F.F_CORR, F.F_RES)


def _gpu_bottom(so, F, name, env, kind, params, rhs_kind, monkeypatch):
    """-> (iters, exit, solution) from a zero guess, and of a second solve on the same handle from that solution"""
    amr = _level(so, name)[1]
    D, bgrids = amr.mg.depth, amr.mg.ops[-1].grids
    fp, fr = _bottom_fields(F, D)
    gpu = _gpu(so, name, env, params, monkeypatch)
    try:
        assert gpu.depth() == D
        upload(gpu, fr, _bottom_rhs(so, name, rhs_kind), depth=D - 1)
        gpu.setVal(fp, 0.0)
        it, ex = gpu.bottomSolve(fp, fr)
        assert gpu.bottomKind() == kind
        first = (it, ex, download_valid(gpu, fp, bgrids, D - 1))
        it2, ex2 = gpu.bottomSolve(fp, fr)
        assert gpu.bottomKind() == kind
        return first, (it2, ex2, download_valid(gpu, fp, bgrids, D - 1))
    finally:
        gpu.undefine()


def _launch_bottom(so, F, name, params, rhs_kind, monkeypatch):
    key = (name, _key(params), rhs_kind)
    if key not in _LAUNCH:
        _LAUNCH[key] = _gpu_bottom(so, F, name, LAUNCH_ENV, 0, params, rhs_kind, monkeypatch)
    return _LAUNCH[key]


def _same(a_list, b_list):
    assert len(a_list) == len(b_list)
    for a, b in zip(a_list, b_list):
        np.testing.assert_array_equal(a, b)


def _check_shape(so, target):
    name, boxes, cells = TARGETS[target][:3]
    grids = _level(so, name)[1].mg.ops[-1].grids
    assert len(grids) == boxes and all(g.numPts() == cells for g in grids), [g.numPts() for g in grids]


def _three_sides(so, F, target, params, rhs_kind, monkeypatch):
    """the kernel against the oracle (first solve) and against the launch path (both solves), bit for bit -> the oracle's"""
    name, _, _, env, kind = TARGETS[target]
    _check_shape(so, target)
    want = _oracle_bottom(so, name, params, rhs_kind)
    first, again = _gpu_bottom(so, F, name, env, kind, params, rhs_kind, monkeypatch)
    lfirst, lagain = _launch_bottom(so, F, name, params, rhs_kind, monkeypatch)
    print(target, params, rhs_kind, "oracle", (want["iters"], want["exit"]), "restarts", want["restarts"], "kernel", first[:2],
          again[:2], "launch path", lfirst[:2], lagain[:2])
    assert first[:2] == (want["iters"], want["exit"])
    _same(first[2], want["sol"])
    assert lfirst[:2] == (want["iters"], want["exit"])
    _same(lfirst[2], want["sol"])
    assert again[:2] == lagain[:2]
    _same(again[2], lagain[2])
    return want


# ---- the branches: what the oracle must do for the case to be the one it is named after ----------------------------------------
def _exit3(numRestarts):
    def check(so, target, params, want):
        # two hung iterations in a row after numRestarts restarts: the early return
        assert want["exit"] == 3 and want["restarts"] == numRestarts == params["numRestarts"]
        assert want["iters"] >= 2 * (numRestarts + 1)
    return check


def _restart_then_converge(so, target, params, want):
    plain = _oracle_bottom(so, TARGETS[target][0], {})
    assert want["exit"] == 1 and want["restarts"] >= 1
    assert plain["exit"] == 1 and want["iters"] != plain["iters"]


def _iteration_limit(so, target, params, want):
    assert want["exit"] == -1 and want["iters"] == params["imax"]


def _small(so, target, params, want):
    # |m| <= small |rho| at once: r := 0, e never touched, the solution stays the zero guess
    assert (want["iters"], want["exit"], want["restarts"]) == (1, 1, 0) and want["applies"] == 1
    assert all(not a.any() for a in want["sol"])


def _reps_first_half_step(so, target, params, want):
    # the first half-step alone halves the residual: no second one, omega still 0, solution alpha * p~
    assert (want["iters"], want["exit"], want["restarts"]) == (1, 1, 0) and want["applies"] == 1
    assert any(a.any() for a in want["sol"])


def _reps_later(so, target, params, want):
    plain = _oracle_bottom(so, TARGETS[target][0], {})
    assert want["exit"] == 1 and 1 < want["iters"] < plain["iters"]


def _rho_zero(so, target, params, want):
    assert (want["iters"], want["exit"], want["restarts"]) == (1, 2, 0) and want["applies"] == 0
    assert all(not a.any() for a in want["sol"])


def _never_entered(so, target, params, want):
    assert (want["iters"], want["exit"], want["restarts"]) == (0, -1, 0) and want["applies"] == 0
    assert all(not a.any() for a in want["sol"])


def _converges(so, target, params, want):
    assert want["exit"] == 1


RESTARTS = {"T": dict(hang=0.6, numRestarts=5), "B1": dict(hang=0.6, numRestarts=5), "B2": dict(hang=0.2, numRestarts=20),
            "B4": dict(hang=0.2, numRestarts=5), "F": dict(hang=0.6, numRestarts=5)}
BRANCHES = []   # (id, target, BiCGStab parameters, right-hand side, the oracle-side check)
for tg in ALL:
    BRANCHES += [
        ("exit3-no-restart", tg, dict(hang=0.9, numRestarts=0), "random", _exit3(0)),
        ("exit3-after-a-restart", tg, dict(hang=0.9, numRestarts=1), "random", _exit3(1)),
        ("restart-then-converge", tg, RESTARTS[tg], "random", _restart_then_converge),
        ("imax-1", tg, dict(imax=1), "random", _iteration_limit),
        ("imax-%d" % (2 if tg == "F" else 3), tg, dict(imax=2 if tg == "F" else 3), "random", _iteration_limit),
        ("small", tg, dict(small=1e30), "random", _small),
        ("reps-0.5", tg, dict(reps=0.5), "random", _reps_first_half_step),
        ("rho-zero-max-norm", tg, dict(normType=0), "tiny", _rho_zero),
        ("rho-zero-one-norm", tg, dict(normType=1), "tiny", _rho_zero),
        ("zero-two-norm", tg, dict(normType=2), "tiny", _never_entered),
        ("zero-rhs", tg, {}, "zero", _never_entered),
    ]
    if tg != "F":
        BRANCHES.append(("reps-0.05", tg, dict(reps=0.05), "random", _reps_later))
    # (test_gpu_box_bottom.py::test_max_norm_and_one_norm_variants: 1024-cell boxes, a right-hand side outside the range)
    BRANCHES += [("max-norm", tg, dict(normType=0), "random", _converges), ("one-norm", tg, dict(normType=1), "random", _converges),
                 ("two-norm", tg, dict(normType=2), "random", _converges)]
for tg in ("T-helmholtz", "B1-helmholtz"):
    BRANCHES += [("deck", tg, {}, "random", _converges),
                 ("exit3-no-restart", tg, dict(hang=0.9, numRestarts=0), "random", _exit3(0))]


@pytest.mark.parametrize("target,params,rhs_kind,check", [b[1:] for b in BRANCHES], ids=["%s-%s" % (b[1], b[0]) for b in BRANCHES])
def test_bottom_kernel_branch_equals_the_oracle_and_the_launch_path(oracle, F, target, params, rhs_kind, check, monkeypatch):
    so = oracle
    _check_shape(so, target)
    check(so, target, params, _oracle_bottom(so, TARGETS[target][0], params, rhs_kind))
    _three_sides(so, F, target, params, rhs_kind, monkeypatch)


# ---- whole solves: the convergence metric in place of the bottom solver's initial norm ----------------------------------------
METRIC_PARAMS = [{}, dict(imax=2), dict(hang=0.9, numRestarts=0), dict(hang=0.9, numRestarts=1), dict(reps=0.3)]
_SOLVES, _KIND0 = {}, {}


def _oracle_solve(so, name, params):
    """the oracle's whole solve with so.BiCGStab(**params) at the bottom -> (iters, exit, history, [(iters, exit) of the
    bottom solve of every cycle]); right-hand side: random_field seed 12345 with its mean removed, on the 19-point level the
    operator applied to random_field seed 3"""
    key = (name, _key(params))
    if key not in _SOLVES:
        (dom, grids, dx, Jgup, Jinv), amr0 = _level(so, name)
        alpha, beta, full = LEVELS[name][6:]
        fac = so.Factory(dom, grids, dx, so.BCHolder(), Jgup, Jinv, alpha=alpha, beta=beta, isDiagonal=not full,
                         maxDepth=LEVELS[name][5])
        bs = so.BiCGStab(**params)
        amr = so.AMRMultiGrid(fac, bs)
        if full:
            rhs = so.LevelData(grids, 1)
            amr.op.apply_op(rhs, so.random_field(grids, 3, (1, 1, 1), dom.box), True)
        else:
            rhs = so.random_field(grids, 12345, (0, 0, 0), dom.box)
            so.remove_weighted_mean(rhs, Jinv)
        cycles = []
        solve = bs.solve

        def recorded(phi, r):
            solve(phi, r)
            cycles.append((bs.iters, bs.exitStatus))
        bs.solve = recorded
        phi = so.LevelData(grids, 1, (1, 1, 1))
        amr.solve(phi, rhs)
        _SOLVES[key] = (rhs, amr.iters, amr.exitStatus, list(amr.history), cycles)
    return _SOLVES[key]


def _gpu_solve(so, F, name, env, kind, params, monkeypatch):
    rhs = _oracle_solve(so, name, params)[0]
    grids = _level(so, name)[0][1]
    gpu = _gpu(so, name, env, params, monkeypatch)
    try:
        assert gpu.depth() == _level(so, name)[1].mg.depth
        upload(gpu, F.F_RHS, rhs)
        st = gpu.solveResident(True, False)
        assert gpu.bottomKind() == kind
        return st, download_valid(gpu, F.F_PHI, grids)
    finally:
        gpu.undefine()


def _check_solve(st, want):
    _, iters, exit_status, history, cycles = want
    assert st["iters"] == iters and st["exitStatus"] == exit_status, (st, iters, exit_status)
    assert (st["bottom_iters"], st["bottom_exit"]) == cycles[-1]
    np.testing.assert_allclose(st["history"], history, rtol=1e-10, atol=1e-10 * history[0])


def _check_restricted(params, cycles, last_converges=True):
    """the bottom solves of the first cycles leave where the parameters make them; the last one converges"""
    print(params, cycles)
    assert cycles[-1][1] == 1 or not last_converges
    if "imax" in params:
        assert sum(1 for it, ex in cycles if ex == -1 and it == params["imax"]) >= 3
    elif "hang" in params:
        assert sum(1 for it, ex in cycles if ex == 3) >= 3


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("params", METRIC_PARAMS, ids=lambda p: "-".join("%s%g" % kv for kv in sorted(p.items())) or "deck")
def test_solve_with_restricted_bottom_solves(oracle, F, params, kind, monkeypatch):
    """16^3 in boxes of 8, two levels deep: a bottom of 8 boxes of 4^3 under the convergence metric of a whole solve"""
    so = oracle
    name = "16^3-two-deep"
    amr = _level(so, name)[1]
    bgrids = amr.mg.ops[-1].grids
    assert amr.mg.depth == 2 and len(bgrids) == 8 and all(g.numPts() == 64 for g in bgrids)
    want = _oracle_solve(so, name, params)
    assert want[2] == 1 and len(want[4]) == want[1]
    _check_restricted(params, want[4])
    key = _key(params)
    if key not in _KIND0:
        _KIND0[key] = _gpu_solve(so, F, name, KIND_ENV[0], 0, params, monkeypatch)
    st0, sol0 = _KIND0[key]
    _check_solve(st0, want)
    if kind != 0:
        st, sol = _gpu_solve(so, F, name, KIND_ENV[kind], kind, params, monkeypatch)
        _check_solve(st, want)
        assert st["history"] == st0["history"]
        _same(sol, sol0)


def test_nineteen_point_solve_with_stagnating_bottom_solves(oracle, F, monkeypatch):
    so = oracle
    params = dict(hang=0.9, numRestarts=0)
    _check_shape(so, "F")
    want = _oracle_solve(so, "sheared", params)
    assert want[2] == 1
    _check_restricted(params, want[4], last_converges=False)     # (here every cycle's bottom solve stagnates)
    st0, sol0 = _gpu_solve(so, F, "sheared", LAUNCH_ENV, 0, params, monkeypatch)
    st, sol = _gpu_solve(so, F, "sheared", FULL_ENV, 2, params, monkeypatch)
    for s in (st0, st):
        _check_solve(s, want)
    assert st["history"] == st0["history"]
    _same(sol, sol0)


# ---- the deferred collect ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["T", "B1"])
def test_graph_cycle_around_an_early_return(oracle, F, target, monkeypatch):
    """test_gpu_bottom_local.py::test_graph_cycle_without_the_host_wait on the multi-box kernels, with a bottom solve that
    leaves through exit 3: vcycleFromZero captures, then replays, the coarse legs as graphs around the bottom kernel and
    reads its (iterations, exit code) only after the up leg is enqueued.  Same correction bit for bit without graphs, with
    the wait restored and on the launch path; bottomSolve afterwards reports what the launch path's reports."""
    so = oracle
    name, _, _, env, kind = TARGETS[target]
    params = dict(hang=0.9, numRestarts=0)
    _check_shape(so, target)
    assert _oracle_bottom(so, name, params)["exit"] == 3
    (dom, grids, dx, Jgup, Jinv), amr = _level(so, name)
    D, bgrids = amr.mg.depth, amr.mg.ops[-1].grids
    fp, fr = _bottom_fields(F, D)
    res = so.random_field(grids, 92, (0, 0, 0), dom.box)
    so.remove_weighted_mean(res, amr.op.Jinv)
    envs = {"graphs": env, "no graphs": dict(env, SOMAR_GRAPH_CELLS="0"), "wait restored": dict(env, SOMAR_BOTTOM_ASYNC="0"),
            "launch path": LAUNCH_ENV}
    got = {}
    for label, e in envs.items():
        gpu = _gpu(so, name, e, params, monkeypatch)
        try:
            upload(gpu, F.F_RES, res)
            gpu.vcycleFromZero(F.F_CORR, F.F_RES)
            k = gpu.bottomKind()
            corr = download_valid(gpu, F.F_CORR, grids)
            gpu.vcycleFromZero(F.F_CORR, F.F_RES)       # the replay (the first call captured the graphs)
            again = download_valid(gpu, F.F_CORR, grids)
            upload(gpu, fr, _bottom_rhs(so, name, "random"), depth=D - 1)
            gpu.setVal(fp, 0.0)
            got[label] = (k, corr, again, gpu.bottomSolve(fp, fr))
        finally:
            gpu.undefine()
    assert got["launch path"][0] == 0 and got["launch path"][3][1] == 3
    for label in envs:
        k, corr, again, status = got[label]
        assert k == (0 if label == "launch path" else kind), label
        _same(corr, got["launch path"][1])
        _same(again, got["launch path"][1])
        assert status == got["launch path"][3], label
