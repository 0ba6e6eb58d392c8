"""The execution-path switches (SOMAR_* variables) are read when a solver is created and hold for its life:
somar_solver_tuning reports what a solver holds.  Two solvers of one process created under different environments each keep
their own values -- the case the per-process `static` reads of earlier versions got wrong, where whichever solver came first
decided for all -- and a variable changed after creation changes nothing for the solver: not at finalize, not at a metric
refresh.  All on one 8^3 box (the smallest level that finalizes)."""
import os
import re

import numpy as np
import pytest

from helpers import download_valid, make_problem, upload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name without SOMAR_, default, a non-default setting, what a solver created under it reports); the rows and their order are
# those of the table of DESIGN.md 8.9 and of SWITCHES in csrc/tuning.cpp.  Presence switches are on whatever the text ("0" too).
SWITCHES = [
    ("FUSED_MIN_CELLS", 262144, "0", 0),
    ("MARCH_MIN_CELLS", 262144, "0", 0),
    ("FUSED_ROWS", 16, "8", 8),
    ("FULL_ROWS", 8, "6", 6),
    ("NO_BALANCED_TILES", 0, "0", 1),
    ("NO_NARROW_TILES", 0, "1", 1),
    ("NARROW_7PT", -1, "0", 0),
    ("NO_LEAN_TILES", 0, "1", 1),
    ("NO_UNIFORM", 0, "1", 1),
    ("NO_ZERO_PLANES", 0, "1", 1),
    ("NO_ZERO_START", 0, "1", 1),
    ("NO_FOLD_PROLONG", 0, "0", 1),
    ("NO_CF_FUSED", 0, "1", 1),
    ("AMR_PLAIN", 0, "1", 1),
    ("FUSED_BOTTOM_MAX_CELLS", 512, "0", 0),
    ("BOX_BOTTOM", 1, "0", 0),
    ("BOX_BOTTOM_MIN_CELLS", 513, "100", 100),
    ("BOX_TIMING", 0, "1", 1),
    ("BOTTOM_ASYNC", 1, "0", 0),
    ("ORDERED_REDUCE_MAX", 4096, "100000", 100000),
    ("ORDERED_SERIAL", 0, "1", 1),
    ("NO_FUSED_PUBLISH", 0, "1", 1),
    ("POLL_FETCH", 1, "0", 0),
    ("GHOST_STAGED", 0, "1", 1),
    ("NO_GHOST_DCE", 0, "1", 1),
    ("FLUX_FIELDS", 0, "1", 1),
    ("FUSED19_MIN_BOX", -1, "0", 0),
    ("CF_FULL_GATHER", 0, "1", 1),
    ("PULL_MAX_CELLS", 262144, "0", 0),
    ("GRAPH_CELLS", 262144, "0", 0),
    ("AGGLOM_CELLS", 2097152, "0", 0),
    ("NO_OVERLAP", 0, "1", 1),
    ("TIMING", 0, "2", 2),
]
NAMES = [s[0] for s in SWITCHES]


def test_switch_list_is_the_documented_one():
    """DESIGN.md's table, tuning.cpp's table and the list above: the same switches in the same order, the same defaults"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    rows = re.findall(r"^\| `SOMAR_([A-Z0-9_]+)` \| `?(-?\d+)`?[^|]*\|", design, flags=re.M)
    assert [(n, int(d)) for n, d in rows] == [(s[0], s[1]) for s in SWITCHES]
    src = open(os.path.join(ROOT, "somar_amd", "csrc", "tuning.cpp")).read()
    assert re.findall(r'^    \{"([A-Z0-9_]+)", &Tuning::', src, flags=re.M) == NAMES
    assert "values are fixed when a solver is created" in design


@pytest.fixture
def clean_env(monkeypatch):
    for name in NAMES:
        monkeypatch.delenv("SOMAR_" + name, raising=False)
    return monkeypatch


def _create(prob):
    from somar_amd import AMRPressureSolver
    dom, grids, dx, Jgup, Jinv = prob
    s = AMRPressureSolver()
    s.define(dom.box.lo, dom.box.hi, dom.periodic, dx, [(g.lo, g.hi) for g in grids])
    return s


def _set_metric(s, prob):
    Jgup, Jinv = prob[3], prob[4]
    for q in range(s.num_local_patches):
        _, _, gi = s.patch_box(q)
        s.setMetricOrtho(q, *[np.asfortranarray(Jgup[gi][d].a[..., d]) for d in range(3)], np.asfortranarray(Jinv[gi].a[..., 0]))


def _solver(prob):
    s = _create(prob)
    _set_metric(s, prob)
    s.finalize()
    return s


@pytest.fixture(scope="module")
def box8(oracle):
    return make_problem(oracle, (8, 8, 8), 8, "stretched")


@pytest.fixture(scope="module")
def box8_cartesian(oracle):
    return make_problem(oracle, (8, 8, 8), 8, "cartesian")


@pytest.mark.gpu
@pytest.mark.parametrize("name,default,text,want", SWITCHES, ids=NAMES)
def test_two_solvers_of_one_process_hold_their_own_values(box8, clean_env, name, default, text, want):
    a = _solver(box8)
    try:
        assert a.tuning(name) == default
        clean_env.setenv("SOMAR_" + name, text)
        b = _solver(box8)
        try:
            assert b.tuning(name) == want
            assert a.tuning(name) == default   # (a process-wide read would have answered for both)
            for other, d, _, _ in SWITCHES:
                if other != name and not (other == "MARCH_MIN_CELLS" and name == "FUSED_MIN_CELLS"):
                    assert b.tuning(other) == d, other
        finally:
            b.undefine()
    finally:
        a.undefine()


@pytest.mark.gpu
def test_march_min_cells_follows_fused_min_cells_when_unset(box8, clean_env):
    clean_env.setenv("SOMAR_FUSED_MIN_CELLS", "1000")
    s = _create(box8)
    try:
        assert (s.tuning("FUSED_MIN_CELLS"), s.tuning("MARCH_MIN_CELLS")) == (1000, 1000)
    finally:
        s.undefine()


@pytest.mark.gpu
def test_unknown_switch_is_an_error(box8, clean_env):
    from somar_amd import SomarError
    s = _create(box8)
    try:
        with pytest.raises(SomarError):
            s.tuning("NO_SUCH_SWITCH")
        with pytest.raises(SomarError):
            s.tuning("SOMAR_FUSED_ROWS")   # the name goes without its prefix
    finally:
        s.undefine()


@pytest.mark.gpu
def test_a_variable_changed_after_creation_changes_nothing(box8_cartesian, clean_env):
    """SOMAR_NO_UNIFORM set between create and finalize, then (another solver) between finalize and a metric refresh: the
    solver keeps its creation-time value, and its behaviour -- a Cartesian metric is still found uniform"""
    prob = box8_cartesian
    s = _create(prob)
    try:
        clean_env.setenv("SOMAR_NO_UNIFORM", "1")
        _set_metric(s, prob)
        s.finalize()
        assert s.tuning("NO_UNIFORM") == 0
        assert s.metricUniform(0) is not None
    finally:
        s.undefine()
    clean_env.delenv("SOMAR_NO_UNIFORM")
    s = _solver(prob)
    try:
        uni = s.metricUniform(0)
        assert uni is not None
        clean_env.setenv("SOMAR_NO_UNIFORM", "1")
        clean_env.setenv("SOMAR_NARROW_7PT", "0")
        with s.metricUpdate():
            _set_metric(s, prob)
        assert (s.tuning("NO_UNIFORM"), s.tuning("NARROW_7PT")) == (0, -1)
        assert s.metricUniform(0) == uni
        off = _solver(prob)   # (a solver created now does hold the new value)
        try:
            assert off.tuning("NO_UNIFORM") == 1 and off.metricUniform(0) is None
        finally:
            off.undefine()
    finally:
        s.undefine()


@pytest.mark.gpu
def test_poll_fetch_decides_per_solver_how_the_bottom_runs(oracle, box8, clean_env):
    """SOMAR_POLL_FETCH was read once per process: a default solver runs the one-box bottom as one launch (kind 2, as
    tests/test_gpu_bottom_local.py expects for one box), a solver created under SOMAR_POLL_FETCH=0 launch by launch (kind 0),
    a third created with the variable unset as the first again -- and the three corrections of one V-cycle are the same bits"""
    from somar_amd import api as F
    so = oracle
    dom, grids, dx, Jgup, Jinv = box8
    res = so.random_field(grids, 92, (0, 0, 0), dom.box)
    so.remove_weighted_mean(res, Jinv)
    solvers, kinds, corr = [], [], []
    try:
        for poll in (None, "0", None):
            if poll is None:
                clean_env.delenv("SOMAR_POLL_FETCH", raising=False)
            else:
                clean_env.setenv("SOMAR_POLL_FETCH", poll)
            solvers.append(_solver(box8))
        for s in solvers:   # (all three exist before the first one runs)
            upload(s, F.F_RES, res)
            s.setVal(F.F_CORR, 0.0)
            s.vcycle(F.F_CORR, F.F_RES)
            kinds.append(s.bottomKind())
            corr.append(download_valid(s, F.F_CORR, grids))
        assert [s.tuning("POLL_FETCH") for s in solvers] == [1, 0, 1]
        assert kinds == [2, 0, 2]
        for c in corr[1:]:
            for x, y in zip(c, corr[0]):
                np.testing.assert_array_equal(x, y)
        assert float(np.max(np.abs(corr[0][0]))) > 0.0
    finally:
        for s in solvers:
            s.undefine()
