"""CPU side of several components on a non-diagonal handle (somar_solver_set_components_full): the library builds for gfx950
and exports the entry point, the header declares it with the design's signature next to somar_solver_set_components,
api.EXPORTS and the Python method name it, the ABI version does not move (an addition), the header stays plain C99, the host
stubs of the N-field 19-point forms that ship (profiles/r14_multi_full19.md) are compiled in, and the class-0 tables the
batched depths get (PressureSolver::mc_setup: march_plan::full_nf_shape) cover the layouts of tests/test_gpu_multi_full.py the
way tests/test_march_plan.py checks the 7-point ones.  No GPU call is made."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "somar_amd", "csrc")
NAME = "somar_solver_set_components_full"


@pytest.fixture(scope="module")
def built_lib():
    from somar_amd import build
    path = build.build()
    assert os.path.exists(path)
    return path


def _header():
    return open(os.path.join(ROOT, "include", "somar_amd.h")).read()


def test_library_exports_it_and_the_abi_version_stays(built_lib):
    lib = C.CDLL(built_lib)
    assert hasattr(lib, NAME), "missing export " + NAME
    assert hasattr(lib, "somar_solver_set_components")
    assert lib.somar_abi_version() == 13   # an addition


def test_header_declares_it_next_to_set_components():
    txt = " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())
    pattern = r"\bint\s+%s\s*\(\s*somar_solver_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*long long\s+\w+\s*\)\s*;" % NAME
    assert re.search(pattern, txt), NAME
    assert re.search(r"int somar_solver_set_components\s*\([^)]*\)\s*;\s*int %s\s*\(" % NAME, txt)


def test_header_says_what_it_offers_and_what_stays_refused():
    txt = " ".join(_header().split())
    assert "AMRNavierStokesInit.cpp:887-1010" in txt and "m_viscSolverPtrs" in txt
    i = txt.index("somar_solver_set_components_full:")
    body = txt[i:txt.index("*/", i)]
    for words in ("NON-diagonal", "bit for bit", "COMPUTED", "profiles/r14_multi_full19.md", "diagonal metric",
                  "AMR hierarchy", "leptic", "relax_mode", "num_mg", "coarse-fine", "more than one rank", "metric update",
                  "somar_comp_set_op is refused", "fp32"):
        assert words in body, words
    assert "19-point operator" in txt   # where somar_solver_set_components lists what it does not offer


def test_binding_and_python_method_name_it(built_lib):
    from somar_amd import AMRPressureSolver, api
    assert NAME in api.EXPORTS
    assert callable(getattr(AMRPressureSolver, "setComponentsFull"))
    assert hasattr(api.lib(), NAME)


def test_header_with_the_new_entry_point_is_plain_c99(tmp_path):
    src = tmp_path / "abi_multi_full.c"
    src.write_text('#include "somar_amd.h"\ntypedef int (*fn)(somar_solver_t*, int, long long);\n'
                   'int main(void) {\n    fn f = %s;\n    return f == 0;\n}\n' % NAME)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_refusals_keep_their_words():
    src = open(os.path.join(CSRC, "solver_multi.cpp")).read()
    body = src[src.index("std::string PressureSolver::multi_refusal() const"):]
    body = body[:body.index("\n}\n")]
    assert "non-diagonal" in body
    full = src[src.index("void PressureSolver::set_components_full("):]
    full = full[:full.index("\n}\n")]
    assert "somar_solver_set_components" in full and "1 to 4" in full and "multi_refusal()" in full
    op = src[src.index("void PressureSolver::comp_set_op("):]
    assert "non-diagonal" in op[:op.index("\n}\n")]
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert "set_components_full: more than one component is not available for the handles of a leptic solver" in capi


# The forms of k_full_march_nf<MODE, FM_J, ZXY, NF> that ship, as profiles/r14_multi_full19.md records the choice
SHIPPED = [(mode, 8, zxy, 2) for mode in (0, 2) for zxy in (0, 1)]
# three fields at 6 rows: measured slower per field than the single-field kernel; at 8 rows: 192 KiB of LDS
DROPPED = [(mode, rows, zxy, 3) for mode in (0, 2) for rows in (6, 8) for zxy in (0, 1)]


def test_n_field_19_point_stubs_are_compiled_in(built_lib):
    blob = open(built_lib, "rb").read()
    for form in SHIPPED:
        assert b"k_full_march_nfILi%dELi%dELb%dELi%dE" % form in blob, form
    for form in DROPPED:
        assert b"k_full_march_nfILi%dELi%dELb%dELi%dE" % form not in blob, form
    for mode in (1, 3):   # the operator alone and the shell pass stay single-field
        assert b"k_full_march_nfILi%dE" % mode not in blob
    note = open(os.path.join(ROOT, "profiles", "r14_multi_full19.md")).read()
    for mode, rows, zxy, nf in SHIPPED:
        assert "k_full_march_nf<%d, %d, %s, %d>" % (mode, rows, "true" if zxy else "false", nf) in note


PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "march_plan.h"
using namespace somar::march_plan;
// ROWS N0 N1 N2 [N0 N1 N2 ...] -> "classes", then the eight ints of every tile of march_tiles(full_nf_shape(ROWS), boxes)
int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    std::vector<BoxSize> boxes;
    for (int a = 2; a + 2 < argc; a += 3) boxes.push_back({std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2])});
    const Table t = march_tiles(full_nf_shape(std::atoi(argv[1])), boxes);
    std::printf("%d\n", t.classes);
    for (const somar::Tile& q : t.tiles) std::printf("%d %d %d %d %d %d %d %d\n", q.patch, q.i0, q.j0, q.k0, q.nk, q.w, q.cls, q.slot);
    return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("full_nf_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(rows, boxes):
        out = subprocess.check_output([str(exe), str(rows)] + [str(n) for b in boxes for n in b], text=True).splitlines()
        return int(out[0]), [tuple(int(x) for x in line.split()) for line in out[1:]]
    return run


# depth-0 boxes of the layouts of tests/test_gpu_multi_full.py (and the second batched depth of `dirichlet`), with the columns
# (i0, w) per box width written out, not recomputed: 128 -> two columns of 64 where the level's own table holds 124 + 4
NFIELD_BOXES = {
    "seams": [(12, 8, 8)] * 4,
    "periodic": [(8, 8, 8)] * 8,
    "wide": [(128, 6, 4)],
    "dirichlet": [(16, 16, 16)] * 4,
    "dirichlet-depth-1": [(8, 8, 8)] * 4,
}
NFIELD_COLUMNS = {12: [(0, 12)], 8: [(0, 8)], 128: [(0, 64), (64, 64)], 16: [(0, 16)]}


@pytest.mark.parametrize("rows", [8])   # region rows of the two-field form: 6 tile rows
@pytest.mark.parametrize("layout", sorted(NFIELD_BOXES))
def test_tables_of_the_n_field_19_point_launches_are_class_0(planner, layout, rows):
    boxes = NFIELD_BOXES[layout]
    classes, tiles = planner(rows, boxes)
    assert classes == 0 and tiles
    cover = [np.zeros(b, dtype=np.int32) for b in boxes]
    for patch, i0, j0, k0, nk, w, cls, slot in tiles:
        n0, n1, n2 = boxes[patch]
        assert cls == 0 and slot == 0
        assert (i0, w) in NFIELD_COLUMNS[n0], (patch, i0, w)
        assert 0 <= i0 < n0 and 0 <= j0 < n1 and 0 <= k0 < n2 and nk > 0 and k0 + nk <= n2   # no empty tile, none past the box
        assert w <= 124 and i0 % 2 == 0 and j0 % (rows - 2) == 0
        cover[patch][i0:min(i0 + w, n0), j0:min(j0 + rows - 2, n1), k0:k0 + nk] += 1
    for patch, c in enumerate(cover):
        assert c.min() == 1 and c.max() == 1, (patch, int(c.min()), int(c.max()))
    for patch, (n0, _, _) in enumerate(boxes):
        assert sorted({(t[1], t[5]) for t in tiles if t[0] == patch}) == NFIELD_COLUMNS[n0]   # every column is there
    if layout == "wide":
        # what the layout is there for: the level's own 8-row table cuts 128 columns into 124 + 4 (narrow classes)
        from tests.helpers import march_columns
        assert march_columns(128, True) == [(124, 0), (4, 4)]
