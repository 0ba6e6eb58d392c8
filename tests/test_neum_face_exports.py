"""CPU-side checks of the interface of position-dependent Neumann values (somar_solver_set_neum_face_values): the entry
point is declared in the header with the signature of its Dirichlet twin, bound in api.EXPORTS and exported by the built
library; the header with it stays plain C99; the ABI version is still 13; the header cites the reference's lines; the
Python mirror has its method on the level solver class, which AMR level handles are instances of."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "somar_solver_set_neum_face_values"
TWIN = "somar_solver_set_bc_face_values"


@pytest.fixture(scope="module")
def built_lib():
    from somar_amd import build
    path = build.build()
    assert os.path.exists(path)
    return path


def _header():
    return open(os.path.join(ROOT, "include", "somar_amd.h")).read()


def test_entry_point_in_header_binding_and_library(built_lib):
    from somar_amd import api
    declared = set(re.findall(r"\b(somar_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    lib = C.CDLL(built_lib)
    assert NAME in declared
    assert NAME in api.EXPORTS
    assert hasattr(lib, NAME), "missing export " + NAME
    assert api.lib().somar_solver_set_neum_face_values.argtypes == api.lib().somar_solver_set_bc_face_values.argtypes
    assert lib.somar_abi_version() == 13   # an addition only
    assert callable(getattr(api.AMRPressureSolver, "setNeumFaceValues", None))
    assert callable(getattr(api.AMRPressureSolver, "setBCFaceValues", None))   # the Dirichlet call stays


def test_signature_matches_the_dirichlet_twin():
    txt = " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())

    def params(name):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        return [re.sub(r"\s*\b\w+$", "", p.strip()) for p in m.group(1).split(",")]   # types only

    assert params(NAME) == params(TWIN)


def test_header_with_the_entry_point_is_plain_c99(tmp_path):
    src = tmp_path / "abi_neum_face.c"
    src.write_text('#include "somar_amd.h"\ntypedef void (*fn)(void);\nint main(void) {\n    fn t[] = {(fn)%s};\n'
                   '    return sizeof(t) / sizeof(t[0]) != 1;\n}\n' % NAME)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_cites_the_reference_and_keeps_the_abi_version():
    txt = " ".join(_header().replace("*", " ").split())
    assert "EllipticBCUtils.cpp:696-947" in txt
    assert "EllipticBCUtils.cpp:842-843" in txt
    assert re.search(r"#define SOMAR_AMD_ABI_VERSION 13\b", _header())
