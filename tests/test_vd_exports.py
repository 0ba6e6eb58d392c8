"""CPU-side checks of the volume-discrepancy correction's interface (somar_amr_vd_correction and its pieces): the six entry
points are declared in the header, bound in api.EXPORTS and exported by the built library; the header with them stays plain
C99; the ABI version is still 13; the header cites the reference's lines and names the later-box-wins rule as unpinned; the
Python mirror has its six methods."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD_NAMES = ["somar_amr_vd_correction", "somar_amr_vd_rhs", "somar_amr_comp_gradient_mac", "somar_amr_average_down_faces",
            "somar_amr_vd_correction_host", "somar_amr_vd_correction_dev"]
VD_METHODS = ["vdCorrection", "vdRhs", "compGradientMAC", "averageDownFaces", "vdCorrectionHost", "vdCorrectionDev"]


@pytest.fixture(scope="module")
def built_lib():
    from somar_amd import build
    path = build.build()
    assert os.path.exists(path)
    return path


def _header():
    return open(os.path.join(ROOT, "include", "somar_amd.h")).read()


def test_entry_points_in_header_binding_and_library(built_lib):
    from somar_amd import api
    declared = set(re.findall(r"\b(somar_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    lib = C.CDLL(built_lib)
    for name in VD_NAMES:
        assert name in api.EXPORTS, name
        assert name in declared, name
        assert hasattr(lib, name), "missing export " + name
    assert lib.somar_abi_version() == 13   # additions only
    for m in VD_METHODS:
        assert callable(getattr(api.AMRPressureSolver, m, None)), m


def test_dev_signature_matches_the_host_twin():
    txt = " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())

    def params(name):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        return [re.sub(r"\s*\b\w+$", "", p.strip()) for p in m.group(1).split(",")]   # types only

    assert params("somar_amr_vd_correction_dev") == params("somar_amr_vd_correction_host")


def test_header_with_vd_entry_points_is_plain_c99(tmp_path):
    src = tmp_path / "abi_vd.c"
    table = ", ".join("(fn)%s" % name for name in VD_NAMES)
    src.write_text('#include "somar_amd.h"\ntypedef void (*fn)(void);\nint main(void) {\n    fn t[] = {%s};\n'
                   '    return sizeof(t) / sizeof(t[0]) != %d;\n}\n' % (table, len(VD_NAMES)))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_cites_the_reference_and_names_the_unpinned_rule():
    txt = " ".join(_header().replace("*", " ").split())
    assert "AMRNavierStokesSync.cpp:850-1060" in txt
    assert "MappedCoarseAverageF.ChF:182-237" in txt and "MappedCoarseAverage.cpp:400-520" in txt
    m = re.search(r"later-box-wins rule is UNPINNED against the reference", txt)
    assert m, "the header must name the later-box-wins rule as unpinned"
    assert "LATER in layout order wins, periodic images last" in txt
    assert re.search(r"#define SOMAR_AMD_ABI_VERSION 13\b", _header())
