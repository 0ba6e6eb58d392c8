"""CPU side of the multi-component level solve (somar_solver_set_components): the library builds for gfx950 and exports the
eight entry points, the header declares them with the signatures of the design, api.EXPORTS and the Python methods name them,
the N-field kernel stubs are compiled in, the header stays plain C, and the ABI version does not move (additions only).  No
GPU call is made."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, I, LL, PD, PI = r"somar_solver_t\s*\*\s*\w+", r"int\s+\w+", r"long long\s+\w+", r"double\s*\*\s*\w+", r"int\s*\*\s*\w+"
CPD, CPI, ST = r"const double\s*\*\s*\w+", r"const int\s*\*\s*\w+", r"somar_stats_t\s*\*\s*\w+"
SIGNATURES = {
    "somar_solver_set_components": [S, I, LL],
    "somar_solver_get_components": [S, PI, PI, r"long long\s*\*\s*\w+"],
    "somar_comp_upload": [S, I, I, I, CPD, CPI],       # comp, then somar_field_upload's arguments
    "somar_comp_download": [S, I, I, I, PD, CPI],      # comp, then somar_field_download's
    "somar_solver_solve_multi": [S, I, I, ST],
    "somar_vcycle_multi": [S, I],
    "somar_heat_step_multi": [S, I, r"double\s+\w+", I, ST],
    "somar_comp_history": [S, I, PD, I, PI],
}
METHODS = ["setComponents", "getComponents", "uploadComp", "downloadComp", "solveMulti", "vcycleMulti", "heatStepMulti",
           "compHistory"]


@pytest.fixture(scope="module")
def built_lib():
    from somar_amd import build
    path = build.build()
    assert os.path.exists(path)
    return path


def _header_text():
    txt = open(os.path.join(ROOT, "include", "somar_amd.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", txt, flags=re.S).split())


def test_library_exports_the_eight_names(built_lib):
    lib = C.CDLL(built_lib)
    assert len(SIGNATURES) == 8
    for name in SIGNATURES:
        assert hasattr(lib, name), "missing export " + name
    assert lib.somar_abi_version() == 13   # additions only


def test_header_declares_them_with_the_designs_signatures():
    txt = _header_text()
    for name, params in SIGNATURES.items():
        pattern = r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, r"\s*,\s*".join(params))
        assert re.search(pattern, txt), name
    # the component I/O takes a component, then exactly what the field I/O takes
    def types(name):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        return [re.sub(r"\s*\b\w+$", "", p.strip()) for p in m.group(1).split(",")]
    assert types("somar_comp_upload") == types("somar_field_upload")[:1] + ["int"] + types("somar_field_upload")[1:]
    assert types("somar_comp_download") == types("somar_field_download")[:1] + ["int"] + types("somar_field_download")[1:]


def test_header_states_the_reference_and_what_is_out_of_scope():
    txt = " ".join(open(os.path.join(ROOT, "include", "somar_amd.h")).read().split())
    assert "AMRNavierStokesInit.cpp:887-1010" in txt and "m_viscSolverPtrs" in txt
    for words in ("per-component Dirichlet values", "per-component BC types", "_dev twins", "sharded over ranks",
                  "19-point operator"):
        assert words in txt, words


def test_binding_and_python_methods_name_them(built_lib):
    from somar_amd import AMRPressureSolver, api
    for name in SIGNATURES:
        assert name in api.EXPORTS, name
    for m in METHODS:
        assert callable(getattr(AMRPressureSolver, m)), m


def test_n_field_kernel_stubs_are_compiled_in(built_lib):
    """the host stubs of the N-field sweep (plain on 2 fields, from zero on 2 and 3; with and without Dirichlet sides), of
    the residual (2 and 3 fields) and of the residual + restriction (2 fields) are in the library -- and the forms that
    measured slower than the single-field kernels (plain on 3 fields, the folded prolongation) are not"""
    blob = open(built_lib, "rb").read()
    one = b"NS_13StencilParamsEEE"   # the operator carrier (the kernels' last template argument): one for all fields
    for mode, nf in ((0, 2), (1, 2), (1, 3)):
        for diri in (0, 1):
            assert b"k_gsrb_fused_nfILi%dELb%dELi%dE" % (mode, diri, nf) + one in blob, (mode, diri, nf)
    for nf in (2, 3):
        assert b"k_resid_march_nfILi0ELi%dE" % nf + one in blob, nf
    assert b"k_resid_march_nfILi2ELi2E" + one in blob
    assert b"k_gsrb_fused_nfILi3E" not in blob and b"k_gsrb_fused_nfILi0ELb0ELi3E" + one not in blob
    assert b"k_resid_march_nfILi2ELi3E" + one not in blob


def test_header_with_the_new_entry_points_is_plain_c(tmp_path):
    src = tmp_path / "abi_multi.c"
    table = ", ".join("(fn)%s" % name for name in SIGNATURES)
    src.write_text('#include "somar_amd.h"\ntypedef void (*fn)(void);\nint main(void) {\n    fn t[] = {%s};\n'
                   '    return sizeof(t) / sizeof(t[0]) != 8;\n}\n' % table)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_refusals_name_their_reason():
    src = open(os.path.join(ROOT, "somar_amd", "csrc", "solver_multi.cpp")).read()
    body = src[src.index("std::string PressureSolver::multi_refusal() const"):]
    body = body[:body.index("\n}\n")]
    for word in ("AMR hierarchy", "non-diagonal", "relax_mode", "num_mg", "coarse-fine", "more than one rank", "set_precision"):
        assert word in body, word
    capi = open(os.path.join(ROOT, "somar_amd", "csrc", "capi.cpp")).read()
    assert "set_components: more than one component is not available for the handles of a leptic solver" in capi
