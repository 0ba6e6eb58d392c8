"""CPU side of the per-component operators (somar_comp_set_op): the library exports the four entry points, the header declares
them with the signatures of the design and stays plain C, api.EXPORTS and the Python methods name them, the ABI version does
not move (additions only), and the per-operator kernel stubs are compiled in -- for the launch shapes of the shared-operator
kernels, no others.  No GPU call is made."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, I, PD, PI = r"somar_solver_t\s*\*\s*\w+", r"int\s+\w+", r"double\s*\*\s*\w+", r"int\s*\*\s*\w+"
CPD, CPI, DBL = r"const double\s*\*\s*\w+", r"const int\s*\*\s*\w+", r"double\s+\w+"
SIGNATURES = {
    "somar_comp_set_op": [S, I, CPI, CPD, DBL, DBL],
    "somar_comp_get_op": [S, I, PI, PD, PD, PD, PI],
    "somar_comp_reset_op": [S, I],
    "somar_solver_get_op_launches": [S, r"long long\s*\*\s*\w+"],
}
METHODS = ["setCompOp", "getCompOp", "resetCompOp", "opLaunches"]


@pytest.fixture(scope="module")
def built_lib():
    from somar_amd import build
    path = build.build()
    assert os.path.exists(path)
    return path


def _header_text():
    txt = open(os.path.join(ROOT, "include", "somar_amd.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", txt, flags=re.S).split())


def test_library_exports_the_four_names(built_lib):
    lib = C.CDLL(built_lib)
    for name in SIGNATURES:
        assert hasattr(lib, name), "missing export " + name
    assert lib.somar_abi_version() == 13   # additions only


def test_header_declares_them_with_the_designs_signatures():
    txt = _header_text()
    for name, params in SIGNATURES.items():
        pattern = r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, r"\s*,\s*".join(params))
        assert re.search(pattern, txt), name


def test_header_points_at_the_new_entry_for_what_was_not_offered():
    txt = " ".join(open(os.path.join(ROOT, "include", "somar_amd.h")).read().split())
    block = txt[txt.index("Several right-hand sides in one level solve"):txt.index("int somar_solver_set_components")]
    assert "Through somar_comp_set_op" in block
    offered, rest = block[block.index("Through somar_comp_set_op"):].split("Not offered (yet)")
    assert "per-component Dirichlet values" in offered and "per-component BC types" in offered
    assert "face-valued Dirichlet sides per component" in rest


def test_binding_and_python_methods_name_them(built_lib):
    from somar_amd import AMRPressureSolver, api
    for name in SIGNATURES:
        assert name in api.EXPORTS, name
    for m in METHODS:
        assert callable(getattr(AMRPressureSolver, m)), m


def test_per_operator_kernel_stubs_are_compiled_in(built_lib):
    """the sweep plain on 2 fields and from zero on 2 and 3 (with and without Dirichlet sides), the residual on 2 and 3 and the
    residual + restriction on 2: the shapes of the shared-operator kernels, and none of the shapes those left out"""
    blob = open(built_lib, "rb").read()
    per = b"NS_8FieldOpsILi%dEEEEE"   # the operator carrier (the kernels' last template argument): one per field
    for mode, nf in ((0, 2), (1, 2), (1, 3)):
        for diri in (0, 1):
            assert b"k_gsrb_fused_nfILi%dELb%dELi%dE" % (mode, diri, nf) + per % nf in blob, (mode, diri, nf)
    for nf in (2, 3):
        assert b"k_resid_march_nfILi0ELi%dE" % nf + per % nf in blob, nf
    assert b"k_resid_march_nfILi2ELi2E" + per % 2 in blob
    assert b"k_gsrb_fused_nfILi3E" not in blob and b"k_gsrb_fused_nfILi0ELb0ELi3E" + per % 3 not in blob
    assert b"k_resid_march_nfILi2ELi3E" + per % 3 not in blob
    assert b"k_gsrb_fused_nfo" not in blob and b"k_resid_march_nfo" not in blob   # (the separate per-operator texts are gone)


def test_header_with_the_new_entry_points_is_plain_c(tmp_path):
    src = tmp_path / "abi_multi_ops.c"
    table = ", ".join("(fn)%s" % name for name in SIGNATURES)
    src.write_text('#include "somar_amd.h"\ntypedef void (*fn)(void);\nint main(void) {\n    fn t[] = {%s};\n'
                   '    return sizeof(t) / sizeof(t[0]) != 4;\n}\n' % table)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])
