"""CPU side of the sharded mixed-precision cycle: the library builds for gfx950 and exports somar_solver_exchange_bytes, the
header declares it, and the Python binding knows it (tests/test_capi_exports.py then holds header and binding together).  The
fp32 pack / unpack kernels and the fp32 neighbour exchange are compiled in.  No GPU call is made."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from somar_amd import build
    path = build.build()
    assert os.path.exists(path)
    return path


def test_library_exports_exchange_bytes(built_lib):
    lib = C.CDLL(built_lib)
    assert hasattr(lib, "somar_solver_exchange_bytes")
    assert hasattr(lib, "somar_solver_exchange_bytes_depth")
    assert lib.somar_abi_version() == 13


def test_header_binding_and_python_method_name_it(built_lib):
    from somar_amd import AMRPressureSolver, api
    txt = open(os.path.join(ROOT, "include", "somar_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+somar_solver_exchange_bytes\s*\(\s*somar_solver_t\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*\)", txt)
    assert "somar_solver_exchange_bytes" in api.EXPORTS
    assert callable(getattr(AMRPressureSolver, "exchangeBytes"))
    # the signatures the issue pins
    assert re.search(r"\bint\s+somar_solver_set_precision\s*\(\s*somar_solver_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*long long\s+\w+\s*\)", txt)


def test_fp32_halo_kernels_are_compiled_in(built_lib):
    """the host stubs of the float pack / unpack instantiations (k_pack_items<PACK, float>) are in the library"""
    blob = open(built_lib, "rb").read()
    for pack in (b"Lb1E", b"Lb0E"):
        assert b"k_pack_itemsI" + pack + b"fE" in blob, pack
        assert b"k_pack_itemsI" + pack + b"dE" in blob, pack


def test_refusal_of_more_than_one_rank_is_gone():
    src = open(os.path.join(ROOT, "somar_amd", "csrc", "solver.cpp")).read()
    body = src[src.index("std::string PressureSolver::mixed_refusal() const"):]
    body = body[:body.index("\n}\n")]
    assert "comm_->size" not in body
    # the five refusals that stay
    for word in ("AMR hierarchy", "non-diagonal", "relax_mode", "num_mg", "coarse-fine"):
        assert word in body, word
