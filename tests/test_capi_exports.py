"""CPU-side checks of the drop-in boundary: the shared library builds for gfx950, loads, and exports
exactly the entry points include/somar_amd.h declares.  No compute call is made (no GPU here)."""
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


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "somar_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(somar_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_binding_agree(built_lib):
    from somar_amd import api
    assert _header_functions() == api.EXPORTS


def test_library_exports_every_declared_symbol(built_lib):
    lib = C.CDLL(built_lib)
    for name in _header_functions():
        assert hasattr(lib, name), "missing export " + name
    assert lib.somar_abi_version() == 13


def test_no_cpu_fallback_without_gpu(built_lib):
    """On a box without a GPU the product must fail loudly, not compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from somar_amd import AMRPressureSolver, SomarError
    s = AMRPressureSolver()
    with pytest.raises(SomarError):
        s.define((0, 0, 0), (7, 7, 7), (0, 0, 0), (1.0, 1.0, 1.0), [((0, 0, 0), (7, 7, 7))])


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "somar_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "liboracle" not in src, f


def test_header_is_plain_c(tmp_path):
    """the boundary is a C ABI: include/somar_amd.h must compile as C99 on its own (no C++-isms, no torch/HIP types)"""
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text('#include "somar_amd.h"\nint main(void) { int (*f)(void) = somar_abi_version; return f == 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def _header_defines(prefix):
    txt = open(os.path.join(ROOT, "include", "somar_amd.h")).read()
    return {m[0]: int(m[1]) for m in re.findall(r"^#define\s+(%s[A-Z_]+)\s+\(?(-?\d+)\)?\s*$" % prefix, txt, flags=re.M)}


def _solver_h_enum(first):
    txt = open(os.path.join(ROOT, "somar_amd", "csrc", "solver.h")).read()
    body = re.search(r"enum\s*\{\s*(%s\b[^}]*)\}" % first, txt).group(1)
    return {k: int(v) for k, v in re.findall(r"\b([A-Z_]+)\s*=\s*(-?\d+)", body)}


def test_relax_and_precond_codes_match_the_reference():
    """The header's relax_mode / precond_mode codes are the ones the input files use, utils/ProblemContext.H:322-340
    (PrecondMode: None = -1, DiagRelax = 0, DiagLineRelax = 1; RelaxMode: JACOBI = 0, LEVEL_GSRB = 1, LOOSE_GSRB = 2,
    LINE_GSRB = 3), and the ones the solver compares against (solver.h)."""
    reference = {"RELAX_JACOBI": 0, "RELAX_LEVEL_GSRB": 1, "RELAX_LOOSE_GSRB": 2, "RELAX_LINE_GSRB": 3,
                 "PRECOND_NONE": -1, "PRECOND_DIAG_RELAX": 0, "PRECOND_DIAG_LINE_RELAX": 1}
    header = {k[len("SOMAR_"):]: v for k, v in {**_header_defines("SOMAR_RELAX_"), **_header_defines("SOMAR_PRECOND_")}.items()}
    assert header == reference
    assert {**_solver_h_enum("RELAX_JACOBI"), **_solver_h_enum("PRECOND_NONE")} == reference


def _csrc_sources():
    d = os.path.join(ROOT, "somar_amd", "csrc")
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith((".cpp", ".h", ".hip"))}


def test_device_memory_has_one_owner():
    """csrc/devbuf.h is the only place that allocates or frees device memory (the stand-alone probes under tools/ are their
    own programs); the hand-written upload / free helpers it replaced stay gone, and no destructor names a device buffer --
    DevBuf members release themselves"""
    srcs = _csrc_sources()
    assert "devbuf.h" in srcs
    for f, txt in srcs.items():
        if f != "devbuf.h":
            for call in ("hipMalloc(", "hipMallocAsync(", "hipFree(", "hipFreeAsync("):
                assert call not in txt, "%s calls %s" % (f, call)
        for gone in ("free_field", "free_program", "table_to_device", "to_device"):
            assert not re.search(r"\b%s\b" % gone, txt), "%s still has %s" % (f, gone)
    # every buffer member: declared as DevBuf<...> name[, name...] in a header
    members = set()
    for f, txt in srcs.items():
        if f.endswith(".h"):
            for decl in re.findall(r"^\s*(?:std::vector<)?DevBuf<[^;()]*?>+\s+([^;()]+);", txt, flags=re.M):
                members.update(re.findall(r"\b([A-Za-z_]\w*)\b(?:\[\d+\])*\s*(?:,|$)", decl))
    assert {"f_phi", "d_patches", "jinv", "d_ordbuf_", "buf", "d_avg", "d_sbuf"} <= members
    ndtor = 0
    for f, txt in srcs.items():
        if f == "devbuf.h" or f.endswith(".hip"):
            continue
        for m in re.finditer(r"~\w+\(\)[^;{]*\{", txt):
            depth, i = 1, m.end()
            while depth:
                depth += {"{": 1, "}": -1}.get(txt[i], 0)
                i += 1
            body = txt[m.end():i - 1]
            ndtor += 1
            named = sorted(set(re.findall(r"\b\w+\b", body)) & members)
            assert not named, "%s: %s names %s" % (f, m.group(0), named)
    assert ndtor >= 4
