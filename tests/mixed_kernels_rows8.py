"""Child process of tests/test_gpu_mixed_kernels.py::test_8_row_kernels_in_a_child_process, run with SOMAR_FUSED_ROWS=8
(fused_rows() reads it once per process).  The 8-row fused sweep takes no narrow lane classes and no uniform-metric kernel.

1. The fp64 fused sweep bit for bit against the oracle's relax, 1-3 sweeps, on a stretched Neumann layout of 64-wide boxes
   and a Cartesian layout with Dirichlet sides.
2. The fp32 cycle against the oracle's one_cycle, per box, on the wide Cartesian (uniform-metric) case: with 8 rows its sweep
   streams the coefficient arrays, so mp_convert_metric must have made their fp32 copies.

Exits non-zero on the first failure; prints "rows8 ok" at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle import somar_oracle as so  # noqa: E402
from tests import test_gpu_mixed_kernels as T  # noqa: E402
from tests.helpers import download_valid, upload  # noqa: E402

# (name, n, box, variant, periodic, L, bc types)
SWEEP_LAYOUTS = [
    ("stretched-neumann", (64, 16, 8), (64, 8, 8), "stretched", (False, True, False), (2.0, 1.0, 0.5), None),
    ("cartesian-dirichlet", (64, 32, 16), 32, "cartesian", (False, False, False), (1.0, 0.5, 0.25), [T.D] * 6),
]


def sweep_bit_exact(layout):
    from somar_amd import api as F
    name, n, box, variant, periodic, L, bc = layout
    case = T.Case(name, n, box, variant, periodic, L, bc, 0.0, 1.0, None, 0, None, None, None)
    prob = T.problem(so, case)
    dom, grids, dx, Jgup, Jinv = prob
    fac = so.Factory(dom, grids, dx, T._bc_holder(so, case), Jgup, Jinv)
    op = so.AMRMultiGrid(fac, so.BiCGStab()).mg.ops[0]
    for sweeps in (1, 2, 3):
        s = T.gpu_solver(case, prob)
        try:
            phi = so.random_field(grids, 41, (1, 1, 1), dom.box)
            rhs = so.random_field(grids, 42, (0, 0, 0), dom.box)
            upload(s, F.F_PHI, phi)
            upload(s, F.F_RHS, rhs)
            op.relax(phi, rhs, sweeps)
            s.relax(0, F.F_PHI, F.F_RHS, sweeps)
            got = download_valid(s, F.F_PHI, grids)
        finally:
            s.undefine()
        for g, w in zip(got, [f.view(b)[..., 0] for b, f in zip(phi.grids, phi.fabs)]):
            np.testing.assert_array_equal(g, w)
        print("%s: fp64 fused sweep x%d bit-exact" % (name, sweeps))


def main():
    assert os.environ.get("SOMAR_FUSED_ROWS") == "8" and os.environ.get("SOMAR_FUSED_MIN_CELLS") == "0"
    so.lib()
    for layout in SWEEP_LAYOUTS:
        sweep_bit_exact(layout)
    case = next(c for c in T.CASES if c.name == "wide-cartesian")
    T.check_cycles(so, case)
    print("rows8 ok")


if __name__ == "__main__":
    main()
