"""The oracle's tridiagonal restatement against the reference's own utils/ThomasAlgorithm.f90.
tests/golden/thomas_ref.npz holds seeded systems and the solutions that Fortran computed for them
(tests/golden/make_thomas_ref.py); where oracle/_ref is built (oracle/Makefile, flang), the live library is checked too."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, "..", "oracle", "_ref", "libthomas_ref.so")
GOLD = os.path.join(HERE, "golden", "thomas_ref.npz")


def test_tridiag_matches_reference_fortran(oracle):
    gold = np.load(GOLD)
    ref = C.CDLL(REF) if os.path.exists(REF) else None
    P = C.POINTER(C.c_double)
    for n in (3, 8, 64, 257):
        a, b, c, d = (gold[k + str(n)] for k in "abcd")
        x1, x2 = np.zeros(n), np.zeros(n)
        oracle.lib().orc_solve_tridiag(a.ctypes.data_as(P), b.ctypes.data_as(P), c.ctypes.data_as(P),
                                       d.ctypes.data_as(P), x1.ctypes.data_as(P), n)
        # flang may contract a*b+c into FMA; allow a few ulp
        np.testing.assert_allclose(x1, gold["x%d" % n], rtol=1e-14, atol=1e-16)
        if ref is not None:
            nn = C.c_int(n)
            ref.solve_tridiag_(a.ctypes.data_as(P), b.ctypes.data_as(P), c.ctypes.data_as(P),
                               d.ctypes.data_as(P), x2.ctypes.data_as(P), C.byref(nn))
            np.testing.assert_allclose(x1, x2, rtol=1e-14, atol=1e-16)
