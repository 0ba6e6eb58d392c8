#!/usr/bin/env python3
"""Regenerates tests/golden/thomas_ref.npz: seeded tridiagonal systems and their solutions computed by the REFERENCE's
own utils/ThomasAlgorithm.f90 (oracle/_ref/libthomas_ref.so, built by oracle/Makefile's `ref` target where the reference
sources and flang are present).  tests/test_oracle_ref.py checks the oracle's restatement against these stored solutions,
so the check runs on a checkout that has no reference build.

    python tests/golden/make_thomas_ref.py        # rewrites thomas_ref.npz
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, "..", "..", "oracle", "_ref", "libthomas_ref.so")
SIZES = (3, 8, 64, 257)


def systems():
    """-> [(a, b, c, d)] per size in SIZES: diagonally dominant, seeded (default_rng(9))"""
    rng = np.random.default_rng(9)
    out = []
    for n in SIZES:
        a = -rng.uniform(0.5, 1.0, n - 1)
        c = -rng.uniform(0.5, 1.0, n - 1)
        b = 2.5 + rng.uniform(0.0, 1.0, n)
        d = rng.uniform(-1, 1, n)
        out.append((a, b, c, d))
    return out


def solve_ref(ref, a, b, c, d):
    P = C.POINTER(C.c_double)
    x = np.zeros(len(b))
    nn = C.c_int(len(b))
    ref.solve_tridiag_(a.ctypes.data_as(P), b.ctypes.data_as(P), c.ctypes.data_as(P),
                       d.ctypes.data_as(P), x.ctypes.data_as(P), C.byref(nn))
    return x


def main():
    ref = C.CDLL(REF)
    out = {}
    for n, (a, b, c, d) in zip(SIZES, systems()):
        out.update({"a%d" % n: a, "b%d" % n: b, "c%d" % n: c, "d%d" % n: d, "x%d" % n: solve_ref(ref, a, b, c, d)})
    np.savez_compressed(os.path.join(HERE, "thomas_ref.npz"), **out)


if __name__ == "__main__":
    main()
