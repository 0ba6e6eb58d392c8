"""The per-cell arithmetic of the 19-point kernels (somar_amd/csrc/full19_point.h, whose statements are full19_point.inc) from
a stand-alone host program: the header is plain C++ without a HIP include, so the program below calls its three functions on
one small box and holds every result, by memcmp of the doubles, against the repository's own restatement of the reference
kernels, oracle/kernels.c, linked into the same program:

  full19_gsrb_interior  against orc_gsrbiter3d with lapDiag from orc_fillmappedlapdiag3d, every cell, both colours, in both
                        forms: lapDiag recomputed from the coefficients, and a perturbed array handed over to both;
  full19_gsrb_boundary  against orc_gsrbboundaryiter3d, every cell, both colours, each of the 64 `stencil` masks;
  full19_op             against orc_mappedgetflux + (boundary fluxes zeroed) + flux *= beta + orc_mappedfluxdivergence3d +
                        orc_axbyip, every cell, for alpha = 0 and alpha != 0 and the flag sets all-clear, all-set and one face
                        each (a set flag zeroes the fluxes on that face of the BOX, as a Neumann domain face does).

6 x 5 x 4 cells with a one-cell frame; phi, a DIFFERENT extrap array, rhs, the nine J g^{ab} planes and 1 / J filled with fixed
pseudo-random values (diagonals and 1 / J positive); alpha = 0.7, beta = -0.3, dx unequal per direction.  The program is built
a second time with -fsanitize=address,undefined and run once more."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "somar_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "full19_point.h"
using namespace somar;

extern "C" {
void orc_gsrbiter3d(double*, const int*, const int*, int, const double*, const int*, const int*, const double*, const int*,
                    const int*, const double*, const int*, const int*, const double*, const int*, const int*, const double*,
                    const int*, const int*, const double*, const int*, const int*, const double*, const int*, const int*,
                    const int*, const int*, const double*, double, double, int);
void orc_gsrbboundaryiter3d(double*, const int*, const int*, int, const double*, const int*, const int*, const double*,
                            const int*, const int*, const double*, const int*, const int*, const double*, const int*,
                            const int*, const double*, const int*, const int*, const double*, const int*, const int*,
                            const int*, const int*, const double*, double, double, const int*, int);
void orc_fillmappedlapdiag3d(double*, const int*, const int*, const double*, const int*, const int*, const double*, const int*,
                             const int*, const double*, const int*, const int*, const double*, const int*, const int*,
                             const int*, const int*, const double*);
void orc_mappedgetflux(double*, const int*, const int*, int, const double*, const int*, const int*, const double*, const int*,
                       const int*, const double*, const int*, const int*, const int*, const int*, double, const double*, int);
void orc_mappedfluxdivergence3d(double*, const int*, const int*, int, const double*, const int*, const int*, const double*,
                                const int*, const int*, const double*, const int*, const int*, const double*, const int*,
                                const int*, const int*, const int*, const double*);
void orc_axbyip(double*, const int*, const int*, int, const double*, const int*, const int*, double, double, const int*,
                const int*);
}

// a Fortran-ordered array over the inclusive box [lo, hi] with nc components
struct Fab {
    int lo[3], hi[3], nc;
    std::vector<double> v;
    Fab(const int* l, const int* h, int ncomp) : nc(ncomp)
    {
        for (int d = 0; d < 3; ++d) { lo[d] = l[d]; hi[d] = h[d]; }
        v.assign(size() * nc, 0.0);
    }
    size_t size() const { return (size_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1); }
    double& at(int i, int j, int k, int n = 0)
    {
        const size_t n0 = hi[0] - lo[0] + 1, n1 = hi[1] - lo[1] + 1;
        return v[(size_t)(i - lo[0]) + n0 * ((size_t)(j - lo[1]) + n1 * (size_t)(k - lo[2])) + size() * n];
    }
    double* comp(int n) { return v.data() + size() * n; }
};

static unsigned long long seed = 0x9E3779B97F4A7C15ull;
static double rnd()   // in (-1, 1), fixed sequence
{
    seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
    return (double)(seed >> 11) / 4503599627370496.0 - 1.0;
}
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    const int vlo[3] = {0, 0, 0}, vhi[3] = {5, 4, 3};          // 6 x 5 x 4 cells
    const int flo[3] = {-1, -1, -1}, fhi[3] = {6, 5, 4};       // with the one-cell frame
    const double dx[3] = {0.37, 0.21, 0.53};
    const double alpha = 0.7, beta = -0.3;
    Fab phi(flo, fhi, 1), ext(flo, fhi, 1), rhs(vlo, vhi, 1), jinv(vlo, vhi, 1), lapd(vlo, vhi, 1);
    for (double& x : phi.v) x = rnd();
    for (double& x : ext.v) x = rnd();
    for (double& x : rhs.v) x = rnd();
    for (double& x : jinv.v) x = 1.5 + 0.5 * rnd();
    std::vector<Fab> jg;
    for (int d = 0; d < 3; ++d) {
        int h[3] = {vhi[0], vhi[1], vhi[2]};
        h[d] += 1;
        jg.emplace_back(vlo, h, 3);
        for (int n = 0; n < 3; ++n)
            for (size_t q = 0; q < jg[d].size(); ++q) jg[d].comp(n)[q] = (n == d) ? 1.5 + 0.5 * rnd() : 0.4 * rnd();
    }
    orc_fillmappedlapdiag3d(lapd.v.data(), lapd.lo, lapd.hi, jg[0].v.data(), jg[0].lo, jg[0].hi, jg[1].v.data(), jg[1].lo, jg[1].hi,
                            jg[2].v.data(), jg[2].lo, jg[2].hi, jinv.v.data(), jinv.lo, jinv.hi, vlo, vhi, dx);

    Fab lapd2 = lapd;
    for (double& x : lapd2.v) x *= 1.0 + 0.25 * rnd();

    const Full19Scales S = full19_scales(dx[0], dx[1], dx[2]);
    auto coef = [&](int i, int j, int k) {
        Full19Coef C;
        C.x0l = jg[0].at(i, j, k, 0); C.x0h = jg[0].at(i + 1, j, k, 0);
        C.x1l = jg[0].at(i, j, k, 1); C.x1h = jg[0].at(i + 1, j, k, 1);
        C.x2l = jg[0].at(i, j, k, 2); C.x2h = jg[0].at(i + 1, j, k, 2);
        C.y0l = jg[1].at(i, j, k, 0); C.y0h = jg[1].at(i, j + 1, k, 0);
        C.y1l = jg[1].at(i, j, k, 1); C.y1h = jg[1].at(i, j + 1, k, 1);
        C.y2l = jg[1].at(i, j, k, 2); C.y2h = jg[1].at(i, j + 1, k, 2);
        C.z0l = jg[2].at(i, j, k, 0); C.z0h = jg[2].at(i, j, k + 1, 0);
        C.z1l = jg[2].at(i, j, k, 1); C.z1h = jg[2].at(i, j, k + 1, 1);
        C.z2l = jg[2].at(i, j, k, 2); C.z2h = jg[2].at(i, j, k + 1, 2);
        C.ji = jinv.at(i, j, k);
        return C;
    };
    long checked = 0, bad = 0;
    auto check = [&](const char* what, int a, int b, int i, int j, int k, double got, double want) {
        ++checked;
        if (same(got, want)) return;
        if (++bad <= 10) std::printf("MISMATCH %s %d %d cell %d %d %d: %a != %a\n", what, a, b, i, j, k, got, want);
    };
#define CELLS for (int k = vlo[2]; k <= vhi[2]; ++k) for (int j = vlo[1]; j <= vhi[1]; ++j) for (int i = vlo[0]; i <= vhi[0]; ++i)

    // ---- the two GSRB updates, both colours ----
    for (int rb = 0; rb < 2; ++rb) {
        Fab out = phi;
        orc_gsrbiter3d(out.v.data(), out.lo, out.hi, 1, ext.v.data(), ext.lo, ext.hi, rhs.v.data(), rhs.lo, rhs.hi,
                       jg[0].v.data(), jg[0].lo, jg[0].hi, jg[1].v.data(), jg[1].lo, jg[1].hi, jg[2].v.data(), jg[2].lo, jg[2].hi,
                       jinv.v.data(), jinv.lo, jinv.hi, lapd.v.data(), lapd.lo, lapd.hi, vlo, vhi, dx, alpha, beta, rb);
        // the same with a lapDiag array that is NOT the expression's value, as k_gsrb_full may be handed one
        Fab out2 = phi;
        orc_gsrbiter3d(out2.v.data(), out2.lo, out2.hi, 1, ext.v.data(), ext.lo, ext.hi, rhs.v.data(), rhs.lo, rhs.hi,
                       jg[0].v.data(), jg[0].lo, jg[0].hi, jg[1].v.data(), jg[1].lo, jg[1].hi, jg[2].v.data(), jg[2].lo, jg[2].hi,
                       jinv.v.data(), jinv.lo, jinv.hi, lapd2.v.data(), lapd2.lo, lapd2.hi, vlo, vhi, dx, alpha, beta, rb);
        CELLS {
            if ((i + j + k + rb) & 1) { check("untouched", rb, 0, i, j, k, out.at(i, j, k), phi.at(i, j, k)); continue; }
            auto P = [&](int di, int dj, int dk) { return phi.at(i + di, j + dj, k + dk); };
            auto E = [&](int di, int dj, int dk) { return ext.at(i + di, j + dj, k + dk); };
            check("interior", rb, 0, i, j, k, full19_gsrb_interior(coef(i, j, k), S, alpha, beta, rhs.at(i, j, k), P, E),
                  out.at(i, j, k));
            // the overload k_gsrb_full calls: lapDiag handed over
            check("interior, stored lapDiag", rb, 0, i, j, k,
                  full19_gsrb_interior(coef(i, j, k), S, alpha, beta, rhs.at(i, j, k), lapd2.at(i, j, k), P, E), out2.at(i, j, k));
        }
        for (int mask = 0; mask < 64; ++mask) {
            int stencil[6];   // loX hiX loY hiY loZ hiZ; 0 = BC_NEUM: the face is skipped
            for (int f = 0; f < 6; ++f) stencil[f] = (mask >> f) & 1;
            Fab ob = phi;
            orc_gsrbboundaryiter3d(ob.v.data(), ob.lo, ob.hi, 1, ext.v.data(), ext.lo, ext.hi, rhs.v.data(), rhs.lo, rhs.hi,
                                   jg[0].v.data(), jg[0].lo, jg[0].hi, jg[1].v.data(), jg[1].lo, jg[1].hi, jg[2].v.data(),
                                   jg[2].lo, jg[2].hi, jinv.v.data(), jinv.lo, jinv.hi, vlo, vhi, dx, alpha, beta, stencil, rb);
            CELLS {
                if ((i + j + k + rb) & 1) continue;
                auto P = [&](int di, int dj, int dk) { return phi.at(i + di, j + dj, k + dk); };
                auto E = [&](int di, int dj, int dk) { return ext.at(i + di, j + dj, k + dk); };
                check("boundary", rb, mask, i, j, k,
                      full19_gsrb_boundary(coef(i, j, k), S, alpha, beta, rhs.at(i, j, k), P, E, !stencil[0], !stencil[1],
                                           !stencil[2], !stencil[3], !stencil[4], !stencil[5]),
                      ob.at(i, j, k));
            }
        }
    }

    // ---- the operator: alpha = 0 and != 0; flag sets all-clear, all-set, one face each ----
    const double alphas[2] = {0.0, alpha};
    for (int ia = 0; ia < 2; ++ia)
        for (int set = 0; set < 8; ++set) {
            bool z[6];   // xl xh yl yh zl zh
            for (int f = 0; f < 6; ++f) z[f] = (set == 1) || (set >= 2 && set - 2 == f);
            std::vector<Fab> flux;
            for (int d = 0; d < 3; ++d) {
                flux.emplace_back(jg[d].lo, jg[d].hi, 1);
                orc_mappedgetflux(flux[d].v.data(), flux[d].lo, flux[d].hi, 1, phi.v.data(), phi.lo, phi.hi, ext.v.data(), ext.lo,
                                  ext.hi, jg[d].v.data(), jg[d].lo, jg[d].hi, flux[d].lo, flux[d].hi, 1.0, dx, d);
            }
            CELLS {   // the box's faces as Neumann domain faces: flux := 0
                if (z[0] && i == vlo[0]) flux[0].at(i, j, k) = 0.0;
                if (z[1] && i == vhi[0]) flux[0].at(i + 1, j, k) = 0.0;
                if (z[2] && j == vlo[1]) flux[1].at(i, j, k) = 0.0;
                if (z[3] && j == vhi[1]) flux[1].at(i, j + 1, k) = 0.0;
                if (z[4] && k == vlo[2]) flux[2].at(i, j, k) = 0.0;
                if (z[5] && k == vhi[2]) flux[2].at(i, j, k + 1) = 0.0;
            }
            for (int d = 0; d < 3; ++d)
                for (double& x : flux[d].v) x *= beta;
            Fab lhs(vlo, vhi, 1);
            orc_mappedfluxdivergence3d(lhs.v.data(), lhs.lo, lhs.hi, 1, flux[0].v.data(), flux[0].lo, flux[0].hi, flux[1].v.data(),
                                       flux[1].lo, flux[1].hi, flux[2].v.data(), flux[2].lo, flux[2].hi, jinv.v.data(), jinv.lo,
                                       jinv.hi, vlo, vhi, dx);
            if (alphas[ia] != 0.0) orc_axbyip(lhs.v.data(), lhs.lo, lhs.hi, 1, phi.v.data(), phi.lo, phi.hi, alphas[ia], 1.0, vlo, vhi);
            CELLS {
                auto P = [&](int di, int dj, int dk) { return phi.at(i + di, j + dj, k + dk); };
                auto E = [&](int di, int dj, int dk) { return ext.at(i + di, j + dj, k + dk); };
                check("operator", ia, set, i, j, k,
                      full19_op(coef(i, j, k), S, alphas[ia], beta, phi.at(i, j, k), P, E, z[0] && i == vlo[0], z[1] && i == vhi[0],
                                z[2] && j == vlo[1], z[3] && j == vhi[1], z[4] && k == vlo[2], z[5] && k == vhi[2]),
                      lhs.at(i, j, k));
            }
        }
    std::printf("checked %ld mismatches %ld\n", checked, bad);
    return bad ? 1 : 0;
}
"""

# cells 120; per colour: 120 (interior + untouched) + 60 (interior with the stored lapDiag) + 64 masks x 60 cells of the colour; operator: 2 alphas x 8 sets x 120
CHECKS = 2 * (120 + 60 + 64 * 60) + 2 * 8 * 120


def oracle_cflags():
    text = open(os.path.join(ORACLE, "Makefile")).read()
    return re.search(r"^CFLAGS\s*\?=\s*(.*)$", text, re.M).group(1).split()


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    d = tmp_path_factory.mktemp("full19_point")
    src = d / "point.cpp"
    src.write_text(PROGRAM)

    obj = d / "kernels.o"
    subprocess.check_call(["gcc"] + oracle_cflags() + ["-c", os.path.join(ORACLE, "kernels.c"), "-o", str(obj)])

    def make(name, extra):   # the program and the header under test with `extra`; the oracle's object as the Makefile builds it
        exe = d / name
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                              ["-I", CSRC, str(src), str(obj), "-lm", "-o", str(exe)])
        return str(exe)

    return make


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "checked %d mismatches 0" % CHECKS, r.stdout + r.stderr


def test_point_functions_equal_the_oracle_kernels_bit_for_bit(build):
    run(build("point", []))


def test_point_program_runs_clean_under_address_and_undefined_sanitizers(build):
    exe = build("point_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run(exe)
