// somar_amd/csrc/full19_point.h -- the per-cell arithmetic of the NON-diagonal (19-point) operator and GSRB update, written
// once.  Its users: the k-marching kernels on LDS planes (full19_march.hip, full19_multi.hip) and the direct-load kernels on
// global memory (full19.hip: k_op_full, k_gsrb_full's 3-D branches).  full19_fused.hip, off by default, keeps a marked
// copy of the two update blocks (see there).  On the same operands they give
// the same bits, field by field and path by path, BECAUSE they share this text; tests/test_full19_point.py holds the functions
// against oracle/kernels.c from a stand-alone host program (plain C++: this header includes no HIP header).
//
// Reference kernels restated here, arithmetic in the Fortran's order (-ffp-contract=off => the oracle's bits):
//   full19_op                     MAPPEDGETFLUX (beta = a_ref = 1)   calculus/AMRElliptic/MappedAMRPoissonOpF.ChF:335-427,
//                                 then EllipticConstNeumBCFluxClass's zero flux on Neumann domain faces, flux *= beta,
//                                 MAPPEDFLUXDIVERGENCE3D (DivCurlGrad/DivCurlGradF.ChF:1122-1215) and AXBYIP (k_op_full's
//                                 sequence)
//   full19_gsrb_interior          GSRBITER3D   calculus/AMRElliptic/RelaxationMethods/GSRBF.ChF:283-439.  Its lapDiag is one
//                                 operand with two sources.  The marching kernels recompute it from the cell's coefficients
//                                 by FILLMAPPEDLAPDIAG3D's expression (MappedAMRPoissonOpF.ChF:233-274; k_lapdiag).
//                                 k_gsrb_full hands over the level's stored array (the second overload).  The two are the
//                                 same bits only where the coefficient arrays still are what k_lapdiag read: a coarsened
//                                 depth fills lapDiag BEFORE fill_metric_ghosts (build_coarser, solver.cpp) replaces the high-side copy
//                                 of every face two boxes share by the low-side owner's, so where the two copies are
//                                 not bitwise equal the stored value -- the reference's, a per-box FAB -- is not the
//                                 expression's on the arrays as they stand afterwards.  With the recomputed value in
//                                 k_gsrb_full, tests/test_gpu_c5.py, test_gpu_box_bottom.py (19-point case) and
//                                 test_gpu_metric_refresh.py (non-diagonal maps) miss the oracle; with the stored one
//                                 they meet it.
//   full19_gsrb_boundary          GSRBBOUNDARYITER3D   .../GSRBF.ChF:1024-1230
//
// Neighbours come through two accessors, called with constant offsets: P(di, dj, dk) = phi, E(di, dj, dk) = the extrapolated
// copy ("extrap": phi inside the box, psi in its frame) the cross terms read.
#pragma once

#ifdef __HIPCC__
#define SOMAR_F19 __host__ __device__ __forceinline__
#else
#define SOMAR_F19 inline
#endif

namespace somar {

// J g^{ab} on the low (l) and high (h) a-face of one cell -- x0 = J g^{xx}, x1 = J g^{xy}, x2 = J g^{xz}, y0 = J g^{yx}, ... --
// and 1 / J of the cell
struct Full19Coef {
    double x0l, x0h, x1l, x1h, x2l, x2h;
    double y0l, y0h, y1l, y1h, y2l, y2h;
    double z0l, z0h, z1l, z1h, z2l, z2h;
    double ji;
};

// what depends on dx alone, built once per kernel
struct Full19Scales {
    double dxi0, dxi1, dxi2;         // 1 / dx_a
    double a0, a1, a2, q0, q1, q2;   // MAPPEDGETFLUX's with beta = a_ref = 1: aScale = 1.0 * dxi[a], b/cScale = 0.25 * 1.0 * dxi[b/c]
    double xx, yy, zz, xy, yz, zx;   // GSRBITER3D's: 1 / dx_a^2, 0.25 / (dx_a dx_b)
};

SOMAR_F19 Full19Scales full19_scales(double dx0, double dx1, double dx2)
{
    Full19Scales S;
    S.dxi0 = 1.0 / dx0, S.dxi1 = 1.0 / dx1, S.dxi2 = 1.0 / dx2;
    S.a0 = 1.0 * S.dxi0, S.a1 = 1.0 * S.dxi1, S.a2 = 1.0 * S.dxi2;
    S.q0 = 0.25 * 1.0 * S.dxi0, S.q1 = 0.25 * 1.0 * S.dxi1, S.q2 = 0.25 * 1.0 * S.dxi2;
    S.xx = 1.0 / (dx0 * dx0);
    S.yy = 1.0 / (dx1 * dx1);
    S.zz = 1.0 / (dx2 * dx2);
    S.xy = 0.25 / (dx0 * dx1);
    S.yz = 0.25 / (dx1 * dx2);
    S.zx = 0.25 / (dx2 * dx0);
    return S;
}

// Where cell (gi, gj, gk) sits, for kernels that have `int gi, gj, gk` and their `StencilParams P` in scope under exactly
// these names (macros: as functions they renumber the registers of the marching kernels).  NOT for use inside this header's
// own functions, where P is the phi accessor: those take the six flags as arguments.
// FULL19_ONB: it touches a domain face (GSRBBOUNDARYITER3D's cells).  FULL19_NF(f): its face f = xl, xh, yl, yh, zl, zh is a
// Neumann domain face: no flux through it, no share of the diagonal.
#define FULL19_ONB                                                                                                    \
    ((gi == P.dom_lo[0]) || (gi == P.dom_hi[0]) || (gj == P.dom_lo[1]) || (gj == P.dom_hi[1]) || (gk == P.dom_lo[2]) || \
     (gk == P.dom_hi[2]))
#define FULL19_NF(f) FULL19_NF_##f
#define FULL19_NF_xl ((gi == P.dom_lo[0]) && P.neum[0][0])
#define FULL19_NF_xh ((gi == P.dom_hi[0]) && P.neum[0][1])
#define FULL19_NF_yl ((gj == P.dom_lo[1]) && P.neum[1][0])
#define FULL19_NF_yh ((gj == P.dom_hi[1]) && P.neum[1][1])
#define FULL19_NF_zl ((gk == P.dom_lo[2]) && P.neum[2][0])
#define FULL19_NF_zh ((gk == P.dom_hi[2]) && P.neum[2][1])

// The coefficients of cell s (0 / 1) of a lane's pair into the Full19Coef C, from the plane's pair registers of a marching
// kernel, which has them in scope under these names: x-faces Jx0, Jx1, Jx2 (the pair's two low faces) and jx0n, jx1n, jx2n (the
// next lane's first: the high face of cell 1), y-faces Jy* / Jy*h (row j / j + 1), z-faces Jz*c / Jz*p (plane k / k + 1), Ji.
// (A macro for the reason given below: as a function, by reference, by value or through an out-parameter, it moved all 24.)
#define FULL19_PICK(C, s)                                            \
    C.x0l = (s) ? Jx0.y : Jx0.x, C.x0h = (s) ? jx0n : Jx0.y;         \
    C.x1l = (s) ? Jx1.y : Jx1.x, C.x1h = (s) ? jx1n : Jx1.y;         \
    C.x2l = (s) ? Jx2.y : Jx2.x, C.x2h = (s) ? jx2n : Jx2.y;         \
    C.y0l = (s) ? Jy0.y : Jy0.x, C.y0h = (s) ? Jy0h.y : Jy0h.x;      \
    C.y1l = (s) ? Jy1.y : Jy1.x, C.y1h = (s) ? Jy1h.y : Jy1h.x;      \
    C.y2l = (s) ? Jy2.y : Jy2.x, C.y2h = (s) ? Jy2h.y : Jy2h.x;      \
    C.z0l = (s) ? Jz0c.y : Jz0c.x, C.z0h = (s) ? Jz0p.y : Jz0p.x;    \
    C.z1l = (s) ? Jz1c.y : Jz1c.x, C.z1h = (s) ? Jz1p.y : Jz1p.x;    \
    C.z2l = (s) ? Jz2c.y : Jz2c.x, C.z2h = (s) ? Jz2p.y : Jz2p.x;    \
    C.ji = (s) ? Ji.y : Ji.x

// The three functions.  Their statements stand in full19_point.inc, which the marching kernels include in place instead of
// calling these: every function form tried moved the register allocation of all 24 instantiations of k_full_march, which sit
// at the edge of three waves per SIMD (profiles/r16_full19_one_text.md); the included text compiles to the instructions the
// kernels had.  Either way it is one text.
#define Pn(di, dj, dk) P(di, dj, dk)
#define En(di, dj, dk) E(di, dj, dk)
#define CF(n) C.n
#define SC(n) S.n
#define NEU(f) n##f
#define F19_RESULT(v) return v

// L[phi] of one cell: k_op_full's sequence.  pc = P(0, 0, 0); n** = the face is a Neumann domain face (its flux is zero).
template <class PA, class EA>
SOMAR_F19 double full19_op(const Full19Coef& C, const Full19Scales& S, double alpha, double beta, double pc, const PA& P,
                           const EA& E, bool nxl, bool nxh, bool nyl, bool nyh, bool nzl, bool nzh)
{
#define FULL19_PART 1
#include "full19_point.inc"
    return l;
}

// One GSRB update of a cell that touches no domain face.  rh = its right-hand side.
template <class PA, class EA>
SOMAR_F19 double full19_gsrb_interior(const Full19Coef& C, const Full19Scales& S, double alpha, double beta, double rh,
                                      const PA& P, const EA& E)
{
#define FULL19_PART 2
#include "full19_point.inc"
}

// The same with the cell's lapDiag handed over (k_gsrb_full: the level's stored array, see the first comment).
template <class PA, class EA>
SOMAR_F19 double full19_gsrb_interior(const Full19Coef& C, const Full19Scales& S, double alpha, double beta, double rh,
                                      double lapDiag, const PA& P, const EA& E)
{
#define FULL19_LAPD lapDiag
#define FULL19_PART 2
#include "full19_point.inc"
#undef FULL19_LAPD
}

// One GSRB update of a cell on a domain face.  n** = skip this face (a Neumann domain face; a 2-D caller skips both z faces).
template <class PA, class EA>
SOMAR_F19 double full19_gsrb_boundary(const Full19Coef& C, const Full19Scales& S, double alpha, double beta, double rh,
                                      const PA& P, const EA& E, bool nxl, bool nxh, bool nyl, bool nyh, bool nzl, bool nzh)
{
#define FULL19_PART 3
#include "full19_point.inc"
}

#undef Pn
#undef En
#undef CF
#undef SC
#undef NEU
#undef F19_RESULT

}  // namespace somar
