// somar_amd/csrc/stencil_point.h -- the per-cell arithmetic of the k-marching 7-point kernels, shared by their single-field
// forms (gsrb_fused.hip, resid_march.hip) and their N-field forms (multi_march.hip): one GSRB point update and one operator
// evaluation.  The N-field kernels are bit-for-bit the single-field ones per field BECAUSE they call these.
#pragma once
#include "common.h"

namespace somar {

// T: the element type of the fields and coefficient arrays -- double, or float on the depths of the opt-in mixed-precision
// cycle (PressureSolver::set_precision), whose arithmetic then stays in float throughout
template <class T>
__device__ __forceinline__ T pick(const typename Vec2<T>::type& v, int s) { return s ? v.y : v.x; }

// load a[idx], a[idx+1] with per-element predicates (idx is pair-aligned by construction)
template <class T>
__device__ __forceinline__ typename Vec2<T>::type ld2(const T* __restrict__ a, long long idx, bool ok0, bool ok1,
                                                      long long safe)
{
    // branch-free: always one aligned 16-byte load (from `safe`, any valid aligned element of the patch, when
    // neither element may be touched), then selects.  Straight-line loads let the compiler count outstanding
    // loads exactly (s_waitcnt vmcnt(N)) instead of draining everything at every predicated branch.
#ifdef SOMAR_NT_LOADS
    // streamed once per launch: keep the coefficient / right-hand-side lines out of the way of the phi halo reuse in L2
    typedef T v2d_ __attribute__((ext_vector_type(2)));
    const v2d_ w = __builtin_nontemporal_load(reinterpret_cast<const v2d_*>(a + ((ok0 || ok1) ? idx : safe)));
    const typename Vec2<T>::type v = mk2<T>(w.x, w.y);
#else
    const typename Vec2<T>::type v = *reinterpret_cast<const typename Vec2<T>::type*>(a + ((ok0 || ok1) ? idx : safe));
#endif
    return mk2<T>(ok0 ? v.x : T(0), ok1 ? v.y : T(0));
}

// One GSRB point update of cell (gi,gj,gk): interior form = GSRBITER3DORTHO, cells touching a domain
// face = GSRBBOUNDARYITER3DORTHO (a Neumann face contributes neither flux nor diagonal; a Dirichlet face contributes
// both, its ghost being -own).  own = the cell's value before this update.
// INT: the caller's tile (its red ring included) touches no domain face and no seam in x and y, so only the plane's position
// in z -- the same for every lane -- decides between the two forms: the per-lane classification (periodic wrap, six
// compares, a divergent branch) collapses into one scalar test per plane.
template <bool DIRI, bool INT, class T>
__device__ __forceinline__ T gsrb_point(const StencilParams& P, T xxS, T yyS, T zzS, int gi,
                                        int gj, int gk, T pxl, T pxh, T pyl, T pyh,
                                        T pzl, T pzh, T gxl, T gxh, T gyl, T gyh,
                                        T gzl, T gzh, T Ji, T rhs, T own)
{
    // a ring cell may be the periodic image of a cell on the far side: classify the REAL cell
    if (!INT && P.periodic[0]) { const int n = P.dom_hi[0] - P.dom_lo[0] + 1; gi = gi < P.dom_lo[0] ? gi + n : (gi > P.dom_hi[0] ? gi - n : gi); }
    if (!INT && P.periodic[1]) { const int n = P.dom_hi[1] - P.dom_lo[1] + 1; gj = gj < P.dom_lo[1] ? gj + n : (gj > P.dom_hi[1] ? gj - n : gj); }
    if (P.periodic[2]) { const int n = P.dom_hi[2] - P.dom_lo[2] + 1; gk = gk < P.dom_lo[2] ? gk + n : (gk > P.dom_hi[2] ? gk - n : gk); }
    const bool onb = (!INT && ((gi == P.dom_lo[0]) || (gi == P.dom_hi[0]) || (gj == P.dom_lo[1]) || (gj == P.dom_hi[1]))) ||
                     (gk == P.dom_lo[2]) || (gk == P.dom_hi[2]);
    if (!onb) {
        const T JDxx = xxS * (gxh * pxh + gxl * pxl);
        const T JDyy = yyS * (gyh * pyh + gyl * pyl);
        const T JDzz = zzS * (gzh * pzh + gzl * pzl);
        const T lphi = T(P.beta) * Ji * (JDxx + JDyy + JDzz);
        // lapDiag: FILLMAPPEDLAPDIAG3D's expression, bitwise the stored array's value
        const T lapd = -Ji * ((gxh + gxl) * xxS + (gyh + gyl) * yyS + (gzh + gzl) * zzS);
        return (rhs - lphi) / (T(P.alpha) + T(P.beta) * lapd);
    }
    const bool nxl = !INT && (gi == P.dom_lo[0]) && P.neum[0][0];
    const bool nxh = !INT && (gi == P.dom_hi[0]) && P.neum[0][1];
    const bool nyl = !INT && (gj == P.dom_lo[1]) && P.neum[1][0];
    const bool nyh = !INT && (gj == P.dom_hi[1]) && P.neum[1][1];
    const bool nzl = (gk == P.dom_lo[2]) && P.neum[2][0];
    const bool nzh = (gk == P.dom_hi[2]) && P.neum[2][1];
    // A Dirichlet face: the neighbour beyond it is the ghost ELLIPTICCONSTDIRIBCGHOST (order 1, homogeneous inside the
    // smoother) derives from this very cell, -phi(cell).  The cell keeps its value through the other colour's pass, so
    // the ghost LevelGSRB refills before each pass is -own in both; it never has to exist in memory.
    // (DIRI is a template parameter: the Neumann / periodic instantiations carry none of this.)
    if (DIRI) {   // (never together with INT)
        if ((gi == P.dom_lo[0]) && P.diri[0][0]) pxl = -own;
        if ((gi == P.dom_hi[0]) && P.diri[0][1]) pxh = -own;
        if ((gj == P.dom_lo[1]) && P.diri[1][0]) pyl = -own;
        if ((gj == P.dom_hi[1]) && P.diri[1][1]) pyh = -own;
        if ((gk == P.dom_lo[2]) && P.diri[2][0]) pzl = -own;
        if ((gk == P.dom_hi[2]) && P.diri[2][1]) pzh = -own;
    }
    T JDloX = 0, JDhiX = 0, JDloY = 0, JDhiY = 0, JDloZ = 0, JDhiZ = 0, ld = 0;
    if (!nxl) { JDloX = gxl * pxl; ld = ld - xxS * gxl; }
    if (!nyl) { JDloY = gyl * pyl; ld = ld - yyS * gyl; }
    if (!nzl) { JDloZ = gzl * pzl; ld = ld - zzS * gzl; }
    if (!nxh) { JDhiX = gxh * pxh; ld = ld - xxS * gxh; }
    if (!nyh) { JDhiY = gyh * pyh; ld = ld - yyS * gyh; }
    if (!nzh) { JDhiZ = gzh * pzh; ld = ld - zzS * gzh; }
    ld = ld * Ji;
    const T lphi = T(P.beta) * Ji * ((JDloX + JDhiX) * xxS + (JDloY + JDhiY) * yyS + (JDloZ + JDhiZ) * zzS);
    return (rhs - lphi) / (T(P.alpha) + T(P.beta) * ld);
}

// L[phi] of one cell, the expression order of k_op_ortho (= MAPPEDGETFLUXORTHO + zero Neumann flux + flux*=beta +
// MAPPEDFLUXDIVERGENCE3D + AXBYIP).  s*: 1 / dx; z**: the face is a Neumann domain face (its flux is zero).
template <class E>
__device__ __forceinline__ E op_point(const StencilParams& P, E sx, E sy, E sz, E pc, E pxl, E pxh, E pyl, E pyh, E pzl,
                                      E pzh, E gxl, E gxh, E gyl, E gyh, E gzl, E gzh, E ji, bool zxl, bool zxh, bool zyl,
                                      bool zyh, bool zzl, bool zzh)
{
    E fxl = gxl * sx * (pc - pxl);
    E fxh = gxh * sx * (pxh - pc);
    E fyl = gyl * sy * (pc - pyl);
    E fyh = gyh * sy * (pyh - pc);
    E fzl = gzl * sz * (pc - pzl);
    E fzh = gzh * sz * (pzh - pc);
    if (zxl) fxl = 0;
    if (zxh) fxh = 0;
    if (zyl) fyl = 0;
    if (zyh) fyh = 0;
    if (zzl) fzl = 0;
    if (zzh) fzh = 0;
    const E beta = E(P.beta);
    fxl *= beta; fxh *= beta; fyl *= beta; fyh *= beta; fzl *= beta; fzh *= beta;
    E l = ji * ((fxh - fxl) * sx + (fyh - fyl) * sy + (fzh - fzl) * sz);
    if (P.alpha != 0.0) l = E(P.alpha) * pc + E(1.0) * l;
    return l;
}

}  // namespace somar
