// somar_amd/csrc/full19.hip -- the NON-diagonal metric path: 19-point operator, 19-point GSRB, and the ghost
// "programs" (extrapolation / copy / Neumann-with-cross-terms) that feed them.
//
// Reference kernels restated here (arithmetic in the Fortran's order; -ffp-contract=off => bit-identical to
// oracle/kernels.c):
//   MAPPEDGETFLUX                 calculus/AMRElliptic/MappedAMRPoissonOpF.ChF:335-427
//   GSRBITER2D / GSRBBOUNDARYITER2D   calculus/AMRElliptic/RelaxationMethods/GSRBF.ChF:155-281 (the 3-D forms, and the
//                                 operator's per-cell sequence: full19_point.h, which k_op_full and k_gsrb_full call)
//   EXTRAPOLATEFACENOEV           calculus/extrapolation/ExtrapolationUtilsF.ChF:35-138
//   ELLIPTICCONSTNEUMBCGHOST      calculus/BCInterface/EllipticBCUtilsF.ChF (cross-term Neumann ghost)
// and the call sequences of fillExtrap (MappedAMRPoissonOp.cpp:2244-2270), RelaxationMethod::
// fillGhostsAndExtrapolate (RelaxationMethod.cpp:376-435), ExtrapolateFaceAndCopy (ExtrapolationUtils.cpp:
// 109-155) and setSideNeumBC (EllipticBCUtils.cpp:128-214), which the host compiles into per-level op lists
// (solver_full.cpp): one launch per op "stage", the ops of one stage touch different boxes.
//
// psi ("extrap") is the reference's second copy of phi whose out-of-domain ghosts hold EXTRAPOLATED values; the
// cross-derivative terms read psi, the normal terms read phi.  In GSRB psi is a snapshot taken before each
// colour pass, i.e. the cross terms lag -- reproduced as is.
#include "common.h"
#include "kernels.h"
#include "full19_point.h"

namespace somar {

__device__ __forceinline__ long long fidx(const PatchDesc& p, int i, int j, int k)
{
    return p.off + i + (long long)p.pj * j + p.pk * k;
}

// ------------------------------------------------------------------------------------
// ghost programs
// ------------------------------------------------------------------------------------
// REDIRECT: psi is kept in the boxes' frames only (its copy inside the valid region is never made): a read of psi at a
// cell INSIDE the box's valid region returns phi there -- the value the full copy psi := phi would have put.
// one op over the threads [t0, t0 + nt, ...) of the caller
// bcf: the level's face-value buffer (GHOST_DIRI_FACE ops read bcf[op.voff + loop index]; null where no such op exists)
// T: the fields' element type (float: the homogeneous physical ghosts of a mixed-precision depth, arithmetic in float)
template <bool REDIRECT, class T = double>
__device__ __forceinline__ void ghost_op_body(const GhostOp& op, const PatchDesc& p, T* phi, T* psi,   // may alias
                                              const JgFull& J, const StencilParams& P, const double* __restrict__ bcf,
                                              int t0, int nt)
{
    const int n0 = op.n[0], n01 = op.n[0] * op.n[1];
    const int cells = n01 * op.n[2];   // a ghost region of one box: far below 2^31 (32-bit index arithmetic: no 64-bit divisions)
    T* dst = op.dstf ? psi : phi;
    const T* src = op.srcf ? psi : phi;
    const long long st[3] = {1, (long long)p.pj, p.pk};
    for (int idx = t0; idx < cells; idx += nt) {
        const int k = idx / n01;
        const int r = idx - k * n01;
        const int j = r / n0, i = r - j * n0;
        const int l0 = op.lo[0] + i, l1 = op.lo[1] + j, l2 = op.lo[2] + k;
        const long long c = fidx(p, l0, l1, l2);
        // value of field `f` (1 = psi) at this cell moved by m steps along direction dd (and mt steps along dt)
        auto rd = [&](const T* f, bool is_psi, int dd, int m, int dt = 0, int mt = 0) {
            int q[3] = {l0, l1, l2};
            q[dd] += m;
            q[dt] += mt;
            const long long cc = c + m * st[dd] + mt * st[dt];
            if (REDIRECT && is_psi && q[0] >= 0 && q[0] < p.n[0] && q[1] >= 0 && q[1] < p.n[1] && q[2] >= 0 && q[2] < p.n[2])
                return phi[cc];
            return f[cc];
        };
        if (op.type == GHOST_COPY) {
            dst[c] = rd(src, op.srcf != 0, 0, 0);
        } else if (op.type == GHOST_EXTRAP) {
            const int s = -op.sgn;  // values come from 1, 2, 3 steps back along dir
            const bool ps = op.srcf != 0;
            if (op.order == 0) dst[c] = rd(src, ps, op.dir, s);
            else if (op.order == 1) dst[c] = T(2.0) * rd(src, ps, op.dir, s) - rd(src, ps, op.dir, 2 * s);
            else dst[c] = T(3.0) * (rd(src, ps, op.dir, s) - rd(src, ps, op.dir, 2 * s)) + rd(src, ps, op.dir, 3 * s);
        } else if (op.type == GHOST_DIRI) {
            // ELLIPTICCONSTDIRIBCGHOST, order 1 (EllipticBCUtilsF.ChF:71-84): the value sits on the face
            const long long s = op.sgn * st[op.dir];
            const T bcval = P.bc_homog ? T(0) : T(op.val);
            if (bcval == T(0)) dst[c] = -src[c - s];
            else dst[c] = T(2.0) * bcval - src[c - s];
        } else if (op.type == GHOST_DIRI_FACE) {
            // EllipticDiriBCGhostClass, cell-centred branch, order 1 (EllipticBCUtils.cpp:588-636): ghost = (-first valid) +
            // 2 g(face); no shortcut for g == 0 (the reference has none).  Homogeneous: -first valid, as the constant form.
            const long long s = op.sgn * st[op.dir];
            if (P.bc_homog) dst[c] = -src[c - s];
            else dst[c] = (-src[c - s]) + T(2.0) * T(bcf[op.voff + idx]);
        } else if (op.type == GHOST_NEUM_FACE) {
            // EllipticNeumBCGhostClass on a DIAGONAL metric (EllipticBCUtils.cpp:842-843, the cross term being zero):
            // ghost = first valid + ((sgn dx) g(face)) / Jg^{dd}(boundary face), in that order.  Homogeneous: the first valid
            // cell's value, the ghost of a zero flux.  The coefficient comes from the level's own array, or from
            // StencilParams::uc on a uniform-metric depth.
            const long long sd = st[op.dir];
            const long long s = op.sgn * sd;
            if (P.bc_homog) dst[c] = src[c - s];
            else {
                const long long f = (op.sgn < 0) ? c + sd : c;   // boundary face (index of the cell it is the low face of)
                const double jg = P.uniform ? P.uc[op.dir] : J.c[op.dir][op.dir][f];
                dst[c] = src[c - s] + T(((op.sgn * P.dx[op.dir]) * bcf[op.voff + idx]) / jg);
            }
        } else {  // GHOST_NEUM: phi ghost such that the boundary flux (cross terms from psi included) equals bcval = 0
            const int a = op.dir, b = (a + 1) % 3, cc = (a + 2) % 3;
            const long long sa = st[a], sb = st[b], sc = st[cc];
            const long long g = c;                                  // ghost cell
            const long long v = c - op.sgn * sa;                    // first valid cell
            const long long f = (op.sgn < 0) ? c + sa : c;          // boundary face (index of the cell it is the low face of)
            const T idxb = T(-0.25) / T(P.dx[b]), idxc = T(-0.25) / T(P.dx[cc]);
            (void)sb; (void)sc;
            // g = this cell, v = this cell moved one step back along a
            const int bk = -op.sgn;
            const T cross = (rd(psi, true, b, 1) - rd(psi, true, b, -1) + rd(psi, true, a, bk, b, 1) - rd(psi, true, a, bk, b, -1)) * T(J.c[a][b][f]) * idxb +
                            (rd(psi, true, cc, 1) - rd(psi, true, cc, -1) + rd(psi, true, a, bk, cc, 1) - rd(psi, true, a, bk, cc, -1)) * T(J.c[a][cc][f]) * idxc;
            phi[g] = phi[v] + (T(0.0) - cross) * T(P.dx[a]) / T(J.c[a][a][f]);
        }
    }
}

template <bool REDIRECT, class T = double>
__global__ void k_ghost_ops(const GhostOp* __restrict__ ops, const PatchDesc* __restrict__ patches,
                            T* phi, T* psi, JgFull J, StencilParams P, const double* __restrict__ bcf)
{
    const GhostOp op = ops[blockIdx.x];
    const PatchDesc p = patches[op.patch];
    ghost_op_body<REDIRECT, T>(op, p, phi, psi, J, P, bcf, (int)(blockIdx.y * blockDim.x + threadIdx.x), (int)(gridDim.y * blockDim.x));
}

// A whole ghost program in ONE launch, one workgroup per box.  Every op of a program reads and writes the storage of its own
// box only (the exchange that feeds it has already run), so the stage boundaries of the dependence schedule -- kernel boundaries
// in the staged form, 12-20 launches per application -- need only a workgroup barrier.  box_ops: the ops of box b, sorted by
// stage (GhostOp::stage, which also counts the ops of the same stage that follow), are box_ops[box_first[b] .. box_first[b + 1]).  For the SMALL levels (boxes of at most a few thousand
// cells: a face is a few hundred cells, one 256-thread workgroup is plenty): on BASELINE C5 5 500 of the 7 700 dispatches of an
// AMR V-cycle were staged ghost ops of such levels, three quarters of them inside the bottom solver.
constexpr int GP_MAX_OPS = 160;   // ops of one box staged in LDS (10 KB); a longer program walks the rest from global memory
template <bool REDIRECT>
__global__ __launch_bounds__(512) void k_ghost_program(const GhostOp* __restrict__ box_ops, const int* __restrict__ box_first,
                                                       const PatchDesc* __restrict__ patches, double* phi, double* psi,
                                                       JgFull J, StencilParams P, int copy_all, const double* __restrict__ bcf)
{
    __shared__ alignas(16) GhostOp sops[GP_MAX_OPS];
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const PatchDesc p = patches[b];
    const int first = box_first[b], nops = box_first[b + 1] - first;
    // the box's op list: one coalesced copy, every load in flight at once (walking it from global memory cost a load
    // latency per op: 100-odd ops per box)
    {
        const int4* src = reinterpret_cast<const int4*>(box_ops + first);
        int4* dst = reinterpret_cast<int4*>(sops);
        const int n16 = min(nops, GP_MAX_OPS) * (int)(sizeof(GhostOp) / 16);
        for (int q = tid; q < n16; q += nth) dst[q] = src[q];
    }
    if (copy_all) {
        // the leading psi := phi of the full-copy programs (run_full_program), on the box grown by its one-cell frame: all a
        // program of this box and the stencil kernel behind it read of psi
        const int m0 = p.n[0] + 2, m1 = p.n[1] + 2, m2 = P.active[2] ? p.n[2] + 2 : 1, z0 = P.active[2] ? -1 : 0;
        for (int idx = tid; idx < m0 * m1 * m2; idx += nth) {
            const int k = idx / (m0 * m1), r = idx - k * (m0 * m1);
            const long long c = fidx(p, r % m0 - 1, r / m0 - 1, k + z0);
            psi[c] = phi[c];
        }
    }
    __threadfence_block();
    __syncthreads();
    // stage by stage; the ops of a stage are independent of each other: one wavefront per op, side by side
    const int wave = tid >> 6, lane = tid & 63, nwaves = nth >> 6;
    int q = 0;
    while (q < nops) {
        // the ops of this stage: this one and those that follow it
        const int e = q + 1 + ghost_following(q < GP_MAX_OPS ? sops[q].stage : box_ops[first + q].stage);
        for (int o = q + wave; o < e; o += nwaves) {
            const GhostOp op = o < GP_MAX_OPS ? sops[o] : box_ops[first + o];
            ghost_op_body<REDIRECT>(op, p, phi, psi, J, P, bcf, lane, 64);
        }
        __threadfence_block();
        __syncthreads();
        q = e;
    }
}

// ------------------------------------------------------------------------------------
// 19-point operator / residual.  Thread = one i-pair, k-loop over the tile (as k_op_ortho).
// MODE 0: out = rhs - L[phi]   MODE 1: out = L[phi]
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double flux19(const double* __restrict__ phi, const double* __restrict__ E, const JgFull& J,
                                         long long c, int a, const long long st[3], const double dxi[3])
{
    // MAPPEDGETFLUX with beta = a_ref = 1 at the face that is the LOW face of cell c in direction a
    const int b = (a + 1) % 3, cc = (a + 2) % 3;
    const long long sa = st[a], sb = st[b], sc = st[cc];
    const double aScale = 1.0 * dxi[a], bScale = 0.25 * 1.0 * dxi[b], cScale = 0.25 * 1.0 * dxi[cc];
    return aScale * J.c[a][a][c] * (phi[c] - phi[c - sa]) +
           bScale * J.c[a][b][c] * (E[c + sb] - E[c - sb] + E[c + sb - sa] - E[c - sb - sa]) +
           cScale * J.c[a][cc][c] * (E[c + sc] - E[c - sc] + E[c + sc - sa] - E[c - sc - sa]);
}

// MAPPEDGETFLUX (beta = a_ref = 1) on every face of every patch: cell c holds its low face, the last cell of a row
// also fills the high face (the next cell's slot in the frame)
struct F3 { double* v[3]; };
__global__ __launch_bounds__(512) void k_flux_full(const Tile* __restrict__ tiles, const PatchDesc* __restrict__ patches,
                                                   F3 out, const double* __restrict__ phi, const double* __restrict__ psi,
                                                   JgFull J, StencilParams P)
{
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
    const int lj = t.j0 + threadIdx.y;
    const int li0 = t.i0 + 2 * threadIdx.x;
    if (lj >= p.n[1] || li0 >= p.n[0]) return;
    const double dxi[3] = {1.0 / P.dx[0], 1.0 / P.dx[1], 1.0 / P.dx[2]};
    const long long st[3] = {1, (long long)p.pj, p.pk};
    const int npair = (li0 + 1 < p.n[0]) ? 2 : 1;
    for (int kk = 0; kk < t.nk; ++kk) {
        const int lk = t.k0 + kk;
        for (int q = 0; q < npair; ++q) {
            const int l[3] = {li0 + q, lj, lk};
            const long long c = fidx(p, l[0], l[1], l[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!P.active[a]) continue;
                out.v[a][c] = flux19(phi, psi, J, c, a, st, dxi);
                if (l[a] == p.n[a] - 1) out.v[a][c + st[a]] = flux19(phi, psi, J, c + st[a], a, st, dxi);
            }
        }
    }
}

// the coefficients of cell c from global memory (full19_point.h).  flat (SpaceDim 2): there are no z faces, their entries are
// never used and not loaded
__device__ __forceinline__ Full19Coef coef_at(const JgFull& J, const double* __restrict__ jinv, long long c, long long sj,
                                              long long sk, bool flat)
{
    Full19Coef C;
    C.x0l = J.c[0][0][c]; C.x0h = J.c[0][0][c + 1];
    C.x1l = J.c[0][1][c]; C.x1h = J.c[0][1][c + 1];
    C.x2l = J.c[0][2][c]; C.x2h = J.c[0][2][c + 1];
    C.y0l = J.c[1][0][c]; C.y0h = J.c[1][0][c + sj];
    C.y1l = J.c[1][1][c]; C.y1h = J.c[1][1][c + sj];
    C.y2l = J.c[1][2][c]; C.y2h = J.c[1][2][c + sj];
    C.z0l = flat ? 0.0 : J.c[2][0][c]; C.z0h = flat ? 0.0 : J.c[2][0][c + sk];
    C.z1l = flat ? 0.0 : J.c[2][1][c]; C.z1h = flat ? 0.0 : J.c[2][1][c + sk];
    C.z2l = flat ? 0.0 : J.c[2][2][c]; C.z2h = flat ? 0.0 : J.c[2][2][c + sk];
    C.ji = jinv[c];
    return C;
}

template <int MODE>
__global__ __launch_bounds__(512) void k_op_full(const Tile* __restrict__ tiles, const PatchDesc* __restrict__ patches,
                                                 double* __restrict__ out, const double* __restrict__ phi,
                                                 const double* __restrict__ psi, const double* __restrict__ rhs,
                                                 JgFull J, const double* __restrict__ jinv, StencilParams P)
{
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
    const int lj = t.j0 + threadIdx.y;
    const int li0 = t.i0 + 2 * threadIdx.x;
    if (lj >= p.n[1] || li0 >= p.n[0]) return;
    const Full19Scales S = full19_scales(P.dx[0], P.dx[1], P.dx[2]);
    const long long sj = p.pj, sk = p.pk;
    const int gj = p.lo[1] + lj;
    const int npair = (li0 + 1 < p.n[0]) ? 2 : 1;
    for (int kk = 0; kk < t.nk; ++kk) {
        const int lk = t.k0 + kk;
        const int gk = p.lo[2] + lk;
        for (int q = 0; q < npair; ++q) {
            const int li = li0 + q;
            const int gi = p.lo[0] + li;
            const long long c = fidx(p, li, lj, lk);
            const auto Pn = [=](int di, int dj, int dk) { return phi[c + di + sj * dj + sk * dk]; };
            const auto En = [=](int di, int dj, int dk) { return psi[c + di + sj * dj + sk * dk]; };
            const Full19Coef C = coef_at(J, jinv, c, sj, sk, false);
            const double l = full19_op(C, S, P.alpha, P.beta, phi[c], Pn, En, FULL19_NF(xl), FULL19_NF(xh), FULL19_NF(yl),
                                       FULL19_NF(yh), FULL19_NF(zl), FULL19_NF(zh));
            out[c] = (MODE == 0) ? (rhs[c] - l) : l;
        }
    }
}

// ------------------------------------------------------------------------------------
// 19-point GSRB, one colour.  Interior cells: GSRBITER3D; cells touching a domain face: GSRBBOUNDARYITER3D.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_gsrb_full(const Tile* __restrict__ tiles, const PatchDesc* __restrict__ patches,
                                                   double* __restrict__ phi, const double* __restrict__ E,
                                                   const double* __restrict__ rhs, JgFull J,
                                                   const double* __restrict__ jinv, const double* __restrict__ lapd,
                                                   StencilParams P, int color)
{
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
    const int lj = t.j0 + threadIdx.y;
    const int li0 = t.i0 + 2 * threadIdx.x;
    if (lj >= p.n[1] || li0 >= p.n[0]) return;
    const Full19Scales S = full19_scales(P.dx[0], P.dx[1], P.dx[2]);
    const long long sj = p.pj, sk = p.pk;
    const int gj = p.lo[1] + lj;
    const double* Jx0 = J.c[0][0]; const double* Jx1 = J.c[0][1];
    const double* Jy0 = J.c[1][0]; const double* Jy1 = J.c[1][1];
    for (int kk = 0; kk < t.nk; ++kk) {
        const int lk = t.k0 + kk;
        const int gk = p.lo[2] + lk;
        const int li = li0 + ((p.lo[0] + li0 + gj + gk + color) & 1);
        if (li >= p.n[0]) continue;
        const int gi = p.lo[0] + li;
        const long long c = fidx(p, li, lj, lk);
        const bool flat = !P.active[2];  // SpaceDim 2: the 9-point kernels GSRBITER2D / GSRBBOUNDARYITER2D
        const bool onb = (gi == P.dom_lo[0]) || (gi == P.dom_hi[0]) || (gj == P.dom_lo[1]) || (gj == P.dom_hi[1]) ||
                         (!flat && ((gk == P.dom_lo[2]) || (gk == P.dom_hi[2])));
#define EE(di, dj, dk) E[c + (di) + sj * (dj) + sk * (dk)]
        double out;
        if (!onb && flat) {
            // GSRBITER2D (GSRBF.ChF:155-281) writes its cross sums out term by term (a - b + c - d) where GSRBITER3D
            // goes through pdx / pdy: they round differently, so this is not the 3-D branch with z dropped
            const double JDxx = Jx0[c + 1] * phi[c + 1] + Jx0[c] * phi[c - 1];
            const double JDxy = Jx1[c + 1] * (EE(1, 1, 0) - EE(1, -1, 0) + EE(0, 1, 0) - EE(0, -1, 0)) -
                                Jx1[c] * (EE(0, 1, 0) - EE(0, -1, 0) + EE(-1, 1, 0) - EE(-1, -1, 0));
            const double JDyx = Jy0[c + sj] * (EE(1, 1, 0) - EE(-1, 1, 0) + EE(1, 0, 0) - EE(-1, 0, 0)) -
                                Jy0[c] * (EE(1, 0, 0) - EE(-1, 0, 0) + EE(1, -1, 0) - EE(-1, -1, 0));
            const double JDyy = Jy1[c + sj] * phi[c + sj] + Jy1[c] * phi[c - sj];
            const double lphi = P.beta * jinv[c] * (JDxx * S.xx + JDyy * S.yy + (JDxy + JDyx) * S.xy);
            out = (rhs[c] - lphi) / (P.alpha + P.beta * lapd[c]);
        } else {
            const auto Pn = [=](int di, int dj, int dk) { return phi[c + di + sj * dj + sk * dk]; };
            const auto En = [=](int di, int dj, int dk) { return EE(di, dj, dk); };
            const Full19Coef C = coef_at(J, jinv, c, sj, sk, flat);
            // flat: no z faces at all; the zx / yz terms of the x and y faces multiply all-zero metric planes
            if (!onb) out = full19_gsrb_interior(C, S, P.alpha, P.beta, rhs[c], lapd[c], Pn, En);
            else out = full19_gsrb_boundary(C, S, P.alpha, P.beta, rhs[c], Pn, En, FULL19_NF(xl), FULL19_NF(xh), FULL19_NF(yl),
                                            FULL19_NF(yh), flat || FULL19_NF(zl), flat || FULL19_NF(zh));
        }
#undef EE
        phi[c] = out;
    }
}

// ------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------
JgFull jgfull(const LevelDev& L)
{
    JgFull J;
    for (int d = 0; d < 3; ++d)
        for (int c = 0; c < 3; ++c) J.c[d][c] = L.jgf[d][c];
    // a diagonal-metric level keeps no jgf: its GHOST_NEUM_FACE ops read J g^{dd} through the same table
    for (int d = 0; d < 3; ++d)
        if (!J.c[d][d]) J.c[d][d] = L.jg[d];
    return J;
}

void launch_ghost_ops(hipStream_t st, const LevelDev& L, const GhostOp* ops, int nops, double* phi, double* psi,
                      bool bc_homog, bool redirect)
{
    if (nops == 0) return;
    StencilParams P = L.P;
    P.bc_homog = bc_homog ? 1 : 0;
    if (redirect) hipLaunchKernelGGL(k_ghost_ops<true>, dim3(nops, L.ghost_gy), dim3(256), 0, st, ops, L.patches, phi, psi, jgfull(L), P, L.bc_face);
    else hipLaunchKernelGGL(k_ghost_ops<false>, dim3(nops, L.ghost_gy), dim3(256), 0, st, ops, L.patches, phi, psi, jgfull(L), P, L.bc_face);
}

void launch_ghost_ops(hipStream_t st, const LevelDev& L, const GhostOp* ops, int nops, float* phi)
{
    if (nops == 0) return;
    StencilParams P = L.P;
    P.bc_homog = 1;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ghost_ops<false, float>), dim3(nops, L.ghost_gy), dim3(256), 0, st, ops, L.patches, phi, phi,
                       jgfull(L), P, L.bc_face);
}

void launch_ghost_program(hipStream_t st, const LevelDev& L, const GhostOp* box_ops, const int* box_first, double* phi,
                          double* psi, bool bc_homog, bool redirect, bool copy_all)
{
    if (L.npatches == 0) return;
    StencilParams P = L.P;
    P.bc_homog = bc_homog ? 1 : 0;
    if (redirect) hipLaunchKernelGGL(k_ghost_program<true>, dim3(L.npatches), dim3(512), 0, st, box_ops, box_first, L.patches, phi, psi, jgfull(L), P, copy_all ? 1 : 0, L.bc_face);
    else hipLaunchKernelGGL(k_ghost_program<false>, dim3(L.npatches), dim3(512), 0, st, box_ops, box_first, L.patches, phi, psi, jgfull(L), P, copy_all ? 1 : 0, L.bc_face);
}

void launch_flux_full(hipStream_t st, const LevelDev& L, double* const out[3], const double* phi, const double* psi)
{
    if (L.ntiles == 0) return;
    F3 o;
    for (int a = 0; a < 3; ++a) o.v[a] = out[a];
    hipLaunchKernelGGL(k_flux_full, dim3(L.ntiles), dim3(64, L.tile_j, 1), 0, st, L.tiles, L.patches, o, phi, psi, jgfull(L), L.P);
}

void launch_op_full(hipStream_t st, const LevelDev& L, double* out, const double* phi, const double* psi,
                    const double* rhs, int mode)
{
    if (L.ntiles == 0) return;
    dim3 b(64, L.tile_j, 1);
    if (mode == 0)
        hipLaunchKernelGGL(k_op_full<0>, dim3(L.ntiles), b, 0, st, L.tiles, L.patches, out, phi, psi, rhs, jgfull(L),
                           L.jinv, L.P);
    else
        hipLaunchKernelGGL(k_op_full<1>, dim3(L.ntiles), b, 0, st, L.tiles, L.patches, out, phi, psi, rhs, jgfull(L),
                           L.jinv, L.P);
}

void launch_gsrb_full(hipStream_t st, const LevelDev& L, double* phi, const double* psi, const double* rhs, int color)
{
    if (L.ntiles == 0) return;
    hipLaunchKernelGGL(k_gsrb_full, dim3(L.ntiles), dim3(64, L.tile_j, 1), 0, st, L.tiles, L.patches, phi, psi, rhs,
                       jgfull(L), L.jinv, L.lapdiag, L.P, color);
}

}  // namespace somar
