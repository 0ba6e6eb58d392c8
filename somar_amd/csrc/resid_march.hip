// somar_amd/csrc/resid_march.hip -- operator / residual of a large level as a k-marching, LDS-staged kernel.
//
// Why: k_op_ortho (kernels.hip) reads phi through L2 and, measured with rocprofv3 PMC at 512^3, moves 136 B
// per cell over the fabric against 56 algorithmic: the k+-1 (and j+-1) reuse distance of a 7-point stencil
// does not fit the 4 MiB per-XCD L2 when 256 workgroups stream different slabs.  Here a workgroup owns a
// (124 x 14) column of cells and marches in k, exactly like the fused GSRB sweep (gsrb_fused.hip):
//   * phi of plane k is staged in LDS (2 rotating planes of 128 x 16 doubles, one wavefront per row, one
//     double2 per lane, ONE barrier per plane); the k-neighbours and Jg^zz stay in registers;
//   * every array is read once: phi 8 (x 128*16/(124*14) halo), rhs 8, Jg 24, Jinv 8, out 8 = ~58 B/cell.
//
// Arithmetic: the expression order of k_op_ortho (= MAPPEDGETFLUXORTHO + zero Neumann flux + flux*=beta +
// MAPPEDFLUXDIVERGENCE3D + AXBYIP + SUBTRACTOP) => bit-identical to it and to the CPU oracle.
// MODE 0: out = rhs - L[phi]   MODE 1: out = L[phi]
#include "common.h"
#include "kernels.h"
#include "stencil_point.h"   // ld2, op_point: shared with the fused sweep and the N-field kernels (multi_march.hip)

namespace somar {

constexpr int RM_J = 16;   // region rows = 14-row tile + 1 low + 1 high

// E: the element type of the fields and coefficient arrays -- double, or float on the depths of the opt-in mixed-precision
// cycle (PressureSolver::set_precision), whose arithmetic then stays in float; only the volume sum is accumulated in double.
// ld2 (stencil_point.h): the branch-free predicated pair load
// unconditional: the zeros ld2 returns under a false predicate only reach cells that are not written (see gsrb_fused.hip)
template <class T>
__device__ __forceinline__ typename Vec2<T>::type rm_uni2(double c, bool, bool) { return mk2<T>(T(c), T(c)); }

// UNI: uniform metric, the four coefficient arrays are not read (StencilParams::uc)
// CLS: the tile's lane class (see full19_march.hip): a wavefront covers 2^CLS region rows of 128 >> CLS columns
template <int MODE, bool UNI, int CLS, class E>
__device__ __forceinline__ void resid_march_body(E* __restrict__ S, E* __restrict__ T, const Tile& t,
                                                 const PatchDesc& p, E* __restrict__ out,
                                                 const E* __restrict__ phi, const E* __restrict__ rhs,
                                                 const E* __restrict__ jgx, const E* __restrict__ jgy,
                                                 const E* __restrict__ jgz, const E* __restrict__ jinv,
                                                 const StencilParams& P, const PatchDesc* __restrict__ cpatches, int r0,
                                                 int r1, int r2, double dxProduct, double* __restrict__ volsum)
{
    typedef typename Vec2<E>::type E2;
    constexpr int LPR = 64 >> CLS;                 // lanes per region row
    constexpr int NR = RM_J << CLS;                // region rows of the workgroup
    constexpr int PITCH = 2 * LPR + (CLS >= 2 ? 2 : 0);
#define Sx(slot, r, c) S[((slot) * NR + (r)) * PITCH + (c)]
#define Tx(slot, r, l) (T + ((((slot) * NR + (r)) * LPR + (l)) << 2))
    // class 0: the region row is the wavefront's index, a scalar -- everything derived from it stays in scalar registers
    const int lane = CLS == 0 ? (int)threadIdx.x : (int)(threadIdx.x & (LPR - 1));
    const int row = CLS == 0 ? (int)threadIdx.y
                             : (int)(((threadIdx.y >> 1) << (CLS + 1)) + (threadIdx.y & 1) + 2 * (threadIdx.x >> (6 - CLS)));
    const int ri = 2 * lane;
    const int li = t.i0 - 2 + ri;  // even: rows are 16-byte aligned
    const int wi = t.w > 0 ? t.w : 2 * LPR - 4;  // output columns of this tile (see gsrb_fused.hip)
    const int lj = t.j0 - 1 + row;
    const int gj = p.lo[1] + lj;
    const E sx = E(1.0) / E(P.dx[0]), sy = E(1.0) / E(P.dx[1]), sz = E(1.0) / E(P.dx[2]);

    // phi may be touched inside the 1-cell ghost layer, coefficients only at the tile's own cells / faces
    const bool fj = (lj >= -1) && (lj <= p.n[1]);
    const bool f0 = fj && (li >= -1) && (li <= p.n[0]) && (ri < wi + 4);
    const bool f1 = fj && (li + 1 >= -1) && (li + 1 <= p.n[0]) && (ri + 1 < wi + 4);
    const bool own_j = (lj >= 0) && (lj < p.n[1]) && (row >= 1) && (row <= NR - 2) && (lj < t.j0 + (NR - 2));
    bool o[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int l = li + s, r = ri + s;
        o[s] = own_j && (l >= 0) && (l < p.n[0]) && (r >= 2) && (r < wi + 2);
    }
    // Jg^xx is also needed on the face right of the pair's second cell (next lane's first component): load the
    // pair if either of its cells, or the cell left of it, is an output cell
    // (the shuffle must run with all lanes active: keep it out of the short-circuit)
    const int left_o1 = __shfl_up((int)o[1], 1, 64);
    const bool gxo0 = o[0] || (left_o1 != 0);
    const bool any = o[0] || o[1];
    const long long sj = p.pj, sk = p.pk;
    const long long base = p.off + li + sj * lj;
    const bool zyl = (gj == P.dom_lo[1]) && P.neum[1][0];
    const bool zyh = (gj == P.dom_hi[1]) && P.neum[1][1];
    bool zxl[2], zxh[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int gi = p.lo[0] + li + s;
        zxl[s] = (gi == P.dom_lo[0]) && P.neum[0][0];
        zxh[s] = (gi == P.dom_hi[0]) && P.neum[0][1];
    }

    // MODE 2 state: this pair's (res/J, 1/J) of the previous plane, running sums of up to two coarse cells
    E pv[4] = {0, 0, 0, 0}, cs[2] = {0, 0}, cjs[2] = {0, 0};
    const bool leader = (MODE == 2) && any && (r1 == 1 || ((lj & 1) == 0));
    auto accumulate = [&](int kp) {
        // MAPPEDAVERAGE2's loop order: ii2 (planes), ii1 (rows), ii0 (cells of the pair)
        if (!leader) return;
        const bool first = (r2 == 1) || ((kp & 1) == 0);
        const bool last = (r2 == 1) || ((kp & 1) == 1);
        if (first) { cs[0] = cs[1] = 0; cjs[0] = cjs[1] = 0; }
        E q[4] = {0, 0, 0, 0};
        if (r1 == 2) {
            const E* src = Tx(kp & 1, row + 1, lane);
            q[0] = src[0]; q[1] = src[1]; q[2] = src[2]; q[3] = src[3];
        }
        if (r0 == 2) {
            cs[0] = cs[0] + pv[0]; cjs[0] = cjs[0] + pv[2];
            cs[0] = cs[0] + pv[1]; cjs[0] = cjs[0] + pv[3];
            if (r1 == 2) {
                cs[0] = cs[0] + q[0]; cjs[0] = cjs[0] + q[2];
                cs[0] = cs[0] + q[1]; cjs[0] = cjs[0] + q[3];
            }
        } else {
            cs[0] = cs[0] + pv[0]; cjs[0] = cjs[0] + pv[2];
            cs[1] = cs[1] + pv[1]; cjs[1] = cjs[1] + pv[3];
            if (r1 == 2) {
                cs[0] = cs[0] + q[0]; cjs[0] = cjs[0] + q[2];
                cs[1] = cs[1] + q[1]; cjs[1] = cjs[1] + q[3];
            }
        }
        if (last) {
            const PatchDesc cp = cpatches[t.patch];
            const long long c = cp.off + (li / r0) + (long long)cp.pj * (lj / r1) + cp.pk * (kp / r2);
            if (r0 == 2) {
                out[c] = cs[0] / cjs[0];
            } else {
                if (o[0]) out[c] = cs[0] / cjs[0];
                if (o[1]) out[c + 1] = cs[1] / cjs[1];
            }
        }
    };

    // MODE 2 with volsum: this block's sum of dvol * phi over its own cells (dvol = dxProduct / Jinv), the fine
    // half of the zero-average prolongation's mean (see PressureSolver::cycle); tree order
    double vsum = 0.0;

    int k = t.k0;
    E2 Pm = ld2(phi, base + sk * (k - 1), o[0], o[1], p.off);
    E2 Pc = ld2(phi, base + sk * k, f0, f1, p.off);
    E2 Gzc = UNI ? rm_uni2<E>(P.uc[2], o[0], o[1]) : ld2(jgz, base + sk * k, o[0], o[1], p.off);
    const int kend = t.k0 + t.nk;
    for (; k < kend; ++k) {
        const int gk = p.lo[2] + k;
        const bool more = (k + 1 < kend);
        // ---- this step's loads ----
        const E2 Pp = ld2(phi, base + sk * (k + 1), more ? f0 : o[0], more ? f1 : o[1], p.off);
        const E2 Gzp = UNI ? rm_uni2<E>(P.uc[2], o[0], o[1]) : ld2(jgz, base + sk * (k + 1), o[0], o[1], p.off);
        E2 Rh = mk2<E>(E(0), E(0));
        if (MODE != 1) Rh = ld2(rhs, base + sk * k, o[0], o[1], p.off);
        const E2 Ji = UNI ? rm_uni2<E>(P.uc[3], o[0], o[1]) : ld2(jinv, base + sk * k, o[0], o[1], p.off);
        const E2 Gx = UNI ? rm_uni2<E>(P.uc[0], gxo0, o[0] || o[1]) : ld2(jgx, base + sk * k, gxo0, o[0] || o[1], p.off);
        const E2 Gy = UNI ? rm_uni2<E>(P.uc[1], o[0], o[1]) : ld2(jgy, base + sk * k, o[0], o[1], p.off);
        const E2 Gyh = UNI ? rm_uni2<E>(P.uc[1], o[0], o[1]) : ld2(jgy, base + sk * k + sj, o[0], o[1], p.off);
        const E gx_next = __shfl_down(Gx.x, 1, 64);

        // ---- stage plane k; slot k&1 was last read two steps ago, one barrier per plane suffices ----
        const int slot = k & 1;
        *reinterpret_cast<E2*>(&Sx(slot, row, ri)) = Pc;
        __syncthreads();
        if (MODE == 2 && k > t.k0) accumulate(k - 1);

        if (any) {
            const bool zzl = (gk == P.dom_lo[2]) && P.neum[2][0];
            const bool zzh = (gk == P.dom_hi[2]) && P.neum[2][1];
            E res[2] = {0, 0};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!o[s]) continue;
                const int rc = ri + s;
                const E pc = s ? Pc.y : Pc.x;
                const E pxl = s ? Pc.x : Sx(slot, row, rc - 1);
                const E pxh = s ? Sx(slot, row, rc + 1) : Pc.y;
                const E pyl = Sx(slot, row - 1, rc), pyh = Sx(slot, row + 1, rc);
                const E gxl = s ? Gx.y : Gx.x, gxh = s ? gx_next : Gx.y;
                const E l = op_point<E>(P, sx, sy, sz, pc, pxl, pxh, pyl, pyh, s ? Pm.y : Pm.x, s ? Pp.y : Pp.x, gxl, gxh,
                                        s ? Gy.y : Gy.x, s ? Gyh.y : Gyh.x, s ? Gzc.y : Gzc.x, s ? Gzp.y : Gzp.x,
                                        s ? Ji.y : Ji.x, zxl[s], zxh[s], zyl, zyh, zzl, zzh);
                res[s] = (MODE != 1) ? ((s ? Rh.y : Rh.x) - l) : l;
            }
            if (MODE == 2) {
                // coarseSum + fine/J, coarseCCJSum + 1.0/J  (MAPPEDAVERAGE2)
                pv[0] = o[0] ? res[0] / Ji.x : E(0);
                pv[1] = o[1] ? res[1] / Ji.y : E(0);
                pv[2] = o[0] ? E(1.0) / Ji.x : E(0);
                pv[3] = o[1] ? E(1.0) / Ji.y : E(0);
                if (volsum) {
                    // fp32 fields: each term and the sum in double
                    if (o[0]) vsum = vsum + dxProduct * (double)pv[2] * (double)Pc.x;
                    if (o[1]) vsum = vsum + dxProduct * (double)pv[3] * (double)Pc.y;
                }
                if (r1 == 2) {
                    E* dstT = Tx(k & 1, row, lane);
                    *reinterpret_cast<E2*>(dstT) = mk2<E>(pv[0], pv[1]);
                    *reinterpret_cast<E2*>(dstT + 2) = mk2<E>(pv[2], pv[3]);
                }
            } else {
                E* dst = out + base + sk * k;
                if (o[0] && o[1]) *reinterpret_cast<E2*>(dst) = mk2<E>(res[0], res[1]);
                else if (o[0]) dst[0] = res[0];
                else dst[1] = res[1];
            }
        }
        Pm = Pc;
        Pc = Pp;
        Gzc = Gzp;
    }
    if (MODE == 2) {
        __syncthreads();
        accumulate(kend - 1);
        if (volsum) {
            __shared__ double red[RM_J];
            for (int o2 = 32; o2 > 0; o2 >>= 1) vsum += __shfl_down(vsum, o2, 64);
            if (threadIdx.x == 0) red[threadIdx.y] = vsum;
            __syncthreads();
            if (threadIdx.x == 0 && threadIdx.y == 0) {
                double tot = red[0];
                for (int q = 1; q < RM_J; ++q) tot = tot + red[q];
                volsum[t.slot] = tot;   // the tile's place in the level's full tile list: split launches (overlap) keep the order of the sum
            }
        }
    }
#undef Sx
#undef Tx
}

template <int MODE, bool UNI = false, class E = double>
// uniform metric, plain output: 64 VGPRs, two workgroups per CU (the narrow classes' per-lane row arithmetic must not cost that)
__global__ __launch_bounds__(64 * RM_J, (UNI && MODE != 2) ? 8 : 4) void k_resid_march(const Tile* __restrict__ tiles,
                                                           const PatchDesc* __restrict__ patches,
                                                           E* __restrict__ out,
                                                           const E* __restrict__ phi,
                                                           const E* __restrict__ rhs,
                                                           const E* __restrict__ jgx,
                                                           const E* __restrict__ jgy,
                                                           const E* __restrict__ jgz,
                                                           const E* __restrict__ jinv, StencilParams P,
                                                           const PatchDesc* __restrict__ cpatches, int r0, int r1,
                                                           int r2, double dxProduct, double* __restrict__ volsum)
{
    __shared__ __attribute__((aligned(16))) E S[2 * RM_J * 160];   // one slot = the largest class's region (16 RM_J rows of 8 + 2)
    // MODE 2: (res/J, 1/J) of both cells of every pair, handed from the odd row of a coarse cell to the even one
    __shared__ __attribute__((aligned(16))) E T[MODE == 2 ? 2 * RM_J * 64 * 4 : 4];
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
    const int cls = t.cls;
    if (cls == 0) resid_march_body<MODE, UNI, 0, E>(S, T, t, p, out, phi, rhs, jgx, jgy, jgz, jinv, P, cpatches, r0, r1, r2, dxProduct, volsum);
    else if (cls == 1) resid_march_body<MODE, UNI, 1, E>(S, T, t, p, out, phi, rhs, jgx, jgy, jgz, jinv, P, cpatches, r0, r1, r2, dxProduct, volsum);
    else resid_march_body<MODE, UNI, 4, E>(S, T, t, p, out, phi, rhs, jgx, jgy, jgz, jinv, P, cpatches, r0, r1, r2, dxProduct, volsum);
}

void launch_resid_march(hipStream_t st, TileSpan tiles, const LevelDev& L, double* out,
                        const double* phi, const double* rhs, int mode)
{
    if (tiles.n == 0) return;
    if (L.P.uniform) {
        if (mode == 0)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_resid_march<0, true>), dim3(tiles.n), dim3(64, RM_J, 1), 0, st, tiles.p, L.patches, out,
                               phi, rhs, L.jg[0], L.jg[1], L.jg[2], L.jinv, L.P, nullptr, 1, 1, 1, 0.0, nullptr);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_resid_march<1, true>), dim3(tiles.n), dim3(64, RM_J, 1), 0, st, tiles.p, L.patches, out,
                               phi, rhs, L.jg[0], L.jg[1], L.jg[2], L.jinv, L.P, nullptr, 1, 1, 1, 0.0, nullptr);
        return;
    }
    if (mode == 0)
        hipLaunchKernelGGL(k_resid_march<0>, dim3(tiles.n), dim3(64, RM_J, 1), 0, st, tiles.p, L.patches, out, phi, rhs,
                           L.jg[0], L.jg[1], L.jg[2], L.jinv, L.P, nullptr, 1, 1, 1, 0.0, nullptr);
    else
        hipLaunchKernelGGL(k_resid_march<1>, dim3(tiles.n), dim3(64, RM_J, 1), 0, st, tiles.p, L.patches, out, phi, rhs,
                           L.jg[0], L.jg[1], L.jg[2], L.jinv, L.P, nullptr, 1, 1, 1, 0.0, nullptr);
}

// restrictResidual in one pass: crse = J-weighted average (MAPPEDAVERAGE2) of rhs - L[phi]; the fine residual is
// never written.  Needs tiles whose k-extent is even (Level::rtiles are) and a coarsenable layout.
// volsum (optional, ntiles doubles): per-block sums of (dxProduct / Jinv) * phi over the block's cells
template <class E>
static void launch_resid_restrict_t(hipStream_t st, TileSpan tiles, const LevelDev& F, const MetricPtrs<E>& M,
                                    const LevelDev& C, E* crse, const E* phi, const E* rhs, const int r[3], double dxProduct,
                                    double* volsum)
{
    if (tiles.n == 0) return;
    if (F.P.uniform) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_resid_march<2, true, E>), dim3(tiles.n), dim3(64, RM_J, 1), 0, st, tiles.p, F.patches, crse, phi,
                           rhs, M.jg[0], M.jg[1], M.jg[2], M.jinv, F.P, C.patches, r[0], r[1], r[2], dxProduct, volsum);
        return;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_resid_march<2, false, E>), dim3(tiles.n), dim3(64, RM_J, 1), 0, st, tiles.p, F.patches, crse, phi, rhs,
                       M.jg[0], M.jg[1], M.jg[2], M.jinv, F.P, C.patches, r[0], r[1], r[2], dxProduct, volsum);
}

void launch_resid_restrict(hipStream_t st, TileSpan tiles, const LevelDev& F, const MetricPtrs<double>& M,
                           const LevelDev& C, double* crse, const double* phi, const double* rhs, const int r[3],
                           double dxProduct, double* volsum)
{
    launch_resid_restrict_t<double>(st, tiles, F, M, C, crse, phi, rhs, r, dxProduct, volsum);
}

void launch_resid_restrict(hipStream_t st, TileSpan tiles, const LevelDev& F, const MetricPtrs<float>& M,
                           const LevelDev& C, float* crse, const float* phi, const float* rhs, const int r[3],
                           double dxProduct, double* volsum)
{
    SOMAR_CHECK(F.P.uniform || (M.jg[0] && M.jg[1] && M.jg[2] && M.jinv),
                "internal: the residual restriction streams the metric of this depth, but its fp32 copies are missing");
    launch_resid_restrict_t<float>(st, tiles, F, M, C, crse, phi, rhs, r, dxProduct, volsum);
}

}  // namespace somar
