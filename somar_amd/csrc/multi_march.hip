// somar_amd/csrc/multi_march.hip -- the k-marching 7-point kernels on NF fields of one level (PressureSolver::
// set_components): the fused red+black sweep, the residual + J-weighted restriction and the plain residual.  One kernel text
// per launch kind, templated on the operator carrier OPS: StencilParams where the fields share ONE operator, FieldOps<NF>
// (kernels.h) where they DIFFER in it (PressureSolver::comp_set_op).
//
// Why: the single-field sweep (gsrb_fused.hip) moves 56 B per cell, of which only 24 belong to the field (phi in, phi out,
// rhs); the other 32 are the metric.  The viscous / diffusive solves of a time step run the same operator on SpaceDim (and
// more) fields, so a launch that carries NF fields streams Jg^xx, Jg^yy, Jg^zz and Jinv once for all of them:
// (24 NF + 32) / NF B per cell and field -- 40 for two fields, 34.7 for three.
//
// Per field the kernels are the single-field ones: the same march, the same LDS staging, the same predicates, and the
// arithmetic of stencil_point.h (gsrb_point, op_point) on the same operands in the same order => bit-identical, field by
// field, to gsrb_fused.hip / resid_march.hip and hence to the CPU oracle.  Only what does not depend on the field is hoisted:
// the coefficient loads, the cell classification, 1 / Jinv of the restriction.
//
// What these forms leave out, because PressureSolver batches no depth that needs it: lane classes other than 0 (the solver
// builds class-0 tables of its own for the batched depths, march_plan.h), the uniform-metric kernels (no coefficient stream
// to share), coarse-fine faces, the mean removal of a zero-average prolongation (in-modes 2 and 4, the fold sums), fp32.
//
// LDS: a sweep stages 3 planes x 16 rows x 128 doubles = 48 KiB per field, so 96 KiB for two fields and 144 KiB for three of
// the 160 KiB a workgroup may declare; four do not fit and run as two launches of two.  Either way one 1024-thread workgroup
// per CU, which is how the single-field 16-row sweep runs (its 48 KiB would admit two, its 16 wavefronts of > 64 VGPRs do not).
//
// Registers, not LDS, decide which forms exist: 1024 threads leave 128 VGPRs per lane.  Built and measured at 512^3
// (profiles/r08_multi.md), then REMOVED because they spilled 108 - 388 B per lane and ran slower per field than the
// single-field sweep: the plain sweep on three fields (+44 %) and the sweep with the prolongation folded in (in-mode 3) on
// two (+20 %) and three (+74 %).  What is instantiated is what measured faster: in-mode 0 on two fields, in-mode 1 (from
// zero) on two and three.  The folded sweep stays single-field until a form that does not spill exists (fewer threads per
// workgroup, or the k-1 plane read back from LDS).
//
// Fields that differ in operator: the sides and alpha / beta are per field (op_of(O, f)), everything else stays shared -- the
// coefficient loads, the memory predicates, 1 / J of the restriction.  Per field vary: the ring predicate of the sweep
// (comp_ij, computed), the Neumann flags of the residual, and what gsrb_point / op_point read of their parameters (the
// classification of a boundary cell, the Dirichlet ghost -own, alpha, beta) -- they are handed field f's StencilParams, so the
// arithmetic is still the one text of stencil_point.h.  NQ = 1 or NF counts the operators; what is per operator is sized
// [NQ] and indexed NQ == 1 ? 0 : f.  DIRI: some field has a Dirichlet side; one without passes the `if (DIRI)` tests unchanged.
//
// The red update is the one place where the text is NOT shared, because its shape alone moves the register allocator
// (profiles/r13_multi_one_text.md section 2; scratch in B per lane, instantiations in the order of the table there):
//   * `update(f)` as a lambda under one ring test (one operator):  12 16 124 108 72 76  ->  8 12 132 104 84 84;
//   * one loop body with `continue` for a field whose ring cell is not computed (several operators):
//     0 0 72 76 60 44 -> 0 0 76 84 24 32, and 127 -> 121 / 120 VGPRs;
//   * the ring test through the `computed` lambda instead of inline (one operator): the same scratch, other SGPR spills.
// Each carrier therefore keeps the shape it was measured with (profiles/r08_multi.md, r12_multi_ops.md), under `if constexpr
// (NQ == 1)`, and all eighteen resource listings equal those of the two separate texts this file used to hold.  A single
// text with the ring test inside the field loop for both carriers spills LESS in ten of the twelve sweeps (section 2 there);
// it is a change of speed to be measured on its own, not part of a merge that promises none.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "stencil_point.h"

namespace somar {

constexpr int MF_J = 16;            // region rows of the sweep (12-row tiles) and of the residual (14-row tiles)
constexpr int LDS_MAX = 160 * 1024; // gfx950: what one workgroup may declare

// The operator carrier OPS of a kernel: StencilParams (one operator for all fields) or FieldOps<NF> (one per field).
__host__ __device__ __forceinline__ const StencilParams& op_of(const StencilParams& P, int) { return P; }
template <int NF>
__host__ __device__ __forceinline__ const StencilParams& op_of(const FieldOps<NF>& O, int f) { return O.P[f]; }

// ---------------------------------------------------------------------------------------------------------------------------
// fused red+black sweep, NF fields.  See gsrb_fused_body (gsrb_fused.hip) for the march; the comments here only mark what is
// per field and what is shared.
// ---------------------------------------------------------------------------------------------------------------------------
template <int INMODE, bool DIRI, int NF, class OPS>
__global__ __launch_bounds__(64 * MF_J) void k_gsrb_fused_nf(const Tile* __restrict__ tiles,
                                                             const PatchDesc* __restrict__ patches, SweepFields<NF> F,
                                                             const double* __restrict__ jgx, const double* __restrict__ jgy,
                                                             const double* __restrict__ jgz, const double* __restrict__ jinv,
                                                             OPS O)
{
    typedef double T;
    typedef double2 T2;
    constexpr int NQ = std::is_same<OPS, StencilParams>::value ? 1 : NF;   // operators of the launch
    const StencilParams& P = op_of(O, 0);   // the level's geometry: the same in every field's parameters
    static_assert(INMODE == 0 || INMODE == 1, "plain, or from zero: the folded prolongation and the mean removal stay single-field");
    static_assert(NF >= 2 && sizeof(T) * NF * 3 * MF_J * 128 <= LDS_MAX, "the staged planes of NF fields must fit the LDS of a workgroup");
    __shared__ __attribute__((aligned(16))) T S[NF * 3 * MF_J * 128];
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
    constexpr int NR = MF_J, PITCH = 128;
#define Sx(f, slot, r, c) S[(((f) * 3 + (slot)) * NR + (r)) * PITCH + (c)]
    const int lane = (int)threadIdx.x;
    const int row = (int)threadIdx.y;
    const int ri = 2 * lane;
    const int li = t.i0 - 2 + ri;
    const int wi = t.w > 0 ? t.w : 124;
    const int lj = t.j0 - 2 + row;
    auto ldphi = [&](int f, int kp, bool ok0, bool ok1) {
        if (INMODE == 1) return mk2<T>(T(0), T(0));
        return ld2(F.in[f], p.off + li + (long long)p.pj * lj + p.pk * kp, ok0, ok1, p.off);
    };
    const int gj = p.lo[1] + lj;
    const T xxS = T(1.0) / (T(P.dx[0]) * T(P.dx[0]));
    const T yyS = T(1.0) / (T(P.dx[1]) * T(P.dx[1]));
    const T zzS = T(1.0) / (T(P.dx[2]) * T(P.dx[2]));

    // ---- shared by the fields: memory predicates, which cells are computed / owned -----------------
    const bool fj = (lj >= -FRAME) && (lj < p.n[1] + FRAME);
    const bool fjh = (lj + 1 >= -FRAME) && (lj + 1 < p.n[1] + FRAME);
    const bool f0 = fj && (li >= -FRAME) && (li < p.n[0] + FRAME) && (ri < wi + 4);
    const bool f1 = fj && (li + 1 >= -FRAME) && (li + 1 < p.n[0] + FRAME) && (ri + 1 < wi + 4);
    const bool cf = (row >= 1) && (row <= NR - 2);
    const bool c0 = f0 && cf, c1 = f1 && cf;
    bool comp_ij[NQ][2], out_ij[2];   // comp_ij: per operator (a ring cell beyond a physical side is not computed)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int l = li + s, g = p.lo[0] + l, r = ri + s;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const StencilParams& Q = op_of(O, q);
            bool cmp = (l >= -1) && (l <= p.n[0]) && (r >= 1) && (r <= wi + 2) && (lj >= -1) && (lj <= p.n[1]) &&
                       (row >= 1) && (row <= NR - 2);
            if ((g < P.dom_lo[0] && (Q.neum[0][0] || (DIRI && Q.diri[0][0]))) ||
                (g > P.dom_hi[0] && (Q.neum[0][1] || (DIRI && Q.diri[0][1]))))
                cmp = false;
            if ((gj < P.dom_lo[1] && (Q.neum[1][0] || (DIRI && Q.diri[1][0]))) ||
                (gj > P.dom_hi[1] && (Q.neum[1][1] || (DIRI && Q.diri[1][1]))))
                cmp = false;
            comp_ij[q][s] = cmp;
        }
        out_ij[s] = (l >= 0) && (l < p.n[0]) && (lj >= 0) && (lj < p.n[1]) && (r >= 2) && (r < wi + 2) &&
                    (row >= 2) && (row < NR - 2);
    }
    const long long sj = p.pj, sk = p.pk;
    const long long base = p.off + li + sj * lj;

    // ---- prologue ----------------------------------------------------------------------------------
    int k = t.k0 - 1;
    bool fk = (k - 1 >= -FRAME) && (k - 1 < p.n[2] + FRAME);
    T2 Pm[NF], Pc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) Pm[f] = ldphi(f, k - 1, f0 && fk, f1 && fk);
    fk = (k >= -FRAME) && (k < p.n[2] + FRAME);
#pragma unroll
    for (int f = 0; f < NF; ++f) Pc[f] = ldphi(f, k, f0 && fk, f1 && fk);
    T2 Gzc = ld2(jgz, base + sk * k, c0 && fk, c1 && fk, p.off);                      // shared
    T b_ji = 1, b_gxl = 0, b_gxh = 0, b_gyl = 0, b_gyh = 0, b_gzl = 0;                 // shared
    T b_rhs[NF], redPrev1[NF], redPrev2[NF];                                           // per field
#pragma unroll
    for (int f = 0; f < NF; ++f) { b_rhs[f] = 0; redPrev1[f] = 0; redPrev2[f] = 0; }

    const int kend = t.k0 + t.nk;
    auto step = [&](auto CC) {
        constexpr int c = decltype(CC)::value;
        const int gk = p.lo[2] + k;
        fk = (k >= -FRAME) && (k < p.n[2] + FRAME);
        const bool fkp = (k + 1 >= -FRAME) && (k + 1 < p.n[2] + FRAME);
        // ---- loads: per field phi of plane k+1 and rhs of plane k; ONCE the coefficients ------------
        T2 Pp[NF], Rh[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            Pp[f] = ldphi(f, k + 1, f0 && fkp, f1 && fkp);
            Rh[f] = ld2(F.rhs[f], base + sk * k, c0 && fk, c1 && fk, p.off);
        }
        const T2 Gzp = ld2(jgz, base + sk * (k + 1), c0 && fkp, c1 && fkp, p.off);
        const T2 Ji = ld2(jinv, base + sk * k, c0 && fk, c1 && fk, p.off);
        const T2 Gx = ld2(jgx, base + sk * k, c0 && fk, c1 && fk, p.off);
        const T2 Gy = ld2(jgy, base + sk * k, c0 && fk, c1 && fk, p.off);
        const T2 Gyh = ld2(jgy, base + sk * k + sj, c0 && fk && fjh, c1 && fk && fjh, p.off);
        const T gx_next = __shfl_down(Gx.x, 1, 64);

        // ---- stage plane k of every field; ONE barrier per plane ------------------------------------
        const int slot = ((k % 3) + 3) % 3;
#pragma unroll
        for (int f = 0; f < NF; ++f) *reinterpret_cast<T2*>(&Sx(f, slot, row, ri)) = Pc[f];
        __syncthreads();

        // ---- red(k) at column c ---------------------------------------------------------------------
        const int rc = ri + c;
        T red[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) red[f] = pick<T>(Pc[f], c);
        // TWO TEXTS of one update, on purpose (header: "The red update"; profiles/r13_multi_one_text.md section 2): one
        // operator tests the ring once, inline, around the field loop; several test it per field through two lambdas.  A fix
        // to either goes into both.
        {
            if constexpr (NQ == 1) {
                bool comp = comp_ij[0][c] && (k >= -1) && (k <= p.n[2]);
                if ((gk < P.dom_lo[2] && (P.neum[2][0] || (DIRI && P.diri[2][0]))) ||
                    (gk > P.dom_hi[2] && (P.neum[2][1] || (DIRI && P.diri[2][1]))))
                    comp = false;
                if (comp) {
#pragma unroll
                    for (int f = 0; f < NF; ++f) {
                        const T pxl = Sx(f, slot, row, rc - 1), pxh = Sx(f, slot, row, rc + 1);
                        const T pyl = Sx(f, slot, row - 1, rc), pyh = Sx(f, slot, row + 1, rc);
                        red[f] = gsrb_point<DIRI, false, T>(P, xxS, yyS, zzS, p.lo[0] + li + c, gj, gk, pxl, pxh, pyl, pyh,
                                                            pick<T>(Pm[f], c), pick<T>(Pp[f], c), c ? Gx.y : Gx.x, c ? gx_next : Gx.y,
                                                            pick<T>(Gy, c), pick<T>(Gyh, c), pick<T>(Gzc, c), pick<T>(Gzp, c),
                                                            pick<T>(Ji, c), pick<T>(Rh[f], c), red[f]);
                        Sx(f, slot, row, rc) = red[f];
                    }
                }
            } else {
                // is the ring cell computed under operator q (the ring cells beyond a physical side are not)
                auto computed = [&](int q) {
                    const StencilParams& Q = op_of(O, q);
                    bool comp = comp_ij[q][c] && (k >= -1) && (k <= p.n[2]);
                    if ((gk < P.dom_lo[2] && (Q.neum[2][0] || (DIRI && Q.diri[2][0]))) ||
                        (gk > P.dom_hi[2] && (Q.neum[2][1] || (DIRI && Q.diri[2][1]))))
                        comp = false;
                    return comp;
                };
                auto update = [&](int f) {
                    const T pxl = Sx(f, slot, row, rc - 1), pxh = Sx(f, slot, row, rc + 1);
                    const T pyl = Sx(f, slot, row - 1, rc), pyh = Sx(f, slot, row + 1, rc);
                    red[f] = gsrb_point<DIRI, false, T>(op_of(O, f), xxS, yyS, zzS, p.lo[0] + li + c, gj, gk, pxl, pxh, pyl, pyh,
                                                        pick<T>(Pm[f], c), pick<T>(Pp[f], c), c ? Gx.y : Gx.x, c ? gx_next : Gx.y,
                                                        pick<T>(Gy, c), pick<T>(Gyh, c), pick<T>(Gzc, c), pick<T>(Gzp, c),
                                                        pick<T>(Ji, c), pick<T>(Rh[f], c), red[f]);
                    Sx(f, slot, row, rc) = red[f];
                };
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    if (computed(f)) update(f);
            }
        }

        // ---- black(k-1) at the same column c ----------------------------------------------------------
        {
            const int kb = k - 1;
            if ((kb >= t.k0) && (kb < t.k0 + t.nk) && (out_ij[0] || out_ij[1])) {
                const int sb = ((kb % 3) + 3) % 3;
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    T black = 0;
                    if (out_ij[c]) {
                        const T pxl = Sx(f, sb, row, rc - 1), pxh = Sx(f, sb, row, rc + 1);
                        const T pyl = Sx(f, sb, row - 1, rc), pyh = Sx(f, sb, row + 1, rc);
                        black = gsrb_point<DIRI, false, T>(op_of(O, f), xxS, yyS, zzS, p.lo[0] + li + c, gj, p.lo[2] + kb, pxl, pxh, pyl,
                                                           pyh, redPrev2[f], red[f], b_gxl, b_gxh, b_gyl, b_gyh, b_gzl,
                                                           pick<T>(Gzc, c), b_ji, b_rhs[f], Sx(f, sb, row, rc));
                    }
                    T* dst = F.out[f] + base + sk * kb;
                    const T ox = c ? redPrev1[f] : black, oy = c ? black : redPrev1[f];
                    if (out_ij[0] && out_ij[1]) *reinterpret_cast<T2*>(dst) = mk2<T>(ox, oy);
                    else if (out_ij[0]) dst[0] = ox;
                    else dst[1] = oy;
                }
            }
        }

        // ---- rotate -----------------------------------------------------------------------------------
        {
            const int cb = c ^ 1;
            b_ji = pick<T>(Ji, cb);
            b_gxl = cb ? Gx.y : Gx.x;
            b_gxh = cb ? gx_next : Gx.y;
            b_gyl = pick<T>(Gy, cb);
            b_gyh = pick<T>(Gyh, cb);
            b_gzl = pick<T>(Gzc, cb);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                b_rhs[f] = pick<T>(Rh[f], cb);
                redPrev2[f] = redPrev1[f];
                redPrev1[f] = red[f];
                Pm[f] = Pc[f];
                Pc[f] = Pp[f];
            }
        }
        Gzc = Gzp;
    };
    const int cfirst = __builtin_amdgcn_readfirstlane((p.lo[0] + li + gj + p.lo[2] + k) & 1);
    if (cfirst) {
        for (;;) {
            if (k > kend) break;
            step(std::integral_constant<int, 1>{});
            ++k;
            if (k > kend) break;
            step(std::integral_constant<int, 0>{});
            ++k;
        }
    } else {
        for (;;) {
            if (k > kend) break;
            step(std::integral_constant<int, 0>{});
            ++k;
            if (k > kend) break;
            step(std::integral_constant<int, 1>{});
            ++k;
        }
    }
#undef Sx
}

template <int NF, class OPS>
void launch_gsrb_fused_nf(hipStream_t st, TileSpan tiles, const LevelDev& L, const SweepFields<NF>& F, const OPS& O, int in_mode)
{
    constexpr int NQ = std::is_same<OPS, StencilParams>::value ? 1 : NF;
    if (tiles.n == 0) return;
    SOMAR_CHECK(tiles.classes == 0 && L.fused_rows == MF_J && !op_of(O, 0).uniform,
                "internal: the N-field sweep takes class-0 tiles of the 16-row form on a streamed metric");
    SOMAR_CHECK(in_mode == 1 || (in_mode == 0 && NF == 2),
                "internal: the N-field sweep is built plain on two fields and from zero on two and three");
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(tiles.n), dim3(64, MF_J, 1), 0, st, tiles.p, L.patches, F, L.jg[0], L.jg[1], L.jg[2],
                           L.jinv, O);
    };
    bool diri = false;   // DIRI: some field has a Dirichlet side; one without passes through the `if (DIRI)` tests unchanged
    for (int q = 0; q < NQ; ++q)
        for (int d = 0; d < 3; ++d) diri = diri || op_of(O, q).diri[d][0] || op_of(O, q).diri[d][1];
    if (in_mode == 1) {
        if (diri) go(k_gsrb_fused_nf<1, true, NF, OPS>);
        else go(k_gsrb_fused_nf<1, false, NF, OPS>);
    } else if constexpr (NF == 2) {
        if (diri) go(k_gsrb_fused_nf<0, true, NF, OPS>);
        else go(k_gsrb_fused_nf<0, false, NF, OPS>);
    }
}
template void launch_gsrb_fused_nf<2>(hipStream_t, TileSpan, const LevelDev&, const SweepFields<2>&, const StencilParams&, int);
template void launch_gsrb_fused_nf<3>(hipStream_t, TileSpan, const LevelDev&, const SweepFields<3>&, const StencilParams&, int);
template void launch_gsrb_fused_nf<2>(hipStream_t, TileSpan, const LevelDev&, const SweepFields<2>&, const FieldOps<2>&, int);
template void launch_gsrb_fused_nf<3>(hipStream_t, TileSpan, const LevelDev&, const SweepFields<3>&, const FieldOps<3>&, int);

// ---------------------------------------------------------------------------------------------------------------------------
// residual (MODE 0: out = rhs - L[phi]) and residual + J-weighted restriction (MODE 2: crse = MAPPEDAVERAGE2 of it), NF
// fields.  See resid_march_body (resid_march.hip).  MODE 2 hands (res / J) of every field and (1 / J) once from the odd row
// of a coarse cell to the even one through LDS: the tiles start on even rows, so only the even region rows are kept.
// LDS: 2 planes x 16 x 128 doubles = 32 KiB per field, MODE 2 plus 16 KiB per field and 16 KiB shared: 112 KiB for two fields
// (MODE 2 is instantiated for two fields only: launch_resid_nf).
// ---------------------------------------------------------------------------------------------------------------------------
template <int MODE, int NF, class OPS>
__global__ __launch_bounds__(64 * MF_J) void k_resid_march_nf(const Tile* __restrict__ tiles,
                                                              const PatchDesc* __restrict__ patches, ResidFields<NF> F,
                                                              const double* __restrict__ jgx, const double* __restrict__ jgy,
                                                              const double* __restrict__ jgz, const double* __restrict__ jinv,
                                                              OPS O, const PatchDesc* __restrict__ cpatches, int r0,
                                                              int r1, int r2)
{
    typedef double E;
    typedef double2 E2;
    constexpr int NQ = std::is_same<OPS, StencilParams>::value ? 1 : NF;   // operators of the launch
    const StencilParams& P = op_of(O, 0);   // the level's geometry: the same in every field's parameters
    static_assert(MODE == 0 || MODE == 2, "residual, or residual + restriction");
    constexpr int NR = MF_J, PITCH = 128, LPR = 64;
    constexpr int TN = MODE == 2 ? 2 * (NR / 2) * LPR * 2 : 2;   // doubles per handed-over quantity: 2 slots x 8 rows x 64 pairs
    static_assert(NF >= 2 && sizeof(E) * (NF * 2 * NR * PITCH + (MODE == 2 ? (NF + 1) * TN : 0)) <= LDS_MAX,
                  "the staged planes of NF fields must fit the LDS of a workgroup");
    __shared__ __attribute__((aligned(16))) E S[NF * 2 * NR * PITCH];
    __shared__ __attribute__((aligned(16))) E TR[NF * TN];   // res / J of both cells of a pair, per field
    __shared__ __attribute__((aligned(16))) E TJ[TN];        // 1 / J of both cells: the same for every field
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
#define Sx(f, slot, r, c) S[(((f) * 2 + (slot)) * NR + (r)) * PITCH + (c)]
#define Tix(slot, r, l) (((((slot) * (NR / 2) + ((r) >> 1)) * LPR + (l)) << 1))
    const int lane = (int)threadIdx.x;
    const int row = (int)threadIdx.y;
    const int ri = 2 * lane;
    const int li = t.i0 - 2 + ri;
    const int wi = t.w > 0 ? t.w : 124;
    const int lj = t.j0 - 1 + row;
    const int gj = p.lo[1] + lj;
    const E sx = E(1.0) / E(P.dx[0]), sy = E(1.0) / E(P.dx[1]), sz = E(1.0) / E(P.dx[2]);

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
    const int left_o1 = __shfl_up((int)o[1], 1, 64);
    const bool gxo0 = o[0] || (left_o1 != 0);
    const bool any = o[0] || o[1];
    const long long sj = p.pj, sk = p.pk;
    const long long base = p.off + li + sj * lj;
    bool zyl[NQ], zyh[NQ], zxl[NQ][2], zxh[NQ][2];   // Neumann faces: per operator
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const StencilParams& Q = op_of(O, q);
        zyl[q] = (gj == P.dom_lo[1]) && Q.neum[1][0];
        zyh[q] = (gj == P.dom_hi[1]) && Q.neum[1][1];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int gi = p.lo[0] + li + s;
            zxl[q][s] = (gi == P.dom_lo[0]) && Q.neum[0][0];
            zxh[q][s] = (gi == P.dom_hi[0]) && Q.neum[0][1];
        }
    }

    // MODE 2 state: (res / J) of the previous plane and the running sums per field; (1 / J) and its sums once
    E pvr[NF][2], cs[NF][2];
    E pvj[2] = {0, 0}, cjs[2] = {0, 0};
#pragma unroll
    for (int f = 0; f < NF; ++f) { pvr[f][0] = pvr[f][1] = 0; cs[f][0] = cs[f][1] = 0; }
    const bool leader = (MODE == 2) && any && (r1 == 1 || ((lj & 1) == 0));
    auto accumulate = [&](int kp) {
        // MAPPEDAVERAGE2's loop order: ii2 (planes), ii1 (rows), ii0 (cells of the pair)
        if (!leader) return;
        const bool first = (r2 == 1) || ((kp & 1) == 0);
        const bool last = (r2 == 1) || ((kp & 1) == 1);
        E qj[2] = {0, 0};
        if (r1 == 2) { const E* src = TJ + Tix(kp & 1, row + 1, lane); qj[0] = src[0]; qj[1] = src[1]; }
        if (first) cjs[0] = cjs[1] = 0;
        if (r0 == 2) {
            cjs[0] = cjs[0] + pvj[0];
            cjs[0] = cjs[0] + pvj[1];
            if (r1 == 2) { cjs[0] = cjs[0] + qj[0]; cjs[0] = cjs[0] + qj[1]; }
        } else {
            cjs[0] = cjs[0] + pvj[0];
            cjs[1] = cjs[1] + pvj[1];
            if (r1 == 2) { cjs[0] = cjs[0] + qj[0]; cjs[1] = cjs[1] + qj[1]; }
        }
        const PatchDesc cp = cpatches[t.patch];
        const long long c = cp.off + (li / r0) + (long long)cp.pj * (lj / r1) + cp.pk * (kp / r2);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (first) cs[f][0] = cs[f][1] = 0;
            E q[2] = {0, 0};
            if (r1 == 2) { const E* src = TR + f * TN + Tix(kp & 1, row + 1, lane); q[0] = src[0]; q[1] = src[1]; }
            if (r0 == 2) {
                cs[f][0] = cs[f][0] + pvr[f][0];
                cs[f][0] = cs[f][0] + pvr[f][1];
                if (r1 == 2) { cs[f][0] = cs[f][0] + q[0]; cs[f][0] = cs[f][0] + q[1]; }
            } else {
                cs[f][0] = cs[f][0] + pvr[f][0];
                cs[f][1] = cs[f][1] + pvr[f][1];
                if (r1 == 2) { cs[f][0] = cs[f][0] + q[0]; cs[f][1] = cs[f][1] + q[1]; }
            }
            if (last) {
                if (r0 == 2) {
                    F.out[f][c] = cs[f][0] / cjs[0];
                } else {
                    if (o[0]) F.out[f][c] = cs[f][0] / cjs[0];
                    if (o[1]) F.out[f][c + 1] = cs[f][1] / cjs[1];
                }
            }
        }
    };

    int k = t.k0;
    E2 Pm[NF], Pc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        Pm[f] = ld2(F.phi[f], base + sk * (k - 1), o[0], o[1], p.off);
        Pc[f] = ld2(F.phi[f], base + sk * k, f0, f1, p.off);
    }
    E2 Gzc = ld2(jgz, base + sk * k, o[0], o[1], p.off);
    const int kend = t.k0 + t.nk;
    for (; k < kend; ++k) {
        const int gk = p.lo[2] + k;
        const bool more = (k + 1 < kend);
        // ---- loads: per field phi of plane k+1 and rhs of plane k; ONCE the coefficients ----
        E2 Pp[NF], Rh[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            Pp[f] = ld2(F.phi[f], base + sk * (k + 1), more ? f0 : o[0], more ? f1 : o[1], p.off);
            Rh[f] = ld2(F.rhs[f], base + sk * k, o[0], o[1], p.off);
        }
        const E2 Gzp = ld2(jgz, base + sk * (k + 1), o[0], o[1], p.off);
        const E2 Ji = ld2(jinv, base + sk * k, o[0], o[1], p.off);
        const E2 Gx = ld2(jgx, base + sk * k, gxo0, o[0] || o[1], p.off);
        const E2 Gy = ld2(jgy, base + sk * k, o[0], o[1], p.off);
        const E2 Gyh = ld2(jgy, base + sk * k + sj, o[0], o[1], p.off);
        const E gx_next = __shfl_down(Gx.x, 1, 64);

        const int slot = k & 1;
#pragma unroll
        for (int f = 0; f < NF; ++f) *reinterpret_cast<E2*>(&Sx(f, slot, row, ri)) = Pc[f];
        __syncthreads();
        if (MODE == 2 && k > t.k0) accumulate(k - 1);

        if (any) {
            bool zzl[NQ], zzh[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                zzl[q] = (gk == P.dom_lo[2]) && op_of(O, q).neum[2][0];
                zzh[q] = (gk == P.dom_hi[2]) && op_of(O, q).neum[2][1];
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const int q = NQ == 1 ? 0 : f;   // field f's flag set
                E res[2] = {0, 0};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (!o[s]) continue;
                    const int rc = ri + s;
                    const E pc = s ? Pc[f].y : Pc[f].x;
                    const E pxl = s ? Pc[f].x : Sx(f, slot, row, rc - 1);
                    const E pxh = s ? Sx(f, slot, row, rc + 1) : Pc[f].y;
                    const E pyl = Sx(f, slot, row - 1, rc), pyh = Sx(f, slot, row + 1, rc);
                    const E gxl = s ? Gx.y : Gx.x, gxh = s ? gx_next : Gx.y;
                    const E l = op_point<E>(op_of(O, f), sx, sy, sz, pc, pxl, pxh, pyl, pyh, s ? Pm[f].y : Pm[f].x,
                                            s ? Pp[f].y : Pp[f].x, gxl, gxh, s ? Gy.y : Gy.x, s ? Gyh.y : Gyh.x, s ? Gzc.y : Gzc.x,
                                            s ? Gzp.y : Gzp.x, s ? Ji.y : Ji.x, zxl[q][s], zxh[q][s], zyl[q], zyh[q], zzl[q], zzh[q]);
                    res[s] = (s ? Rh[f].y : Rh[f].x) - l;
                }
                if (MODE == 2) {
                    // coarseSum + fine/J  (MAPPEDAVERAGE2)
                    pvr[f][0] = o[0] ? res[0] / Ji.x : E(0);
                    pvr[f][1] = o[1] ? res[1] / Ji.y : E(0);
                    if (r1 == 2 && !(row & 1)) *reinterpret_cast<E2*>(TR + f * TN + Tix(slot, row, lane)) = mk2<E>(pvr[f][0], pvr[f][1]);
                } else {
                    E* dst = F.out[f] + base + sk * k;
                    if (o[0] && o[1]) *reinterpret_cast<E2*>(dst) = mk2<E>(res[0], res[1]);
                    else if (o[0]) dst[0] = res[0];
                    else dst[1] = res[1];
                }
            }
            if (MODE == 2) {
                // coarseCCJSum + 1.0/J
                pvj[0] = o[0] ? E(1.0) / Ji.x : E(0);
                pvj[1] = o[1] ? E(1.0) / Ji.y : E(0);
                if (r1 == 2 && !(row & 1)) *reinterpret_cast<E2*>(TJ + Tix(slot, row, lane)) = mk2<E>(pvj[0], pvj[1]);
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) { Pm[f] = Pc[f]; Pc[f] = Pp[f]; }
        Gzc = Gzp;
    }
    if (MODE == 2) {
        __syncthreads();
        accumulate(kend - 1);
    }
#undef Sx
#undef Tix
}

template <int NF, class OPS>
void launch_resid_nf(hipStream_t st, TileSpan tiles, const LevelDev& F, const ResidFields<NF>& fields, const OPS& O,
                     const LevelDev* C, const int* r)
{
    if (tiles.n == 0) return;
    SOMAR_CHECK(tiles.classes == 0 && !op_of(O, 0).uniform, "internal: the N-field residual takes class-0 tiles on a streamed metric");
    if (!C) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_resid_march_nf<0, NF, OPS>), dim3(tiles.n), dim3(64, MF_J, 1), 0, st, tiles.p,
                           F.patches, fields, F.jg[0], F.jg[1], F.jg[2], F.jinv, O, nullptr, 1, 1, 1);
        return;
    }
    SOMAR_CHECK(r && (r[0] == 1 || r[0] == 2) && (r[1] == 1 || r[1] == 2) && (r[2] == 1 || r[2] == 2),
                "internal: the marching restriction takes multigrid ratios of 1 or 2 per direction");
    // two fields: with three the staged planes and the handed-over rows fill the LDS to the last byte (and the kernel spills)
    if constexpr (NF == 2)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_resid_march_nf<2, NF, OPS>), dim3(tiles.n), dim3(64, MF_J, 1), 0, st, tiles.p,
                           F.patches, fields, F.jg[0], F.jg[1], F.jg[2], F.jinv, O, C->patches, r[0], r[1], r[2]);
    else
        SOMAR_CHECK(NF == 2, "internal: the residual + restriction carries two fields per launch");
}
template void launch_resid_nf<2>(hipStream_t, TileSpan, const LevelDev&, const ResidFields<2>&, const StencilParams&, const LevelDev*,
                                 const int*);
template void launch_resid_nf<3>(hipStream_t, TileSpan, const LevelDev&, const ResidFields<3>&, const StencilParams&, const LevelDev*,
                                 const int*);
template void launch_resid_nf<2>(hipStream_t, TileSpan, const LevelDev&, const ResidFields<2>&, const FieldOps<2>&, const LevelDev*,
                                 const int*);
template void launch_resid_nf<3>(hipStream_t, TileSpan, const LevelDev&, const ResidFields<3>&, const FieldOps<3>&, const LevelDev*,
                                 const int*);

}  // namespace somar
