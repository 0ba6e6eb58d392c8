// somar_amd/csrc/full19_multi.hip -- the k-marching 19-point residual and GSRB colour pass (full19_march.hip) on NF fields of
// one level (PressureSolver::set_components_full): MODE 0 (out = rhs - L[phi]) and MODE 2 (one colour pass into the other buffer).
//
// Why: by full19_march.hip's accounting a pass moves about 106 B per cell, of which 80 are coefficients (nine J g^{ab} planes
// and Jinv) and 26 belong to the field.  The viscous / diffusive solves of a time step run the same operator on SpaceDim (and
// more) fields, so a launch that carries NF fields streams the 80 B once: (80 + 26 NF) / NF B per cell and field -- 66 for two
// fields, 53 for three (computed; what was measured is in profiles/r14_multi_full19.md).
//
// Per field the kernel is the single-field one: the same k-march, the same four rotating plane slots of phi and of E (phi inside
// the box, psi in its one-cell frame) staged per field, the same predicates, and the per-cell arithmetic of full19_point.h on
// the same operands => bit-identical, field by field, to full19_march.hip BECAUSE both take that text.  Only what does not depend on the field is
// hoisted, loaded or computed once per plane and held in registers while the fields take their turns: the thirteen coefficient
// loads (ten with ZXY) and the shuffles of the x-face components, the carried k-face planes, Jinv, the memory and ownership
// predicates, the colour selector, the boundary classification and the scale constants.  Every field of a launch shares one
// StencilParams: a component with an operator of its own is not offered on a non-diagonal metric (comp_set_op).
//
// Left out, because PressureSolver batches no depth that needs it: MODE 1 and MODE 3, lane classes other than 0 (the solver
// builds class-0 tables of its own for the batched depths, march_plan.h).
//
// LDS per field: 2 arrays x 4 slots x FM_J rows x 128 doubles = FM_J x 8 KiB; a workgroup may declare 160 KiB:
//   2 fields at 8 rows (512 threads) 128 KiB;  3 fields at 6 rows (384 threads) 144 KiB;  3 fields at 8 rows would need 192.
// Only the two-field form is instantiated: the three-field one measured slower per field than the single-field kernel
// // (profiles/r14_multi_full19.md; a build with -DSOMAR_FULL19_NF3 has it, for that measurement).  Three fields run as 2 + 1,
// four as 2 + 2.  One workgroup per CU either way, two wavefronts per SIMD: a budget of 256 VGPRs, which every instantiation
// keeps without scratch (the resource listing is in profiles/r14_multi_full19.md).
#include "common.h"
#include "kernels.h"
#include "stencil_point.h"
#include "full19_point.h"

namespace somar {

namespace {

constexpr int FN_S = 4;              // plane slots, as full19_march.hip's FM_S
constexpr int FN_LDS_MAX = 160 * 1024;   // gfx950: what one workgroup may declare (LDS_MAX of multi_march.hip)

// The kernel's own argument type, in this unnamed namespace ON PURPOSE: it gives k_full_march_nf internal linkage, the form
// it was measured in.  With the shared JgFull of kernels.h as the argument the residual kernel ran 0.7 % slower
// (profiles/r16_full19_one_text.md, section 3).  Filled from jgfull(L).
struct JgFullN { const double* c[3][3]; };

}  // namespace

// MODE 0: out[f] = rhs[f] - L[phi[f]]   MODE 2: out[f] = phi[f] with the cells of `color` relaxed (one GSRB pass)
// ZXY: as in k_full_march.  Class-0 tiles: one 128-column region row per wavefront, the row index a scalar.
template <int MODE, int FM_J, bool ZXY, int NF>
__global__ __launch_bounds__(64 * FM_J) void k_full_march_nf(const Tile* __restrict__ tiles, const PatchDesc* __restrict__ patches,
                                                             FullFields<NF> F, JgFullN J, const double* __restrict__ jinv,
                                                             StencilParams P, int color)
{
    static_assert(MODE == 0 || MODE == 2, "the residual, or one colour pass: the operator alone and the shell pass stay single-field");
    static_assert(NF >= 2 && sizeof(double) * NF * 2 * FN_S * FM_J * 128 <= FN_LDS_MAX,
                  "the staged planes of NF fields must fit the LDS of a workgroup");
    constexpr int NR = FM_J, PITCH = 128;
    __shared__ __attribute__((aligned(16))) double SP[NF * FN_S * NR * PITCH];  // phi
    __shared__ __attribute__((aligned(16))) double SE[NF * FN_S * NR * PITCH];  // E: phi inside the box, psi in its frame
#define SPx(f, slot, r, c) SP[(((f) * FN_S + (slot)) * NR + (r)) * PITCH + (c)]
#define SEx(f, slot, r, c) SE[(((f) * FN_S + (slot)) * NR + (r)) * PITCH + (c)]
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
    const int lane = (int)threadIdx.x;
    const int row = (int)threadIdx.y;
    const int ri = 2 * lane;
    const int li = t.i0 - 2 + ri;  // even: rows are 16-byte aligned
    const int wi = t.w > 0 ? t.w : 124;
    const int lj = t.j0 - 1 + row;
    const int gj = p.lo[1] + lj;

    // ---- shared by the fields: memory and ownership predicates (full_march_body's) --------------------------------------
    const bool fj = (lj >= -1) && (lj <= p.n[1]);
    const bool f0 = fj && (li >= -1) && (li <= p.n[0]) && (ri < wi + 4);
    const bool f1 = fj && (li + 1 >= -1) && (li + 1 <= p.n[0]) && (ri + 1 < wi + 4);
    const bool inj = (lj >= 0) && (lj < p.n[1]);
    const bool in0 = inj && (li >= 0) && (li < p.n[0]);          // inside the box (in i, j): E = phi there
    const bool in1 = inj && (li + 1 >= 0) && (li + 1 < p.n[0]);
    const bool own_j = inj && (row >= 1) && (row <= NR - 2) && (lj < t.j0 + (NR - 2));
    bool o[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int l = li + s, r = ri + s;
        o[s] = own_j && (l >= 0) && (l < p.n[0]) && (r >= 2) && (r < wi + 2);
    }
    const int left_o1 = __shfl_up((int)o[1], 1, 64);   // all lanes active here
    const bool gxo0 = o[0] || (left_o1 != 0);           // my first x-face is the high face of the left lane's second cell
    const bool any = o[0] || o[1];
    const long long sj = p.pj, sk = p.pk;
    const long long base = p.off + li + sj * lj;
    const Full19Scales S = full19_scales(P.dx[0], P.dx[1], P.dx[2]);

    // ---- per field: stage plane kp of phi and E into its slot -----------------------------------------------------------
    auto load_plane = [&](int f, int kp, double2& vp, double2& ve) {
        const bool fk = (kp >= -1) && (kp <= p.n[2]);
        const bool ink = (kp >= 0) && (kp < p.n[2]);
        const long long idx = base + sk * kp;
        vp = ld2<double>(F.phi[f], idx, f0 && fk, f1 && fk, p.off);
        const bool e0 = f0 && fk && !(in0 && ink), e1 = f1 && fk && !(in1 && ink);   // frame cells: E = psi
        const double2 vs = ld2<double>(F.psi[f], idx, e0, e1, p.off);
        ve = make_double2(e0 ? vs.x : vp.x, e1 ? vs.y : vp.y);
    };
    auto store_plane = [&](int f, int kp, const double2& vp, const double2& ve) {
        const int slot = kp & (FN_S - 1);
        *reinterpret_cast<double2*>(&SPx(f, slot, row, ri)) = vp;
        *reinterpret_cast<double2*>(&SEx(f, slot, row, ri)) = ve;
    };

    int k = t.k0;
    const int kend = t.k0 + t.nk;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        double2 vp, ve;
        load_plane(f, k - 1, vp, ve);
        store_plane(f, k - 1, vp, ve);
        load_plane(f, k, vp, ve);
        store_plane(f, k, vp, ve);
    }
    // k-face components on the LOW face of plane k (shared, carried from plane to plane)
    double2 Jz0c = ld2<double>(J.c[2][0], base + sk * k, o[0], o[1], p.off);
    double2 Jz1c = ld2<double>(J.c[2][1], base + sk * k, o[0], o[1], p.off);
    double2 Jz2c = ld2<double>(J.c[2][2], base + sk * k, o[0], o[1], p.off);

    for (; k < kend; ++k) {
        const int gk = p.lo[2] + k;
        // ---- this step's loads: phi / psi of plane k+1 and rhs of plane k per field, the coefficients of plane k once ----
        double2 vp[NF], ve[NF], Rh[NF];
        const long long ck = base + sk * k;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            load_plane(f, k + 1, vp[f], ve[f]);
            Rh[f] = ld2<double>(F.rhs[f], ck, o[0], o[1], p.off);
        }
        const double2 Jz0p = ld2<double>(J.c[2][0], ck + sk, o[0], o[1], p.off);
        const double2 Jz1p = ld2<double>(J.c[2][1], ck + sk, o[0], o[1], p.off);
        const double2 Jz2p = ld2<double>(J.c[2][2], ck + sk, o[0], o[1], p.off);
        const double2 Ji = ld2<double>(jinv, ck, o[0], o[1], p.off);
        const double2 Jx0 = ld2<double>(J.c[0][0], ck, gxo0, any, p.off);
        const double2 Jx1 = ZXY ? make_double2(0.0, 0.0) : ld2<double>(J.c[0][1], ck, gxo0, any, p.off);
        const double2 Jx2 = ld2<double>(J.c[0][2], ck, gxo0, any, p.off);
        const double2 Jy0 = ZXY ? make_double2(0.0, 0.0) : ld2<double>(J.c[1][0], ck, o[0], o[1], p.off);
        const double2 Jy1 = ld2<double>(J.c[1][1], ck, o[0], o[1], p.off);
        const double2 Jy2 = ld2<double>(J.c[1][2], ck, o[0], o[1], p.off);
        const double2 Jy0h = ZXY ? make_double2(0.0, 0.0) : ld2<double>(J.c[1][0], ck + sj, o[0], o[1], p.off);
        const double2 Jy1h = ld2<double>(J.c[1][1], ck + sj, o[0], o[1], p.off);
        const double2 Jy2h = ld2<double>(J.c[1][2], ck + sj, o[0], o[1], p.off);
        const double jx0n = __shfl_down(Jx0.x, 1, 64), jx1n = __shfl_down(Jx1.x, 1, 64), jx2n = __shfl_down(Jx2.x, 1, 64);

#pragma unroll
        for (int f = 0; f < NF; ++f) store_plane(f, k + 1, vp[f], ve[f]);
        __syncthreads();

        if (any) {
            const int sm = (k - 1) & (FN_S - 1), sc = k & (FN_S - 1), sp = (k + 1) & (FN_S - 1);
            const int csel = (p.lo[0] + li + gj + gk + color) & 1;   // MODE 2: the cell of the pair that has this colour
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                double res[2] = {0.0, 0.0};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int rc = ri + s;
                    const double pc = SPx(f, sc, row, rc);
                    if (MODE == 2 && s != csel) { res[s] = pc; continue; }
                    if (!o[s]) continue;
                    const int gi = p.lo[0] + li + s;
                    // neighbours: Pn(di,dj,dk) = phi, En(di,dj,dk) = E
#define Pn(di, dj, dk) SPx(f, (dk) < 0 ? sm : ((dk) > 0 ? sp : sc), row + (dj), rc + (di))
#define En(di, dj, dk) SEx(f, (dk) < 0 ? sm : ((dk) > 0 ? sp : sc), row + (dj), rc + (di))
#define CF(n) C.n
#define SC(n) S.n
#define NEU(f) FULL19_NF(f)
#define F19_RESULT(v) res[s] = v
                    // full19_point.inc in place reads, from this scope: C and S (through CF, SC), alpha, beta, pc (operator) or rh (updates),
                    // and P, gi, gj, gk (through FULL19_NF / FULL19_ONB); FULL19_PICK reads Jx0..Jx2, jx0n..jx2n, Jy0..Jy2h, Jz0c..Jz2p, Ji
                    // coefficients on the low / high face of this cell
                    Full19Coef C;
                    FULL19_PICK(C, s);
                    const double alpha = P.alpha, beta = P.beta;
                    if (MODE == 0) {
#define FULL19_PART 1
#include "full19_point.inc"
                        res[s] = pick<double>(Rh[f], s) - l;
                    } else {
                        const bool onb = FULL19_ONB;
                        const double rh = pick<double>(Rh[f], s);
                        if (!onb) {
#define FULL19_PART 2
#include "full19_point.inc"
                        } else {
#define FULL19_PART 3
#include "full19_point.inc"
                        }
                    }
#undef Pn
#undef En
#undef CF
#undef SC
#undef NEU
#undef F19_RESULT
                }
                double* dst = F.out[f] + base + sk * k;
                if (o[0] && o[1]) *reinterpret_cast<double2*>(dst) = make_double2(res[0], res[1]);
                else if (o[0]) dst[0] = res[0];
                else dst[1] = res[1];
            }
        }
        Jz0c = Jz0p;
        Jz1c = Jz1p;
        Jz2c = Jz2p;
    }
#undef SPx
#undef SEx
}

// The form that ships (profiles/r14_multi_full19.md): two fields at 8 region rows.  Three fields at 6 rows were measured at
// 512^3 and lost per field to the single-field kernel (colour pass +22 %, residual +0.7 %): they are instantiated, and
// PressureSolver's launch plan takes them, only in a build with -DSOMAR_FULL19_NF3, which is how the note's figures were taken.
template <int NF>
struct FullNfRows { static constexpr int value = 8; };
#ifdef SOMAR_FULL19_NF3
template <>
struct FullNfRows<3> { static constexpr int value = 6; };
#endif

template <int NF>
void launch_full_march_nf(hipStream_t st, TileSpan tiles, const LevelDev& L, const FullFields<NF>& F, int mode, int color)
{
    if (tiles.n == 0) return;
    constexpr int ROWS = FullNfRows<NF>::value;
    SOMAR_CHECK(tiles.classes == 0, "internal: the N-field 19-point kernels take class-0 tiles");
    SOMAR_CHECK(mode == 0 || mode == 2, "internal: the N-field 19-point kernels are the residual and the colour pass");
    const JgFull G = jgfull(L);
    JgFullN J;
    for (int d = 0; d < 3; ++d)
        for (int c = 0; c < 3; ++c) J.c[d][c] = G.c[d][c];
    const bool z = L.P.zero_xy != 0;
#define SOMAR_FN(MODE, Z)                                                                                                     \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_full_march_nf<MODE, ROWS, Z, NF>), dim3(tiles.n), dim3(64, ROWS, 1), 0, st, tiles.p,   \
                       L.patches, F, J, L.jinv, L.P, color)
    if (mode == 0) { if (z) SOMAR_FN(0, true); else SOMAR_FN(0, false); }
    else { if (z) SOMAR_FN(2, true); else SOMAR_FN(2, false); }
#undef SOMAR_FN
}
template void launch_full_march_nf<2>(hipStream_t, TileSpan, const LevelDev&, const FullFields<2>&, int, int);
#ifdef SOMAR_FULL19_NF3
template void launch_full_march_nf<3>(hipStream_t, TileSpan, const LevelDev&, const FullFields<3>&, int, int);
#endif

int full_march_nf_rows(int nf)
{
#ifdef SOMAR_FULL19_NF3
    if (nf == 3) return FullNfRows<3>::value;
#endif
    SOMAR_CHECK(nf == 2, "internal: the N-field 19-point kernels carry two fields per launch");
    return FullNfRows<2>::value;
}

}  // namespace somar
