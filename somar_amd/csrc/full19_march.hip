// somar_amd/csrc/full19_march.hip -- the NON-diagonal (19-point) operator / residual and GSRB colour pass of a large
// level as k-marching, LDS-staged kernels (the non-diagonal counterpart of resid_march.hip).
//
// Why: k_op_full / k_gsrb_full (full19.hip) read phi and its extrapolated copy psi through L2 with 19-point reach and
// nine coefficient planes per cell; the k+-1 reuse distance does not fit the 4 MiB per-XCD L2, every application is
// preceded by a whole-field copy psi := phi (16 B/cell), and lapDiag is a tenth coefficient stream.  Here
//   * a workgroup owns a (124 x 6) column of cells and marches in k; per plane it stages phi AND the cross-term
//     operand E in LDS (4 rotating plane slots each, 128 x 8 doubles per plane, one wavefront per row, one double2 per
//     lane, ONE barrier per plane; 512 threads: the nine coefficient streams need > 128 VGPRs per lane); all 18 neighbours come from LDS, the nine J g^{ab} planes stream through registers
//     exactly once per launch (k-face components are carried from plane to plane);
//   * psi is never copied: E = phi inside the box, psi only in the one-cell FRAME around it -- the only place where
//     the reference's `extrap` FAB differs from phi (extrapolated out-of-domain ghosts, and the box-edge cells
//     ExtrapolateFaceAndCopy rewrites; see solver_full.cpp: the frame-only ghost programs);
//   * lapDiag is recomputed from the diagonal components with FILLMAPPEDLAPDIAG3D's own expression (the stored array's bits
//     wherever the coefficient arrays still are what k_lapdiag read: full19_point.h);
//   * the colour pass writes a second array (updated cells of the colour + untouched cells of the other): the
//     same-colour diagonal neighbours a cross term reads must be PRE-pass values (the reference reads them from the
//     snapshot `extrap`), which an in-place update cannot give a neighbouring workgroup.
// Traffic per cell: residual phi 8 (x halo) + rhs 8 + Jg 72 + Jinv 8 + out 8 = ~106 B (algorithmic 112); colour pass the
// same without rhs -> with it: ~106 B per pass, 212 per red+black sweep (algorithmic 120; the two-pass form reads every
// coefficient line once per colour).
//
// Arithmetic: the text of full19_point.h (operator, interior and boundary GSRB update of one cell), which k_op_full /
// k_gsrb_full call and the N-field and fused kernels share => bit-identical to them and to the CPU oracle.
#include "common.h"
#include "kernels.h"
#include "stencil_point.h"
#include "full19_point.h"

namespace somar {

// region rows FM_J = tile rows + 1 low + 1 high, a template parameter: 8 (6-row tile, 512 threads, 64 KB LDS; at 160 VGPRs
// a SIMD holds 3 waves, so ONE such workgroup fits a CU: 8 waves per CU) or 6 (4-row tile, 384 threads, 48 KB LDS: TWO
// workgroups per CU = 12 waves, the occupancy limit, for 1.5 instead of 1.33 times the phi / psi halo traffic -- 1.4 B/cell
// of about 106).  SOMAR_FULL_ROWS selects; the tile tables follow (Level::define).
constexpr int FM_S = 4;    // plane slots: k-1, k, k+1 are read while k+2's slot is being written

// MODE 0: out = rhs - L[phi]   MODE 1: out = L[phi]   MODE 2: out = phi with the cells of `color` relaxed (one GSRB pass)
// MODE 3: the colour pass on the cells of the three outer layers of each box only, in place, after k_full_fused (see there)
// ZXY: J g^{xy} on x-faces and J g^{yx} on y-faces are identically zero (StencilParams::zero_xy): those two planes are not
// streamed -- three of the pass's thirteen coefficient loads per plane -- and zeros stand in for them; the products are the
// zeros the stored planes would give (up to the sign of zero).
// CLS: the tile's lane class (Tile::cls, march_plan.h): a wavefront covers 2^CLS region rows of 128 >> CLS columns each.
// CLS 0 = one 128-column row per wavefront (124 output columns); CLS 1 = two 64-column rows (60 output columns: a 64-wide
// box is one such tile + a 4-wide one instead of a tile that leaves 30 of 64 lanes idle); CLS 4 = sixteen 8-column rows (the
// 4-column remainder of a box, 128 -> 124 + 4).  Region rows of a wavefront have the same parity (row = 2^(CLS+1) (y / 2) +
// (y & 1) + 2 sub), which the 7-point fused sweep needs and the others share.  Same arithmetic on the same values: same bits.
template <int MODE, int FM_J, bool ZXY, int CLS>
__device__ __forceinline__ void full_march_body(double* __restrict__ SP, double* __restrict__ SE, const Tile& t,
                                                const PatchDesc& p, double* __restrict__ out,
                                                const double* __restrict__ phi, const double* __restrict__ psi,
                                                const double* __restrict__ rhs, const JgFull& J,
                                                const double* __restrict__ jinv, const StencilParams& P, int color,
                                                const double* __restrict__ phi2)
{
    constexpr int LPR = 64 >> CLS;                 // lanes per region row
    constexpr int NR = FM_J << CLS;                // region rows of the workgroup
    constexpr int PITCH = 2 * LPR + (CLS >= 2 ? 2 : 0);   // LDS row pitch; narrow rows padded against bank conflicts
#define SPx(slot, r, c) SP[((slot) * NR + (r)) * PITCH + (c)]
#define SEx(slot, r, c) SE[((slot) * NR + (r)) * PITCH + (c)]
    // class 0: the region row is the wavefront's index, a scalar -- everything derived from it stays in scalar registers
    const int lane = CLS == 0 ? (int)threadIdx.x : (int)(threadIdx.x & (LPR - 1));
    const int row = CLS == 0 ? (int)threadIdx.y
                             : (int)(((threadIdx.y >> 1) << (CLS + 1)) + (threadIdx.y & 1) + 2 * (threadIdx.x >> (6 - CLS)));
    const int ri = 2 * lane;
    const int li = t.i0 - 2 + ri;  // even: rows are 16-byte aligned
    const int wi = t.w > 0 ? t.w : 2 * LPR - 4;
    const int lj = t.j0 - 1 + row;
    const int gj = p.lo[1] + lj;

    // phi / psi may be touched inside the 1-cell ghost layer; coefficients only at the tile's own cells / faces
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

    // stage plane kp of phi and E into its slot (global loads first, LDS writes by the caller's schedule)
    auto load_plane = [&](int kp, double2& vp, double2& ve) {
        const bool fk = (kp >= -1) && (kp <= p.n[2]);
        const bool ink = (kp >= 0) && (kp < p.n[2]);
        const long long idx = base + sk * kp;
        vp = ld2<double>(phi, idx, f0 && fk, f1 && fk, p.off);
        if (MODE == 3) {
            // the pass's colour INSIDE the box comes from phi2 (the sweep's input: the pre-pass value of a cell the fused kernel
            // may already have relaxed), everything else -- the other colour, every ghost cell -- from phi
            const int cs = (p.lo[0] + li + gj + p.lo[2] + kp + color) & 1;
            const bool m0 = in0 && ink && cs == 0, m1 = in1 && ink && cs == 1;
            const double2 vq = ld2<double>(phi2, idx, m0, m1, p.off);
            vp = make_double2(m0 ? vq.x : vp.x, m1 ? vq.y : vp.y);
        }
        const bool e0 = f0 && fk && !(in0 && ink), e1 = f1 && fk && !(in1 && ink);   // frame cells: E = psi
        const double2 vs = ld2<double>(psi, idx, e0, e1, p.off);
        ve = make_double2(e0 ? vs.x : vp.x, e1 ? vs.y : vp.y);
    };
    auto store_plane = [&](int kp, const double2& vp, const double2& ve) {
        const int slot = kp & (FM_S - 1);
        *reinterpret_cast<double2*>(&SPx(slot, row, ri)) = vp;
        *reinterpret_cast<double2*>(&SEx(slot, row, ri)) = ve;
    };

    int k = t.k0;
    const int kend = t.k0 + t.nk;
    {
        double2 vp, ve;
        load_plane(k - 1, vp, ve);
        store_plane(k - 1, vp, ve);
        load_plane(k, vp, ve);
        store_plane(k, vp, ve);
    }
    // k-face components on the LOW face of plane k
    double2 Jz0c = ld2<double>(J.c[2][0], base + sk * k, o[0], o[1], p.off);
    double2 Jz1c = ld2<double>(J.c[2][1], base + sk * k, o[0], o[1], p.off);
    double2 Jz2c = ld2<double>(J.c[2][2], base + sk * k, o[0], o[1], p.off);

    for (; k < kend; ++k) {
        const int gk = p.lo[2] + k;
        // ---- this step's loads: phi / psi of plane k+1, coefficients of plane k ----
        double2 vp, ve;
        load_plane(k + 1, vp, ve);
        const long long ck = base + sk * k;
        const double2 Jz0p = ld2<double>(J.c[2][0], ck + sk, o[0], o[1], p.off);
        const double2 Jz1p = ld2<double>(J.c[2][1], ck + sk, o[0], o[1], p.off);
        const double2 Jz2p = ld2<double>(J.c[2][2], ck + sk, o[0], o[1], p.off);
        double2 Rh = make_double2(0.0, 0.0);
        if (MODE != 1) Rh = ld2<double>(rhs, ck, o[0], o[1], p.off);
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

        store_plane(k + 1, vp, ve);
        __syncthreads();

        if (any) {
            const int sm = (k - 1) & (FM_S - 1), sc = k & (FM_S - 1), sp = (k + 1) & (FM_S - 1);
            double res[2] = {0.0, 0.0};
            bool o3 = true;
            const int csel = (p.lo[0] + li + gj + gk + color) & 1;   // MODE 2: the cell of the pair that has this colour
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int rc = ri + s;
                const double pc = SPx(sc, row, rc);
                if (MODE >= 2 && s != csel) { res[s] = pc; continue; }
                if (!o[s]) continue;
                if (MODE == 3 && min(min(min(li + s, p.n[0] - 1 - (li + s)), min(lj, p.n[1] - 1 - lj)), min(k, p.n[2] - 1 - k)) >= 3) {
                    o3 = false;   // three layers inside the box: k_full_fused relaxed this cell
                    continue;
                }
                const int gi = p.lo[0] + li + s;
                // neighbours: Pn(di,dj,dk) = phi, En(di,dj,dk) = E
#define Pn(di, dj, dk) SPx((dk) < 0 ? sm : ((dk) > 0 ? sp : sc), row + (dj), rc + (di))
#define En(di, dj, dk) SEx((dk) < 0 ? sm : ((dk) > 0 ? sp : sc), row + (dj), rc + (di))
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
                if (MODE < 2) {
#define FULL19_PART 1
#include "full19_point.inc"
                    res[s] = (MODE == 0) ? (pick<double>(Rh, s) - l) : l;
                } else {
                    const bool onb = FULL19_ONB;
                    const double rh = pick<double>(Rh, s);
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
            double* dst = out + base + sk * k;
            if (MODE == 3) {
                if (o[csel] && o3) dst[csel] = res[csel];   // in place: only the shell cells of the colour
            } else if (o[0] && o[1]) *reinterpret_cast<double2*>(dst) = make_double2(res[0], res[1]);
            else if (o[0]) dst[0] = res[0];
            else dst[1] = res[1];
        }
        Jz0c = Jz0p;
        Jz1c = Jz1p;
        Jz2c = Jz2p;
    }
#undef SPx
#undef SEx
}

// NARROW: the tile table holds narrow lane classes; the instantiation without them is the one-body kernel with 64 KB of LDS
// (one 512-wide box: colour pass 3.02 ms against 3.24 with the three-body kernel on the same class-0 tiles).
template <int MODE, int FM_J, bool ZXY, bool NARROW>
// (an occupancy hint of 3 waves per SIMD on every instantiation changed the scheduling of those that need none: 512^3 colour pass
// 3.02 -> 3.29 ms, C5 53.1 -> 55.8 ms; only the three-body operator without zero planes would otherwise take 169 VGPRs)
__global__ __launch_bounds__(64 * FM_J, (NARROW && !ZXY && MODE == 1) ? 3 : 1) void k_full_march(const Tile* __restrict__ tiles,
                                                             const PatchDesc* __restrict__ patches,
                                                             double* __restrict__ out, const double* __restrict__ phi,
                                                             const double* __restrict__ psi,
                                                             const double* __restrict__ rhs, JgFull J,
                                                             const double* __restrict__ jinv, StencilParams P, int color,
                                                          const double* __restrict__ phi2)
{
    // one slot = the largest class's region: FM_J rows of 128, or 16 FM_J rows of 8 + 2 columns
    __shared__ __attribute__((aligned(16))) double SP[FM_S * FM_J * (NARROW ? 160 : 128)];  // phi
    __shared__ __attribute__((aligned(16))) double SE[FM_S * FM_J * (NARROW ? 160 : 128)];  // E: phi inside the box, psi in its frame
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
    const int cls = NARROW ? t.cls : 0;
    if (!NARROW || cls == 0) full_march_body<MODE, FM_J, ZXY, 0>(SP, SE, t, p, out, phi, psi, rhs, J, jinv, P, color, phi2);
    else if (cls == 1) full_march_body<MODE, FM_J, ZXY, NARROW ? 1 : 0>(SP, SE, t, p, out, phi, psi, rhs, J, jinv, P, color, phi2);
    else full_march_body<MODE, FM_J, ZXY, NARROW ? 4 : 0>(SP, SE, t, p, out, phi, psi, rhs, J, jinv, P, color, phi2);
}

// mode 0: out = rhs - L[phi], 1: out = L[phi], 2: one GSRB colour pass.  psi needs to be right only in the one-cell frame of every box.
template <int MODE>
static void launch_march(hipStream_t st, TileSpan tiles, const LevelDev& L, double* out, const double* phi,
                         const double* psi, const double* rhs, int color, const double* phi2 = nullptr)
{
    const bool six = L.full_rows == 6, z = L.P.zero_xy != 0, nw = tiles.classes != 0;   // (6-row tables never hold narrow classes)
#define SOMAR_FM(ROWS, Z, N)                                                                                                   \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_full_march<MODE, ROWS, Z, N>), dim3(tiles.n), dim3(64, ROWS, 1), 0, st, tiles.p, L.patches, \
                       out, phi, psi, rhs, jgfull(L), L.jinv, L.P, color, phi2)
    if (six) { if (z) SOMAR_FM(6, true, false); else SOMAR_FM(6, false, false); }
    else if (nw) { if (z) SOMAR_FM(8, true, true); else SOMAR_FM(8, false, true); }
    else { if (z) SOMAR_FM(8, true, false); else SOMAR_FM(8, false, false); }
#undef SOMAR_FM
}

void launch_full_march(hipStream_t st, TileSpan tiles, const LevelDev& L, double* out, const double* phi,
                       const double* psi, const double* rhs, int mode)
{
    if (tiles.n == 0) return;
    if (mode == 0) launch_march<0>(st, tiles, L, out, phi, psi, rhs, 0);
    else launch_march<1>(st, tiles, L, out, phi, psi, rhs, 0);
}

// one colour pass of the 19-point GSRB: out = phi with the cells of `color` relaxed (out != phi)
void launch_gsrb_full_march(hipStream_t st, TileSpan tiles, const LevelDev& L, double* out,
                            const double* phi, const double* psi, const double* rhs, int color)
{
    if (tiles.n == 0) return;
    launch_march<2>(st, tiles, L, out, phi, psi, rhs, color);
}

}  // namespace somar

namespace somar {
// the black cells of the three outer layers of every box after k_full_fused (full19_fused.hip): in place on phi, their same-colour
// neighbours from phi_in (the sweep's input); tiles = Level::stiles (box faces only, narrow classes on the x faces)
void launch_gsrb_full_shell(hipStream_t st, TileSpan tiles, const LevelDev& L, double* phi, const double* phi_in,
                            const double* psi, const double* rhs)
{
    if (tiles.n == 0) return;
    SOMAR_CHECK(L.full_rows == 8, "internal: the shell pass uses the 8-row marching kernels");
    launch_march<3>(st, tiles, L, phi, phi, psi, rhs, 1, phi_in);
}
}  // namespace somar
