// somar_amd/csrc/gsrb_fused.hip -- one launch = one full red+black GSRB sweep (diagonal metric).
//
// Why: the two-pass form of LevelGSRB (GSRB.cpp:58-98) streams every coefficient line twice per
// sweep (each colour touches half of every 128-B line) and, measured with rocprofv3 PMC on
// MI355X, re-fetches phi 3x and Jg^zz 2x per pass because the k+-1 reuse distance (a whole
// j-slab of every resident workgroup) does not fit the 4 MiB per-XCD L2: 78 B/cell/pass against
// 32 B/cell algorithmic.  This kernel reads every array ONCE per sweep:
//
//   * a workgroup owns a (124 x 12) column of cells and MARCHES in k; per plane it stages phi in
//     LDS (3 rotating planes of 128 x 16 doubles, one wavefront per row, one double2 per lane) and
//     keeps the k-neighbours and the k-face coefficients in registers;
//   * red and black are pipelined one plane apart: step k computes red(k) from OLD black, then
//     black(k-1) from the NEW red of planes k-2, k-1, k -- exactly the values LevelGSRB produces,
//     because a red update only reads black cells and vice versa; one barrier per plane;
//   * the 1-cell ring of red cells around the tile is recomputed redundantly (from a 2-deep phi halo
//     and 1-deep coefficient/rhs halos) instead of being exchanged between the colours, so a level
//     needs ONE ghost exchange per sweep instead of two -- on a sharded level that also halves the
//     number of xGMI round trips;
//   * lapDiag is not loaded: it is recomputed from Jg/Jinv with FILLMAPPEDLAPDIAG3D's own expression
//     (MappedAMRPoissonOpF.ChF:266-271), which yields the identical bits and saves 8 B/cell;
//   * results go to a second array (ping-pong): neighbouring workgroups read each other's halo from
//     the untouched input.
//
// Traffic per cell and sweep: phi 8 in + 8 out, rhs 8, Jg 24, Jinv 8 = 56 B + halo overhead
// (phi x 128*16/(124*12), ring coefficients) ~ 63 B, versus 128-156 B for the two-pass form.
//
// Arithmetic: identical operation order to GSRBITER3DORTHO / GSRBBOUNDARYITER3DORTHO
// (GSRBF.ChF:545-701, 1362-1505) => bit-identical to the two-pass kernel and to the CPU oracle.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "stencil_point.h"   // pick, ld2, gsrb_point: shared with the N-field sweep (multi_march.hip)

namespace somar {


// the "load" of a uniform coefficient.  ld2 returns zeros where its predicate is off; those values only ever reach cells that
// are not computed (a computed cell's coefficients lie inside the frame by construction), so the constant may stand in
// unconditionally -- which makes every coefficient a wave-uniform loop invariant: the diagonal and the selects between the
// pair's two members fold away.
template <class T>
__device__ __forceinline__ typename Vec2<T>::type uni2(double c, bool, bool) { return mk2<T>(T(c), T(c)); }

// Staged coefficients (STG): the six coefficient pairs a step consumes -- rhs, 1/J, J g^xx, J g^yy at j and j + 1 of
// plane k and J g^zz of plane k + 1 -- are fetched ONE STEP AHEAD by loads that write LDS directly (no register destination:
// the streamed instantiations have no registers left to prefetch in), into a slot per (stream, lane) that only the lane itself
// reads back.  The destination of such a load is wave base + 16 x lane, which is exactly that slot; no other wave touches it,
// so the wait for the loads (vmcnt(0) ahead of the plane's barrier) is all the ordering the slots need, and the lane's own
// lgkmcnt(0) after the read covers the write-after-read before the next plane is staged.
constexpr int STG_STREAMS = 6;
// Which sweeps are staged, by INMODE, from the register count of each instantiation (profiles/r14_staged_coefficients.md): the
// folded prolongation (3, 4) would have to carry its coarse parents a step as well and spills, and so does the mixed-class
// kernel (NARROW 1, three bodies) with a phi pair in flight (0, 2).  Those keep the loads into registers.
constexpr bool STAGED_MODES[5] = {true, true, true, false, false};
constexpr bool STAGED_MODES_MIXED[5] = {false, true, false, false, false};
template <class T>
__device__ __forceinline__ void stage2(const T* __restrict__ safe, long long rel, bool ok0, bool ok1, T* wave_slot)
{
    // ld2's address, written as safe + (rel or 0) (safe: the element ld2 reads when neither element of the pair may be touched, a
    // scalar pointer; rel: the pair's distance from it); ld2's zero-select is applied when the slot is read
    static_assert(sizeof(T) == 8, "a staged pair is one 16-byte load: fp64 only");
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(safe + ((ok0 || ok1) ? rel : 0LL)),
                                     (__attribute__((address_space(3))) void*)wave_slot, 16, 0, 0);
}
// a value that is the same in every lane, moved to scalar registers (the staged form has no vector register to spare for it)
__device__ __forceinline__ double wave_uniform(double x)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
template <class T>
__device__ __forceinline__ typename Vec2<T>::type sel2(const typename Vec2<T>::type& v, bool ok0, bool ok1)
{
    return mk2<T>(ok0 ? v.x : T(0), ok1 ? v.y : T(0));
}

// blockDim = (64, FR_J): lane = i-pair of the region, threadIdx.y = region row (one wavefront each).
// FR_J = 16: 124 x 12 output columns per 1024-thread workgroup (one per CU);
// FR_J =  8: 124 x 4 per 512-thread workgroup, two resident per CU so one computes while the other waits.
// INMODE 0: plain.  1: phi_in is taken to be zero everywhere and is not read (first sweep on a zero correction).
// 2: every value of phi_in is read as (value - sums[0]/sums[1]): the mean removal of ZeroAvgConstInterpPS
//    (a_phiThisLevel[dit] -= avgPhi over the whole FAB, ProlongationStrategy.cpp:160-163) folded into the first
//    post-smoothing sweep instead of a separate 16 B/cell pass.
// 3: phi_in is read as value + crse(i / r): the prolongation (CONSTINTERPPS) folded into the first post-smoothing
//    sweep -- ghosts included, which needs crse exchanged one cell deep.  4: as 3, minus sums[0]/sums[1].
// INT (uniform-metric instantiations only): this tile and its red ring touch no domain face, periodic seam or coarse-fine face
// in x and y -- over 90 % of the tiles of a large level -- so everything that classifies a cell against those per lane
// is compiled out (gsrb_point<.., INT>, the ring's existence tests, the coarse-fine ghosts of x and y).  Same arithmetic on
// the same values: same bits.
// CLS: the tile's lane class (see full19_march.hip): a wavefront covers 2^CLS region rows of 128 >> CLS columns, all of the
// same parity, so the colour column c stays wave-uniform.
// sums (modes 2, 4) are fp64 whatever T is: the mean is formed in double, then taken to T
// STG: the coefficients come through the staging slots G (above); phi of plane k + 2 is issued in step k like the UNI form's, and
// nothing a plain load returns is touched before the next step's barrier -- a use in between would make the compiler wait for
// every load in flight, the staged ones included, in the middle of the arithmetic.
template <int FR_J, int INMODE, bool DIRI, bool UNI, bool INT, int CLS, bool STG, class T>
__device__ __forceinline__ void gsrb_fused_body(T* __restrict__ S, T* __restrict__ G, const Tile& t, const PatchDesc& p,
                                                T* __restrict__ phi_out,
                                                const T* __restrict__ phi_in,
                                                const T* __restrict__ rhs,
                                                const T* __restrict__ jgx,
                                                const T* __restrict__ jgy,
                                                const T* __restrict__ jgz,
                                                const T* __restrict__ jinv, const StencilParams& P,
                                                const double* __restrict__ sums,
                                                const PatchDesc* __restrict__ cpatches,
                                                const T* __restrict__ crse, int r0, int r1, int r2)
{
    typedef typename Vec2<T>::type T2;
    T avg = (INMODE == 2 || INMODE == 4) ? T(sums[0] / sums[1]) : T(0);
    if constexpr (STG) avg = wave_uniform(avg);
    constexpr int LPR = 64 >> CLS;                 // lanes per region row
    constexpr int NR = FR_J << CLS;                // region rows of the workgroup
    constexpr int PITCH = 2 * LPR + (CLS >= 2 ? 2 : 0);
    // (STG: the same element addressed from the lane's own cell Sp, so that every neighbour is that one register plus a
    // constant instead of a register of its own)
#define Sx(slot, r, c) \
    (*(STG ? &Sp[(slot) * (NR * PITCH) + ((r) - row) * PITCH + ((c) - ri)] : &S[((slot) * NR + (r)) * PITCH + (c)]))
    // class 0: the region row is the wavefront's index, a scalar -- everything derived from it stays in scalar registers
    const int lane = CLS == 0 ? (int)threadIdx.x : (int)(threadIdx.x & (LPR - 1));
    const int row = CLS == 0 ? (int)threadIdx.y
                             : (int)(((threadIdx.y >> 1) << (CLS + 1)) + (threadIdx.y & 1) + 2 * (threadIdx.x >> (6 - CLS)));
    const int ri = 2 * lane;       // region column of the pair's first cell
    T* const Sp = S + row * PITCH + ri;
    const int li = t.i0 - 2 + ri;  // local i of the pair's first cell (even: rows are 16-byte aligned)
    // output columns of this tile (even, <= region width - 4); the region beyond wi + 4 columns is neither loaded nor computed
    const int wi = t.w > 0 ? t.w : 2 * LPR - 4;
    const int lj = t.j0 - 2 + row;
    // INMODE 3/4: where this pair's coarse parents live (floor division: ghosts map to coarse ghosts)
    long long cbase = 0, cpk = 0, coff = 0;
    int cstep = 0, csh2 = 0;
    if (INMODE >= 3) {
        const PatchDesc cp = cpatches[t.patch];
        auto fdiv = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
        const int ci0 = fdiv(li, r0);
        cstep = fdiv(li + 1, r0) - ci0;  // 0 when both cells share a parent
        coff = cp.off;
        cbase = cp.off + ci0 + (long long)cp.pj * fdiv(lj, r1);
        cpk = cp.pk;
        csh2 = r2 >> 1;                  // multigrid ratios are 1 or 2 per direction (checked by the launcher)
    }
    auto ldphi = [&](int kp, bool ok0, bool ok1) {
        if (INMODE == 1) return mk2<T>(T(0), T(0));
        T2 v = ld2(phi_in, p.off + li + (long long)p.pj * lj + p.pk * kp, ok0, ok1, p.off);
        if (INMODE >= 3) {
            // floor(kp / r2) as an arithmetic shift; both coarse loads are unconditional loads from a safe address (no branch,
            // no load that waits for another: a branch here made the compiler drain vmcnt(0) in every plane)
            const bool any = ok0 || ok1;
            const long long c = any ? cbase + cpk * (long long)(kp >> csh2) : coff;
            const long long c2 = any ? c + cstep : coff;
            const T c0 = crse[c];
            const T c1 = crse[c2];
            v.x = ok0 ? v.x + c0 : T(0);
            v.y = ok1 ? v.y + c1 : T(0);
        }
        if (INMODE == 2 || INMODE == 4) { v.x = v.x - avg; v.y = v.y - avg; }
        return v;
    };
    // STG: ldphi in two halves -- the loads now (raw: phi's pair and, INMODE 3/4, its coarse parents), everything that USES what
    // they return (the zero-select, the parents, the mean) one step later, with the same predicates: the same values.
    // (INMODE 3/4 are written out although STAGED_MODES leaves them off: it is the form whose spills the profile note records.)
    struct RawPhi { T2 v; T c0, c1; };
    auto ldphi_raw = [&](int kp, bool ok0, bool ok1) {
        RawPhi w;
        w.v = mk2<T>(T(0), T(0));
        w.c0 = w.c1 = T(0);
        if (INMODE == 1) return w;
        const bool any = ok0 || ok1;
        w.v = *reinterpret_cast<const T2*>(phi_in + (any ? p.off + li + (long long)p.pj * lj + p.pk * kp : p.off));
        if (INMODE >= 3) {
            const long long c = any ? cbase + cpk * (long long)(kp >> csh2) : coff;
            const long long c2 = any ? c + cstep : coff;
            w.c0 = crse[c];
            w.c1 = crse[c2];
        }
        return w;
    };
    auto ldphi_use = [&](const RawPhi& w, bool ok0, bool ok1) {
        if (INMODE == 1) return mk2<T>(T(0), T(0));
        T2 v = sel2<T>(w.v, ok0, ok1);
        if (INMODE >= 3) {
            v.x = ok0 ? v.x + w.c0 : T(0);
            v.y = ok1 ? v.y + w.c1 : T(0);
        }
        if (INMODE == 2 || INMODE == 4) { v.x = v.x - avg; v.y = v.y - avg; }
        return v;
    };
    const int gj = p.lo[1] + lj;
    T xxS = T(1.0) / (T(P.dx[0]) * T(P.dx[0]));
    T yyS = T(1.0) / (T(P.dx[1]) * T(P.dx[1]));
    T zzS = T(1.0) / (T(P.dx[2]) * T(P.dx[2]));
    if constexpr (STG) { xxS = wave_uniform(xxS); yyS = wave_uniform(yyS); zzS = wave_uniform(zzS); }

    // memory predicates: a cell may be touched only inside the patch's 2-cell frame
    const bool fj = (lj >= -FRAME) && (lj < p.n[1] + FRAME);
    const bool fjh = (lj + 1 >= -FRAME) && (lj + 1 < p.n[1] + FRAME);
    const bool f0 = fj && (li >= -FRAME) && (li < p.n[0] + FRAME) && (ri < wi + 4);
    const bool f1 = fj && (li + 1 >= -FRAME) && (li + 1 < p.n[0] + FRAME) && (ri + 1 < wi + 4);
    // the outermost region rows only supply phi to the red ring: they need no coefficients
    const bool cf = (row >= 1) && (row <= NR - 2);
    const bool c0 = f0 && cf, c1 = f1 && cf;
    // red is computed on the tile grown by one cell, restricted to cells that exist: a cell beyond a
    // non-periodic (Neumann) domain face does not; a periodic image or a neighbour box's cell does
    // (its phi was exchanged two deep, its coefficients one deep).  out_* = cells this tile owns.
    bool comp_ij[2], out_ij[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int l = li + s, g = p.lo[0] + l, r = ri + s;
        bool cmp = (l >= -1) && (l <= p.n[0]) && (r >= 1) && (r <= wi + 2) && (lj >= -1) && (lj <= p.n[1]) &&
                   (row >= 1) && (row <= NR - 2);
        if (!INT) {
            if ((g < P.dom_lo[0] && (P.neum[0][0] || (DIRI && P.diri[0][0]))) ||
                (g > P.dom_hi[0] && (P.neum[0][1] || (DIRI && P.diri[0][1]))))
                cmp = false;
            if ((gj < P.dom_lo[1] && (P.neum[1][0] || (DIRI && P.diri[1][0]))) ||
                (gj > P.dom_hi[1] && (P.neum[1][1] || (DIRI && P.diri[1][1]))))
                cmp = false;
            // beyond a coarse-fine face of this box there is no cell of this level either: the ghost there is an
            // interpolated value (filled before the sweep for the red phase, recomputed below for the black one)
            if ((l < 0 && (p.cf & 1)) || (l >= p.n[0] && (p.cf & 2))) cmp = false;
            if ((lj < 0 && (p.cf & 4)) || (lj >= p.n[1] && (p.cf & 8))) cmp = false;
        }
        comp_ij[s] = cmp;
        out_ij[s] = (l >= 0) && (l < p.n[0]) && (lj >= 0) && (lj < p.n[1]) && (r >= 2) && (r < wi + 2) &&
                    (row >= 2) && (row < NR - 2);
    }
    const long long sj = p.pj, sk = p.pk;
    const long long base = p.off + li + sj * lj;
    const int rel0 = li + p.pj * lj;   // base - p.off: a row of a patch's plane is far below 2^31 elements

    // ---- prologue: planes k0-2 and k0-1 ------------------------------------------------------------
    int k = t.k0 - 1;  // first red plane (the ring below the tile)
    bool fk = (k - 1 >= -FRAME) && (k - 1 < p.n[2] + FRAME);
    T2 Pm = ldphi(k - 1, f0 && fk, f1 && fk);
    fk = (k >= -FRAME) && (k < p.n[2] + FRAME);
    T2 Pc = ldphi(k, f0 && fk, f1 && fk);
    // Jg^zz on the LOW face of plane k
    T2 Gzc = UNI ? uni2<T>(P.uc[2], c0 && fk, c1 && fk) : ld2(jgz, base + sk * k, c0 && fk, c1 && fk, p.off);
    // coefficients of the black cell of plane k-1 (column c), captured one step earlier
    T b_rhs = 0, b_ji = 1, b_gxl = 0, b_gxh = 0, b_gyl = 0, b_gyh = 0, b_gzl = 0;
    T redPrev1 = 0, redPrev2 = 0;
    // UNI: with the coefficient streams gone a plane's loads are 2 x 16 bytes per lane, too little in flight to cover the memory
    // latency a lock-stepped (one barrier per plane) workgroup exposes: phi and rhs are fetched ONE PLANE FURTHER AHEAD
    // (phi of plane k+2 and rhs of plane k+1 are issued in step k and consumed in step k+1)
    T2 Pn = mk2<T>(T(0), T(0)), Rn = mk2<T>(T(0), T(0));
    if (UNI) {
        const bool fkp0 = (k + 1 >= -FRAME) && (k + 1 < p.n[2] + FRAME);
        Pn = ldphi(k + 1, f0 && fkp0, f1 && fkp0);
        Rn = ld2(rhs, base + sk * k, c0 && fk, c1 && fk, p.off);
    }
    // STG: stream s of this wavefront lands at GW(s), the lane's own pair at GL(s).  stage(kk) issues what step kk consumes.
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);   // a scalar: so are the loads' LDS bases
#define GW(s) (G + (wave * STG_STREAMS + (s)) * 128)
#define GL(s) (*reinterpret_cast<const T2*>(GW(s) + 2 * (int)threadIdx.x))
    auto stage = [&](int kk) {
        // (the last step stages for a step that does not come: every predicate off, and no branch -- one around these loads
        // made the compiler wait for them where the paths join)
        const bool gk0 = (kk >= -FRAME) && (kk < p.n[2] + FRAME) && (kk <= t.k0 + t.nk);
        const bool gk1 = (kk + 1 >= -FRAME) && (kk + 1 < p.n[2] + FRAME) && (kk <= t.k0 + t.nk);
        if constexpr (STG) {
            const long long rel = rel0 + sk * kk;   // = base + sk * kk - p.off
            stage2(rhs + p.off, rel, c0 && gk0, c1 && gk0, GW(0));
            stage2(jinv + p.off, rel, c0 && gk0, c1 && gk0, GW(1));
            stage2(jgx + p.off, rel, c0 && gk0, c1 && gk0, GW(2));
            stage2(jgy + p.off, rel, c0 && gk0, c1 && gk0, GW(3));
            stage2(jgy + p.off, rel + sj, c0 && gk0 && fjh, c1 && gk0 && fjh, GW(4));
            stage2(jgz + p.off, rel + sk, c0 && gk1, c1 && gk1, GW(5));
        }
    };
    RawPhi Pr;
    Pr.v = mk2<T>(T(0), T(0));
    Pr.c0 = Pr.c1 = T(0);
    if constexpr (STG) {
        const bool fkp0 = (k + 1 >= -FRAME) && (k + 1 < p.n[2] + FRAME);
        stage(k);
        Pr = ldphi_raw(k + 1, f0 && fkp0, f1 && fkp0);
    }

    const int kend = t.k0 + t.nk;  // last red plane (the ring above the tile)
    // One plane of the march.  The colour column c = (i + j + k) & 1 of the pair is the same for every lane of a wavefront
    // (li is even, gj and gk are wave-uniform) and alternates from plane to plane: the body is instantiated for c = 0 and
    // c = 1 and the loop below calls them in turn, so every select between the pair's two members is resolved at compile
    // time (a quarter of the loop's vector instructions were v_cndmask on a lane-varying-looking c).
    auto step = [&](auto CC) {
        constexpr int c = decltype(CC)::value;
        const int gk = p.lo[2] + k;
        fk = (k >= -FRAME) && (k < p.n[2] + FRAME);
        const bool fkp = (k + 1 >= -FRAME) && (k + 1 < p.n[2] + FRAME);
        // ---- this step's loads: phi and Jg^zz of plane k+1, cell coefficients of plane k --------
        T2 Pp, Rh, Gzp, Ji, Gx, Gy, Gyh;
        T gx_next;
        if constexpr (!STG) {
        if (UNI) {
            Pp = Pn;
            Rh = Rn;
            const bool fkpp = (k + 2 >= -FRAME) && (k + 2 < p.n[2] + FRAME);
            Pn = ldphi(k + 2, f0 && fkpp, f1 && fkpp);
            Rn = ld2(rhs, base + sk * (k + 1), c0 && fkp, c1 && fkp, p.off);
        } else {
            Pp = ldphi(k + 1, f0 && fkp, f1 && fkp);
            Rh = ld2(rhs, base + sk * k, c0 && fk, c1 && fk, p.off);
        }
        Gzp = UNI ? uni2<T>(P.uc[2], c0 && fkp, c1 && fkp) : ld2(jgz, base + sk * (k + 1), c0 && fkp, c1 && fkp, p.off);
        Ji = UNI ? uni2<T>(P.uc[3], c0 && fk, c1 && fk) : ld2(jinv, base + sk * k, c0 && fk, c1 && fk, p.off);
        Gx = UNI ? uni2<T>(P.uc[0], c0 && fk, c1 && fk) : ld2(jgx, base + sk * k, c0 && fk, c1 && fk, p.off);
        Gy = UNI ? uni2<T>(P.uc[1], c0 && fk, c1 && fk) : ld2(jgy, base + sk * k, c0 && fk, c1 && fk, p.off);
        Gyh = UNI ? uni2<T>(P.uc[1], c0 && fk && fjh, c1 && fk && fjh)
                           : ld2(jgy, base + sk * k + sj, c0 && fk && fjh, c1 && fk && fjh, p.off);
        // Jg^xx on the face right of the pair = first component of the next lane's pair
        gx_next = __shfl_down(Gx.x, 1, 64);
        }

        // ---- stage plane k (old values) in LDS; ONE barrier per plane -----------------------------
        //   slot k%3 was last read two steps ago (black of plane k-3); every wave has passed the
        //   previous barrier since, so overwriting it is safe.
        const int slot = ((k % 3) + 3) % 3;
        *reinterpret_cast<T2*>(&Sx(slot, row, ri)) = Pc;
        __syncthreads();
        if constexpr (STG) {
            // every load of the previous step has landed (the wait ahead of the barrier): take what it staged and fetched,
            // with ld2's / ldphi's selects under this plane's predicates, then issue ALL of the next plane's loads at once
            Pp = ldphi_use(Pr, f0 && fkp, f1 && fkp);
            Rh = sel2<T>(GL(0), c0 && fk, c1 && fk);
            Ji = sel2<T>(GL(1), c0 && fk, c1 && fk);
            Gx = sel2<T>(GL(2), c0 && fk, c1 && fk);
            Gy = sel2<T>(GL(3), c0 && fk, c1 && fk);
            Gyh = sel2<T>(GL(4), c0 && fk && fjh, c1 && fk && fjh);
            Gzp = sel2<T>(GL(5), c0 && fkp, c1 && fkp);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the slots are read: they may be overwritten
            const bool fkpp = (k + 2 >= -FRAME) && (k + 2 < p.n[2] + FRAME);
            stage(k + 1);
            Pr = ldphi_raw(k + 2, f0 && fkpp, f1 && fkpp);
            gx_next = __shfl_down(Gx.x, 1, 64);
        }

        // ---- red(k) at column c: reads only black cells of the plane, writes only red ones ---------
        // red = pass 0 = even i+j+k (GSRBF.ChF:381-387): c is this plane's red column of the pair
        const int rc = ri + c;
        T red = pick<T>(Pc, c);  // cells not computed here keep their old value
        {
            bool comp = comp_ij[c] && (k >= -1) && (k <= p.n[2]);
            if ((gk < P.dom_lo[2] && (P.neum[2][0] || (DIRI && P.diri[2][0]))) ||
                (gk > P.dom_hi[2] && (P.neum[2][1] || (DIRI && P.diri[2][1]))))
                comp = false;
            if ((k < 0 && (p.cf & 16)) || (k >= p.n[2] && (p.cf & 32))) comp = false;
            if (comp) {
                const T pxl = Sx(slot, row, rc - 1), pxh = Sx(slot, row, rc + 1);
                const T pyl = Sx(slot, row - 1, rc), pyh = Sx(slot, row + 1, rc);
                red = gsrb_point<DIRI, INT, T>(P, xxS, yyS, zzS, p.lo[0] + li + c, gj, gk, pxl, pxh, pyl, pyh, pick<T>(Pm, c),
                                 pick<T>(Pp, c), c ? Gx.y : Gx.x, c ? gx_next : Gx.y, pick<T>(Gy, c), pick<T>(Gyh, c),
                                 pick<T>(Gzc, c), pick<T>(Gzp, c), pick<T>(Ji, c), pick<T>(Rh, c), red);
                Sx(slot, row, rc) = red;  // visible to the black phase of the NEXT step (after its barrier)
            }
        }

        // ---- black(k-1) at the same column c: in-plane neighbours = new red of plane k-1 (LDS),
        //      below = red(c,k-2) and above = red(c,k), both computed by this very lane -------------
        {
            const int kb = k - 1;
            if ((kb >= t.k0) && (kb < t.k0 + t.nk) && (out_ij[0] || out_ij[1])) {
                const int sb = ((kb % 3) + 3) % 3;
                T black = 0;
                if (out_ij[c]) {
                    T pxl = Sx(sb, row, rc - 1), pxh = Sx(sb, row, rc + 1);
                    T pyl = Sx(sb, row - 1, rc), pyh = Sx(sb, row + 1, rc);
                    T pzl = redPrev2, pzh = red;
                    if (INT ? (p.cf & 48) != 0 : p.cf != 0) {
                        // homogeneousCFInterp between the colours (LevelGSRB refills the CF ghosts before the
                        // black pass): ghost = c1 * first valid cell (this black cell, old value) + c2 * second
                        // valid cell (its opposite neighbour, a NEW red value)
                        const T own = Sx(sb, row, rc);
                        const int l = li + c;
                        const T xl = pxl, xh = pxh, yl = pyl, yh = pyh, zl = pzl, zh = pzh;
                        if (!INT) {
                            if ((p.cf & 1) && l == 0) pxl = T(P.cf_c1[0]) * own + T(P.cf_c2[0]) * xh;
                            if ((p.cf & 2) && l == p.n[0] - 1) pxh = T(P.cf_c1[0]) * own + T(P.cf_c2[0]) * xl;
                            if ((p.cf & 4) && lj == 0) pyl = T(P.cf_c1[1]) * own + T(P.cf_c2[1]) * yh;
                            if ((p.cf & 8) && lj == p.n[1] - 1) pyh = T(P.cf_c1[1]) * own + T(P.cf_c2[1]) * yl;
                        }
                        if ((p.cf & 16) && kb == 0) pzl = T(P.cf_c1[2]) * own + T(P.cf_c2[2]) * zh;
                        if ((p.cf & 32) && kb == p.n[2] - 1) pzh = T(P.cf_c1[2]) * own + T(P.cf_c2[2]) * zl;
                    }
                    black = gsrb_point<DIRI, INT, T>(P, xxS, yyS, zzS, p.lo[0] + li + c, gj, p.lo[2] + kb, pxl, pxh, pyl, pyh,
                                       pzl, pzh, b_gxl, b_gxh, b_gyl, b_gyh, b_gzl, pick<T>(Gzc, c), b_ji, b_rhs,
                                       Sx(sb, row, rc));
                }
                // plane k-1: column c is the new black, column c^1 is red(k-1) (= redPrev1)
                // (STG: the same address from the 32-bit rel0, so that the 64-bit base need not stay in registers)
                T* dst = STG ? phi_out + p.off + (rel0 + sk * kb) : phi_out + base + sk * kb;
                const T ox = c ? redPrev1 : black, oy = c ? black : redPrev1;
                if (out_ij[0] && out_ij[1]) *reinterpret_cast<T2*>(dst) = mk2<T>(ox, oy);
                else if (out_ij[0]) dst[0] = ox;
                else dst[1] = oy;
            }
        }

        // ---- rotate: the next black cell is column c^1 of plane k ------------------------------------
        {
            const int cb = c ^ 1;
            b_rhs = pick<T>(Rh, cb);
            b_ji = pick<T>(Ji, cb);
            b_gxl = cb ? Gx.y : Gx.x;
            b_gxh = cb ? gx_next : Gx.y;
            b_gyl = pick<T>(Gy, cb);
            b_gyh = pick<T>(Gyh, cb);
            b_gzl = pick<T>(Gzc, cb);
        }
        redPrev2 = redPrev1;
        redPrev1 = red;
        Pm = Pc;
        Pc = Pp;
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
    // nothing may still be in flight towards this workgroup's LDS when it ends
    if constexpr (STG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef GL
#undef GW
#undef Sx
}

// NARROW 1: the tile table holds narrow lane classes (uniform-metric depths, or SOMAR_NARROW_7PT=1); the instantiation without
// them (0) is the one-body kernel with 48 KB of LDS that the HBM-bound streaming sweep was tuned as.  NARROW 2: every tile is
// class 1 (tall tiles, march_plan.h): one body again, the same 48 KB, the region read as 32 rows of 64.
// STG: the staged-coefficient form (above): 96 KB of slots next to the phi planes, still one workgroup per CU.
template <int FR_J, int INMODE, bool DIRI = false, bool UNI = false, int NARROW = 0, class T = double, bool STG = false>
__global__ __launch_bounds__(64 * FR_J) void k_gsrb_fused(const Tile* __restrict__ tiles,
                                                     const PatchDesc* __restrict__ patches,
                                                     T* __restrict__ phi_out,
                                                     const T* __restrict__ phi_in,
                                                     const T* __restrict__ rhs,
                                                     const T* __restrict__ jgx,
                                                     const T* __restrict__ jgy,
                                                     const T* __restrict__ jgz,
                                                     const T* __restrict__ jinv, StencilParams P,
                                                     const double* __restrict__ sums,
                                                     const PatchDesc* __restrict__ cpatches,
                                                     const T* __restrict__ crse, int r0, int r1, int r2, int lean_ok)
{
    // one slot = the largest class's region: FR_J rows of 128, or 16 FR_J rows of 8 + 2
    __shared__ __attribute__((aligned(16))) T S[3 * FR_J * (NARROW == 1 ? 160 : 128)];
    // an array of its own, not a part of S: the compiler then knows that the phi planes' reads and writes cannot touch a slot a
    // load is still writing, and does not wait for the loads in front of them
    __shared__ __attribute__((aligned(16))) T G[STG ? STG_STREAMS * FR_J * 128 : 2];
    static_assert(!STG || (FR_J == 16 && !UNI && sizeof(T) == 8), "staged coefficients: the fp64 streamed 16-row kernels");
    const Tile t = tiles[blockIdx.x];
    const PatchDesc p = patches[t.patch];
    const int cls = NARROW == 1 ? t.cls : (NARROW == 2 ? 1 : 0);
    bool lean = false;
    if (UNI && !DIRI) {
        // does the tile grown by its red ring stay clear of every domain face (periodic seams included: the boundary form of
        // the update applies there too) and of every coarse-fine face, in x and y?  One scalar test per workgroup.
        const int wi = t.w > 0 ? t.w : 124;
        const int ilo = t.i0 - 1, ihi = min(t.i0 + wi, p.n[0]), jlo = t.j0 - 1, jhi = min(t.j0 + (FR_J << cls) - 4, p.n[1]);
        lean = lean_ok && p.lo[0] + ilo > P.dom_lo[0] && p.lo[0] + ihi < P.dom_hi[0] && p.lo[1] + jlo > P.dom_lo[1] &&
               p.lo[1] + jhi < P.dom_hi[1] && !((p.cf & 1) && ilo < 0) && !((p.cf & 2) && ihi >= p.n[0]) &&
               !((p.cf & 4) && jlo < 0) && !((p.cf & 8) && jhi >= p.n[1]);
    }
#define SOMAR_FUSED_BODY(INT_, CLS_)                                                                                          \
    gsrb_fused_body<FR_J, INMODE, DIRI, UNI, INT_, CLS_, STG, T>(S, G, t, p, phi_out, phi_in, rhs, jgx, jgy, jgz, jinv, P, sums, cpatches, \
                                                        crse, r0, r1, r2)
    if constexpr (NARROW == 2) {
        SOMAR_FUSED_BODY(false, 1);   // (never with UNI: no lean form)
    } else if (!NARROW || cls == 0) {
        if (lean) SOMAR_FUSED_BODY(UNI && !DIRI, 0);
        else SOMAR_FUSED_BODY(false, 0);
    } else if (cls == 1) {
        if (lean) SOMAR_FUSED_BODY(UNI && !DIRI, NARROW ? 1 : 0);
        else SOMAR_FUSED_BODY(false, NARROW ? 1 : 0);
    } else {
        SOMAR_FUSED_BODY(false, NARROW ? 4 : 0);   // remainder columns sit on a box edge: never clear of it
    }
#undef SOMAR_FUSED_BODY
}

// which instantiations have a staged-coefficient twin: fp64 (a float pair is 8 bytes, not a width the load has), a streamed
// metric, 16 rows (the 8-row kernels hide latency with a second workgroup per CU)
template <class T>
constexpr bool staged_mode(int rows, bool uni, int narrow, int in_mode)
{
    return sizeof(T) == 8 && rows == 16 && !uni && (narrow == 1 ? STAGED_MODES_MIXED[in_mode] : STAGED_MODES[in_mode]);
}

// M: the level's coefficient arrays in T (L.jg / L.jinv, or their fp32 copies)
template <class T>
static void launch_gsrb_fused_t(hipStream_t st, TileSpan tiles, const LevelDev& L, const MetricPtrs<T>& M,
                                T* phi_out, const T* phi_in, const T* rhs, int in_mode, const double* sums,
                                const LevelDev* C, const T* crse, const int* r)
{
    if (tiles.n == 0) return;
    const PatchDesc* cpatches = C ? C->patches : nullptr;
    const int r0 = r ? r[0] : 1, r1 = r ? r[1] : 1, r2 = r ? r[2] : 1;
    SOMAR_CHECK(in_mode < 3 || ((r0 == 1 || r0 == 2) && (r1 == 1 || r1 == 2) && (r2 == 1 || r2 == 2)),
                "internal: the prolongation folded into a sweep takes multigrid ratios of 1 or 2 per direction");
    // the staged-coefficient twin of a streamed fp64 16-row kernel (the kernel itself otherwise): SOMAR_NO_STAGED_COEF=1 and
    // every other instantiation keep the loads into registers
    auto go = [&](auto kern0, auto kern1, int rows) {
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(tiles.n), dim3(64, rows, 1), 0, st, tiles.p, L.patches, phi_out, phi_in, rhs, M.jg[0],
                               M.jg[1], M.jg[2], M.jinv, L.P, sums, cpatches, crse, r0, r1, r2, L.lean_tiles);
        };
        if (L.staged_coef) launch(kern1);
        else launch(kern0);
    };
    // (rows, mode, Dirichlet sides, uniform metric, narrow lane classes in the tile table: 0 none, 1 mixed, 2 all class 1)
#define SOMAR_FUSED_KERN(ROWS, D, U, N, M) \
    k_gsrb_fused<ROWS, M, D, U, N, T>, k_gsrb_fused<ROWS, M, D, U, N, T, staged_mode<T>(ROWS, U, N, M)>
#define SOMAR_FUSED_MODES(ROWS, D, U, N, M0, M1, M2, M3, M4)                    \
    switch (in_mode) {                                                          \
        case 1: go(SOMAR_FUSED_KERN(ROWS, D, U, N, M1), ROWS); break;           \
        case 2: go(SOMAR_FUSED_KERN(ROWS, D, U, N, M2), ROWS); break;           \
        case 3: go(SOMAR_FUSED_KERN(ROWS, D, U, N, M3), ROWS); break;           \
        case 4: go(SOMAR_FUSED_KERN(ROWS, D, U, N, M4), ROWS); break;           \
        default: go(SOMAR_FUSED_KERN(ROWS, D, U, N, M0), ROWS);                 \
    }
    const bool rows16 = L.fused_rows == 16;
    const bool narrow = tiles.classes != 0 && rows16;   // march_plan::fused_shape hands the 8-row kernels class-0 tiles only
    const bool tall = tiles.classes == 2;               // ... and tall tiles to the 16-row kernels of a non-uniform metric only
    SOMAR_CHECK(!tall || (rows16 && !L.P.uniform), "internal: tall tiles on a level whose fused sweep has no class-1 kernel");
    bool diri = false;
    for (int d = 0; d < 3; ++d) diri = diri || L.P.diri[d][0] || L.P.diri[d][1];
    if (diri) {
        // Dirichlet sides: no null space, hence never a mean removal (modes 2 / 4 fall back to 0 / 3 in the table below; checked)
        SOMAR_CHECK(in_mode == 0 || in_mode == 1 || in_mode == 3, "internal: mean removal on a level with Dirichlet sides");
        if (!rows16) { SOMAR_FUSED_MODES(8, true, false, false, 0, 1, 0, 3, 3) }
        else if (tall) { SOMAR_FUSED_MODES(16, true, false, 2, 0, 1, 0, 3, 3) }
        else if (narrow) { SOMAR_FUSED_MODES(16, true, false, true, 0, 1, 0, 3, 3) }
        else { SOMAR_FUSED_MODES(16, true, false, false, 0, 1, 0, 3, 3) }
        return;
    }
    if (L.P.uniform && rows16) {
        // uniform metric: the four coefficient streams come from StencilParams
        if (narrow) { SOMAR_FUSED_MODES(16, false, true, true, 0, 1, 2, 3, 4) }
        else { SOMAR_FUSED_MODES(16, false, true, false, 0, 1, 2, 3, 4) }
        return;
    }
    if (!rows16) { SOMAR_FUSED_MODES(8, false, false, false, 0, 1, 2, 3, 4) }
    else if (tall) { SOMAR_FUSED_MODES(16, false, false, 2, 0, 1, 2, 3, 4) }
    else if (narrow) { SOMAR_FUSED_MODES(16, false, false, true, 0, 1, 2, 3, 4) }
    else { SOMAR_FUSED_MODES(16, false, false, false, 0, 1, 2, 3, 4) }
#undef SOMAR_FUSED_MODES
#undef SOMAR_FUSED_KERN
}

void launch_gsrb_fused(hipStream_t st, TileSpan tiles, const LevelDev& L, const MetricPtrs<double>& M,
                       double* phi_out, const double* phi_in, const double* rhs, int in_mode, const double* sums,
                       const LevelDev* C, const double* crse, const int* r)
{
    launch_gsrb_fused_t<double>(st, tiles, L, M, phi_out, phi_in, rhs, in_mode, sums, C, crse, r);
}

void launch_gsrb_fused(hipStream_t st, TileSpan tiles, const LevelDev& L, const MetricPtrs<float>& M,
                       float* phi_out, const float* phi_in, const float* rhs, int in_mode, const double* sums,
                       const LevelDev* C, const float* crse, const int* r)
{
    // the fp32 copies of a uniform depth are not made (PressureSolver::mp_convert_metric): only the UNI kernels may run without them
    SOMAR_CHECK(fused_uniform_kernel(L) || (M.jg[0] && M.jg[1] && M.jg[2] && M.jinv),
                "internal: the fused sweep streams the metric of this depth, but its fp32 copies are missing");
    launch_gsrb_fused_t<float>(st, tiles, L, M, phi_out, phi_in, rhs, in_mode, sums, C, crse, r);
}

// the launcher's choice above: the uniform-metric kernels (coefficients from StencilParams::uc, no array read) run on a uniform
// depth without Dirichlet sides in the 16-row form; the Dirichlet and 8-row tables stream the four arrays whatever the flag says
bool fused_uniform_kernel(const LevelDev& L)
{
    bool diri = false;
    for (int d = 0; d < 3; ++d) diri = diri || L.P.diri[d][0] || L.P.diri[d][1];
    return L.P.uniform && L.fused_rows == 16 && !diri;
}

}  // namespace somar
