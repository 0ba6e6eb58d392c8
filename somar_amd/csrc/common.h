// somar_amd/csrc/common.h -- shared host/device declarations for the MI355X (gfx950)
// implementation of SOMAR's pressure-projection multigrid.  HIP only; no CUDA paths.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "march_plan.h"   // Tile: the work item of a sweep kernel

namespace somar {

// Error convention of the C ABI (include/somar_amd.h): 0 ok, <0 failure.  Inside the
// library failures are C++ exceptions, translated at the ABI boundary.
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define SOMAR_HIP(call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            throw ::somar::Error(-2, std::string("HIP error ") + hipGetErrorString(e_) + " at " \
                                         + __FILE__ + ":" + std::to_string(__LINE__));          \
    } while (0)

#define SOMAR_CHECK(cond, msg)                                                      \
    do {                                                                            \
        if (!(cond))                                                                \
            throw ::somar::Error(-1, std::string(msg) + " (" #cond ") at " + __FILE__ + \
                                         ":" + std::to_string(__LINE__));         \
    } while (0)

// "Set for the duration of the call": ScopedSet saves a variable, sets it, and puts the saved value back when the scope ends,
// by return or by exception; ScopeExit runs any other way back (its lambda) at that point.
template <class T>
struct ScopedSet {
    T& var;
    const T saved;
    ScopedSet(T& v, const T& value) : var(v), saved(v) { var = value; }
    ~ScopedSet() { var = saved; }
    ScopedSet(const ScopedSet&) = delete;
};
template <class F>
struct ScopeExit {
    F f;
    ~ScopeExit() { f(); }
};
template <class F>
ScopeExit(F) -> ScopeExit<F>;

// BCType codes, reference calculus/BCInterface/BCDescriptor.H:34-39
enum { BC_UNDEFINED = -2, BC_NONE = -1, BC_NEUM = 0, BC_DIRI = 1, BC_PERIODIC = 2, BC_CF = 3 };

// Ghost frame allocated around every patch, in cells.  All fields of a level (cell- and
// face-centred alike) share one shape so a single offset addresses every array; face
// index i is the LOW face of cell i (reference convention, MappedAMRPoissonOpF.ChF:412-415).
constexpr int FRAME = 2;

// One box of a level as stored in HBM.  Element (i,j,k) (local, 0-based from the valid
// low corner; ghosts are negative) of any field lives at  base[off + i + pj*j + pk*k].
struct PatchDesc {
    int lo[3];  // global index of the valid low corner
    int n[3];   // valid cells per direction
    int pj;     // j pitch (elements), even => 16-byte aligned rows
    int cf;     // bit (2*dir + side): that whole face of the box is a coarse-fine boundary (levels on a coarser one)
    long long pk;   // k pitch
    long long off;  // offset of local cell (0,0,0)
};

// a pair of cells of one field (the marching kernels hold one per lane), for either element type of a field: fp64, or fp32 on the
// depths of an opt-in mixed-precision cycle (PressureSolver::set_precision)
template <class T> struct Vec2;
template <> struct Vec2<double> { typedef double2 type; };
template <> struct Vec2<float> { typedef float2 type; };
template <class T>
__host__ __device__ __forceinline__ typename Vec2<T>::type mk2(T a, T b)
{
    typename Vec2<T>::type v;
    v.x = a;
    v.y = b;
    return v;
}
constexpr int TILE_I = 128;  // cells in i per block (64 lanes x double2)
constexpr int TILE_J_MAX = 8;   // rows per block (blockDim.y), chosen per level
constexpr int TILE_K_MAX = 32;  // planes marched by one block, chosen per level

// One box-to-box ghost copy ("motion item" of a Chombo Copier).
struct CopyItem {
    int src_patch, dst_patch;
    int src_lo[3];  // local start in the source patch
    int dst_lo[3];  // local start in the destination patch
    int n[3];
    int pad_;
};

// One coarse-fine ghost cell of a level that sits on a coarser one (homogeneous CF interpolation).
struct CFCell {
    long long off;  // the ghost cell
    int stride;     // signed element stride pointing OUT of the box: off - stride is the first valid cell
    int dir;        // direction | 4 if the box is one cell wide in that direction
};

// One step of a ghost "program" of the non-diagonal (19-point) path (full19.hip): a region of one patch.
// GHOST_DIRI_FACE: a Dirichlet side with one value per boundary face (EllipticDiriBCGhostClass) instead of one per side
// GHOST_NEUM_FACE: a Neumann side of a DIAGONAL-metric level with one value per boundary face (EllipticNeumBCGhostClass)
enum { GHOST_COPY = 0, GHOST_EXTRAP = 1, GHOST_NEUM = 2, GHOST_DIRI = 3, GHOST_DIRI_FACE = 4, GHOST_NEUM_FACE = 5 };
__host__ __device__ inline bool ghost_is_diri(int type) { return type == GHOST_DIRI || type == GHOST_DIRI_FACE; }
struct GhostOp {
    int patch, type;
    int lo[3];       // local start of the region
    int n[3];
    int dir, sgn;    // EXTRAP / NEUM / DIRI: direction and side sign (+1 high, -1 low)
    int order;       // EXTRAP: 0, 1 or 2
    int dstf, srcf;  // 0 = phi, 1 = psi (the extrapolated copy)
    // the op's stage in its ghost program.  In the box-sorted copy of a program (PressureSolver::upload_program, k_ghost_program)
    // the upper half counts the ops of the same stage that follow: stage | following << 16 (ghost_stage / ghost_following)
    int stage;
    union {
        double val;      // DIRI: the boundary value of that side
        long long voff;  // DIRI_FACE / NEUM_FACE: start of this op's slice of the level's face-value buffer (LevelDev::bc_face),
                         // one value per cell of the region in the op's own loop order (i fastest)
    };
};
__host__ __device__ inline int ghost_stage(int packed) { return packed & 0xffff; }
__host__ __device__ inline int ghost_following(int packed) { return packed >> 16; }
// k_ghost_program stages GP_MAX_OPS of these in LDS with 16-byte copies
static_assert(sizeof(GhostOp) == 64 && sizeof(GhostOp) % 16 == 0, "GhostOp must stay 64 bytes (LDS staging, int4 copy)");

// Per-level constants handed to the stencil kernels by value.
struct StencilParams {
    int dom_lo[3], dom_hi[3];  // domain box at this depth
    int neum[3][2];            // 1 = homogeneous-Neumann physical face (no ghost, no flux)
    int active[3];             // activeDirs
    int periodic[3];
    double dx[3];
    double alpha, beta;
    double cf_c1[3], cf_c2[3];  // homogeneous CF interpolation: ghost = c1 * first valid + c2 * second valid
    int bc_homog;               // ghost programs: Dirichlet sides take the value 0 instead of their own
    int pad2_;
    int diri[3][2];             // 1 = Dirichlet physical face (ghost = 2 value - first cell)
    // uniform metric (a Cartesian map: CartesianMap.cpp:261-280 fills constants): J g^{aa} == uc[a] on every face and
    // J^{-1} == uc[3] in every cell of this depth, found by PressureSolver::detect_metric_flags.  The k-marching kernels
    // then take the four values from here instead of streaming four arrays of them (56 -> 24 B/cell on a sweep).
    int uniform = 0;
    // non-diagonal metric: J g^{xy} on x-faces and J g^{yx} on y-faces are zero everywhere on this depth (any map with x = xi,
    // y = eta: BathymetricBaseMap and its DEM / Ledge / BeamGenerator subclasses); the marching 19-point kernels then stream
    // seven coefficient planes instead of nine (PressureSolver::detect_metric_flags)
    int zero_xy = 0;
    double uc[4] = {0.0, 0.0, 0.0, 0.0};
};

}  // namespace somar
