// somar_amd/csrc/kernels.h -- launcher prototypes for kernels.hip
#pragma once
#include "common.h"

namespace somar {

// A tile table on the device as a launcher takes it (TileTable::span, level.h).  classes is how the table was planned
// (march_plan::Table): 0 every tile is class 0, 1 it holds narrow lane classes, 2 every tile is class 1 (tall tiles).  The
// launchers pick the kernel instantiation from it: a table cannot reach a kernel that misreads its tiles.
struct TileSpan {
    const Tile* p = nullptr;
    int n = 0;
    int classes = 0;
};

// Device-side view of one (AMR level, MG depth): tables + coefficient planes in HBM.
struct LevelDev {
    const Tile* tiles = nullptr;        // XCD-contiguous order
    int ntiles = 0;
    int tile_j = 4;                     // blockDim.y of every tile kernel on this level
    // pull exchange (small single-rank levels): per tile, the local ghost copies that land in the tile's one-cell halo; a
    // stencil kernel refreshes exactly the ghosts it is about to read, so the separate copy launch disappears (null: not built)
    const CopyItem* tile_items = nullptr;
    const int* tile_item_start = nullptr;
    int ghost_gy = 16;                  // workgroups per ghost op (k_ghost_ops): the largest box face / 1024, within [16, 256]
    const PatchDesc* patches = nullptr;
    int npatches = 0;
    double* jg[3] = {nullptr, nullptr, nullptr};  // J g^{aa} on a-faces
    double* jinv = nullptr;
    double* lapdiag = nullptr;
    // non-diagonal metric: all components J g^{ab} on a-faces, jgf[a][b]; jgf[a][a] aliases jg[a]
    double* jgf[3][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    StencilParams P;
    // position-dependent Dirichlet / Neumann values of this level (depth 0 only): the slices GHOST_DIRI_FACE / GHOST_NEUM_FACE
    // ops read at GhostOp::voff (PressureSolver::build_face_slices); the address never changes after finalize
    const double* bc_face = nullptr;
    // what the launchers take from the solver's Tuning (Level::define copies it here)
    int fused_rows = 16;                // region rows per workgroup of the fused 7-point sweep (tile rows = rows - 4): 16 or 8
    int full_rows = 8;                  // ... of the 19-point marching kernels: 8 or 6
    int lean_tiles = 1;                 // interior tiles of the uniform-metric fused sweep take the lean body
    int staged_coef = 0;                // the streamed fp64 16-row fused sweep fetches its coefficients a plane ahead through LDS
    int ordered_serial = 0;             // serial-order sums walk all boxes in one chain (launch_reduce)
};

// the coefficient arrays a marching kernel streams, in its element type: the level's own (fp64), or their fp32 copies on the
// depths of the opt-in mixed-precision cycle (PressureSolver::set_precision; null where StencilParams::uniform stands in)
template <class T>
struct MetricPtrs { const T* jg[3]; const T* jinv; };
inline MetricPtrs<double> metric_ptrs(const LevelDev& L) { return MetricPtrs<double>{{L.jg[0], L.jg[1], L.jg[2]}, L.jinv}; }

// operands of MAPPEDGETFLUX with a non-diagonal metric, evaluated where a flux register needs it (amr_kernels.hip: reg_flux19)
struct FullFlux { const double* psi = nullptr; const double* J[3][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}}; double dxi[3] = {0, 0, 0}; };

// 19-point path (full19.hip)
// every J g^{ab} plane of a level as a kernel argument, c[faceDir][component]; on a diagonal-metric level (no jgf) the
// diagonal entries are its jg (what the GHOST_NEUM_FACE ops read) and the others stay null
struct JgFull { const double* c[3][3]; };
JgFull jgfull(const LevelDev& L);
// redirect: a read of psi that lands INSIDE the box's valid region takes phi instead (psi is then maintained in the
// boxes' frames only -- the frame-only programs of the marching 19-point kernels, full19_march.hip)
void launch_ghost_ops(hipStream_t st, const LevelDev& L, const GhostOp* ops, int nops, double* phi, double* psi,
                      bool bc_homog = true, bool redirect = false);
// homogeneous physical ghosts of an fp32 field (mixed-precision depths; ops without cross terms)
void launch_ghost_ops(hipStream_t st, const LevelDev& L, const GhostOp* ops, int nops, float* phi);
// a whole ghost program in one launch, one workgroup per box (ops sorted by box, then GhostOp::stage; box b owns
// box_ops[box_first[b] .. box_first[b + 1])); copy_all: psi := phi on every box grown by one cell first
void launch_ghost_program(hipStream_t st, const LevelDev& L, const GhostOp* box_ops, const int* box_first, double* phi,
                          double* psi, bool bc_homog, bool redirect, bool copy_all);
// k-marching 19-point operator / residual (mode 0: out = rhs - L[phi], 1: out = L[phi]) and one GSRB colour pass
// (out = phi with the colour's cells relaxed; out != phi); psi valid in the one-cell frames only (full19_march.hip)
void launch_full_march(hipStream_t st, TileSpan tiles, const LevelDev& L, double* out, const double* phi,
                       const double* psi, const double* rhs, int mode);
void launch_gsrb_full_march(hipStream_t st, TileSpan tiles, const LevelDev& L, double* out,
                            const double* phi, const double* psi, const double* rhs, int color);
// red + black in one launch for the cells three layers inside their box (full19_fused.hip), then -- after the between-colour
// ghost work on `out` -- the black cells of the outer layers in place (full19_march.hip, MODE 3)
void launch_full_fused(hipStream_t st, TileSpan tiles, const LevelDev& L, double* out, const double* phi,
                       const double* psi, const double* rhs);
void launch_gsrb_full_shell(hipStream_t st, TileSpan tiles, const LevelDev& L, double* phi, const double* phi_in,
                            const double* psi, const double* rhs);
void launch_flux_full(hipStream_t st, const LevelDev& L, double* const out[3], const double* phi, const double* psi);
void launch_op_full(hipStream_t st, const LevelDev& L, double* out, const double* phi, const double* psi,
                    const double* rhs, int mode);
void launch_gsrb_full(hipStream_t st, const LevelDev& L, double* phi, const double* psi, const double* rhs, int color);

// loose: 0 LevelGSRB pass; 1 / 2: interior / box-shell phase of LooseGSRB (see k_gsrb_ortho)
// pull: refresh the ghosts the pass reads inside the kernel (LevelDev::tile_items; LevelGSRB passes only)
void launch_gsrb_ortho(hipStream_t st, const LevelDev& L, double* phi, const double* rhs, int color, int loose = 0,
                       bool pull = false);
// one full red+black sweep, phi_in -> phi_out (gsrb_fused.hip); needs phi_in ghosts 2 deep and
// rhs / Jg / Jinv ghosts 1 deep wherever a neighbouring box or periodic image exists
// in_mode 0: plain; 1: phi_in is taken to be all zeros and is not read; 2: phi_in is read as
// (value - sums[0]/sums[1]) (deferred mean removal of the zero-average prolongation); 3: phi_in is read as
// value + crse(i / r) (prolongation folded in; C = coarse level, crse exchanged one deep); 4: 3 and 2 together
// M: the level's coefficient arrays in the fields' element type (metric_ptrs(L), or the fp32 copies)
void launch_gsrb_fused(hipStream_t st, TileSpan tiles, const LevelDev& L, const MetricPtrs<double>& M,
                       double* phi_out, const double* phi_in, const double* rhs, int in_mode, const double* sums,
                       const LevelDev* C, const double* crse, const int* r);
// the same sweep on fp32 fields and coefficients (mixed-precision depths); sums stay fp64
void launch_gsrb_fused(hipStream_t st, TileSpan tiles, const LevelDev& L, const MetricPtrs<float>& M,
                       float* phi_out, const float* phi_in, const float* rhs, int in_mode, const double* sums,
                       const LevelDev* C, const float* crse, const int* r);
// whether launch_gsrb_fused takes a uniform-metric kernel on this level (it then reads none of the four coefficient arrays)
bool fused_uniform_kernel(const LevelDev& L);
// k-marching operator/residual of a large level (resid_march.hip); mode 0: out = rhs - L[phi], 1: out = L[phi]
void launch_resid_march(hipStream_t st, TileSpan tiles, const LevelDev& L, double* out,
                        const double* phi, const double* rhs, int mode);
void launch_resid_restrict(hipStream_t st, TileSpan tiles, const LevelDev& F, const MetricPtrs<double>& M,
                           const LevelDev& C, double* crse, const double* phi, const double* rhs, const int r[3],
                           double dxProduct, double* volsum);
// the same on fp32 fields and coefficients (mixed-precision depths); volsum is accumulated in fp64
void launch_resid_restrict(hipStream_t st, TileSpan tiles, const LevelDev& F, const MetricPtrs<float>& M,
                           const LevelDev& C, float* crse, const float* phi, const float* rhs, const int r[3],
                           double dxProduct, double* volsum);
// The same three launches on NF = 2 or 3 fields of one level (multi_march.hip; PressureSolver::set_components): the
// coefficient arrays are streamed once per launch, each field's arithmetic is the single-field kernel's.
// Class-0 tiles of the 16-row forms on a streamed (non-uniform) diagonal metric without coarse-fine faces; fp64.
// The operator is handed over explicitly (L.P is not read) in one of two carriers OPS:
//   StencilParams   one operator for all fields;
//   FieldOps<NF>    one per field (PressureSolver::comp_set_op): P[f] is the level's StencilParams with the sides (neum /
//                   diri) and alpha / beta of field f's operator; everything else in it is the level's and equal in all of them.
// in_mode 0 (plain; NF = 2 only) or 1 (from zero) as above; the folded prolongation (3) stays with launch_gsrb_fused.
template <int NF>
struct SweepFields { double* out[NF]; const double* in[NF]; const double* rhs[NF]; };
template <int NF>
struct FieldOps { StencilParams P[NF]; };
template <int NF, class OPS>
void launch_gsrb_fused_nf(hipStream_t st, TileSpan tiles, const LevelDev& L, const SweepFields<NF>& F, const OPS& O, int in_mode);
// C null: out[f] = rhs[f] - L[phi[f]] on the level; else out[f] on C = the J-weighted average of it (ratio r; NF = 2 only)
template <int NF>
struct ResidFields { double* out[NF]; const double* phi[NF]; const double* rhs[NF]; };
template <int NF, class OPS>
void launch_resid_nf(hipStream_t st, TileSpan tiles, const LevelDev& F, const ResidFields<NF>& fields, const OPS& O,
                     const LevelDev* C, const int* r);
// The 19-point marching residual (mode 0: out[f] = rhs[f] - L[phi[f]]) and colour pass (mode 2: out[f] = phi[f] with the cells
// of `color` relaxed; out != phi) on NF = 2 fields of one level (full19_multi.hip; PressureSolver::set_components_full):
// the nine J g^{ab} planes and Jinv are streamed once per launch, each field's arithmetic is launch_full_march's /
// launch_gsrb_full_march's.  Every field has its own psi (right in the one-cell frames) and all share L.P.  Class-0 tiles of
// full_march_nf_rows(NF) region rows (two fields: 8), whatever L.full_rows says.  The three-field form (6 rows) measured
// slower than the single-field kernel and is not instantiated (profiles/r14_multi_full19.md).
template <int NF>
struct FullFields { double* out[NF]; const double* phi[NF]; const double* psi[NF]; const double* rhs[NF]; };
template <int NF>
void launch_full_march_nf(hipStream_t st, TileSpan tiles, const LevelDev& L, const FullFields<NF>& F, int mode, int color);
int full_march_nf_rows(int nf);
// crse(ic) = sum over the children of ic of dxProduct / fjinv(child): the volume a coarse value is spread over
void launch_child_volume(hipStream_t st, const LevelDev& C, const LevelDev& F, double* crse, const int r[3],
                         double dxProduct);
void launch_sum_partials(hipStream_t st, const double* partials, int n, double* out);  // out[0] = sum (fixed order)
// out[0] = a[0] + b[0]; out[1] = c[0]
void launch_combine_sums(hipStream_t st, double* out, const double* a, const double* b, const double* c);
// one colour of vertical-line GSRB (line_gsrb.hip); ctiles = whole-column tiles (k0 = 0, nk = n2)
// LineGSRBIter2D (space_dim 2: lines along y); maxN0: the widest local box in x
void launch_line_gsrb_2d(hipStream_t st, const LevelDev& L, int maxN0, double* phi, const double* rhs, double* dmod, int color,
                         const double* psi);
void launch_line_gsrb_ortho(hipStream_t st, TileSpan ctiles, int tile_j, const LevelDev& L,
                            double* phi, const double* rhs, double* dmod, int color, const double* psi = nullptr);
void launch_op_ortho(hipStream_t st, const LevelDev& L, double* out, const double* phi, const double* rhs, int mode,
                     bool pull = false);
// Face-valued Neumann sides of a diagonal-metric level (ops: its GHOST_NEUM_FACE ops; foff[6 * patch + 2 * dir + side]: the
// start of that patch's slice of L.bc_face, -1 where there is none).  The cells next to those sides evaluated again with the
// planes' values as their boundary fluxes (mode as launch_op_ortho), over the result an operator launch left in out ...
void launch_op_neum_face(hipStream_t st, const LevelDev& L, const GhostOp* ops, int nops, const long long* foff, double* out,
                         const double* phi, const double* rhs, int mode);
// ... and the planes' values into the boundary faces of a face-centred field (flux[a]: direction a, null: skipped)
void launch_set_neum_faces(hipStream_t st, const LevelDev& L, const GhostOp* ops, int nops, double* const flux[3]);
void launch_lapdiag(hipStream_t st, const LevelDev& L);
void launch_diag(hipStream_t st, const LevelDev& L, double* phi, const double* r, int mode);
void launch_restrict(hipStream_t st, const LevelDev& C, const LevelDev& F, double* crse, const double* fine,
                     const int r[3]);
void launch_prolong(hipStream_t st, const LevelDev& F, const LevelDev& C, double* fine, const double* crse,
                    const int r[3], bool zeroAvg, double dxProduct, double* partials, double* sums,
                    long long fieldElems, bool ordered = false);
void launch_sub_mean(hipStream_t st, double* f, long long n, const double* sums);
void launch_avg_harmonic(hipStream_t st, const LevelDev& C, const LevelDev& F, double* crse, const double* fine,
                         const int r[3]);
void launch_avg_face(hipStream_t st, const LevelDev& C, const LevelDev& F, int patch, const int cn[3], double* crse,
                     const double* fine, int dir, const int r[3]);
void launch_copy_items(hipStream_t st, const LevelDev& L, const CopyItem* items, int nitems, double* f);
void launch_copy_items(hipStream_t st, const LevelDev& L, const CopyItem* items, int nitems, float* f);
void launch_pack(hipStream_t st, const LevelDev& L, const CopyItem* items, const long long* bufoff, int nitems,
                 double* f, double* buf, bool pack);
void launch_pack(hipStream_t st, const LevelDev& L, const CopyItem* items, const long long* bufoff, int nitems,
                 float* f, float* buf, bool pack);
void launch_set(hipStream_t st, double* a, long long n, double v);
void launch_set(hipStream_t st, float* a, long long n, float v);
// n device values -> coherent host memory, then the sequence number (system-scope release)
void launch_publish(hipStream_t st, const double* src, int n, double* host_dst, unsigned long long* host_seq,
                    unsigned long long seq);
void launch_copy(hipStream_t st, double* d, const double* s, long long n);
void launch_copy(hipStream_t st, float* d, const float* s, long long n);
void launch_incr(hipStream_t st, double* y, const double* x, double a, long long n);
void launch_incr(hipStream_t st, double* y, const float* x, double a, long long n);   // y += a * (double)x
// mixed-precision boundary: n values converted, one launch for up to four arrays (dst[q] = src[q]; null pairs are skipped)
void launch_convert(hipStream_t st, float* const dst[4], const double* const src[4], long long n);
void launch_convert(hipStream_t st, double* dst, const float* src, long long n, double scale = 1.0);   // dst = scale * src
void launch_convert(hipStream_t st, float* dst, const double* src, long long n, double scale = 1.0);
void launch_incr2(hipStream_t st, double* y1, const double* x1, double a1, double* y2, const double* x2, double a2, long long n);
void launch_bicg_p(hipStream_t st, double* p, const double* v, const double* r, double beta, double bw, long long n);  // p = (p*beta + bw*v) + r
void launch_incr_copy(hipStream_t st, double* y, double* x, double a, long long n);  // y += a*x; x = y
void launch_scale(hipStream_t st, double* y, double a, long long n);
void launch_mul(hipStream_t st, double* y, const double* x, long long n);   // y *= x elementwise
void launch_axby(hipStream_t st, double* z, const double* x, const double* y, double a, double b, long long n);
// where a reduction's result is also stored for the host: coherent host memory + a sequence number the host spins on
// (PressureSolver::fetch_scalars); fused into the reduction's last kernel it saves the separate one-thread publish launch
struct ScalarPublish { double* host_dst; unsigned long long* host_seq; unsigned long long seq; };
// the whole BiCGStab bottom solve of a tiny level in one single-workgroup launch (k_tiny_bicgstab, kernels.hip); the caller
// fills phi, rhs, w (r, r~, e, p, p~, s~, t, v), the parameters, info (device, 2 doubles: iterations, exit code) and pub
struct TinyBicg {
    const Tile* tiles; int ntiles; int tile_j;
    const PatchDesc* patches; int npatches;
    const CopyItem* items; int nitems;
    long long field_elems;
    const double* jg[3]; const double* jinv; const double* lapd;
    StencilParams P;
    double* phi; const double* rhs;
    double* w[8];
    int imax, numRestarts, normType, precondIters;   // precondIters: 0 no preconditioner, < 0 the diagonal scaling alone (a level the reference's sweep does not visit)
    double eps, reps, hang, small, metric;
    double* info;
    ScalarPublish pub;
};
void launch_tiny_bicgstab(hipStream_t st, const LevelDev& L, const CopyItem* items, int nitems, long long field_elems, TinyBicg A);
// the BiCGStab bottom solve of a level of up to BOX_MAX_WG boxes of up to BOX_MAX_CELLS cells as ONE persistent launch, one
// workgroup per box (k_box_bicgstab, kernels.hip): device-wide barriers where the launch-by-launch path has kernel boundaries.
// nb: for every valid cell (boxes back to back, Fortran order inside a box; box b starts at cstart[b]) the field offsets of the
// six cells its stencil reads (x-, x+, y-, y+, z-, z+): the neighbour itself, or -- across a box edge -- the valid cell the ghost
// exchange would have copied from (built on the host from the level's exchange plan), so no ghost cell is ever filled.
constexpr int BOX_MAX_WG = 128, BOX_MAX_CELLS = 2048;
// 19-point variant: cells of a box grown by one cell; per box and ghost program the entries (one per written cell), stages and
// cross-term Neumann ghost cells the kernel keeps in LDS
constexpr int BOX_FAB_MAX = 2048, BOX_MAX_ENT = 2048, BOX_MAX_STAGES = 63, BOX_MAX_NEUM = 512;
// One written cell of a ghost program, compiled on the host from the box's GhostOps (PressureSolver::build_box_tables): indices
// into the LDS copy of the box grown by one cell.  kind 0: dst := src (the other field); 1 / 2 / 3: extrapolation of order
// 0 / 1 / 2 from s1, s2, s3; 4: the cross-term Neumann ghost (flags: direction and side; nslot: its coefficient triple).
struct alignas(4) BoxProgEntry {
    unsigned short dst, s1, s2, s3;
    unsigned char kind, flags;   // flags: bit 0 dst field (1 = psi), bit 1 src field, bits 2-3 direction, bit 4 high side
    unsigned short nslot;
};
struct BoxBicg {
    const PatchDesc* patches; int npatches;
    const int* nb; const int* cstart;
    const double* jg[3]; const double* jinv; const double* lapd;
    StencilParams P;
    double* phi; const double* rhs;
    double* z[2];        // p~ and s~ in the level's layout: the only fields a workgroup reads outside its own box
    int imax, numRestarts, normType, precondIters;   // precondIters: 0 no preconditioner, < 0 the diagonal scaling alone (a level the reference's sweep does not visit)
    double eps, reps, hang, small, metric;
    double* sums;        // 4 * BOX_MAX_WG doubles: per-box partial results of the running reduction(s), double-buffered
    unsigned* sync;      // BOX_MAX_WG + 1: per workgroup the number of the last barrier it reached; abort flag (a barrier gave up); zeroed per launch
    // 19-point variant (non-diagonal metric, 3-D, boxes of at most 256 cells): all J g^{ab}; for every cell of box b grown by one
    // cell (x fastest, box b starts at fab_start[b]) the field offset its value comes from -- the cell itself, the valid cell
    // the ghost exchange copies there, or -1 (a ghost beyond a wall: the program fills it); the ghost programs [0] operator,
    // [1] smoother compiled into per-cell entries: box b owns ent[w][ent_first[w][b] .. ent_first[w][b + 1]), sorted by stage;
    // stg[w][stg_first[w][b] ..]: where each of its stages starts (relative to the box's first entry; one more than stages);
    // nfg[w][nfg_first[w][b] ..]: the boundary face (field offset) of each of its cross-term Neumann ghost cells
    int full;
    const double* jgf[3][3];
    const int* fab_src; const int* fab_start;
    const BoxProgEntry* ent[2]; const int* ent_first[2];
    const int* stg[2]; const int* stg_first[2];
    const int* nfg[2]; const int* nfg_first[2];
    long long* dbg;      // optional (SOMAR_BOX_TIMING=1): workgroup 0's clock ticks in {staging loads, ghost program, stencil, barrier, sums, count}
    int serial;          // sums in the reference's serial order (levels of at most ordered_max cells) or by a fixed tree per box
    double* info;        // device: iterations, exit code
    ScalarPublish pub;
};
void launch_box_bicgstab(hipStream_t st, const LevelDev& L, int max_box_cells, BoxBicg A);
// streaming probe (diagnostics): kind 0 copy, 1 read, 2 six reads + one write; in6: six arrays of `cells` doubles
void launch_stream_probe(hipStream_t st, int kind, int workgroups, double* const* in6, double* out, long long cells);
constexpr int MM_CH = 64;   // k-chunks per patch of k_minmax_all
// metric refresh (metric_refresh.hip): every coarse metric array of one MG depth from the next finer one in one launch --
// item dir 0..2: arithmetic average over faces(valid, dir) (k_avg_face), dir -1: harmonic cell average (k_avg_harmonic)
struct CoarsenItem { const double* fine; double* crse; int patch; int dir; };
void launch_coarsen_metric(hipStream_t st, const LevelDev& C, const LevelDev& F, const CoarsenItem* items, int nitems,
                           int gy, const int r[3]);
// (min, max) per (item, k-chunk) of a table of arrays of any depth, over the valid cells (dir < 0) or the valid dir-faces of the
// item's patch: out[2 * (item * MM_CH + chunk)] = min, [... + 1] = max
struct MinMaxItem { const double* a; const PatchDesc* patches; int patch; int dir; };
void launch_minmax_all(hipStream_t st, const MinMaxItem* items, int nitems, double* out);
// mode 0: sum a*b, 1: max|a|, 2: sum|a|, 3: signed max a  -> out[0] (device)
// ordered: reference-ordered serial sum (modes 0 and 2; meant for small levels, see k_reduce_ordered)
void launch_reduce(hipStream_t st, const LevelDev& L, const double* a, const double* b, int mode, double* partials,
                   double* out, bool ordered = false, const ScalarPublish* pub = nullptr);
// mode 0 (sum a*b) with a in fp32: each term and the sum in fp64, in the tree order of the fp64 form
void launch_reduce(hipStream_t st, const LevelDev& L, const float* a, const double* b, int mode, double* partials,
                   double* out);
// sharded small level: the rank's per-cell terms into their slot of the serial sequence (mode 0: a*b, 2: |a|, 6: X = dxProduct/b*a,
// Y = dxProduct/b), then -- after a sum-allreduce of X (and Y) -- the walk in the reference's order (k_reduce_ordered_flat)
void launch_ord_fill(hipStream_t st, const LevelDev& L, const long long* start, const double* a, const double* b,
                     int mode, double dxProduct, double* X, double* Y);
void launch_reduce_ordered_flat(hipStream_t st, int nboxes, const long long* box_start, const double* X, const double* Y,
                                int mode, double* out);
void launch_div_mac(hipStream_t st, const LevelDev& L, double* out, const double* u0, const double* u1,
                    const double* u2, double dt);
void launch_jgup_from_dxdxi(hipStream_t st, long long n, int mu, const double* const x9[9], const double* J, double scale,
                            double* out);
void launch_altered_jgup(hipStream_t st, long long n, double* dest, const double* nsq, const double* dmu,
                         const double* dnu, const double* ix, const double* jy, const double* iy, const double* jx,
                         const double* gup, const double* J, double theta, double coriolisF, bool offdiag);
void launch_face_axpy(hipStream_t st, const LevelDev& L, double* const vel[3], double* const grad[3], double s);
void launch_mac_correct(hipStream_t st, const LevelDev& L, double* const vel[3], const double* phi, double dtScale);
// cell-centred level projection: CellToEdge (+ zero normal flux on walls), EdgeToCell + correction (null cc[a] = skip a)
void launch_face_wall(hipStream_t st, const LevelDev& L, double* const edge[3]);  // zero normal flux on solid walls (null = skip)
// coordinate maps' metric producers (maps.hip): kind 1 cylindrical (diagonal), 2 bathymetric (non-diagonal, nodal depth)
void launch_map_metric(hipStream_t st, const LevelDev& L, int kind, const double dXi[3], const double Lc[3],
                       const double* d_depth, const int dlo[2], const int dn[2], bool diagonal, const double* domLen = nullptr);
void launch_face_bc(hipStream_t st, const LevelDev& L, double* const edge[3], const int kind[6], const double value[6]);
void launch_cell_to_edge(hipStream_t st, const LevelDev& L, double* const edge[3], double* const cc[3], bool wall);
void launch_cc_correct(hipStream_t st, const LevelDev& L, double* const cc[3], const double* phi, double dtScale);
void launch_edge_to_cell_axpy(hipStream_t st, const LevelDev& L, double* const cc[3], double* const grad[3], double dtScale);
void launch_cf_homog(hipStream_t st, const CFCell* cells, int n, double* phi, const double c1[3], const double c2[3],
                     const double fac[3]);
void launch_copy_items2(hipStream_t st, const PatchDesc* spatches, const PatchDesc* dpatches, const CopyItem* items,
                        int nitems, const double* src, double* dst);
void launch_fill_hash(hipStream_t st, const LevelDev& L, double* f, unsigned long long seed);
// box I/O between caller arrays in DEVICE memory and the level's layout (box_io.hip): one launch for every local patch and
// component.  An item is one (patch, component): the caller's box (low corner, pitches; Fortran order) and the region to move,
// both in global indices.  The caller's pointers are a column of their own (ptrs[slot]; NULL skips the item), the only part of
// a table that changes between calls.  Item i owns the tiles [tile0, tile0 of item i + 1): tiles_ij tiles of BIO_THREADS
// (i, j) pairs of the region's flattened i-j plane for each chunk of BIO_KC k-planes.
constexpr int BIO_THREADS = 256, BIO_KC = 8;
struct BoxIoItem {
    int clo[3];      // low corner of the caller's box
    int cpj;         // caller j pitch (elements)
    long long cpk;   // caller k pitch
    long long coff;  // where this item's component starts in the caller's array (elements)
    int rlo[3];      // low corner of the region
    int n[3];        // its size; never empty
    int patch;
    int comp;        // which of the launch's fields (the cell-centred velocity: its component)
    int slot;        // row of the pointer column: the local patch
    int tile0, tiles_ij;
    int pad_;
};
// field[comp]: the level's arrays (unused entries null); to_level: caller -> level, else level -> caller
void launch_box_io(hipStream_t st, const LevelDev& L, const BoxIoItem* items, double* const* ptrs, int nitems, int ntiles,
                   double* const field[3], bool to_level);

}  // namespace somar
