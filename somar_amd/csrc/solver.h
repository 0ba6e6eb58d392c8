// somar_amd/csrc/solver.h -- host-side multigrid driver (C++), the MI355X counterpart of
//   MappedAMRPoissonOpFactory::MGnewOp      calculus/AMRElliptic/MappedAMRPoissonOpFactory.cpp:363-702
//   MappedMultiGrid<T>::define/init/cycle   calculus/AMRElliptic/MappedMultiGrid.H:328-434, 555-653
//   MappedAMRMultiGrid<T>::solveNoInitResid calculus/AMRElliptic/MappedAMRMultiGrid.H:979-1183
//   MappedAMRPoissonOp (level operator)     calculus/AMRElliptic/MappedAMRPoissonOp.cpp
//   LevelGSRB / Jacobi                      calculus/AMRElliptic/RelaxationMethods/GSRB.cpp:58-98, Jacobi.cpp:54-90
//   Chombo 3.1 BiCGStabSolver (EXTERNAL)    restated from its published algorithm
// All level data stay resident in HBM for the life of the solver; the host only sequences
// kernel launches on one HIP stream and reads back the few scalars the stopping tests need.
#pragma once
#include <exception>
#include <functional>
#include <memory>
#include <vector>

#include "level.h"
#include "outer_loop.h"   // StopCriteria, SolveStats, OuterLoop, tga_coefficients

namespace somar {

enum { RELAX_JACOBI = 0, RELAX_LEVEL_GSRB = 1, RELAX_LOOSE_GSRB = 2, RELAX_LINE_GSRB = 3 };  // ProblemContext.H:322-340
enum { PRECOND_NONE = -1, PRECOND_DIAG_RELAX = 0, PRECOND_DIAG_LINE_RELAX = 1 };

// AMRPressureSolver::setAMRMGParameters / setBottomParameters (projection/AMRPressureSolver.H:53-77);
// defaults utils/ProblemContext.cpp:1147-1236.  StopCriteria (outer_loop.h): imin, imax, eps, hang, normThresh
struct SolverParams : StopCriteria {
    int num_smooth_down = 2, num_smooth_up = 2, num_smooth_bottom = 2, num_smooth_precond = 2;
    int numMG = 1, maxDepth = -1, precondMode = PRECOND_DIAG_RELAX, relaxMode = RELAX_LEVEL_GSRB;
    int verbosity = 0;
    int spaceDim = 3;  // 2: the reference built with CH_SPACEDIM = 2 (boxes one cell thick in z, which is inactive)
    int bottom_imax = 80, bottom_numRestarts = 5, bottom_normType = 2, bottom_verbosity = 0;
    double bottom_eps = 1e-6, bottom_reps = 1e-12, bottom_hang = 1e-15, bottom_small = 1e-30;
};

class PressureSolver {
public:
    // shared: run on the caller's stream (the levels of an AMR hierarchy share one) instead of an own one
    // tune: the execution-path switches, fixed for the life of the solver; a composite (AMRSolver, LepticSolver, the
    // agglomerated tail) reads the environment once and hands every part the same value
    PressureSolver(Comm* comm, hipStream_t shared, const Tuning& tune);
    ~PressureSolver();

    // ---- definition (MappedAMRPoissonOpFactory::define + MappedAMRMultiGrid::define) -----
    void define(const IBox& domain, const bool periodic[3], const double dx[3], const int bc_type[3][2],
                const std::vector<IBox>& boxes, const std::vector<int>& owner, double alpha, double beta,
                const SolverParams& prm, const double* dxCrse = nullptr);
    bool has_cf() const { return hasCF_; }
    const double* dx_crse() const { return hasCF_ ? dxCrse_ : nullptr; }
    // Diagonal metric of one LOCAL patch in Chombo FRA layout: Jg_aa on faces(valid,a), Jinv on valid.
    void set_metric_ortho(int patch, const double* jg0, const double* jg1, const double* jg2, const double* jinv);
    // Non-diagonal metric of one LOCAL patch: jgD = J g^{Db} on faces(valid, D), 3 components, component slowest
    // (LevelGeometry::getFCJgup's FluxBox layout).  Switches the solver to the 19-point kernels (full19.hip).
    void set_metric_full(int patch, const double* jg0, const double* jg1, const double* jg2, const double* jinv);
    // a Cartesian map's constants (CartesianMap::fill_Jgup / fill_Jinv) into every local patch, on the device
    void set_metric_uniform(const double c4[4]);
    bool is_full() const { return full_; }
    // before finalize: switch this solver to the non-diagonal path with every cross plane allocated (zero) -- for callers that
    // fill the metric planes of level(0).dev.jgf on the device themselves (the leptic solver's J-scaled and flat operators)
    void make_full();
    // ghost-op lists built with the reference's helpers for other callers (leptic): which 0 = extrapAllGhosts(phi, order 2)
    // (ExtrapolationUtils.cpp:388-420), 1 = ExtrapolateFaceAndCopy(phi, phi, FAB & domain, vertical dir, lo then hi, order 2)
    // (levelVertHorizGradient, LevelLepticSolver.cpp:1107-1176); run on depth 0, in place on phi
    void run_aux_program(int which, double* phi);
    void set_amr_member() { amr_member_ = true; }
    bool amr_member() const { return amr_member_; }  // a level of an AMRSolver hierarchy (whose reflux tables carry beta)
    void finalize();  // builds the semicoarsened hierarchy, coarse metrics, lapDiag, null-space probes
    // ---- metric refresh of a finalized solver (the implicit-gravity projector's per-step AlteredMetric, AMRNavierStokes-
    // AdvancePPMIG.cpp:331-342): between begin and end the set_metric_* producers write the depth-0 arrays in place; end
    // recomputes what finalize derived from the metric (ghosts, lapDiag, coarse depths, uniform / zero-plane flags, folded-
    // prolongation volumes, null-space probes; the agglomerated tail) into the existing buffers and drops the graphs.
    // amr_member_ok: the caller is the hierarchy (AMRSolver::metric_update_begin).  only_if_written: refresh only when a
    // producer ran since begin; returns whether it refreshed.
    void metric_update_begin(bool amr_member_ok = false);
    bool metric_update_end(bool only_if_written = false);
    bool metric_updating() const { return updating_; }
    void refresh_metric();   // the recomputation alone (no begin / end bookkeeping): leptic internal solvers
    void check_idle(const char* what) const;   // refuses while a metric update is open

    // ---- data movement across the boundary (caller-owned arrays, Chombo FRA layout) ---------------------
    // One resident array that crosses the boundary: its level, its level arrays (one per component) and what moves
    // (BoxIoShape).  Each array below has ONE description, whichever memory the caller's side lives in.
    struct CallerArray {
        Level* L;
        double* f[3];
        BoxIoShape shape;
    };
    CallerArray io_field(double* field, int depth, const int ghost[3], bool with_ghosts);   // a field at a depth; region valid.grow(ghost) or valid
    CallerArray io_vel(int dir);                                // MAC velocity J*u^dir on faces(valid, dir)
    CallerArray io_cc_vel(const int ghost[3], bool up);         // SpaceDim comps; up: one ghost layer in the space directions, down: valid cells
    CallerArray io_scale_cc(int which, const int ghost[3]);     // cell-centred J (0) / Jinv (1): the region of io_cc_vel up
    CallerArray io_scale_face(int which, int dir);
    CallerArray io_heat_flux(int dir);
    // which 0..2: J g^{aa} on faces(valid, a); 3: J^{-1}; 4: lapDiag (valid); 16 + 3a + b: J g^{ab} of the non-diagonal metric.
    // up: a producer writes depth 0 (set_metric_*); down needs a finalized solver
    CallerArray io_metric(int depth, int which, bool up);
    // The two movers.  Host memory: one local patch and one pointer (a null pointer or a patch index out of range is an
    // error); blocks until the caller's array is free / filled.  Device memory: a HOST table of one device pointer per local
    // patch, all of them in one launch (a null entry skips its patch); every pointer is checked before the launch unless
    // `checked` says a check_table did; drains the stream.
    void upload(const CallerArray& a, int patch, const double* host) { move_host(a, patch, const_cast<double*>(host), true); }
    void download(const CallerArray& a, int patch, double* host) { move_host(a, patch, host, false); }
    void move_dev(const CallerArray& a, double* const* dev, bool up, bool checked = false);
    // ---- calls on caller arrays: check every table, shape and (device memory) pointer; upload; run the resident call;
    // download.  Written once, with where the caller's arrays live as an argument: a table is one pointer per local patch
    // either way, and a null entry skips its patch.  Both memories follow the same rules: (1) nothing moves and nothing is
    // solved before every argument passed its check; (2) the ghost width of an array of which only valid cells move (rhs,
    // the velocity on its way down) is not bounded by the device frame; (3) null table entries skip.
    enum class Mem { Host, Device };
    void check_table(Mem where, const CallerArray& a, const double* const* table, const char* what);
    void move_table(Mem where, const CallerArray& a, double* const* table, bool up);   // after check_table
    void solve_on(Mem where, double* const* phi, const int phi_ghost[3], const double* const* rhs, const int rhs_ghost[3],
                  bool zeroPhi, bool forceHomogeneous, SolveStats& st);
    void mac_project_on(Mem where, double* const* const u[3], double dt, bool zeroPressure, bool forceHomogeneous, SolveStats& st);
    void cc_project_on(Mem where, double* const* vel, const int ghost[3], double dt, bool zeroPressure, bool forceHomogeneous,
                       bool wall, SolveStats& st);

    // ---- AMREllipticSolver::solve on the resident phi/rhs (AMREllipticSolver.H:33-48) -----
    void solve(bool zeroPhi, bool forceHomogeneous, SolveStats& st);

    // ---- pieces, exposed for benchmarks and kernel-level parity tests -----------------------
    // MG depths of the whole hierarchy (the agglomerated tail included)
    int depth() const { return coarse_ ? agglom_depth_ + coarse_->depth() : (int)lev.size(); }
    // Coarse-level agglomeration (sharded runs only): from the first depth with at most SOMAR_AGGLOM_CELLS cells
    // on, EVERY rank holds all boxes and runs the rest of the cycle redundantly -- no halo exchange, no
    // allreduce and no host round trip per BiCGStab scalar where the work is microseconds and the wire is not.
    // One allgather of the restricted residual goes down; nothing comes back (every rank already has the
    // correction).  Same arithmetic, same order (in fact the serial order), so results do not change.
    int agglom_depth() const { return coarse_ ? agglom_depth_ : -1; }
    PressureSolver* coarse_solver() { return coarse_.get(); }
    // depth d of the whole hierarchy; depths inside the agglomerated tail (d > agglom_depth()) are the replicated
    // solver's, depth == agglom_depth() is the sharded landing layout
    Level& level(int d) { return (coarse_ && d > agglom_depth_) ? coarse_->level(d - agglom_depth_) : *lev[d]; }
    std::array<int, 3> ref_ratio(int d) const
    {
        return (coarse_ && d >= agglom_depth_) ? coarse_->ref_ratio(d - agglom_depth_) : mgRefRatios.at(d);
    }
    double* phi() { return f_phi; }
    double* rhs() { return f_rhs; }
    double* work(int which);  // 0 uberResidual 1 uberCorrection 2 bestPhi
    double* field(int depth, int which);  // SOMAR_F_* handle -> device pointer (nullptr if absent)
    // e_zero: e is to be taken as all zeros, whatever it holds (saves the memset and the first sweep's read)
    // e_shift: device pointer to (sum, volume): e is to be read as e - sum/volume (deferred mean removal); only
    //          legal when fused_relax(d, iters) holds
    // e_plus: (coarse level, coarse correction): e is to be read as e + coarse(i / r) -- the prolongation folded
    //         into the first sweep; the coarse field must have been exchanged
    void relax(int d, double* e, const double* res, int iters, bool e_zero = false, const double* e_shift = nullptr,
               const Level* e_plus_level = nullptr, const double* e_plus = nullptr);
    bool fused_relax(int d, int iters) const;
    // homogeneous: physical BC values taken as zero (the values of Dirichlet sides and of face-valued Neumann sides)
    void residual(int d, double* out, double* phi, const double* rhs, bool homogeneous = true);   // homogeneous CF ghosts, then residual_i
    void apply_op(int d, double* out, double* phi, bool homogeneous = true);
    void residual_i(int d, double* out, double* phi, const double* rhs, bool homogeneous = true) // residualI: CF ghosts as they are
    {
        operator_i(d, 0, out, phi, rhs, homogeneous);
    }
    // residualI of depth 0 and its J-weighted average (MAPPEDAVERAGE2) onto the layout C coarsened by r, in ONE marching pass
    // (the fine residual is never stored); CF ghosts of phi as they are.  false: not available here (non-diagonal metric, small
    // level, a ratio entry other than 1 or 2) -- the caller then runs residual_i + launch_restrict
    bool residual_restrict_i(const LevelDev& C, double* crse, double* phi, const double* rhs, const int r[3]);
    void apply_op_i(int d, double* out, double* phi, bool homogeneous = true) { operator_i(d, 1, out, phi, nullptr, homogeneous); }
    // Dirichlet sides (EllipticConstDiriBCGhostClass, BCInterface/EllipticBCUtils.cpp:382-424): values per
    // {loX,hiX,loY,hiY,loZ,hiZ}, before finalize.  Such a solver runs the two-pass / direct-load kernels.
    void set_bc_values(const double v[6]);
    // Position-dependent values of the Dirichlet side (dir, side) (EllipticDiriBCGhostClass, BCInterface/EllipticBCUtils.cpp:
    // 548-646): one value per boundary face over the whole domain box of depth 0, Fortran order over the two transverse
    // directions in increasing order.  nullptr: back to the constant of set_bc_values.  Before or after finalize; after it
    // only copies into the existing device buffers (op lists and face values keep their addresses).
    void set_bc_face_values(int dir, int side, const double* values);
    // Position-dependent values of the Neumann side (dir, side) of a DIAGONAL-metric solver (EllipticNeumBCGhostClass /
    // EllipticNeumBCFluxClass, BCInterface/EllipticBCUtils.cpp:696-947): the layout of set_bc_face_values; a value is
    // J g^{dd} dphi/dxi_d at the face on both sides.  nullptr: back to zero Neumann.  Before or after finalize; after it only
    // copies into the existing device buffers.  The inhomogeneous operator of depth 0 takes them (operator_i), nothing else.
    void set_neum_face_values(int dir, int side, const double* values);
    bool has_neum_face_values() const
    {
        for (int d = 0; d < 3; ++d)
            for (int s = 0; s < 2; ++s)
                if (neum_face_[d][s]) return true;
        return false;
    }
    // a non-diagonal metric on a solver with face-valued Neumann sides is refused (who: the call that would set it)
    void refuse_full_with_neum_faces(const char* who) const;
    // Dirichlet or Neumann
    bool has_face_values() const
    {
        for (int d = 0; d < 3; ++d)
            for (int s = 0; s < 2; ++s)
                if (face_[d][s]) return true;
        return false;
    }
    // Non-diagonal metric on a level with coarse-fine boundaries:
    //   cf_ev: ExtrapolateCFEV(phi, cfregion, 2) -- the edge / vertex ghosts next to the CF faces, after a CF fill
    //   (interpCFGhosts, MappedAMRPoissonOp.cpp:2193-2216);  flux_fields: getFlux (fillExtrap + MAPPEDGETFLUX, beta = 1)
    //   on every face of depth 0, for the flux register (reflux, :1615-1707)
    void cf_ev(int d, double* phi);
    double* const* flux_fields(double* phi);
    void flux_at_faces(double* phi, FullFlux& ff);   // getFlux's operands for the register kernels: fillExtrap run, nothing stored
    void mac_grad_full(double* phi);  // f_flux := MAC gradient of phi, non-diagonal metric (phi exchanged)
    // the MAC gradient G^a = J g^{ab} d_b(phi) on every a-face of depth 0, STORED (either metric; phi exchanged, CF ghosts
    // filled by the caller): levelGradientMAC's per-box part (Gradient.cpp:124-160)
    double* const* mac_grad(double* phi);
    bool has_diri() const { return diri_; }
    bool bc_values_zero() const
    {
        for (int d = 0; d < 3; ++d)
            for (int s = 0; s < 2; ++s)
                if (bc_value_[d][s] != 0.0 || face_[d][s]) return false;
        return true;
    }
    // ConstInterpPS / ZeroAvgConstInterpPS of depth 0 from a coarse field living on layout C (AMRProlong)
    void prolong_from(const LevelDev& C, const double* crse, const int r[3], double* fine);
    double* amr_field(int which);  // 0 m_correction, 1 m_residual of MappedAMRMultiGrid (allocated on first use)
    void restrict_residual(int d, double* resCoarse, double* phiFine, const double* rhsFine);
    // defer_mean: leave the zero-average mean (if any) to the caller; returns the device (sum, volume) pair to
    //             subtract, or nullptr if nothing is pending
    const double* prolong_increment(int d, double* phiFine, const double* corrCoarse, bool defer_mean = false);
    void pre_cond(int d, double* phi, const double* rhs);
    void vcycle(double* e, const double* res, bool e_zero = false);  // MappedMultiGrid::oneCycle
    // ---- opt-in mixed precision (NOT the reference's arithmetic, which is fp64 throughout) -------------------------------
    // mode 0: fp64 (the default).  mode 1: the V-cycle's leading depths run in fp32 -- depth d does when the fused sweep runs
    // there (fused_relax) and it has at least min_cells cells (<= 0: the fused sweep's own threshold); the rest of the cycle,
    // the residuals and phi stay fp64, so the outer defect-correction loop still drives the fp64 residual.  Before or after
    // finalize (after: allocates the fp32 copies, converts the metric, drops the graphs); refused while a metric update is
    // open and where the fp32 path does not reach (mixed_refusal).  On a sharded solver the fp32 depths exchange their ghosts in
    // fp32 messages, so mode, min_cells and K are part of the message format: a finalized solver's set_precision (and a
    // finalize) is COLLECTIVE, every rank calls it with the same arguments -- ranks that disagree all get an error, and mode 0.
    void set_precision(int mode, long long min_cells);
    // payload bytes this rank has sent in the ghost exchanges of this solver's levels: [0] fp64 fields, [1] fp32 fields
    void exchange_bytes(long long out2[2]) const;
    int precision_mode() const { return mp_mode_; }
    int fp32_depths() const { return mp_K_; }
    // ---- several components on ONE operator (solver_multi.cpp) -----------------------------------------------------------
    // The viscous / diffusive solves of a time step run the same Helmholtz operator on SpaceDim (and more) fields; the reference
    // keeps one solver per velocity component (m_viscSolverPtrs[idir], NavierStokes/AMRNavierStokesInit.cpp:887-1010).  Here one
    // solver carries ncomp (1..4) components: each owns its depth-0 fields, all share the metric hierarchy, alpha / beta, the BC
    // types and Dirichlet values.  Component 0 is the solver's own fields, which every other call keeps addressing.  After
    // finalize; ncomp = 1 releases what the others held.  min_cells: a depth is BATCHED -- its sweeps and its residual +
    // restriction are launches that carry several active components and read the coefficient arrays once (multi_march.hip)
    // -- when it has at least that many cells (<= 0: the fused sweep's own threshold) and runs the fold path of the cycle on a
    // streamed metric (mc_setup); the depths below go through the single-field cycle, one component after the other.  Either way solve_multi
    // leaves every component as ncomp successive solve() calls would, bit for bit.  Refused where that does not reach
    // (multi_refusal).
    void set_components(int ncomp, long long min_cells);
    // The same on a handle with a NON-diagonal metric (19-point operator; refused on a diagonal one, which takes the call above).
    // A depth is batched -- its colour passes and residuals are N-field launches of full19_multi.hip, which stream the nine
    // J g^{ab} planes and Jinv once -- where the marching 19-point kernels run (full_march) and the fused red+black sweep does
    // not, before the serial-order sums and the graph-replayed legs, without coarse-fine faces or a zero-average prolongation,
    // with at least min_cells cells (<= 0: the marching kernels' own threshold).  The bottom depth of a hierarchy whose boxes
    // stop coarsening while the level still marches is batched too: its bottom sweeps, the bottom solve stays per field.  The ghost
    // programs stay per field (each component has a psi frame array of its own on the batched depths).  Components with an
    // operator of their own are not offered here (comp_set_op): the ghost programs carry one operator's sides and values.
    void set_components_full(int ncomp, long long min_cells);
    int components() const { return ncomp_; }
    int batched_depths() const { return mc_K_; }
    long long batched_launches() const { return mc_launches_; }   // N-field launches so far (tests: a case reached its kernels)
    // which: SOMAR_F_PHI (0), RHS (1), RES (2), CORR (3), BEST (4), HEAT_OLD (8), HEAT_SRC (9), depth 0; nullptr: no such field
    double* comp_field(int comp, int which);
    void solve_multi(bool zeroPhi, bool forceHomogeneous, std::vector<SolveStats>& st);
    void vcycle_multi(bool from_zero);   // per component: F_CORR := one V-cycle of F_RES, as vcycle(e, res, from_zero)
    void heat_step_multi(int scheme, double dt, bool zeroPhi, std::vector<SolveStats>& st);
    const std::vector<double>& comp_history(int comp) const;   // residual history of the component's last multi solve
    // ---- a component's own operator (solver_multi.cpp): BC type and Dirichlet constant per side {loX,hiX,loY,hiY,loZ,hiZ} and
    // the coefficient pair set_alpha_beta scales.  Component 0 is the solver's create-time operator and not settable; a
    // component without an operator of its own keeps the solver's (face-valued sides included).  The multi calls then leave
    // component c as the single-field call would on a separate one-component solver created with c's operator on the same
    // metric.  Refused (nothing changed): comp 0 or out of range, a type other than Neumann / Dirichlet on a non-periodic
    // side, an operator with a null space (the null-space probe run at every depth with the operator in place), an open
    // metric update.  A periodic (or inactive) direction keeps the solver's entries.
    void comp_set_op(int comp, const int bc_type6[6], const double bc_values6[6], double alpha, double beta);
    void comp_get_op(int comp, int bc_type6[6], double bc_values6[6], double* alpha, double* beta, bool* own);
    void comp_reset_op(int comp);
    long long op_launches() const { return mc_op_launches_; }   // N-field launches whose fields had different operators
    // MG ratios imposed on the first depths (set before finalize): the coarsening pattern of the mini V-cycle of a
    // level refined by more than 2 (MappedAMRMultiGrid.H:1455-1482), and that mini V-cycle itself (:742-754)
    std::vector<std::array<int, 3>> forcedRatios;
    void mini_vcycle(double* corr, const double* res);
    void bottom_solve(double* phi, const double* rhs);
    double norm(int d, const double* a, int ord);
    double dot(int d, const double* a, const double* b);
    void fill_hash(int d, double* f, unsigned long long seed);
    // ---- MAC level projection pieces (LevelMACProjector / BaseProjector::project), depth 0 -------------
    double* vel(int dir);   // resident face field J*u^dir (allocated on first use)
    void divergence_mac(double* out, double dt);                 // out = div(vel) [/ dt]
    void mac_correct(double* phi, double dt);                    // vel -= dt * G(phi)
    void mac_project(double dt, bool zeroPressure, bool forceHomogeneous, SolveStats& st);
    void set_metric_map(int kind, const double Lc[3], const double* depth, const int dlo[2], const int dn[2]);
    void set_vel_bc(const int kind[6], const double value[6]);   // inflow / outflow sides of BasicVelocityBCGhostClass
    void vel_wall_bc();   // the velocity BC levelDivergenceMAC applies through a_fluxBC, solid walls: zero wall-normal faces of vel()
    // viscous / diffusive Helmholtz solves through the same operator
    // amr_member_ok: the caller (AMRSolver::set_alpha_beta) looks after the flux-register scales, which carry beta
    void set_alpha_beta(double a, double b, bool amr_member_ok = false);
    // a_flux of the level heat integrators: thisFlux (+)= getFlux(phi) = J Grad(phi), NO beta (MappedBaseLevelHeatSolver::
    // incrementFlux, MappedBaseLevelHeatSolver.cpp:183-209; MappedAMRPoissonOp::getFlux(FluxBox&,...), :2129-2151); phi's ghosts
    // as the last operation left them
    void increment_heat_flux(double* phi, bool setToZero);
    double* heat_flux(int dir);
    double* heat_field(int which);             // 0: phiOld, 1: src (depth 0, allocated on first use)
    void heat_step(int scheme, double dt, bool zeroPhi, SolveStats& st);   // 0 backward Euler, 1 Crank-Nicolson, 2 TGA
    // cell-centred level projection (LevelCCProjector): velocity J*u, SpaceDim comps, resident with one ghost layer
    double* cc_vel(int comp);
    void divergence_cc(double* out, double dt, bool wall);                   // CellToEdge [+ wall BC] -> vel(); div [/ dt]
    void cc_correct(double* phi, double dt);                                 // cc_vel -= dt * EdgeToCell(G(phi))
    void cc_project(double dt, bool zeroPressure, bool forceHomogeneous, bool wall, SolveStats& st);
    // LevelGeometry::multByJ / divByJ on the resident velocities (geometry/LevelGeometryUtil.cpp:287-339, 372-420, 456-...):
    // data *= J resp. data *= Jinv, the scale arrays being the caller's (getCCJ / getCCJinv over valid.grow(ghost), fill_J /
    // fill_Jinv on the face boxes; they arrive through io_scale_cc / io_scale_face).  which: 0 = J, 1 = Jinv.  centring 0: the
    // MAC velocity (set per direction), 1: cell-centred.
    void scale_vel(int centring, int which);
    void remove_mean(int d, double* f);
    void sync();
    // per-kernel HIP-event timing of the depth-0 launches (0 = GSRB colour pass, 1 = operator/residual)
    void profile_enable(bool on);
    void profile_get(int kernel, int* count, double* total_ms);
    hipStream_t stream() const { return st_; }
    const Tuning& tuning() const { return tune_; }

    SolverParams prm;
    // The null-space probe compares against ProblemContext's GLOBAL AMRMG.eps (MappedAMRPoissonOpFactory.cpp:679), not
    // against this solver's own eps; a solver set up by another one (leptic: horizontal / full multigrid) inherits it.
    double probe_eps = -1.0;
    // bottom-solver state shared with MappedAMRMultiGrid (setConvergenceMetrics)
    double bottom_metric = -1.0, bottom_eps_eff = 1e-6;
    int bottom_iters = 0, bottom_exit = 0;
    long long counters[5] = {0, 0, 0, 0, 0};   // overlapped sweeps, one-launch ghost programs, staged ghost programs, bottom solves, fused 19-point sweeps
    int bottom_kind = 0;   // how the last bottom solve ran: 0 launch by launch, 1 k_tiny_bicgstab, 2 k_box_bicgstab
    std::vector<std::array<int, 3>> mgRefRatios;

private:
    void move_host(const CallerArray& a, int patch, double* host, bool up);
    void cycle(int d, double* corr, const double* res, bool corr_zero = false);
    // the stages of backward Euler, Crank-Nicolson and TGA, for heat_step and heat_step_multi (solver.cpp)
    void heat_stages(int scheme, double dt, bool zeroPhi, const std::function<void(const std::function<void()>&)>& each,
                     const std::function<void(bool)>& solve);
    // residual_i (mode 0) and apply_op_i (mode 1) in one: mode 0 out = rhs - L[phi] (timed in a profiled pass), mode 1 out = L[phi] (rhs unused)
    void operator_i(int d, int mode, double* out, double* phi, const double* rhs, bool homogeneous);
    // prolong_from and prolong_increment in one: depth d += the coarse field on layout C (ratio r), then the zero-average mean
    // removal (or its deferral)
    const double* prolong_onto(int d, const LevelDev& C, const double* crse, const int r[3], double* fine, bool defer_mean);
    // ---- mixed precision: depths 0 .. mp_K_ - 1 run the fold path of the cycle (below) on fp32 fields ----
    struct Depth32 {
        DevBuf<float> jg[3];   // fp32 copies of the metric (not made where the depth is uniform)
        DevBuf<float> jinv;
        DevBuf<float> corr, res, pp;   // correction, residual, ping-pong buffer (depth K: corr, res only)
    };
    int mp_mode_ = 0;
    long long mp_min_cells_ = 0;
    int mp_K_ = 0;                  // depths 0 .. mp_K_ - 1 run in fp32
    std::vector<Depth32> f32_;      // mp_K_ + 1 entries once set up
    std::string mixed_refusal() const;   // why mode 1 is not available here ("" = it is)
    void mp_setup();                // after finalize: K (agreed on by every rank), buffers, metric copies
    void mp_free();
    void mp_convert_metric();       // one launch per fp32 depth (finalize, set_precision, metric refresh)
    void cycle32(int d, float* corr, const float* res, bool corr_zero);   // the fp32 driver: fold path, seam conversion, recursion
    void vcycle_mixed(double* e, const double* res, double rnorm, bool e_zero, bool add_to_phi);
    // ---- the fold path of the cycle, ONE code path for T = double (relax / restrict_residual / cycle_up on their large-level
    // branches) and T = float (cycle32): fused sweeps, residual + restriction in one marching pass with the fold sums, the
    // prolongation folded into the first post-smoothing sweep.  Arguments as relax / restrict_residual take them.
    template <class T>
    void fused_sweeps(int d, T* e, const T* res, int iters, bool e_zero, const double* e_shift, const Level* e_plus_level,
                      const T* e_plus);
    template <class T>
    void march_restrict(int d, T* resCoarse, T* phiFine, const T* rhsFine);
    // crse: depth d + 1's correction; exchange_crse: it still needs its ghost exchange (not at the fp32 / fp64 seam, where the
    // fp64 field was exchanged before its conversion)
    template <class T>
    void fold_up(int d, T* corr, const T* res, T* crse, bool exchange_crse);
    // the element type shows in these four places only
    template <class T>
    T* pingpong(int d) const;                  // f_pp[d] | f32_[d].pp
    template <class T>
    MetricPtrs<T> metric(int d) const;         // the level's own arrays | their fp32 copies
    void diri_homog(int d, double* f) { apply_diri(d, f, true); }   // homogeneous Dirichlet ghosts
    void diri_homog(int d, float* f) { launch_ghost_ops(st_, lev[d]->dev, d_diri_ops_[d], n_diri_ops_[d], f); }
    // coarse-fine ghosts (ext: plus the edge ghosts the fused sweep's red ring reads); fp32 depths have none (mixed_refusal)
    void cf_fill(const Level& L, double* f, bool ext)
    {
        if (ext) L.cf_homog_ext(f, st_);
        else L.cf_homog(f, st_);
    }
    void cf_fill(const Level& L, float*, bool) { SOMAR_CHECK(L.ncf == 0, "internal: an fp32 depth with coarse-fine faces"); }
    // ---- several components (solver_multi.cpp) ----
    enum { MC_MAX = 4 };
    struct CompOp;   // a component's own operator (below, after CoarseGraph)
    // depth 0 of a component beyond 0; op: its own operator, null while it shares the solver's
    struct Component { DevBuf<double> phi, rhs, res, corr, best, heat[3]; std::unique_ptr<CompOp> op; };
    struct CompDepth { DevBuf<double> corr, res, pp, psi; };   // psi: non-diagonal metric (the frame array of the ghost programs)
    int ncomp_ = 1;
    long long mc_min_cells_ = 0, mc_launches_ = 0, mc_op_launches_ = 0;
    int mc_K_ = 0;                                   // depths 0 .. mc_K_ - 1 are batched
    std::vector<Component> comps_;                   // [comp - 1]
    // [comp][depth 0 .. K]: component 0 takes the solver's own arrays on the batched depths and owns depth K's pair only (the
    // seam: every component's restricted residual waits there for its turn in the single-field cycle); the others own corr / res
    // of depths 1 .. K and a ping-pong buffer per batched depth
    std::vector<std::vector<CompDepth>> mc_depth_;
    // per batched depth: class-0 tables of the N-field sweep / residual; non-diagonal metric: mc_ftiles_ alone, of the
    // 19-point kernels' two-field (8-row) form
    std::vector<TileTable> mc_ftiles_, mc_rtiles_;
    bool mc_full_call_ = false;                      // set_components_full is asking (multi_refusal)
    std::vector<std::vector<double>> mc_history_;
    std::string multi_refusal() const;               // why ncomp > 1 is not available here ("" = it is)
    void mc_setup();                                 // K, the components' buffers, the tile tables (set_components, metric refresh)
    void mc_free();
    // component comp's depth-0 fields <-> the solver's own, and its operator, if it has one, <-> the solver's (comp 0: nothing)
    void swap_comp(int comp);
    // runs f with component comp in the place of the solver's own fields: the single-field code on that component.  (Where the
    // graph-replayed legs start at depth 0 -- a level of at most Tuning::graph_cells cells, so nothing is batched and every
    // multi call comes here -- the graphs are keyed on depth 0's correction / residual arrays, which change with the
    // component: graph_cycle drops and recaptures them per component and call.  Same results; such a handle pays a graph
    // instantiation per component where a one-component handle replays.)
    template <class Fn>
    void on_comp(int comp, Fn f)
    {
        swap_comp(comp);
        ScopeExit back{[&]() { swap_comp(comp); }};
        f();
    }
    // the fields of the active components, by position in the active list
    struct CompFields { int n = 0; int comp[MC_MAX]; double* corr[MC_MAX]; double* res[MC_MAX]; };
    double* mc_corr(int comp, int d) const { return (comp == 0 && d < mc_K_) ? f_corr[d].get() : mc_depth_[comp][d].corr.get(); }
    double* mc_res(int comp, int d) const { return (comp == 0 && d < mc_K_) ? f_res[d].get() : mc_depth_[comp][d].res.get(); }
    double* mc_pp(int comp, int d) const { return comp == 0 ? f_pp[d].get() : mc_depth_[comp][d].pp.get(); }
    double* mc_psi(int comp, int d) const { return comp == 0 ? f_psi[d].get() : mc_depth_[comp][d].psi.get(); }
    // per active component: the bottom solver's convergence metric going in (null: as it stands), its counts coming out
    struct CompBottom { const double* metric = nullptr; int iters[MC_MAX], exit[MC_MAX]; };
    void multi_cycle(int d, const CompFields& F, bool corr_zero, CompBottom& B);
    void multi_sweeps(int d, const CompFields& F, int iters, bool e_zero, double* const* e_plus);
    void multi_restrict(int d, const CompFields& F, double* const* crse);
    // the same three on a batched depth of a non-diagonal metric, as relax() / restrict_residual() / prolong_increment() run there
    void multi_full_sweeps(int d, const CompFields& F, int iters, bool e_zero);
    void multi_full_restrict(int d, const CompFields& F, double* const* crse);
    // mode 0: out[i] = rhs[i] - L[phi[i]] (the frame programs of the operator have run), 2: the colour pass out[i] := phi[i] with
    // `color` relaxed (those of the smoother have): N-field launches by the launch plan, a lone field through the level's own table
    void multi_full_launches(int d, int n, const int* comp, double* const* out, double* const* phi, double* const* rhs, int mode,
                             int color);
    // out[i] = rhs[i] - L[phi[i]] on depth 0 with the physical BCs (homogeneous or not), as residual()
    // (comp[i]: the component of position i, whose operator the physical ghosts and the launch take)
    void multi_residual0(int n, const int* comp, double* const* out, double* const* phi, double* const* rhs, bool homogeneous);
    double fetch_scalar(int slot);
    void fetch_scalars(int slot, int n);
    unsigned long long fetch_seq_ = 0;
    unsigned long long* h_seq_ = nullptr;  // in the coherent host block behind h_scalars
    bool build_coarser(int depth);
    void probe_null_space(int d);
    void fill_metric_ghosts(Level& L);
    // StencilParams::uniform / uc (diagonal metric) resp. zero_xy (non-diagonal metric) of every 3-D depth, in one k_minmax_all
    // launch and one download; then the tile tables that follow from them (finalize and metric refresh)
    void detect_metric_flags();
    void choose_narrow_tiles();    // lane classes of the 7-point marching tables per depth; re-sizes d_partials after a rebuild
    bool updating_ = false, metric_written_ = false;
    void metric_written(const char* producer);   // a producer's check: before finalize, or inside an open update
    std::vector<DevBuf<CoarsenItem>> d_coarsen_;        // per depth d >= 1: k_coarsen_metric's work items (built at the first refresh)
    std::vector<int> n_coarsen_, gy_coarsen_;
    DevBuf<MinMaxItem> d_mm_items_;
    int n_mm_items_ = 0;
    std::vector<int> mm_first_;                  // per depth: first item of (jg0, jg1, jg2, jinv) resp. (jgf01, jgf10), 4 / 2 arrays
    DevBuf<double> d_mm_out_;
    void line_relax(int d, double* e, const double* res);
    DevBuf<double> f_vel[3], f_ccvel[3], f_heat[3], f_sc_cc[2], f_sc_face[2][3];
    double aCoef_ = 0.0, bCoef_ = 1.0;  // the factory's alpha / beta (MappedAMRPoissonOpFactory.cpp:585-586)
    bool coefs_saved_ = false;
    bool velbc_default_ = true;                      // every non-periodic side a solid wall
    int velbc_kind_[6] = {0, 0, 0, 0, 0, 0};
    double velbc_value_[6] = {0, 0, 0, 0, 0, 0};
    bool amr_member_ = false;
    DevBuf<double> f_amr[2];
    bool hasCF_ = false;
    DevBuf<double> f_heatflux[3];
    bool own_stream_ = true;
    double dxCrse_[3] = {0, 0, 0};
    std::vector<DevBuf<double>> f_pp;  // per-depth ping-pong buffer of the fused sweep
    // LevelGSRB sweeps the shells of the domain shrunk by one cell (RelaxationMethod::collectBoundaryData) and the cells inside
    // it: when two or more active directions of the domain are at most two cells wide every one of those boxes is empty, and
    // a sweep of the reference touches no cell at all (a preconditioner is then its diagonal scaling alone)
    bool unswept(int d) const
    {
        const Level& L = *lev[d];
        int narrow = 0;
        for (int a = 0; a < 3; ++a)
            if (L.active[a] && L.domain.size(a) <= 2) ++narrow;
        return prm.relaxMode == RELAX_LEVEL_GSRB && narrow >= 2;
    }
    bool fused_bottom(int d) const;   // the whole BiCGStab bottom solve in one single-workgroup launch (k_tiny_bicgstab)
    // the BiCGStab bottom solve of a multi-box bottom level as one persistent launch, one workgroup per box (k_box_bicgstab;
    // Tuning::box_bottom, and box_bottom_min_cells except on a level of ONE box).  The neighbour table is built at the first use.
    bool box_bottom(int d) const;
    void build_box_tables(int d);
    int box_depth_ = -1, box_max_cells_ = 0;
    struct BoxTables {
        DevBuf<int> nb, cstart, fab, fabstart;
        DevBuf<double> sums;
        DevBuf<unsigned> sync;
        // 19-point variant: the two ghost programs compiled into per-cell entries (kernels.h: BoxProgEntry), per box
        DevBuf<BoxProgEntry> ent[2];
        DevBuf<int> entfirst[2], stg[2], stgfirst[2], nfg[2], nfgfirst[2];
    };
    BoxTables box_;
    bool box_full_ok_ = false;   // the compiled programs fit the kernel's LDS tables
    bool ordered(int d) const { return lev[d]->valid_cells_global <= tune_.ordered_reduce_max; }
    // large 3-D levels of the diagonal path run the k-marching 7-point kernels (resid_march.hip); full_march is the 19-point twin
    bool ortho_march(int d) const
    {
        const Level& L = *lev[d];
        return !full_ && L.active[2] && L.valid_cells_global >= tune_.march_min_cells;
    }
    // A small level that is SHARDED keeps the serial order too: every rank contributes the per-cell terms of its boxes to
    // one vector in the serial (box after box) sequence, a sum-allreduce completes it, one wavefront walks it
    // (k_ord_fill / k_reduce_ordered_flat) -- so a sharded solve adds the same numbers in the same order as one rank.
    bool ord_sharded(int d) const { return ordered(d) && comm_->size > 1; }
    DevBuf<double> d_ordbuf_;                // 2 * Tuning::ordered_reduce_max doubles
    std::vector<DevBuf<long long>> d_ord_start_, d_box_start_;  // per depth: serial start of each LOCAL patch / of every box (+ end)
    void ordered_sums(int d, const double* a, const double* b, int mode, double dxProduct, double* out);
    // out[0] = sum over the level (mode 0: a*b, 2: |a|), every rank: serial order on small levels, tree order on large ones
    bool fused_publish(int d) const;
    double reduce_fetch(int d, const double* a, const double* b, int mode);   // reduction + host fetch, published by the reduction
    void wait_published(unsigned long long want);
    // a one-launch bottom solve whose published (iterations, exit code) the host has not read yet: the sequence number it
    // publishes (0: none).  graph_cycle defers the read until the up leg is enqueued (Tuning::bottom_async); every other caller
    // of bottom_solve reads at once.
    void bottom_collect();
    unsigned long long bottom_pending_ = 0;
    bool bottom_defer_ = false;
    void reduce_sum(int d, const double* a, const double* b, int mode, double* out);

    const Tuning tune_;
    Comm* comm_;
    Comm self_;
    hipStream_t st_ = nullptr;
    std::vector<std::unique_ptr<Level>> lev;
    std::vector<DevBuf<double>> f_res, f_corr, f_scratch;  // per depth
    DevBuf<double> f_phi, f_rhs, f_uberRes, f_uberCorr, f_best;
    DevBuf<double> bicg[8];
    DevBuf<double> d_partials;
    DevBuf<double> d_scalars;  // device scalar slots
    double* h_scalars = nullptr;  // pinned
    bool finalized = false;
    // ---- prolongation folded into the first post-smoothing sweep (large levels) ----
    // f_W[d+1]: per coarse cell the volume of its children on depth d; d_fold: per depth {S_f, S_c, V, sum, V}
    std::vector<DevBuf<double>> f_W;
    DevBuf<double> d_fold;
    std::vector<char> sf_valid_;
    bool fold_prolong(int d) const;
    // ---- non-diagonal metric (19-point) path, solver_full.cpp ----
    // d_ops: the ops stage by stage (first / count per stage) for the staged form, one launch per stage; d_box_ops / d_box_first:
    // the same ops sorted by box, then GhostOp::stage, for the one-launch form (k_ghost_program, small levels)
    struct FullProgram { DevBuf<GhostOp> d_ops; std::vector<int> first, count; DevBuf<GhostOp> d_box_ops; DevBuf<int> d_box_first; int max_box_ops = 0;
                         std::vector<GhostOp> h_box_ops; std::vector<int> h_box_first;   // host copy of the box-sorted list (k_box_bicgstab's tables)
                         std::vector<GhostOp> h_ops; };                                   // ... and of d_ops (refresh_diri_ops)
    void upload_program(FullProgram& P, const std::vector<std::vector<GhostOp>>& stages, int npatches);
    // small levels run a ghost program as ONE launch, one workgroup per box (Tuning::ghost_staged: always stage by stage)
    bool box_program(int d) const { return !tune_.ghost_staged && !full_march(d) && lev[d]->npatches() > 0; }
    void run_program(int d, const FullProgram& P, double* phi, double* psi, bool homogeneous, bool redirect, bool copy_all);
    bool full_ = false;
    std::vector<DevBuf<double>> f_psi;                         // per depth: the extrapolated copy of phi
    // per depth: [0] operator, [1] smoother, [2] fillExtrap alone (getFlux of the flux register), [3] ExtrapolateCFEV
    FullProgram aux_prog_[2];
    bool aux_built_[2] = {false, false};
    std::vector<std::array<FullProgram, 7>> full_prog_;   // + [4] / [5]: [0] / [1] writing psi in the boxes' frames only (marching kernels); [6]: the plain frame copy (copy_frames)
    // face fluxes of depth 0 (refluxing with a non-diagonal metric, MAC gradient); alloc_flux: the first ndir of them, on first use
    DevBuf<double> flux_own_[3];
    double* f_flux[3] = {nullptr, nullptr, nullptr};   // their view, in the form the launchers take
    void alloc_flux(int ndir);
    void build_full_programs(int d);
    void run_full_program(int d, int which, double* phi, bool homogeneous = true);
    void run_full_program_frames(int d, int which, double* phi, bool homogeneous = true);
    void copy_frames(int d, const double* src, double* dst);   // dst := src in the one-cell frame of every box
    // large 3-D levels of the non-diagonal path run the k-marching 19-point kernels (full19_march.hip)
    bool full_march(int d) const
    {
        const Level& L = *lev[d];
        return full_ && L.active[2] && L.valid_cells_global >= tune_.march_min_cells;
    }
    // ... or, where every box of the level is at least Tuning::fused19_min_box cells wide in every direction, red + black in one launch
    // plus a shell pass (full19_fused.hip).  OFF by default (negative): measured on one MI355X it loses at every box size --
    // 512^3 in one box: 9.1 ms (fused) + 0.38 ms (shell) against 2 x 2.85 ms; boxes of 128: 14.9 against 6.6 ms; of 64: 16.0
    // against 6.0 (profiles/r03_fused19.txt).  SOMAR_FUSED19_MIN_BOX = 0 forces it onto every marching level (tests, A/B).
    std::vector<char> fused19_;   // per depth, decided in finalize
    bool fused19(int d) const { return d < (int)fused19_.size() && fused19_[d] != 0; }
    std::unique_ptr<PressureSolver> coarse_;   // replicated tail of the hierarchy (agglomeration)
    int agglom_depth_ = -1;
    // (Tuning::agglom_cells: 128^3 -- below this a level costs less to replicate, ~0.2 ms of sweeps, than to exchange, ~8 x 60 us)
    Copier agglom_gather_;                      // sharded depth agglom_depth_ -> replicated depth 0 of coarse_
    Copier agglom_metric_;                      // the same for the metric (one layer of faces beyond the cells)
    DevBuf<CopyItem> d_agglom_back_;       // my boxes of the replicated correction -> sharded layout
    int n_agglom_back_ = 0;
    void build_agglomerated_tail(int depth);
    void agglom_cycle(double* corr, const double* res, bool corr_zero);
    // ---- launch-bound coarse depths replayed as HIP graphs ----
    // From the first depth with at most Tuning::graph_cells cells on, one V-cycle is ~20 microsecond-sized launches per
    // depth; the legs on either side of the bottom solve (whose loop needs host decisions) are captured once and
    // replayed.  Only where nothing but kernels is enqueued: one rank (which includes the replicated tail).
    struct CoarseGraph {
        hipGraphExec_t down = nullptr, up = nullptr;
        int d0 = -1, pre = -1, post = -1, bottom = -1;
        const double *corr = nullptr, *res = nullptr;
    };
    CoarseGraph cg_;
    static void drop_graph(CoarseGraph& g);
    // ---- a component's own operator (comp_set_op; solver_multi.cpp) ----
    // What of the solver an operator decides, for the operator that is NOT in place: sides and coefficients (every depth
    // carries the same ones), the Dirichlet values and op lists per depth, the null-space probe's verdict per depth, and the
    // captured coarse legs, whose kernel arguments embed all of that.  exchange_op swaps it with the solver's live state, so a
    // second call puts everything back; between the two the whole single-field code runs the component's operator.
    struct OpState {
        int bc[3][2] = {{0, 0}, {0, 0}, {0, 0}};
        double val[3][2] = {{0, 0}, {0, 0}, {0, 0}};
        double alpha = 0.0, beta = 1.0;   // as in force now (set_alpha_beta's scaling applied)
        bool diri = false;
        std::vector<DevBuf<GhostOp>> d_ops;
        std::vector<int> n_ops;
        std::vector<GhostOp> h_ops0;
        std::vector<char> zeroAvg;
        CoarseGraph cg;
    };
    struct CompOp {
        double alpha0 = 0.0, beta0 = 1.0;   // the pair comp_set_op received (a separate solver's create-time alpha / beta)
        OpState st;
        ~CompOp() { drop_graph(st.cg); }
    };
    double ab_scale_[2] = {1.0, 1.0};   // set_alpha_beta's last (a, b)
    int op_in_place_ = 0;               // the component whose operator is live (0: the solver's own)
    CompOp* comp_op(int comp) const { return comp > 0 && comp <= (int)comps_.size() ? comps_[comp - 1].op.get() : nullptr; }
    void exchange_op(OpState& o);
    // runs f with component comp's operator in place (fields untouched); nothing to do for a component that shares the solver's
    template <class Fn>
    void on_op(int comp, Fn f)
    {
        CompOp* o = comp_op(comp);
        if (!o) { f(); return; }
        exchange_op(o->st);
        op_in_place_ = comp;
        ScopeExit back{[&]() { exchange_op(o->st); op_in_place_ = 0; }};
        f();
    }
    bool probe_op(CompOp& o, int* depth);                  // the null-space probe at every depth with o in place: any zeroAvg?
    void ensure_face_copiers(const int bc[3][2]);          // Level::cf_faces for the operator's Dirichlet HIGH sides, every depth
    StencilParams comp_params(int comp, int d) const;      // depth d's StencilParams under component comp's operator
    LevelDev comp_level(int comp, int d) const;            // depth d's LevelDev with them as its P: what a single-field launch takes
    void comp_diri(int comp, int d, double* phi, bool homogeneous);   // the Dirichlet ghosts of comp's operator (none: nothing)
    // one N-field launch on the fields at positions i0 .. i0 + NF - 1 of the active list: with one StencilParams where their
    // operators agree (the solver's or not), with one per field where they differ.  field_ops fills O with the fields'
    // comp_params, COUNTS the launch (mc_launches_; mc_op_launches_ where they differ) and returns whether they differ.
    template <int NF>
    bool field_ops(int d, const int* comp, FieldOps<NF>& O);
    template <int NF>
    void sweep_launch(int d, const int* comp, const SweepFields<NF>& S, int mode);
    template <int NF>
    void resid_launch(int d, const int* comp, const ResidFields<NF>& R, bool restrict);
    std::vector<GhostOp> make_diri_ops(int d, const int bc[3][2], const double val[3][2], bool sides_of_solver) const;
    int graph_from_ = -1;
    bool capturing_ = false;
    bool diri_ = false;
    double bc_value_[3][2] = {{0, 0}, {0, 0}, {0, 0}};
    std::vector<DevBuf<GhostOp>> d_diri_ops_;
    std::vector<int> n_diri_ops_;
    DevBuf<GhostOp> d_extrapbc_ops_;  // order-2 extrapolation BC on the physical ghosts of depth 0 (gradient BC)
    int n_extrapbc_ops_ = 0;
    void build_diri_ops(int d);
    void apply_diri(int d, double* phi, bool homogeneous);
    // ---- position-dependent Dirichlet values (depth 0; every coarser depth and correction is homogeneous) ----
    // face_[a][s]: side (a, s) takes face_plane_[a][s] instead of bc_value_[a][s].  Every Dirichlet op of depth 0 covers the
    // ghost layer of one (local patch, side) and owns that pair's slice of d_bcface_ (face_off_[6 * patch + 2 * a + s], -1:
    // the patch does not touch the side); slices hold the plane's values in the op's loop order.
    bool face_[3][2] = {{false, false}, {false, false}, {false, false}};
    std::vector<double> face_plane_[3][2];
    std::vector<long long> face_off_;
    std::vector<double> h_bcface_;
    DevBuf<double> d_bcface_;
    std::vector<GhostOp> h_diri_ops0_;   // host copy of d_diri_ops_[0]
    void build_face_slices();
    void fill_face_values();
    long long face_slice_of(const GhostOp& op, const char* what) const;   // the op covers its (patch, side) ghost layer: its slice
    void set_diri_op(GhostOp& op) const;   // depth-0 Dirichlet op: constant or face-valued, as its side is now
    void refresh_diri_ops();
    // ---- position-dependent Neumann values (diagonal metric, depth 0, the solver's own operator) ----
    // neum_face_[a][s]: the Neumann side (a, s) is face-valued (face_ / face_plane_ / its slices of d_bcface_ serve both kinds:
    // a side is one or the other).  d_neum_ops_ has room for one op per (local patch, physical Neumann side it touches), built
    // at finalize; the ops of the face-valued sides stand first (n_neum_face_ops_ of them: all that is ever launched) and are
    // rewritten in place when a side changes kind.  d_neum_off_[6 * patch + 2 * a + s]: the slice of a face-valued Neumann
    // side on that patch, -1 otherwise (k_op_neum_face).  No plane set: n_neum_face_ops_ == 0 and nothing is launched.
    bool neum_face_[3][2] = {{false, false}, {false, false}, {false, false}};
    std::vector<GhostOp> h_neum_ops_;
    DevBuf<GhostOp> d_neum_ops_;
    int n_neum_face_ops_ = 0;
    std::vector<long long> h_neum_off_;
    DevBuf<long long> d_neum_off_;
    void build_neum_ops();     // finalize: the buffers at their final size
    void refresh_neum_ops();   // the ops and the offsets as the sides are now; one copy each into the existing buffers
    // the inhomogeneous operator of depth 0 takes face-valued Neumann sides now (not while a component's own operator is in place)
    bool neum_face_live() const { return n_neum_face_ops_ > 0 && op_in_place_ == 0; }
    // EllipticNeumBCGhostClass: the ghosts of those sides; EllipticNeumBCFluxClass: the cells next to them evaluated with the
    // planes' values as boundary fluxes, over what the operator launch left in out (mode as operator_i)
    void neum_face_ghosts(double* phi);
    void neum_face_cells(int mode, double* out, const double* phi, const double* rhs);
    int mini_depth_ = 0;  // > 0 while a mini V-cycle runs: the depth count it is limited to
    int cycle_override_ = 0;  // != 0 inside an F-cycle's inner V-cycles: the effective numMG ("m_cycle = 1" hack, MappedMultiGrid.H:603-605)
    void cycle_down(int d, double* corr, const double* res, bool corr_zero);  // pre-smoothing + restriction
    void cycle_up(int d, double* corr, const double* res);                    // prolongation + post-smoothing
    void cycle_bottom_relax(double* corr, const double* res, bool corr_zero);
    bool graph_cycle(int d, double* corr, const double* res, bool corr_zero);
    void drop_graphs();
    struct Prof { std::vector<hipEvent_t> a, b; int used = 0; };
    Prof prof_[4];   // 0: GSRB launches of depth 0, 1: its operator / residual launches, 2: ghost exchanges with other ranks (any
                     // depth), 3: the replicated tail of a sharded hierarchy (agglom_cycle)
    // ghost exchange of a level of this solver (timed in a profiled pass when other ranks take part); T: double or float
    template <class T>
    void xchg(const Level& L, T* f);
    // Sharded large levels: the messages of a sweep's one ghost exchange travel on a second stream while the tiles that read no
    // remote ghost cell are swept (the LooseGSRB idea, GSRB.cpp:122-140, without its change of the iteration: the fused sweep's
    // tiles are independent, so this is the same sweep bit for bit).  Tuning::no_overlap is the A/B switch.
    hipStream_t st_comm_ = nullptr;
    hipEvent_t ev_ready_ = nullptr, ev_done_ = nullptr;
    bool resid_overlap(const Level& L) const
    {
        return !tune_.no_overlap && !L.plan.peers.empty() && !L.rtiles.own.empty() && !capturing_ && !profiling_ && !diri_;
    }
    // exchange of f with its remote half on the second stream; run(tiles) is issued for the tiles that read no remote ghost
    // first, for the others once the messages have landed.  T: double, or float on the fp32 depths of a mixed cycle.
    template <class T, class Run>
    void overlapped(const Level& L, T* f, const SplitTileTable& table, Run run)
    {
        if (!st_comm_) {
            SOMAR_HIP(hipStreamCreateWithFlags(&st_comm_, hipStreamNonBlocking));
            SOMAR_HIP(hipEventCreateWithFlags(&ev_ready_, hipEventDisableTiming));
            SOMAR_HIP(hipEventCreateWithFlags(&ev_done_, hipEventDisableTiming));
        }
        SOMAR_HIP(hipEventRecord(ev_ready_, st_));
        SOMAR_HIP(hipStreamWaitEvent(st_comm_, ev_ready_, 0));
        L.exchange_local(f, st_);
        run(table.own.span());
        L.exchange_remote(f, st_comm_);   // (a host-staged transport may block here: the tiles above are already queued)
        SOMAR_HIP(hipEventRecord(ev_done_, st_comm_));
        SOMAR_HIP(hipStreamWaitEvent(st_, ev_done_, 0));
        run(table.rem.span());
        ++counters[0];
    }
    bool fused_overlap(const Level& L) const
    {
        return !tune_.no_overlap && !L.plan.peers.empty() && !L.ftiles.own.empty() && !capturing_ && !profiling_;
    }
    bool profiling_ = false;
    void prof_begin(int k);
    void prof_end(int k);
    // times what is enqueued during its life into slot k: only in a profiled pass, on depth 0 (and where `on` holds).  An error
    // thrown inside the scope passes through it: the end event is then not recorded, as with a begin / end pair it skipped.
    struct ProfScope {
        PressureSolver* s;
        int k, unwinding;
        ProfScope(PressureSolver& ps, int d, int k_, bool on = true)
            : s(ps.profiling_ && d == 0 && on ? &ps : nullptr), k(k_), unwinding(std::uncaught_exceptions())
        {
            if (s) s->prof_begin(k);
        }
        ~ProfScope() noexcept(false) { if (s && std::uncaught_exceptions() == unwinding) s->prof_end(k); }
        ProfScope(const ProfScope&) = delete;
    };
};

}  // namespace somar
