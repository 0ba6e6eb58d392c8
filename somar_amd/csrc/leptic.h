// somar_amd/csrc/leptic.h -- the leptic level solver: the MI355X counterpart of
//   LevelLepticSolver::define / solve     calculus/LepticSolver/LevelLepticSolver.cpp:147-437, 646-956
//   LepticOperator (what it asks of the level operator)   calculus/LepticSolver/LepticOperator.H:33-45
//
// Design (not a port): the level's boxes are vertically complete columns -- the layout the reference re-creates
// with LepticBoxUtils::createVerticalSolverGrids before every solve path; here the caller hands it over once, a
// 288 GB HBM holds such columns whole -- so the reference's four re-layout Copiers (orig <-> vertical, flat <->
// horizontal) disappear.  Three PressureSolvers share one stream and the layout: the level's own operator (for
// the initial residual), the J-scaled operator (J^{-1} := 1, alpha 0, beta 1) with the full 3-D multigrid used
// as fallback, and the flat 2-D multigrid on the vertically averaged metric.  Everything in between is column
// kernels (leptic_kernels.hip); the host sequences launches and reads back one norm per order.
//
// Scope: diagonal or non-diagonal metric; coarse-fine boundaries on the lateral sides of the columns (the level of an AMR
// hierarchy refined by (r, r, 1): attach()); columns that are ALL Neumann-Neumann (horizontal solves), ALL ended by a
// Dirichlet wall / a coarse-fine interface (LepticLapackVerticalSolver + dptsv, no horizontal solves), or a MIX of the two on
// one level (a fine level refined in the vertical as well: m_flatDI / m_flatDIComplement, LevelLepticSolver.cpp:318-333 --
// the flat problem lives on the spanning boxes only, the footprint of the others is its coarse-fine boundary; diagonal
// metric and one rank only, anything else raises); homogeneous-Neumann lateral boundaries,
// non-periodic directions (the reference leaves the averaged gradient on a periodic horizontal boundary face
// unset, LevelLepticSolver.cpp:997-1001, and refuses a periodic vertical, :1315).
#pragma once
#include <memory>
#include <vector>

#include "solver.h"

namespace somar {

struct LepticParams {
    // setDefaultParameters, LevelLepticSolver.cpp:461-508
    int maxOrder = 4;
    double hang = 1e-15;
    int normType = 0;
    double horizRhsTol = 1e-14;
    double domainHeight = 0.0;  // LevelGeometry::getDomainLength(SpaceDim-1); 0: dz * Nz
    SolverParams horiz, full;
    LepticParams();
};

struct LepticStats {
    int exitStatus = -1;  // LevelLepticSolver::ExitStatus: 0 converge, 1 iter, 2 hang, 3 diverge, 4 kaboom
    int orders = 0;
    int horizSolves = 0;
    int usedFullSolver = 0;
    std::vector<double> resNorms;  // [0] initial |J res|, [k] after order k-1
    SolveStats horizStats, fullStats;
};

class LepticSolver {
public:
    // shared: run on the caller's stream (an AMR hierarchy's) instead of an own one
    // tune: handed to every internal level solver (an attached solver's hierarchy passes its own)
    LepticSolver(Comm* comm, hipStream_t shared, const Tuning& tune);
    ~LepticSolver();
    void define(const IBox& domain, const bool periodic[3], const double dx[3], const int bc_type[3][2],
                const std::vector<IBox>& boxes, const std::vector<int>& owner, double alpha, double beta,
                const SolverParams& prmOrig, const LepticParams& lp, const double* dxCrse = nullptr);
    // LevelLepticSolver::define(opPtr, homogeneous) on the FINALIZED operator of an AMR level (AMRLepticSolver::init,
    // AMRLepticSolver.cpp:185-195): layout, spacing, boundary types and dxCrse are the operator's; not owned
    void attach(PressureSolver* orig, const LepticParams& lp);
    // the level's own operator: metric, phi and rhs go through it (somar_solver_* entry points)
    PressureSolver& orig() { return *orig_; }
    PressureSolver& vert() { return *vert_; }
    PressureSolver& horiz() { return *horiz_; }
    // null: no column is Neumann-Neumann, there is no flat problem.  On a mixed level (attach() only: it needs a coarser level)
    // its patches are the spanning boxes only
    PressureSolver* horiz_ptr() { return horiz_.get(); }
    void finalize();  // after the metric of orig() is set: finalizes all three solvers
    // after a metric refresh of orig(): the J-scaled operator's copy, the flat problem's vertical averages, then both solvers
    void refresh_metric();
    // LevelLepticSolver::solve(phi, rhs) on orig()'s resident phi / rhs: phi += leptic correction
    void solve(bool homogeneous, LepticStats& S);
    // the same on any two fields of the level's layout: phi += leptic correction for rhs - L[phi] (homogeneous CF / BC values)
    void solve_fields(double* phi, const double* rhs, LepticStats& S, bool homogeneous = true);
    bool do_horiz_solve() const { return doHorizSolve_; }
    void sync() { SOMAR_HIP(hipStreamSynchronize(st_)); }
    LepticParams prm;

private:
    void set_zero_avg(double* hphi);
    void solve_fields_no_horiz(double* phi, const double* rhs, LepticStats& S, bool homogeneous);
    const Tuning tune_;
    Comm* comm_;
    hipStream_t st_ = nullptr;
    void define_inner(const IBox& domain, const bool periodic[3], const double dx[3], const int bc_type[3][2],
                      const std::vector<IBox>& boxes, const std::vector<int>& owner, const double* dxCrse, double probeEps);
    PressureSolver* orig_ = nullptr;
    std::unique_ptr<PressureSolver> own_orig_, vert_, horiz_;
    bool own_stream_ = true, hasCF_ = false;
    double dx_[3] = {1, 1, 1};
    double H_ = 1.0;
    bool horizRemoveAvg_ = false;
    long long horizCells_ = 0;
    bool finalized_ = false;
    bool full_ = false;   // non-diagonal metric (decided when orig()'s metric has been set)
    // 3-D work fields (vertical layout) and flat ones (horizontal layout)
    DevBuf<double> f_total, f_rhsA, f_rhsB, f_gam;
    DevBuf<double> h_excess, h_bcLo, h_bcHi, h_gx, h_gy;
    DevBuf<double> d_avg;  // (sum, count) for setZeroAvg
    // columns ending at Dirichlet walls / coarse-fine interfaces (gatherVerticalBCTypes): per box (lo, hi) 0 Neum, 1 Diri, 2 CF
    std::vector<int> vbc_;
    bool doHorizSolve_ = true;
    double dzCrse_ = 0.0;
    DevBuf<double> f_efac;
    DevBuf<int> d_vbc, d_bad;
    void upload_vbc();
    void check_bad();   // raises if a dptsv pivot was not positive
    // a level that mixes Neumann-Neumann (spanning) columns with the other kind: the flat problem holds the spanning boxes only
    // (the reference's m_flatDI), so the column kernels that touch flat fields run on the spanning boxes' tiles and find the
    // flat patch of vertical patch p at d_flatOf[p] (complement patches: unused, zeroed)
    bool mixed_ = false;
    std::vector<int> flatDI_;          // global box indices of the spanning boxes, ascending
    TileTable stiles_;                 // the whole-column tiles of the spanning patches
    DevBuf<PatchDesc> d_flatOf;
    // tiles / flat view for the kernels that pair a column with its flat cell: the level's own where nothing is mixed
    TileSpan span_tiles() const { return mixed_ ? stiles_.span() : vert_->level(0).ctiles.span(); }
    LevelDev flat_dev() const
    {
        LevelDev H = horiz_->level(0).dev;
        if (mixed_) H.patches = d_flatOf;
        return H;
    }
};

void launch_lep_avg_metric(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H);
// non-diagonal metric: the horizontal block averaged, MAPPEDMACGRAD with cross terms, LEPTICVERTHORIZGRAD
void launch_lep_avg_metric_full(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H);
void launch_lep_hgrad_full(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H,
                           const double* phi, double* gx, double* gy);
void launch_lep_vhgrad(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H,
                       const double* phi, double* bcLo, double* bcHi, double scale);
void launch_lep_excess(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H,
                       const double* rhs, const double* bcLo, const double* bcHi, double* excess, double dzScale);
void launch_lep_vsolve(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H,
                       double* phi, double* rhs, double* gam, const double* bcLo, const double* bcHi, double dz);
void launch_lep_vsolve_lapack(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, double* phi,
                              const double* rhs, double* dfac, double* efac, const int* vbc, double dz, double dzCrse, int* bad);
// a mixed level: per tile the Neumann-Neumann sweep or the dptsv restatement, by vbc; flatOf[patch]: the flat patch of a
// spanning box
void launch_lep_vsolve_mixed(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const PatchDesc* flatOf,
                             double* phi, double* rhs, double* dfac, double* efac, const double* bcLo, const double* bcHi,
                             const int* vbc, double dz, double dzCrse, int* bad);
void launch_lep_hgrad(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H,
                      const double* phi, double* gx, double* gy);
void launch_lep_hrhs(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H,
                     const double* gx, const double* gy, const double* excess, double* hrhs, double sx, double sy,
                     double negInvH, bool useExcess);
void launch_lep_extrude(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, const LevelDev& H,
                        double* phi, const double* flat);
void launch_lep_divide(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, double* y, const double* x,
                       const double* b);
void launch_lep_axpy(hipStream_t st, TileSpan ct, int tj, const LevelDev& V, double* y, const double* x,
                     double a);

}  // namespace somar
