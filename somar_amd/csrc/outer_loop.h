// somar_amd/csrc/outer_loop.h -- the outer iteration of a solve, host only (plain C++, no HIP: a stand-alone host program can
// include it, tests/test_outer_loop.py does).
//   MappedAMRMultiGrid<T>::solveNoInitResid  calculus/AMRElliptic/MappedAMRMultiGrid.H:979-1183
// OuterLoop holds that loop's state and decisions -- the four go* tests, the best-phi bookkeeping, the two "blew up" verdicts
// and the exitStatus bits -- and nothing else: no fields, no launches, no levels or components.  Its callers own those and
// feed it one residual norm per cycle: PressureSolver::solve, solve_multi (one OuterLoop per component) and
// AMRSolver::solve_impl.  Also here: the stopping criteria and statistics of a solve, and the TGA integrator's coefficients.
#pragma once
#include <cmath>
#include <vector>

namespace somar {

// The five criteria of the loop: the head of SolverParams (solver.h), where the rest of a solver's parameters live.
// AMRPressureSolver::setAMRMGParameters (projection/AMRPressureSolver.H:53-77); defaults utils/ProblemContext.cpp:1147-1236
struct StopCriteria {
    int imin = 5, imax = 20;
    double eps = 1e-6, hang = 1e-15, normThresh = 1e-30;
};

struct SolveStats {
    int iters = 0;
    int exitStatus = 0;         // !goRedu + 2*!goIter + 4*!goHang + 8*!goNorm (MappedAMRMultiGrid.H:1148)
    int status = 0;             // 0 ok, 1 "kaboom", 2 "solver blew up"
    double initial_rnorm = 0, final_rnorm = 0;
    std::vector<double> history;  // max-norm residual after each V-cycle (history[0] = initial)
    int bottom_iters_last = 0, bottom_exit_last = 0;
};

// One solve:  start(r0);  while (go()) { begin_cycle(); <cycle, phi += correction, residual>; if (end_cycle(r)) <bestPhi = phi>; }
//             if (finish(..., stats)) <phi = bestPhi>;
struct OuterLoop {
    double initial = 0, rnorm = 0, norm_last = 0, best = 0;
    bool useBest = false, converged = false, goNorm = false, goRedu = false, goIter = false, goHang = false;
    int iter = 0;
    std::vector<double> history;

    void start(double r0, const StopCriteria& prm)
    {
        *this = OuterLoop();
        initial = rnorm = best = r0;
        norm_last = 2 * r0;
        history.push_back(r0);
        tests(prm);
    }
    bool go() const { return goIter && goRedu && goHang && goNorm; }
    void begin_cycle() { norm_last = rnorm; }
    // r: the residual norm after the cycle.  True: it is the best so far, and the caller copies phi to bestPhi
    bool end_cycle(double r, const StopCriteria& prm)
    {
        rnorm = r;
        ++iter;
        history.push_back(r);
        if (r <= best) {
            best = r;
            useBest = false;
            converged = true;
        } else {
            useBest = true;
        }
        tests(prm);
        return !useBest;
    }
    // The verdicts and counts into s (the bottom solver's counts are the caller's).  report_blowup: status 2 is reported
    // (AMRLepticSolver only prints there, AMRLepticSolver.cpp:384-388).  True: the caller copies bestPhi back to phi
    bool finish(const StopCriteria& prm, bool report_blowup, SolveStats& s)
    {
        if (useBest) rnorm = best;
        s.status = 0;
        if (rnorm > 10. * initial && rnorm > 10. * prm.eps) s.status = 1;                                          // "kaboom" :1134
        else if (report_blowup && !converged && rnorm >= initial && rnorm >= prm.eps) s.status = 2;                // :1141
        s.exitStatus = int(!goRedu) + int(!goIter) * 2 + int(!goHang) * 4 + int(!goNorm) * 8;
        s.iters = iter;
        s.initial_rnorm = initial;
        s.final_rnorm = rnorm;
        s.history = history;
        return useBest;
    }

private:
    void tests(const StopCriteria& prm)
    {
        goNorm = rnorm > prm.normThresh;
        goRedu = rnorm > prm.eps * initial;
        goIter = iter < prm.imax;
        goHang = iter < prm.imin || rnorm < (1 - prm.hang) * norm_last;
    }
};

// MappedLevelTGA's constructor, AMRParabolic/MappedLevelTGA.cpp:30-56
struct TGACoefficients { double mu1, mu2, mu3, mu4, r1; };
inline TGACoefficients tga_coefficients()
{
    const double tgaEpsilon = 1.e-12;
    const double a = 2.0 - std::sqrt(2.0) - tgaEpsilon;
    const double discr = std::sqrt(a * a - 4.0 * a + 2.0);
    return {(a - discr) / 2.0, (a + discr) / 2.0, 1.0 - a, 0.5 - a, (2.0 * a - 1.0) / (a + discr)};
}

}  // namespace somar
