// somar_amd/csrc/leptic.cpp -- host side of the leptic level solver (see leptic.h).
#include "leptic.h"

#include <cmath>
#include <cstring>

namespace somar {

LepticParams::LepticParams()
{
    // horizontal 2-D multigrid + its bottom solver (setHorizMGParameters / setHorizBottomParameters defaults)
    horiz.imin = 5; horiz.imax = 20;
    horiz.num_smooth_down = horiz.num_smooth_up = horiz.num_smooth_bottom = 4;
    horiz.num_smooth_precond = 2;
    horiz.relaxMode = RELAX_LEVEL_GSRB; horiz.precondMode = PRECOND_DIAG_RELAX;
    horiz.numMG = 1; horiz.maxDepth = -1;
    horiz.eps = 1e-12; horiz.hang = 1e-15; horiz.normThresh = 1e-30;
    horiz.bottom_imax = 80; horiz.bottom_eps = 1e-12; horiz.bottom_numRestarts = 5; horiz.bottom_hang = 1e-15;
    horiz.bottom_normType = 0;
    horiz.spaceDim = 2;
    // full 3-D multigrid (setFullMGParameters); its bottom solver only gets imax / restarts / normType
    // (LevelLepticSolver.cpp:270-276), the rest are Chombo's BiCGStabSolver defaults
    full.imin = 5; full.imax = 20;
    full.num_smooth_down = full.num_smooth_up = full.num_smooth_bottom = 4;
    full.num_smooth_precond = 4;
    full.relaxMode = RELAX_LINE_GSRB; full.precondMode = PRECOND_DIAG_LINE_RELAX;
    full.numMG = 1; full.maxDepth = -1;
    full.eps = 1e-6; full.hang = 1e-15; full.normThresh = 1e-30;
    full.bottom_imax = 80; full.bottom_numRestarts = 5; full.bottom_eps = 1e-6; full.bottom_hang = 1e-8;
    full.bottom_normType = 0;
    full.spaceDim = 3;
}

LepticSolver::LepticSolver(Comm* comm, hipStream_t shared, const Tuning& tune) : tune_(tune), comm_(comm)
{
    if (shared) { st_ = shared; own_stream_ = false; }
    else SOMAR_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
}

LepticSolver::~LepticSolver()
{
    horiz_.reset();
    vert_.reset();
    own_orig_.reset();
    if (st_ && own_stream_) hipStreamDestroy(st_);
}

void LepticSolver::define(const IBox& domain, const bool periodic[3], const double dx[3], const int bc_type[3][2],
                          const std::vector<IBox>& boxes, const std::vector<int>& owner, double alpha, double beta,
                          const SolverParams& prmOrig, const LepticParams& lp, const double* dxCrse)
{
    SOMAR_CHECK(!orig_, "leptic solver already defined");
    prm = lp;
    SOMAR_CHECK(prmOrig.spaceDim == 3, "the leptic solver is implemented for space_dim 3");
    own_orig_.reset(new PressureSolver(comm_, st_, tune_));
    orig_ = own_orig_.get();
    orig_->define(domain, periodic, dx, bc_type, boxes, owner, alpha, beta, prmOrig, dxCrse);
    define_inner(domain, periodic, dx, bc_type, boxes, owner, dxCrse, prmOrig.eps);
}

void LepticSolver::attach(PressureSolver* orig, const LepticParams& lp)
{
    SOMAR_CHECK(!orig_, "leptic solver already defined");
    SOMAR_CHECK(orig && orig->prm.spaceDim == 3, "the leptic solver is implemented for space_dim 3");
    prm = lp;
    orig_ = orig;
    const Level& L = orig->level(0);
    define_inner(L.domain, L.periodic, L.dx, L.bc_type, L.boxes, L.owner, orig->dx_crse(), orig->prm.eps);
    finalize();
}

void LepticSolver::define_inner(const IBox& domain, const bool periodic[3], const double dx[3], const int bc_type[3][2],
                                const std::vector<IBox>& boxes, const std::vector<int>& owner, const double* dxCrse,
                                double probeEps)
{
    SOMAR_CHECK(prm.normType == 0, "the leptic solver offers the max norm (norm_type 0, the reference's default)");
    SOMAR_CHECK(prm.maxOrder >= 0, "max_order must be >= 0");
    SOMAR_CHECK(domain.size(2) >= 2, "the vertical line solver wants at least two cells per column");
    for (int d = 0; d < 3; ++d)
        SOMAR_CHECK(!periodic[d], "the leptic solver does not support periodic directions (neither does the reference: "
                                  "LevelLepticSolver.cpp:997-1001, 1315)");
    hasCF_ = dxCrse != nullptr;
    // gatherVerticalBCTypes (LevelLepticSolver.cpp:1523-1640): an end of a column is a physical boundary (Neumann or Dirichlet)
    // or, inside the domain, a coarse-fine interface over the whole box end (anything else: "Vertical grids are ill-formed")
    vbc_.assign(2 * boxes.size(), 0);
    bool anyNN = false, allNN = true;
    flatDI_.clear();
    for (size_t bi = 0; bi < boxes.size(); ++bi) {
        const IBox& b = boxes[bi];
        SOMAR_CHECK(b.size(2) >= 2, "the vertical line solver wants at least two cells per column");
        for (int s = 0; s < 2; ++s) {
            const bool atDom = s == 0 ? b.lo[2] == domain.lo[2] : b.hi[2] == domain.hi[2];
            int t;
            if (atDom) {
                t = bc_type[2][s] == 0 ? 0 : 1;
            } else {
                SOMAR_CHECK(hasCF_, "Vertical grids are ill-formed: a column ends inside the domain of a level without a coarser one");
                IBox adj = b;
                adj.lo[2] = adj.hi[2] = s == 0 ? b.lo[2] - 1 : b.hi[2] + 1;
                for (const IBox& o : boxes)
                    SOMAR_CHECK((o & adj).empty(), "Vertical grids are ill-formed: a box is split in the vertical");
                t = 2;
            }
            vbc_[2 * bi + s] = t;
        }
        const bool nn = vbc_[2 * bi] == 0 && vbc_[2 * bi + 1] == 0;
        anyNN = anyNN || nn;
        allNN = allNN && nn;
        if (nn) flatDI_.push_back((int)bi);
    }
    doHorizSolve_ = anyNN;
    // m_flatDI / m_flatDIComplement (:318-333): the Neumann-Neumann boxes span the domain and carry the flat problem, the others
    // (the complement) take no part in it.  A Neumann-Neumann column needs Neumann walls, and between Neumann walls every
    // spanning column is Neumann-Neumann: the two notions cannot come apart.
    mixed_ = anyNN && !allNN;
    SOMAR_CHECK(!mixed_ || !comm_ || comm_->size == 1,
                "the leptic solver takes a level that mixes Neumann-Neumann columns with Dirichlet / coarse-fine ended ones "
                "on one rank only: the flat problem's patch map is not built per rank");
    dzCrse_ = dxCrse ? dxCrse[2] : 0.0;
    for (int d = 0; d < 3; ++d) dx_[d] = dx[d];
    H_ = prm.domainHeight > 0.0 ? prm.domainHeight : dx[2] * domain.size(2);
    // the J-scaled operator and the full multigrid on it (alpha 0, beta 1), with the level's CFRegion and dxCrse
    //                                                                                   LevelLepticSolver.cpp:214-300
    SolverParams pf = prm.full;
    pf.spaceDim = 3;
    vert_.reset(new PressureSolver(comm_, st_, tune_));
    vert_->define(domain, periodic, dx, bc_type, boxes, owner, 0.0, 1.0, pf, dxCrse);
    vert_->probe_eps = probeEps;
    if (!doHorizSolve_) return;   // no Neumann-Neumann column: no excess, no flat problem (:304)
    // flat grids: the Neumann-Neumann boxes, one cell thick at the domain's lowest vertical index :304-432
    IBox flatDom = domain;
    flatDom.hi[2] = flatDom.lo[2];
    // createHorizontalSolverGrids (LepticBoxUtils.cpp:100-117): the spanning boxes only.  On a mixed level the footprint of
    // the complement is then a coarse-fine boundary of the flat problem, and horizRemoveAvg_ comes out false
    std::vector<IBox> flat;
    std::vector<int> flatOwner;
    horizCells_ = 0;
    for (int bi : flatDI_) {
        IBox b = boxes[bi];
        b.lo[2] = b.hi[2] = domain.lo[2];
        horizCells_ += b.numPts();
        flat.push_back(b);
        flatOwner.push_back(owner[bi]);
    }
    horizRemoveAvg_ = horizCells_ == flatDom.numPts();
    SolverParams ph = prm.horiz;
    ph.spaceDim = 2;
    horiz_.reset(new PressureSolver(comm_, st_, tune_));
    horiz_->define(flatDom, periodic, dx, bc_type, flat, flatOwner, 0.0, 1.0, ph, dxCrse);   // forceDxCrse(m_dxCrse), :381
    horiz_->probe_eps = probeEps;
}

void LepticSolver::finalize()
{
    SOMAR_CHECK(orig_ && !finalized_, "finalize before define / twice");
    full_ = orig_->is_full();
    // levelVertHorizGradient hands the complement's Neumann ends boundary data too, non-zero only with cross terms
    SOMAR_CHECK(!(mixed_ && full_), "the leptic solver takes a level that mixes Neumann-Neumann columns with Dirichlet / "
                                    "coarse-fine ended ones for a diagonal metric only: this level has a non-diagonal metric");
    if (full_) {
        // the J-scaled operator and the flat problem inherit LevelGeometry::isDiagonal() == false: 19-point / 9-point kernels
        vert_->make_full();
        if (horiz_) horiz_->make_full();
    }
    if (own_orig_) orig_->finalize();
    Level& O = orig_->level(0);
    Level& V = vert_->level(0);
    SOMAR_CHECK(O.field_elems == V.field_elems && O.npatches() == V.npatches(), "internal: layouts differ");
    if (!doHorizSolve_) {
        // columns ending at Dirichlet walls / coarse-fine interfaces: the J-scaled operator, two factor fields, the end codes
        if (full_) {
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) launch_copy(st_, V.dev.jgf[a][b], O.dev.jgf[a][b], V.field_elems);
        } else {
            for (int d = 0; d < 3; ++d) launch_copy(st_, V.dev.jg[d], O.dev.jg[d], V.field_elems);
        }
        launch_set(st_, V.dev.jinv, V.field_elems, 1.0);
        sync();
        vert_->finalize();
        f_total = V.alloc_field();
        f_rhsA = V.alloc_field();
        f_rhsB = V.alloc_field();
        f_gam = V.alloc_field();
        f_efac = V.alloc_field();
        upload_vbc();
        SOMAR_HIP(hipDeviceSynchronize());
        finalized_ = true;
        return;
    }
    Level& F = horiz_->level(0);
    if (mixed_) {
        // the spanning patches' column tiles, and for every vertical patch its flat patch (one rank: patch == box index)
        std::vector<int> flatPatch(V.boxes.size(), -1);
        for (size_t h = 0; h < flatDI_.size(); ++h) flatPatch[flatDI_[h]] = (int)h;
        SOMAR_CHECK(F.npatches() == (int)flatDI_.size(), "internal: layouts differ");
        std::vector<PatchDesc> flatOf(V.npatches());
        std::memset(flatOf.data(), 0, flatOf.size() * sizeof(PatchDesc));
        for (int pi = 0; pi < V.npatches(); ++pi) {
            const int h = flatPatch[V.local[pi]];
            if (h < 0) continue;
            const PatchDesc &vp = V.hpatches[pi], &fp = F.hpatches[h];
            SOMAR_CHECK(vp.lo[0] == fp.lo[0] && vp.lo[1] == fp.lo[1] && vp.n[0] == fp.n[0] && vp.n[1] == fp.n[1],
                        "internal: a flat patch is not the footprint of its spanning patch");
            flatOf[pi] = fp;
        }
        std::vector<Tile> st;
        for (const Tile& t : V.ctiles.host())
            if (flatPatch[V.local[t.patch]] >= 0) st.push_back(t);
        stiles_.assign(std::move(st), 0);
        d_flatOf = DevBuf<PatchDesc>::from(flatOf);
    } else {
        SOMAR_CHECK(V.npatches() == F.npatches(), "internal: layouts differ");
    }
    // metric of the J-scaled operator: the level's J g^{ab}, J^{-1} := 1
    if (full_) {
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) launch_copy(st_, V.dev.jgf[a][b], O.dev.jgf[a][b], V.field_elems);
    } else {
        for (int d = 0; d < 3; ++d) launch_copy(st_, V.dev.jg[d], O.dev.jg[d], V.field_elems);
    }
    launch_set(st_, V.dev.jinv, V.field_elems, 1.0);
    // metric of the flat problem: vertical average of the horizontal components, J^{-1} := 1
    if (full_) launch_lep_avg_metric_full(st_, V.ctiles.span(), V.ctile_j, V.dev, F.dev);
    else launch_lep_avg_metric(st_, span_tiles(), V.ctile_j, V.dev, flat_dev());
    launch_set(st_, F.dev.jinv, F.field_elems, 1.0);
    sync();
    vert_->finalize();
    horiz_->finalize();
    f_total = V.alloc_field();
    f_rhsA = V.alloc_field();
    f_rhsB = V.alloc_field();
    f_gam = V.alloc_field();
    h_excess = F.alloc_field();
    h_bcLo = F.alloc_field();
    h_bcHi = F.alloc_field();
    h_gx = F.alloc_field();
    h_gy = F.alloc_field();
    if (mixed_) {   // the complement's columns: dptsv factors and end codes
        f_efac = V.alloc_field();
        upload_vbc();
    }
    d_avg = DevBuf<double>(2);
    SOMAR_HIP(hipDeviceSynchronize());
    finalized_ = true;
}

// per local patch the (lo, hi) end codes of its columns, and the counter of non-positive dptsv pivots
void LepticSolver::upload_vbc()
{
    Level& V = vert_->level(0);
    std::vector<int> local(2 * (size_t)std::max(1, V.npatches()), 0);
    for (int pi = 0; pi < V.npatches(); ++pi)
        for (int s2 = 0; s2 < 2; ++s2) local[2 * pi + s2] = vbc_[2 * V.local[pi] + s2];
    d_vbc = DevBuf<int>::from(local);
    d_bad = DevBuf<int>::zeros(1);
}

void LepticSolver::refresh_metric()
{
    SOMAR_CHECK(finalized_, "leptic metric refresh before finalize");
    Level& O = orig_->level(0);
    Level& V = vert_->level(0);
    if (full_) {
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) launch_copy(st_, V.dev.jgf[a][b], O.dev.jgf[a][b], V.field_elems);
    } else {
        for (int d = 0; d < 3; ++d) launch_copy(st_, V.dev.jg[d], O.dev.jg[d], V.field_elems);
    }
    launch_set(st_, V.dev.jinv, V.field_elems, 1.0);
    if (doHorizSolve_) {
        Level& F = horiz_->level(0);
        if (full_) launch_lep_avg_metric_full(st_, V.ctiles.span(), V.ctile_j, V.dev, F.dev);
        else launch_lep_avg_metric(st_, span_tiles(), V.ctile_j, V.dev, flat_dev());
        launch_set(st_, F.dev.jinv, F.field_elems, 1.0);
    }
    sync();
    vert_->refresh_metric();
    if (doHorizSolve_) horiz_->refresh_metric();
}

// setZeroAvg, LevelLepticSolver.cpp:1668-1710: plain (unweighted) mean over the valid cells, removed from the whole FAB
void LepticSolver::set_zero_avg(double* hphi)
{
    Level& F = horiz_->level(0);
    const double sum = horiz_->dot(0, hphi, F.dev.jinv);  // J^{-1} == 1: the dot product is the sum, in the same order
    const double pair[2] = {sum, (double)horizCells_};
    SOMAR_HIP(hipMemcpyAsync(d_avg, pair, sizeof(pair), hipMemcpyHostToDevice, st_));
    SOMAR_HIP(hipStreamSynchronize(st_));
    launch_sub_mean(st_, hphi, F.field_elems, d_avg);
}

void LepticSolver::solve(bool homogeneous, LepticStats& S)
{
    orig_->check_idle("leptic solve");
    // Neumann walls are homogeneous either way; a Dirichlet wall's values enter the first residual unless homogeneous
    solve_fields(orig_->phi(), orig_->rhs(), S, homogeneous);
}

// no column is Neumann-Neumann (gatherVerticalBCTypes, :1615-1627): m_doHorizSolve is false, every order is one
// LepticLapackVerticalSolver pass, the residual test and the full-multigrid fallback (LevelLepticSolver.cpp:762-933)
void LepticSolver::solve_fields_no_horiz(double* a_phi, const double* a_rhs, LepticStats& S, bool homogeneous)
{
    PressureSolver &Os = *orig_, &Vs = *vert_;
    Level& V = Vs.level(0);
    const TileSpan ct = V.ctiles.span();
    const int tj = V.ctile_j;
    const long long n = V.field_elems;
    const int maxOrder = prm.maxOrder;
    double* vertPhi = Vs.phi();
    double* rhsP = f_rhsA;
    double* tmpP = f_rhsB;
    S = LepticStats();
    Os.residual(0, rhsP, a_phi, a_rhs, homogeneous);
    launch_lep_divide(st_, ct, tj, V.dev, rhsP, rhsP, Os.level(0).dev.jinv);
    double resNorm = Vs.norm(0, rhsP, prm.normType);
    S.resNorms.push_back(resNorm);
    launch_set(st_, f_total, n, 0.0);
    int exitStatus = -1;
    for (int order = 0; order <= maxOrder; ++order) {
        S.orders = order + 1;
        // a Neumann end rolls in the boundary data, which stay zero without horizontal solves: rhs + 0
        launch_lep_vsolve_lapack(st_, ct, tj, V.dev, vertPhi, rhsP, f_gam, f_efac, d_vbc, dx_[2], dzCrse_, d_bad);
        Vs.residual(0, tmpP, vertPhi, rhsP);
        resNorm = Vs.norm(0, tmpP, prm.normType);
        double relResNorm = resNorm / S.resNorms[0];
        const double prevRelResNorm = S.resNorms.back() / S.resNorms[0];
        double redu = prevRelResNorm - relResNorm;
        if (redu <= prm.hang && order == maxOrder) {
            launch_copy(st_, Vs.rhs(), rhsP, n);
            Vs.solve(true, true, S.fullStats);
            Vs.residual(0, tmpP, vertPhi, rhsP);
            resNorm = Vs.norm(0, tmpP, prm.normType);
            relResNorm = resNorm / S.resNorms[0];
            S.usedFullSolver = 1;
        }
        std::swap(rhsP, tmpP);
        S.resNorms.push_back(resNorm);
        redu = prevRelResNorm - relResNorm;
        if (redu > prm.hang || order < maxOrder) {
            launch_lep_axpy(st_, ct, tj, V.dev, f_total, vertPhi, 1.0);
            exitStatus = (order < maxOrder - 1) ? 0 : 1;
        } else if (-redu > prm.hang) {
            exitStatus = (order == 0) ? 4 : 3;
            break;
        } else {
            exitStatus = (order == 0) ? 4 : 2;
            break;
        }
    }
    if (exitStatus != 4) launch_lep_axpy(st_, ct, tj, V.dev, a_phi, f_total, 1.0);
    S.exitStatus = exitStatus;
    check_bad();
}

void LepticSolver::check_bad()
{
    int bad = 0;
    SOMAR_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st_));
    sync();
    if (bad) {
        SOMAR_HIP(hipMemset(d_bad, 0, sizeof(int)));
        SOMAR_CHECK(false, "LepticLapackVerticalSolver: dptsv met a non-positive pivot (INFO != 0)");
    }
}

void LepticSolver::solve_fields(double* a_phi, const double* a_rhs, LepticStats& S, bool homogeneous)
{
    SOMAR_CHECK(finalized_, "solve before finalize");
    if (!doHorizSolve_) {
        solve_fields_no_horiz(a_phi, a_rhs, S, homogeneous);
        return;
    }
    PressureSolver &Os = *orig_, &Vs = *vert_, &Hs = *horiz_;
    Level& V = Vs.level(0);
    Level& F = Hs.level(0);
    const TileSpan ct = V.ctiles.span();
    const int tj = V.ctile_j;
    // the kernels that pair a column with its flat cell run on the spanning boxes: every box, unless the level is mixed
    const TileSpan sct = span_tiles();
    const LevelDev Fd = flat_dev();
    const long long n = V.field_elems, hn = F.field_elems;
    const int maxOrder = prm.maxOrder;
    const double dz = dx_[2];
    double* vertPhi = Vs.phi();  // the full multigrid solves in place
    double* rhsP = f_rhsA;
    double* tmpP = f_rhsB;
    bool useExcess = true, useHorizPhi = true;  // m_doHorizSolve: Neumann at both vertical ends
    S = LepticStats();

    // J * residual of the level's own operator                                                   :697-715
    Os.residual(0, rhsP, a_phi, a_rhs, homogeneous);
    launch_lep_divide(st_, ct, tj, V.dev, rhsP, rhsP, Os.level(0).dev.jinv);
    double resNorm = Vs.norm(0, rhsP, prm.normType);
    S.resNorms.push_back(resNorm);
    launch_set(st_, f_total, n, 0.0);
    launch_set(st_, h_bcLo, hn, 0.0);
    launch_set(st_, h_bcHi, hn, 0.0);
    int exitStatus = -1;

    for (int order = 0; order <= maxOrder; ++order) {
        S.orders = order + 1;
        if (order >= 1) {  // levelVertHorizGradient: zero for a diagonal metric                   :1107-1176
            launch_set(st_, h_bcLo, hn, 0.0);
            launch_set(st_, h_bcHi, hn, 0.0);
            if (full_) {
                Vs.run_aux_program(1, vertPhi);   // ExtrapolateFaceAndCopy in z, lo then hi, order 2, in place
                launch_lep_vhgrad(st_, ct, tj, V.dev, Fd, vertPhi, h_bcLo, h_bcHi, -1.0);
            }
        }
        if (order >= 1 && useExcess) launch_incr(st_, h_bcHi, h_excess, 1.0, hn);
        if (useExcess) {
            launch_lep_excess(st_, sct, tj, V.dev, Fd, rhsP, h_bcLo, h_bcHi, h_excess, -1.0 * dz);
            if (order == 1) useExcess = false;
        }
        if (order == 0 && useExcess) launch_incr(st_, h_bcHi, h_excess, -1.0, hn);

        // the complement's Neumann ends roll in boundary data that stay zero for a diagonal metric: rhs + 0
        if (mixed_) launch_lep_vsolve_mixed(st_, ct, tj, V.dev, d_flatOf, vertPhi, rhsP, f_gam, f_efac, h_bcLo, h_bcHi, d_vbc,
                                            dz, dzCrse_, d_bad);
        else launch_lep_vsolve(st_, ct, tj, V.dev, Fd, vertPhi, rhsP, f_gam, h_bcLo, h_bcHi, dz);

        if (useHorizPhi) {
            if (full_) {
                Vs.run_aux_program(0, vertPhi);   // extrapAllGhosts(phi, 2): every ghost of every box, then the exchanges
                if (hasCF_) V.cf_homog(vertPhi, st_);   // homogeneousCFInterp                                     :1005
                V.exchange(vertPhi, st_);
                if (hasCF_) {                           // ExtrapolateCFEV + the corner exchange                  :1008-1013
                    Vs.cf_ev(0, vertPhi);
                    V.exchange(vertPhi, st_);
                }
                launch_lep_hgrad_full(st_, ct, tj, V.dev, Fd, vertPhi, h_gx, h_gy);
            } else {
                if (hasCF_) V.cf_homog(vertPhi, st_);
                V.exchange(vertPhi, st_);
                launch_lep_hgrad(st_, sct, tj, V.dev, Fd, vertPhi, h_gx, h_gy);
            }
            launch_lep_hrhs(st_, sct, tj, V.dev, Fd, h_gx, h_gy, h_excess, Hs.rhs(), -1.0 / dx_[0],
                            -1.0 / dx_[1], -1.0 / H_, useExcess);
            const double horizRhsNorm = Hs.norm(0, Hs.rhs(), prm.normType);
            if (prm.horizRhsTol * S.resNorms[0] > horizRhsNorm) useHorizPhi = false;
        }
        if (useHorizPhi) {
            Hs.solve(true, true, S.horizStats);
            if (horizRemoveAvg_) set_zero_avg(Hs.phi());
            launch_lep_extrude(st_, sct, tj, V.dev, Fd, vertPhi, Hs.phi());
            ++S.horizSolves;
        }

        // finalize the order                                                                     :836-933
        Vs.residual(0, tmpP, vertPhi, rhsP);
        resNorm = Vs.norm(0, tmpP, prm.normType);
        double relResNorm = resNorm / S.resNorms[0];
        const double prevRelResNorm = S.resNorms.back() / S.resNorms[0];
        double redu = prevRelResNorm - relResNorm;
        if (redu <= prm.hang && order == maxOrder) {
            launch_copy(st_, Vs.rhs(), rhsP, n);
            Vs.solve(true, true, S.fullStats);  // initial guess 0, homogeneous
            // on a mixed level the level solve stalls by itself and the fallback is known to blow up (so does the restated
            // reference, which aborts there): an error, never a wrong correction
            SOMAR_CHECK(!(mixed_ && S.fullStats.status != 0),
                        "the leptic solver's full-multigrid fallback failed on a level that mixes Neumann-Neumann columns "
                        "with Dirichlet / coarse-fine ended ones (MappedAMRMultiGrid: kaboom / solver blew up); choose a "
                        "max_order at which the last order still reduces the residual");
            Vs.residual(0, tmpP, vertPhi, rhsP);
            resNorm = Vs.norm(0, tmpP, prm.normType);
            relResNorm = resNorm / S.resNorms[0];
            S.usedFullSolver = 1;
        }
        std::swap(rhsP, tmpP);
        S.resNorms.push_back(resNorm);

        redu = prevRelResNorm - relResNorm;
        if (redu > prm.hang || order < maxOrder) {
            launch_lep_axpy(st_, ct, tj, V.dev, f_total, vertPhi, 1.0);
            exitStatus = (order < maxOrder - 1) ? 0 : 1;
        } else if (-redu > prm.hang) {
            exitStatus = (order == 0) ? 4 : 3;
            break;
        } else {
            exitStatus = (order == 0) ? 4 : 2;
            break;
        }
        if (!full_) useHorizPhi = false;  // LevelGeometry::isDiagonal()
    }

    if (exitStatus != 4) launch_lep_axpy(st_, ct, tj, V.dev, a_phi, f_total, 1.0);
    S.exitStatus = exitStatus;
    if (mixed_) check_bad();
    else sync();
}

}  // namespace somar
