// somar_amd/csrc/solver.cpp -- see solver.h for the reference map.
#include "solver.h"

#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace somar {

static const int S_MAX_COARSE = 4;  // MappedAMRPoissonOp::s_maxCoarse, MappedAMRPoissonOp.cpp:55
enum { SLOT_TMP = 0, SLOT_SUMS = 8, NSLOTS = 16 };

PressureSolver::PressureSolver(Comm* comm, hipStream_t shared, const Tuning& tune) : tune_(tune), comm_(comm ? comm : &self_)
{
    if (shared) { st_ = shared; own_stream_ = false; }
    else SOMAR_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    d_scalars = DevBuf<double>::zeros(NSLOTS);
    SOMAR_HIP(hipDeviceSynchronize());
    SOMAR_HIP(hipHostMalloc(&h_scalars, (NSLOTS + 2) * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped));
    h_seq_ = reinterpret_cast<unsigned long long*>(h_scalars + NSLOTS);
    *h_seq_ = 0;
}

PressureSolver::~PressureSolver()
{
    drop_graphs();
    mp_free();
    mc_free();
    if (st_) hipStreamSynchronize(st_);
    if (st_comm_) { hipStreamSynchronize(st_comm_); hipStreamDestroy(st_comm_); }
    if (ev_ready_) hipEventDestroy(ev_ready_);
    if (ev_done_) hipEventDestroy(ev_done_);
    for (Prof& p : prof_) {
        for (hipEvent_t e : p.a) hipEventDestroy(e);
        for (hipEvent_t e : p.b) hipEventDestroy(e);
    }
    if (h_scalars) hipHostFree(h_scalars);
    coarse_.reset();
    lev.clear();
    if (st_ && own_stream_) hipStreamDestroy(st_);
}

void PressureSolver::sync() { SOMAR_HIP(hipStreamSynchronize(st_)); }

void PressureSolver::profile_enable(bool on)
{
    const int POOL = 4096;
    if (on)
        for (Prof& p : prof_) {
            while ((int)p.a.size() < POOL) {
                hipEvent_t e0, e1;
                SOMAR_HIP(hipEventCreate(&e0));
                SOMAR_HIP(hipEventCreate(&e1));
                p.a.push_back(e0);
                p.b.push_back(e1);
            }
            p.used = 0;
        }
    profiling_ = on;
}
void PressureSolver::prof_begin(int k)
{
    Prof& p = prof_[k];
    if (p.used < (int)p.a.size()) SOMAR_HIP(hipEventRecord(p.a[p.used], st_));
}
void PressureSolver::prof_end(int k)
{
    Prof& p = prof_[k];
    if (p.used < (int)p.a.size()) { SOMAR_HIP(hipEventRecord(p.b[p.used], st_)); ++p.used; }
}
void PressureSolver::profile_get(int kernel, int* count, double* total_ms)
{
    SOMAR_CHECK(kernel >= 0 && kernel < 4, "profile id: 0 GSRB, 1 operator / residual, 2 remote ghost exchanges, 3 replicated tail");
    sync();
    Prof& p = prof_[kernel];
    double tot = 0.0;
    for (int i = 0; i < p.used; ++i) {
        float ms = 0.f;
        SOMAR_HIP(hipEventElapsedTime(&ms, p.a[i], p.b[i]));
        tot += ms;
    }
    *count = p.used;
    *total_ms = tot;
    p.used = 0;
}

template <class T>
void PressureSolver::xchg(const Level& L, T* f)
{
    const bool timed = profiling_ && !L.plan.peers.empty();
    if (timed) prof_begin(2);
    L.exchange(f, st_);
    if (timed) prof_end(2);
}
template void PressureSolver::xchg<double>(const Level&, double*);   // (solver_multi.cpp calls it too)

double PressureSolver::fetch_scalar(int slot)
{
    fetch_scalars(slot, 1);
    return h_scalars[slot];
}

// d_scalars[slot .. slot+n) -> h_scalars[slot .. slot+n).  The stopping tests of BiCGStab and of the outer iteration need
// a handful of scalars per V-cycle on the host; a copy + stream synchronize costs ~25 us each.  Instead a one-thread
// kernel stores the values into coherent host memory followed by a sequence number, and the host spins on that
// number: the round trip drops to the latency of a PCIe write (SOMAR_POLL_FETCH=0 restores copy + synchronize).
void PressureSolver::fetch_scalars(int slot, int n)
{
    if (!tune_.poll_fetch || capturing_) {
        SOMAR_HIP(hipMemcpyAsync(h_scalars + slot, d_scalars + slot, n * sizeof(double), hipMemcpyDeviceToHost, st_));
        SOMAR_HIP(hipStreamSynchronize(st_));
        return;
    }
    bottom_collect();   // (the spin below compares for equality with ONE sequence number: nothing may be outstanding)
    const unsigned long long want = ++fetch_seq_;
    launch_publish(st_, d_scalars + slot, n, h_scalars + slot, h_seq_, want);
    wait_published(want);
}

// the host side of a published scalar: spin on the sequence number the device stores last
void PressureSolver::wait_published(unsigned long long want)
{
    unsigned long long spins = 0;
    while (__atomic_load_n(h_seq_, __ATOMIC_ACQUIRE) != want) {
        if ((++spins & 0xfffff) == 0) {  // every ~1M spins: has the stream died or drained without publishing?
            const hipError_t q = hipStreamQuery(st_);
            if (q == hipSuccess) {
                if (__atomic_load_n(h_seq_, __ATOMIC_ACQUIRE) == want) break;
                throw Error(-2, "scalar publish kernel finished without publishing");
            }
            if (q != hipErrorNotReady) SOMAR_HIP(q);
        }
    }
}

// the host side of a one-launch bottom solve: its (iterations, exit code), published by the kernel's last thread.  Nothing in
// the cycle branches on them, so graph_cycle enqueues the up leg first and the GPU never waits for this round trip.
void PressureSolver::bottom_collect()
{
    if (!bottom_pending_) return;
    const unsigned long long want = bottom_pending_;
    bottom_pending_ = 0;   // (dropped whatever happens below)
    wait_published(want);
    bottom_iters = (int)h_scalars[SLOT_TMP];
    bottom_exit = (int)h_scalars[SLOT_TMP + 1];
}

double* PressureSolver::work(int which)
{
    return which == 0 ? f_uberRes : (which == 1 ? f_uberCorr : f_best);
}

double* PressureSolver::field(int depth, int which)
{
    if (depth < 0 || depth >= (int)lev.size() || !finalized) return nullptr;
    switch (which) {
        case 0: return depth == 0 ? f_phi : nullptr;
        case 1: return depth == 0 ? f_rhs : nullptr;
        case 2: return depth == 0 ? f_uberRes : f_res[depth];
        case 3: return depth == 0 ? f_uberCorr : f_corr[depth];
        case 4: return depth == 0 ? f_best : nullptr;
        case 5: return f_scratch[depth];
        case 6: return depth == 0 ? amr_field(0) : nullptr;
        case 7: return depth == 0 ? amr_field(1) : nullptr;
        case 8: return depth == 0 ? heat_field(0) : nullptr;
        case 9: return depth == 0 ? heat_field(1) : nullptr;
        case 10: case 11: case 12: return (depth == 0 && which - 10 < prm.spaceDim) ? heat_flux(which - 10) : nullptr;
        default: return nullptr;
    }
}

// ------------------------------------------------------------------------------------
// definition
// ------------------------------------------------------------------------------------
void PressureSolver::define(const IBox& domain, const bool periodic[3], const double dx[3],
                            const int bc_type[3][2], const std::vector<IBox>& boxes,
                            const std::vector<int>& owner, double alpha, double beta, const SolverParams& p,
                            const double* dxCrse)
{
    SOMAR_CHECK(lev.empty(), "solver already defined");
    prm = p;
    hasCF_ = dxCrse != nullptr;
    if (hasCF_)
        for (int d = 0; d < 3; ++d) dxCrse_[d] = dxCrse[d];
    SOMAR_CHECK(prm.relaxMode == RELAX_LEVEL_GSRB || prm.relaxMode == RELAX_JACOBI || prm.relaxMode == RELAX_LINE_GSRB ||
                    prm.relaxMode == RELAX_LOOSE_GSRB,
                "relax_mode must be 0 (Jacobi), 1 (LevelGSRB), 2 (LooseGSRB) or 3 (LineGSRB)");
    SOMAR_CHECK(prm.precondMode == PRECOND_DIAG_RELAX || prm.precondMode == PRECOND_NONE ||
                    prm.precondMode == PRECOND_DIAG_LINE_RELAX,
                "bad precondMode");
    for (int d = 0; d < p.spaceDim; ++d)
        for (int s = 0; s < 2; ++s)
            SOMAR_CHECK(periodic[d] || bc_type[d][s] == BC_NEUM || bc_type[d][s] == BC_DIRI,
                        "physical BCs are Neumann (0) or Dirichlet (1)");
    SOMAR_CHECK(prm.spaceDim == 2 || prm.spaceDim == 3, "space_dim must be 2 or 3");
    diri_ = false;
    for (int d = 0; d < p.spaceDim; ++d)
        for (int s = 0; s < 2; ++s)
            if (!periodic[d] && bc_type[d][s] == BC_DIRI) diri_ = true;
    std::unique_ptr<Level> L(new Level);
    if (prm.spaceDim == 2) {
        SOMAR_CHECK(domain.size(2) == 1, "space_dim 2 wants a domain (and boxes) one cell thick in z");
        if (prm.relaxMode == RELAX_LINE_GSRB || prm.precondMode == PRECOND_DIAG_LINE_RELAX)
            for (const IBox& b : boxes)   // 'LineGSRBIter2D: region must have a vertical lower bound of zero' (GSRBF.ChF:1561-1565)
                SOMAR_CHECK(b.lo[1] == domain.lo[1],
                            "2-D line relaxation wants boxes that start at the bottom of the vertical (direction 1)");
        L->active[2] = 0;
    }
    L->alpha = alpha;
    L->beta = beta;
    L->define(domain, periodic, dx, bc_type, boxes, owner, comm_, tune_);
    L->alloc_metric();
    if (hasCF_) {
        L->define_cf(dxCrse_);
        // Line relaxation with coarse-fine boundaries at the ENDS of a column: LineGSRB::relax hands the Fortran the codes of
        // BCDescriptor::stencil (BCInterface/BCDescriptor.H:218-229), which is BCType::None for every box end inside the domain --
        // the BCType_CF row of LineGSRBIter3D / 2D (GSRBF.ChF:1804-1817, 1588-1590) is never reached from there -- so such an end
        // gets coeff1 = 0 ("low-order extrapolation") and the coarse-fine ghost is not read.  The kernels do exactly that.
    }
    lev.push_back(std::move(L));
}

void PressureSolver::set_metric_ortho(int patch, const double* jg0, const double* jg1, const double* jg2,
                                      const double* jinv)
{
    metric_written("ortho");
    const double* jg[4] = {jg0, jg1, jg2, jinv};
    for (int w = 0; w < 4; ++w) {
        if (w < 3 && w >= prm.spaceDim) continue;
        SOMAR_CHECK(jg[w] != nullptr, "null metric array");
        const CallerArray a = io_metric(0, w, true);
        a.L->move_host(a.f, patch, const_cast<double*>(jg[w]), a.shape, true, st_);
    }
    sync();
}

// Semicoarsening rule + fallback, MappedAMRPoissonOpFactory.cpp:476-550
bool PressureSolver::build_coarser(int depth)
{
    if (prm.maxDepth >= 0 && depth > prm.maxDepth) {
        SOMAR_CHECK(depth > (int)forcedRatios.size(), "You must make the maxDepth large enough to accomodate the mini V-cycles");
        return false;
    }
    Level& F = *lev[depth - 1];
    int prev[3] = {1, 1, 1};
    for (auto& r : mgRefRatios)
        for (int d = 0; d < 3; ++d) prev[d] *= r[d];
    const int nd = prm.spaceDim;
    const int mmc[3] = {S_MAX_COARSE, S_MAX_COARSE, nd == 3 ? S_MAX_COARSE : 1};
    int r[3] = {1, 1, 1};
    const bool forced = depth <= (int)forcedRatios.size();  // the mini V-cycle's coarsening pattern, Factory.cpp:414-441
    if (forced) {
        for (int d = 0; d < 3; ++d) r[d] = forcedRatios[depth - 1][d];
        int tot[3];
        for (int d = 0; d < 3; ++d) tot[d] = prev[d] * r[d] * mmc[d];
        SOMAR_CHECK(coarsenable(lev[0]->boxes, tot),
                    "Could not coarsen grids for mini V-cycle: the block factor is too small for this refinement ratio");
    }
    double maxDx = 0.0;
    for (int d = 0; d < nd; ++d) maxDx = std::max(maxDx, F.dx[d]);
    for (int d = 0; d < nd && !forced; ++d)
        if (F.dx[d] <= maxDx / 2.0) r[d] = 2;
    if (!forced && r[0] * r[1] * r[2] == 1) { r[0] = r[1] = 2; r[2] = nd == 3 ? 2 : 1; }
    int tot[3];
    for (int d = 0; d < 3; ++d) tot[d] = prev[d] * r[d] * mmc[d];
    const std::vector<IBox>& base = lev[0]->boxes;
    if (!forced && !coarsenable(base, tot)) {
        int q[3] = {1, 1, 1};
        for (int d = 0; d < nd; ++d) {
            q[d] = 2;
            int t2[3];
            for (int e = 0; e < 3; ++e) t2[e] = prev[e] * mmc[e] * q[e];
            if (!coarsenable(base, t2)) q[d] = 1;
        }
        if (q[0] * q[1] * q[2] == 1) return false;
        int refDir = 0;
        while (refDir < nd && q[refDir] != 1) ++refDir;
        SOMAR_CHECK(refDir < nd, "semicoarsening fallback: no stuck direction");
        for (int d = 0; d < nd; ++d)
            if (q[d] > 1 && F.dx[d] / F.dx[refDir] > 0.5) q[d] = 1;
        if (q[0] * q[1] * q[2] == 1) return false;
        for (int d = 0; d < 3; ++d) { r[d] = q[d]; tot[d] = prev[d] * r[d] * mmc[d]; }
        if (!coarsenable(base, tot)) return false;
    }
    mgRefRatios.push_back({r[0], r[1], r[2]});
    for (int d = 0; d < 3; ++d) F.mgCrseRefRatio[d] = r[d];
    F.hasCoarser = true;

    std::unique_ptr<Level> C(new Level);
    C->active[2] = F.active[2];
    C->alpha = F.alpha;
    C->beta = F.beta;
    std::vector<IBox> cb;
    for (const IBox& b : F.boxes) cb.push_back(b.coarsen(r));
    double cdx[3];
    for (int d = 0; d < 3; ++d) cdx[d] = F.dx[d] * (double)r[d];
    C->define(F.domain.coarsen(r), F.periodic, cdx, F.bc_type, cb, F.owner, comm_, tune_);
    C->alloc_metric();
    if (hasCF_) C->define_cf(dxCrse_);  // CFRegion::coarsen + the AMR coarser level's spacing (Factory.cpp:596-600)
    // coarse metrics: fill_MGfields, MappedAMRPoissonOpFactory.cpp:1164-1234
    for (int pi = 0; pi < C->npatches(); ++pi)
        for (int d = 0; d < nd; ++d)
            launch_avg_face(st_, C->dev, F.dev, pi, C->hpatches[pi].n, C->dev.jg[d], F.dev.jg[d], d, r);
    if (full_) {
        C->alloc_cross_metric();
        for (int pi = 0; pi < C->npatches(); ++pi)
            for (int d = 0; d < nd; ++d)
                for (int c = 0; c < nd; ++c)
                    if (c != d)
                        launch_avg_face(st_, C->dev, F.dev, pi, C->hpatches[pi].n, C->dev.jgf[d][c], F.dev.jgf[d][c], d, r);
    }
    launch_avg_harmonic(st_, C->dev, F.dev, C->dev.jinv, F.dev.jinv, r);
    launch_lapdiag(st_, C->dev);
    fill_metric_ghosts(*C);
    lev.push_back(std::move(C));
    return true;
}

// The fused sweep recomputes its neighbours' red ring, so Jg and Jinv need ghost values wherever a
// neighbouring box or a periodic image exists.  NOTE: a face shared by two boxes (or by periodic
// images) is stored by both; this exchange makes the two copies identical (the low-side owner's
// value wins).  They already are identical when both come from one evaluation of the map.
void PressureSolver::fill_metric_ghosts(Level& L)
{
    // on a level with coarse-fine boundaries the recomputed red ring also needs a neighbour's coefficient on a face
    // that no box owns as a low face (see Copier::define_faces); the ordinary exchange then has the last word
    for (int d = 0; d < 3; ++d)
        if (L.cf_faces[d]) L.cf_faces[d]->run(L.dev.jg[d], L.dev.jg[d], st_);
    for (int d = 0; d < 3; ++d) xchg(L, L.dev.jg[d]);
    if (full_)
        for (int d = 0; d < 3; ++d)
            for (int c = 0; c < 3; ++c)
                if (c != d && L.dev.jgf[d][c]) xchg(L, L.dev.jgf[d][c]);
    xchg(L, L.dev.jinv);
}

// null-space probe, MappedAMRPoissonOpFactory.cpp:659-693
void PressureSolver::probe_null_space(int d)
{
    Level& L = *lev[d];
    DevBuf<double> phi = L.alloc_field(), rhs0 = L.alloc_field(), res = L.alloc_field();
    launch_set(st_, phi, L.field_elems, 0.0);
    apply_op(d, rhs0, phi);
    launch_set(st_, phi, L.field_elems, 1.0);
    residual(d, res, phi, rhs0);
    launch_reduce(st_, L.dev, res, nullptr, 3, d_partials, d_scalars + SLOT_TMP);
    comm_->allreduce(d_scalars + SLOT_TMP, 1, 1, st_);
    const double maxNorm = std::fabs(fetch_scalar(SLOT_TMP));
    L.zeroAvg = maxNorm < 0.01 * (probe_eps > 0.0 ? probe_eps : prm.eps);
}

void PressureSolver::finalize()
{
    SOMAR_CHECK(!lev.empty() && !finalized, "finalize before define / twice");
    if (mp_mode_ == 1) {
        const std::string why = mixed_refusal();   // (the metric kind is only known now)
        SOMAR_CHECK(why.empty(), "finalize: mixed precision (set_precision mode 1) is not available for " + why);
    }
    // Tuning::timing: wall time of the stages below on stderr (what a re-definition of the hierarchy costs)
    const bool timing = tune_.timing != 0;
    auto now = [&]() { if (timing) hipDeviceSynchronize(); return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double>(b - a).count();
    };
    const auto t0 = now();
    launch_lapdiag(st_, lev[0]->dev);
    fill_metric_ghosts(*lev[0]);
    int depth = 1;
    while (build_coarser(depth)) {
        if (comm_->size > 1 && lev[depth]->valid_cells_global <= tune_.agglom_cells && !full_) {
            build_agglomerated_tail(depth);
            break;
        }
        ++depth;
    }
    const auto t1 = now();
    detect_metric_flags();
    {
        // the fused red+black 19-point sweep on levels of large boxes
        const int min_box = (int)tune_.fused19_min_box;
        fused19_.assign(lev.size(), 0);
        for (size_t d = 0; d < lev.size(); ++d) {
            Level& L = *lev[d];
            bool ok = full_ && min_box >= 0 && full_march((int)d) && tune_.full_rows == 8 && !L.boxes.empty();
            for (const IBox& b : L.boxes)
                for (int a = 0; a < 3; ++a) ok = ok && b.size(a) >= std::max(min_box, 8) && (a != 0 || b.size(a) % 2 == 0);
            fused19_[d] = ok ? 1 : 0;
            if (ok != L.march.fused19) L.build_march_tiles(MarchRequest{L.march.narrow7, L.march.tall7, ok});
        }
    }
    choose_narrow_tiles();
    const auto t2 = now();
    struct Report {
        bool on; std::chrono::steady_clock::time_point t0, t1, t2; long long cells;
        ~Report() {
            if (!on) return;
            hipDeviceSynchronize();
            const auto t3 = std::chrono::steady_clock::now();
            fprintf(stderr, "[somar timing] finalize %lld cells: coarse hierarchy %.3f s, uniform detection %.3f s, fields + probes %.3f s\n",
                    cells, std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count(),
                    std::chrono::duration<double>(t3 - t2).count());
        }
    } report{timing, t0, t1, t2, lev[0]->valid_cells_global};
    (void)secs;
    const int D = (int)lev.size();
    for (auto* v : {&f_res, &f_corr, &f_scratch, &f_pp}) {
        v->clear();
        v->resize(D);
    }
    if (full_) refuse_full_with_neum_faces("finalize");
    build_face_slices();   // before the op lists of depth 0, which take their slices from it
    if (full_) {
        SOMAR_CHECK(prm.relaxMode == RELAX_LEVEL_GSRB || prm.relaxMode == RELAX_JACOBI || prm.relaxMode == RELAX_LINE_GSRB,
                    "the non-diagonal metric path offers LevelGSRB, LineGSRB and Jacobi");
        // (space_dim 2: LineGSRBIter2D with its two cross terms, line_gsrb.hip)
        f_psi.clear();
        f_psi.resize(D);
        full_prog_.resize(D);
        for (int d = 0; d < D; ++d) {
            f_psi[d] = lev[d]->alloc_field();
            build_full_programs(d);
        }
    }
    d_diri_ops_.clear();
    d_diri_ops_.resize(D);
    n_diri_ops_.assign(D, 0);
    if (diri_)
        for (int d = 0; d < D; ++d) build_diri_ops(d);
    build_neum_ops();
    for (int d = 0; d < D; ++d) {
        if (d > 0) { f_res[d] = lev[d]->alloc_field(); f_corr[d] = lev[d]->alloc_field(); }
        f_scratch[d] = lev[d]->alloc_field();
        f_pp[d] = lev[d]->alloc_field();
    }
    Level& L0 = *lev[0];
    f_phi = L0.alloc_field();
    f_rhs = L0.alloc_field();
    f_uberRes = L0.alloc_field();
    f_uberCorr = L0.alloc_field();
    f_best = L0.alloc_field();
    // folded prolongation: child volumes and total volume per depth
    f_W.clear();
    f_W.resize(D);
    sf_valid_.assign(D, 0);
    d_fold = DevBuf<double>::zeros((size_t)D * 8);
    SOMAR_HIP(hipDeviceSynchronize());
    for (int d = 0; d + 1 < D; ++d) {
        Level& F = *lev[d];
        Level& C = *lev[d + 1];
        f_W[d + 1] = C.alloc_field();
        launch_child_volume(st_, C.dev, F.dev, f_W[d + 1], F.mgCrseRefRatio, F.dxProduct);
        launch_reduce(st_, C.dev, f_W[d + 1], nullptr, 2, d_partials, d_fold + 8 * d + 2);  // V = sum of volumes (> 0)
        comm_->allreduce(d_fold + 8 * d + 2, 1, 0, st_);
    }
    for (int i = 0; i < 8; ++i) bicg[i] = lev[D - 1]->alloc_field();
    for (int d = 0; d < D; ++d) probe_null_space(d);
    // first depth whose V-cycle leg is launch-bound (see solver.h); one rank only, never inside a sharded region
    graph_from_ = -1;
    if (comm_->size == 1 && !coarse_ && tune_.graph_cells > 0)
        for (int d = 0; d <= D - 2; ++d)
            if (lev[d]->valid_cells_global <= tune_.graph_cells) { graph_from_ = d; break; }
    sync();
    finalized = true;
    if (mp_mode_ == 1 || comm_->size > 1) mp_setup();   // (sharded: every rank's mode has to be the same one, fp64 included)
}

// The hierarchy from `depth` on, replicated on every rank (see solver.h).  lev[depth] stays as the sharded
// landing layout of the restriction; its data are allgathered into depth 0 of a communicator-less solver that
// owns every box and builds the remaining depths itself with the same rules.
void PressureSolver::build_agglomerated_tail(int depth)
{
    Level& T = *lev[depth];
    SolverParams cp = prm;
    if (cp.maxDepth >= 0) cp.maxDepth = std::max(0, cp.maxDepth - depth);
    Tuning ct = tune_;
    ct.graph_cells = 0;  // graph replay is exercised (and measured) on single-process runs only
    coarse_.reset(new PressureSolver(nullptr, st_, ct));
    coarse_->probe_eps = probe_eps > 0.0 ? probe_eps : prm.eps;
    for (int a = 0; a < 3; ++a)
        for (int q = 0; q < 2; ++q) coarse_->bc_value_[a][q] = bc_value_[a][q];
    std::vector<int> own(T.boxes.size(), 0);
    coarse_->define(T.domain, T.periodic, T.dx, T.bc_type, T.boxes, own, T.alpha, T.beta, cp,
                    hasCF_ ? dxCrse_ : nullptr);
    Level& R = *coarse_->lev[0];
    // metric: faces of a box live at indices 0..n, so take one layer beyond the valid cells
    agglom_metric_.define_allgather(T, R, 1, comm_);   // kept: a metric refresh runs it again
    for (int d = 0; d < prm.spaceDim; ++d) agglom_metric_.run(T.dev.jg[d], R.dev.jg[d], st_);
    agglom_metric_.run(T.dev.jinv, R.dev.jinv, st_);
    sync();
    coarse_->finalize();
    agglom_depth_ = depth;
    agglom_gather_.define_allgather(T, R, 0, comm_);
    std::vector<CopyItem> back;
    for (int pi = 0; pi < T.npatches(); ++pi) {
        CopyItem it;
        std::memset(&it, 0, sizeof(it));
        it.src_patch = T.local[pi];  // replicated layout: patch index = global box index
        it.dst_patch = pi;
        for (int d = 0; d < 3; ++d) it.n[d] = T.hpatches[pi].n[d];
        back.push_back(it);
    }
    n_agglom_back_ = (int)back.size();
    if (n_agglom_back_) {
        d_agglom_back_ = DevBuf<CopyItem>::from(back);
        SOMAR_HIP(hipDeviceSynchronize());
    }
}

void PressureSolver::agglom_cycle(double* corr, const double* res, bool corr_zero)
{
    Level& T = *lev[agglom_depth_];
    PressureSolver& C = *coarse_;
    double* rC = C.work(0);
    double* cC = C.work(1);
    if (profiling_) prof_begin(3);
    agglom_gather_.run(res, rC, st_);
    if (!corr_zero) agglom_gather_.run(corr, cC, st_);
    C.bottom_metric = bottom_metric;
    C.bottom_eps_eff = bottom_eps_eff;
    C.prm.num_smooth_down = prm.num_smooth_down;
    C.prm.num_smooth_up = prm.num_smooth_up;
    C.prm.num_smooth_bottom = prm.num_smooth_bottom;
    C.prm.numMG = prm.numMG;
    C.cycle_override_ = cycle_override_;   // inside an F-cycle's inner V-cycle the replicated tail runs a V-cycle too
    C.cycle(0, cC, rC, corr_zero);
    C.cycle_override_ = 0;
    bottom_iters = C.bottom_iters;
    bottom_exit = C.bottom_exit;
    launch_copy_items2(st_, C.lev[0]->dev.patches, T.dev.patches, d_agglom_back_, n_agglom_back_, cC, corr);
    if (profiling_) prof_end(3);
}

// ------------------------------------------------------------------------------------
// metric refresh of a finalized solver (see solver.h).  The layout, the BCs and the coefficients stay; everything finalize
// derived from the metric is recomputed, in finalize's order, into the buffers it allocated -- so the result is what a
// fresh define + set_metric + finalize with the new metric computes, bit for bit.
// ------------------------------------------------------------------------------------
void PressureSolver::check_idle(const char* what) const
{
    SOMAR_CHECK(!updating_, std::string(what) + " while a metric update is open (end it first: somar_solver_metric_update_end / "
                                                "somar_amr_metric_update_end)");
}

void PressureSolver::metric_written(const char* producer)
{
    SOMAR_CHECK(!lev.empty() && (!finalized || updating_), "set_metric before define / after finalize");
    if (!finalized) return;
    const bool diag = !strcmp(producer, "ortho") || !strcmp(producer, "uniform") || !strcmp(producer, "cylindrical");
    SOMAR_CHECK(!(diag && full_), std::string("set_metric_") + producer +
                                      ": this solver was finalized with the non-diagonal metric (its kernels and ghost programs "
                                      "are fixed at finalize); use set_metric_full / set_metric_map with a non-diagonal map");
    SOMAR_CHECK(diag || full_, std::string("set_metric_") + producer +
                                   ": this solver was finalized with a diagonal metric (its kernels and ghost programs are fixed "
                                   "at finalize); use set_metric_ortho / set_metric_uniform");
    metric_written_ = true;
}

void PressureSolver::metric_update_begin(bool amr_member_ok)
{
    SOMAR_CHECK(finalized, "metric_update_begin: the solver is not finalized (set the metric before finalize instead)");
    SOMAR_CHECK(!amr_member_ || amr_member_ok,
                "metric update on a level of an AMR hierarchy goes through the hierarchy (somar_amr_metric_update_begin / _end)");
    SOMAR_CHECK(!updating_, "metric_update_begin: an update is already open");
    updating_ = true;
    metric_written_ = false;
}

bool PressureSolver::metric_update_end(bool only_if_written)
{
    SOMAR_CHECK(updating_, "metric_update_end without metric_update_begin");
    const bool run = metric_written_ || !only_if_written;
    updating_ = false;
    metric_written_ = false;
    if (run) refresh_metric();
    return run;
}

// Diagonal metric: a Cartesian map hands over constant arrays (CartesianMap.cpp:261-280): J g^{aa} and J^{-1} are then the same
// number on every face / in every cell of a depth -- and of every coarser depth, whose averages of equal numbers are exact.  The
// k-marching kernels take such coefficients from StencilParams instead of streaming them (same arithmetic, same bits).
// Tuning::no_uniform disables the detection (A/B measurements, parity tests of the streaming path on Cartesian inputs).
// Non-diagonal metric: are J g^{xy} (x-faces) and J g^{yx} (y-faces) identically zero on a depth?  True for every map of the
// form x = xi, y = eta, z = z(xi, eta, zeta) -- BathymetricBaseMap (geometry/maps/BathymetricBaseMap.cpp:133-313) and all its
// subclasses: the x-face normal has no eta component.  Coarse depths inherit it (averages of zeros).  Tuning::no_zero_planes
// switches the detection off (A/B; the kernels then multiply the stored zeros, same values).
// One launch and one download for every depth and array; the item table is built at finalize and serves every refresh -- so a
// depth with a plane missing at finalize (mm_first_ = -1) stays "not zero" for the life of the solver, which is the safe side.
void PressureSolver::detect_metric_flags()
{
    const int D = (int)lev.size();
    const bool uni_on = !tune_.no_uniform && !full_ && prm.spaceDim == 3;
    const bool zero_on = !tune_.no_zero_planes && full_ && prm.spaceDim == 3;
    for (auto& Lp : lev) { Lp->dev.P.uniform = 0; Lp->dev.P.zero_xy = 0; }
    if (!uni_on && !zero_on) return;
    const int na = uni_on ? 4 : 2;
    auto array = [&](Level& L, int a, int* dir) -> const double* {
        if (uni_on) { *dir = a < 3 ? a : -1; return a < 3 ? L.dev.jg[a] : L.dev.jinv; }
        *dir = a;
        return a == 0 ? L.dev.jgf[0][1] : L.dev.jgf[1][0];
    };
    if (!d_mm_items_) {
        std::vector<MinMaxItem> items;
        mm_first_.assign(D, 0);
        for (int d = 0; d < D; ++d) {
            Level& L = *lev[d];
            mm_first_[d] = (int)items.size();
            int dir;
            for (int a = 0; a < na; ++a)
                if (!array(L, a, &dir)) mm_first_[d] = -1;   // a plane that was never allocated: the depth counts as "not zero"
            for (int a = 0; a < na && mm_first_[d] >= 0; ++a)
                for (int pi = 0; pi < L.npatches(); ++pi) {
                    MinMaxItem it;
                    it.a = array(L, a, &it.dir);
                    it.patches = L.dev.patches;
                    it.patch = pi;
                    items.push_back(it);
                }
        }
        n_mm_items_ = (int)items.size();
        d_mm_out_ = DevBuf<double>(2 * (size_t)std::max(n_mm_items_, 1) * MM_CH + 9 * (size_t)D);
        if (n_mm_items_) {
            d_mm_items_ = DevBuf<MinMaxItem>::from(items);
            SOMAR_HIP(hipDeviceSynchronize());   // null-stream copy vs the solver's non-blocking stream
        } else d_mm_items_ = DevBuf<MinMaxItem>(1);
    }
    std::vector<double> mm(2 * (size_t)n_mm_items_ * MM_CH);
    launch_minmax_all(st_, d_mm_items_, n_mm_items_, d_mm_out_);
    if (n_mm_items_) SOMAR_HIP(hipMemcpyAsync(mm.data(), d_mm_out_, sizeof(double) * mm.size(), hipMemcpyDeviceToHost, st_));
    SOMAR_HIP(hipStreamSynchronize(st_));
    // per depth: uniform -- (max, -min) of the four arrays, -inf where a rank holds no box; zero planes -- max |value|
    std::vector<double> h(9 * (size_t)D, -HUGE_VAL);
    for (int d = 0; d < D; ++d) {
        Level& L = *lev[d];
        const int np = L.npatches();
        double* hd = h.data() + 9 * d;
        hd[8] = (mm_first_[d] < 0 && np) ? 1.0 : 0.0;
        for (int a = 0; a < na && np && mm_first_[d] >= 0; ++a) {
            const size_t q0 = (size_t)(mm_first_[d] + a * np) * MM_CH, q1 = q0 + (size_t)np * MM_CH;
            for (size_t q = q0; q < q1; ++q) {
                if (uni_on) {
                    hd[2 * a] = std::max(hd[2 * a], mm[2 * q + 1]);
                    hd[2 * a + 1] = std::max(hd[2 * a + 1], -mm[2 * q]);
                } else {
                    if (std::isfinite(mm[2 * q])) hd[8] = std::max(hd[8], std::fabs(mm[2 * q]));
                    if (std::isfinite(mm[2 * q + 1])) hd[8] = std::max(hd[8], std::fabs(mm[2 * q + 1]));
                }
            }
        }
    }
    if (comm_->size > 1) {
        double* dh = d_mm_out_ + 2 * (size_t)std::max(n_mm_items_, 1) * MM_CH;
        SOMAR_HIP(hipMemcpyAsync(dh, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st_));
        comm_->allreduce(dh, (int)h.size(), 1, st_);
        SOMAR_HIP(hipMemcpyAsync(h.data(), dh, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st_));
        SOMAR_HIP(hipStreamSynchronize(st_));
    }
    for (int d = 0; d < D; ++d) {
        Level& L = *lev[d];
        if (!(L.active[0] && L.active[1] && L.active[2])) continue;
        const double* hd = h.data() + 9 * d;
        if (zero_on) { L.dev.P.zero_xy = hd[8] == 0.0 ? 1 : 0; continue; }
        bool uni = true;
        for (int a = 0; a < 4; ++a) uni = uni && std::isfinite(hd[2 * a]) && hd[2 * a] == -hd[2 * a + 1];
        if (!uni) continue;
        L.dev.P.uniform = 1;
        for (int a = 0; a < 4; ++a) L.dev.P.uc[a] = hd[2 * a];
    }
}

// Narrow lane classes for the 7-point marching kernels where the metric is uniform (Level::build_march_tiles says why);
// Tuning::narrow_7pt = 0 | 1 forces never / always (A/B).  d_partials holds two doubles per tile of the largest table: sized at
// finalize, again when a table was rebuilt.  Where the metric is not uniform the fused sweep's table may take tall tiles
// (march_plan.h; Tuning::narrow_7pt = 0 and Tuning::no_narrow_tiles keep the equal columns).
void PressureSolver::choose_narrow_tiles()
{
    bool rebuilt = false;
    for (auto& Lp : lev) {
        const bool want = tune_.narrow_7pt >= 0 ? tune_.narrow_7pt != 0 : Lp->dev.P.uniform != 0;
        // (march_plan::tall_eligible holds the rule, the metric flag included; here only: can the fused sweep run on this level?)
        const bool tall = !full_ && Lp->dev.P.uniform == 0 && Lp->active[0] && Lp->active[1] && Lp->active[2];
        if (want != Lp->march.narrow7 || tall != Lp->march.tall7) { Lp->build_march_tiles(MarchRequest{want, tall, Lp->march.fused19}); rebuilt = true; }
    }
    if (d_partials && !rebuilt) return;
    int maxTiles = 1;
    for (auto& L : lev) maxTiles = std::max(std::max(maxTiles, L->dev.ntiles), std::max(L->rtiles.all.size(), L->ftiles.all.size()));
    SOMAR_HIP(hipStreamSynchronize(st_));
    d_partials.reset();
    d_partials = DevBuf<double>((size_t)maxTiles * 2);
}

void PressureSolver::refresh_metric()
{
    SOMAR_CHECK(finalized, "metric refresh before finalize");
    const bool timing = tune_.timing != 0;
    auto now = [&]() { if (timing) SOMAR_HIP(hipStreamSynchronize(st_)); return std::chrono::steady_clock::now(); };
    const auto t0 = now();
    const int D = (int)lev.size();
    const int nd = prm.spaceDim;
    if (d_coarsen_.empty()) {
        // k_coarsen_metric's work items per depth: the (face direction, component) arrays build_coarser averages, then J^{-1}
        d_coarsen_.resize(D);
        n_coarsen_.assign(D, 0);
        gy_coarsen_.assign(D, 1);
        for (int d = 1; d < D; ++d) {
            Level& F = *lev[d - 1];
            Level& C = *lev[d];
            std::vector<CoarsenItem> items;
            long long maxGroups = 1;
            for (int pi = 0; pi < C.npatches(); ++pi) {
                auto add = [&](const double* f, double* c, int dir) {
                    items.push_back(CoarsenItem{f, c, pi, dir});
                    const int* n = C.hpatches[pi].n;
                    const long long nj = n[1] + (dir == 1), nk = n[2] + (dir == 2);
                    maxGroups = std::max(maxGroups, (nj + 3) / 4 * nk);
                };
                for (int a = 0; a < nd; ++a) add(F.dev.jg[a], C.dev.jg[a], a);
                if (full_)
                    for (int a = 0; a < nd; ++a)
                        for (int c = 0; c < nd; ++c)
                            if (c != a) add(F.dev.jgf[a][c], C.dev.jgf[a][c], a);
                add(F.dev.jinv, C.dev.jinv, -1);
            }
            n_coarsen_[d] = (int)items.size();
            // enough workgroups to fill the device a few times over, spread evenly over the items
            gy_coarsen_[d] = (int)std::min<long long>(maxGroups, std::max<long long>(1, 8192 / std::max<int>(1, n_coarsen_[d])));
            if (!items.empty()) {
                d_coarsen_[d] = DevBuf<CoarsenItem>::from(items);
                SOMAR_HIP(hipDeviceSynchronize());   // null-stream copy vs the solver's non-blocking stream
            }
        }
    }
    launch_lapdiag(st_, lev[0]->dev);
    fill_metric_ghosts(*lev[0]);
    for (int d = 1; d < D; ++d) {
        Level& F = *lev[d - 1];
        Level& C = *lev[d];
        launch_coarsen_metric(st_, C.dev, F.dev, d_coarsen_[d], n_coarsen_[d], gy_coarsen_[d], F.mgCrseRefRatio);
        launch_lapdiag(st_, C.dev);
        fill_metric_ghosts(C);
    }
    if (coarse_) {
        Level& T = *lev[agglom_depth_];
        Level& R = *coarse_->lev[0];
        for (int a = 0; a < nd; ++a) agglom_metric_.run(T.dev.jg[a], R.dev.jg[a], st_);
        agglom_metric_.run(T.dev.jinv, R.dev.jinv, st_);
        sync();
        coarse_->refresh_metric();
    }
    const auto t1 = now();
    detect_metric_flags();
    choose_narrow_tiles();
    const auto t2 = now();
    for (int d = 0; d + 1 < D; ++d) {
        Level& F = *lev[d];
        Level& C = *lev[d + 1];
        launch_child_volume(st_, C.dev, F.dev, f_W[d + 1], F.mgCrseRefRatio, F.dxProduct);
        launch_reduce(st_, C.dev, f_W[d + 1], nullptr, 2, d_partials, d_fold + 8 * d + 2);
        comm_->allreduce(d_fold + 8 * d + 2, 1, 0, st_);
    }
    // the probe runs with the factory's coefficients, as at finalize (set_alpha_beta keeps the probe's choice, and so does this)
    const bool swap = coefs_saved_ && (lev[0]->alpha != aCoef_ || lev[0]->beta != bCoef_);
    std::vector<std::pair<double, double>> ab;
    if (swap)
        for (auto& L : lev) {
            ab.emplace_back(L->alpha, L->beta);
            L->alpha = aCoef_;
            L->beta = bCoef_;
            L->refresh_params();
        }
    for (int d = 0; d < D; ++d) probe_null_space(d);
    if (swap)
        for (int d = 0; d < D; ++d) {
            lev[d]->alpha = ab[d].first;
            lev[d]->beta = ab[d].second;
            lev[d]->refresh_params();
        }
    // the components' own operators stay (comp_set_op); their probes run again, as a separate solver's refresh would run them
    for (Component& c : comps_)
        if (c.op) probe_op(*c.op, nullptr);
    drop_graphs();   // captured launches carry the old StencilParams and tile tables in their arguments
    if (mp_K_ > 0) mp_convert_metric();   // the fp32 copies of a mixed-precision cycle (the uniform flags may have changed)
    if (ncomp_ > 1) mc_setup();           // the batched depths of a multi-component solver (likewise)
    sync();
    if (timing)
        fprintf(stderr, "[somar timing] metric refresh %lld cells: coarse depths %.3f s, flags + tiles %.3f s, volumes + probes %.3f s\n",
                lev[0]->valid_cells_global, std::chrono::duration<double>(t1 - t0).count(),
                std::chrono::duration<double>(t2 - t1).count(), std::chrono::duration<double>(now() - t2).count());
}

// ------------------------------------------------------------------------------------
// boundary transfers: what each resident array moves (one description), the two movers, the calls on caller arrays
// ------------------------------------------------------------------------------------
PressureSolver::CallerArray PressureSolver::io_metric(int depth, int which, bool up)
{
    SOMAR_CHECK(up ? depth == 0 : finalized && depth >= 0 && depth < this->depth(), "metric_download: depth out of range / not finalized");
    Level& L = level(depth);
    double* f = nullptr;
    int dir = -1;
    if (which >= 0 && which < 3) { f = L.dev.jg[which]; dir = which; }
    else if (which == 3) f = L.dev.jinv;
    else if (which == 4) f = L.dev.lapdiag;
    else if (which >= 16 && which < 25) { dir = (which - 16) / 3; f = L.dev.jgf[dir][(which - 16) % 3]; }
    SOMAR_CHECK(f && (dir < 0 || dir < prm.spaceDim), "metric_download: no such array (which 0..4, or 16 + 3a + b of a non-diagonal metric)");
    return {&L, {f, nullptr, nullptr}, dir >= 0 ? BoxIoShape::faces(dir) : BoxIoShape()};
}

PressureSolver::CallerArray PressureSolver::io_field(double* field, int depth, const int ghost[3], bool with_ghosts)
{
    SOMAR_CHECK(field && ghost, "no such field / null ghost");
    return {&level(depth), {field, nullptr, nullptr}, BoxIoShape::cells(ghost, with_ghosts)};
}

PressureSolver::CallerArray PressureSolver::io_vel(int dir)
{
    return {lev[0].get(), {vel(dir), nullptr, nullptr}, BoxIoShape::faces(dir)};
}

PressureSolver::CallerArray PressureSolver::io_cc_vel(const int ghost[3], bool up)
{
    SOMAR_CHECK(ghost, "null ghost");
    BoxIoShape s = BoxIoShape::cells(ghost, false);
    s.ncomp = prm.spaceDim;
    for (int d = 0; d < prm.spaceDim && up; ++d) {
        SOMAR_CHECK(ghost[d] >= 1, "the cell-centred velocity needs one ghost layer (CellToEdge reads it)");
        s.grow[d] = 1;
    }
    return {lev[0].get(), {cc_vel(0), cc_vel(1), prm.spaceDim > 2 ? cc_vel(2) : nullptr}, s};
}

PressureSolver::CallerArray PressureSolver::io_scale_cc(int which, const int ghost[3])
{
    Level& L = *lev[0];
    SOMAR_CHECK(finalized && (which == 0 || which == 1) && ghost, "set_scale_cc: bad argument");
    BoxIoShape s = BoxIoShape::cells(ghost, false);
    for (int d = 0; d < prm.spaceDim; ++d) {
        SOMAR_CHECK(ghost[d] >= 1, "the cell-centred scale needs the velocity's ghost layer");
        s.grow[d] = 1;
    }
    if (!f_sc_cc[which]) f_sc_cc[which] = L.alloc_field();
    return {&L, {f_sc_cc[which], nullptr, nullptr}, s};
}

PressureSolver::CallerArray PressureSolver::io_scale_face(int which, int dir)
{
    Level& L = *lev[0];
    SOMAR_CHECK(finalized && (which == 0 || which == 1) && dir >= 0 && dir < prm.spaceDim, "set_scale_face: bad argument");
    if (!f_sc_face[which][dir]) f_sc_face[which][dir] = L.alloc_field();
    return {&L, {f_sc_face[which][dir], nullptr, nullptr}, BoxIoShape::faces(dir)};
}

PressureSolver::CallerArray PressureSolver::io_heat_flux(int dir)
{
    return {lev[0].get(), {heat_flux(dir), nullptr, nullptr}, BoxIoShape::faces(dir)};
}

void PressureSolver::move_host(const CallerArray& a, int patch, double* host, bool up)
{
    a.L->move_host(a.f, patch, host, a.shape, up, st_);
    sync();
}

void PressureSolver::move_dev(const CallerArray& a, double* const* dev, bool up, bool checked)
{
    if (up) a.L->upload_dev(a.f, dev, a.shape, st_, checked);
    else a.L->download_dev(a.f, dev, a.shape, st_, checked);
}

void PressureSolver::check_table(Mem where, const CallerArray& a, const double* const* table, const char* what)
{
    if (where == Mem::Device) return a.L->check_dev_ptrs(table, a.shape, what);
    check_shape(a.shape);
    SOMAR_CHECK(table != nullptr, std::string(what) + ": null pointer table");
}

void PressureSolver::move_table(Mem where, const CallerArray& a, double* const* table, bool up)
{
    if (where == Mem::Device) return move_dev(a, table, up, true);
    for (int p = 0; p < a.L->npatches(); ++p)
        if (table[p]) a.L->move_host(a.f, p, table[p], a.shape, up, st_);
    sync();   // one drain after the last copy: the caller's arrays are free again / hold the result
}

void PressureSolver::solve_on(Mem where, double* const* phi, const int phi_ghost[3], const double* const* rhs, const int rhs_ghost[3],
                              bool zeroPhi, bool forceHomogeneous, SolveStats& st)
{
    SOMAR_CHECK(finalized, "solve on caller arrays: solver not finalized");
    const CallerArray P = io_field(f_phi, 0, phi_ghost, true), R = io_field(f_rhs, 0, rhs_ghost, false);
    check_table(where, P, phi, "phi");
    check_table(where, R, rhs, "rhs");
    move_table(where, R, const_cast<double* const*>(rhs), true);
    if (!zeroPhi) move_table(where, io_field(f_phi, 0, phi_ghost, false), phi, true);   // the valid cells
    solve(zeroPhi, forceHomogeneous, st);
    move_table(where, P, phi, false);
}

void PressureSolver::mac_project_on(Mem where, double* const* const u[3], double dt, bool zeroPressure, bool forceHomogeneous,
                                    SolveStats& st)
{
    SOMAR_CHECK(finalized, "MAC projection on caller arrays: solver not finalized");
    static const char* const name[3] = {"u0", "u1", "u2"};
    for (int d = 0; d < 3; ++d) check_table(where, io_vel(d), u[d], name[d]);
    for (int d = 0; d < 3; ++d) move_table(where, io_vel(d), u[d], true);
    mac_project(dt, zeroPressure, forceHomogeneous, st);
    for (int d = 0; d < 3; ++d) move_table(where, io_vel(d), u[d], false);
}

void PressureSolver::cc_project_on(Mem where, double* const* vel, const int ghost[3], double dt, bool zeroPressure,
                                   bool forceHomogeneous, bool wall, SolveStats& st)
{
    SOMAR_CHECK(finalized, "cell-centred projection on caller arrays: solver not finalized");
    const CallerArray up = io_cc_vel(ghost, true);
    check_table(where, up, vel, "vel");
    move_table(where, up, vel, true);
    cc_project(dt, zeroPressure, forceHomogeneous, wall, st);
    move_table(where, io_cc_vel(ghost, false), vel, false);
}

// ------------------------------------------------------------------------------------
// level operator
// ------------------------------------------------------------------------------------
bool PressureSolver::fused_relax(int d, int iters) const
{
    const Level& L = *lev[d];
    // levels with coarse-fine boundaries qualify when their layout allows it (Level::cf_fusable)
    return prm.relaxMode == RELAX_LEVEL_GSRB && !unswept(d) && L.valid_cells_global >= tune_.fused_min_cells && iters > 0 &&
           (L.ncf == 0 || L.cf_fusable) && L.active[2] && !(tune_.no_cf_fused && L.ncf > 0) && !full_;  // Dirichlet sides: ghosts synthesized in the kernel
}

// ------------------------------------------------------------------------------------
// The fold path of the cycle on fields of type T: double, or float on the fp32 depths of the mixed cycle.  The element type
// shows in pingpong / metric (below), diri_homog / cf_fill (solver.h) and the launchers' overloads, nowhere else.
// ------------------------------------------------------------------------------------
template <> double* PressureSolver::pingpong<double>(int d) const { return f_pp[d]; }
template <> float* PressureSolver::pingpong<float>(int d) const { return f32_[d].pp; }
template <> MetricPtrs<double> PressureSolver::metric<double>(int d) const { return metric_ptrs(lev[d]->dev); }
template <> MetricPtrs<float> PressureSolver::metric<float>(int d) const
{
    const Depth32& z = f32_[d];
    return MetricPtrs<float>{{z.jg[0], z.jg[1], z.jg[2]}, z.jinv};
}

// LevelGSRB::relax (GSRB.cpp:58-98) as ONE fused red+black launch per sweep (gsrb_fused.hip):
// same values bit for bit, one ghost exchange per sweep instead of two, ping-pong buffers.
template <class T>
void PressureSolver::fused_sweeps(int d, T* e, const T* res, int iters, bool e_zero, const double* e_shift,
                                  const Level* e_plus_level, const T* e_plus)
{
    Level& L = *lev[d];
    if (e_zero && tune_.no_zero_start) {   // A/B switch: the fused sweep gets its zeros from a memset, not from in_mode 1
        launch_set(st_, e, L.field_elems, T(0));
        e_zero = false;
    }
    xchg(L, const_cast<T*>(res));  // rhs ghosts: constant over the sweeps
    T* cur = e;
    T* alt = pingpong<T>(d);
    for (int it = 0; it < iters; ++it) {
        const bool zin = e_zero && it == 0;  // zeros need neither an exchange nor a read
        int mode = 0;
        if (zin) mode = 1;
        else if (it == 0 && e_plus) mode = e_shift ? 4 : 3;
        else if (it == 0 && e_shift) mode = 2;
        auto sweep = [&](TileSpan tl) {
            launch_gsrb_fused(st_, tl, L.dev, metric<T>(d), alt, cur, res, mode, e_shift,
                              e_plus_level ? &e_plus_level->dev : nullptr, e_plus, L.mgCrseRefRatio);
        };
        if (!zin && fused_overlap(L)) {
            // the sweep's one exchange in flight on the second stream while the tiles that read none of its cells are swept
            // (the CF ghosts are other cells, computed from this rank's valid cells: filled before the first tiles run)
            cf_fill(L, cur, true);
            overlapped(L, cur, L.ftiles, sweep);
        } else {
            if (!zin) {
                xchg(L, cur);
                cf_fill(L, cur, true);  // CF ghosts (faces + the edge ghosts the red ring reads), pre-sweep values
            }
            ProfScope timed(*this, d, 0);
            sweep(L.ftiles.all.span());
        }
        std::swap(cur, alt);
    }
    if (cur != e) launch_copy(st_, e, cur, L.field_elems);
}

// restrictResidual on a large level: residual and J-weighted average in one marching pass, the fine residual is never
// stored; with the fine half of the folded prolongation's mean
template <class T>
void PressureSolver::march_restrict(int d, T* resCoarse, T* phiFine, const T* rhsFine)
{
    Level& F = *lev[d];
    cf_fill(F, phiFine, false);
    const bool want = F.zeroAvg && !ordered(d);  // the fine half of the folded prolongation's mean
    auto pass = [&](TileSpan tl) {
        launch_resid_restrict(st_, tl, F.dev, metric<T>(d), lev[d + 1]->dev, resCoarse, phiFine, rhsFine, F.mgCrseRefRatio,
                              F.dxProduct, want ? d_partials : nullptr);
    };
    const bool overlap = resid_overlap(F);  // (never with Dirichlet sides, never in a profiled pass)
    if (!overlap) {
        xchg(F, phiFine);
        if (diri_) diri_homog(d, phiFine);  // homogeneous Dirichlet ghosts, as residual() fills them
    }
    ProfScope timed(*this, d, 1);
    if (overlap) overlapped(F, phiFine, F.rtiles, pass);
    else pass(F.rtiles.all.span());
    if (want) launch_sum_partials(st_, d_partials, F.rtiles.all.size(), d_fold + 8 * d);
    sf_valid_[d] = want ? 1 : 0;
}

// Large level: neither the prolongation nor the zero-average mean removal gets a pass of its own -- the first
// post-smoothing sweep reads corr + coarse(i/r) - mean.  mean = (S_f + S_c) / V with S_f = sum dvol * corr
// (gathered by the fused restriction), S_c = sum over coarse cells of coarse * (volume of its children), V the
// level's volume: the same number as ZeroAvgConstInterpPS's sum dvol * (corr + coarse) / sum dvol up to the
// association of the (already tree-ordered) sum.  The sums are fp64 whatever T is.
template <class T>
void PressureSolver::fold_up(int d, T* corr, const T* res, T* crse, bool exchange_crse)
{
    Level& F = *lev[d];
    Level& C = *lev[d + 1];
    if (exchange_crse) xchg(C, crse);
    const double* shift = nullptr;
    if (F.zeroAvg) {
        double* s = d_fold + 8 * d;
        launch_reduce(st_, C.dev, crse, f_W[d + 1], 0, d_partials, s + 1);
        comm_->allreduce(s, 2, 0, st_);  // (S_f, S_c) over the ranks
        launch_combine_sums(st_, s + 3, s, s + 1, s + 2);
        shift = s + 3;
    }
    fused_sweeps(d, corr, res, prm.num_smooth_up, false, shift, &C, crse);
}

void PressureSolver::relax(int d, double* e, const double* res, int iters, bool e_zero, const double* e_shift,
                           const Level* e_plus_level, const double* e_plus)
{
    Level& L = *lev[d];
    const bool fused_path = fused_relax(d, iters);
    SOMAR_CHECK((!e_shift && !e_plus) || fused_path, "deferred mean removal / folded prolongation need the fused sweep");
    if (fused_path) {
        fused_sweeps(d, e, res, iters, e_zero, e_shift, e_plus_level, e_plus);
        return;
    }
    if (e_zero) launch_set(st_, e, L.field_elems, 0.0);
    if (unswept(d)) return;   // a domain two cells wide in two directions: the reference's sweep has no cell to visit
    if (prm.relaxMode == RELAX_LEVEL_GSRB && full_march(d) && fused19(d)) {
        // LevelGSRB::relax with a non-diagonal metric on a level of large boxes: red everywhere and black three layers inside
        // every box in ONE marching launch (full19_fused.hip), the between-colour ghost work on its output exactly as in the
        // two-pass form below, then the black cells of the outer layers in place (k_full_march<3>).  Same values, same bits.
        double* cur = e;
        double* alt = f_pp[d];
        for (int it = 0; it < iters; ++it) {
            L.cf_homog(cur, st_);
            xchg(L, cur);
            run_full_program_frames(d, 1, cur);
            copy_frames(d, cur, alt);
            {
                ProfScope timed(*this, d, 0);
                launch_full_fused(st_, L.gtiles.span(), L.dev, alt, cur, f_psi[d], res);
            }
            L.cf_homog(alt, st_);
            xchg(L, alt);
            run_full_program_frames(d, 1, alt);
            {
                ProfScope timed(*this, d, 0);   // (slot 0 then holds two launches per sweep, as in the two-pass form)
                launch_gsrb_full_shell(st_, L.stiles.span(), L.dev, alt, cur, f_psi[d], res);
            }
            ++counters[4];
            std::swap(cur, alt);
        }
        if (cur != e) launch_copy(st_, e, cur, L.field_elems);
        return;
    }
    if (prm.relaxMode == RELAX_LEVEL_GSRB && full_march(d)) {
        // LevelGSRB::relax with a non-diagonal metric on a large level: per colour the same exchange / CF fill / ghost
        // program, then ONE marching pass (full19_march.hip) that reads the pre-pass values everywhere (the snapshot
        // semantics of the reference's `extrap`) and writes the other buffer.
        double* cur = e;
        double* alt = f_pp[d];
        for (int it = 0; it < iters; ++it)
            for (int pass = 0; pass < 2; ++pass) {
                L.cf_homog(cur, st_);
                xchg(L, cur);
                run_full_program_frames(d, 1, cur);
                // the pass rewrites the valid cells only; the ghost frame travels with them (edge / vertex ghosts at
                // coarse-fine corners keep whatever the last ExtrapolateCFEV left there, as in the reference's in-place sweep)
                copy_frames(d, cur, alt);
                ProfScope timed(*this, d, 0);
                launch_gsrb_full_march(st_, L.qtiles.span(), L.dev, alt, cur, f_psi[d], res, pass);
                std::swap(cur, alt);
            }
        // an even number of passes: the result is back in e
        return;
    }
    for (int it = 0; it < iters; ++it) {
        if (prm.relaxMode == RELAX_LEVEL_GSRB) {
            // LevelGSRB::relax, GSRB.cpp:58-98.  The Neumann ghost fill of
            // fillGhostsAndExtrapolate is dead code for a diagonal metric (the boundary
            // stencil never reads a Neumann ghost), so only the exchange remains.
            for (int pass = 0; pass < 2; ++pass) {
                // pull exchange: the colour pass refreshes the ghosts it reads itself (coarse-fine and Dirichlet ghosts are
                // other cells, computed from valid cells only: their order against the exchange does not matter)
                const bool pull = !full_ && L.pull_ready();
                L.cf_homog(e, st_);  // homogeneousCFInterp (Relaxer::fillGhostsAndExtrapolate)
                if (!pull) xchg(L, e);
                if (diri_ && !full_) apply_diri(d, e, true);  // ... and its physical ghosts (doBCs); non-diagonal: in the program
                if (full_) run_full_program(d, 1, e);  // psi snapshot + extrapolation (order 1) + Neumann ghosts
                ProfScope timed(*this, d, 0);
                if (full_) launch_gsrb_full(st_, L.dev, e, f_psi[d], res, pass);
                else launch_gsrb_ortho(st_, L.dev, e, res, pass, 0, pull);
            }
        } else if (prm.relaxMode == RELAX_LOOSE_GSRB) {
            // LooseGSRB::relax, GSRB.cpp:104-141: ONE exchange per sweep; red+black on the cells strictly inside
            // each box, then red+black on the box shells.  (The exchange "begun" before the interior phase only
            // carries shell cells, which that phase does not touch: completing it first changes nothing.)
            L.cf_homog(e, st_);
            xchg(L, e);
            if (diri_) apply_diri(d, e, true);
            launch_gsrb_ortho(st_, L.dev, e, res, 0, 1);
            launch_gsrb_ortho(st_, L.dev, e, res, 1, 1);
            launch_gsrb_ortho(st_, L.dev, e, res, 0, 2);
            launch_gsrb_ortho(st_, L.dev, e, res, 1, 2);
        } else if (prm.relaxMode == RELAX_LINE_GSRB) {
            line_relax(d, e, res);
        } else {
            // Jacobi::relax, Jacobi.cpp:54-90
            residual(d, f_scratch[d], e, res);
            launch_diag(st_, L.dev, e, f_scratch[d], 1);
        }
    }
}

// LineGSRB::relax, GSRB.cpp:148-330: per colour exchange, then every (i,j) column of that colour is solved
// exactly in z (line_gsrb.hip); f_pp[d] receives dgtsv's modified diagonal.
void PressureSolver::line_relax(int d, double* e, const double* res)
{
    Level& L = *lev[d];
    for (int pass = 0; pass < 2; ++pass) {
        xchg(L, e);
        L.cf_homog(e, st_);  // fillGhostsAndExtrapolate: homogeneous CF values in the lateral ghost cells
        if (diri_ && !full_) apply_diri(d, e, true);  // ... and the ghosts of lateral Dirichlet sides (the vertical ends are folded in)
        if (full_) run_full_program(d, 1, e);  // extrap copy (order 1) + physical ghosts: the cross terms are explicit
        if (prm.spaceDim == 2) {
            int maxN0 = 1;
            for (const PatchDesc& q : L.hpatches) maxN0 = std::max(maxN0, q.n[0]);
            launch_line_gsrb_2d(st_, L.dev, maxN0, e, res, f_pp[d], pass, full_ ? f_psi[d] : nullptr);
            continue;
        }
        launch_line_gsrb_ortho(st_, L.ctiles.span(), L.ctile_j, L.dev, e, res, f_pp[d], pass, full_ ? f_psi[d] : nullptr);
    }
}

void PressureSolver::residual(int d, double* out, double* phi, const double* rhs, bool homogeneous)
{
    lev[d]->cf_homog(phi, st_);  // interpCFGhosts(homogeneous), MappedAMRPoissonOp.cpp:628-640
    cf_ev(d, phi);
    residual_i(d, out, phi, rhs, homogeneous);
}

void PressureSolver::apply_op(int d, double* out, double* phi, bool homogeneous)
{
    lev[d]->cf_homog(phi, st_);
    cf_ev(d, phi);
    apply_op_i(d, out, phi, homogeneous);
}

void PressureSolver::operator_i(int d, int mode, double* out, double* phi, const double* rhs, bool homogeneous)
{
    Level& L = *lev[d];
    // small levels (direct-load operator): the kernel pulls the ghosts it reads, no copy launch
    const bool pull = !full_ && L.pull_ready() && !ortho_march(d);
    if (!pull) xchg(L, phi);  // exchangeComplete, MappedAMRPoissonOp.cpp:2222-2238
    if (diri_ && !full_) apply_diri(d, phi, homogeneous);  // m_bc.setGhosts, :822 (non-diagonal: inside the program)
    // face-valued Neumann sides (diagonal metric, depth 0): their ghosts with the Dirichlet ones, their boundary fluxes after
    // the launch below, which is the one of a solver without such sides
    const bool neum_faces = d == 0 && !homogeneous && neum_face_live();
    if (neum_faces) neum_face_ghosts(phi);
    ProfScope timed(*this, d, 1, mode == 0);
    if (full_march(d)) {
        run_full_program_frames(d, 0, phi, homogeneous);
        launch_full_march(st_, L.qtiles.span(), L.dev, out, phi, f_psi[d], rhs, mode);
    } else if (full_) {
        // exchangeComplete, fillExtrap (order 2), physical ghosts (Neumann with cross terms / Dirichlet), then the 19-point fluxes
        run_full_program(d, 0, phi, homogeneous);
        launch_op_full(st_, L.dev, out, phi, f_psi[d], rhs, mode);
    } else if (ortho_march(d)) launch_resid_march(st_, L.rtiles.all.span(), L.dev, out, phi, rhs, mode);  // Dirichlet sides: their ghosts were just written, the kernel only zeroes NEUMANN fluxes
    else launch_op_ortho(st_, L.dev, out, phi, rhs, mode, pull);
    if (neum_faces) neum_face_cells(mode, out, phi, rhs);
}

void PressureSolver::prolong_from(const LevelDev& C, const double* crse, const int r[3], double* fine)
{
    prolong_onto(0, C, crse, r, fine, false);
}

const double* PressureSolver::prolong_increment(int d, double* phiFine, const double* corrCoarse, bool defer_mean)
{
    return prolong_onto(d, lev[d + 1]->dev, corrCoarse, lev[d]->mgCrseRefRatio, phiFine, defer_mean);
}

const double* PressureSolver::prolong_onto(int d, const LevelDev& C, const double* crse, const int r[3], double* fine,
                                           bool defer_mean)
{
    // ConstInterpPS / ZeroAvgConstInterpPS, ProlongationStrategy.cpp:49-164.  The two scalar
    // MPI_Allreduce calls of the reference become one 2-element device-side reduction.
    Level& F = *lev[d];
    const bool os = F.zeroAvg && ord_sharded(d);
    launch_prolong(st_, F.dev, C, fine, crse, r, F.zeroAvg && !os, F.dxProduct, d_partials, d_scalars + SLOT_SUMS,
                   F.field_elems, ordered(d));
    if (!F.zeroAvg) return nullptr;
    if (os) ordered_sums(d, fine, F.dev.jinv, 6, F.dxProduct, d_scalars + SLOT_SUMS);
    else comm_->allreduce(d_scalars + SLOT_SUMS, 2, 0, st_);
    if (defer_mean) return d_scalars + SLOT_SUMS;
    launch_sub_mean(st_, fine, F.field_elems, d_scalars + SLOT_SUMS);
    return nullptr;
}

double* PressureSolver::amr_field(int which)
{
    SOMAR_CHECK(which == 0 || which == 1, "bad AMR work field");
    if (!f_amr[which]) f_amr[which] = lev[0]->alloc_field();
    return f_amr[which];
}

bool PressureSolver::residual_restrict_i(const LevelDev& C, double* crse, double* phi, const double* rhs, const int r[3])
{
    Level& F = *lev[0];
    for (int d = 0; d < 3; ++d)
        if (r[d] != 1 && r[d] != 2) return false;
    if (!ortho_march(0)) return false;
    xchg(F, phi);  // exchangeComplete, as residual_i
    if (diri_) apply_diri(0, phi, true);
    launch_resid_restrict(st_, F.rtiles.all.span(), F.dev, metric<double>(0), C, crse, phi, rhs, r, F.dxProduct, nullptr);
    return true;
}

void PressureSolver::restrict_residual(int d, double* resCoarse, double* phiFine, const double* rhsFine)
{
    // restrictResidual, MappedAMRPoissonOp.cpp:1281-1304
    if (ortho_march(d)) {
        march_restrict(d, resCoarse, phiFine, rhsFine);
        return;
    }
    residual(d, f_scratch[d], phiFine, rhsFine);
    launch_restrict(st_, lev[d + 1]->dev, lev[d]->dev, resCoarse, f_scratch[d], lev[d]->mgCrseRefRatio);
}

void PressureSolver::pre_cond(int d, double* phi, const double* rhs)
{
    // preCond, MappedAMRPoissonOp.cpp:684-734
    Level& L = *lev[d];
    if (prm.num_smooth_precond == 0 || prm.precondMode == PRECOND_NONE) {
        launch_copy(st_, phi, rhs, L.field_elems);
        return;
    }
    launch_diag(st_, L.dev, phi, rhs, 0);
    if (prm.precondMode == PRECOND_DIAG_LINE_RELAX && prm.relaxMode != RELAX_LINE_GSRB) {
        for (int it = 0; it < prm.num_smooth_precond; ++it) line_relax(d, phi, rhs);  // m_precondRelaxPtr = LineGSRB
        return;
    }
    relax(d, phi, rhs, prm.num_smooth_precond);
}

double PressureSolver::norm(int d, const double* a, int ord)
{
    Level& L = *lev[d];
    if (ord == 0) {
        if (fused_publish(d)) {
            const ScalarPublish P{h_scalars + SLOT_TMP, h_seq_, ++fetch_seq_};
            launch_reduce(st_, L.dev, a, nullptr, 1, d_partials, d_scalars + SLOT_TMP, false, &P);
            wait_published(P.seq);
            return h_scalars[SLOT_TMP];
        }
        launch_reduce(st_, L.dev, a, nullptr, 1, d_partials, d_scalars + SLOT_TMP);
        comm_->allreduce(d_scalars + SLOT_TMP, 1, 1, st_);
        return fetch_scalar(SLOT_TMP);
    }
    if (ord == 1) {
        if (fused_publish(d)) return reduce_fetch(d, a, nullptr, 2);
        reduce_sum(d, a, nullptr, 2, d_scalars + SLOT_TMP);
        return fetch_scalar(SLOT_TMP);
    }
    SOMAR_CHECK(ord == 2, "norm order must be 0, 1 or 2");
    if (fused_publish(d)) return std::sqrt(reduce_fetch(d, a, a, 0));
    reduce_sum(d, a, a, 0, d_scalars + SLOT_TMP);
    return std::sqrt(fetch_scalar(SLOT_TMP));
}

// single-rank, polling fetch: the reduction's last kernel publishes its result itself (one launch less per scalar)
bool PressureSolver::fused_publish(int d) const
{
    return tune_.poll_fetch && !tune_.no_fused_publish && !capturing_ && comm_->size == 1 && !ord_sharded(d);
}

double PressureSolver::reduce_fetch(int d, const double* a, const double* b, int mode)
{
    const ScalarPublish P{h_scalars + SLOT_TMP, h_seq_, ++fetch_seq_};
    launch_reduce(st_, lev[d]->dev, a, b, mode, d_partials, d_scalars + SLOT_TMP, ordered(d), &P);
    wait_published(P.seq);
    return h_scalars[SLOT_TMP];
}

double PressureSolver::dot(int d, const double* a, const double* b)
{
    if (fused_publish(d)) return reduce_fetch(d, a, b, 0);
    reduce_sum(d, a, b, 0, d_scalars + SLOT_TMP);
    return fetch_scalar(SLOT_TMP);
}

void PressureSolver::reduce_sum(int d, const double* a, const double* b, int mode, double* out)
{
    if (ord_sharded(d)) {
        ordered_sums(d, a, b, mode, 0.0, out);
        return;
    }
    launch_reduce(st_, lev[d]->dev, a, b, mode, d_partials, out, ordered(d));
    comm_->allreduce(out, 1, 0, st_);
}

void PressureSolver::ordered_sums(int d, const double* a, const double* b, int mode, double dxProduct, double* out)
{
    Level& L = *lev[d];
    const int nb = (int)L.boxes.size();
    if ((int)d_ord_start_.size() <= d) { d_ord_start_.resize(lev.size()); d_box_start_.resize(lev.size()); }
    if (!d_box_start_[d]) {
        std::vector<long long> bs(nb + 1, 0), ls(std::max<size_t>(L.local.size(), 1), 0);
        for (int i = 0; i < nb; ++i) bs[i + 1] = bs[i] + L.boxes[i].numPts();
        for (size_t q = 0; q < L.local.size(); ++q) ls[q] = bs[L.local[q]];
        d_box_start_[d] = DevBuf<long long>::from(bs);
        d_ord_start_[d] = DevBuf<long long>::from(ls);   // (ls holds one entry at least: never a null table)
    }
    const long long n = L.valid_cells_global;
    if (!d_ordbuf_) d_ordbuf_ = DevBuf<double>((size_t)2 * tune_.ordered_reduce_max);
    const int nvec = mode == 6 ? 2 : 1;
    double *X = d_ordbuf_, *Y = d_ordbuf_ + n;
    launch_set(st_, X, nvec * n, 0.0);
    launch_ord_fill(st_, L.dev, d_ord_start_[d], a, b, mode, dxProduct, X, Y);
    comm_->allreduce(X, (int)(nvec * n), 0, st_);
    launch_reduce_ordered_flat(st_, nb, d_box_start_[d], X, Y, mode, out);
}

// f -= sum(f*J)/sum(J): the J-weighted mean removal the callers apply to make an all-Neumann/periodic
// right-hand side solvable (computeMappedSum + setZeroAvg, MappedChombo/computeMappedSum.cpp)
void PressureSolver::remove_mean(int d, double* f)
{
    Level& L = *lev[d];
    launch_reduce(st_, L.dev, f, L.dev.jinv, 4, d_partials, d_scalars + SLOT_SUMS);
    launch_reduce(st_, L.dev, f, L.dev.jinv, 5, d_partials, d_scalars + SLOT_SUMS + 1);
    comm_->allreduce(d_scalars + SLOT_SUMS, 2, 0, st_);
    launch_sub_mean(st_, f, L.field_elems, d_scalars + SLOT_SUMS);
}

// ------------------------------------------------------------------------------------
// MAC level projection: BaseProjector<FluxBox>::project (projection/BaseProjectorI.H:176-299) with
// LevelMACProjector::computeDiv/computeGrad/applyCorrection (LevelMACProjector.cpp:156-241), velocity in
// flux form (a_velIsFlux = true).  Boundary-face values of the velocity are taken as given.
// ------------------------------------------------------------------------------------
double* PressureSolver::vel(int dir)
{
    SOMAR_CHECK(dir >= 0 && dir < 3 && finalized, "bad velocity direction / solver not finalized");
    if (!f_vel[dir]) f_vel[dir] = lev[0]->alloc_field();
    return f_vel[dir];
}

void PressureSolver::divergence_mac(double* out, double dt)
{
    launch_div_mac(st_, lev[0]->dev, out, vel(0), vel(1), vel(2), dt);
}

void PressureSolver::mac_correct(double* phi, double dt)
{
    Level& L = *lev[0];
    xchg(L, phi);  // Copier excp(grids, grids, domain, ghost, true); a_phi.exchange(excp)  (Gradient.cpp:118-121)
    double* v[3] = {vel(0), vel(1), prm.spaceDim == 3 ? vel(2) : nullptr};
    if (full_) {
        // singleBoxMacGrad with a non-diagonal metric (Gradient.cpp:946-1101): extrap from the exchanged phi first, then
        // the extrapolation BC on phi's own physical ghosts, then MAPPEDMACGRAD == MAPPEDGETFLUX(beta = 1) on every face
        mac_grad_full(phi);
        launch_face_axpy(st_, L.dev, v, f_flux, dt == 0.0 ? -1.0 : -dt);
        return;
    }
    launch_mac_correct(st_, L.dev, v, phi, dt == 0.0 ? -1.0 : -dt);
}

void PressureSolver::scale_vel(int centring, int which)
{
    Level& L = *lev[0];
    SOMAR_CHECK(which == 0 || which == 1, "which: 0 = J, 1 = Jinv");
    if (centring == 1) {
        SOMAR_CHECK(f_sc_cc[which], "the cell-centred J / Jinv has not been set (somar_solver_set_cc_j)");
        for (int c = 0; c < prm.spaceDim; ++c) launch_mul(st_, cc_vel(c), f_sc_cc[which], L.field_elems);
    } else {
        for (int d = 0; d < prm.spaceDim; ++d) {
            SOMAR_CHECK(f_sc_face[which][d], "the face-centred J / Jinv has not been set (somar_solver_set_face_j)");
            launch_mul(st_, vel(d), f_sc_face[which][d], L.field_elems);
        }
    }
}

void PressureSolver::alloc_flux(int ndir)
{
    for (int a = 0; a < ndir; ++a) {
        if (!flux_own_[a]) flux_own_[a] = lev[0]->alloc_field();
        f_flux[a] = flux_own_[a];
    }
}

double* const* PressureSolver::mac_grad(double* phi)
{
    Level& L = *lev[0];
    if (full_) {
        mac_grad_full(phi);
        return f_flux;
    }
    alloc_flux(3);
    // G = 0 + 1.0 * (dxinv * Jg * dphi): k_mac_correct's own expression, stored instead of subtracted (exact)
    double* g[3] = {f_flux[0], f_flux[1], prm.spaceDim == 3 ? f_flux[2] : nullptr};
    for (int a = 0; a < prm.spaceDim; ++a) launch_set(st_, f_flux[a], L.field_elems, 0.0);
    launch_mac_correct(st_, L.dev, g, phi, 1.0);
    return f_flux;
}

// uStarFuncBC without inflow / outflow sides on the face-centred velocity (LevelMACProjector::computeDiv hands &m_divBC to
// levelDivergenceMAC, Divergence.cpp:73-100, which overwrites the caller's boundary faces): solid walls, zero normal flux
void PressureSolver::vel_wall_bc()
{
    double* e[3] = {vel(0), vel(1), prm.spaceDim == 3 ? vel(2) : nullptr};
    if (velbc_default_) launch_face_wall(st_, lev[0]->dev, e);
    else launch_face_bc(st_, lev[0]->dev, e, velbc_kind_, velbc_value_);
}

// BasicVelocityBCGhostClass's inflow / outflow sides (EllipticBCUtils.cpp:1244-1327): what vel_wall_bc and the
// cell-centred divergence's face BC apply from now on
void PressureSolver::set_vel_bc(const int kind[6], const double value[6])
{
    velbc_default_ = true;
    for (int i = 0; i < 6; ++i) {
        SOMAR_CHECK(kind[i] >= 0 && kind[i] <= 2, "velocity BC kind: 0 solid wall, 1 prescribed normal velocity, 2 outflow");
        velbc_kind_[i] = kind[i];
        velbc_value_[i] = kind[i] == 1 ? value[i] : 0.0;
        if (kind[i] != 0) velbc_default_ = false;
    }
}

void PressureSolver::mac_project(double dt, bool zeroPressure, bool forceHomogeneous, SolveStats& s)
{
    check_idle("mac_project");
    divergence_mac(f_rhs, dt);
    solve(zeroPressure, forceHomogeneous, s);
    mac_correct(f_phi, dt);
    sync();
}

// ------------------------------------------------------------------------------------
// Viscous / diffusive Helmholtz solves (single level).
//   MappedAMRPoissonOp::setAlphaAndBeta (MappedAMRPoissonOp.cpp:582-619) on every op of the hierarchy, as
//   MappedBaseLevelHeatSolver::resetSolverAlphaAndBeta does (MappedBaseLevelHeatSolver.cpp:257-270): alpha = a * aCoef,
//   beta = b * bCoef with aCoef / bCoef the alpha / beta the solver was created with.  The reference refills lapDiag with
//   the same values (it depends on neither coefficient) and keeps the prolongation strategy the factory's null-space
//   probe chose at construction; so does this.
// ------------------------------------------------------------------------------------
void PressureSolver::set_alpha_beta(double a, double b, bool amr_member_ok)
{
    SOMAR_CHECK(finalized, "set_alpha_beta before finalize");
    SOMAR_CHECK(!amr_member_ || amr_member_ok,
                "set_alpha_beta on a level of an AMR hierarchy goes through the hierarchy (somar_amr_set_alpha_beta)");
    // in: a component's own operator is in place (comp_set_op; the single-field heat_step of that component comes here): the
    // live pair is then that operator's, and the solver's own waits in its OpState
    CompOp* in = comp_op(op_in_place_);
    if (!coefs_saved_) {
        aCoef_ = in ? in->st.alpha : lev[0]->alpha;
        bCoef_ = in ? in->st.beta : lev[0]->beta;
        coefs_saved_ = true;
    }
    for (auto& L : lev) {
        L->alpha = a * (in ? in->alpha0 : aCoef_);
        L->beta = b * (in ? in->beta0 : bCoef_);
        L->refresh_params();
    }
    // every operator kept aside is scaled too, each like a separate solver created with its pair would be
    ab_scale_[0] = a;
    ab_scale_[1] = b;
    for (Component& c : comps_)
        if (c.op) {
            c.op->st.alpha = a * (c.op.get() == in ? aCoef_ : c.op->alpha0);
            c.op->st.beta = b * (c.op.get() == in ? bCoef_ : c.op->beta0);
        }
    drop_graphs();  // captured launches carry the old coefficients in their kernel arguments
    if (coarse_) coarse_->set_alpha_beta(a, b);
}

double* PressureSolver::heat_flux(int dir)
{
    SOMAR_CHECK(dir >= 0 && dir < prm.spaceDim && finalized, "bad direction / solver not finalized");
    if (!f_heatflux[dir]) f_heatflux[dir] = lev[0]->alloc_field();
    return f_heatflux[dir];
}

void PressureSolver::increment_heat_flux(double* phi, bool setToZero)
{
    Level& L = *lev[0];
    double* const* G = full_ ? flux_fields(phi) : mac_grad(phi);
    for (int d = 0; d < prm.spaceDim; ++d) {
        double* acc = heat_flux(d);
        if (setToZero) launch_set(st_, acc, L.field_elems, 0.0);
        launch_incr(st_, acc, G[d], 1.0, L.field_elems);   // thisFlux += tempFlux
    }
    // EllipticNeumBCFluxClass: the flux through a boundary face of a face-valued Neumann side is the plane's value itself,
    // whatever the stages of the step added up there
    if (neum_face_live()) {
        double* acc[3] = {heat_flux(0), heat_flux(1), prm.spaceDim == 3 ? heat_flux(2) : nullptr};
        launch_set_neum_faces(st_, L.dev, d_neum_ops_, n_neum_face_ops_, acc);
    }
}

double* PressureSolver::heat_field(int which)
{
    SOMAR_CHECK(which >= 0 && which < 3 && finalized, "bad heat field / solver not finalized");
    if (!f_heat[which]) f_heat[which] = lev[0]->alloc_field();
    return f_heat[which];
}

// MappedLevelBackwardEuler::updateSoln (AMRParabolic/MappedLevelBackwardEuler.cpp:52-158) and
// MappedLevelCrankNicolson::updateSoln (MappedLevelCrankNicolson.cpp:52-152) on one level, with applyHelm / solveHelm
// (MappedBaseLevelHeatSolver.cpp:154-255).  phiNew = F_PHI (initial guess unless zeroPhi), phiOld / src = heat fields.
//   BE: rhs = phiOld (the source term is commented out in the reference);   solve (aCoef I - dt bCoef L) phiNew = rhs
//   CN: rhs = dt src + (aCoef I + dt/2 bCoef L) phiOld [inhomogeneous BCs]; solve (aCoef I - dt/2 bCoef L) phiNew = rhs
//   TGA: (I - mu1 dt L)(I - mu2 dt L) phiNew = (I + mu3 dt L) phiOld + (I + mu4 dt L) dt src; stats are the last solve's
// Written once for one field and for every component (heat_step_multi): each(f) runs f with every component in turn in the
// place of the solver's own fields, solve(last) is solve or solve_multi (last: the step's final solve).  One dt and one
// set_alpha_beta serve all components (it scales every component's own pair), so the stages that set the coefficients run
// component after component between them.
void PressureSolver::heat_stages(int scheme, double dt, bool zeroPhi, const std::function<void(const std::function<void()>&)>& each,
                                 const std::function<void(bool)>& solve)
{
    const long long n = lev[0]->field_elems;
    if (scheme == 0) {
        each([&]() { launch_copy(st_, f_rhs, heat_field(0), n); });
        set_alpha_beta(1.0, -dt * 1.0);
    } else if (scheme == 1) {
        set_alpha_beta(1.0, 0.5 * dt);
        each([&]() {
            apply_op(0, f_scratch[0], heat_field(0), false);
            launch_copy(st_, f_rhs, heat_field(1), n);
            launch_scale(st_, f_rhs, dt, n);
            launch_incr(st_, f_rhs, f_scratch[0], 1.0, n);
        });
        set_alpha_beta(1.0, -dt * 0.5);
    } else {
        // MappedLevelTGA::updateSolnWithTimeIndependentOp, MappedLevelTGA.cpp:231-387
        const TGACoefficients c = tga_coefficients();
        // heat_field(2): srct, then phis (the caller's initial guess for both solves)
        each([&]() {
            launch_copy(st_, heat_field(2), heat_field(1), n);   // srct = dt * src
            launch_scale(st_, heat_field(2), dt, n);
        });
        set_alpha_beta(1.0, c.mu4 * dt);
        each([&]() { apply_op(0, f_rhs, heat_field(2), true); });   // rhst = (I + mu4 dt L) srct, homogeneous BCs
        set_alpha_beta(1.0, c.mu3 * dt);
        each([&]() {
            apply_op(0, f_scratch[0], heat_field(0), false);         // (I + mu3 dt L) phiOld with the inhomogeneous BCs
            launch_incr(st_, f_rhs, f_scratch[0], 1.0, n);
            if (!zeroPhi) launch_copy(st_, heat_field(2), f_phi, n);
        });
        set_alpha_beta(1.0, -dt * c.mu2);
        solve(false);                                                // (I - mu2 dt L) phi* = rhst
        each([&]() {
            launch_copy(st_, f_rhs, f_phi, n);                       // assign(rhst, phiNew)
            if (!zeroPhi) launch_copy(st_, f_phi, heat_field(2), n);
        });
        set_alpha_beta(1.0, -dt * c.mu1);                            // (I - mu1 dt L) phiNew = phi*
    }
    solve(true);
}

void PressureSolver::heat_step(int scheme, double dt, bool zeroPhi, SolveStats& s)
{
    check_idle("heat_step");
    SOMAR_CHECK(scheme >= 0 && scheme <= 2, "heat scheme: 0 backward Euler, 1 Crank-Nicolson, 2 TGA");
    SOMAR_CHECK(dt >= 0.0, "negative time step");
    heat_stages(scheme, dt, zeroPhi, [](const std::function<void()>& f) { f(); }, [&](bool) { solve(zeroPhi, false, s); });
    sync();
}

// ------------------------------------------------------------------------------------
// Cell-centred level projection: BaseProjector<FArrayBox>::project (projection/BaseProjectorI.H:176-299) with
// LevelCCProjector::computeDiv/computeGrad/applyCorrection (LevelCCProjector.cpp:163-255), velocity in flux form.
// The velocity's ghost layer is the caller's (the reference does not exchange it before CellToEdge either).
// ------------------------------------------------------------------------------------
double* PressureSolver::cc_vel(int comp)
{
    SOMAR_CHECK(comp >= 0 && comp < prm.spaceDim && finalized, "bad velocity component / solver not finalized");
    if (!f_ccvel[comp]) f_ccvel[comp] = lev[0]->alloc_field();
    return f_ccvel[comp];
}

void PressureSolver::divergence_cc(double* out, double dt, bool wall)
{
    double* e[3] = {vel(0), vel(1), vel(2)};
    double* c[3] = {cc_vel(0), cc_vel(1), prm.spaceDim == 3 ? cc_vel(2) : nullptr};
    launch_cell_to_edge(st_, lev[0]->dev, e, c, wall && velbc_default_);  // Divergence::levelDivergenceCC, Divergence.cpp:361-396
    if (wall && !velbc_default_) {
        double* eb[3] = {e[0], e[1], prm.spaceDim == 3 ? e[2] : nullptr};
        launch_face_bc(st_, lev[0]->dev, eb, velbc_kind_, velbc_value_);
    }
    divergence_mac(out, dt);
}

void PressureSolver::cc_correct(double* phi, double dt)
{
    Level& L = *lev[0];
    xchg(L, phi);
    double* c[3] = {cc_vel(0), cc_vel(1), prm.spaceDim == 3 ? cc_vel(2) : nullptr};
    const double dtScale = dt == 0.0 ? -1.0 : -dt;
    if (full_) {
        mac_grad_full(phi);  // singleBoxMacGrad's sequence, as in mac_correct
        launch_edge_to_cell_axpy(st_, L.dev, c, f_flux, dtScale);
        return;
    }
    launch_cc_correct(st_, L.dev, c, phi, dtScale);
}

void PressureSolver::cc_project(double dt, bool zeroPressure, bool forceHomogeneous, bool wall, SolveStats& s)
{
    check_idle("cc_project");
    divergence_cc(f_rhs, dt, wall);
    solve(zeroPressure, forceHomogeneous, s);
    cc_correct(f_phi, dt);
    sync();
}

void PressureSolver::fill_hash(int d, double* f, unsigned long long seed)
{
    launch_fill_hash(st_, lev[d]->dev, f, seed);
}

// ------------------------------------------------------------------------------------
// MappedMultiGrid::cycle, MappedMultiGrid.H:555-653 (V/W cycles; F-cycle not offered)
// ------------------------------------------------------------------------------------
void PressureSolver::vcycle(double* e, const double* res, bool e_zero)
{
    check_idle("vcycle");
    if (mp_K_ > 0) {
        double rnorm = norm(0, res, 0);
        if (!e_zero) rnorm = std::max(rnorm, norm(0, e, 0));
        vcycle_mixed(e, res, rnorm, e_zero, false);
        return;
    }
    cycle(0, e, res, e_zero);
}

// corr_zero: the correction is to be taken as zero whatever the array holds (the reference zeroes it with
// setToZero right before: MappedMultiGrid.H:589, MappedAMRMultiGrid.H:1203); a smoother that knows this skips the
// memset and the read.  Only honoured when at least one smoothing sweep will overwrite the whole array.
void PressureSolver::cycle_bottom_relax(double* corr, const double* res, bool corr_zero)
{
    const int d = (int)lev.size() - 1;
    if (lev[d]->domain.numPts() == 1) {
        relax(d, corr, res, 1, corr_zero);
        return;
    }
    if (corr_zero && prm.num_smooth_bottom == 0) launch_set(st_, corr, lev[d]->field_elems, 0.0);
    relax(d, corr, res, prm.num_smooth_bottom, corr_zero && prm.num_smooth_bottom > 0);
}

void PressureSolver::cycle_down(int d, double* corr, const double* res, bool corr_zero)
{
    if (corr_zero && prm.num_smooth_down == 0) launch_set(st_, corr, lev[d]->field_elems, 0.0);
    relax(d, corr, res, prm.num_smooth_down, corr_zero && prm.num_smooth_down > 0);
    restrict_residual(d, f_res[d + 1], corr, res);
}

void PressureSolver::cycle_up(int d, double* corr, const double* res)
{
    if (fold_prolong(d)) {
        fold_up(d, corr, res, f_corr[d + 1].get(), true);
        return;
    }
    // the zero-average mean is folded into the first post-smoothing sweep when that sweep is the fused kernel
    const double* shift = prolong_increment(d, corr, f_corr[d + 1], fused_relax(d, prm.num_smooth_up));
    relax(d, corr, res, prm.num_smooth_up, false, shift);
}

void PressureSolver::cycle(int d, double* corr, const double* res, bool corr_zero)
{
    if (coarse_ && d == agglom_depth_) {
        agglom_cycle(corr, res, corr_zero);
        return;
    }
    const int D = (int)lev.size();
    if (mini_depth_ > 0 && d == mini_depth_ - 1) {
        // Bottom of a mini V-cycle: the reference smooths here (m_bottom sweeps) and then calls the AMR solver's
        // NoOpSolver, whose solve() is Chombo 3.1's "m_op->setToZero(a_phi)" -- so what goes back up is ZERO and the
        // sweeps are dead work.  Reproduced as the reference behaves (not as its name suggests): just the zero.
        (void)corr_zero;
        launch_set(st_, corr, lev[d]->field_elems, 0.0);
        return;
    }
    if (d == D - 1) {
        cycle_bottom_relax(corr, res, corr_zero);
        if (lev[d]->domain.numPts() != 1) bottom_solve(corr, res);
        return;
    }
    const int ncyc = cycle_override_ ? cycle_override_ : prm.numMG;
    SOMAR_CHECK(ncyc != 0, "numMG must not be 0");
    if (ncyc < 0) {
        // F-cycle (MappedMultiGrid.H:577-619): a recursive F-cycle first, pre-smoothing, then |numMG| V-cycles ("hack to
        // get a V-cycle": m_cycle = 1 around the inner call), post-smoothing.  No folding, no graphs: plain passes.
        const int cycles = -ncyc;
        Level& L = *lev[d];
        if (corr_zero) launch_set(st_, corr, L.field_elems, 0.0);
        restrict_residual(d, f_res[d + 1], corr, res);
        cycle(d + 1, f_corr[d + 1], f_res[d + 1], true);
        prolong_increment(d, corr, f_corr[d + 1]);
        relax(d, corr, res, prm.num_smooth_down);
        for (int img = 0; img < cycles; ++img) {
            restrict_residual(d, f_res[d + 1], corr, res);
            {
                ScopedSet<int> as_vcycle(cycle_override_, 1);
                cycle(d + 1, f_corr[d + 1], f_res[d + 1], true);
            }
            prolong_increment(d, corr, f_corr[d + 1]);
        }
        relax(d, corr, res, prm.num_smooth_up);
        return;
    }
    if (mini_depth_ == 0 && graph_cycle(d, corr, res, corr_zero)) return;
    cycle_down(d, corr, res, corr_zero);
    for (int img = 0; img < ncyc; ++img) cycle(d + 1, f_corr[d + 1], f_res[d + 1], img == 0);
    cycle_up(d, corr, res);
}

// MappedAMRMultiGrid::relax on a level whose refinement ratio to the coarser AMR level has an entry > 2
// (MappedAMRMultiGrid.H:742-754): a V-cycle over the forced depths only, nothing solved at its bottom.
void PressureSolver::mini_vcycle(double* corr, const double* res)
{
    SOMAR_CHECK(!forcedRatios.empty() && (int)lev.size() > (int)forcedRatios.size(), "no forced MG depths on this level");
    SOMAR_CHECK(!coarse_ || agglom_depth_ > (int)forcedRatios.size(), "internal: forced depths inside the replicated tail");
    ScopedSet<int> limit(mini_depth_, (int)forcedRatios.size() + 1);
    cycle(0, corr, res, false);
}

void PressureSolver::set_bc_values(const double v[6])
{
    SOMAR_CHECK(!lev.empty() && !finalized, "set_bc_values before define / after finalize");
    for (int d = 0; d < 3; ++d)
        for (int s = 0; s < 2; ++s) bc_value_[d][s] = v[2 * d + s];
}

// one GHOST_DIRI op per (patch, Dirichlet side it touches): the face-adjacent ghost layer, setSideDiriBC's destBox
void PressureSolver::build_diri_ops(int d)
{
    std::vector<GhostOp> ops = make_diri_ops(d, lev[d]->bc_type, bc_value_, true);
    if (d == 0) h_diri_ops0_ = ops;
    n_diri_ops_[d] = (int)ops.size();
    d_diri_ops_[d] = DevBuf<GhostOp>::from(ops);
}

// sides_of_solver: bc / val are the solver's own sides, which at depth 0 may be face-valued (set_diri_op); a component's
// operator (comp_set_op) has constants only
std::vector<GhostOp> PressureSolver::make_diri_ops(int d, const int bc[3][2], const double val[3][2], bool sides_of_solver) const
{
    const Level& L = *lev[d];
    std::vector<GhostOp> ops;
    for (int pi = 0; pi < L.npatches(); ++pi) {
        const IBox valid = L.boxes[L.local[pi]];
        for (int a = 0; a < 3; ++a) {
            if (!L.active[a] || L.periodic[a]) continue;
            for (int s = 0; s < 2; ++s) {
                if (bc[a][s] != BC_DIRI) continue;
                if ((s ? valid.hi[a] : valid.lo[a]) != (s ? L.domain.hi[a] : L.domain.lo[a])) continue;
                GhostOp op;
                std::memset(&op, 0, sizeof(op));
                op.patch = pi;
                op.type = GHOST_DIRI;
                for (int q = 0; q < 3; ++q) { op.lo[q] = 0; op.n[q] = valid.size(q); }
                op.lo[a] = s ? valid.size(a) : -1;
                op.n[a] = 1;
                op.dir = a;
                op.sgn = s ? 1 : -1;
                op.val = val[a][s];
                if (d == 0 && sides_of_solver) set_diri_op(op);
                ops.push_back(op);
            }
        }
    }
    return ops;
}

void PressureSolver::apply_diri(int d, double* phi, bool homogeneous)
{
    launch_ghost_ops(st_, lev[d]->dev, d_diri_ops_[d], n_diri_ops_[d], phi, phi, homogeneous);
}

void PressureSolver::set_bc_face_values(int dir, int side, const double* values)
{
    SOMAR_CHECK(!lev.empty(), "set_bc_face_values before define");
    SOMAR_CHECK(dir >= 0 && dir < 3 && (side == 0 || side == 1), "set_bc_face_values: dir must be 0..2, side 0 (low) or 1 (high)");
    const Level& L = *lev[0];
    SOMAR_CHECK(L.active[dir], "set_bc_face_values: direction " + std::to_string(dir) + " is inactive (space_dim 2)");
    SOMAR_CHECK(!L.periodic[dir], "set_bc_face_values: direction " + std::to_string(dir) + " is periodic");
    SOMAR_CHECK(L.bc_type[dir][side] == BC_DIRI, "set_bc_face_values: side (" + std::to_string(dir) + ", " +
                                                     std::to_string(side) + ") is not a Dirichlet side");
    const bool was = face_[dir][side];
    if (values) {
        const int t0 = (dir + 1) % 3 < (dir + 2) % 3 ? (dir + 1) % 3 : (dir + 2) % 3, t1 = 3 - dir - t0;
        const size_t n = (size_t)L.domain.size(t0) * L.domain.size(t1);
        face_plane_[dir][side].assign(values, values + n);
        face_[dir][side] = true;
    } else {
        face_plane_[dir][side].clear();
        face_[dir][side] = false;
    }
    if (!finalized) return;   // finalize builds the ops and the buffer from these
    sync();                   // nothing in flight reads the op lists or the values while they are rewritten
    if (was != face_[dir][side]) refresh_diri_ops();
    fill_face_values();
}

// One slice of d_bcface_ per (local patch of depth 0, Dirichlet side it touches), in patch order: the ghost layer over the
// patch's transverse extent, as build_diri_ops and build_program cover it.  Allocated once, whether or not a side is
// face-valued yet, so that a later set_bc_face_values only copies.  With a diagonal metric the Neumann sides have theirs too
// (set_neum_face_values).
void PressureSolver::build_face_slices()
{
    const Level& L = *lev[0];
    face_off_.assign((size_t)6 * L.npatches(), -1);
    long long total = 0;
    for (int pi = 0; pi < L.npatches(); ++pi) {
        const IBox valid = L.boxes[L.local[pi]];
        for (int a = 0; a < 3; ++a) {
            if (!L.active[a] || L.periodic[a]) continue;
            for (int s = 0; s < 2; ++s) {
                if (L.bc_type[a][s] != BC_DIRI && (L.bc_type[a][s] != BC_NEUM || full_)) continue;
                if ((s ? valid.hi[a] : valid.lo[a]) != (s ? L.domain.hi[a] : L.domain.lo[a])) continue;
                face_off_[6 * pi + 2 * a + s] = total;
                total += valid.numPts() / valid.size(a);
            }
        }
    }
    h_bcface_.assign((size_t)std::max(total, 1LL), 0.0);
    d_bcface_ = DevBuf<double>(h_bcface_.size());
    lev[0]->dev.bc_face = d_bcface_;
    fill_face_values();
}

// host mirror of every slice (face-valued sides from their planes, constant sides their constant -- zero on a Neumann side --
// which no op reads), then one copy into the device buffer
void PressureSolver::fill_face_values()
{
    const Level& L = *lev[0];
    for (int pi = 0; pi < L.npatches(); ++pi) {
        const IBox valid = L.boxes[L.local[pi]];
        for (int a = 0; a < 3; ++a)
            for (int s = 0; s < 2; ++s) {
                const long long off = face_off_[6 * pi + 2 * a + s];
                if (off < 0) continue;
                const int t0 = (a + 1) % 3 < (a + 2) % 3 ? (a + 1) % 3 : (a + 2) % 3, t1 = 3 - a - t0;
                const long long nt0 = L.domain.size(t0);
                // the op's loop order: i fastest over its region (extent 1 along a), i.e. t0 fastest, then t1
                long long q = off;
                for (int g1 = valid.lo[t1]; g1 <= valid.hi[t1]; ++g1)
                    for (int g0 = valid.lo[t0]; g0 <= valid.hi[t0]; ++g0, ++q)
                        h_bcface_[q] = face_[a][s] ? face_plane_[a][s][(g0 - L.domain.lo[t0]) + nt0 * (g1 - L.domain.lo[t1])]
                                                   : (L.bc_type[a][s] == BC_DIRI ? bc_value_[a][s] : 0.0);
            }
    }
    SOMAR_HIP(hipMemcpy(d_bcface_, h_bcface_.data(), h_bcface_.size() * sizeof(double), hipMemcpyHostToDevice));
}

// The slice of a physical-boundary op of depth 0.  The op must cover exactly the (patch, side) ghost layer its slice was laid
// out for, so that bcf[voff + loop index] stays inside the buffer -- checked here, on the host, for every op before any upload.
long long PressureSolver::face_slice_of(const GhostOp& op, const char* what) const
{
    const Level& L = *lev[0];
    const std::string w(what);
    SOMAR_CHECK(op.patch >= 0 && op.patch < L.npatches() && op.dir >= 0 && op.dir < 3 && (op.sgn == 1 || op.sgn == -1),
                w + " ghost op: bad patch / direction / side");
    const int a = op.dir, s = op.sgn > 0 ? 1 : 0;
    const IBox valid = L.boxes[L.local[op.patch]];
    for (int q = 0; q < 3; ++q) {
        const int lo = q == a ? (s ? valid.size(a) : -1) : 0, n = q == a ? 1 : valid.size(q);
        SOMAR_CHECK(op.lo[q] == lo && op.n[q] == n, w + " ghost op does not cover its patch's ghost layer");
    }
    const long long off = face_off_.at((size_t)6 * op.patch + 2 * a + s);
    const long long cells = (long long)op.n[0] * op.n[1] * op.n[2];
    SOMAR_CHECK(off >= 0 && off + cells <= (long long)h_bcface_.size(), w + " ghost op: face-value slice out of range");
    return off;
}

// A Dirichlet op of depth 0 as its side now is: GHOST_DIRI with the side's constant, or GHOST_DIRI_FACE reading its slice.
void PressureSolver::set_diri_op(GhostOp& op) const
{
    const long long off = face_slice_of(op, "Dirichlet");
    const int a = op.dir, s = op.sgn > 0 ? 1 : 0;
    if (face_[a][s]) {
        op.type = GHOST_DIRI_FACE;
        op.voff = off;
    } else {
        op.type = GHOST_DIRI;
        op.val = bc_value_[a][s];
    }
}

// after finalize: the Dirichlet ops of depth 0 rewritten in place (same lists, same lengths, same device addresses)
void PressureSolver::refresh_diri_ops()
{
    auto fix = [&](std::vector<GhostOp>& v, GhostOp* dev) {
        bool any = false;
        for (GhostOp& op : v)
            if (ghost_is_diri(op.type)) { set_diri_op(op); any = true; }
        if (any) {
            SOMAR_CHECK(dev != nullptr, "Dirichlet ghost ops without a device list");
            SOMAR_HIP(hipMemcpy(dev, v.data(), v.size() * sizeof(GhostOp), hipMemcpyHostToDevice));
        }
    };
    if (!d_diri_ops_.empty()) fix(h_diri_ops0_, d_diri_ops_[0]);
    if (full_ && !full_prog_.empty())
        for (FullProgram& P : full_prog_[0]) {
            fix(P.h_ops, P.d_ops);
            fix(P.h_box_ops, P.d_box_ops);
        }
}

// ------------------------------------------------------------------------------------
// Position-dependent Neumann values on a diagonal metric (EllipticNeumBCGhostClass / EllipticNeumBCFluxClass,
// BCInterface/EllipticBCUtils.cpp:696-947).  Everything but the inhomogeneous operator of depth 0 sees zero, i.e. the folded
// "no ghost, no flux" face of StencilParams::neum, and launches what it launched before.
// ------------------------------------------------------------------------------------
void PressureSolver::refuse_full_with_neum_faces(const char* who) const
{
    SOMAR_CHECK(!has_neum_face_values(), std::string(who) + ": this solver has position-dependent Neumann values "
                    "(somar_solver_set_neum_face_values), which are defined for a diagonal metric only");
}

void PressureSolver::set_neum_face_values(int dir, int side, const double* values)
{
    SOMAR_CHECK(!lev.empty(), "set_neum_face_values before define");
    SOMAR_CHECK(dir >= 0 && dir < 3 && (side == 0 || side == 1), "set_neum_face_values: dir must be 0..2, side 0 (low) or 1 (high)");
    SOMAR_CHECK(op_in_place_ == 0, "internal: set_neum_face_values while a component's operator is in place");
    const Level& L = *lev[0];
    SOMAR_CHECK(L.active[dir], "set_neum_face_values: direction " + std::to_string(dir) + " is inactive (space_dim 2)");
    SOMAR_CHECK(!L.periodic[dir], "set_neum_face_values: direction " + std::to_string(dir) + " is periodic");
    SOMAR_CHECK(L.bc_type[dir][side] == BC_NEUM, "set_neum_face_values: side (" + std::to_string(dir) + ", " +
                                                     std::to_string(side) + ") is not a Neumann side");
    SOMAR_CHECK(!full_, "set_neum_face_values: this solver has a non-diagonal metric; position-dependent Neumann values are "
                        "defined for a diagonal metric only (the reference's two Neumann ghost rules differ in the cross term)");
    const bool was = neum_face_[dir][side];
    if (values) {
        const int t0 = (dir + 1) % 3 < (dir + 2) % 3 ? (dir + 1) % 3 : (dir + 2) % 3, t1 = 3 - dir - t0;
        const size_t n = (size_t)L.domain.size(t0) * L.domain.size(t1);
        face_plane_[dir][side].assign(values, values + n);
    } else {
        face_plane_[dir][side].clear();
    }
    face_[dir][side] = neum_face_[dir][side] = values != nullptr;
    if (!finalized) return;   // finalize builds the ops and the buffers from these
    sync();                   // nothing in flight reads the op list or the values while they are rewritten
    if (was != neum_face_[dir][side]) refresh_neum_ops();
    fill_face_values();
}

// room for one op per (local patch of depth 0, physical Neumann side it touches), and the offset table, at their final sizes
void PressureSolver::build_neum_ops()
{
    const Level& L = *lev[0];
    h_neum_ops_.clear();
    h_neum_off_.assign((size_t)std::max(6 * L.npatches(), 1), -1);
    n_neum_face_ops_ = 0;
    if (full_) return;
    for (int pi = 0; pi < L.npatches(); ++pi)
        for (int a = 0; a < 3; ++a)
            for (int s = 0; s < 2; ++s)
                if (L.bc_type[a][s] == BC_NEUM && face_off_[6 * pi + 2 * a + s] >= 0) h_neum_ops_.push_back(GhostOp());
    if (h_neum_ops_.empty()) return;
    d_neum_ops_ = DevBuf<GhostOp>(h_neum_ops_.size());
    d_neum_off_ = DevBuf<long long>(h_neum_off_.size());
    refresh_neum_ops();
}

// the ops of the face-valued Neumann sides first (the rest of the list is never launched), each checked against its slice on
// the host; then one copy of the list and one of the offset table into the buffers build_neum_ops made
void PressureSolver::refresh_neum_ops()
{
    if (h_neum_ops_.empty()) return;   // no local patch touches a Neumann side (a rank of a sharded level)
    const Level& L = *lev[0];
    std::vector<GhostOp> ops;
    std::fill(h_neum_off_.begin(), h_neum_off_.end(), -1);
    for (int pi = 0; pi < L.npatches(); ++pi) {
        const IBox valid = L.boxes[L.local[pi]];
        for (int a = 0; a < 3; ++a)
            for (int s = 0; s < 2; ++s) {
                if (!neum_face_[a][s] || face_off_[6 * pi + 2 * a + s] < 0) continue;
                GhostOp op;
                std::memset(&op, 0, sizeof(op));
                op.patch = pi;
                op.type = GHOST_NEUM_FACE;
                for (int q = 0; q < 3; ++q) { op.lo[q] = 0; op.n[q] = valid.size(q); }
                op.lo[a] = s ? valid.size(a) : -1;
                op.n[a] = 1;
                op.dir = a;
                op.sgn = s ? 1 : -1;
                op.voff = face_slice_of(op, "Neumann");
                h_neum_off_[6 * pi + 2 * a + s] = op.voff;
                ops.push_back(op);
            }
    }
    SOMAR_CHECK(ops.size() <= h_neum_ops_.size(), "internal: more face-valued Neumann ops than the list has room for");
    n_neum_face_ops_ = (int)ops.size();
    GhostOp idle;   // behind the launched ones: an empty region
    std::memset(&idle, 0, sizeof(idle));
    idle.type = GHOST_COPY;
    ops.resize(h_neum_ops_.size(), idle);
    h_neum_ops_ = ops;
    SOMAR_HIP(hipMemcpy(d_neum_ops_, h_neum_ops_.data(), h_neum_ops_.size() * sizeof(GhostOp), hipMemcpyHostToDevice));
    SOMAR_HIP(hipMemcpy(d_neum_off_, h_neum_off_.data(), h_neum_off_.size() * sizeof(long long), hipMemcpyHostToDevice));
}

void PressureSolver::neum_face_ghosts(double* phi)
{
    launch_ghost_ops(st_, lev[0]->dev, d_neum_ops_, n_neum_face_ops_, phi, phi, false);
}

void PressureSolver::neum_face_cells(int mode, double* out, const double* phi, const double* rhs)
{
    launch_op_neum_face(st_, lev[0]->dev, d_neum_ops_, n_neum_face_ops_, d_neum_off_, out, phi, rhs, mode);
}

void PressureSolver::drop_graph(CoarseGraph& g)
{
    if (g.down) hipGraphExecDestroy(g.down);
    if (g.up) hipGraphExecDestroy(g.up);
    g = CoarseGraph();
}

// the graphs of the operator in place and of every operator kept aside (comp_set_op): one pair per operator
void PressureSolver::drop_graphs()
{
    drop_graph(cg_);
    for (Component& c : comps_)
        if (c.op) drop_graph(c.op->st.cg);
}

// The V-cycle from depth d down to the bottom and back as two graph replays around the bottom solve.  Returns
// false when this call is not the one the graphs describe (the caller then runs the launches one by one).
bool PressureSolver::graph_cycle(int d, double* corr, const double* res, bool corr_zero)
{
    const int D = (int)lev.size();
    if (graph_from_ < 0 || d != graph_from_ || capturing_ || !corr_zero || prm.numMG != 1 || comm_->size != 1 ||
        coarse_ || profiling_ || d > D - 2)
        return false;
    if (cg_.down && (cg_.d0 != d || cg_.corr != corr || cg_.res != res || cg_.pre != prm.num_smooth_down ||
                     cg_.post != prm.num_smooth_up || cg_.bottom != prm.num_smooth_bottom))
        drop_graph(cg_);   // (the operator in place alone: the graphs of the others describe other calls)
    if (!cg_.down) {
        auto capture = [&](bool down) -> hipGraphExec_t {
            hipGraph_t g = nullptr;
            capturing_ = true;
            SOMAR_HIP(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
            try {
                if (down) {
                    cycle_down(d, corr, res, true);
                    for (int q = d + 1; q <= D - 2; ++q) cycle_down(q, f_corr[q], f_res[q], true);
                    cycle_bottom_relax(f_corr[D - 1], f_res[D - 1], true);
                } else {
                    for (int q = D - 2; q > d; --q) cycle_up(q, f_corr[q], f_res[q]);
                    cycle_up(d, corr, res);
                }
            } catch (...) {
                hipStreamEndCapture(st_, &g);
                if (g) hipGraphDestroy(g);
                capturing_ = false;
                throw;
            }
            capturing_ = false;
            SOMAR_HIP(hipStreamEndCapture(st_, &g));
            hipGraphExec_t e = nullptr;
            const hipError_t rc = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
            hipGraphDestroy(g);
            SOMAR_HIP(rc);
            return e;
        };
        cg_.down = capture(true);
        cg_.up = capture(false);
        cg_.d0 = d;
        cg_.corr = corr;
        cg_.res = res;
        cg_.pre = prm.num_smooth_down;
        cg_.post = prm.num_smooth_up;
        cg_.bottom = prm.num_smooth_bottom;
    }
    SOMAR_HIP(hipGraphLaunch(cg_.down, st_));
    if (lev[D - 1]->domain.numPts() != 1) {
        // a one-launch bottom solve leaves its (iterations, exit code) pending until the up leg is in the queue
        bottom_defer_ = tune_.bottom_async != 0;
        try {
            bottom_solve(f_corr[D - 1], f_res[D - 1]);
        } catch (...) {
            bottom_defer_ = false;
            bottom_pending_ = 0;
            throw;
        }
        bottom_defer_ = false;
    }
    const hipError_t rc = hipGraphLaunch(cg_.up, st_);
    if (rc != hipSuccess) bottom_pending_ = 0;
    SOMAR_HIP(rc);
    bottom_collect();
    return true;
}

// ------------------------------------------------------------------------------------
// Opt-in mixed precision (NOT the reference's arithmetic).  solve() is a defect-correction loop: the cycle only has to
// produce an approximate correction of the fp64 residual, which the loop then measures in fp64 again.  Depths 0 .. K-1 run
// the fold path of the cycle (fused sweeps, residual + restriction in one pass, prolongation folded into the first
// post-smoothing sweep) on fp32 fields and fp32 copies of the metric: half the bytes of those HBM-bound kernels.  Depth K and
// below run the fp64 code unchanged (graph replay, bottom solver); at the seam the restricted residual is converted to fp64
// and depth K's correction back to fp32.  Sums (zero-average means, fold sums) read fp32 and accumulate in fp64.
// ------------------------------------------------------------------------------------
std::string PressureSolver::mixed_refusal() const
{
    if (amr_member_) return "a level of an AMR hierarchy (the composite cycle runs in fp64)";
    if (full_) return "a non-diagonal metric (19-point operator)";
    if (prm.relaxMode != RELAX_LEVEL_GSRB) return "a relax_mode other than LevelGSRB";
    if (prm.numMG != 1) return "num_mg != 1 (W- and F-cycles run plain passes, no folding)";
    if (hasCF_ || !forcedRatios.empty()) return "a level with coarse-fine boundaries";
    return "";
}

void PressureSolver::set_precision(int mode, long long min_cells)
{
    check_idle("set_precision");
    SOMAR_CHECK(mode == 0 || mode == 1, "set_precision: mode is 0 (fp64) or 1 (mixed: fp32 cycle on the large depths)");
    if (mode == 1) {
        const std::string why = mixed_refusal();
        SOMAR_CHECK(why.empty(), "set_precision: mixed precision is not available for " + why);
        SOMAR_CHECK(ncomp_ == 1, "set_precision: mixed precision is not available for a solver of more than one component "
                                 "(set_components: the fp32 cycle carries one field)");
    }
    mp_mode_ = mode;
    mp_min_cells_ = min_cells;
    if (finalized) mp_setup();
}

void PressureSolver::mp_free()
{
    if (f32_.empty()) return;
    if (st_) hipStreamSynchronize(st_);
    f32_.clear();
    mp_K_ = 0;
}

void PressureSolver::mp_setup()
{
    mp_free();
    drop_graphs();
    const bool no_fold = tune_.no_fold_prolong != 0;   // (fold_prolong's A/B switch)
    const long long minc = mp_min_cells_ > 0 ? mp_min_cells_ : tune_.fused_min_cells;
    // (sharded: lev.back() is the landing layout of the replicated tail, or a serial-order depth comes first -- both stay fp64)
    const int D = (int)lev.size();
    int K = 0;
    for (int d = 0; d + 1 < D && !no_fold && mp_mode_ == 1; ++d) {
        const Level& L = *lev[d];
        if (graph_from_ >= 0 && d >= graph_from_) break;   // the graph-replayed legs stay fp64
        if (!fused_relax(d, prm.num_smooth_down) || !fused_relax(d, prm.num_smooth_up)) break;
        if (L.valid_cells_global < minc || L.valid_cells_global < tune_.march_min_cells || ordered(d)) break;
        bool r12 = true;
        for (int q = 0; q < 3; ++q) r12 = r12 && (L.mgCrseRefRatio[q] == 1 || L.mgCrseRefRatio[q] == 2);
        if (!r12) break;
        K = d + 1;
    }
    if (comm_->size > 1) {
        // The mode and K decide the element type of every halo message of depths 0 .. K-1: a rank in fp32 talking to a rank in
        // fp64 would wait in the transport for a message of the other size.  min and max over the ranks in ONE max-allreduce.
        const double mine[3] = {(double)mp_mode_, (double)K, (double)(mp_mode_ == 1 ? minc : 0)};
        double v[6];
        for (int q = 0; q < 3; ++q) { v[q] = mine[q]; v[3 + q] = -mine[q]; }
        SOMAR_HIP(hipMemcpyAsync(d_scalars + SLOT_SUMS, v, sizeof(v), hipMemcpyHostToDevice, st_));
        comm_->allreduce(d_scalars + SLOT_SUMS, 6, 1, st_);
        SOMAR_HIP(hipMemcpyAsync(v, d_scalars + SLOT_SUMS, sizeof(v), hipMemcpyDeviceToHost, st_));
        SOMAR_HIP(hipStreamSynchronize(st_));
        bool same = true;
        for (int q = 0; q < 3; ++q) same = same && v[q] == -v[3 + q];
        if (!same) {
            mp_mode_ = 0;   // on every rank alike: the solver stays usable, in fp64
            mp_min_cells_ = 0;
            throw Error(-1, "set_precision is collective on a sharded solver: every rank must call it with the same mode and "
                            "min_cells and arrive at the same fp32 depths (mode " + std::to_string((int)-v[3]) + " .. " +
                            std::to_string((int)v[0]) + ", fp32 depths " + std::to_string((int)-v[4]) + " .. " +
                            std::to_string((int)v[1]) + ", min_cells " + std::to_string((long long)-v[5]) + " .. " +
                            std::to_string((long long)v[2]) + " over the ranks); the solver is back in mode 0");
        }
    }
    if (K == 0) return;
    f32_.resize(K + 1);   // (mp_free left it empty)
    for (int d = 0; d <= K; ++d) {
        const size_t n = (size_t)std::max(lev[d]->field_elems, 1LL);
        f32_[d].corr = DevBuf<float>::zeros(n);
        f32_[d].res = DevBuf<float>::zeros(n);
        if (d < K) f32_[d].pp = DevBuf<float>::zeros(n);
    }
    SOMAR_HIP(hipDeviceSynchronize());   // null-stream memsets vs the solver's non-blocking stream
    mp_K_ = K;
    mp_convert_metric();
    sync();
}

void PressureSolver::mp_convert_metric()
{
    for (int d = 0; d < mp_K_; ++d) {
        Level& L = *lev[d];
        Depth32& z = f32_[d];
        // no copy only where neither kernel reads the arrays: k_resid_march takes StencilParams::uc on every uniform depth, the
        // fused sweep only where its launcher picks the uniform-metric table (not with Dirichlet sides, not in the 8-row form)
        if (L.dev.P.uniform && fused_uniform_kernel(L.dev)) continue;
        const long long n = L.field_elems;
        for (int a = 0; a < 3; ++a)
            if (!z.jg[a]) z.jg[a] = DevBuf<float>((size_t)n);
        if (!z.jinv) z.jinv = DevBuf<float>((size_t)n);
        float* const dst[4] = {z.jg[0], z.jg[1], z.jg[2], z.jinv};
        const double* const src[4] = {L.dev.jg[0], L.dev.jg[1], L.dev.jg[2], L.dev.jinv};
        launch_convert(st_, dst, src, n);
    }
}

void PressureSolver::exchange_bytes(long long out2[2]) const
{
    out2[0] = out2[1] = 0;
    for (const auto& L : lev)
        for (int q = 0; q < 2; ++q) out2[q] += L->sent_bytes[q];
}

void PressureSolver::cycle32(int d, float* corr, const float* res, bool corr_zero)
{
    fused_sweeps<float>(d, corr, res, prm.num_smooth_down, corr_zero, nullptr, nullptr, nullptr);
    float* rc = f32_[d + 1].res;
    march_restrict(d, rc, corr, res);
    if (d + 1 < mp_K_) {
        cycle32(d + 1, f32_[d + 1].corr, rc, true);
    } else {
        // the seam: depth K runs the fp64 cycle on the converted residual; its exchanged correction comes back in fp32
        const int K = d + 1;
        const long long n = lev[K]->field_elems;
        launch_convert(st_, f_res[K], rc, n);
        cycle(K, f_corr[K], f_res[K], true);
        xchg(*lev[K], f_corr[K].get());
        launch_convert(st_, f32_[K].corr, f_corr[K], n);
    }
    fold_up(d, corr, res, f32_[d + 1].corr.get(), d + 1 < mp_K_);   // (the seam's correction was exchanged in fp64, above)
}

// e (fp64, depth 0) := the fp32 cycle's correction of res, or (add_to_phi) e += it.  rnorm: the max norm of res (and of an
// e that is not zero).  The cycle is linear, so it runs on res * s with s = 2^-ilogb(rnorm): the fp32 fields then hold values
// of order one whatever the scale of the problem (fp32 alone would flush corrections below 2^-149 to zero and overflow above
// 2^128), and every scaling is by a power of two, so it is exact and the mixed solve is as scale-equivariant as the fp64 one.
// The bottom solver of the fp64 seam compares its residual with bottom_metric in absolute terms: it is scaled alike.
void PressureSolver::vcycle_mixed(double* e, const double* res, double rnorm, bool e_zero, bool add_to_phi)
{
    const long long n = lev[0]->field_elems;
    if (rnorm == 0.0) {   // a zero residual (and correction): the correction is zero
        if (!add_to_phi && e_zero) launch_set(st_, e, n, 0.0);
        return;
    }
    const int ex = std::isfinite(rnorm) ? std::min(std::max(-std::ilogb(rnorm), -1022), 1022) : 0;   // (s, 1 / s normal)
    const double s = std::ldexp(1.0, ex), inv = std::ldexp(1.0, -ex);
    const double bm = bottom_metric;
    bottom_metric = bm * s;
    Depth32& z = f32_[0];
    launch_convert(st_, z.res, res, n, s);
    if (!e_zero) launch_convert(st_, z.corr, e, n, s);
    cycle32(0, z.corr, z.res, e_zero);
    if (add_to_phi) launch_incr(st_, e, z.corr, inv, n);
    else launch_convert(st_, e, z.corr, n, inv);
    bottom_metric = bm;
}

bool PressureSolver::fold_prolong(int d) const
{
    const Level& F = *lev[d];
    if (tune_.no_fold_prolong || !fused_relax(d, prm.num_smooth_up) || ordered(d) || hasCF_) return false;
    return !F.zeroAvg || sf_valid_[d];
}

// ------------------------------------------------------------------------------------
// Chombo 3.1 BiCGStabSolver<T>::solve (EXTERNAL to the reference; restated from the published
// algorithm, same variable names).  Runs on the coarsest MG depth.
// ------------------------------------------------------------------------------------
// A bottom level small enough for the one-launch BiCGStab (k_tiny_bicgstab): all boxes on this rank,
// the 7-point operator, Neumann / periodic sides, no coarse-fine faces, point GSRB) and serial-order sums.
// SOMAR_FUSED_BOTTOM_MAX_CELLS (default 512, 0 = off) is the A/B switch.
bool PressureSolver::fused_bottom(int d) const
{
    const long long maxc = tune_.fused_bottom_max_cells;
    const Level& L = *lev[d];
    return maxc > 0 && tune_.poll_fetch && !full_ && !diri_ && L.ncf == 0 && L.plan.peers.empty() && !profiling_ && !capturing_ &&
           comm_->size == 1 && L.valid_cells_global <= maxc && ordered(d) && !ord_sharded(d) && L.dev.ntiles > 0 &&
           L.dev.tile_j >= 1 && L.dev.tile_j <= 16 && (1024 % (64 * L.dev.tile_j)) == 0 &&
           prm.relaxMode == RELAX_LEVEL_GSRB && prm.precondMode != PRECOND_DIAG_LINE_RELAX && bicg[7] != nullptr;
}

// A bottom level for the persistent one-workgroup-per-box BiCGStab (k_box_bicgstab): every box on this rank, the boxes cover
// the whole domain (no coarse-fine faces), the 7-point operator with Neumann / periodic sides, point GSRB, at most BOX_MAX_WG
// boxes of at most BOX_MAX_CELLS cells.
bool PressureSolver::box_bottom(int d) const
{
    const Level& L = *lev[d];
    if (!tune_.box_bottom || !tune_.poll_fetch || diri_ || L.ncf != 0 || !L.plan.peers.empty() || profiling_ || capturing_ ||
        comm_->size != 1 || prm.relaxMode != RELAX_LEVEL_GSRB || prm.precondMode == PRECOND_DIAG_LINE_RELAX || !bicg[7])
        return false;
    // (the 19-point operator has no single-workgroup kernel: its bottoms come here whatever their size; so does a level of
    // one box, which takes the kernel's workgroup-local variant)
    const bool one_box = !full_ && L.npatches() == 1;
    if ((!full_ && !one_box && L.valid_cells_global < tune_.box_bottom_min_cells) || L.valid_cells_global != L.domain.numPts()) return false;
    if (L.npatches() < 1 || L.npatches() > BOX_MAX_WG || L.field_elems > 0x7fffffffll) return false;
    for (const PatchDesc& p : L.hpatches)
        if ((long long)p.n[0] * p.n[1] * p.n[2] > BOX_MAX_CELLS) return false;
    if (full_) {
        // the 19-point variant: 3-D, boxes of at most 256 cells and at least 2 wide (order-2 extrapolation reads three cells
        // back from a ghost), the box grown by one cell and its two ghost programs within the kernel's LDS arrays
        if (!L.active[2] || hasCF_) return false;
        const int d0 = (int)lev.size() - 1;
        if (d != d0 || (int)full_prog_.size() <= d) return false;
        for (const PatchDesc& p : L.hpatches) {
            if ((long long)p.n[0] * p.n[1] * p.n[2] > 256 || p.n[0] < 2 || p.n[1] < 2 || p.n[2] < 2) return false;
            if ((long long)(p.n[0] + 2) * (p.n[1] + 2) * (p.n[2] + 2) > BOX_FAB_MAX) return false;
        }
        if (box_depth_ == d && !box_full_ok_) return false;   // (tables built: a program did not fit the kernel's LDS arrays)
    }
    return true;
}

// For every valid cell of depth d (boxes back to back, Fortran order inside a box) the field offsets of the six cells its
// stencil reads: the neighbour itself, or the valid cell the level's ghost exchange copies into that ghost cell (the exchange
// plan applied to an identity map) -- k_box_bicgstab reads neighbouring boxes directly and never fills a ghost cell.
void PressureSolver::build_box_tables(int d)
{
    if (box_depth_ == d) return;
    SOMAR_CHECK(box_depth_ < 0, "box bottom solver tables built for another depth");
    const Level& L = *lev[d];
    std::vector<int> G((size_t)L.field_elems);
    for (size_t q = 0; q < G.size(); ++q) G[q] = (int)q;
    auto at = [](const PatchDesc& p, int i, int j, int k) { return p.off + i + (long long)p.pj * j + p.pk * k; };
    for (const CopyItem& it : L.plan.local) {
        const PatchDesc& sp = L.hpatches[it.src_patch];
        const PatchDesc& dp = L.hpatches[it.dst_patch];
        for (int k = 0; k < it.n[2]; ++k)
            for (int j = 0; j < it.n[1]; ++j)
                for (int i = 0; i < it.n[0]; ++i)
                    G[(size_t)at(dp, it.dst_lo[0] + i, it.dst_lo[1] + j, it.dst_lo[2] + k)] =
                        (int)at(sp, it.src_lo[0] + i, it.src_lo[1] + j, it.src_lo[2] + k);
    }
    std::vector<int> cstart(L.hpatches.size() + 1, 0), nb;
    box_max_cells_ = 0;
    for (size_t b = 0; b < L.hpatches.size(); ++b) {
        const PatchDesc& p = L.hpatches[b];
        const int cells = p.n[0] * p.n[1] * p.n[2];
        cstart[b + 1] = cstart[b] + cells;
        box_max_cells_ = std::max(box_max_cells_, cells);
        for (int k = 0; k < p.n[2]; ++k)
            for (int j = 0; j < p.n[1]; ++j)
                for (int i = 0; i < p.n[0]; ++i) {
                    const long long c = at(p, i, j, k);
                    const long long off[6] = {c - 1, c + 1, c - p.pj, c + p.pj, c - p.pk, c + p.pk};
                    for (int s = 0; s < 6; ++s) {   // (a flat level has no z frame: those two entries are never read)
                        const long long v = off[s] >= 0 && off[s] < L.field_elems ? G[(size_t)off[s]] : c;
                        nb.push_back((int)v);
                        // a level of one box (the workgroup-local kernel turns the entries into compact cell numbers): the
                        // neighbour inside the box, a valid cell of the box through a periodic seam, or -- a physical side --
                        // the ghost cell's own offset; anything else would be read as the own cell, so it is an error here
                        if (L.hpatches.size() == 1 && !full_ && (s < 4 || L.active[2]) && v != off[s]) {
                            const long long rel = v - p.off;
                            const long long wk = rel >= 0 ? rel / p.pk : -1, wr = rel >= 0 ? rel % p.pk : 0;
                            SOMAR_CHECK(rel >= 0 && wr % p.pj < p.n[0] && wr / p.pj < p.n[1] && wk < p.n[2],
                                        "box bottom solver: a neighbour of a one-box level that is no valid cell of the box");
                        }
                    }
                }
    }
    box_.sums = DevBuf<double>((size_t)4 * BOX_MAX_WG + 8);   // + 6 debug counters (SOMAR_BOX_TIMING)
    box_.sync = DevBuf<unsigned>(BOX_MAX_WG + 1);
    if (full_) {
        // the box grown by one cell: where each of its cells' values comes from
        std::vector<int> fab, fstart(L.hpatches.size() + 1, 0);
        for (size_t b = 0; b < L.hpatches.size(); ++b) {
            const PatchDesc& p = L.hpatches[b];
            fstart[b] = (int)fab.size();
            for (int k = -1; k <= p.n[2]; ++k)
                for (int j = -1; j <= p.n[1]; ++j)
                    for (int i = -1; i <= p.n[0]; ++i) {
                        const long long c = at(p, i, j, k);
                        const bool inside = i >= 0 && i < p.n[0] && j >= 0 && j < p.n[1] && k >= 0 && k < p.n[2];
                        fab.push_back(inside ? (int)c : (G[(size_t)c] != (int)c ? G[(size_t)c] : -1));
                    }
        }
        fstart[L.hpatches.size()] = (int)fab.size();
        box_.fab = DevBuf<int>::from(fab);
        box_.fabstart = DevBuf<int>::from(fstart);
        // the two ghost programs ([0] operator, [1] smoother), one entry per written cell, stage after stage: what the kernel
        // runs on its LDS copy with one thread per entry (decoding ops and their regions there cost 20 us per program)
        box_full_ok_ = true;
        for (int w = 0; w < 2; ++w) {
            const FullProgram& Pg = full_prog_[d][w];
            std::vector<BoxProgEntry> ent;
            std::vector<int> efirst(L.hpatches.size() + 1, 0), stg, sfirst(L.hpatches.size() + 1, 0), nfg, nfirst(L.hpatches.size() + 1, 0);
            for (size_t b = 0; b < L.hpatches.size(); ++b) {
                const PatchDesc& p = L.hpatches[b];
                const int m0 = p.n[0] + 2, m01 = m0 * (p.n[1] + 2);
                const int fs[3] = {1, m0, m01};
                const long long gst[3] = {1, (long long)p.pj, p.pk};
                efirst[b] = (int)ent.size();
                sfirst[b] = (int)stg.size();
                nfirst[b] = (int)nfg.size();
                int cur = -1;
                const int o0 = Pg.h_box_first.empty() ? 0 : Pg.h_box_first[b], o1 = Pg.h_box_first.empty() ? 0 : Pg.h_box_first[b + 1];
                for (int o = o0; o < o1; ++o) {
                    const GhostOp& op = Pg.h_box_ops[o];
                    const int stage = ghost_stage(op.stage);
                    if (stage != cur) { stg.push_back((int)ent.size() - efirst[b]); cur = stage; }
                    SOMAR_CHECK(!ghost_is_diri(op.type), "k_box_bicgstab: Dirichlet ghosts are not compiled (levels with Dirichlet sides take the launch path)");
                    for (int k = 0; k < op.n[2]; ++k)
                        for (int j = 0; j < op.n[1]; ++j)
                            for (int i = 0; i < op.n[0]; ++i) {
                                const int l0 = op.lo[0] + i, l1 = op.lo[1] + j, l2 = op.lo[2] + k;
                                const int f = (l0 + 1) + m0 * (l1 + 1) + m01 * (l2 + 1);
                                BoxProgEntry en;
                                std::memset(&en, 0, sizeof(en));
                                en.dst = (unsigned short)f;
                                en.flags = (unsigned char)((op.dstf ? 1 : 0) | (op.srcf ? 2 : 0));
                                if (op.type == GHOST_COPY) {
                                    en.kind = 0;
                                } else if (op.type == GHOST_EXTRAP) {
                                    const int dd = -op.sgn * fs[op.dir];
                                    en.kind = (unsigned char)(1 + op.order);
                                    en.s1 = (unsigned short)(f + dd);
                                    en.s2 = (unsigned short)(f + 2 * dd);
                                    en.s3 = (unsigned short)(f + 3 * dd);
                                } else {   // GHOST_NEUM: writes phi, reads psi around the face and the first valid cell of phi
                                    en.kind = 4;
                                    en.flags = (unsigned char)((op.dir << 2) | (op.sgn > 0 ? 16 : 0));
                                    en.nslot = (unsigned short)((int)nfg.size() - nfirst[b]);
                                    const long long face = at(p, l0, l1, l2) + (op.sgn < 0 ? gst[op.dir] : 0);
                                    nfg.push_back((int)((face << 2) | op.dir));
                                }
                                ent.push_back(en);
                            }
                }
                stg.push_back((int)ent.size() - efirst[b]);
                if ((int)ent.size() - efirst[b] > BOX_MAX_ENT || (int)stg.size() - sfirst[b] > BOX_MAX_STAGES + 1 ||
                    (int)nfg.size() - nfirst[b] > BOX_MAX_NEUM || L.field_elems >= (1ll << 28))
                    box_full_ok_ = false;
            }
            efirst[L.hpatches.size()] = (int)ent.size();
            sfirst[L.hpatches.size()] = (int)stg.size();
            nfirst[L.hpatches.size()] = (int)nfg.size();
            // an empty table still goes up as one element: the kernel takes no null pointer
            if (ent.empty()) ent.resize(1);
            if (stg.empty()) stg.resize(1);
            if (nfg.empty()) nfg.resize(1);
            box_.ent[w] = DevBuf<BoxProgEntry>::from(ent);
            box_.entfirst[w] = DevBuf<int>::from(efirst);
            box_.stg[w] = DevBuf<int>::from(stg);
            box_.stgfirst[w] = DevBuf<int>::from(sfirst);
            box_.nfg[w] = DevBuf<int>::from(nfg);
            box_.nfgfirst[w] = DevBuf<int>::from(nfirst);
        }
    }
    box_.nb = DevBuf<int>::from(nb);
    box_.cstart = DevBuf<int>::from(cstart);
    box_depth_ = d;
}

void PressureSolver::bottom_solve(double* phi, const double* rhs)
{
    ++counters[3];
    const int d = (int)lev.size() - 1;
    const long long n = lev[d]->field_elems;
    // a level of one box goes to the workgroup-local k_box_bicgstab whatever its size; other tiny levels to k_tiny_bicgstab first
    const bool one_box = !full_ && lev[d]->npatches() == 1;
    if ((one_box || !fused_bottom(d)) && box_bottom(d)) build_box_tables(d);   // (the 19-point tables may turn out not to fit: asked again below)
    if ((one_box || !fused_bottom(d)) && box_bottom(d)) {
        Level& L = *lev[d];
        BoxBicg A;
        std::memset(&A, 0, sizeof(A));
        A.nb = box_.nb;
        A.cstart = box_.cstart;
        A.phi = phi;
        A.rhs = rhs;
        A.z[0] = bicg[4];
        A.z[1] = bicg[5];
        A.imax = prm.bottom_imax;
        A.numRestarts = prm.bottom_numRestarts;
        A.normType = prm.bottom_normType;
        A.precondIters = (prm.num_smooth_precond == 0 || prm.precondMode == PRECOND_NONE) ? 0 : prm.num_smooth_precond;
        if (A.precondIters > 0 && unswept(d)) A.precondIters = -1;   // the diagonal scaling, no sweep
        A.eps = bottom_eps_eff;
        A.reps = prm.bottom_reps;
        A.hang = prm.bottom_hang;
        A.small = prm.bottom_small;
        A.metric = bottom_metric;
        A.sums = box_.sums;
        A.sync = box_.sync;
        A.serial = ordered(d) ? 1 : 0;
        A.dbg = tune_.box_timing ? reinterpret_cast<long long*>(box_.sums + 4 * BOX_MAX_WG) : nullptr;
        A.full = full_ ? 1 : 0;
        if (full_) {
            A.fab_src = box_.fab;
            A.fab_start = box_.fabstart;
            for (int w = 0; w < 2; ++w) {
                A.ent[w] = box_.ent[w]; A.ent_first[w] = box_.entfirst[w];
                A.stg[w] = box_.stg[w]; A.stg_first[w] = box_.stgfirst[w];
                A.nfg[w] = box_.nfg[w]; A.nfg_first[w] = box_.nfgfirst[w];
            }
        }
        A.info = d_scalars + SLOT_TMP;
        A.pub = ScalarPublish{h_scalars + SLOT_TMP, h_seq_, ++fetch_seq_};
        launch_box_bicgstab(st_, L.dev, box_max_cells_, A);
        bottom_pending_ = A.pub.seq;
        bottom_kind = 2;
        if (!bottom_defer_ || tune_.box_timing) bottom_collect();
        if (tune_.box_timing) {
            long long t[6];
            SOMAR_HIP(hipMemcpy(t, A.dbg, sizeof(t), hipMemcpyDeviceToHost));
            fprintf(stderr, "[somar box timing] iterations %d: ticks staging %lld, program %lld, barrier %lld, sums %lld, stagings %lld (100 MHz s_memtime)\n",
                    bottom_iters, t[0], t[1], t[3], t[4], t[5]);
        }
        return;
    }
    if (fused_bottom(d)) {
        Level& L = *lev[d];
        TinyBicg A;
        std::memset(&A, 0, sizeof(A));
        A.phi = phi;
        A.rhs = rhs;
        for (int q = 0; q < 8; ++q) A.w[q] = bicg[q];
        A.imax = prm.bottom_imax;
        A.numRestarts = prm.bottom_numRestarts;
        A.normType = prm.bottom_normType;
        A.precondIters = (prm.num_smooth_precond == 0 || prm.precondMode == PRECOND_NONE) ? 0 : prm.num_smooth_precond;
        if (A.precondIters > 0 && unswept(d)) A.precondIters = -1;   // the diagonal scaling, no sweep
        A.eps = bottom_eps_eff;
        A.reps = prm.bottom_reps;
        A.hang = prm.bottom_hang;
        A.small = prm.bottom_small;
        A.metric = bottom_metric;
        A.info = d_scalars + SLOT_TMP;
        A.pub = ScalarPublish{h_scalars + SLOT_TMP, h_seq_, ++fetch_seq_};
        launch_tiny_bicgstab(st_, L.dev, L.d_local_items, (int)L.plan.local.size(), n, A);
        bottom_pending_ = A.pub.seq;
        bottom_kind = 1;
        if (!bottom_defer_) bottom_collect();
        return;
    }
    double *r = bicg[0], *r_tilde = bicg[1], *e = bicg[2], *p = bicg[3], *p_tilde = bicg[4], *s_tilde = bicg[5],
           *t = bicg[6], *v = bicg[7];
    const int nt = prm.bottom_normType;
    int recount = 0;
    bottom_kind = 0;
    residual(d, r, phi, rhs);
    launch_copy(st_, r_tilde, r, n);
    launch_set(st_, e, n, 0.0);
    launch_set(st_, p_tilde, n, 0.0);
    launch_set(st_, s_tilde, n, 0.0);
    int i = 0;
    double rho[4] = {0, 0, 0, 0};
    double nrm[2];
    nrm[0] = norm(d, r, nt);
    double initial_norm = nrm[0];
    const double initial_rnorm = nrm[0];
    nrm[1] = nrm[0];
    double alpha[2] = {0, 0}, beta[2] = {0, 0}, omega[2] = {0, 0};
    bool init = true;
    int restarts = 0;
    if (bottom_metric > 0) initial_norm = bottom_metric;
    const double eps = bottom_eps_eff;
    bottom_exit = -1;
    while ((i < prm.bottom_imax && nrm[0] > eps * nrm[1]) && (nrm[1] > 0)) {
        ++i;
        nrm[1] = nrm[0];
        alpha[1] = alpha[0]; beta[1] = beta[0]; omega[1] = omega[0];
        rho[3] = rho[2]; rho[2] = rho[1];
        rho[1] = dot(d, r_tilde, r);
        if (rho[1] == 0.0) {
            launch_incr(st_, phi, e, 1.0, n);
            bottom_exit = 2;
            bottom_iters = i;
            return;
        }
        if (init) {
            launch_copy(st_, p, r, n);
            init = false;
        } else {
            beta[1] = (rho[1] / rho[2]) * (alpha[1] / omega[1]);
            launch_bicg_p(st_, p, v, r, beta[1], -beta[1] * omega[1], n);   // scale, incr, incr in one pass (same roundings)
        }
        pre_cond(d, p_tilde, p);
        apply_op(d, v, p_tilde);
        const double m = dot(d, r_tilde, v);
        alpha[0] = rho[1] / m;
        if (std::fabs(m) > prm.bottom_small * std::fabs(rho[1])) {
            launch_incr2(st_, r, v, -alpha[0], e, p_tilde, alpha[0], n);   // r -= alpha v; e += alpha p~ (independent)
            nrm[0] = norm(d, r, nt);
        } else {
            launch_set(st_, r, n, 0.0);
            nrm[0] = 0.0;
        }
        if (nrm[0] > eps * initial_norm && nrm[0] > prm.bottom_reps * initial_rnorm) {
            pre_cond(d, s_tilde, r);
            apply_op(d, t, s_tilde);
            // (t,r) and (t,t) in one host round trip
            if (ord_sharded(d)) {
                ordered_sums(d, t, r, 0, 0.0, d_scalars + SLOT_TMP);
                ordered_sums(d, t, t, 0, 0.0, d_scalars + SLOT_TMP + 1);
            } else {
                launch_reduce(st_, lev[d]->dev, t, r, 0, d_partials, d_scalars + SLOT_TMP, ordered(d));
                launch_reduce(st_, lev[d]->dev, t, t, 0, d_partials, d_scalars + SLOT_TMP + 1, ordered(d));
                comm_->allreduce(d_scalars + SLOT_TMP, 2, 0, st_);
            }
            fetch_scalars(SLOT_TMP, 2);
            const double tr = h_scalars[SLOT_TMP], tt = h_scalars[SLOT_TMP + 1];
            omega[0] = tr / tt;
            launch_incr2(st_, e, s_tilde, omega[0], r, t, -omega[0], n);
            nrm[0] = norm(d, r, nt);
        }
        if (nrm[0] <= eps * initial_norm || nrm[0] <= prm.bottom_reps * initial_rnorm) {
            bottom_exit = 1;
            break;
        }
        if (omega[0] == 0.0 || nrm[0] > (1 - prm.bottom_hang) * nrm[1]) {
            if (recount == 0) {
                recount = 1;
            } else {
                recount = 0;
                launch_incr(st_, phi, e, 1.0, n);
                if (restarts == prm.bottom_numRestarts) {
                    bottom_exit = 3;
                    bottom_iters = i;
                    return;
                }
                residual(d, r, phi, rhs);
                nrm[0] = norm(d, r, nt);
                rho[0] = rho[1] = rho[2] = rho[3] = 0.0;
                alpha[0] = beta[0] = omega[0] = 0.0;
                launch_copy(st_, r_tilde, r, n);
                launch_set(st_, e, n, 0.0);
                ++restarts;
                init = true;
            }
        }
    }
    launch_incr(st_, phi, e, 1.0, n);
    bottom_iters = i;
}

// ------------------------------------------------------------------------------------
// MappedAMRMultiGrid::solveNoInitResid for l_base == l_max == 0, MappedAMRMultiGrid.H:979-1183
// ------------------------------------------------------------------------------------
void PressureSolver::solve(bool zeroPhi, bool forceHomogeneous, SolveStats& s)
{
    SOMAR_CHECK(finalized, "solve before finalize");
    check_idle("solve");
    Level& L = *lev[0];
    const long long n = L.field_elems;
    launch_set(st_, f_uberRes, n, 0.0);
    launch_set(st_, f_uberCorr, n, 0.0);
    if (zeroPhi) launch_set(st_, f_phi, n, 0.0);
    launch_copy(st_, f_best, f_phi, n);
    residual(0, f_uberRes, f_phi, f_rhs, forceHomogeneous);  // computeAMRResidual(..., a_forceHomogeneous), :1021
    OuterLoop o;
    o.start(norm(0, f_uberRes, 0), prm);
    bottom_metric = o.initial;              // setConvergenceMetrics(initial_rnorm, cushion*eps), :1047
    bottom_eps_eff = 1.0 * prm.eps;
    while (o.go()) {
        o.begin_cycle();
        if (mp_K_ > 0) {
            vcycle_mixed(f_phi, f_uberRes, o.rnorm, true, true);   // the fp32 correction from zero, phi += (double)corr in one pass
        } else {
            vcycle(f_uberCorr, f_uberRes, true);          // uberCorrection is zero here (setToZero, :1203)
            launch_incr(st_, f_phi, f_uberCorr, 1.0, n);   // postVCycleOps, :1189-1215
        }
        residual(0, f_uberRes, f_phi, f_rhs, forceHomogeneous);
        if (o.end_cycle(norm(0, f_uberRes, 0), prm)) launch_copy(st_, f_best, f_phi, n);
    }
    if (o.finish(prm, true, s)) launch_copy(st_, f_phi, f_best, n);
    s.bottom_iters_last = bottom_iters;
    s.bottom_exit_last = bottom_exit;
    sync();
}

}  // namespace somar
