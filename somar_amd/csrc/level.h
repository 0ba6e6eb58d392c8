// somar_amd/csrc/level.h -- device-resident level data: the MI355X counterpart of
// Chombo's DisjointBoxLayout + LevelData<FArrayBox> + Copier for ONE (AMR level, MG depth).
//
// Design (not a port): the caller's box layout is honoured semantically (it decides the MG
// depth exactly like the reference's coarsenable() tests) but physically every field of a
// level is ONE HBM allocation holding all local patches back to back, every field shares
// the same patch table, and ghost exchange is one kernel launch over a precomputed list of
// box-to-box copies (plus one packed message per neighbouring rank when the layout is
// sharded over GPUs).
#pragma once
#include <array>
#include <memory>
#include <vector>

#include "common.h"
#include "devbuf.h"
#include "kernels.h"
#include "tuning.h"

namespace somar {

struct IBox {
    int lo[3], hi[3];
    IBox() : lo{0, 0, 0}, hi{-1, -1, -1} {}
    IBox(const int* l, const int* h) { for (int d = 0; d < 3; ++d) { lo[d] = l[d]; hi[d] = h[d]; } }
    bool empty() const { return hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]; }
    int size(int d) const { return hi[d] - lo[d] + 1; }
    long long numPts() const { return empty() ? 0 : (long long)size(0) * size(1) * size(2); }
    IBox grow(const int* g) const { IBox b = *this; for (int d = 0; d < 3; ++d) { b.lo[d] -= g[d]; b.hi[d] += g[d]; } return b; }
    IBox shift(const int* s) const { IBox b = *this; for (int d = 0; d < 3; ++d) { b.lo[d] += s[d]; b.hi[d] += s[d]; } return b; }
    IBox operator&(const IBox& o) const {
        IBox b;
        for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d] > o.lo[d] ? lo[d] : o.lo[d]; b.hi[d] = hi[d] < o.hi[d] ? hi[d] : o.hi[d]; }
        return b;
    }
    bool operator==(const IBox& o) const {
        for (int d = 0; d < 3; ++d) if (lo[d] != o.lo[d] || hi[d] != o.hi[d]) return false;
        return true;
    }
    // Chombo coarsen(): floor division
    static int fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
    IBox coarsen(const int* r) const { IBox b; for (int d = 0; d < 3; ++d) { b.lo[d] = fdiv(lo[d], r[d]); b.hi[d] = fdiv(hi[d], r[d]); } return b; }
    IBox refine(const int* r) const { IBox b; for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d] * r[d]; b.hi[d] = (hi[d] + 1) * r[d] - 1; } return b; }
};

bool coarsenable(const std::vector<IBox>& boxes, const int* r);
void box_subtract(const IBox& a, const IBox& b, std::vector<IBox>& out);
std::vector<std::array<int, 3>> periodic_shifts(const IBox& domain, const bool periodic[3]);
std::vector<IBox> uncovered(const IBox& region, const std::vector<IBox>& boxes, const IBox& domain,
                            const bool periodic[3]);

// Inter-GPU transport used by a sharded level (one process per GPU).  The default is the
// single-rank no-op; comm_rccl.cpp provides the RCCL/xGMI implementation.
struct Comm {
    int rank = 0, size = 1;
    virtual ~Comm() {}
    // in-place on DEVICE memory, enqueued on st.  op: 0 sum, 1 max
    virtual void allreduce(double* dbuf, int n, int op, hipStream_t st) { (void)dbuf; (void)n; (void)op; (void)st; }
    // the same without any single-rank shortcut (somar_comm_selftest)
    virtual void allreduce_raw(double* dbuf, int n, int op, hipStream_t st) { allreduce(dbuf, n, op, st); }
    // grouped neighbour exchange: for every peer q: send sendbuf+soff[q] (scount[q] doubles) and
    // receive into recvbuf+roff[q] (rcount[q] doubles), enqueued on st.
    virtual void neighbor_exchange(const double* sendbuf, double* recvbuf, const std::vector<int>& peers,
                                   const std::vector<long long>& soff, const std::vector<long long>& scount,
                                   const std::vector<long long>& roff, const std::vector<long long>& rcount,
                                   hipStream_t st)
    {
        (void)sendbuf; (void)recvbuf; (void)peers; (void)soff; (void)scount; (void)roff; (void)rcount; (void)st;
    }
    // the same for fp32 payloads (the fp32 depths of a mixed-precision cycle): offsets and counts in floats, 4 bytes per value
    // on the wire -- never widened.  Both sides of a message must use the same form.
    virtual void neighbor_exchange(const float* sendbuf, float* recvbuf, const std::vector<int>& peers,
                                   const std::vector<long long>& soff, const std::vector<long long>& scount,
                                   const std::vector<long long>& roff, const std::vector<long long>& rcount,
                                   hipStream_t st)
    {
        (void)sendbuf; (void)recvbuf; (void)peers; (void)soff; (void)scount; (void)roff; (void)rcount; (void)st;
    }
};

// Host-side plan of the ghost exchange of one level ("Copier(grids,grids,domain,ghost,true)").
struct ExchangePlan {
    std::vector<CopyItem> local;      // both boxes on this rank
    // remote part, grouped by peer rank in ascending order
    std::vector<int> peers;
    std::vector<CopyItem> send_items, recv_items;           // concatenated per peer
    std::vector<long long> send_itemoff, recv_itemoff;      // buffer offset of each item
    std::vector<long long> soff, scount, roff, rcount;      // per peer (doubles)
    long long send_total = 0, recv_total = 0;
};

ExchangePlan build_exchange_plan(const IBox& domain, const bool periodic[3], const int ghost[3],
                                 const std::vector<IBox>& boxes, const std::vector<int>& owner, int myrank);

// What a transfer between a caller's array and a level array moves, per local patch -- the one description both movers
// read (Level::move_host for host memory, upload_dev / download_dev for device memory).  The caller's array is defined on
// valid.grow(ghost) -- or, face >= 0, on faces(valid, face) without ghosts -- with ncomp components, component slowest;
// the region moved is valid.grow(grow) resp. the whole face box.  A field transfer has grow = ghost, a solve's phi / rhs
// upload grow = 0, the cell-centred velocity up grow = 1 in the space directions and down grow = 0.
// check_shape: 0 <= grow <= ghost, grow <= FRAME (the region has to fit the device frame; ghost itself is unbounded, the
// caller box only sets the pitch), face arrays carry no ghosts.
struct BoxIoShape {
    int ghost[3] = {0, 0, 0};
    int grow[3] = {0, 0, 0};
    int face = -1;
    int ncomp = 1;
    bool operator==(const BoxIoShape& o) const
    {
        for (int d = 0; d < 3; ++d) if (ghost[d] != o.ghost[d] || grow[d] != o.grow[d]) return false;
        return face == o.face && ncomp == o.ncomp;
    }
    static BoxIoShape cells(const int g[3], bool with_ghosts)
    {
        BoxIoShape s;
        for (int d = 0; d < 3; ++d) { s.ghost[d] = g[d]; s.grow[d] = with_ghosts ? g[d] : 0; }
        return s;
    }
    static BoxIoShape faces(int dir) { BoxIoShape s; s.face = dir; return s; }
};
void check_shape(const BoxIoShape& s);   // throws "ghost wider than device frame" etc.
struct BoxIoBoxes { IBox caller, region; };

// A tile table: its host copy and its device copy, and how it was planned (TileSpan::classes).
class TileTable {
public:
    void assign(std::vector<Tile> t, int classes)
    {
        dev_.reset();
        host_ = std::move(t);
        dev_ = DevBuf<Tile>::from(host_);
        classes_ = classes;
    }
    void clear() { assign({}, 0); }
    TileSpan span() const { return TileSpan{dev_.get(), size(), classes_}; }
    int size() const { return (int)host_.size(); }
    bool empty() const { return host_.empty(); }
    const std::vector<Tile>& host() const { return host_; }

private:
    std::vector<Tile> host_;
    DevBuf<Tile> dev_;
    int classes_ = 0;
};
// a marching table and its split on a sharded level; own and rem keep the order and the classes of `all`
struct SplitTileTable {
    TileTable all, own, rem;
    void clear() { all.clear(); own.clear(); rem.clear(); }
};
// How PressureSolver asks for the marching tables.  narrow7: the 7-point tables use the narrow lane classes (depths whose
// metric is uniform); tall7: the metric is known not to be uniform, so the fused sweep's table may take tall (all class-1)
// tiles where march_plan::tall_eligible allows them; fused19: build the fused 19-point sweep's tables too.
struct MarchRequest {
    bool narrow7 = false, tall7 = false, fused19 = false;
};

class Level {
public:
    // layout
    IBox domain;
    bool periodic[3] = {false, false, false};
    double dx[3] = {1, 1, 1};
    int active[3] = {1, 1, 1};
    int bc_type[3][2];
    std::vector<IBox> boxes;   // the whole DisjointBoxLayout, in the caller's order
    std::vector<int> owner;    // rank of each box
    std::vector<int> local;    // global box index of each local patch
    std::vector<PatchDesc> hpatches;
    TileTable tiles;             // base table (dev.tiles): 128 x tile_j x tk bricks, XCD-contiguous order
    // (re)builds the marching kernels' tile tables below from march_plan.h; the request is kept in `march`
    void build_march_tiles(const MarchRequest& req);
    MarchRequest march;
    // fused red-black sweep (gsrb_fused.hip).  Sharded levels: own = the tiles that read no ghost cell another rank fills (they
    // may run while the messages are in flight), rem = the rest (fused_overlap in solver.cpp)
    SplitTileTable ftiles;
    SplitTileTable rtiles;       // k-marching operator / residual (resid_march.hip); it reads phi one cell around
    TileTable qtiles;            // k-marching 19-point kernels (full19_march.hip)
    // fused red+black 19-point sweep (full19_fused.hip), built when PressureSolver asks (MarchRequest::fused19): its column tiles
    // and the tiles of the shell pass that follows it (the three outer cell layers of every box)
    TileTable gtiles, stiles;
    TileTable ctiles;            // whole-column tiles (line relaxation): 128 x ctile_j columns, all of k
    int ctile_j = 2;
    long long field_elems = 0;
    long long valid_cells_global = 0;
    ExchangePlan plan;
    Comm* comm = nullptr;
    Tuning tune;               // the owning solver's switches, as define received them (tile tables are rebuilt later)

    // device tables
    DevBuf<PatchDesc> d_patches;
    DevBuf<CopyItem> d_local_items;
    // pull exchange tables (LevelDev::tile_items): built for single-rank levels of at most Tuning::pull_max_cells cells
    DevBuf<CopyItem> d_tile_items;
    DevBuf<int> d_tile_item_start;
    bool pull_ready() const { return bool(d_tile_item_start); }
    DevBuf<CopyItem> d_send_items, d_recv_items;
    DevBuf<long long> d_send_off, d_recv_off;
    DevBuf<double> d_sendbuf, d_recvbuf;
    // metric planes: J g^{aa} on a-faces, J^{-1}, lapDiag; jgx[a][b] (a != b): the cross planes of a non-diagonal metric
    DevBuf<double> jg[3], jinv, lapdiag, jgx[3][3];
    LevelDev dev;  // kernel view (tables + metric planes)

    // operator state
    double alpha = 0.0, beta = 1.0;
    int mgCrseRefRatio[3] = {1, 1, 1};
    bool hasCoarser = false;
    bool zeroAvg = false;
    double dxProduct = 1.0;

    // coarse-fine ghost cells (only on levels that sit on a coarser AMR level): the cells of the 1-deep
    // ghost layer that lie inside the (periodically extended) domain and are covered by no box of this level
    std::vector<CFCell> hcf;
    DevBuf<CFCell> d_cf;
    int ncf = 0;
    double cf_c1[3] = {0, 0, 0}, cf_c2[3] = {0, 0, 0}, cf_fac[3] = {0, 0, 0};
    // The fused red-black sweep on a level with CF boundaries needs (a) every box face to be CF either entirely
    // or not at all (flag bits in PatchDesc.cf), boxes at least two cells wide, and (b) the pre-sweep CF values
    // also in the EDGE ghosts that the recomputed red ring of a neighbouring box reads -- hcfx = hcf + those.  A
    // re-entrant corner of the refined region (one edge ghost wanted with two different values) rules it out.
    std::vector<CFCell> hcfx;
    DevBuf<CFCell> d_cfx;
    int ncfx = 0;
    bool cf_fusable = true;
    std::unique_ptr<class Copier> cf_faces[3];  // high-face coefficients of neighbouring boxes (Copier::define_faces): CF levels, Dirichlet hi walls
    void cf_homog_ext(double* phi, hipStream_t st) const
    {
        launch_cf_homog(st, d_cfx, ncfx, phi, cf_c1, cf_c2, cf_fac);
    }
    // builds hcf/d_cf and the interpolation weights for a coarser-level spacing dxCrse
    void define_cf(const double dxCrse[3]);
    void cf_homog(double* phi, hipStream_t st) const
    {
        launch_cf_homog(st, d_cf, ncf, phi, cf_c1, cf_c2, cf_fac);
    }

    Level() {}
    Level(const Level&) = delete;
    Level& operator=(const Level&) = delete;

    // Build tables for a layout.  bc_type codes: BC_NEUM / BC_DIRI per non-periodic side.  t: the pull-exchange limit, the tile
    // column rules and the marching kernels' row counts; what the launchers need of it is copied into dev.
    void define(const IBox& dom, const bool per[3], const double dx_[3], const int bct[3][2],
                const std::vector<IBox>& bx, const std::vector<int>& own, Comm* c, const Tuning& t);
    // allocate coefficient planes (zero-filled) and fill dev view
    void alloc_metric();
    // the same for the cross planes behind dev.jgf[a][b] of a non-diagonal metric; dev.jgf[a][a] aliases dev.jg[a]
    void alloc_cross_metric();
    void refresh_params();

    DevBuf<double> alloc_field() const;   // zero-initialised, field_elems doubles

    // ghost exchange of one field (faces, edges and corners, 1 cell deep in active dirs)
    void exchange(double* f, hipStream_t st) const;
    // its two halves: what other ranks send (pack, one grouped send / receive per neighbour, unpack) and the box-to-box
    // copies inside this rank; they write disjoint ghost cells and may run on different streams
    void exchange_remote(double* f, hipStream_t st) const;
    void exchange_local(double* f, hipStream_t st) const;
    // fp32 fields: the same plan, item order and offsets (counted in elements); the messages carry 4 bytes per value.  They
    // go through d_sendbuf / d_recvbuf too (sized for doubles, so half used): every exchange of a level, of either element
    // type, is ordered on the stream(s) of its solver exactly as the fp64 ones are.
    void exchange(float* f, hipStream_t st) const;
    void exchange_remote(float* f, hipStream_t st) const;
    void exchange_local(float* f, hipStream_t st) const;
    // payload bytes this rank has put on the wire in the exchanges above: [0] fp64 fields, [1] fp32 fields
    mutable long long sent_bytes[2] = {0, 0};

    // host<->device transfer of one patch in Chombo FRA layout, in box form: `hostbox` is the box the host array is
    // defined on, `region` is what to move.  The primitive under move_host, and what callers with arbitrary FABs use.
    void upload(double* field, int patch, const double* host, const IBox& hostbox, const IBox& region,
                hipStream_t st) const;
    void download(const double* field, int patch, double* host, const IBox& hostbox, const IBox& region,
                  hipStream_t st) const;

    // Caller arrays in HOST memory: patch `patch` of the level arrays field[0 .. ncomp) from (to_level) or to `host`, by
    // shape.  Checks the shape and the patch index, refuses a null host pointer; enqueues on st and does not drain it.
    void move_host(double* const field[3], int patch, double* host, const BoxIoShape& shape, bool to_level, hipStream_t st) const;
    // Caller arrays in DEVICE memory, every local patch (and component) in one launch (box_io.hip).
    // dev: HOST array of npatches() device pointers in local-patch order, a null entry skips its patch; field[c]: the level
    // array component c goes to / comes from.  Every pointer is checked before the launch (check_dev_ptrs); the item table
    // is built on the first call with a given shape and reused, only its pointer column is written per call.  The calls
    // enqueue on st and drain it before they return.
    void upload_dev(double* const field[3], const double* const* dev, const BoxIoShape& shape, hipStream_t st, bool checked = false);
    void download_dev(double* const field[3], double* const* dev, const BoxIoShape& shape, hipStream_t st, bool checked = false);
    // throws unless every non-null dev[p] is device memory on this level's device (and, where the runtime knows the
    // allocation's extent, holds the whole array of patch p); `what` names the argument in the message
    void check_dev_ptrs(const double* const* dev, const BoxIoShape& shape, const char* what) const;

    int npatches() const { return (int)hpatches.size(); }

private:
    struct BoxIoTable {
        BoxIoShape shape;
        DevBuf<BoxIoItem> d_items;
        DevBuf<double*> d_ptrs;
        std::vector<double*> hptrs;   // staging of the pointer column; stable until the stream is drained
        int nitems = 0, ntiles = 0;
    };
    std::vector<std::unique_ptr<BoxIoTable>> io_tables_;
    BoxIoTable& io_table(const BoxIoShape& shape);
    BoxIoBoxes io_boxes(int patch, const BoxIoShape& shape) const;   // the one derivation of (caller box, region moved)
    void run_box_io(double* const field[3], double* const* dev, const BoxIoShape& shape, hipStream_t st, bool to_level,
                    bool checked);
};

// Copier between two layouts of one index space: valid cells of `src` boxes (and their periodic images) into
// the cells of grow(dst box, ghost).  define_allgather: every rank receives EVERY box of `src` (grown by `grow`
// cells) into a replicated layout `dst` that holds all boxes locally (coarse-level agglomeration).
class Copier {
public:
    // ring_only: only the part of each destination box's grown region that lies OUTSIDE the box (its ghost ring)
    void define(const IBox& domain, const bool periodic[3], const Level& src, const Level& dst, const int ghost[3],
                Comm* comm, bool ring_only = false);
    void define_allgather(const Level& src, const Level& dst, int grow, Comm* comm);
    void define_faces(const IBox& domain, const bool periodic[3], const Level& L, int dir, const int ghost[3],
                      Comm* comm);
    // Face-centred data of direction `dir` from one layout onto another (LevelData<FluxBox>::copyTo, one direction): every
    // face of faces(dst box, dir) that is a face of faces(src box, dir), or of a periodic image of it, receives that value.
    // A face several sources supply is written ONCE, by the source box later in layout order, periodic images last; every
    // rank derives the same pieces in the same order, so sends and receives pair up.
    void define_face_copy(const IBox& domain, const bool periodic[3], const Level& src, const Level& dst, int dir, Comm* comm);
    void run(const double* s, double* d, hipStream_t st) const;
    ExchangePlan plan;

private:
    void upload_tables();
    const Level* src_ = nullptr;
    const Level* dst_ = nullptr;
    Comm* comm_ = nullptr;
    DevBuf<CopyItem> d_local, d_send, d_recv;
    DevBuf<long long> d_soff, d_roff;
    DevBuf<double> d_sbuf, d_rbuf;
};

ExchangePlan build_copy_plan(const IBox& domain, const bool periodic[3], const std::vector<IBox>& srcBoxes,
                             const std::vector<int>& srcOwner, const std::vector<IBox>& dstBoxes,
                             const std::vector<int>& dstOwner, const int ghost[3], int myrank, bool ring_only = false);
ExchangePlan build_face_copy_plan(const IBox& domain, const bool periodic[3], const std::vector<IBox>& srcBoxes,
                                  const std::vector<int>& srcOwner, const std::vector<IBox>& dstBoxes,
                                  const std::vector<int>& dstOwner, int dir, int myrank);
// every rank gets every box (grown): items carry GLOBAL box indices on both sides
ExchangePlan build_allgather_plan(const std::vector<IBox>& boxes, const std::vector<int>& owner, int grow, int myrank,
                                  int nranks);

}  // namespace somar
