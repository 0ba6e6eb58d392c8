// somar_amd/csrc/march_plan.h -- how a level's boxes are cut into the tiles of the k-marching kernels: tile columns and their
// lane classes, tile rows, the number of k-chunks, the tiles themselves in launch order, the shell tiles of the fused 19-point
// sweep and the split of a table on a sharded level.  Plain C++, no device header: Level::build_march_tiles uploads what these
// functions return, and a stand-alone host program checks them (tests/test_march_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace somar {

// Work item of a sweep kernel: a brick of one patch.  The base table's tiles (Level::define) are (128 x tile_j x nk) and leave
// w, cls and slot zero; the marching tables' tiles carry their shape.
struct Tile {
    int patch;
    int i0, j0, k0;  // local start
    int nk;
    int w;     // output columns; 0: the kernel's default width
    int cls;   // lane class (march_plan::ColSpec): the tile covers (region rows << cls) - halo rows
    int slot;  // residual table: the tile's place in the unsplit table = its slot in the per-tile partial sums (k_resid_march<2>)
};
static_assert(sizeof(Tile) == 32 && offsetof(Tile, patch) == 0 && offsetof(Tile, i0) == 4 && offsetof(Tile, j0) == 8 &&
                  offsetof(Tile, k0) == 12 && offsetof(Tile, nk) == 16 && offsetof(Tile, w) == 20 && offsetof(Tile, cls) == 24 &&
                  offsetof(Tile, slot) == 28,
              "Tile is read by every sweep kernel: 32 bytes, these offsets");

namespace march_plan {

// Tile columns and their lane class (Tile::cls, see full19_march.hip): class 0 = 124 output columns, one region row
// per wavefront; class 1 = 60 columns, two rows per wavefront; class 4 = 4 columns, sixteen rows per wavefront.
struct ColSpec { int i0, w, cls; };

// One marching table's shape.  region_rows = blockDim.y of the kernel, hrows = region rows that are halo, halo = planes a
// k-chunk reads beyond its own (fused red-black sweep: 3, marching residual: 2), slots = workgroups the device runs at a time.
struct Shape {
    int FT_I = 124;
    int region_rows = 16;
    int hrows = 4;
    double halo = 3.0;
    int slots = 256;
    // narrow lane classes for remainder columns; off: columns of equal width, all class 0 (128 -> 2 x 64, 512 -> 5 x 104)
    bool classes = false;
    bool balanced = true;      // equal columns share the box width evenly (off: FT_I-wide columns and a remainder)
    // the narrow decomposition is taken only where it costs at most that fraction of the equal columns' workgroup-marches (a
    // class-4 workgroup counted as a quarter: it runs long; a class-1 one as a half).  1.0 = always.
    double min_gain = 1.0;
};

struct BoxSize { int n0, n1, n2; };

inline int rows_of(const Shape& s, int cls) { return (s.region_rows << cls) - s.hrows; }

// equal even widths of at most maxw: the width of ceil(n0 / maxw) + extra columns that share n0 cells
inline int even_width(int n0, int maxw, int extra = 0)
{
    const int ncol = (n0 + maxw - 1) / maxw + extra;
    int w = (n0 + ncol - 1) / ncol;
    w += w & 1;
    return std::min(w, maxw);
}

// A box is cut into FT_I-wide columns and its remainder into the narrow classes (128 -> 124 + 4, 64 -> 60 + 4, 512 -> 4 x 124 +
// 4 x 4 -- which min_gain = 0.85 turns down for 5 x 104), so that a remainder column costs a sixteenth (a half) of a
// workgroup-march instead of a whole one.
inline std::vector<ColSpec> columns(const Shape& s, int n0)
{
    std::vector<ColSpec> eq, v;
    {
        const int w = s.balanced ? even_width(n0, s.FT_I) : s.FT_I;
        for (int i0 = 0; i0 < n0; i0 += w) eq.push_back({i0, w, 0});
    }
    if (!s.classes || (n0 & 1)) return eq;
    int i0 = 0, rem = n0;
    double cost = 0.0;
    while (rem >= s.FT_I) { v.push_back({i0, s.FT_I, 0}); i0 += s.FT_I; rem -= s.FT_I; cost += 1.0; }
    if (rem > 76) { v.push_back({i0, rem, 0}); rem = 0; cost += 1.0; }
    if (rem > 16) { const int w = std::min(rem, 60); v.push_back({i0, w, 1}); i0 += w; rem -= w; cost += 0.5; }
    while (rem > 0) { const int w = std::min(rem, 4); v.push_back({i0, w, 4}); i0 += w; rem -= w; cost += 0.25; }
    return cost <= s.min_gain * (double)eq.size() ? v : eq;
}

// ---- tall columns: every tile is class 1 (the fused sweep's table only) ------------------------------------------------
// The 2048-cell region of a 16-wavefront workgroup viewed as 64 x 32 instead of 128 x 16: 60 x 28 outputs.  The halo a tile
// re-reads is mostly its rows (4 of 16 phi rows, 2 of 14 coefficient rows), so the taller region trades 13 % fewer halo rows
// for 4 % more halo columns: 67.6 -> 64.2 B per cell and sweep modelled on a 512-wide box.
constexpr int TALL_MAX_W = 60;
constexpr int TALL_MIN_N0 = 128;   // boxes up to this width fit one or two class-0 / class-1 columns already

// May a level whose local boxes are `boxes` take tall tiles?  Stated in terms of box width and metric: the fused sweep streams
// its four coefficient arrays (metric not uniform: a uniform depth reads two streams, is latency-bound and keeps the lean class-0
// body), in the 16-row form, and every box is even and wider than 128 cells.  Level::build_march_tiles passes the level's own
// metric flag; what is not a matter of width and metric -- the 7-point operator, three active directions, the two switches
// that restore the equal columns -- is checked by the callers (PressureSolver::choose_narrow_tiles, Level::build_march_tiles).
inline bool tall_eligible(const std::vector<BoxSize>& boxes, int region_rows, bool uniform_metric)
{
    if (region_rows != 16 || uniform_metric || boxes.empty()) return false;
    for (const BoxSize& b : boxes)
        if ((b.n0 & 1) || b.n0 <= TALL_MIN_N0) return false;
    return true;
}

// equal even widths of at most 60: ceil(n0 / 60) + extra columns (fewer where the even width already covers the box)
inline std::vector<ColSpec> tall_columns(int n0, int extra)
{
    const int w = even_width(n0, TALL_MAX_W, extra);
    std::vector<ColSpec> v;
    for (int i0 = 0; i0 < n0; i0 += w) v.push_back({i0, w, 1});
    return v;
}

struct Plan {
    int nch = 1;      // k-chunks per box (a box's chunk: ceil(n2 / nch) planes, made even)
    int extra = -1;   // tall columns: ceil(n0 / 60) + extra per box; -1: the columns of columns()
    double eff = -1.0;
};

// workgroups per k-chunk of the level: every box's columns times their tile rows
inline long long column_tiles(const Shape& s, const std::vector<BoxSize>& boxes, int extra)
{
    long long cols = 0;
    for (const BoxSize& b : boxes)
        for (const ColSpec& c : (extra >= 0 ? tall_columns(b.n0, extra) : columns(s, b.n0)))
            cols += (b.n1 + rows_of(s, c.cls) - 1) / rows_of(s, c.cls);
    return cols;
}

// The k-chunk count that fills the slots most evenly: rounds of `slots` workgroups, each chunk paying its halo planes.
// tall: the search runs over (column count, chunk count) together; ties go to fewer columns, then to fewer chunks.  Extra
// columns are for rounding a large level's workgroups to whole rounds: a level that cannot fill the slots even once keeps
// ceil(n0 / 60) columns (the model does not see the halo columns that narrower tiles re-read; short chunks already buy it
// workgroups).
inline Plan plan(const Shape& s, const std::vector<BoxSize>& boxes, bool tall)
{
    int maxn2 = 1;
    for (const BoxSize& b : boxes) maxn2 = std::max(maxn2, b.n2);
    Plan best;
    for (int extra = tall ? 0 : -1; extra <= (tall ? 2 : -1); ++extra) {
        const long long cols = column_tiles(s, boxes, extra);
        long long most = 0;
        for (int nch = 1; nch <= 64 && (nch == 1 || maxn2 / nch >= 4); ++nch) {  // small levels: short chunks, more workgroups
            const long long blocks = cols * nch;
            const long long rounds = (blocks + s.slots - 1) / s.slots;
            const double nk = (double)maxn2 / nch;
            const double eff = (double)blocks / (double)(rounds * s.slots) * nk / (nk + s.halo);
            if (eff > best.eff + 1e-9) { best.eff = eff; best.nch = nch; best.extra = extra; }
            most = blocks;
        }
        if (extra == 0 && most < s.slots) break;
    }
    return best;
}

// planes per k-chunk of a box n2 planes deep.  Even: a chunk never splits the two planes of a coarse cell (fused restriction)
inline int chunk_planes(int n2, int nch)
{
    int nk = (n2 + nch - 1) / nch;
    nk += nk & 1;
    return nk;
}

// ---- today's tables ------------------------------------------------------------------------------------------------------
// (FT_I x tile rows) columns, k split into chunks so that the launch fills the 256 CUs evenly (one 1024-thread workgroup per
// CU at a time).  Every table takes the narrow classes only where they save at least 15 % of the workgroup-marches (64-wide
// boxes: C5 62.8 -> 53.1 ms per AMR V-cycle; 128-wide: C4 136.8 -> 111.6).  One 512-wide box, 5 equal columns against 4 + 4
// narrow, is a wash or worse: 19-point colour pass 3.02 -> 3.07 ms, residual 3.17 -> 3.42; c2_cartesian 151 -> 149-158
// V-cycles/s depending on tile order.  Level::build_march_tiles applies the two Tuning switches that restore the equal columns.
inline Shape make_shape(int region_rows, int hrows, double halo, int slots, bool classes, double min_gain)
{
    Shape s;
    s.region_rows = region_rows; s.hrows = hrows; s.halo = halo; s.slots = slots; s.classes = classes; s.min_gain = min_gain;
    return s;
}
// fused 7-point sweep (gsrb_fused.hip), 16 or 8 region rows: the 8-row kernels take class-0 tiles only
inline Shape fused_shape(int rows, bool narrow) { return make_shape(rows, 4, 3.0, 256, narrow && rows == 16, 0.85); }
// marching operator / residual (resid_march.hip): 124 x 14 columns
inline Shape resid_shape(bool narrow) { return make_shape(16, 2, 2.0, 256, narrow, 0.85); }
// marching 19-point kernels (full19_march.hip), 8 or 6 region rows: 124 x (rows - 2) columns; 6 rows: two workgroups per CU,
// never narrow
inline Shape full_shape(int rows) { return make_shape(rows, 2, 2.0, rows == 6 ? 512 : 256, rows == 8, 0.85); }
// the same kernels on several fields (full19_multi.hip): class-0 columns only, one workgroup per CU at either row count
inline Shape full_nf_shape(int rows) { return make_shape(rows, 2, 2.0, 256, false, 0.85); }
// fused red+black 19-point sweep (full19_fused.hip): 124 x 4 column tiles
inline Shape fused19_shape() { return make_shape(8, 4, 3.0, 256, false, 1.0); }

// XCD-contiguous order: block b runs on XCD (b % 8) under round-robin dispatch, so each XCD gets one contiguous slab of the
// natural (patch, k, j, i) tile order: neighbouring tiles then share their j/k halo rows through the same 4 MiB L2.
template <class T>
std::vector<T> xcd_order(const std::vector<T>& nat)
{
    const int N = (int)nat.size(), NX = 8;
    int start[NX + 1];
    start[0] = 0;
    for (int x = 0; x < NX; ++x) start[x + 1] = start[x] + (N - x + NX - 1) / NX;  // #b with b % 8 == x
    std::vector<T> v(N);
    for (int b = 0; b < N; ++b) v[b] = nat[start[b % NX] + b / NX];
    return v;
}

inline Tile make_tile(int patch, int i0, int j0, int k0, int nk, int w, int cls) { return Tile{patch, i0, j0, k0, nk, w, cls, 0}; }

// classes: what the launchers pick a kernel instantiation from (TileSpan::classes).  0: every tile is class 0; 1: the table
// holds narrow classes -- the three-body instantiations, the slower kernels on class-0 tiles alone (c2_cartesian 151 -> 140
// V-cycles/s), so only where a column of the plan really is narrow; 2: planned tall, every tile is class 1.
struct Table {
    std::vector<Tile> tiles;
    int classes = 0;
};

// One marching table of a level: per box its k-chunks, per chunk columns x rows, in XCD-contiguous order.
inline Table march_tiles(const Shape& shape, const std::vector<BoxSize>& boxes, bool tall = false)
{
    const Plan pl = plan(shape, boxes, tall);
    Table out;
    out.classes = pl.extra >= 0 ? 2 : 0;
    std::vector<Tile> nat;
    for (int pi = 0; pi < (int)boxes.size(); ++pi) {
        const BoxSize& b = boxes[pi];
        const int nk = chunk_planes(b.n2, pl.nch);
        const std::vector<ColSpec> cs = pl.extra >= 0 ? tall_columns(b.n0, pl.extra) : columns(shape, b.n0);
        for (const ColSpec& c : cs)
            if (c.cls && out.classes == 0) out.classes = 1;
        for (int k0 = 0; k0 < b.n2; k0 += nk) {
            // rows outside, columns inside (the natural order: a 512-wide box's 19-point colour pass takes 3.07 ms so, 3.23 ms
            // with the columns outside); a narrow column's tall tile goes where its first row is
            const size_t first = nat.size();
            for (const ColSpec& c : cs)
                for (int j0 = 0; j0 < b.n1; j0 += rows_of(shape, c.cls))
                    nat.push_back(make_tile(pi, c.i0, j0, k0, std::min(nk, b.n2 - k0), c.w, c.cls));
            std::stable_sort(nat.begin() + first, nat.end(), [](const Tile& x, const Tile& y) {
                return x.j0 != y.j0 ? x.j0 < y.j0 : x.i0 < y.i0;
            });
        }
    }
    out.tiles = xcd_order(nat);
    return out;
}

// the residual table's tiles know their place in it: split launches (own / rem) keep the order of the per-tile sums
inline void number_slots(std::vector<Tile>& tiles)
{
    for (size_t q = 0; q < tiles.size(); ++q) tiles[q].slot = (int)q;
}

// Shell pass of the fused 19-point sweep: per box the two x faces (4-wide class-4 columns, 126 rows each), the two y faces (one
// 6-row band of class-0 columns each) in k-chunks of 32 planes, and the two z faces (3 planes over every class-0 tile).  The sets
// overlap at the box edges: a cell relaxed twice gets the same value twice (its inputs are not written by the pass).
inline Table shell_tiles(const std::vector<BoxSize>& boxes)
{
    Table out;
    out.classes = 1;
    std::vector<Tile>& sh = out.tiles;
    const int KC = 32;
    for (int pi = 0; pi < (int)boxes.size(); ++pi) {
        const BoxSize& b = boxes[pi];
        const int wcol = even_width(b.n0, 124);
        for (int k0 = 0; k0 < b.n2; k0 += KC) {
            const int nk = std::min(KC, b.n2 - k0);
            for (int xi : {0, std::max(0, b.n0 - 4)})
                for (int j0 = 0; j0 < b.n1; j0 += 126) sh.push_back(make_tile(pi, xi, j0, k0, nk, 4, 4));
            for (int yj : {0, std::max(0, b.n1 - 6)})
                for (int i0 = 0; i0 < b.n0; i0 += wcol) sh.push_back(make_tile(pi, i0, yj, k0, nk, wcol, 0));
        }
        for (int zk : {0, std::max(0, b.n2 - 3)})
            for (int j0 = 0; j0 < b.n1; j0 += 6)
                for (int i0 = 0; i0 < b.n0; i0 += wcol) sh.push_back(make_tile(pi, i0, j0, zk, std::min(3, b.n2 - zk), wcol, 0));
    }
    return out;
}

// Sharded levels: which tiles read a cell of `regions` (the ghost regions another rank fills, in the patch's local indices)?
// A tile reads `halo` cells around its columns, rows and planes.  rem gets those tiles, own the rest -- they may run while
// the messages are in flight; both keep the table's order.
struct Region { int patch; int lo[3], n[3]; };
inline void split(const std::vector<Tile>& tiles, const Shape& shape, int halo, const std::vector<BoxSize>& boxes,
                  const std::vector<Region>& regions, std::vector<Tile>& own, std::vector<Tile>& rem)
{
    for (const Tile& t : tiles) {
        const BoxSize& b = boxes[t.patch];
        const int w = t.w > 0 ? t.w : shape.FT_I;
        const int lo[3] = {t.i0 - halo, t.j0 - halo, t.k0 - halo};
        const int hi[3] = {std::min(t.i0 + w, b.n0) - 1 + halo, std::min(t.j0 + rows_of(shape, t.cls), b.n1) - 1 + halo,
                           t.k0 + t.nk - 1 + halo};
        bool hit = false;
        for (const Region& r : regions) {
            if (r.patch != t.patch) continue;
            bool ov = true;
            for (int d = 0; d < 3; ++d) ov = ov && std::max(lo[d], r.lo[d]) <= std::min(hi[d], r.lo[d] + r.n[d] - 1);
            if (ov) { hit = true; break; }
        }
        (hit ? rem : own).push_back(t);
    }
}

}  // namespace march_plan
}  // namespace somar
