// somar_amd/csrc/march_plan.h -- how a level's boxes are cut into the tiles of the k-marching kernels: tile columns and their
// lane classes, tile rows, and the number of k-chunks.  Plain C++, no device header: Level::build_march_tiles turns the plan
// into Tile tables, and a stand-alone host program can check it (tests/test_march_plan.py).
#pragma once
#include <algorithm>
#include <vector>

namespace somar {
namespace march_plan {

// Tile columns and their lane class (Tile::pad_[1], see full19_march.hip): class 0 = 124 output columns, one region row
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

// A box is cut into FT_I-wide columns and its remainder into the narrow classes (128 -> 124 + 4, 64 -> 60 + 4, 512 -> 4 x 124 +
// 4 x 4 -- which min_gain = 0.85 turns down for 5 x 104), so that a remainder column costs a sixteenth (a half) of a
// workgroup-march instead of a whole one.
inline std::vector<ColSpec> columns(const Shape& s, int n0)
{
    std::vector<ColSpec> eq, v;
    {
        int w = s.FT_I;
        if (s.balanced) {
            const int ncol = (n0 + s.FT_I - 1) / s.FT_I;
            w = (n0 + ncol - 1) / ncol;
            w += w & 1;
            w = std::min(w, s.FT_I);
        }
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
    const int ncol = (n0 + TALL_MAX_W - 1) / TALL_MAX_W + extra;
    int w = (n0 + ncol - 1) / ncol;
    w += w & 1;
    w = std::min(w, TALL_MAX_W);
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

}  // namespace march_plan
}  // namespace somar
