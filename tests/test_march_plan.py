"""The marching kernels' tile tables (somar_amd/csrc/march_plan.h) from a stand-alone host program: the header is plain C++ and
holds everything Level::build_march_tiles uploads -- columns, k-chunks, the tiles in launch order, the shell tiles of the fused
19-point sweep, the own / rem split of a sharded level -- so the program below calls the builder itself, without a GPU.
Today's columns are pinned (they are also what tests/helpers.march_columns restates), the tall (all class-1) plan of the fused
sweep's table is checked for what the kernel relies on (every cell in exactly one tile, even column starts, at most 60 output
columns, 28 rows per tile, even k-chunks), and whole tables are pinned by digest.

The digests (tile count, 64-bit FNV-1a over the eight ints of every tile in table order) were recorded from the commit before
the builder moved here: its march_tiles lambda and shell-tile block, pasted verbatim into a scratch host program over a
plain-int Tile with the same inputs.  They are literals, not output of the code under test."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import march_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "somar_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "march_plan.h"
using namespace somar::march_plan;
using somar::Tile;

// cols N0 CLASSES                   -> "w cls" per column of the residual / fused tables (FT_I 124, min_gain 0.85)
// plan TALL N0 N1 N2                -> "nch extra" of the fused sweep's table, then "i0 w cls j0 rows k0 nk" per tile
// eligible ROWS UNIFORM N0 [N0 ...] -> 0 / 1
// table NAME CLASSES TALL N0 N1 N2 [N0 N1 N2 ...]  (NAME: fused resid full fused19 shell; CLASSES off: what
//     Tuning::no_narrow_tiles gives)        -> "count fnv1a(hex) classes", then the eight ints of every tile
// xcd N                             -> xcd_order of 0 .. N-1
// split NAME HALO RLO0 RLO1 RLO2 RN0 RN1 RN2 (a 256 x 32 x 32 box, classes on, one region; RN0 = 0: no region)
//                                   -> per tile of all, own, rem: "section" + the eight ints
static void print_tile(const Tile& t) { std::printf("%d %d %d %d %d %d %d %d\n", t.patch, t.i0, t.j0, t.k0, t.nk, t.w, t.cls, t.slot); }

static Shape shape_of(const std::string& name, bool classes)
{
    Shape s = name == "fused" ? fused_shape(16, classes) : name == "resid" ? resid_shape(classes) : name == "full" ? full_shape(8)
                                                                                                     : fused19_shape();
    s.classes = s.classes && classes;
    return s;
}

static Table table_of(const std::string& name, bool classes, bool tall, const std::vector<BoxSize>& boxes)
{
    if (name == "shell") return shell_tiles(boxes);
    Table t = march_tiles(shape_of(name, classes), boxes, tall);
    if (name == "resid") number_slots(t.tiles);
    return t;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    Shape s = fused_shape(16, false);
    if (what == "cols") {
        s = resid_shape(std::atoi(argv[3]) != 0);
        for (const ColSpec& c : columns(s, std::atoi(argv[2]))) std::printf("%d %d\n", c.w, c.cls);
        return 0;
    }
    if (what == "plan") {
        const bool tall = std::atoi(argv[2]) != 0;
        const std::vector<BoxSize> boxes{{std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5])}};
        const Plan p = plan(s, boxes, tall);
        std::printf("%d %d\n", p.nch, p.extra);
        for (const Tile& t : march_tiles(s, boxes, tall).tiles)
            std::printf("%d %d %d %d %d %d %d\n", t.i0, t.w, t.cls, t.j0, rows_of(s, t.cls), t.k0, t.nk);
        return 0;
    }
    if (what == "eligible") {
        std::vector<BoxSize> boxes;
        for (int a = 4; a < argc; ++a) boxes.push_back({std::atoi(argv[a]), 64, 64});
        std::printf("%d\n", tall_eligible(boxes, std::atoi(argv[2]), std::atoi(argv[3]) != 0) ? 1 : 0);
        return 0;
    }
    if (what == "table") {
        std::vector<BoxSize> boxes;
        for (int a = 5; a + 2 < argc; a += 3) boxes.push_back({std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2])});
        const Table t = table_of(argv[2], std::atoi(argv[3]) != 0, std::atoi(argv[4]) != 0, boxes);
        uint64_t h = 1469598103934665603ull;
        for (const Tile& q : t.tiles) {
            const int v[8] = {q.patch, q.i0, q.j0, q.k0, q.nk, q.w, q.cls, q.slot};
            for (int i = 0; i < 8; ++i)
                for (int b = 0; b < 4; ++b) { h ^= (uint64_t)(((unsigned)v[i] >> (8 * b)) & 0xff); h *= 1099511628211ull; }
        }
        std::printf("%zu %016llx %d\n", t.tiles.size(), (unsigned long long)h, t.classes);
        for (const Tile& q : t.tiles) print_tile(q);
        return 0;
    }
    if (what == "xcd") {
        std::vector<int> nat(std::atoi(argv[2]));
        for (size_t q = 0; q < nat.size(); ++q) nat[q] = (int)q;
        for (int v : xcd_order(nat)) std::printf("%d\n", v);
        return 0;
    }
    if (what == "split") {
        const std::string name = argv[2];
        const std::vector<BoxSize> boxes{{256, 32, 32}};
        const Table t = table_of(name, true, false, boxes);
        std::vector<Region> regions;
        if (std::atoi(argv[7]) > 0)
            regions.push_back({0, {std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6])},
                               {std::atoi(argv[7]), std::atoi(argv[8]), std::atoi(argv[9])}});
        std::vector<Tile> own, rem;
        split(t.tiles, shape_of(name, true), std::atoi(argv[3]), boxes, regions, own, rem);
        for (const Tile& q : t.tiles) { std::printf("0 "); print_tile(q); }
        for (const Tile& q : own) { std::printf("1 "); print_tile(q); }
        for (const Tile& q : rem) { std::printf("2 "); print_tile(q); }
        return 0;
    }
    return 2;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("march_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(*args):
        out = subprocess.check_output([str(exe)] + [str(a) for a in args], text=True)
        lines = [line.split() for line in out.splitlines()]
        if args[0] == "table":   # the first line carries the hexadecimal digest
            return (int(lines[0][0]), lines[0][1], int(lines[0][2])), [tuple(int(x) for x in l) for l in lines[1:]]
        return [tuple(int(x) for x in l) for l in lines]
    return run


@pytest.mark.parametrize("n0, classes, want", [
    (128, 1, [(124, 0), (4, 4)]),
    (64, 1, [(60, 1), (4, 4)]),
    (512, 1, [(104, 0)] * 5),
    (132, 1, [(124, 0), (4, 4), (4, 4)]),
    (45, 1, [(46, 0)]),
    (32, 1, [(32, 1)]),
    (128, 0, [(64, 0)] * 2),
    (512, 0, [(104, 0)] * 5),
])
def test_todays_columns_are_unchanged(planner, n0, classes, want):
    assert planner("cols", n0, classes) == want
    assert march_columns(n0, bool(classes)) == want   # the restatement the GPU tests use says the same


def test_todays_k_chunks_are_unchanged(planner):
    """the fused sweep's table of one 512^3 box and of one 256^3 box: 215 column tiles x 7 chunks, 66 x 11"""
    for n, ncols, nch in ((512, 215, 7), (256, 66, 11)):
        out = planner("plan", 0, n, n, n)
        assert out[0] == (nch, -1)
        tiles = out[1:]
        assert len({t[5] for t in tiles}) == nch
        assert len(tiles) == ncols * nch
        assert all(t[2] == 0 and t[4] == 12 for t in tiles)


@pytest.mark.parametrize("n1", [28, 30, 36, 512])
@pytest.mark.parametrize("n0", [130, 136, 256, 512])
def test_tall_plan_covers_every_cell_once(planner, n0, n1):
    n2 = 64
    out = planner("plan", 1, n0, n1, n2)
    nch, extra = out[0]
    tiles = out[1:]
    assert 0 <= extra <= 2 and nch >= 1
    chunks = sorted({(t[5], t[6]) for t in tiles})
    assert chunks[0][0] == 0 and chunks[-1][0] + chunks[-1][1] == n2
    for (a0, an), (b0, _) in zip(chunks[:-1], chunks[1:]):
        assert a0 + an == b0
    assert all(k0 % 2 == 0 and nk % 2 == 0 for k0, nk in chunks)   # a chunk never splits a coarse cell's two planes
    widths = set()
    for k0, _ in chunks:
        count = np.zeros((n0, n1), dtype=np.int32)
        for i0, w, cls, j0, rows, tk0, _nk in tiles:
            if tk0 != k0:
                continue
            assert cls == 1 and rows == 28
            assert i0 % 2 == 0 and w % 2 == 0 and 0 < w <= 60
            assert i0 < n0 and j0 < n1   # no empty tile
            count[i0:min(i0 + w, n0), j0:min(j0 + rows, n1)] += 1
            widths.add(w)
        assert count.min() == 1 and count.max() == 1
    assert len(widths) == 1   # equal widths: the last column is the same tile, clipped by the box
    tile_rows = {t[3] for t in tiles}
    assert len(tile_rows) == -(-n1 // 28)
    if n1 == 28:
        assert tile_rows == {0}


def test_tall_plan_of_the_documented_boxes(planner):
    """136 -> 46 / 46 / 44 (three columns of 46, the last clipped); one 512^3 box -> 10 columns of 52, 19 tile rows, 4 chunks;
    one 256^3 box -> 5 columns of 52, 10 tile rows, 5 chunks (march_plan.h's efficiency model: 0.97 and 0.92)"""
    out = planner("plan", 1, 136, 40, 16)
    assert sorted({(t[0], t[1]) for t in out[1:]}) == [(0, 46), (46, 46), (92, 46)]
    assert sorted({t[3] for t in out[1:]}) == [0, 28]
    for n, cols, rows, nch in ((512, 10, 19, 4), (256, 5, 10, 5)):
        out = planner("plan", 1, n, n, n)
        assert out[0][0] == nch
        assert len({t[0] for t in out[1:]}) == cols and {t[1] for t in out[1:]} == {52}
        assert len({t[3] for t in out[1:]}) == rows


def test_tall_rule(planner):
    """16-row kernels, a metric that is not uniform, every box even and wider than 128"""
    assert planner("eligible", 16, 0, 136) == [(1,)]
    assert planner("eligible", 16, 0, 512, 130) == [(1,)]
    assert planner("eligible", 16, 0, 128) == [(0,)]
    assert planner("eligible", 16, 0, 512, 64) == [(0,)]
    assert planner("eligible", 16, 0, 131) == [(0,)]
    assert planner("eligible", 16, 1, 136) == [(0,)]
    assert planner("eligible", 8, 0, 136) == [(0,)]


BOXES = {
    "32": (32, 32, 32), "64": (64, 64, 64), "128x64x48": (128, 64, 48), "136x40x16": (136, 40, 16), "512": (512, 512, 512),
    "64+132x30x20": (64, 64, 64, 132, 30, 20), "16x16x16": (16, 16, 16), "64x32x24": (64, 32, 24),
}
# (table, classes, tall, boxes) -> "tile count, FNV-1a": recorded from the parent commit's builder (module docstring)
DIGESTS = {
    ("fused", 0, 0, "32"): "24 2b54d116179ac903",
    ("resid", 0, 0, "32"): "24 a1e2d1e53fae35c3",
    ("full", 0, 0, "32"): "48 8e949d22b2701d03",
    ("fused", 1, 0, "32"): "16 80dad8176cf41503",
    ("resid", 1, 0, "32"): "16 5a7d4ce3fa3b99c3",
    ("full", 1, 0, "32"): "24 1268062e449598c3",
    ("fused", 0, 0, "64"): "96 340e2598a7160f83",
    ("resid", 0, 0, "64"): "80 2ab51aa9626c8d03",
    ("full", 0, 0, "64"): "176 1edfa7d9f0024483",
    ("fused", 1, 0, "64"): "64 2191155b8a301883",
    ("resid", 1, 0, "64"): "64 58be5d8d1fab7303",
    ("full", 1, 0, "64"): "96 2e34bd116e46d783",
    ("fused", 0, 0, "128x64x48"): "144 e8d2336d89dafb83",
    ("resid", 0, 0, "128x64x48"): "120 95474b17cfdd2cc3",
    ("full", 0, 0, "128x64x48"): "176 47a27bb8e3ac9f03",
    ("fused", 1, 0, "128x64x48"): "84 3b0bb5249d25e883",
    ("resid", 1, 0, "128x64x48"): "72 eae1a44b655ceec3",
    ("full", 1, 0, "128x64x48"): "144 f1f3c01062530143",
    ("fused", 0, 0, "136x40x16"): "32 2e030d9817be6f83",
    ("resid", 0, 0, "136x40x16"): "24 8aac5838ed2a8983",
    ("full", 0, 0, "136x40x16"): "56 77b8df158dae5f83",
    ("fused", 1, 0, "136x40x16"): "32 2e030d9817be6f83",
    ("resid", 1, 0, "136x40x16"): "24 8aac5838ed2a8983",
    ("full", 1, 0, "136x40x16"): "56 77b8df158dae5f83",
    ("fused", 0, 0, "512"): "1505 33245c7bf04d4ae9",
    ("resid", 0, 0, "512"): "2035 cd450864f56638fe",
    ("full", 0, 0, "512"): "3010 80b8bcb00ab1023a",
    ("fused", 1, 0, "512"): "1505 33245c7bf04d4ae9",
    ("resid", 1, 0, "512"): "2035 cd450864f56638fe",
    ("full", 1, 0, "512"): "3010 80b8bcb00ab1023a",
    ("fused", 0, 0, "64+132x30x20"): "156 2394e8b4810379c3",
    ("resid", 0, 0, "64+132x30x20"): "140 f62b406ec85e36e3",
    ("full", 0, 0, "64+132x30x20"): "221 c1548f2d2eec34a7",
    ("fused", 1, 0, "64+132x30x20"): "114 b35084c9a6442881",
    ("resid", 1, 0, "64+132x30x20"): "114 a44a37d74aac05b0",
    ("full", 1, 0, "64+132x30x20"): "166 28416f1a224de601",
    ("fused", 0, 1, "136x40x16"): "24 bf523bfe7cee3e83",
    ("fused", 0, 1, "512"): "760 0ce63572bfdc85db",
    ("fused19", 0, 0, "16x16x16"): "16 2f3444d9a7242e83",
    ("shell", 0, 0, "16x16x16"): "10 cf57e9bf5cd13558",
    ("fused19", 0, 0, "64x32x24"): "48 c3fce88e2d28c183",
    ("shell", 0, 0, "64x32x24"): "16 7dfde186e8d64585",
}


@pytest.mark.parametrize("key", sorted(DIGESTS), ids=lambda k: "%s-c%d-t%d-%s" % k)
def test_tables_are_what_the_level_built_before(planner, key):
    table, classes, tall, boxes = key
    (count, digest, _), tiles = planner("table", table, classes, tall, *BOXES[boxes])
    assert len(tiles) == count
    assert "%d %s" % (count, digest) == DIGESTS[key]


@pytest.mark.parametrize("table, classes, tall, boxes, want", [
    ("fused", 1, 0, "32", 1),          # not tall, yet every tile is class 1: still the three-body kernel's table
    ("fused", 1, 0, "64", 1),
    ("fused", 1, 0, "512", 0),         # classes asked for, equal columns taken: the one-body kernel
    ("fused", 0, 0, "64", 0),
    ("fused", 0, 1, "512", 2),
    ("fused", 0, 1, "136x40x16", 2),
    ("resid", 1, 0, "64+132x30x20", 1),
    ("full", 1, 0, "128x64x48", 1),
    ("full", 0, 0, "128x64x48", 0),
    ("fused19", 0, 0, "64x32x24", 0),
    ("shell", 0, 0, "64x32x24", 1),    # the x faces are class-4 columns
])
def test_classes_come_from_the_plan(planner, table, classes, tall, boxes, want):
    (_, _, got), tiles = planner("table", table, classes, tall, *BOXES[boxes])
    assert got == want
    cls = {t[6] for t in tiles}
    assert cls == {0} if want == 0 else cls == {1} if want == 2 else cls != {0}


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1505])
def test_xcd_order(planner, n):
    """block b runs on XCD b % 8 and gets element start[b % 8] + b / 8 of the natural order: eight contiguous slabs"""
    got = [v for (v,) in planner("xcd", n)]
    assert sorted(got) == list(range(n))
    start = [0]
    for x in range(8):
        start.append(start[-1] + len(range(x, n, 8)))   # blocks with b % 8 == x
    assert got == [start[b % 8] + b // 8 for b in range(n)]


# one receive region of a 256 x 32 x 32 box: the whole high-x ghost face (two cells deep, as deep as the exchange fills), and a
# patch of it
@pytest.mark.parametrize("region", [(256, 0, 0, 2, 32, 32), (256, 8, 16, 2, 8, 8)])
@pytest.mark.parametrize("table, halo, region_rows, hrows", [("fused", 2, 16, 4), ("resid", 1, 16, 2)])
def test_split(planner, table, halo, region_rows, hrows, region):
    out = planner("split", table, halo, *region)
    all_, own, rem = ([t[1:] for t in out if t[0] == sec] for sec in (0, 1, 2))
    n = (256, 32, 32)

    def touches(t):
        _, i0, j0, k0, nk, w, cls, _ = t
        lo = (i0 - halo, j0 - halo, k0 - halo)
        hi = (min(i0 + w, n[0]) - 1 + halo, min(j0 + (region_rows << cls) - hrows, n[1]) - 1 + halo, k0 + nk - 1 + halo)
        return all(max(lo[d], region[d]) <= min(hi[d], region[d] + region[3 + d] - 1) for d in range(3))
    assert rem == [t for t in all_ if touches(t)] and own == [t for t in all_ if not touches(t)]   # both in table order
    assert rem and own and {t[6] for t in all_} != {0}
    assert sorted(own + rem) == sorted(all_)
    if table == "resid":
        assert [t[7] for t in all_] == list(range(len(all_)))   # slots number the unsplit order, and the halves keep them
        assert sorted(t[7] for t in own + rem) == list(range(len(all_)))
    else:
        assert {t[7] for t in all_} == {0}


@pytest.mark.parametrize("table, halo", [("fused", 2), ("resid", 1)])
def test_split_without_regions(planner, table, halo):
    out = planner("split", table, halo, 0, 0, 0, 0, 0, 0)
    all_, own, rem = ([t[1:] for t in out if t[0] == sec] for sec in (0, 1, 2))
    assert rem == [] and own == all_ and all_


# ---- the tables the N-field launches of a multi-component solver get (PressureSolver::mc_setup) --------------------------------
# mc_setup builds, for every batched depth, march_tiles(fused_shape(16, false), sizes) and march_tiles(resid_shape(false), sizes)
# + number_slots -- class-0 equal columns whatever the level's own tables hold.  The depth-0 boxes of three layouts of
# tests/test_gpu_multi.py, with the columns (i0, w) per box width written out (not recomputed): 256 -> three columns of 86, the
# last one 84 cells of box (the kernels cut it by the box, l < n0, not by w).
NFIELD_BOXES = {
    "extra-wide": [(256, 24, 24)],
    "ragged-mixed-sides": [(48, 48, 32), (48, 16, 32), (32, 16, 32), (32, 48, 32)],
    "ratio-112": [(32, 32, 32), (32, 32, 32)],
}
NFIELD_COLUMNS = {256: [(0, 86), (86, 86), (172, 86)], 48: [(0, 48)], 32: [(0, 32)]}


@pytest.mark.parametrize("table, rows", [("fused", 12), ("resid", 14)])
@pytest.mark.parametrize("layout", sorted(NFIELD_BOXES))
def test_tables_of_the_n_field_launches(planner, layout, table, rows):
    boxes = NFIELD_BOXES[layout]
    (count, _, classes), tiles = planner("table", table, 0, 0, *[n for b in boxes for n in b])
    assert classes == 0 and count == len(tiles) > 0
    cover = [np.zeros(b, dtype=np.int32) for b in boxes]
    for patch, i0, j0, k0, nk, w, cls, _slot in tiles:
        n0, n1, n2 = boxes[patch]
        assert cls == 0
        assert (i0, w) in NFIELD_COLUMNS[n0], (patch, i0, w)
        assert 0 <= i0 < n0 and 0 <= j0 < n1 and 0 <= k0 < n2 and nk > 0 and k0 + nk <= n2   # no empty tile, none past the box
        assert w <= 124 and j0 % rows == 0
        cover[patch][i0:min(i0 + w, n0), j0:min(j0 + rows, n1), k0:k0 + nk] += 1
        if table == "resid":
            # a coarse cell's two rows and two planes lie in one tile
            assert j0 % 2 == 0 and k0 % 2 == 0 and (nk % 2 == 0 or k0 + nk == n2)
    for patch, c in enumerate(cover):
        assert c.min() == 1 and c.max() == 1, (patch, int(c.min()), int(c.max()))
    for patch, (n0, _, _) in enumerate(boxes):
        assert sorted({(t[1], t[5]) for t in tiles if t[0] == patch}) == NFIELD_COLUMNS[n0]   # every column is there
    if table == "resid":
        assert [t[7] for t in tiles] == list(range(len(tiles)))   # the per-tile sums' slots: the table's own order
    else:
        assert {t[7] for t in tiles} == {0}
