"""The marching kernels' tile plan (somar_amd/csrc/march_plan.h) from a stand-alone host program: the header is plain C++, so
the decompositions Level::build_march_tiles gets from it can be checked without a GPU.  Today's columns are pinned (they are
also what tests/helpers.march_columns restates), and the tall (all class-1) plan of the fused sweep's table is checked for
what the kernel relies on: every cell in exactly one tile, even column starts, at most 60 output columns, 28 rows per tile,
even k-chunks."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import march_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "somar_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include "march_plan.h"
using namespace somar::march_plan;

// cols N0 CLASSES                -> "w cls" per column of the residual / fused tables (FT_I 124, min_gain 0.85)
// plan TALL N0 N1 N2             -> "nch extra" of the fused sweep's table, then "i0 w cls j0 rows k0 nk" per tile
// eligible ROWS UNIFORM N0 [N0 ...] -> 0 / 1
int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    Shape s;
    s.FT_I = 124; s.region_rows = 16; s.hrows = 4; s.halo = 3.0; s.slots = 256; s.min_gain = 0.85;
    if (what == "cols") {
        s.hrows = 2; s.halo = 2.0;
        s.classes = std::atoi(argv[3]) != 0;
        for (const ColSpec& c : columns(s, std::atoi(argv[2]))) std::printf("%d %d\n", c.w, c.cls);
        return 0;
    }
    if (what == "plan") {
        const bool tall = std::atoi(argv[2]) != 0;
        const BoxSize b{std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5])};
        const std::vector<BoxSize> boxes{b};
        const Plan p = plan(s, boxes, tall);
        std::printf("%d %d\n", p.nch, p.extra);
        const int nk = chunk_planes(b.n2, p.nch);
        const std::vector<ColSpec> cs = p.extra >= 0 ? tall_columns(b.n0, p.extra) : columns(s, b.n0);
        for (int k0 = 0; k0 < b.n2; k0 += nk)
            for (const ColSpec& c : cs)
                for (int j0 = 0; j0 < b.n1; j0 += rows_of(s, c.cls))
                    std::printf("%d %d %d %d %d %d %d\n", c.i0, c.w, c.cls, j0, rows_of(s, c.cls), k0, std::min(nk, b.n2 - k0));
        return 0;
    }
    if (what == "eligible") {
        std::vector<BoxSize> boxes;
        for (int a = 4; a < argc; ++a) boxes.push_back({std::atoi(argv[a]), 64, 64});
        std::printf("%d\n", tall_eligible(boxes, std::atoi(argv[2]), std::atoi(argv[3]) != 0) ? 1 : 0);
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
        return [tuple(int(x) for x in line.split()) for line in out.splitlines()]
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
