"""CPU: the screen-cell grid and key of the render's counting sort (dss_amd/csrc/cell_sort.h) against the two forms they
replaced -- `make_cells` and the key lines of `cell_hist_kernel` (raster_backward.hip), `make_sort_grid` and the key lines of
`setup_cell_kernel` (raster_forward.hip) --, transcribed into the driver below as the "old" forms.

A wrong key changes no rendered value (the order of the sorted entries is free), it only costs locality: no GPU test would
fail, so the rule is pinned here.  The header's first part is plain C++; the driver is compiled with the host compiler against
the header alone.  Equality is exact:
  * make_cell_grid(N, S, 0) == make_cells(N, S) and make_cell_grid(N, S, 1) == make_sort_grid(N, S) for N in 1..64 and twelve
    image sides, and by value on the edge N * (S / 32)^2 = 16384, where the extra cell of the forward moves the step to
    64-pixel cells and the backward stays at 32;
  * screen_cell == the old key lines on a dense sweep of [-1.5, 1.5]^2 (finite values only: (int)NaN is undefined on the host;
    the device's value, cell 0, is what the GPU tests of the cell-ordered paths rely on) with +-1 exactly and the pixel edges
    of S = 100 and S = 512 with their fp32 neighbours, for every grid the first sweep produced; every key lies in front of the
    extra cells, belongs to the camera it was asked for, and the map is monotone (ix does not increase with px, iy not with
    py)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "cell_sort.h"
#include <math.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <set>
#include <tuple>
#include <vector>
using namespace dss;

// ---- the old forms (parent of the commit that added cell_sort.h), transcribed
struct OldGrid { int shift, cx, cy, total; };
static OldGrid old_make_cells(int N, int S)          // raster_backward.hip
{
    OldGrid c;
    c.shift = 5;
    for (;;) {
        c.cx = ((S - 1) >> c.shift) + 1;
        c.cy = c.cx;
        c.total = N * c.cx * c.cy;
        if (c.total <= 16384 || c.shift >= 14) break;
        ++c.shift;
    }
    return c;
}
static OldGrid old_make_sort_grid(int N, int S)      // raster_forward.hip
{
    OldGrid c;
    c.shift = 5;
    for (;;) {
        c.cx = ((S - 1) >> c.shift) + 1;
        c.cy = c.cx;
        c.total = N * c.cx * c.cy + 1;
        if (c.total <= 16384 || c.shift >= 14) break;
        ++c.shift;
    }
    return c;
}
static uint32_t old_key(float px, float py, int n, int S, const OldGrid &cg)   // cell_hist_kernel == setup_cell_kernel
{
    const float fx = (1.0f - px) * 0.5f * (float)S, fy = (1.0f - py) * 0.5f * (float)S;
    const int ix = std::min(std::max((int)fx, 0), S - 1) >> cg.shift, iy = std::min(std::max((int)fy, 0), S - 1) >> cg.shift;
    return (uint32_t)((n * cg.cy + iy) * cg.cx + ix);
}

static long long grid_cases, grid_mismatches, key_cases, key_mismatches, key_out_of_range, key_wrong_camera, not_monotone;
static bool same(const CellGrid &a, const OldGrid &b) { return a.shift == b.shift && a.cx == b.cx && a.cy == b.cy && a.total == b.total; }

// one line of keys along x (py fixed) or along y (px fixed): `vals` ascending
static void line(const std::vector<float> &vals, float fixed, bool along_x, int n, int S, const CellGrid &g, int extra)
{
    const OldGrid og = {g.shift, g.cx, g.cy, g.total};
    int last = 1 << 30;
    for (float v : vals) {
        const float px = along_x ? v : fixed, py = along_x ? fixed : v;
        const uint32_t k = screen_cell(px, py, n, S, g);
        ++key_cases;
        key_mismatches += k != old_key(px, py, n, S, og);
        key_out_of_range += !(k < (uint32_t)(g.total - extra));
        const int ix = (int)(k % (uint32_t)g.cx), iy = (int)(k / (uint32_t)g.cx % (uint32_t)g.cy), cam = (int)(k / (uint32_t)(g.cx * g.cy));
        key_wrong_camera += cam != n;
        const int moving = along_x ? ix : iy;
        not_monotone += moving > last;
        last = moving;
    }
}

int main()
{
    const int sides[] = {1, 31, 32, 33, 64, 100, 512, 513, 1024, 2048, 4096, 8192};
    std::map<std::tuple<int, int, int>, int> grids;   // (S, extra, shift) -> the largest N with that cell side
    std::set<int> shifts;
    for (int S : sides)
        for (int N = 1; N <= 64; ++N)
            for (int extra = 0; extra <= 1; ++extra) {
                const CellGrid g = make_cell_grid(N, S, extra);
                ++grid_cases;
                grid_mismatches += !same(g, extra ? old_make_sort_grid(N, S) : old_make_cells(N, S));
                shifts.insert(g.shift);
                grids[std::make_tuple(S, extra, g.shift)] = N;
            }
    // the edge N * (S / 32)^2 = 16384, by value
    const int edge[][3] = {{16, 1024, 0}, {16, 1024, 1}, {1, 4096, 0}, {1, 4096, 1}, {17, 1024, 0}};
    printf("{\"edges\": [");
    for (int i = 0; i < 5; ++i) {
        const CellGrid g = make_cell_grid(edge[i][0], edge[i][1], edge[i][2]);
        printf("%s[%d, %d, %d, %d, %d]", i ? ", " : "", edge[i][0], edge[i][1], edge[i][2], g.shift, g.total);
    }
    printf("], ");

    // coordinates: a dense walk over [-1.5, 1.5] (an irrational step: every sub-pixel phase), +-1 and 0 exactly, the pixel
    // edges of S = 100 and S = 512 with their fp32 neighbours
    std::vector<float> vals;
    for (int i = 0; i <= 1500; ++i) vals.push_back(std::min(1.5f, -1.5f + 3.0f * (float)i / 1500.0f + 0.000731f * (float)(i % 13)));
    vals.push_back(-1.5f); vals.push_back(1.5f); vals.push_back(-1.0f); vals.push_back(1.0f); vals.push_back(0.0f);
    for (int S : {100, 512})
        for (int k = 0; k <= S; ++k) {
            const float e = 1.0f - 2.0f * (float)k / (float)S;
            vals.push_back(e); vals.push_back(nextafterf(e, -2.0f)); vals.push_back(nextafterf(e, 2.0f));
        }
    std::sort(vals.begin(), vals.end());
    vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    std::vector<float> fixed;
    for (size_t i = 0; i < vals.size(); i += 37) fixed.push_back(vals[i]);
    fixed.push_back(-1.0f); fixed.push_back(1.0f); fixed.push_back(1.5f);
    for (const auto &t : grids) {
        const int S = std::get<0>(t.first), extra = std::get<1>(t.first), N = t.second;
        const CellGrid g = make_cell_grid(N, S, extra);
        for (int n : {0, N / 2, N - 1})
            for (float f : fixed) {
                line(vals, f, true, n, S, g, extra);
                line(vals, f, false, n, S, g, extra);
            }
    }
    printf("\"grid_cases\": %lld, \"grid_mismatches\": %lld, \"grids_swept\": %d, \"shifts\": %d, \"key_cases\": %lld, \"key_mismatches\": %lld, "
           "\"key_out_of_range\": %lld, \"key_wrong_camera\": %lld, \"not_monotone\": %lld}\n",
           grid_cases, grid_mismatches, (int)grids.size(), (int)shifts.size(), key_cases, key_mismatches, key_out_of_range,
           key_wrong_camera, not_monotone);
    return 0;
}
"""


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    d = tmp_path_factory.mktemp("cell_sort")
    src, exe = str(d / "sweep.cpp"), str(d / "sweep")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "dss_amd", "csrc"), src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(d)
    return d


def test_one_grid_rule_equals_both_old_loops(result):
    assert result["grid_cases"] == 12 * 64 * 2 and result["grid_mismatches"] == 0


def test_grid_edge_where_the_extra_cell_moves_the_step(result):
    # (N, S, extra cells, shift, total): at N * (S / 32)^2 = 16384 the backward keeps 32-pixel cells, the forward takes 64
    assert result["edges"] == [[16, 1024, 0, 5, 16384], [16, 1024, 1, 6, 4097], [1, 4096, 0, 5, 16384], [1, 4096, 1, 6, 4097],
                               [17, 1024, 0, 6, 4352]]


def test_screen_cell_equals_the_old_key_lines_and_is_monotone(result):
    assert result["shifts"] >= 4 and result["grids_swept"] >= 2 * 12      # every shift the grid sweep produced, both forms
    assert result["key_cases"] > 10_000_000
    assert result["key_mismatches"] == 0
    assert result["key_out_of_range"] == 0 and result["key_wrong_camera"] == 0
    assert result["not_monotone"] == 0
