"""CPU: the straight-line tile-rectangle tightening (dss_amd/csrc/tile_rect.h, splat_tile_rect<false>) against the rolled
searches it replaces (splat_tile_rect<true>, kept in the source as the reference implementation).

The header is plain C++; the sweep below is compiled with the host compiler.  Equality is exact -- same verdict, and the same
four tile bounds whenever the verdict is "reaches the band" -- for every case of a dense sweep over centre and radius, image
sides {64, 100, 512, 513, 1024}, whole images, contiguous row bands and tile-row-cyclic bands, negative depth and non-finite
inputs.

Which path a case takes.  ndc_index_range leaves about one pixel of slack per side, so from its range a search stops within
the three candidates of the straight-line form whenever the result is not empty: through splat_tile_rect the loop behind the
candidates (the remainder) decides only between one empty range and another.  The remainder is therefore tested on its own:
splat_tighten -- the tightening, which is exact for ANY starting range -- is called with the range of ndc_index_range loosened
by 0..9 indices per end, so that searches of 4 and more steps end on a NON-empty range, and new form and rolled form must give
the same four indices.  The driver counts, on power-of-two sides only (the others never take the new form): search ends at which
the first candidate passes, ends of the splat_tile_rect sweep that need 4 or more steps, and loosened cases whose non-empty
result needed the remainder at the low end, at the high end.  `ref` mode compares the rolled form with itself (the harness alone
must pass)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "tile_rect.h"
#include <stdio.h>
#include <string.h>
#include <limits>
#include <vector>
using namespace dss;

static long long cases, mismatches, reach, ends_first, ends_loop, ends_total, loose_cases, loose_lo, loose_hi;

// steps of the rolled search from each end of one axis (the loops of splat_tighten, counted), from the range [lo, hi]
static void steps_from(float c, float r, int S, int lo, int hi, int &a, int &b, bool &empty)
{
    const NdcMap ndc(S);
    a = b = 0;
    while (lo <= hi && fabsf(ndc(lo) - c) > r) { ++lo; ++a; }
    while (hi >= lo && fabsf(ndc(hi) - c) > r) { --hi; ++b; }
    empty = lo > hi;
}
static void count_steps(float c, float r, int S)
{
    int lo, hi, a, b;
    bool empty;
    if ((S & (S - 1)) != 0 || !ndc_index_range(c, r, S, lo, hi)) return;
    steps_from(c, r, S, lo, hi, a, b, empty);
    ends_total += 2;
    ends_first += (a == 0) + (b == 0);
    ends_loop += (a >= 4) + (b >= 4);
}

// the tightening alone, from a range loosened by dl / dh indices (x axis) and dh / dl (y axis)
template <bool NEW_IS_ROLLED>
static void loose(float px, float py, float rx, float ry, int S, int dl, int dh)
{
    int xlo, xhi, ylo, yhi;
    if (!ndc_index_range(px, rx, S, xlo, xhi) || !ndc_index_range(py, ry, S, ylo, yhi)) return;
    xlo -= dl; xhi += dh; ylo -= dh; yhi += dl;
    int a[4] = {xlo, xhi, ylo, yhi}, b[4] = {xlo, xhi, ylo, yhi};
    splat_tighten<true>(px, py, rx, ry, S, a[0], a[1], a[2], a[3]);
    splat_tighten<NEW_IS_ROLLED>(px, py, rx, ry, S, b[0], b[1], b[2], b[3]);
    const bool ea = a[0] > a[1] || a[2] > a[3], eb = b[0] > b[1] || b[2] > b[3];
    ++cases; ++loose_cases;
    // (an axis that is not empty must agree index for index, whatever the other axis is)
    const bool bad = ea != eb || (a[0] <= a[1] && (a[0] != b[0] || a[1] != b[1])) || (a[2] <= a[3] && (a[2] != b[2] || a[3] != b[3]));
    if (bad) {
        if (mismatches < 5)
            fprintf(stderr, "MISMATCH (loosened) S=%d p=(%a,%a) r=(%a,%a) from [%d %d %d %d]: [%d %d %d %d] vs [%d %d %d %d]\n", S, px, py, rx,
                    ry, xlo, xhi, ylo, yhi, a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
        ++mismatches;
    }
    if ((S & (S - 1)) == 0) {
        int sa, sb;
        bool empty;
        steps_from(px, rx, S, xlo, xhi, sa, sb, empty);
        if (!empty) { loose_lo += sa >= 4; loose_hi += sb >= 4; }
        steps_from(py, ry, S, ylo, yhi, sa, sb, empty);
        if (!empty) { loose_lo += sa >= 4; loose_hi += sb >= 4; }
    }
}

template <bool NEW_IS_ROLLED>
static void one(float px, float py, float pz, float rx, float ry, const TileGrid &g)
{
    int a[4] = {-7, -7, -7, -7}, b[4] = {-7, -7, -7, -7};
    const bool ra = splat_tile_rect<true>(px, py, pz, rx, ry, g, a[0], a[1], a[2], a[3]);
    const bool rb = splat_tile_rect<NEW_IS_ROLLED>(px, py, pz, rx, ry, g, b[0], b[1], b[2], b[3]);
    ++cases;
    reach += ra;
    if (ra != rb || (ra && memcmp(a, b, sizeof a) != 0)) {
        if (mismatches < 5)
            fprintf(stderr, "MISMATCH S=%d row0=%d rows=%d tshift=%d p=(%a,%a,%a) r=(%a,%a): %d [%d %d %d %d] vs %d [%d %d %d %d]\n", g.S,
                    g.row0, g.rows, g.tshift, px, py, pz, rx, ry, ra, a[0], a[1], a[2], a[3], rb, b[0], b[1], b[2], b[3]);
        ++mismatches;
    }
}

static TileGrid grid(int S, int row0, int row1, int cycle)   // rows [row0, row1) of the image; cycle c: every c-th 8-row tile row
{
    TileGrid g;
    g.S = S; g.row0 = row0; g.tiles_x = (S + DSS_TILE - 1) / DSS_TILE; g.tshift = 3;
    if (cycle > 1) {
        int sh = 0;
        while ((1 << sh) < cycle) ++sh;
        g.tshift = 3 + sh;
        const int all_rows = (S + DSS_TILE - 1) / DSS_TILE, first = row0 / DSS_TILE;
        g.tiles_y = (all_rows - first + cycle - 1) / cycle;
        const int last_row0 = row0 + ((g.tiles_y - 1) << g.tshift);
        g.rows = (g.tiles_y - 1) * DSS_TILE + ((S - last_row0) < DSS_TILE ? (S - last_row0) : DSS_TILE);
    } else {
        g.rows = row1 - row0;
        g.tiles_y = (g.rows + DSS_TILE - 1) / DSS_TILE;
    }
    return g;
}

template <bool NEW_IS_ROLLED> static void sweep()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sides[] = {64, 100, 512, 513, 1024};
    for (int S : sides) {
        std::vector<TileGrid> grids;
        grids.push_back(grid(S, 0, S, 1));
        grids.push_back(grid(S, 8 * (S / 32), 8 * (S / 32) + S / 2, 1));        // contiguous band, tile aligned
        grids.push_back(grid(S, 8 * (S / 16), S, 1));                           // last band (short last tile row when S % 8 != 0)
        grids.push_back(grid(S, 0, S, 2));                                      // cyclic bands: rank 0 and rank 1 of 2, rank 3 of 4
        grids.push_back(grid(S, 8, S, 2));
        grids.push_back(grid(S, 24, S, 4));
        // centres: a dense walk across the image and its borders (an irrational step: every sub-pixel phase), radii from a
        // fraction of a pixel to several tiles
        std::vector<float> cs, rs;
        const float pix = 2.0f / S;
        for (int i = 0; i < 700; ++i) cs.push_back(-1.25f + 2.5f * (float)i / 700.0f + 0.000731f * (float)(i % 13));
        for (int i = -3; i <= 3; ++i) { cs.push_back(-1.0f + i * 0.5f * pix); cs.push_back(1.0f + i * 0.5f * pix); cs.push_back(i * 0.5f * pix); }
        const float rpix[] = {0.0f, 0.01f, 0.49f, 0.5f, 0.51f, 1.0f, 1.5f, 2.0f, 3.7f, 8.0f, 12.3f, 40.0f};
        for (float r : rpix) rs.push_back(r * pix);
        rs.push_back(0.75f); rs.push_back(3.0f);
        for (const TileGrid &g : grids) {
            for (size_t i = 0; i < cs.size(); ++i)
                for (size_t j = 0; j < rs.size(); ++j) {
                    // x sweeps with y fixed at a few places, y sweeps with x fixed: every (centre, radius) pair on both axes
                    const float other[] = {-0.9f, 0.013f, 0.77f};
                    for (float o : other) {
                        one<NEW_IS_ROLLED>(cs[i], o, 1.0f, rs[j], rs[(j + 5) % rs.size()], g);
                        one<NEW_IS_ROLLED>(o, cs[i], 1.0f, rs[(j + 3) % rs.size()], rs[j], g);
                    }
                    if (g.row0 == 0 && g.tshift == 3) {
                        count_steps(cs[i], rs[j], S);
                        if (i % 7 == 0)
                            for (int d = 0; d < 10; ++d) {
                                loose<NEW_IS_ROLLED>(cs[i], 0.013f, rs[j], rs[(j + 5) % rs.size()], S, d, (d * 7 + 3) % 10);
                                loose<NEW_IS_ROLLED>(0.77f, cs[i], rs[(j + 3) % rs.size()], rs[j], S, (d * 3 + 1) % 10, d);
                            }
                    }
                }
            // large magnitudes (the conservative range is computed with cancellation there); every non-finite input; negative depth
            const float big[] = {1e3f, 3e4f, 1e5f, 1e6f, 1.6e7f, 1e9f, 1e30f};
            for (float m : big)
                for (int s = -1; s <= 1; s += 2)
                    for (int k = -40; k <= 40; ++k) {
                        const float c = s * m, r = m + (float)k * 0.05f * (m > 1e5f ? m * 1e-6f : 1.0f);
                        one<NEW_IS_ROLLED>(c, 0.1f, 1.0f, r, 0.3f, g);
                        one<NEW_IS_ROLLED>(-0.2f, c, 1.0f, 0.2f, r, g);
                        one<NEW_IS_ROLLED>(c, -c, 0.0f, r, r, g);
                        if (g.row0 == 0 && g.tshift == 3) count_steps(c, r, S);
                    }
            const float odd[] = {nan, inf, -inf, 0.0f, -0.0f, 0.3f, -1.0f, 1e38f, -1e38f, 1e-40f};
            for (float px : odd) for (float py : odd) for (float rx : odd) for (float ry : odd) {
                one<NEW_IS_ROLLED>(px, py, 1.0f, rx, ry, g);
                one<NEW_IS_ROLLED>(px, py, -1.0f, rx, ry, g);
                one<NEW_IS_ROLLED>(px, py, nan, rx, ry, g);
            }
        }
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "ref")) sweep<true>(); else sweep<false>();
    printf("{\"cases\": %lld, \"mismatches\": %lld, \"reach\": %lld, \"ends\": %lld, \"ends_first_candidate\": %lld, \"ends_4_steps\": %lld, "
           "\"loosened\": %lld, \"loosened_low_end_in_loop\": %lld, \"loosened_high_end_in_loop\": %lld}\n",
           cases, mismatches, reach, ends_total, ends_first, ends_loop, loose_cases, loose_lo, loose_hi);
    return mismatches != 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_rect")
    src, exe = str(d / "sweep.cpp"), str(d / "sweep")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "dss_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_sweep_harness_passes_on_the_rolled_reference_alone(driver):
    d = _run(driver, "ref")
    assert d["mismatches"] == 0 and d["cases"] > 1_000_000


def test_straight_line_rectangle_equals_the_rolled_searches_on_every_case(driver):
    d = _run(driver)
    print(d)
    assert d["mismatches"] == 0 and d["cases"] > 1_000_000
    assert 0 < d["reach"] < d["cases"]                        # both verdicts
    assert d["ends_first_candidate"] > 0.2 * d["ends"]        # "first candidate passes" ...
    # ... and "falls through to the loop", with a non-empty result that depends on it, at either end
    assert d["loosened"] > 100_000 and d["loosened_low_end_in_loop"] > 10_000 and d["loosened_high_end_in_loop"] > 10_000
