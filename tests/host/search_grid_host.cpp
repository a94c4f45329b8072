// Host test of multimesh_amd/csrc/mm_search_grid.h (tests/test_search_grid_host.py builds and runs this; no HIP, no GPU):
// the fit of a search grid's edge to the caps of 1024 cells per axis and 2^22 in all.  The expected cells and numbers of
// x1.25 steps were computed by hand-transcribing the two loops that mm_cutoff_distance (pad 2) and mm_surface_distance
// (pad 1) had before they shared this function, not with the function itself.
#include <stdio.h>

#include "mm_search_grid.h"

static int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

struct Row {
    int pad;
    double extent[3], h0;
    int dims[3], steps;
};

static const double kMargin = 1.0 + 0x1p-30;   // mm_cutoff_distance's edge over its cutoff
static const Row kRows[] = {
    {2, {1.0, 1.0, 1.0}, 0.01 * kMargin, {101, 101, 101}, 0},
    {2, {1.0, 1.0, 1.0}, 0.004 * kMargin, {161, 161, 161}, 2},     // the cap on the cells in all
    {2, {1.0, 1.0, 1.0}, 0.0005 * kMargin, {139, 139, 139}, 12},
    {2, {1.0, 1.0, 0.0}, 0.0005 * kMargin, {821, 821, 2}, 4},      // the cap on the cells per axis
    {2, {1.0, 0.0, 0.0}, 0.0005 * kMargin, {821, 2, 2}, 4},
    {1, {1.0, 1.0, 1.0}, 0x1p-13, {148, 148, 148}, 18},
    {1, {1.0, 1.0, 0.0}, 0x1p-13, {880, 880, 1}, 10},
    {1, {1.0, 1.0, 1.0}, 0x1p-8, {132, 132, 132}, 3},
    {2, {0.0, 0.0, 0.0}, 0.0005 * kMargin, {2, 2, 2}, 0},          // a box that is a point
    {1, {0.0, 0.0, 0.0}, 0x1p-13, {1, 1, 1}, 0},
};

int main()
{
    for (const Row &r : kRows) {
        mm_search_grid g = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0.0, 0.0, {0, 0, 0}};
        const int steps = mm_search_grid_fit(g, r.extent, r.h0, r.pad);
        CHECK(steps == r.steps);
        CHECK(g.dims[0] == r.dims[0] && g.dims[1] == r.dims[1] && g.dims[2] == r.dims[2]);
        double h = r.h0;   // the edges tried: h0, then each 1.25 times the last
        for (int s = 0; s < r.steps; ++s) h *= 1.25;
        CHECK(g.h == h);
        CHECK(g.inv_h == 1.0 / g.h);
        CHECK(g.dims[0] <= mm_grid_max_dim && g.dims[1] <= mm_grid_max_dim && g.dims[2] <= mm_grid_max_dim);
        CHECK((long long)g.dims[0] * g.dims[1] * g.dims[2] <= mm_grid_max_cells);
        if (steps != r.steps || g.dims[0] != r.dims[0] || g.dims[1] != r.dims[1] || g.dims[2] != r.dims[2])
            printf("  pad %d h0 %.17g: %d x %d x %d after %d steps\n", r.pad, r.h0, g.dims[0], g.dims[1], g.dims[2], steps);
        // an edge that fits is never enlarged: the fit of its own result is that result
        mm_search_grid again = g;
        CHECK(mm_search_grid_fit(again, r.extent, g.h, r.pad) == 0);
        CHECK(again.h == g.h && again.inv_h == g.inv_h);
        CHECK(again.dims[0] == g.dims[0] && again.dims[1] == g.dims[1] && again.dims[2] == g.dims[2]);
    }
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("search grid: all checks passed\n");
    return 0;
}
