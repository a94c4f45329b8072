// The uniform search grid of mm_cutoff_distance (points in cells) and mm_surface_distance (triangles in the cells of
// their bounding boxes), and the fit of its edge to the caps.  No HIP: tests/host/search_grid_host.cpp compiles this with
// g++ alone.  The kernels' side -- the cell of a coordinate, the linear index, the bin build -- is in mm_boundary_parts.h.
#pragma once

#include <math.h>

constexpr int mm_grid_max_dim = 1024;                   // cells per axis of a search grid
constexpr long long mm_grid_max_cells = 1ll << 22;      // ... and in all

// Cells of edge h over the box [lo, hi] of the items: dims[a] of them on axis a, inv_h = 1 / h.  mbox, the largest
// |coordinate| of the box, is the surface walk's; the cutoff search leaves it zero and reads lo, inv_h and dims only.
struct mm_search_grid {
    double lo[3], hi[3], h, inv_h, mbox;
    int dims[3];
};

// The least edge h0 * 1.25^s, s = 0, 1, ..., at which the grid over `extent` fits both caps, with dims[a] =
// floor(fl(extent[a] * inv_h)) + pad: pad = 2 where the targets' cells reach one past the sources' on either side
// (mm_cutoff_distance), 1 where every item lies in the box (mm_surface_distance).  Fills h, inv_h and dims; returns s.  A
// larger edge keeps either search valid, so the caps never refuse a call.  extent: finite, >= 0; h0 > 0.
inline int mm_search_grid_fit(mm_search_grid &g, const double (&extent)[3], double h0, int pad)
{
    for (int steps = 0;; ++steps, h0 *= 1.25) {
        g.h = h0;
        g.inv_h = 1.0 / h0;
        double cells = 1.0;
        bool fits = true;
        for (int a = 0; a < 3; ++a) {
            const double da = floor(extent[a] * g.inv_h) + (double)pad;
            fits = fits && da <= (double)mm_grid_max_dim;
            g.dims[a] = fits ? (int)da : 1;
            cells *= da;
        }
        if (fits && cells <= (double)mm_grid_max_cells) return steps;
    }
}
