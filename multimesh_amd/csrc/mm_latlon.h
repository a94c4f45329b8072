// What the kernels that place a point on a latitude x longitude map share, stated once: mm_sample_grid and mm_grid_operator
// (mm_grid_sample.hip) and mm_layered_model_apply (mm_layered.hip).  The statement is published in include/multimesh_hip.h
// (mm_sample_grid); every product, quotient and sum is rounded on its own (-ffp-contract=off), the only libm calls are acos
// and atan2.
//   lat_lon_depth   r = mm_norm3(x, y, z), depth = 6371000 - r, lat = 90 - acos(r > 0 ? z / r : 0) * (180 / pi),
//                   lon = atan2(y, x) * (180 / pi), wrapped once into [lon0, lon0 + 360) on a periodic axis
//   find_cell       i = clip(upper_bound(a, v) - 1, 0, n - 2), t = (v - a[i]) / (a[i + 1] - a[i]); a length-1 axis is constant
#pragma once

#include "mm_stream.h"

namespace mm_latlon {

constexpr int kAxisLds = 2048;      // doubles of LDS for a kernel's axes together (16 KiB: eight workgroups per CU)
constexpr double kEarthRadius = 6371000.0;
constexpr double kRadToDeg = 180.0 / 3.14159265358979323846;

struct Cell {
    int i, i1;
    double t;
    bool inside;
};

// np.searchsorted(a, v, side="right") - 1 clipped to [0, n - 2], and the weight in that cell.  NaN is outside (and, in
// clamp mode, stays NaN: the comparisons are all false for it, so it sorts behind the last node as in NumPy).
__device__ __forceinline__ Cell find_cell(const double *a, int n, double v, bool clamp)
{
    Cell c = {0, 0, 0.0, true};
    if (n == 1) return c;
    const double lo = a[0], hi = a[n - 1];
    if (clamp) {
        v = v < lo ? lo : v;
        v = v > hi ? hi : v;
    } else {
        c.inside = v >= lo && v <= hi;
        if (!c.inside) return c;
    }
    int i = mm_upper_bound(a, 0, n, v) - 1;
    i = i < 0 ? 0 : i;
    i = i > n - 2 ? n - 2 : i;
    c.i = i;
    c.i1 = i + 1;
    c.t = (v - a[i]) / (a[i + 1] - a[i]);
    return c;
}

// (lat, lon, depth) of the point (x, y, z); lon0: the first node of the longitude axis (read on a periodic axis only)
__device__ __forceinline__ void lat_lon_depth(double x, double y, double z, double lon0, int lon_periodic, double &lat,
                                              double &lon, double &depth)
{
    const double r = mm_norm3(x, y, z);
    depth = kEarthRadius - r;
    const double c = r > 0.0 ? z / r : 0.0;
    lat = 90.0 - acos(c) * kRadToDeg;
    lon = atan2(y, x) * kRadToDeg;
    if (lon_periodic) {
        if (lon < lon0) lon += 360.0;
        if (lon >= lon0 + 360.0) lon -= 360.0;
    }
}

}  // namespace mm_latlon
