// A regular latitude x longitude x depth grid sampled at arbitrary points: the import direction of the regular-grid
// drivers (mm_sample_columns_gll is the extract direction).  One lane per point in a grid-stride loop:
//
//   r = mm_norm3(x, y, z)    depth = 6371000 - r    lat = 90 - acos(r > 0 ? z / r : 0) * (180 / pi)
//   lon = atan2(y, x) * (180 / pi), wrapped once into [lon[0], lon[0] + 360) on a periodic axis
//   per axis: i = clip(upper_bound(a, v) - 1, 0, n - 2), t = (v - a[i]) / (a[i + 1] - a[i]); a length-1 axis is constant
//   value = lerp over longitude (4), then latitude (2), then depth (1), by mm_lerp(t, p, q)
//
// Every product, quotient and sum is rounded on its own (the library is built with -ffp-contract=off), so the values are
// bit for bit the NumPy statement of include/multimesh_hip.h evaluated on the (lat, lon, depth) this kernel computed;
// those depend on the device's acos and atan2 and are what latlondepth_out_d hands back.
//
// Traffic: 24 B read + 8 B per component written per point, plus the eight corners per component, which neighbouring
// points share (mesh points are ordered in space, so a wave's corners sit in a few cache lines of a cube that is small
// beside the points).  The axes are staged in LDS when the three together fit kAxisLds doubles and bisected there;
// longer axes are bisected in global memory.  The outside count is an integer sum (mm_count_to): it does not depend on the
// order of arrival.
//
// mm_grid_operator is the same import written as an operator: the (lat, lon, depth), the wrap and the three cells are those
// of mm_sample_grid (point_cells below, which both kernels call), and instead of the values the lane writes the eight
// corners' flat cube indices and trilinear weights, ids[n][8] / w[n][8] with corner c = 4a + 2b + e over (k|k1, j|j1, i|i1)
// and w = (u(tz, a) * u(ty, b)) * u(tx, e), u(t, 0) = 1.0 - t, u(t, 1) = t: rows mm_gather and mm_transpose_* take.
// Traffic: 24 B read and 128 B written per point; a lane owns one 64-byte row of each array and writes it with four
// 16-byte stores when both arrays start on 16 bytes, else with eight 8-byte stores (the same bits).
#include "mm_latlon.h"   // Cell, find_cell and (lat, lon, depth) of a point: shared with mm_layered.hip

#include <limits.h>

namespace {

using mm_stream::kThreads;
using mm_stream::kMaxBlocks;
using mm_latlon::kAxisLds;   // doubles of LDS for the three axes together
using mm_latlon::Cell;
using mm_latlon::find_cell;

enum { kFill = 0, kClamp = 1, kKeep = 2 };

struct GridArgs {
    const double *points;
    i64 npoints;
    const double *depth, *lat, *lon;
    int ndepth, nlat, nlon;
    const double *grid;
    int ncomp;
    int lon_periodic, mode;
    double fill;
    double *out, *lld;
    unsigned long long *outside;
};

// What mm_sample_grid and mm_grid_operator compute per point before they part, stated once: (lat, lon, depth) of point p,
// the periodic wrap, the coordinates handed back through lld when it is not null, and the cell on every axis.  Returns
// whether the point is inside the grid (always, in clamp mode).
__device__ __forceinline__ bool point_cells(const double *points, i64 p, const double *depth_a, int nd, const double *lat_a,
                                            int nla, const double *lon_a, int nlo, double lon0, int lon_periodic, bool clamp,
                                            double *lld, Cell &cd, Cell &ca, Cell &co)
{
    double lat, lon, depth;
    mm_latlon::lat_lon_depth(points[3 * p], points[3 * p + 1], points[3 * p + 2], lon0, lon_periodic, lat, lon, depth);
    if (lld) {
        lld[3 * p] = lat;
        lld[3 * p + 1] = lon;
        lld[3 * p + 2] = depth;
    }
    cd = find_cell(depth_a, nd, depth, clamp);
    ca = find_cell(lat_a, nla, lat, clamp);
    co = find_cell(lon_a, nlo, lon, clamp);
    return cd.inside && ca.inside && co.inside;
}

// The three axes in LDS (s_axes: kAxisLds doubles), depth first: every lane of the workgroup calls it
__device__ __forceinline__ void stage_axes(double *s_axes, const double *depth, int nd, const double *lat, int nla,
                                           const double *lon, int nlo)
{
    for (int q = threadIdx.x; q < nd + nla + nlo; q += kThreads)
        s_axes[q] = q < nd ? depth[q] : (q < nd + nla ? lat[q - nd] : lon[q - nd - nla]);
    __syncthreads();
}

__device__ __forceinline__ double sample_one(const double *__restrict__ g, i64 row, i64 plane, const Cell &cd,
                                             const Cell &ca, const Cell &co)
{
    const double *g0 = g + (i64)cd.i * plane, *g1 = g + (i64)cd.i1 * plane;
    const i64 r0 = (i64)ca.i * row, r1 = (i64)ca.i1 * row;
    const double a00 = mm_lerp(co.t, g0[r0 + co.i], g0[r0 + co.i1]);
    const double a01 = mm_lerp(co.t, g0[r1 + co.i], g0[r1 + co.i1]);
    const double a10 = mm_lerp(co.t, g1[r0 + co.i], g1[r0 + co.i1]);
    const double a11 = mm_lerp(co.t, g1[r1 + co.i], g1[r1 + co.i1]);
    return mm_lerp(cd.t, mm_lerp(ca.t, a00, a01), mm_lerp(ca.t, a10, a11));
}

// NC: components unrolled (1..4), 0: a loop over args.ncomp.  LDS_AXES: the axes are copied to LDS first.
template <int NC, bool LDS_AXES>
__global__ __launch_bounds__(kThreads) void grid_sample_kernel(const GridArgs args)
{
    __shared__ double s_axes[LDS_AXES ? kAxisLds : 1];

    const int nd = args.ndepth, nla = args.nlat, nlo = args.nlon;
    const double *depth_a = args.depth, *lat_a = args.lat, *lon_a = args.lon;
    if (LDS_AXES) {
        stage_axes(s_axes, args.depth, nd, args.lat, nla, args.lon, nlo);
        depth_a = s_axes;
        lat_a = s_axes + nd;
        lon_a = s_axes + nd + nla;
    }
    const int ncomp = NC ? NC : args.ncomp;
    const i64 row = nlo, plane = (i64)nla * nlo, cube = plane * nd, n = args.npoints;
    const bool clamp = args.mode == kClamp;
    const double lon0 = lon_a[0];
    unsigned outside = 0;

    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        Cell cd, ca, co;
        const bool inside = point_cells(args.points, p, depth_a, nd, lat_a, nla, lon_a, nlo, lon0, args.lon_periodic, clamp,
                                        args.lld, cd, ca, co);
        if (inside) {
            if (NC) {
#pragma unroll
                for (int q = 0; q < NC; ++q) args.out[q * n + p] = sample_one(args.grid + q * cube, row, plane, cd, ca, co);
            } else {
                for (int q = 0; q < ncomp; ++q) args.out[q * n + p] = sample_one(args.grid + q * cube, row, plane, cd, ca, co);
            }
        } else {
            ++outside;
            if (args.mode == kFill)
                for (int q = 0; q < ncomp; ++q) args.out[q * n + p] = args.fill;
        }
    }
    mm_count_to(args.outside, outside);
}

template <bool LDS_AXES>
void launch(mm_context *ctx, const GridArgs &a, unsigned grid)
{
    switch (a.ncomp) {
    case 1: hipLaunchKernelGGL((grid_sample_kernel<1, LDS_AXES>), dim3(grid), dim3(kThreads), 0, ctx->stream, a); break;
    case 2: hipLaunchKernelGGL((grid_sample_kernel<2, LDS_AXES>), dim3(grid), dim3(kThreads), 0, ctx->stream, a); break;
    case 3: hipLaunchKernelGGL((grid_sample_kernel<3, LDS_AXES>), dim3(grid), dim3(kThreads), 0, ctx->stream, a); break;
    case 4: hipLaunchKernelGGL((grid_sample_kernel<4, LDS_AXES>), dim3(grid), dim3(kThreads), 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL((grid_sample_kernel<0, LDS_AXES>), dim3(grid), dim3(kThreads), 0, ctx->stream, a); break;
    }
}

struct OperatorArgs {
    const double *points;
    i64 npoints;
    const double *depth, *lat, *lon;
    int ndepth, nlat, nlon;
    int lon_periodic, clamp;
    i64 *ids;
    double *w, *lld;
    unsigned long long *outside;
};

// LDS_AXES as above.  WIDE: ids and w both start on 16 bytes and a row goes out as four longlong2 / double2; else as eight
// single entries.
template <bool LDS_AXES, bool WIDE>
__global__ __launch_bounds__(kThreads) void grid_operator_kernel(const OperatorArgs args)
{
    __shared__ double s_axes[LDS_AXES ? kAxisLds : 1];

    const int nd = args.ndepth, nla = args.nlat, nlo = args.nlon;
    const double *depth_a = args.depth, *lat_a = args.lat, *lon_a = args.lon;
    if (LDS_AXES) {
        stage_axes(s_axes, args.depth, nd, args.lat, nla, args.lon, nlo);
        depth_a = s_axes;
        lat_a = s_axes + nd;
        lon_a = s_axes + nd + nla;
    }
    const i64 n = args.npoints;
    const bool clamp = args.clamp != 0;
    const double lon0 = lon_a[0];
    unsigned outside = 0;

    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        Cell cd, ca, co;
        const bool inside = point_cells(args.points, p, depth_a, nd, lat_a, nla, lon_a, nlo, lon0, args.lon_periodic, clamp,
                                        args.lld, cd, ca, co);
        i64 id[8];
        double wt[8];
        if (inside) {
            const double uz[2] = {1.0 - cd.t, cd.t}, uy[2] = {1.0 - ca.t, ca.t}, ux[2] = {1.0 - co.t, co.t};
            const int kk[2] = {cd.i, cd.i1}, jj[2] = {ca.i, ca.i1}, ii[2] = {co.i, co.i1};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int a = c >> 2, b = (c >> 1) & 1, e = c & 1;
                id[c] = ((i64)kk[a] * nla + jj[b]) * nlo + ii[e];
                wt[c] = (uz[a] * uy[b]) * ux[e];
            }
        } else {
            ++outside;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                id[c] = 0;
                wt[c] = 0.0;
            }
        }
        if (WIDE) {
            longlong2 *i2 = reinterpret_cast<longlong2 *>(args.ids + p * 8);
            double2 *w2 = reinterpret_cast<double2 *>(args.w + p * 8);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                i2[q] = make_longlong2(id[2 * q], id[2 * q + 1]);
                w2[q] = make_double2(wt[2 * q], wt[2 * q + 1]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                args.ids[p * 8 + c] = id[c];
                args.w[p * 8 + c] = wt[c];
            }
        }
    }
    mm_count_to(args.outside, outside);
}

template <bool LDS_AXES>
void launch_operator(mm_context *ctx, const OperatorArgs &a, unsigned grid)
{
    if (((reinterpret_cast<uintptr_t>(a.ids) | reinterpret_cast<uintptr_t>(a.w)) & 15) == 0)
        hipLaunchKernelGGL((grid_operator_kernel<LDS_AXES, true>), dim3(grid), dim3(kThreads), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((grid_operator_kernel<LDS_AXES, false>), dim3(grid), dim3(kThreads), 0, ctx->stream, a);
}

}  // namespace

extern "C" int64_t mm_grid_operator(mm_context *ctx, const double *points_d, int64_t npoints, const double *depth_d,
                                    int64_t ndepth, const double *lat_d, int64_t nlat, const double *lon_d, int64_t nlon,
                                    int lon_periodic, int clamp, int64_t *ids_d, double *w_d, double *latlondepth_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(npoints >= 0, "negative size");
    MM_REQUIRE(depth_d && lat_d && lon_d, "null axis");
    MM_REQUIRE(ndepth >= 1 && nlat >= 1 && nlon >= 1, "every axis needs at least one node");
    MM_REQUIRE((ids_d && w_d) || npoints == 0, "null ids or weights");
    MM_REQUIRE(points_d != nullptr || npoints == 0, "null points");
    if (ndepth > INT_MAX || nlat > INT_MAX || nlon > INT_MAX || npoints >= ((i64)1 << 58) ||
        ndepth > LLONG_MAX / nlat / nlon) {
        mm_set_error(MM_ERR_UNSUPPORTED, "mm_grid_operator: an axis, the cube or the point count is out of range");
        return MM_ERR_UNSUPPORTED;
    }
    if (npoints == 0) return 0;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    unsigned long long *counter = mm_counters_begin(ctx, 0, 1);
    if (!counter) return MM_ERR_HIP;
    OperatorArgs a;
    a.points = points_d;
    a.npoints = npoints;
    a.depth = depth_d;
    a.lat = lat_d;
    a.lon = lon_d;
    a.ndepth = (int)ndepth;
    a.nlat = (int)nlat;
    a.nlon = (int)nlon;
    a.lon_periodic = lon_periodic ? 1 : 0;
    a.clamp = clamp ? 1 : 0;
    a.ids = reinterpret_cast<i64 *>(ids_d);
    a.w = w_d;
    a.lld = latlondepth_out_d;
    a.outside = counter;
    const unsigned grid = mm_blocks(npoints, kThreads, kMaxBlocks);
    if (ndepth + nlat + nlon <= kAxisLds)
        launch_operator<true>(ctx, a, grid);
    else
        launch_operator<false>(ctx, a, grid);
    const i64 *count = mm_counters_end(ctx, 0, 1);
    return count ? count[0] : MM_ERR_HIP;
}

extern "C" int64_t mm_sample_grid(mm_context *ctx, const double *points_d, int64_t npoints, const double *depth_d,
                                  int64_t ndepth, const double *lat_d, int64_t nlat, const double *lon_d, int64_t nlon,
                                  const double *grid_d, int64_t ncomp, int lon_periodic, int outside_mode,
                                  double fill_value, double *out_d, double *latlondepth_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(npoints >= 0 && ncomp >= 0, "negative size");
    MM_REQUIRE(depth_d && lat_d && lon_d, "null axis");
    MM_REQUIRE(ndepth >= 1 && nlat >= 1 && nlon >= 1, "every axis needs at least one node");
    MM_REQUIRE(outside_mode == kFill || outside_mode == kClamp || outside_mode == kKeep, "outside_mode must be 0, 1 or 2");
    MM_REQUIRE(ncomp == 0 || (grid_d && (out_d || npoints == 0)), "null grid or output");
    MM_REQUIRE(points_d != nullptr || npoints == 0, "null points");
    if (ndepth > INT_MAX || nlat > INT_MAX || nlon > INT_MAX || ncomp > INT_MAX || npoints >= ((i64)1 << 58) ||
        (ncomp > 0 && npoints > LLONG_MAX / 8 / ncomp)) {
        mm_set_error(MM_ERR_UNSUPPORTED, "mm_sample_grid: an axis, the component count or the point count is out of range");
        return MM_ERR_UNSUPPORTED;
    }
    if (npoints == 0) return 0;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    unsigned long long *counter = mm_counters_begin(ctx, 0, 1);
    if (!counter) return MM_ERR_HIP;
    GridArgs a;
    a.points = points_d;
    a.npoints = npoints;
    a.depth = depth_d;
    a.lat = lat_d;
    a.lon = lon_d;
    a.ndepth = (int)ndepth;
    a.nlat = (int)nlat;
    a.nlon = (int)nlon;
    a.grid = grid_d;
    a.ncomp = (int)ncomp;
    a.lon_periodic = lon_periodic ? 1 : 0;
    a.mode = outside_mode;
    a.fill = fill_value;
    a.out = out_d;
    a.lld = latlondepth_out_d;
    a.outside = counter;
    const unsigned grid = mm_blocks(npoints, kThreads, kMaxBlocks);
    if (ndepth + nlat + nlon <= kAxisLds)
        launch<true>(ctx, a, grid);
    else
        launch<false>(ctx, a, grid);
    const i64 *count = mm_counters_end(ctx, 0, 1);
    return count ? count[0] : MM_ERR_HIP;
}
