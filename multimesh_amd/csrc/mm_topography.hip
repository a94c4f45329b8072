// Topography: the nodes of a mesh stretched radially between anchor radii by a latitude x longitude map of interface shifts,
// and the flattening that undoes it (include/multimesh_topography.h, which holds the statement; tests/topography_cases.py is
// its NumPy form).
//
//   mm_radial_stretch : (lat, lon) and r of the node as mm_sample_grid forms them; the cell on the two map axes; apply: the
//                       anchor interval of the reference radius (the anchors alone decide it), the two shifts at its ends from
//                       the node's column(s), r' = rho + d; flatten: B_j = A_j + s_j scanned from the top for the first j with
//                       r >= B_{j+1}, rho interpolated between the anchors; p' = p * (new radius / r)
//
// Bit parity with the statement: every product, quotient and sum is rounded on its own (-ffp-contract=off), the coordinates
// come from the device function the sampler uses (mm_latlon.h), the column lookup from the one the layered kernel uses
// (mm_column.h); no float atomics, the count of outside nodes is an integer sum per workgroup.
//
// Shape.  The model tools' launch (mm_stream.h): 256 lanes, at most kMaxBlocks workgroups striding over tiles of 256 nodes, one
// lane per node.  The coordinates of a tile go to LDS coalesced, each lane puts its moved node back into its own three slots, and
// the tile leaves coalesced: in place is safe because a tile is read whole before any of it is written and tiles are disjoint.
// The axes are staged in LDS when the two together fit kAxisLds doubles and bisected there, longer axes in global memory: the
// sampler's rule.  The anchors are read at the loop counter of the scan, which is the same in every lane still scanning: scalar
// loads.  The shifts are column-major; apply reads two entries of the column(s) (one above the top and below the bottom), flatten
// walks down from the top and stops at its interval, so its trip count differs from lane to lane.
// Traffic counted per node: 24 B read, 24 B written, 8 B for each of ref_radius and radius_out.
#include "mm_column.h"
#include "mm_latlon.h"

#include "multimesh_topography.h"

namespace {

using namespace mm_stream;   // kThreads, kWave, kMaxBlocks
using mm_column::Column;
using mm_latlon::Cell;
using mm_latlon::find_cell;
using mm_latlon::kAxisLds;
constexpr i64 kMaxExtent = (i64)1 << 48;
typedef unsigned long long u64;

struct StretchArgs {
    const double *points;
    i64 n;
    const double *ref;
    const double *lat, *lon;
    int nlat, nlon, lon_periodic;
    const double *anchors;
    int na;
    const double *shifts;
    int outside;
    double *out, *radius, *lld;
    u64 *noutside;
};

// Step 3 of the statement: the displacement d of the reference radius rho in the column s.
template <bool BILINEAR>
__device__ __forceinline__ double displacement(const Column<BILINEAR> &s, const double *A, int na, double rho)
{
    double hi = A[0];
    if (rho >= hi) return s.at(0);
    for (int j = 0; j < na - 1; ++j) {
        const double lo = A[j + 1];
        if (rho >= lo) {
            const double u = (rho - lo) / (hi - lo);
            return mm_lerp(u, s.at(j + 1), s.at(j));
        }
        hi = lo;
    }
    return s.at(na - 1);
}

// Step 4: the reference radius rho of the radius r in the column s.
template <bool BILINEAR>
__device__ __forceinline__ double flattened(const Column<BILINEAR> &s, const double *A, int na, double r)
{
    double a_hi = A[0], s_lo = s.at(0);
    double b_hi = a_hi + s_lo;
    if (r >= b_hi) return r - s_lo;
    for (int j = 0; j < na - 1; ++j) {
        const double a_lo = A[j + 1];
        s_lo = s.at(j + 1);
        const double b_lo = a_lo + s_lo;
        if (r >= b_lo) {
            const double u = (r - b_lo) / (b_hi - b_lo);
            return mm_lerp(u, a_lo, a_hi);
        }
        a_hi = a_lo, b_hi = b_lo;
    }
    return r - s_lo;   // (s_{na-1})
}

// LDS_AXES: the axes are copied to LDS first.  FLATTEN: direction = 1.
template <bool LDS_AXES, bool BILINEAR, bool FLATTEN>
__global__ __launch_bounds__(kThreads) void radial_stretch_kernel(const StretchArgs args)
{
    __shared__ double s_axes[LDS_AXES ? kAxisLds : 1];
    __shared__ double xs[3 * kThreads];
    __shared__ unsigned s_count[kThreads / kWave];

    const int tid = threadIdx.x, nla = args.nlat, nlo = args.nlon, na = args.na;
    const double *lat_a = args.lat, *lon_a = args.lon;
    if (LDS_AXES) {
        for (int q = tid; q < nla + nlo; q += kThreads) s_axes[q] = q < nla ? args.lat[q] : args.lon[q - nla];
        lat_a = s_axes;
        lon_a = s_axes + nla;
        __syncthreads();
    }
    const i64 n = args.n, ntiles = (n + kThreads - 1) / kThreads;
    const bool clamp = args.outside == MM_STRETCH_OUTSIDE_CLAMP;
    const double lon0 = lon_a[0];
    unsigned mine = 0;   // outside nodes

    for (i64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const i64 first = t * kThreads;
        const int nnodes = (int)(n - first < kThreads ? n - first : kThreads);
        const double *src = args.points + 3 * first;
        __syncthreads();   // (the previous step's reads of xs are done)
        for (int q = tid; q < 3 * nnodes; q += kThreads) xs[q] = src[q];
        __syncthreads();
        if (tid < nnodes) {
            const i64 node = first + tid;
            const double x = xs[3 * tid], y = xs[3 * tid + 1], z = xs[3 * tid + 2];
            const double r = mm_norm3(x, y, z);
            double lat, lon, depth;
            mm_latlon::lat_lon_depth(x, y, z, lon0, args.lon_periodic, lat, lon, depth);
            if (args.lld) {
                args.lld[3 * node] = lat;
                args.lld[3 * node + 1] = lon;
                args.lld[3 * node + 2] = depth;
            }
            double radius = r;
            bool moved = false;
            if (lat == lat && lon == lon && r > 0.0) {   // (r > 0 is false for a NaN)
                const Cell ca = find_cell(lat_a, nla, lat, clamp), co = find_cell(lon_a, nlo, lon, clamp);
                if (ca.inside && co.inside) {
                    const Column<BILINEAR> s(args.shifts, na, nlo, ca, co);
                    if (FLATTEN) {
                        radius = flattened(s, args.anchors, na, r);
                    } else {
                        const double rho = args.ref ? args.ref[node] : r;
                        radius = rho + displacement(s, args.anchors, na, rho);
                    }
                    moved = true;
                }
            }
            if (moved) {   // (an outside node keeps its bits: its slots of xs are left as they are)
                const double scale = radius / r;
                xs[3 * tid] = x * scale;
                xs[3 * tid + 1] = y * scale;
                xs[3 * tid + 2] = z * scale;
            } else {
                ++mine;
            }
            if (args.radius) args.radius[node] = radius;
        }
        if (args.out) {   // (the same for every lane)
            double *dst = args.out + 3 * first;
            __syncthreads();
            for (int q = tid; q < 3 * nnodes; q += kThreads) dst[q] = xs[q];
        }
    }
    if (args.noutside) {   // one integer sum per workgroup, one atomic
        __syncthreads();
        mine = wave_sum(mine);
        if ((tid & (kWave - 1)) == 0) s_count[tid / kWave] = mine;
        __syncthreads();
        if (tid == 0) {
            unsigned total = 0;
#pragma unroll
            for (int wv = 0; wv < kThreads / kWave; ++wv) total += s_count[wv];
            if (total != 0) atomicAdd(args.noutside, (u64)total);
        }
    }
}

template <bool LDS_AXES, bool BILINEAR>
void launch_direction(mm_context *ctx, unsigned grid, const StretchArgs &a, int direction)
{
    if (direction == MM_STRETCH_DIRECTION_FLATTEN)
        hipLaunchKernelGGL((radial_stretch_kernel<LDS_AXES, BILINEAR, true>), dim3(grid), dim3(kThreads), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((radial_stretch_kernel<LDS_AXES, BILINEAR, false>), dim3(grid), dim3(kThreads), 0, ctx->stream, a);
}

template <bool LDS_AXES>
void launch(mm_context *ctx, unsigned grid, const StretchArgs &a, int direction, int lateral)
{
    if (lateral == MM_STRETCH_LATERAL_BILINEAR)
        launch_direction<LDS_AXES, true>(ctx, grid, a, direction);
    else
        launch_direction<LDS_AXES, false>(ctx, grid, a, direction);
}

}  // namespace

extern "C" int mm_radial_stretch(mm_context *ctx, const double *points_d, int64_t n, const double *ref_radius_d,
                                 const double *lat_d, int nlat, const double *lon_d, int nlon, int lon_periodic,
                                 const double *anchors_d, int na, const double *shifts_d,
                                 int direction, int lateral, int outside,
                                 double *points_out_d, double *radius_out_d,
                                 double *latlondepth_out_d, int64_t *noutside_d)
{
    typedef unsigned __int128 u128;
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && (u128)n * 3 < (u128)kMaxExtent, "points: n negative or extent at or past 2^48 elements");
    MM_REQUIRE(na >= 2 && na <= MM_STRETCH_MAX_NA, "na must lie in [2, 64]");
    MM_REQUIRE(nlat >= 1 && nlon >= 1, "every axis needs at least one node");
    MM_REQUIRE((u128)nlat * (u128)nlon * (u128)na < (u128)kMaxExtent, "shifts: extent at or past 2^48 elements");
    MM_REQUIRE(direction == MM_STRETCH_DIRECTION_APPLY || direction == MM_STRETCH_DIRECTION_FLATTEN, "direction must be 0 or 1");
    MM_REQUIRE(lateral == MM_STRETCH_LATERAL_CELL || lateral == MM_STRETCH_LATERAL_BILINEAR, "lateral must be 0 or 1");
    MM_REQUIRE(outside == MM_STRETCH_OUTSIDE_KEEP || outside == MM_STRETCH_OUTSIDE_CLAMP, "outside must be 0 or 1");
    MM_REQUIRE(lat_d != nullptr && lon_d != nullptr, "null axis");
    MM_REQUIRE(anchors_d != nullptr && shifts_d != nullptr, "null anchors or shifts");
    MM_REQUIRE(n == 0 || points_d != nullptr, "null points");
    MM_REQUIRE(ref_radius_d == nullptr || direction == MM_STRETCH_DIRECTION_APPLY, "ref_radius goes with direction 0: flattening computes it");
    if (n == 0) return MM_OK;
    if (!points_out_d && !radius_out_d && !latlondepth_out_d && !noutside_d) return MM_OK;   // nothing is asked for
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    StretchArgs a;
    a.points = points_d;
    a.n = n;
    a.ref = ref_radius_d;
    a.lat = lat_d;
    a.lon = lon_d;
    a.nlat = nlat;
    a.nlon = nlon;
    a.lon_periodic = lon_periodic ? 1 : 0;
    a.anchors = anchors_d;
    a.na = na;
    a.shifts = shifts_d;
    a.outside = outside;
    a.out = points_out_d;
    a.radius = radius_out_d;
    a.lld = latlondepth_out_d;
    a.noutside = reinterpret_cast<u64 *>(noutside_d);
    const unsigned grid = mm_blocks(n, kThreads, kMaxBlocks);
    if ((i64)nlat + nlon <= kAxisLds)
        launch<true>(ctx, grid, a, direction, lateral);
    else
        launch<false>(ctx, grid, a, direction, lateral);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
