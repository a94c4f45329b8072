// Layered column models: on a latitude x longitude map the depths of a stack of interfaces and one value per layer and
// component, evaluated on the nodes of a mesh (include/multimesh_layered.h, which holds the statement; tests/layered_cases.py
// is its NumPy form).
//
//   mm_layered_model_apply : (lat, lon, depth) of the node as mm_sample_grid forms them; the picking depth dp (the node's or
//                            its element centre's); the cell on the two map axes; b_j of the node's column(s), scanned from the
//                            top for the first j with dp < b_{j+1}; the values of that layer
//
// Bit parity with the statement: every product, quotient and sum is rounded on its own (-ffp-contract=off), the coordinates
// come from the device function the sampler uses (mm_latlon.h), the centre from the one the radial kernel uses
// (mm_radial_table.h); no float atomics, the count of outside nodes is an integer sum per workgroup.
//
// Shape.  The model tools' launch (mm_stream.h): 256 lanes, at most kMaxBlocks workgroups striding over tiles of 256 / P whole
// elements (gll::RunTile; pick = node runs as P = 1: 256 nodes per tile), one lane per node.  The coordinates of a tile go to
// LDS coalesced; with pick = element, lane e < tile forms element e's centre there.  The axes are staged in LDS when the two
// together fit kAxisLds doubles and bisected there, longer axes in global memory: the sampler's rule.
// The scan.  The tables are column-major (bounds [nlat][nlon][nb], values [nlat][nlon][nlayer][ncomp]): a lane reads its
// four corner columns (one in cell mode) as contiguous runs from the top and stops at its layer, so trip counts differ from
// lane to lane and nothing in the loop is wave-wide (Column: mm_column.h, shared with mm_topography.hip); neighbouring nodes of a mesh share their columns, which are small beside
// the points (9 x 180 x 360 doubles are 4.7 MB: they live in L2).  Columns are not staged in LDS.
// Traffic counted per node: 24 B read, 8 B per component written (plus the optional outputs).
#include "mm_column.h"
#include "mm_gll_tile.h"
#include "mm_latlon.h"
#include "mm_radial_table.h"

#include "multimesh_layered.h"

namespace {

using namespace mm_stream;   // kThreads, kWave, kMaxBlocks
using mm_column::Column;
using mm_latlon::Cell;
using mm_latlon::find_cell;
using mm_latlon::kAxisLds;
constexpr i64 kMaxExtent = (i64)1 << 48;
typedef unsigned long long u64;

struct LayeredArgs {
    const double *points;
    i64 ngroups;    // groups of P nodes as the kernel tiles them: pick = node runs with P = 1
    int P;
    const double *lat, *lon;
    int nlat, nlon, lon_periodic;
    const double *bounds;
    int nb;
    const double *values;
    int ncomp;
    int pick, outside;
    double fill;
    i64 n;          // values per component of out
    double *out;
    int *layer;
    double *span, *lld;
    u64 *noutside;
};

// The layer of the picking depth dp in the column b (steps 4 and 5 of the statement): -1 when there is none; top and bot are
// its bounds.
template <bool BILINEAR>
__device__ __forceinline__ int find_layer(const Column<BILINEAR> &b, int nlayer, double dp, bool clamp, double &top, double &bot)
{
    const double b0 = b.at(0);
    double prev = b0;
    if (dp >= b0) {
        int last = -1;             // the last layer of positive thickness passed
        double ltop = 0.0, lbot = 0.0;
        for (int j = 0; j < nlayer; ++j) {
            const double cur = b.at(j + 1);
            if (dp < cur) {
                top = prev, bot = cur;
                return j;
            }
            if (prev < cur) last = j, ltop = prev, lbot = cur;
            prev = cur;
        }
        if (last >= 0 && (clamp || dp == prev)) {   // (prev: the model's bottom)
            top = ltop, bot = lbot;
            return last;
        }
    } else if (clamp && dp < b0) {
        for (int j = 0; j < nlayer; ++j) {
            const double cur = b.at(j + 1);
            if (prev < cur) {
                top = prev, bot = cur;
                return j;
            }
            prev = cur;
        }
    }
    return -1;
}

// NC: components unrolled (1..4), 0: a loop over args.ncomp (none when it is 0).  LDS_AXES: the axes are copied to LDS first.
template <int NC, bool LDS_AXES, bool BILINEAR>
__global__ __launch_bounds__(kThreads) void layered_apply_kernel(const LayeredArgs args)
{
    __shared__ double s_axes[LDS_AXES ? kAxisLds : 1];
    __shared__ double xs[3 * kThreads];
    __shared__ double s_dp[kThreads];   // the picking depth of every element of the tile (pick = element)
    __shared__ unsigned s_count[kThreads / kWave];

    const int tid = threadIdx.x, P = args.P, nla = args.nlat, nlo = args.nlon, nb = args.nb, nlayer = nb - 1;
    const double *lat_a = args.lat, *lon_a = args.lon;
    if (LDS_AXES) {
        for (int q = tid; q < nla + nlo; q += kThreads) s_axes[q] = q < nla ? args.lat[q] : args.lon[q - nla];
        lat_a = s_axes;
        lon_a = s_axes + nla;
        __syncthreads();
    }
    const int ncomp = NC ? NC : args.ncomp;
    const gll::RunTile T(args.ngroups, P);
    const i64 n = args.n;
    const bool clamp = args.outside == MM_LAYERED_OUTSIDE_CLAMP, by_element = args.pick == MM_LAYERED_PICK_ELEMENT;
    const double lon0 = lon_a[0];
    const double nan = __builtin_nan("");
    unsigned mine = 0;   // outside nodes

    for (i64 t = blockIdx.x; t < T.ntiles; t += gridDim.x) {
        const int nel = T.nel(t), nnodes = T.nnodes(t);
        const double *src = T.coords(args.points, t);
        __syncthreads();   // (the previous step's reads of xs and s_dp are done)
        for (int q = tid; q < 3 * nnodes; q += kThreads) xs[q] = src[q];
        __syncthreads();
        if (by_element) {   // (the same for every lane)
            if (tid < nel) s_dp[tid] = mm_latlon::kEarthRadius - mm_radial_table::centre_radius(xs + 3 * tid * P, P);
            __syncthreads();
        }
        if (tid >= nnodes) continue;   // (no barrier below in this step; the next step's comes first for every lane)
        const i64 node = T.first_node(t) + tid;
        double lat, lon, depth;
        mm_latlon::lat_lon_depth(xs[3 * tid], xs[3 * tid + 1], xs[3 * tid + 2], lon0, args.lon_periodic, lat, lon, depth);
        if (args.lld) {
            args.lld[3 * node] = lat;
            args.lld[3 * node + 1] = lon;
            args.lld[3 * node + 2] = depth;
        }
        const double dp = by_element ? s_dp[T.el] : depth;
        int layer = -1;
        double top = nan, bot = nan;
        if (lat == lat && lon == lon && dp == dp) {
            const Cell ca = find_cell(lat_a, nla, lat, clamp), co = find_cell(lon_a, nlo, lon, clamp);
            if (ca.inside && co.inside) {
                const Column<BILINEAR> b(args.bounds, nb, nlo, ca, co);
                layer = find_layer(b, nlayer, dp, clamp, top, bot);
                if (layer < 0) {
                    top = bot = nan;
                } else if (ncomp > 0) {
                    const Column<BILINEAR> v(args.values + (i64)layer * ncomp, (i64)nlayer * ncomp, nlo, ca, co);
                    if (NC) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) args.out[c * n + node] = v.at(c);
                    } else {
                        for (int c = 0; c < ncomp; ++c) args.out[c * n + node] = v.at(c);
                    }
                }
            }
        }
        if (layer < 0) {
            ++mine;
            if (args.outside != MM_LAYERED_OUTSIDE_KEEP)
                for (int c = 0; c < ncomp; ++c) args.out[c * n + node] = args.fill;
        }
        if (args.layer) args.layer[node] = layer;
        if (args.span) {
            args.span[2 * node] = top;
            args.span[2 * node + 1] = bot;
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

template <int NC, bool LDS_AXES>
void launch_lateral(mm_context *ctx, unsigned grid, const LayeredArgs &a, int lateral)
{
    if (lateral == MM_LAYERED_LATERAL_BILINEAR)
        hipLaunchKernelGGL((layered_apply_kernel<NC, LDS_AXES, true>), dim3(grid), dim3(kThreads), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((layered_apply_kernel<NC, LDS_AXES, false>), dim3(grid), dim3(kThreads), 0, ctx->stream, a);
}

template <bool LDS_AXES>
void launch(mm_context *ctx, unsigned grid, const LayeredArgs &a, int lateral)
{
    switch (a.ncomp) {
    case 1: launch_lateral<1, LDS_AXES>(ctx, grid, a, lateral); break;
    case 2: launch_lateral<2, LDS_AXES>(ctx, grid, a, lateral); break;
    case 3: launch_lateral<3, LDS_AXES>(ctx, grid, a, lateral); break;
    case 4: launch_lateral<4, LDS_AXES>(ctx, grid, a, lateral); break;
    default: launch_lateral<0, LDS_AXES>(ctx, grid, a, lateral); break;
    }
}

}  // namespace

extern "C" int mm_layered_model_apply(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P,
                                      const double *lat_d, int nlat, const double *lon_d, int nlon, int lon_periodic,
                                      const double *bounds_d, int nb, const double *values_d, int64_t ncomp,
                                      int lateral, int pick, int outside, double fill_value,
                                      double *out_d, int32_t *layer_out_d, double *span_out_d,
                                      double *latlondepth_out_d, int64_t *noutside_d)
{
    typedef unsigned __int128 u128;
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(ngroups >= 0 && ngroups < kMaxExtent, "ngroups out of range");
    MM_REQUIRE(P >= 1 && P <= MM_LAYERED_MAX_P, "P must lie in [1, 256]");
    MM_REQUIRE(nb >= 2 && nb <= MM_LAYERED_MAX_NB, "nb must lie in [2, 256]");
    MM_REQUIRE(nlat >= 1 && nlon >= 1, "every axis needs at least one node");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(lateral == MM_LAYERED_LATERAL_CELL || lateral == MM_LAYERED_LATERAL_BILINEAR, "lateral must be 0 or 1");
    MM_REQUIRE(pick == MM_LAYERED_PICK_NODE || pick == MM_LAYERED_PICK_ELEMENT, "pick must be 0 or 1");
    MM_REQUIRE(outside >= MM_LAYERED_OUTSIDE_FILL && outside <= MM_LAYERED_OUTSIDE_KEEP, "outside must be 0, 1 or 2");
    const i64 n = ngroups * P;   // (< 2^56)
    const u128 columns = (u128)nlat * (u128)nlon;
    MM_REQUIRE((u128)n * 3 < (u128)kMaxExtent, "points: extent at or past 2^48 elements");
    MM_REQUIRE((u128)ncomp * (u128)n < (u128)kMaxExtent, "out: extent at or past 2^48 elements");
    MM_REQUIRE(columns * (u128)nb < (u128)kMaxExtent, "bounds: extent at or past 2^48 elements");
    MM_REQUIRE(columns * (u128)(nb - 1) * (u128)ncomp < (u128)kMaxExtent, "values: extent at or past 2^48 elements");
    MM_REQUIRE(lat_d != nullptr && lon_d != nullptr, "null axis");
    MM_REQUIRE(bounds_d != nullptr && (values_d != nullptr || ncomp == 0), "null table");
    MM_REQUIRE(ngroups == 0 || (points_d != nullptr && (out_d != nullptr || ncomp == 0)), "null array");
    if (n == 0) return MM_OK;
    if (ncomp == 0 && !layer_out_d && !span_out_d && !latlondepth_out_d && !noutside_d) return MM_OK;   // nothing is asked for
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    LayeredArgs a;
    a.points = points_d;
    a.ngroups = pick == MM_LAYERED_PICK_ELEMENT ? ngroups : n;
    a.P = pick == MM_LAYERED_PICK_ELEMENT ? (int)P : 1;
    a.lat = lat_d;
    a.lon = lon_d;
    a.nlat = nlat;
    a.nlon = nlon;
    a.lon_periodic = lon_periodic ? 1 : 0;
    a.bounds = bounds_d;
    a.nb = nb;
    a.values = values_d;
    a.ncomp = (int)ncomp;
    a.pick = pick;
    a.outside = outside;
    a.fill = fill_value;
    a.n = n;
    a.out = out_d;
    a.layer = layer_out_d;
    a.span = span_out_d;
    a.lld = latlondepth_out_d;
    a.noutside = reinterpret_cast<u64 *>(noutside_d);
    const unsigned grid = mm_blocks(a.ngroups, kThreads / a.P, kMaxBlocks);
    if ((i64)nlat + nlon <= kAxisLds)
        launch<true>(ctx, grid, a, lateral);
    else
        launch<false>(ctx, grid, a, lateral);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
