// What a model asks of its mesh: the least node spacing and the corner-to-corner edge lengths of every element of an
// element-nodal GLL mesh and, with velocities, the time step and the shortest resolved period each element allows; and the
// extreme of a row of values with the place where it stands.
//
//   mm_gll_resolution : out f64[5][E] = spacing, edge_min, edge_max, step, period; info int64[2]; node_h f64[E][P]
//   mm_arg_extreme    : the least or greatest non-NaN value of every row, the lowest index that holds it, the valid count
//
// Bit parity with the NumPy statement (tests/resolution_cases.py, include/multimesh_hip.h): every difference, product, sum,
// root and quotient is rounded on its own (-ffp-contract=off).  The statement takes minima and maxima of DISTANCES; the
// kernel takes them of the SQUARED distances and then one root: the f64 square root is correctly rounded, hence monotone,
// so sqrt(min s) is bit for bit min sqrt(s) -- no root per neighbour, and none per node in a call without velocities and
// without node_h.  Minima and maxima have no order, so the reduction below is free in its shape.
//
// mm_gll_resolution is a streaming kernel on the element tile of mm_gll_tile.h (fetch one step ahead, LDS tile, at most
// kMaxBlocks blocks striding over tiles): 24 B read per node and 24 B written per element, with velocities 8 B more per
// node and component.  Lane t of the block is node t of the tile.  An element's P lanes do not align with waves (P = 125:
// element 1 is lanes 125 .. 249), so the per-element minima go through LDS along the tensor structure, in two steps:
//   1. every lane stores its values at red[.][t]; the lanes with i = 0 take the minimum of their line along direction 0
//      (M consecutive values) and store it in place;
//   2. the element's node 0 takes the minimum of the P / M line results (stride M), reads the 2^DIM corner lanes' least
//      and greatest squared chords, takes the roots and the one division, and writes the element's rows.
// Three barriers per tile: after the coordinates are in LDS, after the lanes' values are, after the line minima are.  The
// lanes that hold no node, and the lanes of elements missing from the last tile, store +inf (and no chord): they can
// never reach a result.  The flags of an element (a coordinate that is not finite; a velocity that is refused) are plain
// LDS stores of 1 by whoever finds one, cleared by the element's node 0 after it has read them.
//
// mm_arg_extreme keeps no scratch: value_d holds the greatest order-preserving integer image of the row (its complement
// for a minimum) and index_d the greatest complement of an index while the passes run -- integer atomicMax only, so the
// result is the same on every run -- and a last kernel replaces them by the value stored at the index and the index.
#include "mm_gll_tile.h"

#include <math.h>

namespace {

using namespace mm_stream;   // kThreads, kWave
typedef unsigned long long u64;

struct ResolutionArgs {
    const double *gp;
    i64 nelem;
    const double *fast, *slow;
    int nfast, nslow;
    double *node_h, *out;
    u64 *info;
};

// (dx*dx + dy*dy) + dz*dz of d = b - a, the argument of mm_norm3's root
template <int DIM>
__device__ __forceinline__ double dist2(const double *a, const double *b)
{
    const double dx = b[0] - a[0], dy = b[1] - a[1];
    if constexpr (DIM == 3) {
        const double dz = b[2] - a[2];
        return (dx * dx + dy * dy) + dz * dz;
    } else {
        return dx * dx + dy * dy;
    }
}

template <int ORDER, int DIM>
__global__ __launch_bounds__(kThreads) void gll_resolution_kernel(const ResolutionArgs a)
{
    using T = gll::Tile<ORDER, DIM>;
    constexpr int M = T::M, P = T::P, NC = 1 << DIM;   // NC corners; TILE * NC <= TILE * P <= kThreads
    __shared__ double xs[T::TILE_DOUBLES];
    __shared__ double red[3][kThreads];        // per node: s = the least squared neighbour distance, h / vfast, vslow
    __shared__ double chord[2][T::TILE * NC];  // per corner: the least and greatest squared chord it starts
    __shared__ int flag[2][T::TILE];           // per element: geometry-invalid, a velocity refused

    const int tid = threadIdx.x;
    const typename T::Node nd;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const bool with_model = a.nfast > 0;
    const i64 nnodes = a.nelem * P;

    // a corner lane: every i[d] is 0 or ORDER; corner c = sum_d (i[d] == ORDER) << d
    bool corner = nd.node_lane;
    int c = 0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        corner = corner && (nd.i[d] == 0 || nd.i[d] == ORDER);
        c |= (nd.i[d] == ORDER ? 1 : 0) << d;
    }
    if (tid < T::TILE) flag[0][tid] = 0, flag[1][tid] = 0;

    const i64 ntiles = (a.nelem + T::TILE - 1) / T::TILE;
    unsigned ngeo = 0, nmodel = 0;
    double stage[T::LOADS];
    i64 tile = blockIdx.x;
    if (tile < ntiles) T::fetch_x(a.gp, a.nelem, tile, stage);
    for (; tile < ntiles; tile += gridDim.x) {
        T::store_x(xs, stage);   // (the previous step's reads of xs ended before its second barrier)
        __syncthreads();
        if (tile + gridDim.x < ntiles) T::fetch_x(a.gp, a.nelem, tile + gridDim.x, stage);
        const bool live = tid < T::tile_nodes(a.nelem, tile);   // a node of an element this tile has
        const i64 node = tile * (i64)T::TILE_NODES + tid;
        double s = inf, q = inf, vs = inf, h = 0.0;
        if (live) {
            const double *x = xs + tid * DIM;
            bool finite = mm_is_finite(x[0]) && mm_is_finite(x[1]);
            if constexpr (DIM == 3) finite = finite && mm_is_finite(x[2]);
            if (!finite) flag[0][nd.el] = 1;
            double cmin = inf, cmax = -inf;
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                const int stride = gll::ipow(M, d);
                if (nd.i[d] > 0) {              // d = later - earlier: this node minus its predecessor
                    const double t = dist2<DIM>(x - stride * DIM, x);
                    s = t < s ? t : s;
                }
                if (nd.i[d] < ORDER) {
                    const double t = dist2<DIM>(x, x + stride * DIM);
                    s = t < s ? t : s;
                }
                if (corner && nd.i[d] == 0) {   // the edge (c, c | 1 << d): the chord to the corner at the line's end
                    const double t = dist2<DIM>(x, x + ORDER * stride * DIM);
                    cmin = t < cmin ? t : cmin;
                    cmax = t > cmax ? t : cmax;
                }
            }
            if (corner) chord[0][nd.el * NC + c] = cmin, chord[1][nd.el * NC + c] = cmax;
            if (with_model || a.node_h) h = sqrt(s);
            if (with_model) {
                double vf = -inf, vfmin = inf;
                bool refused = false;
                for (int k = 0; k < a.nfast; ++k) {
                    const double v = a.fast[k * nnodes + node];
                    refused = refused || !(mm_is_finite(v) && v > 0.0);
                    vf = v > vf ? v : vf;
                    vfmin = v < vfmin ? v : vfmin;
                }
                for (int k = 0; k < a.nslow; ++k) {
                    const double v = a.slow[k * nnodes + node];
                    refused = refused || !(mm_is_finite(v) && v >= 0.0);
                    if (v > 0.0 && v < vs) vs = v;
                }
                if (!(vs < inf)) vs = vfmin;   // no slow velocity above zero (a fluid): the least fast one
                q = h / vf;
                if (refused) flag[1][nd.el] = 1;
            }
        }
        red[0][tid] = s;
        if (with_model) red[1][tid] = q, red[2][tid] = vs;
        __syncthreads();
        if (a.node_h && live) a.node_h[node] = flag[0][nd.el] ? nan : h;
        if (nd.node_lane && nd.i[0] == 0) {   // the line along direction 0, in place: its other lanes are done with theirs
#pragma unroll
            for (int k = 1; k < M; ++k) {
                const double t = red[0][tid + k];
                s = t < s ? t : s;
            }
            red[0][tid] = s;
            if (with_model) {
#pragma unroll
                for (int k = 1; k < M; ++k) {
                    const double tq = red[1][tid + k], tv = red[2][tid + k];
                    q = tq < q ? tq : q;
                    vs = tv < vs ? tv : vs;
                }
                red[1][tid] = q, red[2][tid] = vs;
            }
        }
        __syncthreads();
        if (live && nd.p == 0) {   // node 0 of an element of this tile: the line results, the corners' chords, the rows
            // (a few reads in flight at a time: unrolled in full, the 3 * 24 values of order 4 cost an occupancy step)
#pragma unroll 4
            for (int k = 1; k < P / M; ++k) {
                const double t = red[0][tid + k * M];
                s = t < s ? t : s;
            }
            if (with_model)
#pragma unroll 4
                for (int k = 1; k < P / M; ++k) {
                    const double tq = red[1][tid + k * M], tv = red[2][tid + k * M];
                    q = tq < q ? tq : q;
                    vs = tv < vs ? tv : vs;
                }
            double cmin = inf, cmax = -inf;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const double lo = chord[0][nd.el * NC + k], hi = chord[1][nd.el * NC + k];
                cmin = lo < cmin ? lo : cmin;
                cmax = hi > cmax ? hi : cmax;
            }
            const bool geo = flag[0][nd.el] != 0, model = geo || flag[1][nd.el] != 0;
            flag[0][nd.el] = 0, flag[1][nd.el] = 0;   // (next written after the next tile's first barrier)
            const i64 e = tile * (i64)T::TILE + nd.el;
            const double edge_max = sqrt(cmax);
            a.out[e] = geo ? nan : sqrt(s);
            a.out[a.nelem + e] = geo ? nan : sqrt(cmin);
            a.out[2 * a.nelem + e] = geo ? nan : edge_max;
            if (with_model) {
                a.out[3 * a.nelem + e] = model ? nan : q;
                a.out[4 * a.nelem + e] = model ? nan : edge_max / vs;
            }
            ngeo += geo, nmodel += model;
        }
    }
    mm_count_to(a.info, ngeo);
    mm_count_to(a.info + 1, nmodel);
}

template <int ORDER, int DIM>
void launch_resolution(mm_context *ctx, const ResolutionArgs &a)
{
    hipLaunchKernelGGL((gll_resolution_kernel<ORDER, DIM>), dim3(gll::grid_size(a.nelem, gll::Tile<ORDER, DIM>::TILE)),
                       dim3(kThreads), 0, ctx->stream, a);
}

// ---------------------------------------------------------------------------------------------------- mm_arg_extreme
constexpr i64 kExtremeBlocks = 1024;   // per row; they stride over the rest
constexpr int kExtremePerLane = 8;

// The unsigned order of the image is the numeric order of the doubles; -0.0 takes the image of +0.0.  No image is 0.
__device__ __forceinline__ u64 image_of(double v, int want_max)
{
    const u64 u = (u64)__double_as_longlong(v == 0.0 ? 0.0 : v);
    const u64 k = (u >> 63) ? ~u : (u | ((u64)1 << 63));
    return want_max ? k : ~k;
}

__device__ __forceinline__ u64 wave_max(u64 v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off, kWave);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void extreme_clear_kernel(i64 nrows, u64 *best, u64 *place, u64 *nvalid)
{
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nrows) best[r] = 0, place[r] = 0, nvalid[r] = 0;
}

// best[r] = max of the images of row r's values that are not NaN; nvalid[r] += their number
__global__ __launch_bounds__(kThreads) void extreme_value_kernel(const double *__restrict__ values, i64 n, int want_max,
                                                                 u64 *best, u64 *nvalid)
{
    const i64 r = blockIdx.y;
    const double *row = values + r * n;
    u64 mine = 0;
    unsigned count = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
        const double v = row[idx];
        if (v == v) {
            const u64 k = image_of(v, want_max);
            mine = k > mine ? k : mine;
            ++count;
        }
    }
    mine = wave_max(mine);
    if ((threadIdx.x & (kWave - 1)) == 0 && mine != 0) atomicMax(best + r, mine);
    mm_count_to(nvalid + r, count);
}

// place[r] = max of ~index over the values whose image is best[r]: the lowest such index
__global__ __launch_bounds__(kThreads) void extreme_place_kernel(const double *__restrict__ values, i64 n, int want_max,
                                                                 const u64 *__restrict__ best, u64 *place)
{
    const i64 r = blockIdx.y;
    const u64 want = best[r];
    if (want == 0) return;   // (no valid value: every lane of the grid's row leaves)
    const double *row = values + r * n;
    u64 mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
        const double v = row[idx];
        if (v == v && image_of(v, want_max) == want) {
            mine = ~(u64)idx;   // (a lane's indices ascend: its first hit is its lowest)
            break;
        }
    }
    mine = wave_max(mine);
    if ((threadIdx.x & (kWave - 1)) == 0 && mine != 0) atomicMax(place + r, mine);
}

// the value stored at the index, and the index; NaN and -1 for a row without a valid value
__global__ __launch_bounds__(kThreads) void extreme_finish_kernel(const double *__restrict__ values, i64 n, i64 nrows,
                                                                  double *value, i64 *index)
{
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const u64 img = (u64)index[r];
    if (img == 0) {
        value[r] = __builtin_nan("");
        index[r] = -1;
    } else {
        const i64 idx = (i64)~img;
        value[r] = values[r * n + idx];
        index[r] = idx;
    }
}

}  // namespace

extern "C" int mm_gll_resolution(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem,
                                 const double *fast_d, int64_t nfast, const double *slow_d, int64_t nslow, double *node_h_d,
                                 double *out_d, int64_t *info_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(order == 1 || order == 2 || order == 4, "order must be 1, 2 or 4");
    MM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
    MM_REQUIRE(nelem >= 0 && nelem < ((i64)1 << 40), "nelem out of range");
    MM_REQUIRE(nfast >= 0 && nfast <= 1024 && nslow >= 0 && nslow <= 1024, "nfast and nslow must lie in [0, 1024]");
    MM_REQUIRE(nfast > 0 || (nslow == 0 && slow_d == nullptr), "slow velocities need a fast one (nfast == 0)");
    MM_REQUIRE(info_d != nullptr, "null info");
    MM_REQUIRE(nelem == 0 || (gll_points_d != nullptr && out_d != nullptr), "null array");
    MM_REQUIRE(nelem == 0 || ((nfast == 0 || fast_d != nullptr) && (nslow == 0 || slow_d != nullptr)), "null velocities");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    if (mm_zero_async(ctx, info_d, 2 * sizeof(int64_t)) != MM_OK) return MM_ERR_HIP;
    if (nelem == 0) return MM_OK;
    ResolutionArgs a;
    a.gp = gll_points_d;
    a.nelem = nelem;
    a.fast = fast_d, a.slow = slow_d;
    a.nfast = (int)nfast, a.nslow = (int)nslow;
    a.node_h = node_h_d, a.out = out_d;
    a.info = reinterpret_cast<u64 *>(info_d);
#define MM_RESOLUTION_CASE(O, D) \
    if (order == O && dim == D) launch_resolution<O, D>(ctx, a)
    MM_RESOLUTION_CASE(1, 2);
    MM_RESOLUTION_CASE(2, 2);
    MM_RESOLUTION_CASE(4, 2);
    MM_RESOLUTION_CASE(1, 3);
    MM_RESOLUTION_CASE(2, 3);
    MM_RESOLUTION_CASE(4, 3);
#undef MM_RESOLUTION_CASE
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_arg_extreme(mm_context *ctx, const double *values_d, int64_t nrows, int64_t n, int want_max,
                              double *value_d, int64_t *index_d, int64_t *nvalid_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(nrows >= 0 && nrows < 65536, "nrows must lie in [0, 65536)");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 48), "n out of range");
    MM_REQUIRE(want_max == 0 || want_max == 1, "want_max must be 0 or 1");
    if (nrows == 0) return MM_OK;
    MM_REQUIRE(value_d != nullptr && index_d != nullptr && nvalid_d != nullptr, "null output");
    MM_REQUIRE(n == 0 || values_d != nullptr, "null values");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    u64 *best = reinterpret_cast<u64 *>(value_d), *place = reinterpret_cast<u64 *>(index_d);
    u64 *nvalid = reinterpret_cast<u64 *>(nvalid_d);
    const dim3 rows(mm_blocks(nrows, kThreads, (i64)1 << 30)), block(kThreads);
    const dim3 grid(mm_blocks(n, (i64)kThreads * kExtremePerLane, kExtremeBlocks), (unsigned)nrows);
    hipLaunchKernelGGL(extreme_clear_kernel, rows, block, 0, ctx->stream, (i64)nrows, best, place, nvalid);
    if (n > 0) {
        hipLaunchKernelGGL(extreme_value_kernel, grid, block, 0, ctx->stream, values_d, (i64)n, want_max, best, nvalid);
        hipLaunchKernelGGL(extreme_place_kernel, grid, block, 0, ctx->stream, values_d, (i64)n, want_max, (const u64 *)best,
                           place);
    }
    hipLaunchKernelGGL(extreme_finish_kernel, rows, block, 0, ctx->stream, values_d, (i64)n, (i64)nrows, value_d, (i64 *)index_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
