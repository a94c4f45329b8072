// What mm_boundary.hip and mm_surface.hip both need, each stated once: the launch shape of their streaming kernels, the
// counter words of mm_context::d_counters they own, the face convention (decode and node index), the selection of boundary
// faces by side and the driver that turns the selected faces into items (nodes, triangles), the bounding box of a cloud of
// points by integer maxima (with its decoding on the host), and the search grid of the two distances: the cell of a
// coordinate, the linear index and the bin build (mm_search_grid.h has the struct and the fit of the edge, free of HIP).
#pragma once

#include "mm_search_grid.h"
#include "mm_stream.h"

#include <math.h>
#include <string.h>

namespace {

using namespace mm_stream;   // kThreads, kWave, kMaxBlocks
typedef unsigned long long u64;
typedef mm_search_grid Grid;
constexpr int kSlot = 16, kWords = 8;      // the units' words of mm_context::d_counters (mm_common.h)
constexpr double kMinCutoff = 0x1p-500;

unsigned stream_grid(i64 n) { return mm_blocks(n, kThreads, kMaxBlocks); }

// ---------------------------------------------------------------------------------------------- the face convention
// (include/multimesh_hip.h) local face f = 2 * axis + side, face code 6 e + f.  A face of an element of m^3 nodes, node
// p = i + m j + m^2 k, holds the nodes whose index on the face's axis a is fix = side * (m - 1); (lo, hi) are their
// indices on the two other axes, the lower axis first.
struct Face {
    i64 e;
    int a, fix;
};

__device__ __forceinline__ Face face_of(i64 code, int m)
{
    const i64 e = code / 6;
    const int f = (int)(code - 6 * e);
    return {e, f >> 1, (f & 1) * (m - 1)};
}

// the node at (lo, hi) of the face.  m = 2: the corner c = i + 2 j + 4 k; (0,0), (1,0), (0,1), (1,1) ascend and
// (0,0), (1,0), (1,1), (0,1) go round
__device__ __forceinline__ int face_node(int a, int fix, int m, int lo, int hi)
{
    const int mm = m * m;
    return a == 0 ? fix + m * lo + mm * hi : (a == 1 ? lo + m * fix + mm * hi : lo + m * hi + mm * fix);
}

// ------------------------------------------------------------------------------------- selected faces to their items
// flag[b] = face b is selected; *bad counts the codes outside [0, 6 nelem) and the sides outside [0, 2]
__global__ __launch_bounds__(kThreads) void select_kernel(const i64 *__restrict__ faces, const int *__restrict__ side, i64 nb,
                                                          i64 nelem, int side_mask, int *__restrict__ flag, u64 *bad)
{
    unsigned mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride) {
        const int s = side ? side[b] : 0;
        const bool ok = (u64)faces[b] < (u64)(6 * nelem) && s >= 0 && s <= 2;
        mine += !ok;
        flag[b] = ok && (side == nullptr || ((side_mask >> s) & 1)) ? 1 : 0;
    }
    mm_count_to(bad, mine);
}

// One lane per item of a face: item = b * per + k.  Items: kDoubles per item, per_face(m) items per face, and
// write(X, m, face, k, dst): item k of the face from the element's nodes X.
template <class Items>
__global__ __launch_bounds__(kThreads) void face_items_kernel(const double *__restrict__ points, int m, const i64 *__restrict__ faces,
                                                              i64 nb, const int *__restrict__ flag, const int *__restrict__ rank,
                                                              double *__restrict__ out, u64 *counters)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[1] = (u64)rank[nb];   // the selected faces
    if (counters[0] != 0) return;   // (a refused call writes no item)
    const int per = Items::per_face(m);
    const i64 P = (i64)m * m * m, nitems = nb * per;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 item = (i64)blockIdx.x * blockDim.x + threadIdx.x; item < nitems; item += stride) {
        const i64 b = item / per;
        if (!flag[b]) continue;
        const int k = (int)(item - b * per);
        const Face face = face_of(faces[b], m);
        Items::write(points + 3 * (face.e * P), m, face, k, out + Items::kDoubles * ((i64)rank[b] * per + k));
    }
}

// mm_boundary_nodes and mm_boundary_triangles on behalf of the entry point `who`: the items written, or an error code
template <class Items>
i64 selected_face_items(mm_context *ctx, const char *who, const double *points_d, i64 nelem, int order, const i64 *faces_d,
                        const int *side_d, i64 nb, int side_mask, double *out_d)
{
    MM_REQUIRE_AS(who, ctx != nullptr, "ctx is null");
    MM_REQUIRE_AS(who, order == 1 || order == 2 || order == 4, "order must be 1, 2 or 4");
    MM_REQUIRE_AS(who, nelem >= 0 && nelem < ((i64)1 << 27), "nelem must lie in [0, 2^27)");
    MM_REQUIRE_AS(who, nb >= 0 && nb <= 6 * nelem, "nb must lie in [0, 6 nelem]");
    MM_REQUIRE_AS(who, side_mask >= 0 && side_mask <= 7, "side_mask must lie in [0, 7]");
    MM_REQUIRE_AS(who, nb == 0 || (points_d != nullptr && faces_d != nullptr && out_d != nullptr), "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    if (nb == 0) return 0;
    const int m = order + 1, per = Items::per_face(m);
    int *flag, *rank, *tile_sums;
    mm_scratch_layout lay;
    lay.add(&flag, (size_t)nb + 1);
    lay.add(&rank, (size_t)nb + 1);
    lay.add(&tile_sums, mm_scan_scratch_ints(nb));
    int rc = lay.commit(ctx, who);
    if (rc != MM_OK) return rc;
    u64 *counters = mm_counters_begin(ctx, kSlot, 2);   // [0] bad codes or sides, [1] the selected faces
    if (!counters) return MM_ERR_HIP;
    hipLaunchKernelGGL(select_kernel, dim3(stream_grid(nb)), dim3(kThreads), 0, ctx->stream, faces_d, side_d, nb, nelem, side_mask,
                       flag, counters);
    MM_HIP_CHECK(hipGetLastError());
    rc = mm_exclusive_scan_int(ctx, flag, nb, rank, tile_sums);
    if (rc != MM_OK) return rc;
    hipLaunchKernelGGL(face_items_kernel<Items>, dim3(stream_grid(nb * per)), dim3(kThreads), 0, ctx->stream, points_d, m, faces_d,
                       nb, (const int *)flag, (const int *)rank, out_d, counters);
    const i64 *got = mm_counters_end(ctx, kSlot, 2);
    if (!got) return MM_ERR_HIP;
    if (got[0] != 0) {
        mm_set_error(MM_ERR_ARG, "%s: %lld faces have a code outside [0, %lld) or a side outside [0, 2]", who, (long long)got[0],
                     (long long)(6 * nelem));
        return MM_ERR_ARG;
    }
    return got[1] * per;
}

// ------------------------------------------------------------------------------------------------ the bounding box
// words[1] += the sources with a coordinate that is not finite; words[2 + a] = max of ~key(x_a) (the minimum),
// words[5 + a] = max of key(x_a): integer maxima of the finite coordinates, zero on entry
__global__ __launch_bounds__(kThreads) void sources_box_kernel(const double *__restrict__ src, i64 K, u64 *words)
{
    const double inf = __builtin_inf();
    double b[6] = {inf, -inf, inf, -inf, inf, -inf};
    unsigned mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride) {
        const double x[3] = {src[3 * j], src[3 * j + 1], src[3 * j + 2]};
        if (mm_is_finite(x[0]) && mm_is_finite(x[1]) && mm_is_finite(x[2])) {
#pragma unroll
            for (int a = 0; a < 3; ++a) b[2 * a] = fmin(b[2 * a], x[a]), b[2 * a + 1] = fmax(b[2 * a + 1], x[a]);
        } else {
            ++mine;
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const double o = __shfl_xor(b[a], off, kWave);
            b[a] = (a & 1) ? fmax(b[a], o) : fmin(b[a], o);
        }
    if ((threadIdx.x & (kWave - 1)) == 0 && b[0] <= b[1]) {   // (the wave has seen a finite source)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMax(words + 2 + a, ~mm_key_of((u64)__double_as_longlong(b[2 * a])));
            atomicMax(words + 5 + a, mm_key_of((u64)__double_as_longlong(b[2 * a + 1])));
        }
    }
    mm_count_to(words + 1, mine);
}

// the box of sources_box_kernel's words as read back: lo[a], hi[a] (every source was finite and there was one)
inline void box_of_words(const i64 *got, double (&lo)[3], double (&hi)[3])
{
    for (int a = 0; a < 3; ++a) {
        const u64 lo_bits = mm_bits_of_key(~(u64)got[2 + a]), hi_bits = mm_bits_of_key((u64)got[5 + a]);
        memcpy(&lo[a], &lo_bits, sizeof(double));
        memcpy(&hi[a], &hi_bits, sizeof(double));
    }
}

// ------------------------------------------------------------------------------------------------ the search grid
// v(x) = fl(fl(x - lo) * inv_h), the cell index of a coordinate on axis a before its floor: a MONOTONE function of x, and
// the expression DESIGN.md section 5 derives both searches' margins from.  Every index of either search is formed from it.
__device__ __forceinline__ double grid_coord(const Grid &g, int a, double x) { return (x - g.lo[a]) * g.inv_h; }

// The cell of a coordinate of an item: clamp(floor(v(x)), 0, dims - 1).  For an item 0 <= x - lo and the index stays below
// dims: the clamps only guard the memory.
__device__ __forceinline__ int grid_cell(const Grid &g, int a, double x)
{
    const double v = floor(grid_coord(g, a, x));
    return v >= 0.0 ? (v < (double)g.dims[a] ? (int)v : g.dims[a] - 1) : 0;
}

__device__ __forceinline__ int grid_index(const Grid &g, int x, int y, int z) { return (z * g.dims[1] + y) * g.dims[0] + x; }

// The bins: the items' records cell by cell, rec[Item::kDoubles * j] for start[c] <= j < start[c + 1].  Item: kDoubles per
// record and cells(g, s, c0, c1), the box of cells [c0[a], c1[a]] per axis that the item at s is entered into (a point:
// its one cell).
template <class Item>
__global__ __launch_bounds__(kThreads) void bins_count_kernel(const double *__restrict__ items, i64 N, const Grid g,
                                                              int *__restrict__ count)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += stride) {
        int c0[3], c1[3];
        Item::cells(g, items + Item::kDoubles * t, c0, c1);
        for (int z = c0[2]; z <= c1[2]; ++z)
            for (int y = c0[1]; y <= c1[1]; ++y)
                for (int x = c0[0]; x <= c1[0]; ++x) atomicAdd(&count[grid_index(g, x, y, z)], 1);
    }
}

// count[c] runs down to zero while the cell's records take their places: any order, the minimum has none.  The cells are
// those bins_count_kernel counted (the same function of the same bits), so every place lies in its cell's range.
template <class Item>
__global__ __launch_bounds__(kThreads) void bins_scatter_kernel(const double *__restrict__ items, i64 N, const Grid g,
                                                                const int *__restrict__ start, int *__restrict__ count,
                                                                double *__restrict__ rec)
{
    constexpr int D = Item::kDoubles;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += stride) {
        const double *s = items + D * t;
        int c0[3], c1[3];
        Item::cells(g, s, c0, c1);
        double v[D];
#pragma unroll
        for (int k = 0; k < D; ++k) v[k] = s[k];
        for (int z = c0[2]; z <= c1[2]; ++z)
            for (int y = c0[1]; y <= c1[1]; ++y)
                for (int x = c0[0]; x <= c1[0]; ++x) {
                    const int c = grid_index(g, x, y, z);
                    double *dst = rec + D * ((i64)start[c] + (atomicSub(&count[c], 1) - 1));
#pragma unroll
                    for (int k = 0; k < D; ++k) dst[k] = v[k];
                }
    }
}

// rec and start of the N items' `entries` records in g's cells, in scratch laid out on behalf of the entry point `who`
template <class Item>
int bins_build(mm_context *ctx, const char *who, const double *items_d, i64 N, i64 entries, const Grid &g, double *&rec, int *&start)
{
    const i64 ncells = (i64)g.dims[0] * g.dims[1] * g.dims[2];
    int *count, *tile_sums;
    mm_scratch_layout lay;
    lay.add(&rec, (size_t)entries * Item::kDoubles);
    lay.add(&count, (size_t)ncells + 1);
    lay.add(&start, (size_t)ncells + 1);
    lay.add(&tile_sums, mm_scan_scratch_ints(ncells));
    int rc = lay.commit(ctx, who);
    if (rc != MM_OK) return rc;
    if (mm_zero_async(ctx, count, (size_t)(ncells + 1) * sizeof(int)) != MM_OK) return MM_ERR_HIP;
    const dim3 grid(stream_grid(N)), block(kThreads);
    hipLaunchKernelGGL(bins_count_kernel<Item>, grid, block, 0, ctx->stream, items_d, N, g, count);
    MM_HIP_CHECK(hipGetLastError());
    rc = mm_exclusive_scan_int(ctx, count, ncells, start, tile_sums);
    if (rc != MM_OK) return rc;
    hipLaunchKernelGGL(bins_scatter_kernel<Item>, grid, block, 0, ctx->stream, items_d, N, g, (const int *)start, count, rec);
    return MM_OK;
}

}  // namespace
