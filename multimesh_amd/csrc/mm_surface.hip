// The boundary of a mesh as a surface: its selected faces as triangles through their GLL nodes, and the exact distance of
// points to those triangles, with a cutoff or with none (include/multimesh_surface.h holds the statements).
//
//   mm_boundary_triangles : 2 order^2 triangles per selected face, face by face -- mm_boundary_nodes' sibling
//   mm_surface_distance   : d = min(cutoff, min over the triangles of |p - closest(p; a, b, c)|)
//
// Bit parity with the NumPy statements (tests/surface_cases.py): every product, quotient and sum is rounded on its own
// (-ffp-contract=off), and a lane evaluates the statement's own region walk for every triangle it meets.  Integer atomics
// only, and none of them reaches a result through its order: the histogram of the triangles' sizes and the entry count are
// integer sums that only choose the cell edge, which decides WHICH triangles a lane evaluates beyond those that matter,
// never what a distance is; the order of the records within a cell is free because a minimum has none.
//
// The search ("Boundaries", has the derivation in full).  A uniform grid of cells of edge h over the
// bounding box [lo, hi] of the triangles' vertices; h follows the triangles -- 2^(e + 1) with 2^e <= the median of their
// largest bounding-box extents < 2^(e + 1), from a histogram of the exponents -- and not the cutoff; it is enlarged until
// the grid fits mm_cutoff_distance's caps (1024 cells per axis, 2^22 in all: mm_search_grid_fit) and until the entries are
// at most 16 T.  The grid, its cells and its bins are mm_cutoff_distance's (mm_search_grid.h, mm_boundary_parts.h).  The
// cell of a coordinate is clamp(floor(fl(fl(x - lo) * inv_h)), 0, dims - 1), a MONOTONE function of x, so a triangle
// entered into the cells of its bounding box's corners and all between is in the cell of each of its points.  A lane walks
// the Chebyshev rings k = 0, 1, ... of cells around the cell of p' = clamp(p, lo, hi) and stops when
//     sqrt(E^2 + (g h)^2) * (1 - 2^-24) - 2^-36 * (M + |p|) >= d,
// E = |p - p'|, g = the least of fl(v(p'_a) - x0_a) and fl((x1_a + 1) - v(p'_a)) over the block's faces that are not the
// grid's own, v the unfloored cell index, M the largest |coordinate| of the box, d the best distance so far (the cutoff at
// the start, so the cutoff ends the walk too).  A triangle that is in no cell of the block has all its points at an index
// below x0 or above x1 on some axis, which puts them more than g h (1 - 2^-40) - 2^-40 h from p' on that axis; projection
// onto the box is a contraction, per axis and with the sign kept, so |p - y|^2 >= E^2 + |p' - y|^2 for every y in the box.
#include "mm_boundary_parts.h"
#include "multimesh_surface.h"

namespace {

constexpr int kAuxSlot = 28, kAuxWords = 2;   // d_counters words 28..29: [0] the entries of a grid, [1] the median exponent
constexpr int kHistBins = 2048;               // one per binary exponent of a double
constexpr i64 kEntryCap = 16;                 // entries of the grid per triangle, at most
constexpr double kShrink = 1.0 - 0x1p-24;     // the stopping bound's relative and absolute margins
constexpr double kAbsMargin = 0x1p-36;
constexpr double kMinEdge = 0x1p-1000;

// ------------------------------------------------------------------------------------------- mm_boundary_triangles
// (select_kernel, face_items_kernel and their driver: mm_boundary_parts.h)
// the 2 o^2 triangles of a face: k = 2 * (j * o + i) + (0: the triangle at (j, i)'s lower side, 1: the other)
struct TriangleItems {
    static constexpr int kDoubles = 9;
    __host__ __device__ static int per_face(int m) { return 2 * (m - 1) * (m - 1); }
    __device__ static void write(const double *__restrict__ X, int m, const Face &face, int k, double *__restrict__ dst)
    {
        const int o = m - 1, second = k & 1, j = (k >> 1) / o, i = (k >> 1) - j * o;
        // the vertices (lo, hi) on the face's grid: (i, j), then (i+1, j), (i+1, j+1) or (i+1, j+1), (i, j+1)
        const int vlo[3] = {i, i + 1, second ? i : i + 1}, vhi[3] = {j, second ? j + 1 : j, j + 1};
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const double *src = X + 3 * face_node(face.a, face.fix, m, vlo[v], vhi[v]);
            dst[3 * v] = src[0], dst[3 * v + 1] = src[1], dst[3 * v + 2] = src[2];
        }
    }
};

// --------------------------------------------------------------------------------------------- mm_surface_distance
__device__ __forceinline__ double dot3(const double (&u)[3], const double (&v)[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// the statement's r for the triangle at s[0..8]: the region walk, branch by branch as the header writes it
__device__ __forceinline__ double triangle_distance(const double (&p)[3], const double *__restrict__ s)
{
    double a[3], b[3], c[3], ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = s[k], b[k] = s[3 + k], c[k] = s[6 + k];
        ab[k] = b[k] - a[k], ac[k] = c[k] - a[k];
        ap[k] = p[k] - a[k], bp[k] = p[k] - b[k], cp[k] = p[k] - c[k];
    }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    if (d1 <= 0.0 && d2 <= 0.0) {
        q[0] = a[0], q[1] = a[1], q[2] = a[2];
    } else if (d3 >= 0.0 && d4 <= d3) {
        q[0] = b[0], q[1] = b[1], q[2] = b[2];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k] + v * ab[k];
    } else if (d6 >= 0.0 && d5 <= d6) {
        q[0] = c[0], q[1] = c[1], q[2] = c[2];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k] + w * ac[k];
    } else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
        const double w = e43 / (e43 + e56);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = b[k] + w * (c[k] - b[k]);
    } else {
        const double den = 1.0 / ((va + vb) + vc);
        const double v = vb * den, w = vc * den;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
    }
    return mm_norm3(p[0] - q[0], p[1] - q[1], p[2] - q[2]);
}

// a triangle is a record in every cell [c0[a], c1[a]] per axis that its bounding box overlaps
struct TriangleBins {
    static constexpr int kDoubles = 9;
    __device__ static void cells(const Grid &g, const double *__restrict__ s, int (&c0)[3], int (&c1)[3])
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c0[a] = grid_cell(g, a, fmin(fmin(s[a], s[3 + a]), s[6 + a]));
            c1[a] = grid_cell(g, a, fmax(fmax(s[a], s[3 + a]), s[6 + a]));
        }
    }
};

// hist[e] += the triangles whose largest bounding-box extent has the binary exponent field e (through LDS: the triangles
// of a mesh are of one size, and a global atomic per triangle would queue on one address)
__global__ __launch_bounds__(kThreads) void extent_hist_kernel(const double *__restrict__ tri, i64 T, int *__restrict__ hist)
{
    __shared__ int local[kHistBins];
    for (int e = threadIdx.x; e < kHistBins; e += kThreads) local[e] = 0;
    __syncthreads();
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        const double *s = tri + 9 * t;
        double ext = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            ext = fmax(ext, fmax(fmax(s[a], s[3 + a]), s[6 + a]) - fmin(fmin(s[a], s[3 + a]), s[6 + a]));
        atomicAdd(&local[(int)(((u64)__double_as_longlong(ext) >> 52) & 0x7ff)], 1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kHistBins; e += kThreads)
        if (local[e] != 0) atomicAdd(&hist[e], local[e]);
}

// *out = the exponent field at which the running count of hist first reaches (T + 1) / 2; one workgroup
__global__ __launch_bounds__(kThreads) void median_bin_kernel(const int *__restrict__ hist, i64 T, u64 *out)
{
    __shared__ i64 part[kThreads];
    constexpr int per = kHistBins / kThreads;
    i64 sum = 0;
    for (int e = 0; e < per; ++e) sum += hist[threadIdx.x * per + e];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const i64 need = (T + 1) / 2;
    i64 run = 0;
    int t = 0;
    while (t < kThreads - 1 && run + part[t] < need) run += part[t++];
    int e = t * per;
    while (e < kHistBins - 1 && run + hist[e] < need) run += hist[e++];
    *out = (u64)e;
}

// *total += the entries of the grid: the cells every triangle's bounding box overlaps
__global__ __launch_bounds__(kThreads) void entries_total_kernel(const double *__restrict__ tri, i64 T, const Grid g, u64 *total)
{
    u64 mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        int c0[3], c1[3];
        TriangleBins::cells(g, tri + 9 * t, c0, c1);
        mine += (u64)(c1[0] - c0[0] + 1) * (u64)(c1[1] - c0[1] + 1) * (u64)(c1[2] - c0[2] + 1);   // (below 2^30 each)
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & (kWave - 1)) == 0 && mine != 0) atomicAdd(total, mine);
}

// One lane per point.  start == nullptr: no triangles, every distance is the cutoff.
__global__ __launch_bounds__(kThreads) void surface_query_kernel(const double *__restrict__ pts, i64 n, const double *__restrict__ rec,
                                                                 const int *__restrict__ start, const Grid g, double cutoff,
                                                                 double *__restrict__ dist, u64 *count)
{
    unsigned mine = 0;
    const int dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        double d = cutoff;
        // (a point with a coordinate that is not finite keeps the cutoff: its r is inf or a NaN for every triangle)
        if (start && mm_is_finite(p[0]) && mm_is_finite(p[1]) && mm_is_finite(p[2])) {
            double e[3], v[3], pmax = 0.0;
            int c[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double pc = fmin(fmax(p[a], g.lo[a]), g.hi[a]);   // p', the projection onto the box
                e[a] = p[a] - pc;
                v[a] = grid_coord(g, a, pc);                            // >= 0
                const double fl = floor(v[a]);                          // grid_cell(p'), whose lower clamp cannot act
                c[a] = fl < (double)g.dims[a] ? (int)fl : g.dims[a] - 1;
                pmax = fmax(pmax, fabs(p[a]));
            }
            const double E = mm_norm3(e[0], e[1], e[2]);
            const double slack = kAbsMargin * (g.mbox + pmax);
            auto scan = [&](int first, int last) {   // the records of the cells first .. last of one row: one run
                const int b = start[first], end = start[last + 1];
                const double *s = rec + 9 * (i64)b;   // (64-bit: 9 * entries passes 2^31)
                for (int j = b; j < end; ++j, s += 9) {
                    const double r = triangle_distance(p, s);
                    if (r < d) d = r;
                }
            };
            if (!(E * kShrink - slack >= cutoff)) {   // (else: farther than the cutoff from the box, done at once)
                for (int k = 0;; ++k) {
                    const int x0 = c[0] - k > 0 ? c[0] - k : 0, x1 = c[0] + k < dx ? c[0] + k : dx - 1;
                    const int y0 = c[1] - k > 0 ? c[1] - k : 0, y1 = c[1] + k < dy ? c[1] + k : dy - 1;
                    const int z0 = c[2] - k > 0 ? c[2] - k : 0, z1 = c[2] + k < dz ? c[2] + k : dz - 1;
                    // the shell of ring k inside the grid: whole rows on its z and y faces, the two end cells elsewhere
                    for (int z = z0; z <= z1; ++z) {
                        const bool zface = z == c[2] - k || z == c[2] + k;
                        for (int y = y0; y <= y1; ++y) {
                            const int row = grid_index(g, 0, y, z);
                            if (zface || y == c[1] - k || y == c[1] + k) {
                                scan(row + x0, row + x1);
                            } else {
                                if (c[0] - k >= 0) scan(row + c[0] - k, row + c[0] - k);
                                if (c[0] + k < dx) scan(row + c[0] + k, row + c[0] + k);
                            }
                        }
                    }
                    if (x0 == 0 && x1 == dx - 1 && y0 == 0 && y1 == dy - 1 && z0 == 0 && z1 == dz - 1) break;   // every cell
                    double gap = __builtin_inf();
                    if (x0 > 0) gap = fmin(gap, v[0] - (double)x0);
                    if (x1 < dx - 1) gap = fmin(gap, (double)(x1 + 1) - v[0]);
                    if (y0 > 0) gap = fmin(gap, v[1] - (double)y0);
                    if (y1 < dy - 1) gap = fmin(gap, (double)(y1 + 1) - v[1]);
                    if (z0 > 0) gap = fmin(gap, v[2] - (double)z0);
                    if (z1 < dz - 1) gap = fmin(gap, (double)(z1 + 1) - v[2]);
                    const double gh = gap * g.h;
                    if (sqrt(E * E + gh * gh) * kShrink - slack >= d) break;
                }
            }
        }
        dist[i] = d;
        mine += d < cutoff;
    }
    mm_count_to(count, mine);
}

}  // namespace

extern "C" int64_t mm_boundary_triangles(mm_context *ctx, const double *points_d, int64_t nelem, int order, const int64_t *faces_d,
                                         const int *side_d, int64_t nb, int side_mask, double *tri_d)
{
    return selected_face_items<TriangleItems>(ctx, __func__, points_d, nelem, order, (const i64 *)faces_d, side_d, nb, side_mask,
                                              tri_d);
}

extern "C" int64_t mm_surface_distance(mm_context *ctx, const double *points_d, int64_t n, const double *tri_d, int64_t T,
                                       double cutoff, double *dist_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 48), "n out of range");
    MM_REQUIRE(T >= 0 && T < ((i64)1 << 30), "T must lie in [0, 2^30)");
    MM_REQUIRE(cutoff > 0.0, "cutoff must be positive (+inf: no cutoff)");   // (a NaN fails the test)
    MM_REQUIRE(cutoff >= kMinCutoff, "cutoff below 2^-500: the squares of the offsets would underflow under the margin");
    MM_REQUIRE(n == 0 || (points_d != nullptr && dist_d != nullptr), "null points or distances");
    MM_REQUIRE(T == 0 || tri_d != nullptr, "null triangles");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    u64 *words = mm_counters_begin(ctx, kSlot, kWords);   // [0] points with d < cutoff, [1] bad coordinates, [2..7] the box
    if (!words) return MM_ERR_HIP;
    Grid g = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 1.0, 1.0, 0.0, {1, 1, 1}};
    double *rec = nullptr;
    int *start = nullptr;
    if (T > 0) {
        const dim3 grid(stream_grid(T)), block(kThreads);
        u64 *aux = mm_counters_begin(ctx, kAuxSlot, kAuxWords);
        if (!aux) return MM_ERR_HIP;
        int *hist;
        mm_scratch_layout first;
        first.add(&hist, (size_t)kHistBins);
        int rc = first.commit(ctx, __func__);
        if (rc != MM_OK) return rc;
        if (mm_zero_async(ctx, hist, kHistBins * sizeof(int)) != MM_OK) return MM_ERR_HIP;
        hipLaunchKernelGGL(sources_box_kernel, dim3(stream_grid(3 * T)), block, 0, ctx->stream, tri_d, (i64)(3 * T), words);
        hipLaunchKernelGGL(extent_hist_kernel, grid, block, 0, ctx->stream, tri_d, (i64)T, hist);
        hipLaunchKernelGGL(median_bin_kernel, dim3(1), block, 0, ctx->stream, (const int *)hist, (i64)T, aux + 1);
        const i64 *got = mm_counters_end(ctx, kSlot, kWords);
        if (!got) return MM_ERR_HIP;
        if (got[1] != 0) {
            mm_set_error(MM_ERR_ARG, "mm_surface_distance: %lld triangle vertices are not finite", (long long)got[1]);
            return MM_ERR_ARG;
        }
        box_of_words(got, g.lo, g.hi);
        double extent[3], widest = 0.0;
        for (int a = 0; a < 3; ++a) {
            extent[a] = g.hi[a] - g.lo[a];
            MM_REQUIRE(extent[a] < __builtin_inf(), "the triangles' extent overflows");
            widest = fmax(widest, extent[a]);
            g.mbox = fmax(g.mbox, fmax(fabs(g.lo[a]), fabs(g.hi[a])));
        }
        got = mm_counters_end(ctx, kAuxSlot, kAuxWords);
        if (!got) return MM_ERR_HIP;
        // the edge: 2^(e + 1) for the median exponent e -- between one and two median extents --; the box's widest extent
        // when the median triangle has no extent to speak of; any edge serves a box that is a point
        const int e_med = (int)got[1];
        double h = e_med >= 1 && e_med <= 2045 ? ldexp(1.0, e_med - 1023 + 1) : widest;
        if (!(h >= kMinEdge && h < __builtin_inf())) h = 1.0;
        for (;; h = g.h * 1.5) {
            // enlarged until the grid fits its caps and the entries their cap (a larger edge keeps the search valid); one cell
            // holds T entries, so this ends
            mm_search_grid_fit(g, extent, h, 1);
            aux = mm_counters_begin(ctx, kAuxSlot, 1);
            if (!aux) return MM_ERR_HIP;
            hipLaunchKernelGGL(entries_total_kernel, grid, block, 0, ctx->stream, tri_d, (i64)T, g, aux);
            got = mm_counters_end(ctx, kAuxSlot, 1);
            if (!got) return MM_ERR_HIP;
            if (got[0] <= kEntryCap * T && got[0] < ((i64)1 << 31) - 1) break;
        }
        rc = bins_build<TriangleBins>(ctx, __func__, tri_d, T, got[0], g, rec, start);
        if (rc != MM_OK) return rc;
    }
    if (n > 0)
        hipLaunchKernelGGL(surface_query_kernel, dim3(stream_grid(n)), dim3(kThreads), 0, ctx->stream, points_d, (i64)n,
                           (const double *)rec, (const int *)start, g, cutoff, dist_d, words);
    const i64 *got = mm_counters_end(ctx, kSlot, 1);
    return got ? got[0] : MM_ERR_HIP;
}
