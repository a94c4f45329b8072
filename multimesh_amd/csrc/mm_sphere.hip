// Earth meshes onto the sphere of their 1-D model: the reference's map_to_sphere / map_to_ellipse
// (components/interpolator.py:1085-1144) as streaming passes over the points.
//
//   mm_map_to_sphere     : p <- ((p * R) * rad) / |p| per component where |p| > 0, else p unchanged
//   mm_first_occurrence  : first[n] = min flat index i with connectivity[i] == n (np.unique(..., return_index=True))
//   mm_sphere_ratio      : (|p| / R) / rad, the radial stretch map_to_ellipse interpolates (:1093-1097)
//   mm_scale_points      : p <- factor * p, map_to_ellipse's last step (:1121)
//
// Bit parity with NumPy: |p| = sqrt((x*x + y*y) + z*z) (x**2 is x*x in NumPy, the sum runs left to right) and
// every product / quotient is rounded on its own (the library is built with -ffp-contract=off; the f64 sqrt and
// division of the device are correctly rounded, as IEEE-754 and NumPy's are).  Points whose |p| is not > 0
// (the centre, NaN) are left alone, like the reference's r > 0 mask.
//
// HBM-bound: 24 B read + 8 B radius (+ 8 B index in the node layout) + 24 B written per point, no reuse.
#include "mm_stream.h"

#include <limits.h>

namespace {

using mm_stream::kThreads;

unsigned grid_for(i64 n) { return mm_blocks(n, kThreads, 8192); }   // grid-stride beyond 2 M threads

// radius index of point i: itself (element-nodal layout) or the first occurrence of the node (node layout);
// -1 when that index is not a valid one of rad[nrad]
__device__ __forceinline__ i64 rad_index(const i64 *__restrict__ first, i64 i, i64 nrad)
{
    const i64 j = first ? first[i] : i;
    return (unsigned long long)j < (unsigned long long)nrad ? j : -1;
}

__global__ __launch_bounds__(kThreads) void map_to_sphere_kernel(const double *in, double *out, i64 npoints,
                                                                 const double *__restrict__ rad, i64 nrad,
                                                                 const i64 *__restrict__ first, double r_ref)
{
    // (in and out may be the same array: no __restrict__ on them; each thread reads its point before writing it)
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < npoints; i += stride) {
        const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
        const double r = mm_norm3(x, y, z);
        const i64 j = rad_index(first, i, nrad);
        if (r > 0.0 && j >= 0) {
            const double rr = rad[j];
            out[3 * i] = ((x * r_ref) * rr) / r;
            out[3 * i + 1] = ((y * r_ref) * rr) / r;
            out[3 * i + 2] = ((z * r_ref) * rr) / r;
        } else if (out != in) {
            out[3 * i] = x;
            out[3 * i + 1] = y;
            out[3 * i + 2] = z;
        }
    }
}

__global__ __launch_bounds__(kThreads) void sphere_ratio_kernel(const double *__restrict__ pts, i64 npoints,
                                                                const double *__restrict__ rad, i64 nrad,
                                                                const i64 *__restrict__ first, double r_ref,
                                                                double *__restrict__ ratio)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < npoints; i += stride) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const i64 j = rad_index(first, i, nrad);
        ratio[i] = j >= 0 ? (mm_norm3(x, y, z) / r_ref) / rad[j] : __builtin_nan("");
    }
}

__global__ __launch_bounds__(kThreads) void scale_points_kernel(const double *in, i64 npoints,
                                                                const double *__restrict__ factor, double *out)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < npoints; i += stride) {
        const double f = factor[i];
        const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
        out[3 * i] = f * x;
        out[3 * i + 1] = f * y;
        out[3 * i + 2] = f * z;
    }
}

__global__ __launch_bounds__(kThreads) void first_init_kernel(unsigned long long *first, i64 nnodes)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 n = (i64)blockIdx.x * blockDim.x + threadIdx.x; n < nnodes; n += stride) first[n] = ULLONG_MAX;
}

// atomicMin of the flat index into the node's slot: the result does not depend on the order of the atomics
__global__ __launch_bounds__(kThreads) void first_min_kernel(const i64 *__restrict__ conn, i64 nentries,
                                                             unsigned long long *first, i64 nnodes,
                                                             unsigned long long *out_of_range)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nentries; i += stride) {
        const i64 n = conn[i];
        if ((unsigned long long)n < (unsigned long long)nnodes)
            atomicMin(first + n, (unsigned long long)i);
        else
            atomicAdd(out_of_range, 1ull);
    }
}

// nodes no entry names get -1 and are counted
__global__ __launch_bounds__(kThreads) void first_finish_kernel(unsigned long long *first, i64 nnodes,
                                                                unsigned long long *unreferenced)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 n = (i64)blockIdx.x * blockDim.x + threadIdx.x; n < nnodes; n += stride)
        if (first[n] == ULLONG_MAX) {
            first[n] = (unsigned long long)-1ll;
            atomicAdd(unreferenced, 1ull);
        }
}

bool overlap_but_not_equal(const void *a, const void *b, size_t bytes)
{
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa != pb && pa < pb + bytes && pb < pa + bytes;
}

}  // namespace

extern "C" int mm_map_to_sphere(mm_context *ctx, const double *points_d, int64_t npoints, const double *rad_d,
                                int64_t nrad, const int64_t *first_d, double r_ref, double *out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(npoints >= 0 && nrad >= 0, "negative size");
    MM_REQUIRE(first_d != nullptr || nrad == npoints, "without first_d, rad must hold one value per point");
    MM_REQUIRE(npoints < ((i64)1 << 58), "npoints out of range");
    if (npoints == 0) return MM_OK;
    MM_REQUIRE(points_d && rad_d && out_d, "null array");
    MM_REQUIRE(!overlap_but_not_equal(points_d, out_d, (size_t)npoints * 3 * sizeof(double)),
               "out_d overlaps points_d without being it");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(map_to_sphere_kernel, dim3(grid_for(npoints)), dim3(kThreads), 0, ctx->stream, points_d, out_d,
                       npoints, rad_d, nrad, (const i64 *)first_d, r_ref);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int64_t mm_first_occurrence(mm_context *ctx, const int64_t *connectivity_d, int64_t nentries, int64_t nnodes,
                                       int64_t *first_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(nentries >= 0 && nnodes >= 0, "negative size");
    MM_REQUIRE(nentries < ((i64)1 << 60) && nnodes < ((i64)1 << 60), "size out of range");
    if (nnodes == 0 && nentries == 0) return 0;
    MM_REQUIRE(first_d != nullptr || nnodes == 0, "null array");
    MM_REQUIRE(connectivity_d != nullptr || nentries == 0, "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    unsigned long long *counters = mm_counters_begin(ctx, 2, 2);   // [0] unreferenced, [1] out of range
    if (!counters) return MM_ERR_HIP;
    unsigned long long *first = (unsigned long long *)first_d;
    if (nnodes > 0)
        hipLaunchKernelGGL(first_init_kernel, dim3(grid_for(nnodes)), dim3(kThreads), 0, ctx->stream, first, nnodes);
    if (nentries > 0)
        hipLaunchKernelGGL(first_min_kernel, dim3(grid_for(nentries)), dim3(kThreads), 0, ctx->stream,
                           (const i64 *)connectivity_d, nentries, first, nnodes, counters + 1);
    if (nnodes > 0)
        hipLaunchKernelGGL(first_finish_kernel, dim3(grid_for(nnodes)), dim3(kThreads), 0, ctx->stream, first, nnodes,
                           counters);
    const i64 *count = mm_counters_end(ctx, 2, 2);
    if (!count) return MM_ERR_HIP;
    if (count[1] != 0) {
        mm_set_error(MM_ERR_ARG, "mm_first_occurrence: %lld connectivity entries outside [0, %lld)", (long long)count[1],
                     (long long)nnodes);
        return MM_ERR_ARG;
    }
    return count[0];
}

extern "C" int mm_sphere_ratio(mm_context *ctx, const double *points_d, int64_t npoints, const double *rad_d,
                               int64_t nrad, const int64_t *first_d, double r_ref, double *ratio_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(npoints >= 0 && nrad >= 0, "negative size");
    MM_REQUIRE(first_d != nullptr || nrad == npoints, "without first_d, rad must hold one value per point");
    MM_REQUIRE(npoints < ((i64)1 << 58), "npoints out of range");
    if (npoints == 0) return MM_OK;
    MM_REQUIRE(points_d && rad_d && ratio_d, "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(sphere_ratio_kernel, dim3(grid_for(npoints)), dim3(kThreads), 0, ctx->stream, points_d, npoints,
                       rad_d, nrad, (const i64 *)first_d, r_ref, ratio_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_scale_points(mm_context *ctx, const double *points_d, int64_t npoints, const double *factor_d,
                               double *out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(npoints >= 0, "negative size");
    MM_REQUIRE(npoints < ((i64)1 << 58), "npoints out of range");
    if (npoints == 0) return MM_OK;
    MM_REQUIRE(points_d && factor_d && out_d, "null array");
    MM_REQUIRE(!overlap_but_not_equal(points_d, out_d, (size_t)npoints * 3 * sizeof(double)),
               "out_d overlaps points_d without being it");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(scale_points_kernel, dim3(grid_for(npoints)), dim3(kThreads), 0, ctx->stream, points_d, npoints,
                       factor_d, out_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
