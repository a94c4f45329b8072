// Scattered point models: the rows (index, distance) of a k-nearest-neighbour query turned into values by inverse-distance
// weights relative to the nearest sample -- mm_idw_gather, the value half of the scattered import (mm_knn_query is the
// search half).  One lane per target in a grid-stride loop; per target, for j ascending:
//
//   valid_j = 0 <= idx[j] < nsrc and dist[j] <= max_distance      m = the number of valid j      d0 = the first valid dist
//   exact hit (a valid dist == 0.0, the lowest such j): the sample's bits
//   else r = d0 / dist[j];  q = r * r * ... (power factors, left to right);  w = valid ? q : 0.0;  v = valid ? field : 0.0
//        s = s + w;  num = num + (w * v)  from 0.0;  out = num / s
//
// Every quotient, product and sum is rounded on its own (the library is built with -ffp-contract=off), so the values are
// bit for bit the NumPy statement of include/multimesh_hip.h on the same idx / dist.  d0 is known when the first valid
// entry arrives and every entry before it has weight 0, so one pass over the row serves; an exact hit found later in the
// row discards the sums.
//
// Traffic: 16 * k B of rows read per target, 8 * k B gathered and 8 B written per component.  The rows are k * 8 B apart
// from lane to lane.  A lane reads its row 16 bytes at a time (global_load_dwordx4: two entries) when k is even and both
// arrays start on 16 bytes, 8 bytes at a time otherwise: a wave-instruction then covers 64 pieces of one width in 64 rows,
// every 128-byte line it touches is consumed whole by the same wave's next instructions, and no byte is fetched twice from
// HBM.  Staging a workgroup's rows through LDS would make each instruction contiguous, but a workgroup's rows are
// 256 * k * 16 B (256 KiB at k = 64, more than the LDS), so it would need a second loop over pieces of the row and a
// barrier per piece, for a kernel whose time goes to the C * k gathered 8-byte reads that no layout of the rows changes
// ("Scattered import").  Component-major output is written coalesced (lane i writes out[c][i]).
//
// Components: 1..4 are accumulators in registers inside the j loop; more go through in groups of four, each group one
// more pass over the row (which is in L1 / L2 by then).  The outside count is summed per workgroup -- shuffles, then the
// four wave sums through LDS -- and added by one integer atomic: its order cannot reach the result.
#include "mm_stream.h"

#include <limits.h>

namespace {

using mm_stream::kThreads;
using mm_stream::kWave;
using mm_stream::kMaxBlocks;
typedef unsigned long long u64;
constexpr int kGroup = 4;          // components held in registers at once

enum { kFill = 0, kKeep = 2 };

struct IdwArgs {
    const double *fields;
    i64 nsrc;
    int ncomp;
    const i64 *idx;
    const double *dist;
    i64 npoints;
    int k, power;
    double max_distance;
    int outside;
    double fill;
    double *out;
    int point_major;
    double *nearest;
    int *nused;
    u64 *count;
};

template <int NC>
struct RowState {
    int m = 0;
    bool hit = false;
    i64 hit_id = 0;
    double d0 = 0.0, s = 0.0;
    double num[NC ? NC : 1];
};

// one entry of a row; f: the first of this group's NC components
template <int NC>
__device__ __forceinline__ void idw_entry(const IdwArgs &a, const double *__restrict__ f, i64 id, double d, RowState<NC> &st)
{
    // (a NaN distance fails the comparison; the unsigned comparison refuses negative indices and the padding nsrc)
    const bool valid = (u64)id < (u64)a.nsrc && d <= a.max_distance;
    if (valid && st.m == 0) st.d0 = d;
    st.m += valid ? 1 : 0;
    if (valid && d == 0.0 && !st.hit) {
        st.hit = true;
        st.hit_id = id;
    }
    const double r = st.d0 / d;
    double q = r;
    for (int p = 1; p < a.power; ++p) q = q * r;
    const double w = valid ? q : 0.0;
    st.s = st.s + w;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double v = 0.0;
        if (valid) v = f[(i64)c * a.nsrc + id];   // (an invalid entry's field is never read)
        st.num[c] = st.num[c] + (w * v);
    }
}

// The row of target i for the NC components from c0 on: the values are written, the state comes back.
template <int NC, bool VEC>
__device__ __forceinline__ RowState<NC> idw_row(const IdwArgs &a, i64 i, int c0)
{
    RowState<NC> st;
#pragma unroll
    for (int c = 0; c < NC; ++c) st.num[c] = 0.0;
    const double *f = a.fields + (i64)c0 * a.nsrc;
    const i64 row = i * a.k;
    if (VEC) {
        const longlong2 *ip = reinterpret_cast<const longlong2 *>(a.idx + row);
        const double2 *dp = reinterpret_cast<const double2 *>(a.dist + row);
        const int pairs = a.k >> 1;
#pragma unroll 2
        for (int j = 0; j < pairs; ++j) {
            const longlong2 id = ip[j];
            const double2 d = dp[j];
            idw_entry<NC>(a, f, id.x, d.x, st);
            idw_entry<NC>(a, f, id.y, d.y, st);
        }
    } else {
#pragma unroll 2
        for (int j = 0; j < a.k; ++j) idw_entry<NC>(a, f, a.idx[row + j], a.dist[row + j], st);
    }
    if (NC) {
        const i64 n = a.npoints;
        if (st.m == 0) {
            if (a.outside == kFill) {
#pragma unroll
                for (int c = 0; c < NC; ++c) a.out[a.point_major ? i * a.ncomp + c0 + c : (i64)(c0 + c) * n + i] = a.fill;
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double v = st.hit ? f[(i64)c * a.nsrc + st.hit_id] : st.num[c] / st.s;
                a.out[a.point_major ? i * a.ncomp + c0 + c : (i64)(c0 + c) * n + i] = v;
            }
        }
    }
    return st;
}

// NC: the components (0..4) held in registers; kGroup + 1: any number, in groups.  VEC: rows are read 16 bytes at a time.
template <int NC, bool VEC>
__global__ __launch_bounds__(kThreads) void idw_gather_kernel(const IdwArgs a)
{
    __shared__ unsigned s_count[kThreads / kWave];
    unsigned outside = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < a.npoints; i += stride) {
        int m;
        double d0;
        if (NC <= kGroup) {
            const RowState<NC> st = idw_row<NC, VEC>(a, i, 0);
            m = st.m, d0 = st.d0;
        } else {
            const RowState<kGroup> st = idw_row<kGroup, VEC>(a, i, 0);
            m = st.m, d0 = st.d0;
            int c0 = kGroup;
            for (; c0 + kGroup <= a.ncomp; c0 += kGroup) idw_row<kGroup, VEC>(a, i, c0);
            switch (a.ncomp - c0) {
            case 1: idw_row<1, VEC>(a, i, c0); break;
            case 2: idw_row<2, VEC>(a, i, c0); break;
            case 3: idw_row<3, VEC>(a, i, c0); break;
            default: break;
            }
        }
        outside += m == 0;
        if (a.nearest) a.nearest[i] = m == 0 ? __builtin_inf() : d0;
        if (a.nused) a.nused[i] = m;
    }
    // one integer atomic per workgroup
    outside = wave_sum(outside);
    if ((threadIdx.x & (kWave - 1)) == 0) s_count[threadIdx.x / kWave] = outside;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / kWave; ++w) total += s_count[w];
        if (total != 0) atomicAdd(a.count, (u64)total);
    }
}

template <bool VEC>
void launch(mm_context *ctx, const IdwArgs &a, unsigned grid)
{
    const dim3 g(grid), b(kThreads);
    switch (a.ncomp) {
    case 0: hipLaunchKernelGGL((idw_gather_kernel<0, VEC>), g, b, 0, ctx->stream, a); break;
    case 1: hipLaunchKernelGGL((idw_gather_kernel<1, VEC>), g, b, 0, ctx->stream, a); break;
    case 2: hipLaunchKernelGGL((idw_gather_kernel<2, VEC>), g, b, 0, ctx->stream, a); break;
    case 3: hipLaunchKernelGGL((idw_gather_kernel<3, VEC>), g, b, 0, ctx->stream, a); break;
    case 4: hipLaunchKernelGGL((idw_gather_kernel<4, VEC>), g, b, 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL((idw_gather_kernel<kGroup + 1, VEC>), g, b, 0, ctx->stream, a); break;
    }
}

}  // namespace

extern "C" int64_t mm_idw_gather(mm_context *ctx, const double *fields_d, int64_t nsrc, int64_t ncomp, const int64_t *idx_d,
                                 const double *dist_d, int64_t npoints, int64_t k, int power, double max_distance, int outside,
                                 double fill_value, double *out_d, int out_point_major, double *nearest_out_d,
                                 int32_t *nused_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(nsrc >= 0 && ncomp >= 0 && npoints >= 0, "negative size");
    MM_REQUIRE(ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(k >= 1 && k <= MM_KNN_MAX_K, "k must be in 1..MM_KNN_MAX_K");
    MM_REQUIRE(power >= 1 && power <= 8, "power must be an integer in 1..8");
    MM_REQUIRE(max_distance >= 0.0, "max_distance must not be negative or a NaN (+inf: no limit)");
    MM_REQUIRE(outside == kFill || outside == kKeep, "outside must be 0 (fill) or 2 (keep)");
    MM_REQUIRE(npoints == 0 || (idx_d != nullptr && dist_d != nullptr), "null idx or dist");
    MM_REQUIRE(npoints == 0 || ncomp == 0 || (out_d != nullptr && (fields_d != nullptr || nsrc == 0)), "null fields or output");
    if (npoints >= ((i64)1 << 48) || nsrc > LLONG_MAX / 8 / (ncomp > 0 ? ncomp : 1)) {
        mm_set_error(MM_ERR_UNSUPPORTED, "mm_idw_gather: the point count or the size of the fields is out of range");
        return MM_ERR_UNSUPPORTED;
    }
    if (npoints == 0) return 0;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    u64 *counter = mm_counters_begin(ctx, 0, 1);
    if (!counter) return MM_ERR_HIP;
    IdwArgs a;
    a.fields = fields_d;
    a.nsrc = nsrc;
    a.ncomp = (int)ncomp;
    a.idx = (const i64 *)idx_d;
    a.dist = dist_d;
    a.npoints = npoints;
    a.k = (int)k;
    a.power = power;
    a.max_distance = max_distance;
    a.outside = outside;
    a.fill = fill_value;
    a.out = out_d;
    a.point_major = out_point_major ? 1 : 0;
    a.nearest = nearest_out_d;
    a.nused = nused_out_d;
    a.count = counter;
    const unsigned grid = mm_blocks(npoints, kThreads, kMaxBlocks);
    // rows of an even k whose arrays start on 16 bytes are read two entries at a time; any other view 8 bytes at a time
    if ((k & 1) == 0 && (((uintptr_t)idx_d | (uintptr_t)dist_d) & 15) == 0)
        launch<true>(ctx, a, grid);
    else
        launch<false>(ctx, a, grid);
    const i64 *count = mm_counters_end(ctx, 0, 1);
    return count ? count[0] : MM_ERR_HIP;
}
