// What mm_boundary.hip and mm_surface.hip both need, each stated once: the launch shape of their streaming kernels, the
// counter words of mm_context::d_counters they own, the caps of a search grid, the selection of boundary faces by side and
// the bounding box of a cloud of points by integer maxima (with its decoding on the host).
#pragma once

#include "mm_stream.h"

#include <math.h>
#include <string.h>

namespace {

using namespace mm_stream;   // kThreads, kWave
typedef unsigned long long u64;
constexpr i64 kMaxBlocks = 2048;           // 256 CUs x 8 workgroups; grid-stride beyond
constexpr int kSlot = 16, kWords = 8;      // the units' words of mm_context::d_counters (mm_common.h)
constexpr int kMaxDim = 1024;              // cells per axis of a search grid
constexpr i64 kMaxCells = (i64)1 << 22;    // ... and in all
constexpr double kMinCutoff = 0x1p-500;

unsigned stream_grid(i64 n) { return mm_blocks(n, kThreads, kMaxBlocks); }

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) < __builtin_inf(); }

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

// The unsigned order of key_of(bits) is the numeric order of the doubles (mm_precondition.hip's select uses the same key).
__device__ __host__ __forceinline__ u64 key_of(u64 u) { return (u >> 63) ? ~u : (u | ((u64)1 << 63)); }
__device__ __host__ __forceinline__ u64 bits_of_key(u64 k) { return (k >> 63) ? (k & ~((u64)1 << 63)) : ~k; }

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
        if (is_finite(x[0]) && is_finite(x[1]) && is_finite(x[2])) {
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
            atomicMax(words + 2 + a, ~key_of((u64)__double_as_longlong(b[2 * a])));
            atomicMax(words + 5 + a, key_of((u64)__double_as_longlong(b[2 * a + 1])));
        }
    }
    mm_count_to(words + 1, mine);
}

// the box of sources_box_kernel's words as read back: lo[a], hi[a] (every source was finite and there was one)
inline void box_of_words(const i64 *got, double (&lo)[3], double (&hi)[3])
{
    for (int a = 0; a < 3; ++a) {
        const u64 lo_bits = bits_of_key(~(u64)got[2 + a]), hi_bits = bits_of_key((u64)got[5 + a]);
        memcpy(&lo[a], &lo_bits, sizeof(double));
        memcpy(&hi[a], &hi_bits, sizeof(double));
    }
}

}  // namespace
