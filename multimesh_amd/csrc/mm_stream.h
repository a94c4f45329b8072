// What a streaming or tile kernel of the model tools needs, each stated once: the launch shape, the integer count of a
// launch, the chunked sum of mm_weighted_sum, and the three expressions that are under a bit-parity contract with NumPy
// wherever they appear, the finiteness test and the order-preserving integer key of a double.  Users: mm_sphere, mm_mass,
// mm_diffusion, mm_transpose, mm_grid_sample, mm_radial, mm_precondition, mm_scattered, mm_parametrisation, mm_resolution,
// mm_frames; through mm_gll_tile.h, mm_gradient and mm_order; through mm_boundary_parts.h, mm_boundary and mm_surface.  A new
// unit starts from these.
// (The library is built with -ffp-contract=off: every product, quotient and sum below is rounded on its own.)
#pragma once

#include "mm_common.h"
#include "mm_scan.h"

namespace mm_stream {
constexpr int kThreads = 256;               // lanes of a workgroup
constexpr int kWave = 64;
constexpr int kChunk = 4096;                // values per chunk of a chunked sum (its definition, not a launch shape)
constexpr int kTerms = kChunk / kThreads;   // ... per lane
constexpr i64 kMaxBlocks = 2048;            // 256 CUs x 8 workgroups; grid-stride beyond
}  // namespace mm_stream

// ---- launch shape.  Blocks of a launch over n items, per_block of them per block and step: at least one, at most cap.
// The caps in use: mm_stream::kMaxBlocks and 8192 for kernels that stride over the rest; a kernel that does not stride
// passes the largest grid, 2^31 - 1.
inline unsigned mm_blocks(i64 n, i64 per_block, i64 cap)
{
    const i64 b = (n + per_block - 1) / per_block;
    return (unsigned)(b < cap ? (b > 0 ? b : 1) : cap);
}

// ---- counts.  Adds the wave's sum of `mine` to *counter: shuffles, then one atomic by the wave's first lane when the
// sum is not zero.  Integer sums: neither the form nor the order of the atomics reaches the result.  Every lane of the
// wave calls it.
__device__ __forceinline__ void mm_count_to(unsigned long long *counter, unsigned mine)
{
    mine = wave_sum(mine);
    if ((threadIdx.x & (mm_stream::kWave - 1)) == 0 && mine != 0) atomicAdd(counter, (unsigned long long)mine);
}

// ---- the chunked sum (the definition is published in include/multimesh_hip.h).  A block of kThreads lanes sums the
// kChunk values term(first) .. term(first + kChunk - 1), those at or past n being +0.0: lane l adds its kTerms terms
// l, l + 256, ... in that order -- from its first term (FROM_FIRST_TERM: mm_weighted_sum) or from +0.0
// (mm_binned_weighted_sum) --, then the 256 lane sums are halved eight times, s[l] = s[l] + s[l + h], h = 128 .. 1.
// s: kThreads doubles of LDS.  Every lane gets the sum.
inline i64 mm_chunks_of(i64 n) { return n <= mm_stream::kChunk ? 1 : (n + mm_stream::kChunk - 1) / mm_stream::kChunk; }

template <bool FROM_FIRST_TERM, class Term>
__device__ __forceinline__ double mm_chunk_sum(double *s, i64 first, i64 n, Term term)
{
    using namespace mm_stream;
    const int tid = threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < kTerms; ++r) {
        const i64 idx = first + r * kThreads + tid;
        if constexpr (FROM_FIRST_TERM) {
            double t = 0.0;   // (the padding of the last chunk is added)
            if (idx < n) t = term(idx);
            acc = r == 0 ? t : acc + t;
        } else if (idx < n) {
            acc = acc + term(idx);   // (a sum from +0.0 is never -0.0: adding the padding would not change it)
        }
    }
    s[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
        if (tid < h) s[tid] = s[tid] + s[tid + h];
        __syncthreads();
    }
    return s[0];
}

// The levels of a chunked sum over `count` values per row: level 0 has mm_chunks_of(count) chunk sums per row, level 1
// mm_chunks_of(that) ... down to one.  n: the levels that have more than one (count < 2^42: at most three); their chunk
// sums live in scratch, partial[l] of rows * chunks[l] doubles, and the level that has one writes the caller's output.
struct mm_sum_levels {
    int n = 0;
    i64 chunks[4] = {0, 0, 0, 0};
    double *partial[4] = {nullptr, nullptr, nullptr, nullptr};

    explicit mm_sum_levels(i64 count) { for (i64 m = mm_chunks_of(count); m > 1; m = mm_chunks_of(m)) chunks[n++] = m; }
    i64 chunks_at(int level) const { return level < n ? chunks[level] : 1; }
    void add_to(mm_scratch_layout &lay, i64 rows)
    {
        for (int l = 0; l < n; ++l) lay.add(&partial[l], (size_t)(rows * chunks[l]));
    }
};

// ---- the parity arithmetic
// np.sqrt((x * x + y * y) + z * z): x**2 is x * x in NumPy and the sum runs left to right; the f64 square root of the
// device is correctly rounded, as NumPy's is
__device__ __forceinline__ double mm_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// b + np.searchsorted(a[b:e], v, side="right"): the first index in [b, e) whose value is greater than v (a NaN sorts
// behind every value).  a: anything with a[i] -> double
template <class Axis>
__device__ __forceinline__ int mm_upper_bound(Axis a, int b, int e, double v)
{
    while (b < e) {
        const int mid = (b + e) >> 1;
        if (!(v < a[mid]))
            b = mid + 1;
        else
            e = mid;
    }
    return b;
}

// (1 - t) * p + t * q
__device__ __forceinline__ double mm_lerp(double t, double p, double q) { return (1.0 - t) * p + t * q; }

// ---- bits.  np.isfinite(v)
__device__ __forceinline__ bool mm_is_finite(double v) { return fabs(v) < __builtin_inf(); }

// The unsigned order of mm_key_of(bits of a double) is the numeric order of the doubles; mm_bits_of_key is its inverse.
__device__ __host__ __forceinline__ unsigned long long mm_key_of(unsigned long long u)
{
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __host__ __forceinline__ unsigned long long mm_bits_of_key(unsigned long long k)
{
    return (k >> 63) ? (k & ~(1ull << 63)) : ~k;
}
