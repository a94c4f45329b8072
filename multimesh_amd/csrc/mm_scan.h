// The device scan, stated once: the wave and block primitives, the tile a workgroup of the scan covers, the first kernel
// of mm_exclusive_scan_int and the launcher of the whole scan.  Users: mm_scan.hip (the scan itself, which mm_unique,
// mm_unique_hash, mm_boundary, mm_locate_gll, mm_radix_sort and the kNN tree call through mm_common.h), mm_knn.hip (the
// counting sorts -- the build's grid statistic rides on the first kernel as a hook --, the lane work list, the group scans
// of the tiled kernels, the DPP scans of the lane kernel), mm_radix_sort.hip (the tile's digit offsets), mm_scattered.hip
// and, through mm_stream.h, every user of mm_count_to (the wave sum).  A new unit that counts, ranks or compacts starts here.
// Scratch is sized by mm_scan_scratch_ints (mm_common.h): nothing outside this header knows the tile size.
#pragma once

#include "mm_common.h"

constexpr int kScanBlock = 256;                        // lanes of a scan workgroup
constexpr int kScanItems = 4;                          // items per thread
constexpr int kScanTile = kScanBlock * kScanItems;     // items per block
// at most this many tiles: the last kernel sums the tiles before its own itself (mm_scan_launch_tail)
constexpr int kScanSelfTiles = 2048;

inline int mm_scan_tiles(i64 n) { return (int)((n + kScanTile - 1) / kScanTile); }

// ---- wave primitives
// the wave's sum of v by halving with __shfl_down: lane 0 holds it (the other lanes hold partial sums)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// inclusive prefix sum inside groups of S consecutive lanes (S a power of two)
__device__ __forceinline__ int group_scan(int v, int sl, int S)
{
    for (int d = 1; d < S; d <<= 1) {
        const int t = __shfl_up(v, d, S);
        if (sl >= d) v += t;
    }
    return v;
}

// Wave-wide inclusive prefix sum / maximum with DPP moves (row_shr 1, 2, 4, 8 inside the rows of 16 lanes, then the
// row broadcasts 15 and 31): six VALU instructions with a few cycles of latency each, where __shfl_up is a
// ds_bpermute through the LDS crossbar (~100 cycles each, six of them dependent).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_from(int v, int fill)
{
    // lanes without a source lane (shifted in from outside the row / rows not in ROW_MASK) read `fill`
    return __builtin_amdgcn_update_dpp(fill, v, CTRL, ROW_MASK, 0xF, false);
}

__device__ __forceinline__ int wave_inclusive_sum(int v)
{
    v += dpp_from<0x111, 0xF>(v, 0);   // row_shr:1
    v += dpp_from<0x112, 0xF>(v, 0);   // row_shr:2
    v += dpp_from<0x114, 0xF>(v, 0);   // row_shr:4
    v += dpp_from<0x118, 0xF>(v, 0);   // row_shr:8
    v += dpp_from<0x142, 0xA>(v, 0);   // row_bcast:15 -> rows 1 and 3
    v += dpp_from<0x143, 0xC>(v, 0);   // row_bcast:31 -> rows 2 and 3
    return v;
}

// maximum over the wave of non-negative values (every lane's result is only meaningful in lane 63: read it there)
__device__ __forceinline__ int wave_max_nonneg(int v)
{
    v = max(v, dpp_from<0x111, 0xF>(v, 0));
    v = max(v, dpp_from<0x112, 0xF>(v, 0));
    v = max(v, dpp_from<0x114, 0xF>(v, 0));
    v = max(v, dpp_from<0x118, 0xF>(v, 0));
    v = max(v, dpp_from<0x142, 0xA>(v, 0));
    v = max(v, dpp_from<0x143, 0xC>(v, 0));
    return __builtin_amdgcn_readlane(v, 63);
}

// ---- the block scan (kScanBlock lanes, every one of them calls it)
__device__ __forceinline__ int block_exclusive_scan(int v, int *total)
{
    __shared__ int wave_sums[kScanBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int wv = 0; wv < kScanBlock / 64; ++wv) {
        if (wv < wave) base += wave_sums[wv];
        tot += wave_sums[wv];
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// ---- the tile.  Workgroup b covers items [b * kScanTile, (b + 1) * kScanTile), a lane kScanItems consecutive ones from
// `base` on: v[i] = value_of(base + i) -- the counts in memory, or a value worked out on the spot (the lane work list) --
// and their sum.
struct ScanTile {
    i64 base;
    int v[kScanItems];
    int sum;
};

template <typename F>
__device__ __forceinline__ ScanTile scan_tile_load(F value_of)
{
    ScanTile t;
    t.base = (i64)blockIdx.x * kScanTile + (i64)threadIdx.x * kScanItems;
    t.sum = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        t.v[i] = value_of(t.base + i);
        t.sum += t.v[i];
    }
    return t;
}

// the tile's sum to tile_sums[blockIdx.x]
__device__ __forceinline__ void scan_tile_sum_store(int sum, int *__restrict__ tile_sums)
{
    int total;
    (void)block_exclusive_scan(sum, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// First kernel of the scan: per-tile sums.  hook(v) sees the kScanItems counts every lane has read anyway (every lane of
// the workgroup calls it; it may synchronise): the kNN build accumulates its grid statistic there, in no kernel of its own.
struct ScanNoHook {
    __device__ __forceinline__ void operator()(const int (&)[kScanItems]) const {}
};

template <typename Hook>
__global__ __launch_bounds__(kScanBlock) void scan_tile_sums_kernel(const int *__restrict__ counts, i64 n,
                                                                    int *__restrict__ tile_sums, Hook hook)
{
    const ScanTile t = scan_tile_load([=](i64 i) { return i < n ? counts[i] : 0; });
    hook(t.v);
    scan_tile_sum_store(t.sum, tile_sums);
}

// ---- host side (mm_scan.hip).  mirror (nullable src): n 64-bit words copied on the way from device memory to the
// context's PINNED host mirror by the first kernel behind the tile sums -- the statistic a hook has accumulated (a copy
// command of the runtime's costs a dispatch of 4 us behind a 6 us gap).
struct ScanMirror {
    const long long *src = nullptr;
    long long *dst = nullptr;
    int n = 0;
};
// The scan behind scan_tile_sums_kernel (tile_sums: the RAW sums), one or two dispatches.
void mm_scan_launch_tail(mm_context *ctx, const int *counts, i64 n, int *tile_sums, int *start, const ScanMirror &mirror);
// The single-workgroup kernel alone: tile_sums[0 .. ntiles) -> their exclusive offsets, in place; with_total: the grand
// total behind them, tile_sums[ntiles] (mm_scan_scratch_ints(n, true) ints).
void mm_scan_launch_tile_offsets(mm_context *ctx, int *tile_sums, int ntiles, bool with_total,
                                 const ScanMirror &mirror = ScanMirror());

// The whole scan on ctx->stream: start[0 .. n] (start[n] = the total); tile_sums: mm_scan_scratch_ints(n) ints.
template <typename Hook>
void mm_scan_launch(mm_context *ctx, const int *counts, i64 n, int *start, int *tile_sums, Hook hook,
                    const ScanMirror &mirror = ScanMirror())
{
    hipLaunchKernelGGL(scan_tile_sums_kernel<Hook>, dim3(mm_scan_tiles(n)), dim3(kScanBlock), 0, ctx->stream, counts, n,
                       tile_sums, hook);
    mm_scan_launch_tail(ctx, counts, n, tile_sums, start, mirror);
}
