// The exclusive scan of int counts, mm_exclusive_scan_int: tile sums (mm_scan.h) -> the tiles' offsets -> the running
// sums.  Users: the counting sorts of mm_knn.hip (cells of sources and targets, the tree's work items, the lane work
// list's offsets), the radix sort's [digit][tile] counts (mm_radix_sort.hip), the head flags of mm_unique and
// mm_unique_hash, the face and cell compactions of mm_boundary, the GLL locate's visiting order (mm_locate_gll.hip).
// With few tiles every workgroup of the last kernel adds up the sums of the tiles before its own by itself (at most
// kScanSelfTiles values, L2-resident) and the single-workgroup kernel in between -- a dispatch of 5 us, thirty times per
// mm_unique_points -- is not launched; with many tiles the three-kernel form.
#include "mm_scan.h"

namespace {

// single block: running exclusive scan over the tile sums
__global__ __launch_bounds__(kScanBlock) void scan_tile_offsets_kernel(int *__restrict__ tile_sums, int ntiles, bool with_total,
                                                                       ScanMirror m)
{
    if (m.src && (int)threadIdx.x < m.n) m.dst[threadIdx.x] = m.src[threadIdx.x];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < ntiles; base += kScanBlock) {
        const int i = base + threadIdx.x;
        const int v = i < ntiles ? tile_sums[i] : 0;
        int total;
        const int excl = block_exclusive_scan(v, &total);
        const int c = carry;
        if (i < ntiles) tile_sums[i] = c + excl;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + total;
        __syncthreads();
    }
    if (with_total && threadIdx.x == 0) tile_sums[ntiles] = carry;
}

// the tile's running sums from tile_base on; start[n] = the total number of items, from the last lane of the last block
__device__ __forceinline__ void scan_apply_tile(const int *__restrict__ counts, i64 n, int tile_base, int *__restrict__ start)
{
    const ScanTile t = scan_tile_load([=](i64 i) { return i < n ? counts[i] : 0; });
    int total;
    int excl = block_exclusive_scan(t.sum, &total) + tile_base;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        if (t.base + i < n) start[t.base + i] = excl;
        excl += t.v[i];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kScanBlock - 1) start[n] = excl;
}

// few tiles, straight behind scan_tile_sums_kernel: the workgroup sums the tiles before its own itself (tile_sums are
// the RAW sums here)
__global__ __launch_bounds__(kScanBlock) void scan_apply_self_kernel(const int *__restrict__ counts, i64 n,
                                                                     const int *__restrict__ tile_sums, int *__restrict__ start,
                                                                     ScanMirror m)
{
    if (m.src && blockIdx.x == 0 && (int)threadIdx.x < m.n) m.dst[threadIdx.x] = m.src[threadIdx.x];
    int before = 0;
    for (int t = threadIdx.x; t < (int)blockIdx.x; t += kScanBlock) before += tile_sums[t];
    int tile_base;
    (void)block_exclusive_scan(before, &tile_base);
    scan_apply_tile(counts, n, tile_base, start);
}

__global__ __launch_bounds__(kScanBlock) void scan_apply_kernel(const int *__restrict__ counts, i64 n,
                                                                const int *__restrict__ tile_offsets, int *__restrict__ start)
{
    scan_apply_tile(counts, n, tile_offsets[blockIdx.x], start);
}

}  // namespace

size_t mm_scan_scratch_ints(i64 n, bool with_total) { return (size_t)mm_scan_tiles(n) + (with_total ? 1 : 0); }

void mm_scan_launch_tile_offsets(mm_context *ctx, int *tile_sums, int ntiles, bool with_total, const ScanMirror &mirror)
{
    hipLaunchKernelGGL(scan_tile_offsets_kernel, dim3(1), dim3(kScanBlock), 0, ctx->stream, tile_sums, ntiles, with_total,
                       mirror);
}

void mm_scan_launch_tail(mm_context *ctx, const int *counts, i64 n, int *tile_sums, int *start, const ScanMirror &mirror)
{
    const int ntiles = mm_scan_tiles(n);
    if (ntiles <= kScanSelfTiles) {
        hipLaunchKernelGGL(scan_apply_self_kernel, dim3(ntiles), dim3(kScanBlock), 0, ctx->stream, counts, n,
                           (const int *)tile_sums, start, mirror);
    } else {
        mm_scan_launch_tile_offsets(ctx, tile_sums, ntiles, false, mirror);
        hipLaunchKernelGGL(scan_apply_kernel, dim3(ntiles), dim3(kScanBlock), 0, ctx->stream, counts, n, (const int *)tile_sums,
                           start);
    }
}

int mm_exclusive_scan_int(mm_context *ctx, const int *counts, i64 n, int *start, int *tile_sums)
{
    mm_scan_launch(ctx, counts, n, start, tile_sums, ScanNoHook());
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
