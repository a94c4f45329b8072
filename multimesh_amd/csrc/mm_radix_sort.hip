// The stable LSD radix sort of 64-bit keys with 32-bit values, mm_radix_sort_pairs: 8 bits a pass (radix_hist_kernel ->
// exclusive scan of the [digit][tile] counts, mm_scan.hip -> radix_scatter_kernel); a workgroup ranks its tile of 4096
// keys in order -- per wave and batch of 64 keys: the lanes with the same digit by eight ballots, their rank by a
// popcount, the wave's running offsets of the 256 digits in LDS -- so the scatter is stable.  Users: mm_unique (the sort
// by x, the per-component sorts of structured clouds and of long runs), mm_transpose (contributions by destination, the
// key's low bits only), the kNN tree of mm_knn.hip (Morton keys of sources and targets).
#include "mm_common.h"

namespace {

constexpr int kWave = 64;
constexpr int kBins = 256;            // 8 bits a pass
constexpr int kSortWaves = 4;
constexpr int kSortBlock = kSortWaves * kWave;
constexpr int kItems = 16;            // keys per thread: batches of 64 consecutive keys per wave
constexpr int kTile = kSortBlock * kItems;

typedef unsigned long long u64;

// counts[digit * ntiles + tile]: in that order the exclusive scan is the output offset of the tile's first
// key with that digit
__global__ __launch_bounds__(kSortBlock) void radix_hist_kernel(const u64 *__restrict__ key, i64 n, int shift, int ntiles,
                                                                int *__restrict__ counts)
{
    __shared__ int s_hist[kBins];
    for (int t = threadIdx.x; t < kBins; t += kSortBlock) s_hist[t] = 0;
    __syncthreads();
    const i64 base = (i64)blockIdx.x * kTile;
#pragma unroll 4
    for (int b = 0; b < kItems; ++b) {
        const i64 j = base + (i64)b * kSortBlock + threadIdx.x;   // (any order: this is only a count)
        if (j < n) atomicAdd(&s_hist[(int)((key[j] >> shift) & (kBins - 1))], 1);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kBins; t += kSortBlock) counts[(i64)t * ntiles + blockIdx.x] = s_hist[t];
}

__global__ __launch_bounds__(kSortBlock) void radix_scatter_kernel(const u64 *__restrict__ key_in,
                                                                   const unsigned *__restrict__ val_in, i64 n, int shift,
                                                                   int ntiles, const int *__restrict__ offsets,
                                                                   u64 *__restrict__ key_out,
                                                                   unsigned *__restrict__ val_out)
{
    // The tile is first put in digit order in LDS (stable), then written out: consecutive threads write
    // consecutive addresses inside a digit's run (~16 keys = 128 bytes at 256 digits per 4096 keys) -- scattering
    // straight from registers costs a cache line per 8-byte key in the passes over the mantissa's random bits.
    __shared__ u64 s_key[kTile];
    __shared__ unsigned s_val[kTile];
    __shared__ int s_off[kSortWaves][kBins];   // first the waves' digit counts, then their running positions in the tile
    __shared__ int s_start[kBins];             // where a digit's run starts in the sorted tile
    __shared__ int s_gbase[kBins];             // ... and in the output
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    for (int t = threadIdx.x; t < kSortWaves * kBins; t += kSortBlock) (&s_off[0][0])[t] = 0;
    __syncthreads();
    // wave w owns keys [w * kItems * kWave, (w + 1) * kItems * kWave) of the tile, batch b = 64 consecutive keys: batch
    // order, then lane order, is the input order
    const i64 tbase = (i64)blockIdx.x * kTile;
    const i64 wbase = tbase + (i64)wave * (kItems * kWave);
    u64 k[kItems];
    unsigned v[kItems];
#pragma unroll
    for (int b = 0; b < kItems; ++b) {
        const i64 j = wbase + b * kWave + lane;
        k[b] = j < n ? key_in[j] : 0;
        v[b] = j < n ? val_in[j] : 0;
        if (j < n) atomicAdd(&s_off[wave][(int)((k[b] >> shift) & (kBins - 1))], 1);
    }
    __syncthreads();
    // digit t (one thread each): its count in the tile; exclusive prefix over the digits by the first wave
    int total = 0;
    if (threadIdx.x < kBins) {
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) total += s_off[w][threadIdx.x];
        s_start[threadIdx.x] = total;
        s_gbase[threadIdx.x] = offsets[(i64)threadIdx.x * ntiles + blockIdx.x];
    }
    __syncthreads();
    if (wave == 0) {
        // 256 counts, four per lane
        int c[4], sum = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            c[q] = s_start[4 * lane + q];
            sum += c[q];
        }
        int incl = sum;
        for (int dlt = 1; dlt < kWave; dlt <<= 1) {
            const int t = __shfl_up(incl, dlt);
            if (lane >= dlt) incl += t;
        }
        int run = incl - sum;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s_start[4 * lane + q] = run;
            run += c[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < kBins) {
        int run = s_start[threadIdx.x];
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) {
            const int c = s_off[w][threadIdx.x];
            s_off[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
    const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int b = 0; b < kItems; ++b) {
        const i64 j = wbase + b * kWave + lane;
        const bool active = j < n;
        const int d = (int)((k[b] >> shift) & (kBins - 1));
        // the lanes of this batch that hold the same digit
        u64 same = __ballot(active);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const u64 vote = __ballot((d >> bit) & 1);
            same &= ((d >> bit) & 1) ? vote : ~vote;
        }
        const int rank = __popcll(same & lt);
        const int off = active ? s_off[wave][d] : 0;   // (read by every lane of the group before its head moves it on)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (active && rank == 0) s_off[wave][d] = off + __popcll(same);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (active) {
            s_key[off + rank] = k[b];
            s_val[off + rank] = v[b];
        }
    }
    __syncthreads();
    const int valid = (int)(n - tbase < kTile ? n - tbase : kTile);
#pragma unroll 4
    for (int t = threadIdx.x; t < valid; t += kSortBlock) {
        const u64 key = s_key[t];
        const int d = (int)((key >> shift) & (kBins - 1));
        const i64 pos = (i64)s_gbase[d] + (t - s_start[d]);
        key_out[pos] = key;
        val_out[pos] = s_val[t];
    }
}

}  // namespace

// counts and offsets of ncounts + 1 ints each, then the scan's tile sums
size_t mm_radix_sort_scratch(i64 n)
{
    const i64 ncounts = (i64)kBins * ((n + kTile - 1) / kTile);
    return 2 * mm_round256((size_t)(ncounts + 1) * sizeof(int)) + mm_round256(mm_scan_scratch_ints(ncounts) * sizeof(int));
}

int mm_radix_sort_pairs(mm_context *ctx, unsigned long long *ka, unsigned long long *kb, unsigned *va, unsigned *vb, i64 n,
                        int first_shift, int end_shift, void *scratch, bool *in_a)
{
    *in_a = true;
    if (n <= 0) return MM_OK;
    const int tiles = (int)((n + kTile - 1) / kTile);
    const i64 ncounts = (i64)kBins * tiles;
    char *sp = (char *)scratch;
    int *counts = (int *)sp;
    sp += mm_round256((size_t)(ncounts + 1) * sizeof(int));
    int *offsets = (int *)sp;
    sp += mm_round256((size_t)(ncounts + 1) * sizeof(int));
    int *count_sums = (int *)sp;
    for (int shift = first_shift; shift < end_shift; shift += 8) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)tiles), dim3(kSortBlock), 0, ctx->stream, ka, n, shift, tiles, counts);
        const int src = mm_exclusive_scan_int(ctx, counts, ncounts, offsets, count_sums);
        if (src != MM_OK) return src;
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)tiles), dim3(kSortBlock), 0, ctx->stream, ka, va, n, shift, tiles,
                           offsets, kb, vb);
        u64 *tk = ka;
        ka = kb;
        kb = tk;
        unsigned *tv = va;
        va = vb;
        vb = tv;
        *in_a = !*in_a;
    }
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
