// The search grid's cell arithmetic, the rank-handing histogram atomic and the 32-byte sorted record: what every kernel
// that places a point into the grid must share to the bit -- the counting sorts of mm_knn.hip (mm_knn_grid.inc.h) and
// the one-pass centroid kernel of mm_centroid.hip; the GLL locate's visiting order (mm_locate_gll.hip) takes the
// histogram atomic for its own bins.  Device code only; nothing here may be re-derived elsewhere.
#pragma once

#include "mm_common.h"

struct GridParams {
    int nx, ny, nz;
    double lox, loy, loz;
    double hx, hy, hz;
    double ihx, ihy, ihz;
};

// ---- cell assignment ----------------------------------------------------------------
__device__ __forceinline__ int cell_coord(double x, double lo, double ih, int n)
{
    double t = (x - lo) * ih;
    t = fmin(fmax(t, 0.0), (double)(n - 1));  // NaN -> 0, outside -> clamped
    return (int)t;
}

// The histogram atomic also hands out the item's rank inside its cell, so the scatter pass needs
// no second atomic.  Mesh-ordered points arrive in runs of equal cells (neighbours along the
// fastest axis), and same-address atomics serialise in L2: the first lane of each run of equal
// cells inside the wave adds the run's length, the others take consecutive ranks behind it.
// (Random-order input: every run has length 1, nothing lost but a dozen instructions.)
// Called by every lane of the wave (c = -1, live = false for lanes without an item).
__device__ __forceinline__ int count_and_rank(int c, bool live, int *__restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(c, 1);
    const bool head = lane == 0 || c != prev;
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = heads & (~0ull >> (63 - lane));       // heads at lanes <= mine
    const int head_lane = 63 - __clzll((long long)upto);
    const unsigned long long after = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    int base = 0;
    if (head && live) {
        const int next_head = after ? __ffsll((long long)after) - 1 : 64;
        base = atomicAdd(&counts[c], next_head - lane);
    }
    base = __shfl(base, head_lane);
    return base + (lane - head_lane);
}

// the cell of a point (the count and the scatter pass of a counting sort both call this: same arithmetic, same cell)
__device__ __forceinline__ int cell_of_point(double x, double y, double z, const GridParams &g)
{
    const int cx = cell_coord(x, g.lox, g.ihx, g.nx);
    const int cy = cell_coord(y, g.loy, g.ihy, g.ny);
    const int cz = cell_coord(z, g.loz, g.ihz, g.nz);
    return (cx * g.ny + cy) * g.nz + cz;
}

// Sorted records are 32 bytes {x, y, z, original index (as the bits of a double)}: an item is
// written with two 16-byte stores into its own aligned sector and read back the same way.
constexpr int kRec = 4;

__device__ __forceinline__ void store_record(double *__restrict__ rec, double x, double y, double z, int id)
{
    double2 *r2 = reinterpret_cast<double2 *>(rec);
    r2[0] = make_double2(x, y);
    r2[1] = make_double2(z, __longlong_as_double((long long)id));
}

__device__ __forceinline__ int record_id(double w) { return (int)__double_as_longlong(w); }
// the same id read from the record in memory, as ONE dword: the low word of the fourth double
__device__ __forceinline__ int record_id_at(const double *__restrict__ rec) { return *reinterpret_cast<const int *>(rec + 3); }

// hex8 centroids sorted into the cells of grid g in ONE pass (mm_centroid.hip; mm_knn_build_one_pass calls it): record of
// element e at guess_start[cell] + rank from the zeroed per-cell cursor, per-workgroup boxes of the centroids in partial.
int mm_launch_centroid_sort(mm_context *ctx, i64 nelem, const i64 *conn, const double *points, const GridParams &g,
                            const int *guess_start, int *cursor, double *sorted_rec, double *partial, int nblocks);
