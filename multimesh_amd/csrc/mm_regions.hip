// Regions: for every node, whether it lies inside a region drawn on the sphere as great-circle edges, and its chord distance to
// the outline up to a cutoff (include/multimesh_regions.h, which holds the statement; tests/regions_cases.py is its NumPy form).
//
//   mm_region_distance : region_caps_kernel checks the edge table and the anchor and gives every chunk of kEdgeChunk consecutive
//                        edges a bounding ball and the signs of ta; region_kernel evaluates the statement for the chunks no
//                        cull excludes; region_info_kernel hands the two counts to the caller's array.
//
// Bit parity with the statement: every product, quotient and sum is rounded on its own (-ffp-contract=off); q is a minimum and
// ncross a sum of the edges, so neither depends on their order or on which edges are left out, as long as a left-out edge has a
// false crossing test and a false qe < q IN THE STATEMENT'S OWN ROUNDINGS.  No float atomics; the counts are integer sums, one atomic per
// workgroup and count.
//
// Shape.  A workgroup takes a tile of 256 / P whole groups (gll::RunTile, as mm_point_taper): the coordinates go to LDS
// coalesced a step ahead, a lane normalises its node to p and forms m = p x a, the lanes join their p into the tile's ball
// (T, Rt).  The chunks pass by in batches of 256: lane j holds the record of chunk j of the batch and tests it against the
// tile's ball; the survivors are compacted into LDS in ascending order (a ballot per wave, the waves' counts through LDS).
// Every lane tests a surviving chunk against its own p and q; a wave evaluates the chunk's edges when any of its lanes asks,
// the crossing part and the distance part each only if asked for.  The chunk index is then the same in every lane of the wave
// (readfirstlane), so the edge rows are read through the scalar cache into scalar registers: no LDS traffic and no barrier in
// the edge loop, which is why the rows are not staged in LDS.  The signs of ta = dot(N, a) do not depend on the node: the caps
// kernel evaluates the statement's expression once per edge and stores a bit.
//
// THE CULLS ("Regions", derives them).  An edge's arc lies in the ball about M = (U + V) / 2 of radius
// |U - V| / 2; a chunk's ball (C, Rc) holds the balls of its edges, with Rc rounded up by kSlack and kDelta.
//   crossing: the test needs (su >= 0) != (sv >= 0).  With mc = dot(m, C) and mn = |m| in the statement's arithmetic,
//             |mc| > (mn * Rc) * kSlack + kDelta puts the whole ball on one side of the plane of m by more than the rounding of
//             su and sv (at most 2^-50 for vectors of norm 1): both have the sign of mc, the test is false.  kDelta = 2^-45.
//   distance: the computed qe is at least D^2 - 2^-27, D the true chord from p to the arc, as long as qe < 1 (kMarginQ = 2^-20
//             leaves room), and D >= |p - C| - Rc.  |p - C|^2 > ((Rc + sqrt(q + kMarginQ)) * kSlack)^2 therefore gives
//             qe >= q.  Beyond q + kMarginQ > 1 (a cutoff past 60 degrees) the bound on qe fails near the pole of an edge:
//             the distance cull is then off.
//   the tile's versions bound the same quantities for every p within Rt of T (triangle inequality), with cutoff^2 for q.
// kSlack = 1 + 2^-40 covers the roundings of the few operations of each test itself (2^-50 relative).
#include "mm_gll_tile.h"

#include <math.h>

#include "multimesh_regions.h"

namespace {

using namespace mm_stream;   // kThreads, kWave, kMaxBlocks
constexpr int kWaves = kThreads / kWave;
constexpr int kBatch = kThreads;                  // chunks per batch: one per lane
constexpr int kEdgeChunk = MM_REGION_EDGE_CHUNK;  // edges per chunk: the bits of one unsigned
constexpr int kCapWords = 8;                      // C0 C1 C2 Rc n0 n1 n2 |n|, n = a x C
constexpr int kSlot = 16;                         // d_counters: [0] inside, [1] hit, [2] invalid, [3] bad edges or anchor
constexpr double kSlack = 1.0 + 0x1p-40;
constexpr double kDelta = 0x1p-45;
constexpr double kMarginQ = 0x1p-20;
constexpr double kUnitTol = 0x1p-48;
constexpr double kMinChord2 = 0x1p-40;
constexpr double kMinRadius = 0x1p-500;   // below it the squares of the coordinates leave the normal range and p is no unit vector
typedef unsigned long long u64;

__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2)
{
    return (x0 * y0 + x1 * y1) + x2 * y2;
}

// One lane per chunk: the checks of the header, the chunk's ball, n = a x C and the bits of ta >= 0.  Lane 0 checks the anchor.
__global__ __launch_bounds__(kThreads) void region_caps_kernel(const double *__restrict__ edges, int E, int nchunks,
                                                               const double *__restrict__ anchor, double *__restrict__ caps,
                                                               unsigned *__restrict__ tabits, u64 *bad)
{
    unsigned mine = 0;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const double a0 = anchor[0], a1 = anchor[1], a2 = anchor[2];
    if (k == 0 && !(fabs(dot3(a0, a1, a2, a0, a1, a2) - 1.0) <= kUnitTol)) ++mine;   // (false for a NaN or an inf)
    if (k < nchunks) {
        const int e0 = k * kEdgeChunk, ne = E - e0 < kEdgeChunk ? E - e0 : kEdgeChunk;
        const double inf = __builtin_inf();
        double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
        unsigned bits = 0;
        for (int e = 0; e < ne; ++e) {
            const double *row = edges + 9 * (size_t)(e0 + e);
            const double U0 = row[0], U1 = row[1], U2 = row[2], V0 = row[3], V1 = row[4], V2 = row[5];
            const double N0 = row[6], N1 = row[7], N2 = row[8];
            const double c0 = U1 * V2 - U2 * V1, c1 = U2 * V0 - U0 * V2, c2 = U0 * V1 - U1 * V0;
            const double n = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
            const double d0 = U0 - V0, d1 = U1 - V1, d2 = U2 - V2, s0 = U0 + V0, s1 = U1 + V1, s2 = U2 + V2;
            const bool ok = fabs(dot3(U0, U1, U2, U0, U1, U2) - 1.0) <= kUnitTol && fabs(dot3(V0, V1, V2, V0, V1, V2) - 1.0) <= kUnitTol &&
                            dot3(d0, d1, d2, d0, d1, d2) >= kMinChord2 && dot3(s0, s1, s2, s0, s1, s2) >= kMinChord2 &&
                            N0 == c0 / n && N1 == c1 / n && N2 == c2 / n;
            if (!ok) ++mine;
            lo[0] = fmin(lo[0], fmin(U0, V0)), hi[0] = fmax(hi[0], fmax(U0, V0));
            lo[1] = fmin(lo[1], fmin(U1, V1)), hi[1] = fmax(hi[1], fmax(U1, V1));
            lo[2] = fmin(lo[2], fmin(U2, V2)), hi[2] = fmax(hi[2], fmax(U2, V2));
            if (dot3(N0, N1, N2, a0, a1, a2) >= 0.0) bits |= 1u << e;
        }
        const double C0 = 0.5 * (lo[0] + hi[0]), C1 = 0.5 * (lo[1] + hi[1]), C2 = 0.5 * (lo[2] + hi[2]);
        double Rc = 0.0;
        for (int e = 0; e < ne; ++e) {
            const double *row = edges + 9 * (size_t)(e0 + e);
            const double U0 = row[0], U1 = row[1], U2 = row[2], V0 = row[3], V1 = row[4], V2 = row[5];
            const double dm = mm_norm3(0.5 * (U0 + V0) - C0, 0.5 * (U1 + V1) - C1, 0.5 * (U2 + V2) - C2);
            Rc = fmax(Rc, dm + 0.5 * mm_norm3(U0 - V0, U1 - V1, U2 - V2));
        }
        const double n0 = a1 * C2 - a2 * C1, n1 = a2 * C0 - a0 * C2, n2 = a0 * C1 - a1 * C0;
        double *cap = caps + (size_t)kCapWords * k;
        cap[0] = C0, cap[1] = C1, cap[2] = C2, cap[3] = Rc * kSlack + kDelta;
        cap[4] = n0, cap[5] = n1, cap[6] = n2, cap[7] = mm_norm3(n0, n1, n2);
        tabits[k] = bits;
    }
    mm_count_to(bad, mine);
}

struct RegionArgs {
    const double *points;
    i64 ngroups;
    int P, E, nchunks, anchor_inside;
    double cutoff, scale;
    double *sout;
    int *iout;
    u64 *counters;   // [0] inside, [1] hit, [2] invalid, [3] bad (read)
};

__device__ __forceinline__ double wave_min(double v)
{
    for (int off = kWave / 2; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int off = kWave / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

__global__ __launch_bounds__(kThreads) void region_kernel(const RegionArgs args, const double *__restrict__ edges,
                                                          const double *__restrict__ caps, const unsigned *__restrict__ tabits,
                                                          const double *__restrict__ anchor)
{
    __shared__ double xs[3 * kThreads];      // the tile's coordinates, [node][3] as in memory
    __shared__ double s_wred[7][kWaves];     // lo0 hi0 lo1 hi1 lo2 hi2 of p per wave, then the radius
    __shared__ double s_cap[4][kBatch];      // C0 C1 C2 Rc of the batch's chunks that survive the tile's test
    __shared__ int s_idx[kBatch];            // ... and their indices
    __shared__ int s_wcount[kWaves];
    __shared__ unsigned s_count[3][kWaves];
    if (args.counters[3] != 0) return;   // (a refused call: nothing is written)

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int E = args.E, nchunks = args.nchunks;
    const gll::RunTile T(args.ngroups, args.P);
    const double a0 = anchor[0], a1 = anchor[1], a2 = anchor[2];
    const double q0 = args.cutoff * args.cutoff;
    const bool cull_dist = q0 + kMarginQ <= 1.0;
    const double s0 = sqrt(q0 + kMarginQ);
    const double inf = __builtin_inf();
    unsigned n_inside = 0, n_hit = 0, n_invalid = 0;

    double stage[3];
    auto fetch = [&](i64 t) {
        if (t >= T.ntiles) return;
        const int nd = 3 * T.nnodes(t);
        const double *src = T.coords(args.points, t);
#pragma unroll
        for (int r = 0; r < 3; ++r) stage[r] = r * kThreads + tid < nd ? src[r * kThreads + tid] : 0.0;
    };
    fetch(blockIdx.x);
    for (i64 t = blockIdx.x; t < T.ntiles; t += gridDim.x) {
        const int nnodes = T.nnodes(t);
        __syncthreads();   // (the previous step's reads of xs and the lists are done)
#pragma unroll
        for (int r = 0; r < 3; ++r) xs[r * kThreads + tid] = stage[r];
        fetch(t + gridDim.x);
        __syncthreads();
        const bool node = tid < nnodes;
        double p0 = 0.0, p1 = 0.0, p2 = 0.0;
        bool valid = false;
        if (node) {
            const double x0 = xs[3 * tid], x1 = xs[3 * tid + 1], x2 = xs[3 * tid + 2];
            const double r = mm_norm3(x0, x1, x2);
            valid = mm_is_finite(r) && r >= kMinRadius;
            if (valid) p0 = x0 / r, p1 = x1 / r, p2 = x2 / r;
        }
        const double m0 = p1 * a2 - p2 * a1, m1 = p2 * a0 - p0 * a2, m2 = p0 * a1 - p1 * a0;
        const double mn = mm_norm3(m0, m1, m2);
        // the tile's ball: the centre of the box of the valid p, the largest |p - T|
        double b[6] = {valid ? p0 : inf, valid ? p0 : -inf, valid ? p1 : inf, valid ? p1 : -inf, valid ? p2 : inf, valid ? p2 : -inf};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            b[a] = (a & 1) ? wave_max(b[a]) : wave_min(b[a]);
            if (lane == 0) s_wred[a][wave] = b[a];
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            b[a] = s_wred[a][0];
            for (int w = 1; w < kWaves; ++w) b[a] = (a & 1) ? fmax(b[a], s_wred[a][w]) : fmin(b[a], s_wred[a][w]);
        }
        const bool anyvalid = b[0] <= b[1];
        const double T0 = 0.5 * (b[0] + b[1]), T1 = 0.5 * (b[2] + b[3]), T2 = 0.5 * (b[4] + b[5]);
        double Rt = wave_max(valid ? mm_norm3(p0 - T0, p1 - T1, p2 - T2) : 0.0);
        if (lane == 0) s_wred[6][wave] = Rt;
        __syncthreads();
        Rt = s_wred[6][0];
        for (int w = 1; w < kWaves; ++w) Rt = fmax(Rt, s_wred[6][w]);
        Rt = Rt * kSlack + kDelta;

        double q = q0, sq = s0;
        int hit = 0;
        unsigned ncross = 0;
        for (int k0 = 0; k0 < nchunks; k0 += kBatch) {
            const int nb = nchunks - k0 < kBatch ? nchunks - k0 : kBatch;
            bool keep = false;
            double C0 = 0.0, C1 = 0.0, C2 = 0.0, Rc = 0.0;
            if (tid < nb && anyvalid) {
                const double *cap = caps + (size_t)kCapWords * (k0 + tid);
                C0 = cap[0], C1 = cap[1], C2 = cap[2], Rc = cap[3];
                const double nn = cap[7];
                const double d = mm_norm3(C0 - T0, C1 - T1, C2 - T2);
                const bool far = cull_dist && d > ((Rc + Rt) + s0) * kSlack;
                const double tn = dot3(T0, T1, T2, cap[4], cap[5], cap[6]);
                const bool side = fabs(tn) > ((Rt * nn) + kSlack * Rc) * kSlack + kDelta;
                keep = !(far && side);
            }
            const u64 mask = __ballot(keep);
            __syncthreads();   // (the previous batch's reads of s_wcount, s_cap and s_idx are done)
            if (lane == 0) s_wcount[wave] = __popcll(mask);
            __syncthreads();
            int offset = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                offset += w < wave ? s_wcount[w] : 0;
                total += s_wcount[w];
            }
            if (total == 0) continue;   // (the same for every lane)
            if (keep) {
                const int pos = offset + __popcll(mask & (((u64)1 << lane) - 1));
                s_cap[0][pos] = C0, s_cap[1][pos] = C1, s_cap[2][pos] = C2, s_cap[3][pos] = Rc;
                s_idx[pos] = k0 + tid;
            }
            __syncthreads();
            for (int j = 0; j < total; ++j) {
                const double c0 = s_cap[0][j], c1 = s_cap[1][j], c2 = s_cap[2][j], rc = s_cap[3][j];
                const double mc = dot3(m0, m1, m2, c0, c1, c2);
                const double e0 = p0 - c0, e1 = p1 - c1, e2 = p2 - c2;
                const double dc2 = dot3(e0, e1, e2, e0, e1, e2);
                const double lim = (rc + sq) * kSlack;
                const bool need_c = valid && !(fabs(mc) > (mn * rc) * kSlack + kDelta);
                const bool need_d = valid && !(cull_dist && dc2 > lim * lim);
                const bool do_c = __ballot(need_c) != 0, do_d = __ballot(need_d) != 0;   // (the same in every lane of the wave)
                if (!(do_c || do_d)) continue;
                const int k = __builtin_amdgcn_readfirstlane(s_idx[j]);
                const unsigned bits = tabits[k];
                const int first = k * kEdgeChunk, ne = E - first < kEdgeChunk ? E - first : kEdgeChunk;
                for (int e = 0; e < ne; ++e) {
                    const double *row = edges + 9 * (size_t)(first + e);
                    const double U0 = row[0], U1 = row[1], U2 = row[2], V0 = row[3], V1 = row[4], V2 = row[5];
                    const double N0 = row[6], N1 = row[7], N2 = row[8];
                    if (!valid) continue;
                    const double tp = dot3(N0, N1, N2, p0, p1, p2);
                    if (do_c) {
                        const double su = dot3(m0, m1, m2, U0, U1, U2), sv = dot3(m0, m1, m2, V0, V1, V2);
                        const bool ta_pos = (bits >> e) & 1u, su_pos = su >= 0.0;
                        if (su_pos != (sv >= 0.0) && (tp >= 0.0) != ta_pos && ta_pos == su_pos) ++ncross;
                    }
                    if (do_d) {
                        const double w1 = dot3(U1 * p2 - U2 * p1, U2 * p0 - U0 * p2, U0 * p1 - U1 * p0, N0, N1, N2);
                        const double w2 = dot3(p1 * V2 - p2 * V1, p2 * V0 - p0 * V2, p0 * V1 - p1 * V0, N0, N1, N2);
                        double qe;
                        if (w1 >= 0.0 && w2 >= 0.0) {
                            const double h2 = tp * tp;
                            double g = 1.0 - h2;
                            if (g < 0.0) g = 0.0;
                            qe = (2.0 * h2) / (1.0 + sqrt(g));
                        } else {
                            const double du0 = p0 - U0, du1 = p1 - U1, du2 = p2 - U2, dv0 = p0 - V0, dv1 = p1 - V1, dv2 = p2 - V2;
                            const double du = dot3(du0, du1, du2, du0, du1, du2), dv = dot3(dv0, dv1, dv2, dv0, dv1, dv2);
                            qe = dv < du ? dv : du;
                        }
                        if (qe < q) q = qe, hit = 1;
                    }
                }
                if (do_d) sq = sqrt(q + kMarginQ);
            }
        }
        if (node) {
            const i64 at = T.first_node(t) + tid;
            const double reach = args.scale * args.cutoff;
            int inside = 0;
            double s = -reach;
            if (valid) {
                inside = args.anchor_inside ^ (int)(ncross & 1u);
                const double d = hit ? args.scale * sqrt(q) : reach;
                s = inside ? d : -d;
                n_inside += inside, n_hit += hit;
            } else {
                ++n_invalid;
            }
            if (args.sout) args.sout[at] = s;
            if (args.iout) args.iout[at] = inside;
        }
    }
    // one integer sum per workgroup and count, one atomic each
    __syncthreads();   // (the last tile's reads of s_wcount are done)
    unsigned mine[3] = {n_inside, n_hit, n_invalid};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mine[c] = wave_sum(mine[c]);
        if (lane == 0) s_count[c][wave] = mine[c];
    }
    __syncthreads();
    if (tid < 3) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) total += s_count[tid][w];
        if (total != 0) atomicAdd(args.counters + tid, (u64)total);
    }
}

__global__ void region_info_kernel(const u64 *counters, i64 *info)
{
    if (counters[3] != 0) return;
    info[0] = (i64)counters[1];
    info[1] = (i64)counters[2];
}

}  // namespace

extern "C" int64_t mm_region_distance(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P, const double *edges_d,
                                      int64_t E, const double *anchor_d, int anchor_inside, double cutoff, double scale,
                                      double *signed_out_d, int *inside_out_d, int64_t *info_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(P >= 1 && P <= kThreads, "P must lie in [1, 256]");
    MM_REQUIRE(ngroups >= 0 && ngroups < ((i64)1 << 48), "ngroups out of range");
    MM_REQUIRE(E >= 0 && E <= MM_REGION_MAX_EDGES, "E must lie in [0, 2^20]");
    MM_REQUIRE(cutoff > 0.0 && cutoff <= 2.0, "cutoff must be a chord in (0, 2]");
    MM_REQUIRE(scale > 0.0 && scale < __builtin_inf(), "scale must be positive and finite");
    MM_REQUIRE(anchor_inside == 0 || anchor_inside == 1, "anchor_inside must be 0 or 1");
    MM_REQUIRE(anchor_d != nullptr, "null anchor");
    MM_REQUIRE(E == 0 || edges_d != nullptr, "null edges");
    MM_REQUIRE(ngroups == 0 || points_d != nullptr, "null points");
    MM_REQUIRE(signed_out_d != nullptr || inside_out_d != nullptr, "both outputs are null");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    const int nchunks = (int)((E + kEdgeChunk - 1) / kEdgeChunk);
    double *caps = nullptr;
    unsigned *tabits = nullptr;
    mm_scratch_layout lay;
    lay.add(&caps, (size_t)kCapWords * nchunks);
    lay.add(&tabits, (size_t)nchunks);
    const int rc = lay.commit(ctx, __func__);
    if (rc != MM_OK) return rc;
    u64 *counters = mm_counters_begin(ctx, kSlot, 4);
    if (!counters) return MM_ERR_HIP;
    hipLaunchKernelGGL(region_caps_kernel, dim3(mm_blocks(nchunks, kThreads, (i64)1 << 30)), dim3(kThreads), 0, ctx->stream, edges_d,
                       (int)E, nchunks, anchor_d, caps, tabits, counters + 3);
    MM_HIP_CHECK(hipGetLastError());
    if (ngroups > 0) {
        RegionArgs a;
        a.points = points_d;
        a.ngroups = ngroups;
        a.P = (int)P;
        a.E = (int)E;
        a.nchunks = nchunks;
        a.anchor_inside = anchor_inside;
        a.cutoff = cutoff;
        a.scale = scale;
        a.sout = signed_out_d;
        a.iout = inside_out_d;
        a.counters = counters;
        hipLaunchKernelGGL(region_kernel, dim3(mm_blocks(ngroups, kThreads / P, kMaxBlocks)), dim3(kThreads), 0, ctx->stream, a,
                           edges_d, (const double *)caps, (const unsigned *)tabits, anchor_d);
        MM_HIP_CHECK(hipGetLastError());
    }
    if (info_d) {
        hipLaunchKernelGGL(region_info_kernel, dim3(1), dim3(1), 0, ctx->stream, (const u64 *)counters, (i64 *)info_d);
        MM_HIP_CHECK(hipGetLastError());
    }
    const i64 *count = mm_counters_end(ctx, kSlot, 4);
    if (!count) return MM_ERR_HIP;
    if (count[3] != 0) {
        mm_set_error(MM_ERR_ARG,
                     "mm_region_distance: %lld rows of the edge table (or the anchor) are not unit vectors with the stated normal, "
                     "or hold an edge shorter than 2^-20 or that close to antipodal",
                     (long long)count[3]);
        return MM_ERR_ARG;
    }
    return count[0];
}
