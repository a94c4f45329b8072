// Kernel preconditioning: the cut-out weight around sources and receivers, exact order statistics, clipping.
//
//   mm_point_taper       : w = min over the centres of a smoothstep of the distance, out = w * in; counts the nodes with w < 1
//   mm_order_statistics  : the value of a given rank among the non-NaN values, by most-significant-digit radix select
//   mm_clamp             : out = min(max(v, lo), hi) with bounds that are already on the device; counts the replaced values
//
// Bit parity with the NumPy statements (tests/precondition_cases.py): every product, quotient and sum is rounded on its own
// (-ffp-contract=off), no float atomics anywhere; the three counts are integer sums.
//
// The taper.  w is a minimum of values <= 1, so its order does not show, and a centre with d >= outer for every node of
// an element contributes exactly 1.0 to all of them: such a centre may be SKIPPED for that element.  A workgroup takes a
// tile of 256 / P whole elements (gll::RunTile of mm_gll_tile.h, as mm_radial.hip uses it): the coordinates
// go to LDS coalesced, up to eight lanes form an element's bounding box, the boxes are joined into the tile's box.  The centres
// pass by in batches of kBatch: lane j of the workgroup holds centre j of the batch in registers, tests it against the
// tile's box and, if that does not exclude it, against every element's box; the centres that hit an element are compacted
// into LDS in ascending order (a ballot per wave, the waves' counts through LDS).  Only the nodes of elements with a hit
// walk that list.  Almost every batch of almost every tile ends with an empty list.
//
// The skip test and its margin.  For a box [lo, hi] per axis and a centre c let g = max(lo - c, c - hi, 0) per axis, each
// difference rounded, and G = sqrt((g0*g0 + g1*g1) + g2*g2) in the statement's own arithmetic.  A node x of the element
// has lo <= x <= hi.  Where lo - c > 0, x - c >= lo - c > 0, and rounding is monotone: fl(x - c) >= fl(lo - c) = g.  Where
// c - hi > 0, likewise |fl(x - c)| = fl(c - x) >= fl(c - hi) = g.  Where g = 0 there is nothing to show.  So |dx| >= g >= 0
// on every axis IN THE COMPUTED values, and every later operation of the statement (a correctly rounded product of
// non-negative numbers, a sum, a square root) is monotone non-decreasing in its arguments: the computed d of the node is
// >= the computed G.  G >= outer therefore implies d >= outer, bit for bit, overflow and underflow included: the margin
// is ZERO, because the bound goes through the same roundings as the distance instead of around them.  The statement
// asks d <= inner first, so a skip also needs G > inner (d >= G > inner): with outer >= inner that adds the one case
// G == outer == inner, a hard cut whose rim passes through the box's nearest point.  (A bound through
// the real distance would need a relative margin of 4 * 2^-53 and fail where the squares underflow.)  fmin / fmax pass
// over a NaN coordinate, whose node keeps w = 1 whatever is decided; a box without any finite coordinate on an axis
// compares as a hit (g = 0 from a NaN) or as infinitely far, and both are right since every d of it is NaN.
//
// The select.  Keys: key = sign(u) ? ~u : u | 2^63 of the value's bits u (|v|: the sign bit cleared first), whose unsigned
// order is the numeric order with -0.0 before +0.0.  Eight passes over the values, one per byte of the key from the top:
// a workgroup histograms, in LDS with integer atomics, the byte of every value whose higher bytes equal the prefix of a
// wanted rank (pass 0: of every non-NaN value, which also counts them), adds its non-empty bins to the global histogram,
// and a small kernel scans it and extends every rank's prefix by the byte its rank falls in.  Ranks that share a prefix
// share a histogram (repeated q, close ranks); up to 16 prefixes are carried.  Counts are exact in any order, so the
// result is a function of the values alone.  When all candidates of a wave fall into one bin (all values equal; the top
// bytes of any smooth field) the wave adds their number once instead of serialising on one LDS address.
#include "mm_gll_tile.h"

#include <math.h>

namespace {

using namespace mm_stream;   // kThreads, kWave, kMaxBlocks
constexpr int kWaves = kThreads / kWave;
constexpr int kBatch = kThreads;    // centres per batch: one per lane (multimesh_amd.device.POINT_TAPER_BATCH)
constexpr int kSub = 8;            // lanes that share the nodes of an element for its bounding box
constexpr i64 kMaxCentres = (i64)1 << 20;
constexpr int kMaxRanks = 16;       // q per call: the prefixes a pass carries
constexpr int kBins = 256;          // one byte of the key per pass
constexpr int kPasses = 8;
constexpr int kSelectLoads = 4;     // values per lane and step of the histogram kernel
typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------- mm_point_taper
// *bad = the number of centres with a non-finite coordinate, a non-finite radius, inner < 0 or outer < inner
__global__ __launch_bounds__(kThreads) void centres_check_kernel(const double *__restrict__ centres,
                                                                 const double *__restrict__ inner,
                                                                 const double *__restrict__ outer, int K, u64 *bad)
{
    unsigned mine = 0;
    const int stride = gridDim.x * blockDim.x;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
        const double a = inner[k], b = outer[k];
        const bool ok = mm_is_finite(centres[3 * k]) && mm_is_finite(centres[3 * k + 1]) && mm_is_finite(centres[3 * k + 2]) &&
                        mm_is_finite(a) && mm_is_finite(b) && a >= 0.0 && b >= a;
        if (!ok) ++mine;
    }
    mm_count_to(bad, mine);
}

// the distance of a centre from a box in the statement's arithmetic (see the derivation above): d of a node >= this
__device__ __forceinline__ double box_distance(double lo0, double hi0, double lo1, double hi1, double lo2, double hi2,
                                               double c0, double c1, double c2)
{
    const double g0 = fmax(fmax(lo0 - c0, c0 - hi0), 0.0);
    const double g1 = fmax(fmax(lo1 - c1, c1 - hi1), 0.0);
    const double g2 = fmax(fmax(lo2 - c2, c2 - hi2), 0.0);
    return mm_norm3(g0, g1, g2);
}

struct TaperArgs {
    const double *points;
    i64 ngroups;
    int P;
    const double *centres, *inner, *outer;
    int K, ncomp;
    const double *in;   // (out may be in: no __restrict__, every lane reads its value before it writes it)
    double *out, *weight;
    const u64 *bad;
    u64 *count;
};

__global__ __launch_bounds__(kThreads) void point_taper_kernel(const TaperArgs args)
{
    __shared__ double xs[3 * kThreads];          // the tile's coordinates, [node][3] as in memory
    __shared__ double s_box[6][kThreads];        // lo0, hi0, lo1, hi1, lo2, hi2 of every element of the tile
    __shared__ double s_wbox[6][kWaves];         // ... joined per wave
    __shared__ double s_hitc[5][kBatch];         // the batch's centres that hit an element: c0, c1, c2, inner, outer
    __shared__ int s_hit[kThreads];              // element e of the tile has been hit by a centre
    __shared__ int s_wcount[kWaves];
    if (*args.bad != 0) return;   // (a refused call: nothing is written)

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int P = args.P, K = args.K, ncomp = args.ncomp;
    const gll::RunTile T(args.ngroups, P);
    const int sub = P >= kSub ? kSub : 1;     // lanes per element while the boxes are formed (tile * kSub <= 256)
    const int be = tid / sub, bs = tid - be * sub;
    const i64 n = args.ngroups * P;
    const bool copy = args.out != args.in;
    const double inf = __builtin_inf();
    unsigned mine = 0;

    // the coordinates of a tile are fetched into registers one step ahead and copied to LDS when its step comes
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
        const int nel = T.nel(t), nnodes = T.nnodes(t);
        __syncthreads();   // (the previous step's reads of xs, s_box, s_hit and the lists are done)
#pragma unroll
        for (int r = 0; r < 3; ++r) xs[r * kThreads + tid] = stage[r];
        s_hit[tid] = 0;
        fetch(t + gridDim.x);
        __syncthreads();
        // the elements' boxes: kSub lanes share an element's nodes when it has that many, then join what they found (lanes
        // without an element hold the neutral box); the boxes are joined into the tile's
        double b[6] = {inf, -inf, inf, -inf, inf, -inf};
        if (be < nel) {
            const double *X = xs + 3 * be * P;
            for (int p = bs; p < P; p += sub) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    b[2 * a] = fmin(b[2 * a], X[3 * p + a]);
                    b[2 * a + 1] = fmax(b[2 * a + 1], X[3 * p + a]);
                }
            }
        }
        if (sub > 1) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
                for (int off = 1; off < kSub; off <<= 1) {
                    const double o = __shfl_xor(b[a], off, kWave);
                    b[a] = (a & 1) ? fmax(b[a], o) : fmin(b[a], o);
                }
        }
        if (be < nel && bs == 0) {
#pragma unroll
            for (int a = 0; a < 6; ++a) s_box[a][be] = b[a];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const double o = __shfl_xor(b[a], off, kWave);
                b[a] = (a & 1) ? fmax(b[a], o) : fmin(b[a], o);
            }
            if (lane == 0) s_wbox[a][wave] = b[a];
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            b[a] = s_wbox[a][0];
            for (int w = 1; w < kWaves; ++w) b[a] = (a & 1) ? fmax(b[a], s_wbox[a][w]) : fmin(b[a], s_wbox[a][w]);
        }

        double w = 1.0;
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        if (tid < nnodes) x0 = xs[3 * tid], x1 = xs[3 * tid + 1], x2 = xs[3 * tid + 2];
        for (int k0 = 0; k0 < K; k0 += kBatch) {
            const int nb = K - k0 < kBatch ? K - k0 : kBatch;
            bool hit = false;
            double c0 = 0.0, c1 = 0.0, c2 = 0.0, ri = 0.0, ro = 0.0;
            if (tid < nb) {
                const int k = k0 + tid;
                c0 = args.centres[3 * k], c1 = args.centres[3 * k + 1], c2 = args.centres[3 * k + 2];
                ri = args.inner[k], ro = args.outer[k];
                const double gt = box_distance(b[0], b[1], b[2], b[3], b[4], b[5], c0, c1, c2);
                if (!(gt >= ro && gt > ri)) {
                    for (int e = 0; e < nel; ++e) {
                        const double ge = box_distance(s_box[0][e], s_box[1][e], s_box[2][e], s_box[3][e], s_box[4][e],
                                                       s_box[5][e], c0, c1, c2);
                        if (!(ge >= ro && ge > ri)) {
                            s_hit[e] = 1;   // (every writer writes 1; a lane still walking the previous batch's list may see it
                                            //  early and walk that list for an element it does not touch: exact all the same)
                            hit = true;
                        }
                    }
                }
            }
            const u64 mask = __ballot(hit);
            __syncthreads();   // (the previous batch's reads of s_wcount and s_hitc are done)
            if (lane == 0) s_wcount[wave] = __popcll(mask);
            __syncthreads();
            int offset = 0, total = 0;
#pragma unroll
            for (int q = 0; q < kWaves; ++q) {
                offset += q < wave ? s_wcount[q] : 0;
                total += s_wcount[q];
            }
            if (total == 0) continue;   // (the same for every lane)
            if (hit) {
                const int pos = offset + __popcll(mask & (((u64)1 << lane) - 1));
                s_hitc[0][pos] = c0, s_hitc[1][pos] = c1, s_hitc[2][pos] = c2, s_hitc[3][pos] = ri, s_hitc[4][pos] = ro;
            }
            __syncthreads();
            if (tid < nnodes && s_hit[T.el]) {
                for (int j = 0; j < total; ++j) {
                    const double dx = x0 - s_hitc[0][j], dy = x1 - s_hitc[1][j], dz = x2 - s_hitc[2][j];
                    const double in_k = s_hitc[3][j], out_k = s_hitc[4][j];
                    const double d = mm_norm3(dx, dy, dz);
                    double tk;
                    if (d <= in_k) {
                        tk = 0.0;
                    } else if (d >= out_k) {
                        tk = 1.0;
                    } else {
                        const double s = (d - in_k) / (out_k - in_k);
                        tk = (s * s) * (3.0 - 2.0 * s);
                    }
                    if (tk < w) w = tk;   // (false for a NaN)
                }
            }
        }
        __syncthreads();   // (s_hit is complete: K == 0 or a last batch without a list ends without a barrier of its own)
        if (tid < nnodes) {
            const bool touched = s_hit[T.el] != 0;
            const i64 node = T.first_node(t) + tid;
            if (w < 1.0) ++mine;
            if (args.weight) args.weight[node] = w;
            if (touched || copy) {
                for (int c = 0; c < ncomp; ++c) {
                    const double v = args.in[c * n + node];
                    args.out[c * n + node] = touched ? w * v : v;
                }
            }
        }
    }
    mm_count_to(args.count, mine);
}

// ----------------------------------------------------------------------------------------------- mm_order_statistics
struct SelectState {
    u64 prefix[kMaxRanks];     // the leading bytes of rank j's key found so far (the rest zero)
    i64 rank[kMaxRanks];       // rank j among the values that share its prefix
    int slot[kMaxRanks];       // the histogram rank j reads: the index of its prefix among the distinct ones
    u64 uprefix[kMaxRanks];    // the distinct prefixes
    int nu;                    // how many (0: no valid value)
    i64 nvalid;
};

// every candidate lane of the wave adds one to its bin of h; one add of their number when they all share a bin
__device__ __forceinline__ void vote(unsigned *h, bool candidate, int digit, int lane)
{
    const u64 m = __ballot(candidate);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    const int d0 = __shfl(digit, leader, kWave);
    const u64 same = __ballot(candidate && digit == d0);
    if (same == m) {
        if (lane == leader) atomicAdd(h + d0, (unsigned)__popcll(m));
    } else if (candidate) {
        atomicAdd(h + digit, 1u);
    }
}

// hist u64[ncomp][kMaxRanks][kBins], zero on entry; blockIdx.y = the component
template <bool FIRST>
__global__ __launch_bounds__(kThreads) void select_hist_kernel(const double *__restrict__ values, i64 n, int absolute, int pass,
                                                               const SelectState *__restrict__ state,
                                                               u64 *__restrict__ hist)
{
    __shared__ unsigned h[kMaxRanks * kBins];   // 16 KiB
    __shared__ u64 s_pre[kMaxRanks];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const i64 c = blockIdx.y;
    const int nu = FIRST ? 1 : state[c].nu;
    if (nu == 0) return;   // (no valid value in this component: the same for every lane)
    const int shift = 56 - 8 * pass;
    if (!FIRST && tid < nu) s_pre[tid] = state[c].uprefix[tid] >> (shift + 8);
    for (int q = tid; q < nu * kBins; q += kThreads) h[q] = 0;
    __syncthreads();
    const u64 *v = reinterpret_cast<const u64 *>(values) + c * n;
    const u64 sign = (u64)1 << 63;
    const i64 step = (i64)kThreads * kSelectLoads;
    for (i64 base = (i64)blockIdx.x * step; base < n; base += (i64)gridDim.x * step) {
        u64 u[kSelectLoads];
        bool ok[kSelectLoads];
#pragma unroll
        for (int r = 0; r < kSelectLoads; ++r) {
            const i64 idx = base + r * kThreads + tid;
            ok[r] = idx < n;
            u[r] = ok[r] ? v[idx] : 0;
        }
#pragma unroll
        for (int r = 0; r < kSelectLoads; ++r) {
            const u64 bits = absolute ? (u[r] & ~sign) : u[r];
            const bool valid = ok[r] && (bits & ~sign) <= 0x7ff0000000000000ull;   // (not a NaN)
            const u64 key = mm_key_of(bits);
            const int digit = (int)((key >> shift) & (kBins - 1));
            if (FIRST) {
                vote(h, valid, digit, lane);
            } else {
                const u64 hi = key >> (shift + 8);
                for (int j = 0; j < nu; ++j) vote(h + j * kBins, valid && hi == s_pre[j], digit, lane);
            }
        }
    }
    __syncthreads();
    u64 *dst = hist + c * (kMaxRanks * kBins);
    for (int q = tid; q < nu * kBins; q += kThreads)
        if (h[q]) atomicAdd(dst + q, (u64)h[q]);
}

// One block per component, lane j = rank j: extend its prefix by the byte its rank falls in; lane 0 then lists the
// distinct prefixes.  Pass 0 turns q into ranks; the last pass writes the values.
__global__ __launch_bounds__(kWave) void select_pick_kernel(const u64 *__restrict__ hist, const double *__restrict__ q, int m,
                                                            int method, int pass, SelectState *__restrict__ state,
                                                            double *__restrict__ out, i64 *__restrict__ nvalid_out)
{
    const int j = threadIdx.x;
    const i64 c = blockIdx.x;
    SelectState *st = state + c;
    const u64 *hc = hist + c * (kMaxRanks * kBins);
    const int shift = 56 - 8 * pass;
    if (pass == 0) {
        i64 nvalid = 0;
        for (int b = 0; b < kBins; ++b) nvalid += (i64)hc[b];
        if (j < m) {
            const double pos = q[j] * (double)(nvalid - 1);
            i64 r = (i64)(method == 0 ? floor(pos) : ceil(pos));
            r = r > nvalid - 1 ? nvalid - 1 : r;
            st->rank[j] = r < 0 ? 0 : r;
            st->prefix[j] = 0;
            st->slot[j] = 0;
        }
        if (j == 0) {
            st->nvalid = nvalid;
            nvalid_out[c] = nvalid;
        }
        if (nvalid == 0) {   // (the same for every lane)
            if (j == 0) st->nu = 0;
            if (j < m) out[c * m + j] = __builtin_nan("");
            return;
        }
    } else if (st->nu == 0) {
        return;
    }
    __syncthreads();   // (pass 0: the lanes' own writes above are read back below by the same lane only)
    if (j < m) {
        const u64 *row = hc + st->slot[j] * kBins;
        i64 r = st->rank[j], below = 0;
        int digit = kBins - 1;
        for (int b = 0; b < kBins; ++b) {
            const i64 cnt = (i64)row[b];
            if (r < below + cnt) {
                digit = b;
                break;
            }
            below += cnt;
        }
        const u64 prefix = st->prefix[j] | ((u64)digit << shift);
        st->rank[j] = r - below;
        st->prefix[j] = prefix;
        if (pass == kPasses - 1) out[c * m + j] = __longlong_as_double((long long)mm_bits_of_key(prefix));
    }
    __syncthreads();
    if (j == 0) {
        int nu = 0;
        for (int a = 0; a < m; ++a) {
            int s = 0;
            while (s < nu && st->uprefix[s] != st->prefix[a]) ++s;
            if (s == nu) st->uprefix[nu++] = st->prefix[a];
            st->slot[a] = s;
        }
        st->nu = nu;
    }
}

// ---------------------------------------------------------------------------------------------------------- mm_clamp
// blockIdx.y = the component; out may be in
__global__ __launch_bounds__(kThreads) void clamp_kernel(const double *in, i64 n, const double *__restrict__ lower,
                                                         const double *__restrict__ upper, int symmetric, double *out,
                                                         u64 *changed)
{
    const i64 c = blockIdx.y;
    const double inf = __builtin_inf();
    const double hi = upper ? upper[c] : inf;
    const double lo = symmetric ? -hi : (lower ? lower[c] : -inf);
    const double *src = in + c * n;
    double *dst = out + c * n;
    unsigned mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double v = src[i];
        const bool below = v < lo, above = v > hi;   // (both false for a NaN, and for -0.0 against a bound of 0.0)
        dst[i] = below ? lo : (above ? hi : v);
        if (below || above) ++mine;
    }
    if (changed) mm_count_to(changed + c, mine);
}

unsigned stream_grid(i64 n, i64 per_block) { return mm_blocks(n, per_block, kMaxBlocks); }

}  // namespace

extern "C" int64_t mm_point_taper(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P, const double *centres_d,
                                  const double *inner_d, const double *outer_d, int64_t K, int64_t ncomp, const double *in_d,
                                  double *out_d, double *weight_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(P >= 1 && P <= kThreads, "P must lie in [1, 256]");
    MM_REQUIRE(ngroups >= 0 && ngroups < ((i64)1 << 48), "ngroups out of range");
    MM_REQUIRE(K >= 0 && K <= kMaxCentres, "K must lie in [0, 2^20]");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(K == 0 || (centres_d != nullptr && inner_d != nullptr && outer_d != nullptr), "null centres or radii");
    MM_REQUIRE(ngroups == 0 || points_d != nullptr, "null points");
    MM_REQUIRE(ngroups == 0 || ncomp == 0 || (in_d != nullptr && out_d != nullptr), "null values");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    u64 *counters = mm_counters_begin(ctx, 2, 2);   // [0] nodes with w < 1, [1] bad centres
    if (!counters) return MM_ERR_HIP;
    if (K > 0)
        hipLaunchKernelGGL(centres_check_kernel, dim3(stream_grid(K, kThreads)), dim3(kThreads), 0, ctx->stream, centres_d,
                           inner_d, outer_d, (int)K, counters + 1);
    if (ngroups > 0) {
        TaperArgs a;
        a.points = points_d;
        a.ngroups = ngroups;
        a.P = (int)P;
        a.centres = centres_d;
        a.inner = inner_d;
        a.outer = outer_d;
        a.K = (int)K;
        a.ncomp = (int)ncomp;
        a.in = in_d;
        a.out = out_d;
        a.weight = weight_out_d;
        a.bad = counters + 1;
        a.count = counters;
        hipLaunchKernelGGL(point_taper_kernel, dim3(stream_grid(ngroups, kThreads / P)), dim3(kThreads), 0, ctx->stream, a);
    }
    const i64 *count = mm_counters_end(ctx, 2, 2);
    if (!count) return MM_ERR_HIP;
    if (count[1] != 0) {
        mm_set_error(MM_ERR_ARG,
                     "mm_point_taper: %lld centres are not finite or have radii that are not finite with 0 <= inner <= outer",
                     (long long)count[1]);
        return MM_ERR_ARG;
    }
    return count[0];
}

extern "C" int mm_order_statistics(mm_context *ctx, const double *values_d, int64_t n, int64_t ncomp, int absolute,
                                   const double *q_d, int64_t m, int method, double *out_d, int64_t *nvalid_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(m >= 1 && m <= kMaxRanks, "m must lie in [1, 16]");
    MM_REQUIRE(method == 0 || method == 1, "method must be 0 (lower) or 1 (higher)");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 42), "n out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(q_d != nullptr, "null q");
    MM_REQUIRE(ncomp == 0 || (out_d != nullptr && nvalid_d != nullptr), "null output");
    MM_REQUIRE(n == 0 || ncomp == 0 || values_d != nullptr, "null values");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    double q[kMaxRanks];
    MM_HIP_CHECK(hipMemcpyAsync(q, q_d, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (i64 j = 0; j < m; ++j) MM_REQUIRE(q[j] >= 0.0 && q[j] <= 1.0, "every q must lie in [0, 1]");
    if (ncomp == 0) return MM_OK;
    u64 *hist = nullptr;
    SelectState *state = nullptr;
    mm_scratch_layout lay;
    lay.add(&hist, (size_t)(ncomp * kMaxRanks * kBins));
    lay.add(&state, (size_t)ncomp);
    const int rc = lay.commit(ctx, __func__);
    if (rc != MM_OK) return rc;
    const size_t hist_bytes = (size_t)(ncomp * kMaxRanks * kBins) * sizeof(u64);
    const dim3 grid(stream_grid(n, (i64)kThreads * kSelectLoads), (unsigned)ncomp);
    for (int pass = 0; pass < kPasses; ++pass) {
        if (mm_zero_async(ctx, hist, hist_bytes) != MM_OK) return MM_ERR_HIP;
        if (n > 0) {
            if (pass == 0)
                hipLaunchKernelGGL(select_hist_kernel<true>, grid, dim3(kThreads), 0, ctx->stream, values_d, n, absolute ? 1 : 0,
                                   pass, (const SelectState *)state, hist);
            else
                hipLaunchKernelGGL(select_hist_kernel<false>, grid, dim3(kThreads), 0, ctx->stream, values_d, n,
                                   absolute ? 1 : 0, pass, (const SelectState *)state, hist);
        }
        hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)ncomp), dim3(kWave), 0, ctx->stream, (const u64 *)hist, q_d,
                           (int)m, method, pass, state, out_d, (i64 *)nvalid_d);
    }
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_clamp(mm_context *ctx, const double *in_d, int64_t n, int64_t ncomp, const double *lower_d,
                        const double *upper_d, int symmetric, double *out_d, int64_t *changed_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 48), "n out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(symmetric == 0 || symmetric == 1, "symmetric must be 0 or 1");
    MM_REQUIRE(!symmetric || (lower_d == nullptr && upper_d != nullptr), "symmetric takes upper_d alone");
    MM_REQUIRE(n == 0 || ncomp == 0 || (in_d != nullptr && out_d != nullptr), "null array");
    if (ncomp == 0) return MM_OK;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    if (changed_d && mm_zero_async(ctx, changed_d, (size_t)ncomp * sizeof(i64)) != MM_OK) return MM_ERR_HIP;
    if (n == 0) return MM_OK;
    hipLaunchKernelGGL(clamp_kernel, dim3(stream_grid(n, kThreads), (unsigned)ncomp), dim3(kThreads), 0, ctx->stream, in_d, n,
                       lower_d, upper_d, symmetric, out_d, (u64 *)changed_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
