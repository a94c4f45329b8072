// Radial 1-D profiles: the radial bin of every point, a mass-weighted sum per bin, and a 1-D table evaluated on the nodes.
//
//   mm_radial_bins          : bin[i] = upper_bound(edges, |p_i|) - 1, -1 outside the edges; counts the -1 entries
//   mm_binned_weighted_sum  : out[c][b] = sum over bin[i] == b of mass[i] * f[c][i], all bins in one pass per component
//   mm_radial_model_apply   : ref = the table's layer of the element's centre, lerped at the node's radius; five modes
//
// Bit parity with the NumPy statements (tests/radial_cases.py): |p|, the bisection and the lerp are those of mm_stream.h,
// every product, quotient and sum rounded on its own (-ffp-contract=off).
//
// The binned sum.  The definition (include/multimesh_hip.h) is mm_weighted_sum's rule applied to every bin on its own,
// with +0.0 for the values of other bins and every lane sum started from +0.0.  Such a partial sum is never -0.0
// ((+0.0) + (-0.0) = +0.0, x + (-x) = +0.0), so x + (+0.0) = x for every x it can hold: the terms of other bins are
// SKIPPED, and one pass serves all bins.  A workgroup owns a chunk of 4096 values; a lane keeps its 16 terms and bin ids
// in registers; the chunk's bin range [lo, hi] is walked in windows of kWindow bins.  A window has a table
// tab[kWindow][256] in LDS of which lane l touches only column l while it adds its terms in ascending order (no
// conflicts: consecutive lanes, consecutive doubles; no atomics), then the rows are halved across lanes, all rows of the
// window in one step per barrier.  The chunk sums go to a zero-filled dst[bin][chunk]; the levels above are dense
// (binned_level_kernel: mm_chunk_sum from +0.0).  On a layered mesh a chunk (about 33 order-4 elements) spans a few bins: one window.  A chunk of
// a shuffled cloud takes ceil(span / kWindow) windows over the same registers.
//
// The table evaluation works on tiles of 256 / P whole elements (gll::RunTile of mm_gll_tile.h): the
// coordinates go to LDS coalesced, lane e < tile forms element e's centre and finds its layer, then lane t is node t.
#include "mm_gll_tile.h"
#include "mm_radial_table.h"

#include <limits.h>

#include <vector>

namespace {

using namespace mm_stream;   // kThreads, kWave, kChunk, kTerms, kMaxBlocks
constexpr int kWindow = 8;          // bins per LDS window: 16 KiB of doubles (+ 8 KiB of counts when asked for)
constexpr int kEdgeLds = 2048;      // doubles of LDS for the edges (16 KiB)
constexpr int kTableLds = 4096;     // doubles of LDS for the table, radii and values together (32 KiB)
constexpr i64 kMaxBins = (i64)1 << 20;

unsigned grid_for(i64 n) { return mm_blocks(n, kThreads, kMaxBlocks); }

// ---------------------------------------------------------------------------------------------------- mm_radial_bins
// *bad = the number of i in [0, nbins] with a non-finite edges[i] or (i > 0) edges[i] <= edges[i - 1]
__global__ __launch_bounds__(kThreads) void edges_check_kernel(const double *__restrict__ edges, int nbins,
                                                               unsigned long long *bad)
{
    unsigned mine = 0;
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= nbins; i += stride) {
        const double e = edges[i];
        if (!(fabs(e) < __builtin_inf()) || (i > 0 && !(e > edges[i - 1]))) ++mine;
    }
    mm_count_to(bad, mine);
}

template <bool LDS_EDGES>
__global__ __launch_bounds__(kThreads) void radial_bins_kernel(const double *__restrict__ points, i64 n,
                                                               const double *__restrict__ edges, int nbins,
                                                               int *__restrict__ bin, double *__restrict__ radius,
                                                               const unsigned long long *__restrict__ bad,
                                                               unsigned long long *outside)
{
    __shared__ double s_edges[LDS_EDGES ? kEdgeLds : 1];
    if (*bad != 0) return;   // (the edges are not a valid axis: nothing is written)
    const double *e = edges;
    if (LDS_EDGES) {
        for (int q = threadIdx.x; q <= nbins; q += kThreads) s_edges[q] = edges[q];
        __syncthreads();
        e = s_edges;
    }
    const double lo = e[0], hi = e[nbins];
    unsigned mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const double x = points[3 * p], y = points[3 * p + 1], z = points[3 * p + 2];
        const double r = mm_norm3(x, y, z);
        int b = -1;
        if (r >= lo && r <= hi) {   // (false for a NaN)
            b = mm_upper_bound(e, 0, nbins + 1, r) - 1;
            b = b > nbins - 1 ? nbins - 1 : b;   // r == edges[nbins]
        } else {
            ++mine;
        }
        bin[p] = b;
        if (radius) radius[p] = r;
    }
    mm_count_to(outside, mine);
}

// -------------------------------------------------------------------------------------------- mm_binned_weighted_sum
// One block per chunk.  dst[b * stride + chunk] (zero-filled by the caller) takes the chunk's sum of every bin the chunk
// has a member of; count[b] (COUNT) the number of members.
template <bool COUNT>
__global__ __launch_bounds__(kThreads) void binned_chunk_kernel(const double *__restrict__ mass,
                                                                const double *__restrict__ f,
                                                                const int *__restrict__ bin, i64 n, int nbins,
                                                                int square, double *__restrict__ dst, i64 stride,
                                                                unsigned long long *__restrict__ count)
{
    __shared__ double tab[kWindow * kThreads];
    __shared__ int cnt[COUNT ? kWindow * kThreads : 1];
    __shared__ int s_lo[kThreads / kWave], s_hi[kThreads / kWave];

    const int tid = threadIdx.x;
    const i64 chunk = blockIdx.x;
    const i64 first = chunk * kChunk;
    double t[kTerms];
    int b[kTerms];
    int lo = INT_MAX, hi = -1;
#pragma unroll
    for (int r = 0; r < kTerms; ++r) {
        const i64 idx = first + r * kThreads + tid;
        b[r] = -1;
        t[r] = 0.0;
        if (idx < n) {
            const int q = bin[idx];
            if ((unsigned)q < (unsigned)nbins) {
                const double m = mass[idx];
                double v = m;
                if (f) {
                    const double fv = f[idx];
                    v = m * fv;
                    if (square) v = v * fv;
                }
                b[r] = q;
                t[r] = v;
                lo = q < lo ? q : lo;
                hi = q > hi ? q : hi;
            }
        }
    }
    // the chunk's bin range
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const int l2 = __shfl_xor(lo, off, kWave), h2 = __shfl_xor(hi, off, kWave);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((tid & (kWave - 1)) == 0) s_lo[tid / kWave] = lo, s_hi[tid / kWave] = hi;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) {
        lo = s_lo[w] < lo ? s_lo[w] : lo;
        hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    if (hi < 0) return;   // (no member of any bin: dst keeps its zeros; the same for every lane)

    for (int w0 = lo; w0 <= hi; w0 += kWindow) {
        const int rows = hi - w0 + 1 < kWindow ? hi - w0 + 1 : kWindow;
        // lane l owns column l of every row until the barrier: zero it, then add this lane's terms in ascending order
        for (int j = 0; j < rows; ++j) {
            tab[j * kThreads + tid] = 0.0;
            if (COUNT) cnt[j * kThreads + tid] = 0;
        }
#pragma unroll
        for (int r = 0; r < kTerms; ++r) {
            const int j = b[r] - w0;
            if ((unsigned)j < (unsigned)rows) {
                tab[j * kThreads + tid] = tab[j * kThreads + tid] + t[r];
                if (COUNT) cnt[j * kThreads + tid] += 1;
            }
        }
        __syncthreads();
        // s[l] = s[l] + s[l + h] for h = 128 ... 1, all rows of the window in one step
        for (int h = kThreads / 2, sh = 7; h >= 1; h >>= 1, --sh) {
            for (int q = tid; q < rows * h; q += kThreads) {
                const int j = q >> sh, l = q & (h - 1);
                tab[j * kThreads + l] = tab[j * kThreads + l] + tab[j * kThreads + l + h];
                if (COUNT) cnt[j * kThreads + l] += cnt[j * kThreads + l + h];
            }
            __syncthreads();
        }
        if (tid < rows) {
            dst[(i64)(w0 + tid) * stride + chunk] = tab[tid * kThreads];
            if (COUNT && cnt[tid * kThreads] != 0) atomicAdd(count + w0 + tid, (unsigned long long)cnt[tid * kThreads]);
        }
        __syncthreads();   // (row 0 of every column is read above before the next window zeroes it)
    }
}

// The levels above: src[row][count] dense, block (row, chunk) = blockIdx.x = row * nch + chunk; dst[row * nch + chunk].
__global__ __launch_bounds__(kThreads) void binned_level_kernel(const double *__restrict__ src, i64 count, i64 nch,
                                                                double *__restrict__ dst)
{
    __shared__ double s[kThreads];
    const i64 row = blockIdx.x / nch, chunk = blockIdx.x - row * nch;
    const double *a = src + row * count;
    const double sum = mm_chunk_sum<false>(s, chunk * kChunk, count, [&](i64 idx) { return a[idx]; });
    if (threadIdx.x == 0) dst[blockIdx.x] = sum;
}

// --------------------------------------------------------------------------------------------- mm_radial_model_apply
struct ApplyArgs {
    const double *points;
    i64 ngroups;
    int P;
    const double *radius, *values;   // f64[m], f64[ncomp][m]
    int m, ncomp, mode;
    const int *lstart;               // int32[nlayers + 1]: first row of every layer, then m
    int nlayers;
    const double *in;
    double *out;
};

// LDS_TABLE: radii and values are copied to (dynamic) LDS first and read there.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void radial_apply_kernel(const ApplyArgs args)
{
    extern __shared__ double s_table[];
    __shared__ double xs[3 * kThreads];
    __shared__ int s_a[kThreads], s_b[kThreads];   // the rows [a, b] of every element's layer; a = -1: a NaN centre

    const int tid = threadIdx.x, P = args.P, m = args.m, ncomp = args.ncomp;
    const double *R = args.radius, *V = args.values;
    if (LDS_TABLE) {
        for (int q = tid; q < m * (1 + ncomp); q += kThreads) s_table[q] = q < m ? args.radius[q] : args.values[q - m];
        R = s_table;
        V = s_table + m;
    }
    const gll::RunTile T(args.ngroups, P);
    const i64 n = args.ngroups * P;
    const double *in = args.in;               // (out may be in: no __restrict__, every lane reads its value before writing)
    double *out = args.out;

    for (i64 t = blockIdx.x; t < T.ntiles; t += gridDim.x) {
        const int nel = T.nel(t), nnodes = T.nnodes(t);
        const double *src = T.coords(args.points, t);
        __syncthreads();   // (the previous step's reads of xs, s_a and s_b are done; the table is in place)
        for (int q = tid; q < 3 * nnodes; q += kThreads) xs[q] = src[q];
        __syncthreads();
        if (tid < nel) {
            const double rc = mm_radial_table::centre_radius(xs + 3 * tid * P, P);
            int a = -1, b = -1;
            if (rc == rc) mm_radial_table::layer_of(R, args.lstart, args.nlayers, rc, a, b);
            s_a[tid] = a;
            s_b[tid] = b;
        }
        __syncthreads();
        if (tid < nnodes) {
            const double x = xs[3 * tid], y = xs[3 * tid + 1], z = xs[3 * tid + 2];
            const int a = s_a[T.el], b = s_b[T.el];
            const i64 node = T.first_node(t) + tid;
            int i = 0;
            double w = __builtin_nan("");
            if (a >= 0) mm_radial_table::interval_of(R, a, b, mm_norm3(x, y, z), i, w);
            for (int c = 0; c < ncomp; ++c) {
                const double *Vc = V + (i64)c * m;
                const double ref = a >= 0 ? mm_lerp(w, Vc[i], Vc[i + 1]) : w;
                double o = ref;
                if (args.mode != 0) {
                    const double v = in[c * n + node];
                    switch (args.mode) {
                    case 1: o = v - ref; break;
                    case 2: o = (v - ref) / ref; break;
                    case 3: o = v + ref; break;
                    default: o = ref + v * ref; break;
                    }
                }
                out[c * n + node] = o;
            }
        }
    }
}

}  // namespace

extern "C" int64_t mm_radial_bins(mm_context *ctx, const double *points_d, int64_t n, const double *edges_d, int64_t nbins,
                                  int32_t *bin_d, double *radius_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 58), "n out of range");
    MM_REQUIRE(nbins >= 1 && nbins <= kMaxBins, "nbins out of range");
    MM_REQUIRE(edges_d != nullptr, "null edges");
    MM_REQUIRE((points_d != nullptr && bin_d != nullptr) || n == 0, "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    unsigned long long *counters = mm_counters_begin(ctx, 2, 2);   // [0] outside, [1] bad edges
    if (!counters) return MM_ERR_HIP;
    hipLaunchKernelGGL(edges_check_kernel, dim3(grid_for(nbins + 1)), dim3(kThreads), 0, ctx->stream, edges_d, (int)nbins,
                       counters + 1);
    if (n > 0) {
        if (nbins + 1 <= kEdgeLds)
            hipLaunchKernelGGL(radial_bins_kernel<true>, dim3(grid_for(n)), dim3(kThreads), 0, ctx->stream, points_d, n,
                               edges_d, (int)nbins, (int *)bin_d, radius_out_d, counters + 1, counters);
        else
            hipLaunchKernelGGL(radial_bins_kernel<false>, dim3(grid_for(n)), dim3(kThreads), 0, ctx->stream, points_d, n,
                               edges_d, (int)nbins, (int *)bin_d, radius_out_d, counters + 1, counters);
    }
    const i64 *count = mm_counters_end(ctx, 2, 2);
    if (!count) return MM_ERR_HIP;
    if (count[1] != 0) {
        mm_set_error(MM_ERR_ARG, "mm_radial_bins: the edges are not finite and strictly ascending (%lld of them)",
                     (long long)count[1]);
        return MM_ERR_ARG;
    }
    return count[0];
}

extern "C" int mm_binned_weighted_sum(mm_context *ctx, const double *mass_d, const double *fields_d, const int32_t *bin_d,
                                      int64_t n, int64_t ncomp, int64_t nbins, int square, double *out_d, int64_t *count_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 42), "n out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(nbins >= 1 && nbins <= kMaxBins, "nbins out of range");
    MM_REQUIRE(fields_d != nullptr || ncomp <= 1, "without fields there is one sum");
    MM_REQUIRE(out_d != nullptr || ncomp == 0, "null output");
    MM_REQUIRE((mass_d != nullptr && bin_d != nullptr) || n == 0, "null array");
    mm_sum_levels levels(n);   // one row of chunk sums per bin
    const int nlevels = levels.n;
    if (nlevels > 1 && nbins * levels.chunks[1] >= ((i64)1 << 31)) {
        mm_set_error(MM_ERR_UNSUPPORTED, "mm_binned_weighted_sum: nbins * ceil(n / 4096^2) is out of range");
        return MM_ERR_UNSUPPORTED;
    }
    if (ncomp == 0 && count_d == nullptr) return MM_OK;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    if (nlevels) {
        mm_scratch_layout lay;
        levels.add_to(lay, nbins);
        const int rc = lay.commit(ctx, __func__);
        if (rc != MM_OK) return rc;
    }
    if (count_d && mm_zero_async(ctx, count_d, (size_t)nbins * sizeof(i64)) != MM_OK) return MM_ERR_HIP;
    if (ncomp > 0 && mm_zero_async(ctx, out_d, (size_t)(ncomp * nbins) * sizeof(double)) != MM_OK) return MM_ERR_HIP;
    if (n == 0) return MM_OK;
    // (ncomp == 0 with count_d: one pass for the counts alone, its sums go nowhere but the scratch -- or nowhere at all)
    const i64 passes = ncomp > 0 ? ncomp : 1;
    const i64 nchunks = levels.chunks_at(0);
    double *sink = nullptr;
    if (ncomp == 0 && nlevels == 0) {
        mm_scratch_layout lay;
        lay.add(&sink, (size_t)nbins);
        const int rc = lay.commit(ctx, __func__);
        if (rc != MM_OK) return rc;
    }
    for (i64 c = 0; c < passes; ++c) {
        double *out_c = ncomp > 0 ? out_d + c * nbins : sink;
        double *dst = nlevels ? levels.partial[0] : out_c;
        if (nlevels && mm_zero_async(ctx, dst, (size_t)(nbins * nchunks) * sizeof(double)) != MM_OK) return MM_ERR_HIP;
        const double *f = fields_d ? fields_d + c * n : nullptr;
        const i64 stride = nlevels ? nchunks : 1;
        if (count_d && c == 0)
            hipLaunchKernelGGL(binned_chunk_kernel<true>, dim3((unsigned)nchunks), dim3(kThreads), 0, ctx->stream, mass_d, f,
                               (const int *)bin_d, n, (int)nbins, square ? 1 : 0, dst, stride,
                               (unsigned long long *)count_d);
        else
            hipLaunchKernelGGL(binned_chunk_kernel<false>, dim3((unsigned)nchunks), dim3(kThreads), 0, ctx->stream, mass_d, f,
                               (const int *)bin_d, n, (int)nbins, square ? 1 : 0, dst, stride,
                               (unsigned long long *)nullptr);
        if (ncomp == 0) break;
        for (int l = 0; l < nlevels; ++l) {
            const i64 nch = levels.chunks_at(l + 1);
            double *next = l + 1 < nlevels ? levels.partial[l + 1] : out_c;
            hipLaunchKernelGGL(binned_level_kernel, dim3((unsigned)(nbins * nch)), dim3(kThreads), 0, ctx->stream,
                               (const double *)levels.partial[l], levels.chunks[l], nch, next);
        }
    }
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_radial_model_apply(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P,
                                     const double *radius_d, const double *values_d, int64_t m, int64_t ncomp, int mode,
                                     const double *in_d, double *out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(ngroups >= 0 && ngroups < ((i64)1 << 48), "ngroups out of range");
    MM_REQUIRE(P >= 1 && P <= kThreads, "P must lie in [1, 256]");
    MM_REQUIRE(m >= 2 && m < ((i64)1 << 24), "the table needs between 2 and 2^24 rows");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(mode >= 0 && mode <= 4, "mode must be 0 .. 4");
    MM_REQUIRE(radius_d != nullptr && (values_d != nullptr || ncomp == 0), "null table");
    const bool work = ngroups > 0 && ncomp > 0;
    MM_REQUIRE(!work || (points_d != nullptr && out_d != nullptr), "null array");
    MM_REQUIRE(!work || mode == 0 || in_d != nullptr, "modes 1 to 4 read in_d");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    // the table's radii, checked on the host; the layers are the maximal strictly ascending runs
    std::vector<double> R((size_t)m);
    MM_HIP_CHECK(hipMemcpyAsync(R.data(), radius_d, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    std::vector<int> lstart;
    const int table_rc = mm_radial_table_layers(__func__, R.data(), m, lstart);
    if (table_rc != MM_OK) return table_rc;
    const int nlayers = (int)lstart.size() - 1;
    if (!work) return MM_OK;
    int *lstart_d = nullptr;
    mm_scratch_layout lay;
    lay.add(&lstart_d, lstart.size());
    const int rc = lay.commit(ctx, __func__);
    if (rc != MM_OK) return rc;
    MM_HIP_CHECK(hipMemcpyAsync(lstart_d, lstart.data(), lstart.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // (lstart leaves scope with this call)
    ApplyArgs a;
    a.points = points_d;
    a.ngroups = ngroups;
    a.P = (int)P;
    a.radius = radius_d;
    a.values = values_d;
    a.m = (int)m;
    a.ncomp = (int)ncomp;
    a.mode = mode;
    a.lstart = lstart_d;
    a.nlayers = nlayers;
    a.in = in_d;
    a.out = out_d;
    const unsigned grid = mm_blocks(ngroups, kThreads / P, kMaxBlocks);
    const i64 table = m * (1 + ncomp);
    if (table <= kTableLds)
        hipLaunchKernelGGL(radial_apply_kernel<true>, dim3(grid), dim3(kThreads), (size_t)table * sizeof(double), ctx->stream,
                           a);
    else
        hipLaunchKernelGGL(radial_apply_kernel<false>, dim3(grid), dim3(kThreads), 0, ctx->stream, a);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
