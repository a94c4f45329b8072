// A12 -- the TRANSPOSE of an interpolation operator: what comes back from the target side to the source side
// (a gradient on the event mesh -> the inversion mesh; P^T 1 = the coverage map).  The forward applications are
// mm_gather (node form) and mm_gather_elem (element form) in mm_gather.hip / mm_locate_gll.hip.
//
// Definition -- bit for bit np.add.at on zeros, i.e. the sequential loop:
//   node form    (ids int64[N][P], w f64[N][P]):   out[c][j] = (((+0.0 + t1) + t2) + ...), t = w[n][p] * v[n][c] rounded
//                as a product on its own (no fused multiply-add: -ffp-contract=off), over all (n, p) with ids[n][p] == j
//                in ascending flat index n * P + p.  Every row takes part (the all-zero rows of failed targets too); a
//                destination nobody names is +0.0.
//   element form (elem int64[N], coeffs f64[N][P]): out[c][e][p] = the same sequential sum of coeffs[n][p] * v[n][c] over
//                the n with elem[n] == e, ascending n; rows with elem[n] == -1 are skipped.
// No float atomics and no reordering anywhere: the result is the same on every run.
//
// How.  create groups the contributions by destination ONCE: a stable LSD radix sort (mm_radix_sort_pairs, mm_radix_sort.hip)
// of (destination, flat index), only the passes the destination count needs; stability keeps the flat indices of a
// destination ascending.  Row offsets are a bisection of the sorted keys per destination.  The node form then stores the
// weights and the target index of every contribution in destination order (8 + 4 bytes per contribution, 4 bytes per
// destination); the element form stores only the permutation of the targets (4 bytes per target) and reads the caller's
// coefficient rows through it (borrowed, like mm_source's mesh).
//
// apply, node form: every output is one dependent chain of adds.  Rows come in two bins by length:
//   * up to kLongRow (32) contributions: one LANE per destination (transpose_rows_lane_kernel) -- the lane streams its
//     weights and target indices from the sorted copy and gathers v; the mean row of a mesh-to-mesh operator is P long;
//   * longer rows (a fine target cloud inside a coarse source): one WAVE per destination (transpose_rows_wave_kernel) --
//     64 contributions per step are loaded and multiplied by the 64 lanes, coalesced, and the products are added in
//     lane order (v_readlane of lane 0, 1, ... 63), so the chain is the definition's and only the adds are serial.
// apply, element form: a group of G lanes per source element (G = 4 .. 64, the smallest power of two that holds P; two
// nodes per lane for P > 64).  Lane p owns out[c][e][p]; the group walks its targets in ascending n, G at a time: each
// lane fetches one target's index and values, then the group reads coeffs[n][.] as one coalesced row per target and
// takes v[n][c] from the lane that holds it.
//
// All components go through in one pass over the operator, four at a time (accumulators in registers).
#include <new>

#include "mm_stream.h"

// (public handle: global namespace)
struct mm_transpose {
    int device = 0;
    int elem_form = 0;
    i64 npoints = 0, P = 0, ndst = 0;   // ndst: nsrc (node form) or nelem (element form)
    i64 ncontrib = 0;                   // sorted entries: npoints * P (node form), npoints (element form)
    unsigned *offsets = nullptr;        // owned [ndst + 1]: first sorted entry of every destination
    unsigned *target = nullptr;         // owned [ncontrib]: target index of every sorted entry
    double *weights = nullptr;          // owned [ncontrib], node form: the weights in destination order
    const double *coeffs = nullptr;     // BORROWED, element form: the caller's coeffs[npoints][P]
    int *long_rows = nullptr;           // owned, node form: the destinations with more than kLongRow contributions
    i64 nlong = 0;
};

namespace {

typedef unsigned long long u64;

using namespace mm_stream;   // kThreads, kWave
constexpr int kLongRow = 32;    // node form: rows longer than this are served by a wave each
constexpr int kCompBlock = 4;   // components per pass over the operator
// the sort's tile offsets and mm_exclusive_scan_int are int, and so are the handle's row offsets
constexpr i64 kMaxContrib = 0x7fffffff;

// (no kernel here strides: the cap is the largest grid)
unsigned blocks_for(i64 n) { return mm_blocks(n, kThreads, kMaxContrib); }

// key = the destination, payload = the flat index; ids outside [lo, ndst) are counted (the key is then 0: the handle is
// never built).  minus_one_key: the key of id -1 (element form: ndst, behind every element; node form: unused)
__global__ __launch_bounds__(kThreads) void transpose_keys_kernel(const i64 *__restrict__ ids, i64 n, i64 lo, i64 ndst,
                                                                  u64 *__restrict__ key, unsigned *__restrict__ val,
                                                                  u64 *__restrict__ nbad)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const i64 id = ids[i];
        bad = id < lo || id >= ndst;
        key[i] = bad ? 0ull : (id < 0 ? (u64)ndst : (u64)id);
        val[i] = (unsigned)i;
    }
    mm_count_to(nbad, bad ? 1u : 0u);
}

// offsets[d] = the number of sorted keys below d, d in [0, ndst]
__global__ __launch_bounds__(kThreads) void transpose_offsets_kernel(const u64 *__restrict__ key, i64 n, i64 ndst,
                                                                     unsigned *__restrict__ offsets)
{
    const i64 d = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > ndst) return;
    i64 lo = 0, hi = n;   // key[lo - 1] < d <= key[hi]
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (key[mid] < (u64)d) lo = mid + 1; else hi = mid;
    }
    offsets[d] = (unsigned)lo;
}

// node form: weights and target indices in destination order (P == 1 with w == null: the element form's permutation)
__global__ __launch_bounds__(kThreads) void transpose_fill_kernel(const unsigned *__restrict__ val, i64 n, unsigned P,
                                                                  const double *__restrict__ w, double *__restrict__ weights,
                                                                  unsigned *__restrict__ target)
{
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned flat = val[j];
    if (w) weights[j] = w[flat];
    target[j] = flat / P;
}

// the destinations of the long bin, in any order (every row is summed on its own); list has room for ncontrib / (kLongRow + 1)
__global__ __launch_bounds__(kThreads) void transpose_long_rows_kernel(const unsigned *__restrict__ offsets, i64 ndst,
                                                                       int *__restrict__ list, u64 *__restrict__ count)
{
    const i64 d = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= ndst) return;
    if (offsets[d + 1] - offsets[d] > (unsigned)kLongRow) list[atomicAdd(count, 1ull)] = (int)d;
}

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// ---- node form, rows of up to kLongRow contributions: one lane per destination.  v[n * sn + c * sc]; out[c * ndst + d].
template <int CB>
__global__ __launch_bounds__(kThreads) void transpose_rows_lane_kernel(const unsigned *__restrict__ offsets,
                                                                       const double *__restrict__ weights,
                                                                       const unsigned *__restrict__ target, i64 ndst,
                                                                       const double *__restrict__ v, i64 sn, i64 sc,
                                                                       double *__restrict__ out)
{
    const i64 d = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= ndst) return;
    const unsigned b = offsets[d], e = offsets[d + 1];
    if (e - b > (unsigned)kLongRow) return;   // the wave kernel's
    double acc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = 0.0;
    for (unsigned j = b; j < e; ++j) {
        const double w = weights[j];
        const double *vp = v + (i64)target[j] * sn;
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[c] = acc[c] + w * vp[c * sc];
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) out[(i64)c * ndst + d] = acc[c];
}

// ---- node form, longer rows: one wave per destination; 64 products per step, added in lane order
template <int CB>
__global__ __launch_bounds__(kThreads) void transpose_rows_wave_kernel(const int *__restrict__ list, i64 nlong,
                                                                       const unsigned *__restrict__ offsets,
                                                                       const double *__restrict__ weights,
                                                                       const unsigned *__restrict__ target, i64 ndst,
                                                                       const double *__restrict__ v, i64 sn, i64 sc,
                                                                       double *__restrict__ out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const i64 wid = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wid >= nlong) return;   // (the whole wave)
    const i64 d = list[wid];
    const unsigned b = (unsigned)__builtin_amdgcn_readfirstlane((int)offsets[d]);
    const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)offsets[d + 1]);
    double acc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = 0.0;
    for (unsigned base = b; base < e; base += kWave) {
        const unsigned j = base + lane;
        const bool valid = j < e;
        const double w = valid ? weights[j] : 0.0;
        const double *vp = v + (i64)(valid ? target[j] : 0u) * sn;
        double prod[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) prod[c] = valid ? w * vp[c * sc] : 0.0;
        const int cnt = e - base < (unsigned)kWave ? (int)(e - base) : kWave;
        for (int i = 0; i < cnt; ++i) {
#pragma unroll
            for (int c = 0; c < CB; ++c) acc[c] = acc[c] + readlane_f64(prod[c], i);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < CB; ++c) out[(i64)c * ndst + d] = acc[c];
    }
}

// ---- element form: G lanes per source element, NH nodes per lane (p = g + 64 h).  out[(c * nelem + e) * P + p].
template <int G, int NH, int CB>
__global__ __launch_bounds__(kThreads) void transpose_elem_kernel(const unsigned *__restrict__ offsets,
                                                                  const unsigned *__restrict__ perm,
                                                                  const double *__restrict__ coeffs, i64 nelem, int P,
                                                                  const double *__restrict__ v, i64 sn, i64 sc,
                                                                  double *__restrict__ out)
{
    static_assert(NH == 1 || G == kWave, "two nodes per lane only with a whole wave per element");
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane & (G - 1), gbase = lane & ~(G - 1);
    const i64 e = ((i64)blockIdx.x * blockDim.x + threadIdx.x) / G;
    if (e >= nelem) return;   // (the whole group)
    const unsigned b = offsets[e], end = offsets[e + 1];
    double acc[NH][CB];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[h][c] = 0.0;
    for (unsigned base = b; base < end; base += G) {
        // lane g fetches target base + g of the element: its index and its values
        const unsigned j = base + g;
        const bool valid = j < end;
        const unsigned n_g = valid ? perm[j] : 0u;
        double x_g[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) x_g[c] = valid ? v[(i64)n_g * sn + c * sc] : 0.0;
        const int cnt = end - base < (unsigned)G ? (int)(end - base) : G;
        for (int i = 0; i < cnt; ++i) {
            const i64 n = (i64)(unsigned)__shfl((int)n_g, gbase + i);
            double coef[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int p = g + kWave * h;
                coef[h] = p < P ? coeffs[n * P + p] : 0.0;
            }
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                const double x = __shfl(x_g[c], gbase + i);
#pragma unroll
                for (int h = 0; h < NH; ++h) acc[h][c] = acc[h][c] + coef[h] * x;
            }
        }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int p = g + kWave * h;
        if (p < P) {
#pragma unroll
            for (int c = 0; c < CB; ++c) out[((i64)c * nelem + e) * P + p] = acc[h][c];
        }
    }
}

template <int CB>
void launch_nodes(mm_context *ctx, const mm_transpose *t, const double *v, i64 sn, i64 sc, double *out)
{
    hipLaunchKernelGGL((transpose_rows_lane_kernel<CB>), dim3(blocks_for(t->ndst)), dim3(kThreads), 0, ctx->stream, t->offsets,
                       t->weights, t->target, t->ndst, v, sn, sc, out);
    if (t->nlong > 0)
        hipLaunchKernelGGL((transpose_rows_wave_kernel<CB>), dim3(blocks_for(t->nlong * kWave)), dim3(kThreads), 0, ctx->stream,
                           t->long_rows, t->nlong, t->offsets, t->weights, t->target, t->ndst, v, sn, sc, out);
}

template <int G, int NH, int CB>
void launch_elem_g(mm_context *ctx, const mm_transpose *t, const double *v, i64 sn, i64 sc, double *out)
{
    hipLaunchKernelGGL((transpose_elem_kernel<G, NH, CB>), dim3(blocks_for(t->ndst * G)), dim3(kThreads), 0, ctx->stream,
                       t->offsets, t->target, t->coeffs, t->ndst, (int)t->P, v, sn, sc, out);
}

template <int CB>
void launch_elem(mm_context *ctx, const mm_transpose *t, const double *v, i64 sn, i64 sc, double *out)
{
    const i64 P = t->P;
    if (P <= 4) launch_elem_g<4, 1, CB>(ctx, t, v, sn, sc, out);
    else if (P <= 8) launch_elem_g<8, 1, CB>(ctx, t, v, sn, sc, out);
    else if (P <= 16) launch_elem_g<16, 1, CB>(ctx, t, v, sn, sc, out);
    else if (P <= 32) launch_elem_g<32, 1, CB>(ctx, t, v, sn, sc, out);
    else if (P <= 64) launch_elem_g<64, 1, CB>(ctx, t, v, sn, sc, out);
    else launch_elem_g<64, 2, CB>(ctx, t, v, sn, sc, out);
}

void destroy_handle(mm_transpose *t)
{
    if (!t) return;
    if (t->offsets) (void)mm_raw_free(t->offsets);
    if (t->target) (void)mm_raw_free(t->target);
    if (t->weights) (void)mm_raw_free(t->weights);
    if (t->long_rows) (void)mm_raw_free(t->long_rows);
    delete t;
}

// The grouping both forms share: n entries, destination of entry i = ids[i] in [lo, ndst) (lo = -1: such entries sort
// behind every destination).  Fills t->offsets / t->target (/ t->weights from w, entry for entry).
int build_handle(mm_context *ctx, mm_transpose *t, const i64 *ids, const double *w, i64 n, i64 lo, const char *what)
{
    const i64 ndst = t->ndst;
    const size_t n_sz = (size_t)n;
    int rc = MM_OK;
    u64 *ka = nullptr, *kb = nullptr;
    unsigned *va = nullptr, *vb = nullptr;
    void *sort_scratch = nullptr;
    u64 *counters = nullptr;   // [0] ids out of range, [1] long rows
    bool ok = mm_ctx_alloc(ctx, (void **)&t->offsets, (size_t)(ndst + 1) * sizeof(unsigned)) == hipSuccess;
    if (n > 0) {
        ok = ok && mm_ctx_alloc(ctx, (void **)&t->target, n_sz * sizeof(unsigned)) == hipSuccess;
        if (w) {
            ok = ok && mm_ctx_alloc(ctx, (void **)&t->weights, n_sz * sizeof(double)) == hipSuccess;
            ok = ok && mm_ctx_alloc(ctx, (void **)&t->long_rows, (n_sz / (kLongRow + 1) + 1) * sizeof(int)) == hipSuccess;
        }
        ok = ok && mm_ctx_alloc(ctx, (void **)&ka, n_sz * sizeof(u64)) == hipSuccess;
        ok = ok && mm_ctx_alloc(ctx, (void **)&kb, n_sz * sizeof(u64)) == hipSuccess;
        ok = ok && mm_ctx_alloc(ctx, (void **)&va, n_sz * sizeof(unsigned)) == hipSuccess;
        ok = ok && mm_ctx_alloc(ctx, (void **)&vb, n_sz * sizeof(unsigned)) == hipSuccess;
        ok = ok && mm_ctx_alloc(ctx, &sort_scratch, mm_radix_sort_scratch(n)) == hipSuccess;
    }
    if (!ok) {
        mm_set_error(MM_ERR_ALLOC, "%s: device allocation failed", what);
        rc = MM_ERR_ALLOC;
    }
    const u64 *key = ka;
    const unsigned *val = va;
    const i64 *count = nullptr;
    if (rc == MM_OK && (counters = mm_counters_begin(ctx, 2, 2)) == nullptr) rc = MM_ERR_HIP;
    if (rc == MM_OK && n > 0) {
        hipLaunchKernelGGL(transpose_keys_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, ids, n, lo, ndst, ka, va,
                           counters);
        // the passes the largest key needs (element form: ndst itself is the key of the skipped rows)
        const u64 max_key = lo < 0 ? (u64)ndst : (u64)(ndst > 0 ? ndst - 1 : 0);
        int bits = 0;
        while (bits < 64 && (max_key >> bits) != 0) ++bits;
        bool in_a = true;
        rc = mm_radix_sort_pairs(ctx, ka, kb, va, vb, n, 0, (bits + 7) / 8 * 8, sort_scratch, &in_a);
        key = in_a ? ka : kb;
        val = in_a ? va : vb;
    }
    if (rc == MM_OK) {
        hipLaunchKernelGGL(transpose_offsets_kernel, dim3(blocks_for(ndst + 1)), dim3(kThreads), 0, ctx->stream, key, n, ndst,
                           t->offsets);
        if (n > 0)
            hipLaunchKernelGGL(transpose_fill_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, val, n,
                               (unsigned)(w ? t->P : 1), w, t->weights, t->target);
        if (n > 0 && w && ndst > 0)
            hipLaunchKernelGGL(transpose_long_rows_kernel, dim3(blocks_for(ndst)), dim3(kThreads), 0, ctx->stream, t->offsets,
                               ndst, t->long_rows, counters + 1);
        if ((count = mm_counters_end(ctx, 2, 2)) == nullptr) rc = MM_ERR_HIP;
    } else {
        // (on failure too: the temporaries below must not be freed under a running kernel; mm_counters_end has synchronised)
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (rc == MM_ERR_HIP) mm_set_error(MM_ERR_HIP, "%s: a HIP call failed: %s", what, hipGetErrorString(hipGetLastError()));
    if (ka) (void)mm_raw_free(ka);
    if (kb) (void)mm_raw_free(kb);
    if (va) (void)mm_raw_free(va);
    if (vb) (void)mm_raw_free(vb);
    if (sort_scratch) (void)mm_raw_free(sort_scratch);
    if (rc != MM_OK) return rc;
    if (count[0] != 0) {
        mm_set_error(MM_ERR_ARG, "%s: %lld ids outside [%lld, %lld)", what, (long long)count[0], (long long)lo, (long long)ndst);
        return MM_ERR_ARG;
    }
    t->nlong = count[1];
    return MM_OK;
}

int create_common(mm_context *ctx, const i64 *ids, const double *w, const double *coeffs, i64 npoints, i64 P, i64 ndst,
                  int elem_form, const char *what, mm_transpose **out)
{
    mm_transpose *t = new (std::nothrow) mm_transpose();
    if (!t) {
        mm_set_error(MM_ERR_ALLOC, "out of host memory");
        return MM_ERR_ALLOC;
    }
    t->device = ctx->device;
    t->elem_form = elem_form;
    t->npoints = npoints;
    t->P = P;
    t->ndst = ndst;
    t->ncontrib = elem_form ? npoints : npoints * P;
    t->coeffs = coeffs;
    const int rc = build_handle(ctx, t, ids, w, t->ncontrib, elem_form ? -1 : 0, what);
    if (rc != MM_OK) {
        destroy_handle(t);
        return rc;
    }
    *out = t;
    return MM_OK;
}

}  // namespace

extern "C" int mm_transpose_create_nodes(mm_context *ctx, const int64_t *ids_d, const double *w_d, int64_t npoints, int64_t P,
                                         int64_t nsrc, mm_transpose **out)
{
    MM_REQUIRE(ctx != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    MM_REQUIRE(npoints >= 0 && nsrc >= 0, "negative size");
    MM_REQUIRE(P >= 1 && P <= 128, "P must be in 1..128");
    MM_REQUIRE(nsrc <= kMaxContrib, "nsrc out of range");
    if (npoints > kMaxContrib / P) {   // (sizes only: nothing has been allocated)
        mm_set_error(MM_ERR_UNSUPPORTED, "mm_transpose_create_nodes: npoints * P = %lld * %lld does not fit the sort's 31-bit offsets",
                     (long long)npoints, (long long)P);
        return MM_ERR_UNSUPPORTED;
    }
    MM_REQUIRE(npoints == 0 || (ids_d && w_d), "null array");
    MM_REQUIRE(npoints == 0 || nsrc >= 1, "ids without a destination");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    return create_common(ctx, (const i64 *)ids_d, w_d, nullptr, npoints, P, nsrc, 0, "mm_transpose_create_nodes", out);
}

extern "C" int mm_transpose_create_elem(mm_context *ctx, const int64_t *elem_d, const double *coeffs_d, int64_t npoints,
                                        int64_t P, int64_t nelem, mm_transpose **out)
{
    MM_REQUIRE(ctx != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    MM_REQUIRE(npoints >= 0 && nelem >= 0, "negative size");
    MM_REQUIRE(P >= 1 && P <= 128, "P must be in 1..128");
    MM_REQUIRE(nelem < kMaxContrib, "nelem out of range");
    if (npoints > kMaxContrib) {
        mm_set_error(MM_ERR_UNSUPPORTED, "mm_transpose_create_elem: npoints = %lld does not fit the sort's 31-bit offsets",
                     (long long)npoints);
        return MM_ERR_UNSUPPORTED;
    }
    MM_REQUIRE(npoints == 0 || (elem_d && coeffs_d), "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    return create_common(ctx, (const i64 *)elem_d, nullptr, coeffs_d, npoints, P, nelem, 1, "mm_transpose_create_elem", out);
}

extern "C" int mm_transpose_apply(mm_context *ctx, const mm_transpose *t, const double *values_d, int64_t ncomp,
                                  int values_point_major, double *out_d)
{
    MM_REQUIRE(ctx != nullptr && t != nullptr, "null argument");
    MM_REQUIRE(t->device == ctx->device, "the operator lives on another device");
    MM_REQUIRE(ncomp >= 0 && ncomp < (1 << 20), "ncomp out of range");
    if (ncomp == 0 || t->ndst == 0) return MM_OK;
    MM_REQUIRE(out_d != nullptr && (values_d != nullptr || t->npoints == 0), "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_stage_reset(ctx);
    mm_stage_begin(ctx, MM_STAGE_GATHER);
    // v[n][c] = values[n * sn + c * sc]
    const i64 sn = values_point_major ? ncomp : 1, sc = values_point_major ? 1 : t->npoints;
    const i64 out_stride = t->elem_form ? t->ndst * t->P : t->ndst;
    for (i64 c0 = 0; c0 < ncomp; c0 += kCompBlock) {
        const int cb = (int)(ncomp - c0 < kCompBlock ? ncomp - c0 : kCompBlock);
        const double *v = values_d ? values_d + c0 * sc : nullptr;
        double *o = out_d + c0 * out_stride;
#define MM_TRANSPOSE_LAUNCH(CB)                                   \
    if (t->elem_form) launch_elem<CB>(ctx, t, v, sn, sc, o);      \
    else launch_nodes<CB>(ctx, t, v, sn, sc, o)
        switch (cb) {
        case 1: MM_TRANSPOSE_LAUNCH(1); break;
        case 2: MM_TRANSPOSE_LAUNCH(2); break;
        case 3: MM_TRANSPOSE_LAUNCH(3); break;
        default: MM_TRANSPOSE_LAUNCH(4); break;
        }
#undef MM_TRANSPOSE_LAUNCH
    }
    mm_stage_end(ctx, MM_STAGE_GATHER);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" void mm_transpose_destroy(mm_context *ctx, mm_transpose *t)
{
    if (!t) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    destroy_handle(t);
}
