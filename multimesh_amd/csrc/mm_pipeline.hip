// The fused hot path on resident arrays (mm_interpolate_hex8) and the two LEGACY host-pointer
// symbols that replace the reference's C library one for one (reference multi_mesh/helpers.py:43-81
// binds them; reference scripts/cli.py:62-100 is the call sequence the fused entry reproduces).
#include <cstdlib>
#include <mutex>
#include <new>

#include "mm_common.h"

// candidates delivered up front when the lists are evaluated lazily (99.9 % of mesh-node targets are
// resolved within them; see mm_set_lazy_lists)
static const int64_t kLazyK = 8;
// workgroups of the fused centroid + bounding-box kernel (grid-stride; one partial box each)
static const int kBoxBlocks = 2048;
// components up to which the gather is fused into the locate kernels (see mm_interpolate_hex8)
static const int64_t kFuseGatherMaxComp = 3;   // measured at 10M targets: 1: -0.5 ms, 2: -0.3 ms, 3: even

// -----------------------------------------------------------------------------------------
// Fused pipeline: centroid -> grid build -> kNN -> locate -> gather.
// Intermediates (centroids, candidate lists, and the operator when the caller does not ask for
// it) live in caller-invisible device memory owned by this call.
// -----------------------------------------------------------------------------------------
// Host arrays behind the device-pointer pipeline (mm_interpolate_hex8_host): each upload is issued on the
// context's copy stream just before the stage that needs it, so that it runs beside the kernels of the
// stage before (mesh -> centroids + grid build | targets -> kNN | fields -> locate).  Uploads from
// pageable memory block the host thread, which is why they are interleaved with the (asynchronous) launches
// here instead of being queued up front.
struct mm_host_feed {
    const void *src[4];   // nodes, connectivity, points, fields (host)
    void *dst[4];         // their device copies (context buffer cache)
    size_t bytes[4];
};

static int feed_upload(mm_context *ctx, const mm_host_feed *feed, int first, int last, int event)
{
    for (int a = first; a <= last; ++a)
        if (feed->bytes[a])
            MM_HIP_CHECK(hipMemcpyAsync(feed->dst[a], feed->src[a], feed->bytes[a], hipMemcpyHostToDevice, ctx->copy_stream));
    MM_HIP_CHECK(hipEventRecord(ctx->ev_copy[event], ctx->copy_stream));
    MM_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_copy[event], 0));
    return MM_OK;
}

// A source mesh kept resident for repeated calls (mm_source_create): the caller's node and connectivity arrays
// (borrowed: they must stay alive and unchanged) with the element centroids and the search grid over them, built once --
// what the reference does when it builds its cKDTree once and queries it for every GLL point of the element / every
// time step (scripts/cli.py:141-195).
struct mm_source {
    const double *nodes = nullptr;
    i64 nnodes = 0;
    const i64 *conn = nullptr;
    i64 nelem = 0;
    double *centroids = nullptr;   // owned
    mm_knn_index *index = nullptr; // owned (its arrays are its own, not the context's buffer cache)
    int device = 0;
};

static int64_t interpolate_hex8_impl(mm_context *ctx, const double *nodes_d, int64_t nnodes,
                                     const int64_t *conn_d, int64_t nelem, const double *points_d,
                                     int64_t npoints, const double *fields_d, int64_t ncomp, int64_t k,
                                     double *out_d, int64_t *enc_d, double *w_d, const mm_host_feed *feed,
                                     const mm_source *resident = nullptr)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(nnodes >= 1 && nelem >= 1, "empty source mesh");
    MM_REQUIRE(npoints >= 0 && ncomp >= 0, "negative size");
    MM_REQUIRE(k >= 1 && k <= MM_KNN_MAX_K, "nelem_to_search must be in 1..MM_KNN_MAX_K");
    MM_REQUIRE(nodes_d && conn_d, "null mesh array");
    MM_REQUIRE(npoints == 0 || points_d, "null target array");
    MM_REQUIRE(ncomp == 0 || out_d == nullptr || fields_d, "null field array");
    MM_REQUIRE(nelem < (int64_t)0x7fffffff, "too many elements");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_stage_reset(ctx);
    if (npoints == 0) return 0;

    // Intermediates come from the context's grow-only buffer cache: after the first call with a
    // given problem size there is no allocation, free or extra synchronisation in here.
    double *cen = nullptr, *box_partial = nullptr;
    int *nn = nullptr;  // candidate lists stay int32 inside the pipeline (half the bytes of the public int64)
    i64 *enc = (i64 *)enc_d;
    double *w = w_d;
    mm_knn_index *index = nullptr;
    int64_t result = MM_ERR_HIP;
    hipError_t e = hipSuccess;
    int rc = MM_OK;
    bool guessed = false;

#define MM_PIPE_FAIL(code, msg)                                        \
    do {                                                               \
        mm_set_error(code, "mm_interpolate_hex8: %s", msg);            \
        result = code;                                                 \
        goto done;                                                     \
    } while (0)

    // lazily evaluated candidate lists (mm_set_lazy_lists): the kNN stage delivers the kq nearest, the
    // full k only on demand inside the locate stage
    const int64_t kq = (ctx->lazy_lists && k > kLazyK) ? kLazyK : k;
    int *nn_full = nullptr;
    const double *tsorted = nullptr;
    mm_lazy_lists lazy;
    if (!resident) {
        rc = mm_buffer_get(ctx, MM_BUF_CENTROID, (size_t)nelem * 3 * sizeof(double), (void **)&cen);
        if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_BOX_PARTIAL, (size_t)kBoxBlocks * 6 * sizeof(double), (void **)&box_partial);
    }
    if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_NN, (size_t)npoints * (size_t)kq * sizeof(int), (void **)&nn);
    if (rc == MM_OK && kq < k)
        rc = mm_buffer_get(ctx, MM_BUF_NN_FULL, (size_t)npoints * (size_t)k * sizeof(int), (void **)&nn_full);
    // Few components: the interpolated values are formed inside the locate stage, at the point of
    // acceptance, and the operator rows are only materialised when the caller asks for them (both
    // pointers).  Many components: 8 gathers per component inside the register-heavy locate kernel
    // cost more than writing the rows and streaming them through the gather kernel.
    const bool want_values = out_d && ncomp > 0;
    const bool fuse_gather = want_values && ncomp <= kFuseGatherMaxComp;
    if (!(enc && w)) {
        enc = nullptr;
        w = nullptr;
        if (want_values && !fuse_gather) {
            if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_ENC, (size_t)npoints * 8 * sizeof(i64), (void **)&enc);
            if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_W, (size_t)npoints * 8 * sizeof(double), (void **)&w);
        }
    }
    if (rc != MM_OK) { result = rc; goto done; }

    // rows (and values) of failed points must read as zero (the reference's callers zero-initialise,
    // scripts/cli.py:77-78): the reference-order locate kernel, the only place a point can fail,
    // writes them (no 1.3 GB memset up front)

    // The search grid is laid out from the bounding box of the centroids, which the host would have to wait for in
    // mid-call.  When the previous call of this context left the box of a source mesh of the same size (the usual
    // case: one source mesh, many calls), the grid is GUESSED from that box and the guess is checked against this
    // call's own box after the synchronisation that ends the call; a wrong
    // guess runs the call again the ordinary way (twice wrong: no more guessing in this context).  MM_GRID_GUESS=0
    // switches it off.  A guessed call whose context also still holds the cell_start of that grid's sort
    // (grid_guess.cells_ok) guesses the per-cell counts as well and sorts the centroids as it computes them
    // (mm_knn_build_one_pass); other counts are a miss like another box.
    static const bool guess_on = !(getenv("MM_GRID_GUESS") && atoi(getenv("MM_GRID_GUESS")) == 0);
    // (MM_KNN_LEVELS is read per call by the ordinary build -- tests switch it inside one process -- and a guessed build
    // would ignore it)
    guessed = guess_on && ctx->grid_guess.valid && ctx->grid_guess.nsrc == nelem && ctx->grid_guess.misses < 2 &&
              !getenv("MM_KNN_LEVELS") && !resident;
again:
    ctx->abort_flags = nullptr;
    if (resident) {
        index = resident->index;   // centroids and grid are there: straight to the query
        goto query;
    }
    if (feed && (rc = feed_upload(ctx, feed, 0, 1, 0)) != MM_OK) { result = rc; goto done; }
    if (guessed && ctx->grid_guess.cells_ok) {
        // the context still holds the cell_start of this grid's last sort: centroids, box and sort in one pass over
        // the mesh (no centroid array; mm_knn_build_one_pass brackets both stages itself)
        ++ctx->grid_guess.calls_guessed;
        ctx->abort_flags = reinterpret_cast<int *>(ctx->d_counters + kMmAbortSlot);
        rc = mm_knn_build_one_pass(ctx, (const i64 *)conn_d, nodes_d, nelem, box_partial, kBoxBlocks, &index);
        if (rc != MM_OK) { result = rc; goto done; }
        goto query;
    }
    mm_stage_begin(ctx, MM_STAGE_CENTROID);
    rc = mm_launch_centroid_bbox(ctx, nelem, (const i64 *)conn_d, nodes_d, cen, box_partial, kBoxBlocks);
    mm_stage_end(ctx, MM_STAGE_CENTROID);
    if (rc != MM_OK) { result = rc; goto done; }

    mm_stage_begin(ctx, MM_STAGE_KNN_BUILD);
    ctx->abort_flags = nullptr;
    if (guessed) {
        ++ctx->grid_guess.calls_guessed;
        // (from here to the end of the call the ring searches and the locate kernels return at once when this call's box
        // turns out not to be the guessed one: bbox_final_kernel sets the flags on the device)
        ctx->abort_flags = reinterpret_cast<int *>(ctx->d_counters + kMmAbortSlot);
        rc = mm_knn_build_guessed(ctx, cen, nelem, box_partial, kBoxBlocks, &index);
    } else {
        rc = mm_knn_build_impl(ctx, cen, nelem, 3, &index, true, box_partial, kBoxBlocks);
    }
    mm_stage_end(ctx, MM_STAGE_KNN_BUILD);
    if (rc != MM_OK) { result = rc; goto done; }

query:
    if (feed && (rc = feed_upload(ctx, feed, 2, 2, 1)) != MM_OK) { result = rc; goto done; }
    mm_stage_begin(ctx, MM_STAGE_KNN_QUERY);
    // (the candidate rows come back in the cell-sorted order of the targets whenever the lane kernel serves the
    // query: the locate stage then walks the targets in that order, tsorted = their records)
    // (only with lazily evaluated lists: the reference-order kernel then reads the FULL lists, which are rows
    // by the targets' own indices; with eager lists it reads these rows and needs them in that order)
    rc = mm_knn_query_sorted_impl(ctx, index, points_d, npoints, kq, nn, kq < k ? &tsorted : nullptr);
    mm_stage_end(ctx, MM_STAGE_KNN_QUERY);
    if (rc != MM_OK) { result = rc; goto done; }

    // locate + gather: scripts/cli.py:86-100.  MM_STAGE_GATHER stays empty on this path (mm_gather is
    // the stand-alone A9 for callers that keep the operator).
    if (feed && (rc = feed_upload(ctx, feed, 3, 3, 2)) != MM_OK) { result = rc; goto done; }
    mm_stage_begin(ctx, MM_STAGE_LOCATE);
    lazy.index = index;
    lazy.k_full = k;
    lazy.nn_full = nn_full;
    rc = mm_launch_locate_hex8(ctx, kq, npoints, nn, /*int32=*/true, (const i64 *)conn_d, nelem, /*exodus=*/1, enc,
                               nodes_d, w, points_d, ctx->d_counters, /*zero_failed=*/1,
                               fuse_gather ? fields_d : nullptr, nnodes, ncomp, out_d,
                               kq < k ? &lazy : nullptr, tsorted);
    mm_stage_end(ctx, MM_STAGE_LOCATE);
    if (rc != MM_OK) { result = rc; goto done; }
    if (want_values && !fuse_gather) {
        mm_stage_begin(ctx, MM_STAGE_GATHER);
        rc = mm_launch_gather(ctx, fields_d, nnodes, ncomp, enc, w, npoints, 8, out_d, 1);
        mm_stage_end(ctx, MM_STAGE_GATHER);
        if (rc != MM_OK) { result = rc; goto done; }
    }

    rc = mm_mirror_async(ctx, (long long *)ctx->h_counters, (const long long *)ctx->d_counters, 1);
    if (rc != MM_OK) { result = rc; goto done; }
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) MM_PIPE_FAIL(MM_ERR_HIP, hipGetErrorString(e));
    if (guessed && !mm_knn_guess_confirmed(ctx)) {
        // not this mesh's grid: everything again, the ordinary way (which also leaves the right box for the next call)
        ctx->grid_guess.valid = false;
        ctx->grid_guess.cells_ok = false;
        ++ctx->grid_guess.misses;
        guessed = false;
        ctx->abort_flags = nullptr;
        mm_knn_destroy(nullptr, index);
        index = nullptr;
        feed = nullptr;   // (the device copies of host arrays are in place)
        mm_stage_reset(ctx);
        goto again;
    }
    result = ctx->h_counters[0];
    if (guessed) ctx->grid_guess.cells_ok = true;   // (confirmed: the buffers hold this grid's complete sort)
    // (a long-lived context forgives old misses: every 64 calls that confirmed their guess take one back)
    if (guessed && ctx->grid_guess.misses > 0 && (ctx->grid_guess.calls_guessed & 63) == 0) --ctx->grid_guess.misses;

done:
    ctx->abort_flags = nullptr;
    if (result < 0) (void)hipStreamSynchronize(ctx->stream);
    if (index && !resident) mm_knn_destroy(nullptr, index);  // borrowed arrays stay in the context cache
    return result;
#undef MM_PIPE_FAIL
}

// Debugging aid (not part of the drop-in surface): out4 = {a guess is held, calls that had to be run again, calls
// started from a guess, source elements of the guess}.
extern "C" int mm_debug_grid_guess(mm_context *ctx, long long *out4)
{
    MM_REQUIRE(ctx != nullptr && out4 != nullptr, "null argument");
    out4[0] = ctx->grid_guess.valid ? 1 : 0;
    out4[1] = ctx->grid_guess.misses;
    out4[2] = ctx->grid_guess.calls_guessed;
    out4[3] = ctx->grid_guess.nsrc;
    return MM_OK;
}

extern "C" int64_t mm_interpolate_hex8(mm_context *ctx, const double *nodes_d, int64_t nnodes,
                                       const int64_t *conn_d, int64_t nelem, const double *points_d,
                                       int64_t npoints, const double *fields_d, int64_t ncomp, int64_t k,
                                       double *out_d, int64_t *enc_d, double *w_d)
{
    return interpolate_hex8_impl(ctx, nodes_d, nnodes, conn_d, nelem, points_d, npoints, fields_d, ncomp, k, out_d,
                                 enc_d, w_d, nullptr);
}

extern "C" int mm_source_create(mm_context *ctx, const double *nodes_d, int64_t nnodes, const int64_t *conn_d, int64_t nelem,
                                mm_source **out)
{
    MM_REQUIRE(ctx != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    MM_REQUIRE(nnodes >= 1 && nelem >= 1 && nelem < (int64_t)0x7fffffff, "bad mesh size");
    MM_REQUIRE(nodes_d && conn_d, "null mesh array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_source *s = new (std::nothrow) mm_source();
    if (!s) {
        mm_set_error(MM_ERR_ALLOC, "out of host memory");
        return MM_ERR_ALLOC;
    }
    s->nodes = nodes_d;
    s->nnodes = nnodes;
    s->conn = (const i64 *)conn_d;
    s->nelem = nelem;
    s->device = ctx->device;
    int rc = MM_OK;
    if (mm_raw_alloc(ctx->device, (void **)&s->centroids, (size_t)nelem * 3 * sizeof(double)) != hipSuccess) {
        mm_set_error(MM_ERR_ALLOC, "mm_source_create: device allocation failed");
        rc = MM_ERR_ALLOC;
    }
    mm_stage_reset(ctx);
    if (rc == MM_OK) {
        mm_stage_begin(ctx, MM_STAGE_CENTROID);
        rc = mm_launch_centroid(ctx, 3, nelem, 8, (const i64 *)conn_d, nodes_d, s->centroids);
        mm_stage_end(ctx, MM_STAGE_CENTROID);
    }
    if (rc == MM_OK) {
        mm_stage_begin(ctx, MM_STAGE_KNN_BUILD);
        rc = mm_knn_build_impl(ctx, s->centroids, nelem, 3, &s->index, /*use_context_buffers=*/false, nullptr, 0, /*hex8_centroids=*/true);
        mm_stage_end(ctx, MM_STAGE_KNN_BUILD);
    }
    if (rc == MM_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        mm_set_error(MM_ERR_HIP, "mm_source_create: synchronise failed");
        rc = MM_ERR_HIP;
    }
    if (rc != MM_OK) {
        if (s->index) mm_knn_destroy(nullptr, s->index);
        if (s->centroids) (void)mm_raw_free(s->centroids);
        delete s;
        return rc;
    }
    *out = s;
    return MM_OK;
}

extern "C" void mm_source_destroy(mm_context *ctx, mm_source *source)
{
    if (!source) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    if (source->index) mm_knn_destroy(nullptr, source->index);
    if (source->centroids) (void)mm_raw_free(source->centroids);
    delete source;
}

extern "C" int64_t mm_interpolate_hex8_on(mm_context *ctx, const mm_source *source, const double *points_d,
                                          int64_t npoints, const double *fields_d, int64_t ncomp, int64_t k,
                                          double *out_d, int64_t *enc_d, double *w_d)
{
    MM_REQUIRE(ctx != nullptr && source != nullptr, "null argument");
    MM_REQUIRE(source->device == ctx->device, "the source lives on another device");
    return interpolate_hex8_impl(ctx, source->nodes, source->nnodes, (const int64_t *)source->conn, source->nelem, points_d,
                                 npoints, fields_d, ncomp, k, out_d, enc_d, w_d, nullptr, source);
}

// The same path fed from HOST arrays (what the reference's callers hold: NumPy arrays, scripts/cli.py:62-100):
// uploads overlapped with the kernels as described at mm_host_feed, device copies kept in the context's
// grow-only buffer cache (no hipMalloc / hipFree per call), results copied back into the caller's arrays.
// out_h f64[npoints][ncomp]; enc_h / w_h (both or neither) receive the operator rows.
extern "C" int64_t mm_interpolate_hex8_host(mm_context *ctx, const double *nodes_h, int64_t nnodes,
                                            const int64_t *conn_h, int64_t nelem, const double *points_h,
                                            int64_t npoints, const double *fields_h, int64_t ncomp, int64_t k,
                                            double *out_h, int64_t *enc_h, double *w_h)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(nnodes >= 1 && nelem >= 1, "empty source mesh");
    MM_REQUIRE(npoints >= 0 && ncomp >= 0, "negative size");
    MM_REQUIRE(nodes_h && conn_h, "null mesh array");
    MM_REQUIRE(npoints == 0 || points_h, "null target array");
    MM_REQUIRE(ncomp == 0 || out_h == nullptr || fields_h, "null field array");
    MM_REQUIRE((enc_h == nullptr) == (w_h == nullptr), "enc and w go together");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    if (npoints == 0) return 0;
    if (!ctx->copy_stream) {
        MM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        for (int q = 0; q < 3; ++q) MM_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_copy[q], hipEventDisableTiming));
    }
    const bool want_values = out_h && ncomp > 0;
    mm_host_feed feed;
    feed.src[0] = nodes_h;
    feed.bytes[0] = (size_t)nnodes * 3 * sizeof(double);
    feed.src[1] = conn_h;
    feed.bytes[1] = (size_t)nelem * 8 * sizeof(int64_t);
    feed.src[2] = points_h;
    feed.bytes[2] = (size_t)npoints * 3 * sizeof(double);
    feed.src[3] = fields_h;
    feed.bytes[3] = want_values ? (size_t)ncomp * (size_t)nnodes * sizeof(double) : 0;
    static const int slot[4] = {MM_BUF_H_NODES, MM_BUF_H_CONN, MM_BUF_H_POINTS, MM_BUF_H_FIELDS};
    for (int a = 0; a < 4; ++a) {
        int rc = mm_buffer_get(ctx, slot[a], feed.bytes[a], &feed.dst[a]);
        if (rc != MM_OK) return rc;
    }
    double *out_d = nullptr;
    i64 *enc_d = nullptr;
    double *w_d = nullptr;
    if (want_values) {
        int rc = mm_buffer_get(ctx, MM_BUF_H_OUT, (size_t)npoints * (size_t)ncomp * sizeof(double), (void **)&out_d);
        if (rc != MM_OK) return rc;
    }
    if (enc_h) {
        int rc = mm_buffer_get(ctx, MM_BUF_ENC, (size_t)npoints * 8 * sizeof(i64), (void **)&enc_d);
        if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_W, (size_t)npoints * 8 * sizeof(double), (void **)&w_d);
        if (rc != MM_OK) return rc;
    }
    // the uploads overwrite buffers the previous call's kernels may still read
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int64_t nfailed = interpolate_hex8_impl(ctx, (const double *)feed.dst[0], nnodes, (const int64_t *)feed.dst[1], nelem,
                                                  (const double *)feed.dst[2], npoints, (const double *)feed.dst[3],
                                                  want_values ? ncomp : 0, k, out_d, (int64_t *)enc_d, w_d, &feed);
    if (nfailed < 0) return nfailed;
    if (want_values)
        MM_HIP_CHECK(hipMemcpyAsync(out_h, out_d, (size_t)npoints * (size_t)ncomp * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (enc_h) {
        MM_HIP_CHECK(hipMemcpyAsync(enc_h, enc_d, (size_t)npoints * 8 * sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
        MM_HIP_CHECK(hipMemcpyAsync(w_h, w_d, (size_t)npoints * 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return nfailed;
}

// -----------------------------------------------------------------------------------------
// Legacy symbols (host pointers).  One process-wide context on device 0 / default stream.
// -----------------------------------------------------------------------------------------
static std::mutex g_legacy_mutex;
static mm_context *g_legacy_ctx = nullptr;

static mm_context *legacy_context()
{
    if (!g_legacy_ctx) {
        if (mm_context_create(0, nullptr, &g_legacy_ctx) != MM_OK) g_legacy_ctx = nullptr;
    }
    return g_legacy_ctx;
}

namespace {
// Smallest and largest entry of an index array that is already on the device: the reference's signatures do not
// carry the element and node counts, which are recovered as max + 1.  (Round 3 scanned the HOST arrays: ~1 ns per
// entry on one core, 0.9 of the 1.36 ms a warm triLinearInterpolator call took for 20 k points on a 64 k-element mesh
// -- reference scripts/cli.py:183-195 makes 125 such calls in a row.)
__global__ __launch_bounds__(256) void minmax_init_kernel(long long *out2)
{
    if (threadIdx.x == 0) {
        out2[0] = 0x7fffffffffffffffll;
        out2[1] = -1;
    }
}

__global__ __launch_bounds__(256) void minmax_i64_kernel(const i64 *__restrict__ a, size_t n, long long *__restrict__ out2)
{
    i64 lo = 0x7fffffffffffffffll, hi = -1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const i64 v = a[i];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const i64 l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(out2, lo);
        atomicMax(out2 + 1, hi);
    }
}

// lo / hi of a device array (synchronises the context's stream)
int device_minmax(mm_context *ctx, const i64 *a_d, size_t n, i64 *lo, i64 *hi)
{
    long long *slot = (long long *)(ctx->d_counters + 2);
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(256), 0, ctx->stream, slot);
    if (n > 0) {
        size_t grid = (n + 256 * 8 - 1) / (256 * 8);
        if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL(minmax_i64_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, a_d, n, slot);
    }
    MM_HIP_CHECK(hipGetLastError());
    MM_HIP_CHECK(hipMemcpyAsync(ctx->h_counters + 2, slot, 2 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *lo = ctx->h_counters[2];
    *hi = ctx->h_counters[3];
    return MM_OK;
}
}  // namespace

static int legacy_fail(const char *what)
{
    fprintf(stderr, "multi_mesh_hip: %s failed: %s\n", what, mm_last_error());
    return mm_last_status();
}

extern "C" void centroid(long long ndim, long long nelem, long long nper, long long *connectivity, double *points,
                         double *centroid_out)
{
    std::lock_guard<std::mutex> lock(g_legacy_mutex);
    mm_clear_status();
    if (nelem <= 0) return;
    if (ndim < 1 || ndim > 3 || nper < 1 || !connectivity || !points || !centroid_out) {
        mm_set_error(MM_ERR_ARG, "centroid: bad argument");
        (void)legacy_fail("centroid");
        return;
    }
    mm_context *ctx = legacy_context();
    if (!ctx) {
        (void)legacy_fail("centroid");
        return;
    }
    const size_t nconn = (size_t)nelem * (size_t)nper;
    // device copies from the context's grow-only cache (no hipMalloc / hipFree per call)
    void *d_conn = nullptr, *d_pts = nullptr, *d_out = nullptr;
    if (mm_buffer_get(ctx, MM_BUF_L_CONN, nconn * sizeof(i64), &d_conn) != MM_OK ||
        mm_buffer_get(ctx, MM_BUF_L_W, (size_t)nelem * ndim * sizeof(double), &d_out) != MM_OK) {
        (void)legacy_fail("centroid");
        return;
    }
    hipError_t e = hipMemcpyAsync(d_conn, connectivity, nconn * sizeof(i64), hipMemcpyHostToDevice, ctx->stream);
    // the number of points the signature does not carry: largest node id + 1, found on the device
    i64 id_lo = 0, id_hi = -1;
    if (e == hipSuccess && device_minmax(ctx, (const i64 *)d_conn, nconn, &id_lo, &id_hi) != MM_OK) {
        (void)legacy_fail("centroid");
        return;
    }
    if (e == hipSuccess && id_lo < 0) {
        mm_set_error(MM_ERR_ARG, "centroid: negative node id");
        (void)legacy_fail("centroid");
        return;
    }
    const i64 npoints = id_hi + 1;
    if (e == hipSuccess && mm_buffer_get(ctx, MM_BUF_L_NODES, (size_t)npoints * ndim * sizeof(double), &d_pts) != MM_OK) {
        (void)legacy_fail("centroid");
        return;
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_pts, points, (size_t)npoints * ndim * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        mm_set_error(MM_ERR_HIP, "centroid: %s", hipGetErrorString(e));
        (void)legacy_fail("centroid");
        return;
    }
    if (mm_centroid(ctx, ndim, nelem, nper, (const int64_t *)d_conn, (const double *)d_pts, (double *)d_out) != MM_OK) {
        (void)legacy_fail("centroid");
        return;
    }
    e = hipMemcpyAsync(centroid_out, d_out, (size_t)nelem * ndim * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        mm_set_error(MM_ERR_HIP, "centroid: %s", hipGetErrorString(e));
        (void)legacy_fail("centroid");
    }
}

extern "C" long long triLinearInterpolator(long long k, long long npoints, long long *nn, long long *connectivity,
                                           long long *enc, double *nodes, double *weights, double *points)
{
    std::lock_guard<std::mutex> lock(g_legacy_mutex);
    mm_clear_status();
    if (npoints <= 0 || k <= 0) return 0;  // the reference's loops do nothing
    if (!nn || !connectivity || !enc || !nodes || !weights || !points) {
        mm_set_error(MM_ERR_ARG, "triLinearInterpolator: null array");
        return legacy_fail("triLinearInterpolator");
    }
    mm_context *ctx = legacy_context();
    if (!ctx) return legacy_fail("triLinearInterpolator");
    // sizes the reference signature does not carry: largest index + 1, found on the DEVICE after the upload
    const size_t nnn = (size_t)npoints * (size_t)k;
    // device copies from the context's grow-only cache: the reference's exodus_2_gll flow calls this symbol once per
    // GLL point of the element (scripts/cli.py:183-195: 125 calls on the same mesh), and six hipMalloc / hipFree pairs
    // of mesh-sized buffers per call cost more than the kernels
    void *d_nn = nullptr, *d_conn = nullptr, *d_enc = nullptr, *d_nodes = nullptr, *d_w = nullptr, *d_pts = nullptr;
    if (mm_buffer_get(ctx, MM_BUF_L_NN, nnn * sizeof(i64), &d_nn) != MM_OK ||
        mm_buffer_get(ctx, MM_BUF_L_ENC, (size_t)npoints * 8 * sizeof(i64), &d_enc) != MM_OK ||
        mm_buffer_get(ctx, MM_BUF_L_W, (size_t)npoints * 8 * sizeof(double), &d_w) != MM_OK ||
        mm_buffer_get(ctx, MM_BUF_L_PTS, (size_t)npoints * 3 * sizeof(double), &d_pts) != MM_OK)
        return legacy_fail("triLinearInterpolator");
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(d_nn, nn, nnn * sizeof(i64), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pts, points, (size_t)npoints * 3 * sizeof(double), hipMemcpyHostToDevice, s);
    i64 lo = 0, hi = -1;
    if (e == hipSuccess && device_minmax(ctx, (const i64 *)d_nn, nnn, &lo, &hi) != MM_OK) return legacy_fail("triLinearInterpolator");
    if (e == hipSuccess && lo < 0) {
        mm_set_error(MM_ERR_ARG, "triLinearInterpolator: negative element index");
        return legacy_fail("triLinearInterpolator");
    }
    const i64 nelem = hi + 1;
    if (e == hipSuccess && mm_buffer_get(ctx, MM_BUF_L_CONN, (size_t)nelem * 8 * sizeof(i64), &d_conn) != MM_OK)
        return legacy_fail("triLinearInterpolator");
    if (e == hipSuccess) e = hipMemcpyAsync(d_conn, connectivity, (size_t)nelem * 8 * sizeof(i64), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && device_minmax(ctx, (const i64 *)d_conn, (size_t)nelem * 8, &lo, &hi) != MM_OK) return legacy_fail("triLinearInterpolator");
    if (e == hipSuccess && lo < 0) {
        mm_set_error(MM_ERR_ARG, "triLinearInterpolator: negative node id");
        return legacy_fail("triLinearInterpolator");
    }
    const i64 nnodes = hi + 1;
    if (e == hipSuccess && mm_buffer_get(ctx, MM_BUF_L_NODES, (size_t)nnodes * 3 * sizeof(double), &d_nodes) != MM_OK)
        return legacy_fail("triLinearInterpolator");
    if (e == hipSuccess) e = hipMemcpyAsync(d_nodes, nodes, (size_t)nnodes * 3 * sizeof(double), hipMemcpyHostToDevice, s);
    // in-place contract: rows of failed points keep the caller's contents
    if (e == hipSuccess) e = hipMemcpyAsync(d_enc, enc, (size_t)npoints * 8 * sizeof(i64), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_w, weights, (size_t)npoints * 8 * sizeof(double), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        mm_set_error(MM_ERR_HIP, "triLinearInterpolator: %s", hipGetErrorString(e));
        return legacy_fail("triLinearInterpolator");
    }
    const int64_t nfailed = mm_locate_hex8(ctx, k, npoints, (const int64_t *)d_nn, (const int64_t *)d_conn, nelem, 0,
                                           (int64_t *)d_enc, (const double *)d_nodes, (double *)d_w,
                                           (const double *)d_pts);
    if (nfailed < 0) return legacy_fail("triLinearInterpolator");
    e = hipMemcpyAsync(enc, d_enc, (size_t)npoints * 8 * sizeof(i64), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(weights, d_w, (size_t)npoints * 8 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        mm_set_error(MM_ERR_HIP, "triLinearInterpolator: %s", hipGetErrorString(e));
        return legacy_fail("triLinearInterpolator");
    }
    return nfailed;
}
