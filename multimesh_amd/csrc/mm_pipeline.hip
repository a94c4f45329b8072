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
    i64 *conn_copy = nullptr;      // owned: what conn points to when the caller's array starts off 16 bytes (mm_aligned16)
    double *centroids = nullptr;   // owned
    mm_knn_index *index = nullptr; // owned (its arrays are its own, not the context's buffer cache)
    int device = 0;
};

// The argument checks the device-pointer and the host-array entries share, reported in the name of `who`: the host entry
// makes them before it takes its buffers, and the pipeline then only adds its own two (on k between these, as ever).
static int require_sizes(const char *who, const mm_context *ctx, int64_t nnodes, int64_t nelem, int64_t npoints, int64_t ncomp)
{
    MM_REQUIRE_AS(who, ctx != nullptr, "ctx is null");
    MM_REQUIRE_AS(who, nnodes >= 1 && nelem >= 1, "empty source mesh");
    MM_REQUIRE_AS(who, nelem < (int64_t)0x7fffffff, "too many elements");
    MM_REQUIRE_AS(who, npoints >= 0 && ncomp >= 0, "negative size");
    return MM_OK;
}

static int require_arrays(const char *who, int64_t npoints, int64_t ncomp, const void *nodes, const void *conn,
                          const void *points, const void *fields, const void *out)
{
    MM_REQUIRE_AS(who, nodes && conn, "null mesh array");
    MM_REQUIRE_AS(who, npoints == 0 || points, "null target array");
    MM_REQUIRE_AS(who, ncomp == 0 || out == nullptr || fields, "null field array");
    return MM_OK;
}

// One call of the fused pipeline: its arguments (device pointers) and what is derived from them once.
struct hex8_call {
    const double *nodes;
    int64_t nnodes;
    const i64 *conn;
    int64_t nelem;
    const double *points;
    int64_t npoints;
    const double *fields;
    int64_t ncomp, k;
    double *out;
    const mm_source *resident;
    // lazily evaluated candidate lists (mm_set_lazy_lists): the kNN stage delivers the kq nearest, the
    // full k only on demand inside the locate stage (lazy.nn_full; lazy.index is the attempt's)
    int64_t kq;
    mm_lazy_lists lazy;
    // Few components: the interpolated values are formed inside the locate stage, at the point of
    // acceptance, and the operator rows are only materialised when the caller asks for them (both
    // pointers).  Many components: 8 gathers per component inside the register-heavy locate kernel
    // cost more than writing the rows and streaming them through the gather kernel.
    bool want_values, fuse_gather;
    // Intermediates come from the context's grow-only buffer cache: after the first call with a
    // given problem size there is no allocation, free or extra synchronisation in here.
    double *cen, *box_partial;
    int *nn;  // candidate lists stay int32 inside the pipeline (half the bytes of the public int64)
    i64 *enc;   // the caller's rows, the context's private ones (values wanted, gather not fused), or null
    double *w;
};

// Checks the arguments (host_checked: the host-array entry has made the shared checks), resets the stage timers
// and -- when there are targets -- takes the call's buffers.
static int describe_call(mm_context *ctx, const double *nodes_d, int64_t nnodes, const int64_t *conn_d, int64_t nelem,
                         const double *points_d, int64_t npoints, const double *fields_d, int64_t ncomp, int64_t k,
                         double *out_d, int64_t *enc_d, double *w_d, const mm_source *resident, bool host_checked,
                         hex8_call *call)
{
    static const char *const who = "interpolate_hex8_impl";
    int rc = MM_OK;
    if (!host_checked && (rc = require_sizes(who, ctx, nnodes, nelem, npoints, ncomp)) != MM_OK) return rc;
    MM_REQUIRE_AS(who, k >= 1 && k <= MM_KNN_MAX_K, "nelem_to_search must be in 1..MM_KNN_MAX_K");
    if (!host_checked && (rc = require_arrays(who, npoints, ncomp, nodes_d, conn_d, points_d, fields_d, out_d)) != MM_OK) return rc;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_stage_reset(ctx);
    *call = hex8_call{nodes_d, nnodes, (const i64 *)conn_d, nelem, points_d, npoints, fields_d, ncomp, k, out_d, resident};
    call->kq = (ctx->lazy_lists && k > kLazyK) ? kLazyK : k;
    call->lazy.k_full = k;
    call->want_values = out_d && ncomp > 0;
    call->fuse_gather = call->want_values && ncomp <= kFuseGatherMaxComp;
    if (npoints == 0) return MM_OK;

    const size_t np = (size_t)npoints;
    if (!resident) {
        rc = mm_buffer_get(ctx, MM_BUF_CENTROID, (size_t)nelem * 3 * sizeof(double), (void **)&call->cen);
        if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_BOX_PARTIAL, (size_t)kBoxBlocks * 6 * sizeof(double), (void **)&call->box_partial);
    }
    if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_NN, np * (size_t)call->kq * sizeof(int), (void **)&call->nn);
    if (rc == MM_OK && call->kq < k) rc = mm_buffer_get(ctx, MM_BUF_NN_FULL, np * (size_t)k * sizeof(int), (void **)&call->lazy.nn_full);
    if (enc_d && w_d) {
        call->enc = (i64 *)enc_d;
        call->w = w_d;
    } else if (call->want_values && !call->fuse_gather) {
        if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_ENC, np * 8 * sizeof(i64), (void **)&call->enc);
        if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_W, np * 8 * sizeof(double), (void **)&call->w);
    }
    if (rc != MM_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// The search grid is laid out from the bounding box of the centroids, which the host would have to wait for in
// mid-call.  When the previous call of this context left the box of a source mesh of the same size (the usual
// case: one source mesh, many calls), the grid is GUESSED from that box and the guess is checked against this
// call's own box after the synchronisation that ends the call; a wrong
// guess runs the call again the ordinary way (twice wrong: no more guessing in this context).  MM_GRID_GUESS=0
// switches it off.  A guessed call whose context also still holds the cell_start of that grid's sort
// (grid_guess.cells_ok) guesses the per-cell counts as well and sorts the centroids as it computes them
// (mm_knn_build_one_pass); other counts are a miss like another box.
// The same guess covers the targets: a call keeps its target sort for the next one (mm_context::target_replay), which puts
// its records where that sort put them and checks every one; a target that has left its cell is a miss like another box.
static bool guessing_on(const mm_context *ctx)
{
    static const bool guess_on = !(getenv("MM_GRID_GUESS") && atoi(getenv("MM_GRID_GUESS")) == 0);
    // (MM_KNN_LEVELS is read per call by the ordinary build -- tests switch it inside one process -- and a guessed build
    // would ignore it)
    return guess_on && ctx->grid_guess.misses < 2 && !getenv("MM_KNN_LEVELS");
}

static bool may_guess(const mm_context *ctx, const hex8_call &call)
{
    return guessing_on(ctx) && ctx->grid_guess.valid && ctx->grid_guess.nsrc == call.nelem && !call.resident;
}

// A call on a resident source has no box to guess, but its targets may be the previous call's: the mismatch words the
// replayed sort reports to are cleared here (a guessed build's bbox_final_kernel does it otherwise).
static int begin_resident_replay(mm_context *ctx)
{
    ctx->h_counters[kMmCountsBadSlot] = 0;   // (pinned; the stream is idle: every call that writes it ends with a wait)
    ctx->abort_flags = reinterpret_cast<int *>(ctx->d_counters + kMmAbortSlot);
    return mm_zero_async(ctx, ctx->abort_flags, 8 * sizeof(int));
}

// What a guessed call that ran to its end leaves in the context.
static void settle_guess(mm_context *ctx, bool guessed, bool confirmed)
{
    if (!confirmed) {
        // not this mesh's grid, or not these targets (the call is run again the ordinary way, which also leaves the right
        // box and the right target sort for the next call)
        if (guessed) ctx->grid_guess.valid = false;
        if (guessed) ctx->grid_guess.cells_ok = false;
        ctx->target_replay.ok = false;
        ++ctx->grid_guess.misses;
        return;
    }
    if (!guessed) return;
    ctx->grid_guess.cells_ok = true;   // (the buffers hold this grid's complete sort)
    // (a long-lived context forgives old misses: a confirmed guess that is the context's 64th, 128th, ... guessed call,
    // the missed ones counted, takes one back; with two misses nothing is guessed any more and nothing is taken back)
    if (ctx->grid_guess.misses > 0 && (ctx->grid_guess.calls_guessed & 63) == 0) --ctx->grid_guess.misses;
}

// From here to the end of a guessed attempt the ring searches and the locate kernels return at once when this call's
// box (or per-cell counts) turn out not to be the guessed ones: bbox_final_kernel sets the flags on the device.
static void begin_guessed_build(mm_context *ctx)
{
    ++ctx->grid_guess.calls_guessed;
    ctx->abort_flags = reinterpret_cast<int *>(ctx->d_counters + kMmAbortSlot);
}

// The index for this attempt: the resident source's (borrowed), or one built into `built` -- in one pass over the mesh
// when the context still holds the cell_start of the guessed grid's last sort, else centroids first.
static int index_for_attempt(mm_context *ctx, const hex8_call &call, bool guessed, IndexOwner *built, const mm_knn_index **index)
{
    if (call.resident) {
        *index = call.resident->index;   // centroids and grid are there: straight to the query
        return MM_OK;
    }
    mm_knn_index *made = nullptr;
    int rc = MM_OK;
    if (guessed && ctx->grid_guess.cells_ok) {
        // centroids, box and sort in one pass (no centroid array; mm_knn_build_one_pass brackets both stages itself)
        begin_guessed_build(ctx);
        rc = mm_knn_build_one_pass(ctx, call.conn, call.nodes, call.nelem, call.box_partial, kBoxBlocks, &made);
    } else {
        mm_stage_begin(ctx, MM_STAGE_CENTROID);
        rc = mm_launch_centroid_bbox(ctx, call.nelem, call.conn, call.nodes, call.cen, call.box_partial, kBoxBlocks);
        mm_stage_end(ctx, MM_STAGE_CENTROID);
        if (rc != MM_OK) return rc;
        mm_stage_begin(ctx, MM_STAGE_KNN_BUILD);
        if (guessed) {
            begin_guessed_build(ctx);
            rc = mm_knn_build_guessed(ctx, call.cen, call.nelem, call.box_partial, kBoxBlocks, &made);
        } else {
            rc = mm_knn_build_impl(ctx, call.cen, call.nelem, 3, &made, true, call.box_partial, kBoxBlocks);
        }
        mm_stage_end(ctx, MM_STAGE_KNN_BUILD);
    }
    built->reset(made);
    *index = made;
    return rc;
}

// The stages of one attempt, each host upload just before the stage that needs it (feed may be null); ends with the
// synchronisation after which the failed-point count is in the pinned mirror.
static int64_t run_stages(mm_context *ctx, const hex8_call &call, const mm_host_feed *feed, bool guessed, bool replay,
                          IndexOwner *built)
{
    const bool lazily = call.kq < call.k;
    int rc = MM_OK;
    if (feed && (rc = feed_upload(ctx, feed, 0, 1, 0)) != MM_OK) return rc;
    mm_lazy_lists lazy = call.lazy;
    if ((rc = index_for_attempt(ctx, call, guessed, built, &lazy.index)) != MM_OK) return rc;

    if (feed && (rc = feed_upload(ctx, feed, 2, 2, 1)) != MM_OK) return rc;
    mm_stage_begin(ctx, MM_STAGE_KNN_QUERY);
    // (the candidate rows come back in the cell-sorted order of the targets whenever the lane kernel serves the
    // query: the locate stage then walks the targets in that order, tsorted = their records)
    // (only with lazily evaluated lists: the reference-order kernel then reads the FULL lists, which are rows
    // by the targets' own indices; with eager lists it reads these rows and needs them in that order)
    const double *tsorted = nullptr;
    if (replay && call.resident && ctx->target_replay.ok && (rc = begin_resident_replay(ctx)) != MM_OK) return rc;
    // (the sort is kept while guessing is on; it is replayed where abort_flags is set: a guessed or a resident call)
    rc = mm_knn_query_sorted_impl(ctx, lazy.index, call.points, call.npoints, call.kq, call.nn, lazily ? &tsorted : nullptr,
                                  guessing_on(ctx));
    mm_stage_end(ctx, MM_STAGE_KNN_QUERY);
    if (rc != MM_OK) return rc;

    // locate + gather: scripts/cli.py:86-100.  MM_STAGE_GATHER stays empty on the fused path (mm_gather is
    // the stand-alone A9 for callers that keep the operator).
    // rows (and values) of failed points must read as zero (the reference's callers zero-initialise,
    // scripts/cli.py:77-78): the reference-order locate kernel, the only place a point can fail,
    // writes them (no 1.3 GB memset up front)
    if (feed && (rc = feed_upload(ctx, feed, 3, 3, 2)) != MM_OK) return rc;
    mm_stage_begin(ctx, MM_STAGE_LOCATE);
    rc = mm_launch_locate_hex8(ctx, call.kq, call.npoints, call.nn, /*int32=*/true, call.conn, call.nelem, /*exodus=*/1,
                               call.enc, call.nodes, call.w, call.points, ctx->d_counters, /*zero_failed=*/1,
                               call.fuse_gather ? call.fields : nullptr, call.nnodes, call.ncomp, call.out,
                               lazily ? &lazy : nullptr, tsorted);
    mm_stage_end(ctx, MM_STAGE_LOCATE);
    if (rc != MM_OK) return rc;
    if (call.want_values && !call.fuse_gather) {
        mm_stage_begin(ctx, MM_STAGE_GATHER);
        rc = mm_launch_gather(ctx, call.fields, call.nnodes, call.ncomp, call.enc, call.w, call.npoints, 8, call.out, 1);
        mm_stage_end(ctx, MM_STAGE_GATHER);
        if (rc != MM_OK) return rc;
    }

    rc = mm_mirror_async(ctx, (long long *)ctx->h_counters, (const long long *)ctx->d_counters, 1);
    if (rc != MM_OK) return rc;
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        mm_set_error(MM_ERR_HIP, "mm_interpolate_hex8: %s", hipGetErrorString(e));
        return MM_ERR_HIP;
    }
    return ctx->h_counters[0];
}

// One attempt at the call: the number of failed points, or a negative status after synchronising the stream.  The index
// the attempt built lives until here (its arrays are borrowed from the context cache and stay).
static int64_t attempt(mm_context *ctx, const hex8_call &call, const mm_host_feed *feed, bool guessed, bool replay)
{
    IndexOwner built;
    ctx->abort_flags = nullptr;
    ctx->target_replay.replayed = false;
    const int64_t result = run_stages(ctx, call, feed, guessed, replay, &built);
    ctx->abort_flags = nullptr;
    if (result < 0) {
        (void)hipStreamSynchronize(ctx->stream);
        ctx->target_replay.ok = false;
    }
    return result;
}

static int64_t interpolate_hex8_impl(mm_context *ctx, const double *nodes_d, int64_t nnodes,
                                     const int64_t *conn_d, int64_t nelem, const double *points_d,
                                     int64_t npoints, const double *fields_d, int64_t ncomp, int64_t k,
                                     double *out_d, int64_t *enc_d, double *w_d, const mm_host_feed *feed,
                                     const mm_source *resident, bool checked);

// The device-pointer entries' way in: the caller's operator rows, which the kernels write 16 bytes at a time, go through
// copies when they start off 16 bytes (mm_aligned16; every row is written, so nothing is copied in).  checked: the caller
// has made the shared argument checks.
static int64_t interpolate_hex8_with_rows(mm_context *ctx, const double *nodes_d, int64_t nnodes, const int64_t *conn_d,
                                          int64_t nelem, const double *points_d, int64_t npoints, const double *fields_d,
                                          int64_t ncomp, int64_t k, double *out_d, int64_t *enc_d, double *w_d,
                                          const mm_source *resident, bool checked)
{
    mm_aligned16 enc, w;
    const bool rows = ctx && enc_d && w_d && npoints > 0;
    int rc = rows ? hipSetDevice(ctx->device) == hipSuccess ? MM_OK : MM_ERR_HIP : MM_OK;
    if (rc == MM_OK) rc = enc.take(ctx, rows ? enc_d : nullptr, (size_t)(rows ? npoints : 0) * 8 * sizeof(i64), /*copy_in=*/false);
    if (rc == MM_OK) rc = w.take(ctx, rows ? w_d : nullptr, (size_t)(rows ? npoints : 0) * 8 * sizeof(double), /*copy_in=*/false);
    if (rc != MM_OK) return rc;
    const int64_t result = interpolate_hex8_impl(ctx, nodes_d, nnodes, conn_d, nelem, points_d, npoints, fields_d, ncomp, k, out_d,
                                                 rows ? enc.as<int64_t>() : enc_d, rows ? w.as<double>() : w_d, nullptr, resident, checked);
    if (result < 0) return result;
    if ((rc = enc.give_back()) != MM_OK || (rc = w.give_back()) != MM_OK) return rc;
    return result;
}

static int64_t interpolate_hex8_impl(mm_context *ctx, const double *nodes_d, int64_t nnodes,
                                     const int64_t *conn_d, int64_t nelem, const double *points_d,
                                     int64_t npoints, const double *fields_d, int64_t ncomp, int64_t k,
                                     double *out_d, int64_t *enc_d, double *w_d, const mm_host_feed *feed,
                                     const mm_source *resident, bool checked)
{
    hex8_call call;
    const int rc = describe_call(ctx, nodes_d, nnodes, conn_d, nelem, points_d, npoints, fields_d, ncomp, k, out_d, enc_d, w_d,
                                 resident, /*host_checked=*/checked, &call);
    if (rc != MM_OK) return rc;
    if (npoints == 0) return 0;
    const bool guessed = may_guess(ctx, call);
    int64_t result = attempt(ctx, call, feed, guessed, /*replay=*/true);
    if ((guessed || ctx->target_replay.replayed) && result >= 0) {
        // (a resident source's call guessed its targets alone: the one word the replayed sort raises)
        const bool confirmed = guessed ? mm_knn_guess_confirmed(ctx) : ctx->h_counters[kMmCountsBadSlot] == 0;
        settle_guess(ctx, guessed, confirmed);
        if (!confirmed) {
            // everything again without the guess -- and without the feed: the device copies of host arrays are in place
            mm_stage_reset(ctx);
            result = attempt(ctx, call, nullptr, false, false);
        }
    }
    return result;
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

// Debugging aid like mm_debug_grid_guess: out5 = {a target sort is held, fused calls that replayed it, fused calls that
// recorded one, targets of the held sort, lane work lists built for kept sorts (a replay builds none)}.
extern "C" int mm_debug_target_replay(mm_context *ctx, long long *out5)
{
    MM_REQUIRE(ctx != nullptr && out5 != nullptr, "null argument");
    out5[0] = ctx->target_replay.ok ? 1 : 0;
    out5[1] = ctx->target_replay.replays;
    out5[2] = ctx->target_replay.records;
    out5[3] = ctx->target_replay.npts;
    out5[4] = ctx->target_replay.item_lists;
    return MM_OK;
}

extern "C" int64_t mm_interpolate_hex8(mm_context *ctx, const double *nodes_d, int64_t nnodes,
                                       const int64_t *conn_d, int64_t nelem, const double *points_d,
                                       int64_t npoints, const double *fields_d, int64_t ncomp, int64_t k,
                                       double *out_d, int64_t *enc_d, double *w_d)
{
    // the shared argument checks, here and not in the pipeline: the connectivity rows are read 16 bytes at a time, and an
    // array off 16 bytes is copied (mm_aligned16) once its size is known to be sound
    static const char *const who = "interpolate_hex8_impl";
    int rc = require_sizes(who, ctx, nnodes, nelem, npoints, ncomp);
    if (rc == MM_OK) rc = require_arrays(who, npoints, ncomp, nodes_d, conn_d, points_d, fields_d, out_d);
    if (rc != MM_OK) return rc;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_aligned16 conn;
    if ((rc = conn.take(ctx, npoints > 0 ? conn_d : nullptr, (size_t)nelem * 8 * sizeof(i64))) != MM_OK) return rc;
    return interpolate_hex8_with_rows(ctx, nodes_d, nnodes, npoints > 0 ? conn.as<const int64_t>() : conn_d, nelem, points_d,
                                      npoints, fields_d, ncomp, k, out_d, enc_d, w_d, nullptr, /*checked=*/true);
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
    s->nelem = nelem;
    s->device = ctx->device;
    // the locate kernels read connectivity rows 16 bytes at a time: an array off 16 bytes is kept as a copy of the source's own
    mm_aligned16 conn;
    int rc = conn.take(ctx, conn_d, (size_t)nelem * 8 * sizeof(i64));
    s->conn = conn.as<const i64>();
    s->conn_copy = static_cast<i64 *>(conn.release());   // (the wait before this function returns covers the copy)
    if (rc == MM_OK && mm_ctx_alloc(ctx, (void **)&s->centroids, (size_t)nelem * 3 * sizeof(double)) != hipSuccess) {
        mm_set_error(MM_ERR_ALLOC, "mm_source_create: device allocation failed");
        rc = MM_ERR_ALLOC;
    }
    mm_stage_reset(ctx);
    if (rc == MM_OK) {
        mm_stage_begin(ctx, MM_STAGE_CENTROID);
        rc = mm_launch_centroid(ctx, 3, nelem, 8, s->conn, nodes_d, s->centroids);
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
        if (s->conn_copy) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)mm_raw_free(s->conn_copy);
        }
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
    if (source->conn_copy) (void)mm_raw_free(source->conn_copy);
    delete source;
}

extern "C" int64_t mm_interpolate_hex8_on(mm_context *ctx, const mm_source *source, const double *points_d,
                                          int64_t npoints, const double *fields_d, int64_t ncomp, int64_t k,
                                          double *out_d, int64_t *enc_d, double *w_d)
{
    MM_REQUIRE(ctx != nullptr && source != nullptr, "null argument");
    MM_REQUIRE(source->device == ctx->device, "the source lives on another device");
    return interpolate_hex8_with_rows(ctx, source->nodes, source->nnodes, (const int64_t *)source->conn, source->nelem, points_d,
                                      npoints, fields_d, ncomp, k, out_d, enc_d, w_d, source, /*checked=*/false);
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
    int rc = require_sizes(__func__, ctx, nnodes, nelem, npoints, ncomp);
    if (rc == MM_OK) rc = require_arrays(__func__, npoints, ncomp, nodes_h, conn_h, points_h, fields_h, out_h);
    if (rc != MM_OK) return rc;
    MM_REQUIRE((enc_h == nullptr) == (w_h == nullptr), "enc and w go together");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    if (npoints == 0) return 0;
    if (!ctx->copy_stream) {
        MM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        for (int q = 0; q < 3; ++q) MM_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_copy[q], hipEventDisableTiming));
    }
    const bool want_values = out_h && ncomp > 0;
    const size_t out_bytes = (size_t)npoints * (size_t)ncomp * sizeof(double);
    const size_t enc_bytes = (size_t)npoints * 8 * sizeof(i64), w_bytes = (size_t)npoints * 8 * sizeof(double);
    const struct {
        const void *src;
        size_t bytes;
        int slot;
    } arrays[4] = {{nodes_h, (size_t)nnodes * 3 * sizeof(double), MM_BUF_H_NODES},
                   {conn_h, (size_t)nelem * 8 * sizeof(int64_t), MM_BUF_H_CONN},
                   {points_h, (size_t)npoints * 3 * sizeof(double), MM_BUF_H_POINTS},
                   {fields_h, want_values ? (size_t)ncomp * (size_t)nnodes * sizeof(double) : 0, MM_BUF_H_FIELDS}};
    mm_host_feed feed;
    for (int a = 0; a < 4 && rc == MM_OK; ++a) {
        feed.src[a] = arrays[a].src;
        feed.bytes[a] = arrays[a].bytes;
        rc = mm_buffer_get(ctx, arrays[a].slot, arrays[a].bytes, &feed.dst[a]);
    }
    double *out_d = nullptr;
    i64 *enc_d = nullptr;
    double *w_d = nullptr;
    if (rc == MM_OK && want_values) rc = mm_buffer_get(ctx, MM_BUF_H_OUT, out_bytes, (void **)&out_d);
    if (rc == MM_OK && enc_h) rc = mm_buffer_get(ctx, MM_BUF_ENC, enc_bytes, (void **)&enc_d);
    if (rc == MM_OK && enc_h) rc = mm_buffer_get(ctx, MM_BUF_W, w_bytes, (void **)&w_d);
    if (rc != MM_OK) return rc;
    // the uploads overwrite buffers the previous call's kernels may still read
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int64_t nfailed = interpolate_hex8_impl(ctx, (const double *)feed.dst[0], nnodes, (const int64_t *)feed.dst[1], nelem,
                                                  (const double *)feed.dst[2], npoints, (const double *)feed.dst[3],
                                                  want_values ? ncomp : 0, k, out_d, (int64_t *)enc_d, w_d, &feed, nullptr, /*checked=*/true);
    if (nfailed < 0) return nfailed;
    if (want_values) MM_HIP_CHECK(hipMemcpyAsync(out_h, out_d, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (enc_h) {
        MM_HIP_CHECK(hipMemcpyAsync(enc_h, enc_d, enc_bytes, hipMemcpyDeviceToHost, ctx->stream));
        MM_HIP_CHECK(hipMemcpyAsync(w_h, w_d, w_bytes, hipMemcpyDeviceToHost, ctx->stream));
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

// A failed runtime call of the legacy symbol `who`, as its status.
static int legacy_hip(const char *who, hipError_t e)
{
    if (e == hipSuccess) return MM_OK;
    mm_set_error(MM_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return MM_ERR_HIP;
}

// A host array into the context's cache slot `slot` (grow-only: no hipMalloc / hipFree per call), on the context's stream.
static int legacy_upload(mm_context *ctx, const char *who, int slot, const void *src_h, size_t bytes, void **dst_d)
{
    const int rc = mm_buffer_get(ctx, slot, bytes, dst_d);
    if (rc != MM_OK) return rc;
    return legacy_hip(who, hipMemcpyAsync(*dst_d, src_h, bytes, hipMemcpyHostToDevice, ctx->stream));
}

// The number of rows an index array on the device implies -- the reference's signatures do not carry the element and
// node counts --: largest entry + 1.  A negative `what` is refused before any kernel dereferences it.  Synchronises.
static int legacy_count_rows(mm_context *ctx, const char *who, const char *what, const void *index_d, size_t n, i64 *rows)
{
    i64 lo = 0, hi = -1;
    const int rc = device_minmax(ctx, (const i64 *)index_d, n, &lo, &hi);
    if (rc != MM_OK) return rc;
    if (lo < 0) {
        mm_set_error(MM_ERR_ARG, "%s: negative %s", who, what);
        return MM_ERR_ARG;
    }
    *rows = hi + 1;
    return MM_OK;
}

static int legacy_centroid(long long ndim, long long nelem, long long nper, const long long *connectivity, const double *points,
                           double *centroid_out)
{
    static const char *const who = "centroid";
    if (ndim < 1 || ndim > 3 || nper < 1 || !connectivity || !points || !centroid_out) {
        mm_set_error(MM_ERR_ARG, "centroid: bad argument");
        return MM_ERR_ARG;
    }
    mm_context *ctx = legacy_context();
    if (!ctx) return MM_ERR_HIP;   // (mm_context_create has set the status that legacy_fail reports)
    const size_t nconn = (size_t)nelem * (size_t)nper, out_bytes = (size_t)nelem * ndim * sizeof(double);
    void *d_conn = nullptr, *d_pts = nullptr, *d_out = nullptr;
    i64 npoints = 0;   // (the signature does not carry it)
    int rc = mm_buffer_get(ctx, MM_BUF_L_W, out_bytes, &d_out);
    if (rc == MM_OK) rc = legacy_upload(ctx, who, MM_BUF_L_CONN, connectivity, nconn * sizeof(i64), &d_conn);
    if (rc == MM_OK) rc = legacy_count_rows(ctx, who, "node id", d_conn, nconn, &npoints);
    if (rc == MM_OK) rc = legacy_upload(ctx, who, MM_BUF_L_NODES, points, (size_t)npoints * ndim * sizeof(double), &d_pts);
    if (rc == MM_OK) rc = mm_centroid(ctx, ndim, nelem, nper, (const int64_t *)d_conn, (const double *)d_pts, (double *)d_out);
    if (rc == MM_OK) rc = legacy_hip(who, hipMemcpyAsync(centroid_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (rc == MM_OK) rc = legacy_hip(who, hipStreamSynchronize(ctx->stream));
    return rc;
}

extern "C" void centroid(long long ndim, long long nelem, long long nper, long long *connectivity, double *points,
                         double *centroid_out)
{
    std::lock_guard<std::mutex> lock(g_legacy_mutex);
    mm_clear_status();
    if (nelem <= 0) return;
    if (legacy_centroid(ndim, nelem, nper, connectivity, points, centroid_out) != MM_OK) (void)legacy_fail("centroid");
}

// The reference's exodus_2_gll flow calls this symbol once per GLL point of the element (scripts/cli.py:183-195: 125
// calls on the same mesh), and six hipMalloc / hipFree pairs of mesh-sized buffers per call cost more than the kernels:
// the device copies live in the context's cache.
static int64_t legacy_locate(long long k, long long npoints, const long long *nn, const long long *connectivity, long long *enc,
                             const double *nodes, double *weights, const double *points)
{
    static const char *const who = "triLinearInterpolator";
    if (!nn || !connectivity || !enc || !nodes || !weights || !points) {
        mm_set_error(MM_ERR_ARG, "triLinearInterpolator: null array");
        return MM_ERR_ARG;
    }
    mm_context *ctx = legacy_context();
    if (!ctx) return MM_ERR_HIP;   // (mm_context_create has set the status that legacy_fail reports)
    const size_t nnn = (size_t)npoints * (size_t)k;
    const size_t enc_bytes = (size_t)npoints * 8 * sizeof(i64), w_bytes = (size_t)npoints * 8 * sizeof(double);
    void *d_nn = nullptr, *d_conn = nullptr, *d_enc = nullptr, *d_nodes = nullptr, *d_w = nullptr, *d_pts = nullptr;
    i64 nelem = 0, nnodes = 0;   // (sizes the signature does not carry; nn is counted first: it says how many connectivity rows there are)
    int rc = mm_buffer_get(ctx, MM_BUF_L_ENC, enc_bytes, &d_enc);
    if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_L_W, w_bytes, &d_w);
    if (rc == MM_OK) rc = legacy_upload(ctx, who, MM_BUF_L_NN, nn, nnn * sizeof(i64), &d_nn);
    if (rc == MM_OK) rc = legacy_upload(ctx, who, MM_BUF_L_PTS, points, (size_t)npoints * 3 * sizeof(double), &d_pts);
    if (rc == MM_OK) rc = legacy_count_rows(ctx, who, "element index", d_nn, nnn, &nelem);
    if (rc == MM_OK) rc = legacy_upload(ctx, who, MM_BUF_L_CONN, connectivity, (size_t)nelem * 8 * sizeof(i64), &d_conn);
    if (rc == MM_OK) rc = legacy_count_rows(ctx, who, "node id", d_conn, (size_t)nelem * 8, &nnodes);
    if (rc == MM_OK) rc = legacy_upload(ctx, who, MM_BUF_L_NODES, nodes, (size_t)nnodes * 3 * sizeof(double), &d_nodes);
    // in-place contract: rows of failed points keep the caller's contents
    if (rc == MM_OK) rc = legacy_hip(who, hipMemcpyAsync(d_enc, enc, enc_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (rc == MM_OK) rc = legacy_hip(who, hipMemcpyAsync(d_w, weights, w_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (rc != MM_OK) return rc;
    const int64_t nfailed = mm_locate_hex8(ctx, k, npoints, (const int64_t *)d_nn, (const int64_t *)d_conn, nelem, 0,
                                           (int64_t *)d_enc, (const double *)d_nodes, (double *)d_w, (const double *)d_pts);
    if (nfailed < 0) return nfailed;
    rc = legacy_hip(who, hipMemcpyAsync(enc, d_enc, enc_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (rc == MM_OK) rc = legacy_hip(who, hipMemcpyAsync(weights, d_w, w_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (rc == MM_OK) rc = legacy_hip(who, hipStreamSynchronize(ctx->stream));
    return rc != MM_OK ? rc : nfailed;
}

extern "C" long long triLinearInterpolator(long long k, long long npoints, long long *nn, long long *connectivity,
                                           long long *enc, double *nodes, double *weights, double *points)
{
    std::lock_guard<std::mutex> lock(g_legacy_mutex);
    mm_clear_status();
    if (npoints <= 0 || k <= 0) return 0;  // the reference's loops do nothing
    const int64_t nfailed = legacy_locate(k, npoints, nn, connectivity, enc, nodes, weights, points);
    return nfailed < 0 ? legacy_fail("triLinearInterpolator") : nfailed;
}
