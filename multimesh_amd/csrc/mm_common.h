// Internal declarations shared by the HIP translation units of multi_mesh_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <memory>

#include "multimesh_hip.h"
#include "mm_scratch_layout.h"

typedef long long i64;

void mm_set_error(int code, const char *fmt, ...);

#define MM_HIP_CHECK(expr)                                                              \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            mm_set_error(MM_ERR_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,      \
                         hipGetErrorString(_e));                                        \
            return MM_ERR_HIP;                                                          \
        }                                                                               \
    } while (0)

#define MM_REQUIRE(cond, msg)                                                           \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            mm_set_error(MM_ERR_ARG, "%s: %s", __func__, msg);                          \
            return MM_ERR_ARG;                                                          \
        }                                                                               \
    } while (0)

// MM_REQUIRE on behalf of the entry point `who` (a helper's or a lambda's own __func__ would name the wrong function)
#define MM_REQUIRE_AS(who, cond, msg)                                                   \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            mm_set_error(MM_ERR_ARG, "%s: %s", who, msg);                               \
            return MM_ERR_ARG;                                                          \
        }                                                                               \
    } while (0)

// Grow-only device scratch: bump-allocated within one API call, reset at the start of the
// next.  Growing frees the old block after synchronising the stream (only while warming up).
struct mm_scratch {
    char *base = nullptr;
    size_t capacity = 0;
    size_t used = 0;
    size_t reserved = 0;          // bytes of the current reservation [base, base + reserved); 0 under MM_GUARD_ALLOC
    void *guard_piece[256] = {};  // MM_GUARD_ALLOC runs: every carve is an allocation of its own (a query over nine density
                                  // levels carves ~8 arrays per level on top of the shared ones)
    int guard_pieces = 0;
};

// Device allocations of the library go through these two.  With MM_GUARD_ALLOC=1 in the environment (test
// runs: tools/guard_run.sh) every allocation -- and every scratch carve -- is mapped so that it ENDS at the
// end of its mapping with unmapped address space behind it: a kernel that reads or writes past an array
// faults at once instead of now and then (there is no GPU AddressSanitizer on this pool).
// The guard catches reads PAST an array; reads of an array nobody has written are MM_SCRATCH_FILL's (below).
hipError_t mm_raw_alloc(int device, void **out, size_t bytes);
hipError_t mm_raw_free(void *ptr);
bool mm_guard_alloc(void);

// Grow-only device buffers the fused pipeline reuses from call to call (hipMalloc/hipFree of
// gigabyte-sized intermediates would otherwise cost milliseconds and a device sync per call).
enum mm_buffer_slot {
    MM_BUF_CENTROID = 0,
    MM_BUF_NN,
    MM_BUF_ENC,
    MM_BUF_W,
    MM_BUF_CELL_START,
    MM_BUF_SORTED_XYZ,
    MM_BUF_NN_FULL,
    MM_BUF_BOX_PARTIAL,
    MM_BUF_TSORTED,                       // targets in cell order {x, y, z, index} (kept for the locate stage)
    MM_BUF_H_NODES,                       // device copies of host arrays (mm_interpolate_hex8_host)
    MM_BUF_H_CONN,
    MM_BUF_H_POINTS,
    MM_BUF_H_FIELDS,
    MM_BUF_H_OUT,
    MM_BUF_L_NN,                          // device copies of the LEGACY symbols' host arrays (centroid, triLinearInterpolator):
    MM_BUF_L_CONN,                        //   grow-only like the rest, so a loop of calls (reference scripts/cli.py:183-195
    MM_BUF_L_ENC,                         //   calls triLinearInterpolator once per GLL point of the element: 125 times)
    MM_BUF_L_NODES,                       //   allocates once
    MM_BUF_L_W,
    MM_BUF_L_PTS,
    MM_BUF_LOC_SLOW,                      // locate stage: list of targets for the reference-order kernel + its counters
    MM_BUF_TREE_KEYS,                     // the kNN tree (graded clouds): Morton keys, records, leaf levels, search table
    MM_BUF_TREE_XYZ,
    MM_BUF_TREE_LEVEL,
    MM_BUF_TREE_COARSE,
    MM_BUF_TREE_DOWN,                     //   ... targets of a query whose first window overflowed the tile (second pass)
    MM_BUF_TPOS,                          // the fused hex8 pipeline's target sort, kept for the next call's replay
    MM_BUF_TSTART,                        //   (mm_context::target_replay): every target's position in MM_BUF_TSORTED, the
    MM_BUF_LANE_ITEMS,                    //   targets' cell starts, the lane kernel's work-item slots
    MM_BUF_LEVELS,                        // density levels of the kNN grid: {cell_start, sorted_xyz} per level
    MM_BUF_SAMPLE_POINTS = MM_BUF_LEVELS + 2 * 8,   // mm_sample_columns_gll: the chunk's generated targets
    MM_BUF_COUNT
};

struct mm_context {
    int device = 0;
    hipStream_t stream = nullptr;
    mm_scratch scratch;
    void *buf_ptr[MM_BUF_COUNT] = {};
    size_t buf_cap[MM_BUF_COUNT] = {};
    // failed-point counter + small readback area (device) and its pinned host mirror
    i64 *d_counters = nullptr;
    i64 *h_counters = nullptr;
    // stage timers
    int profiling = 0;
    int lazy_lists = 1;   // mm_set_lazy_lists
    int fp_mode = 0;      // mm_set_fp_mode (MM_FP_EXACT; MM_FP_MODE=tol in the environment starts contexts in MM_FP_TOL)
    hipEvent_t ev_begin[MM_STAGE_COUNT];
    hipEvent_t ev_end[MM_STAGE_COUNT];
    bool ev_used[MM_STAGE_COUNT];
    bool ev_created = false;
    hipEvent_t ev_misc = nullptr;   // host waits on small readbacks while later work stays queued
    // mm_interpolate_hex8: the bounding box of the previous call's centroids (one level, default density), from which
    // the next call over a source mesh of the same size lays its search grid out without waiting for its own box
    // (mm_knn_build_guessed / mm_knn_guess_confirmed in mm_knn.hip); misses: calls that had to be run again
    struct {
        bool valid = false;
        i64 nsrc = 0;
        double box[6] = {0, 0, 0, 0, 0, 0};
        int stat_shift = -1;
        // MM_BUF_CELL_START / MM_BUF_SORTED_XYZ hold the completed level-0 sort of nsrc sources on the grid of `box`, built
        // or confirmed by the previous call: the next guessed call may place its records by that cell_start in one pass
        // (mm_knn_build_one_pass).  Cleared by whatever else writes those two buffers (build_level).
        bool cells_ok = false;
        int misses = 0;
        long long calls_guessed = 0;   // (mm_debug_grid_guess: what the tests look at)
    } grid_guess;
    // mm_interpolate_hex8: the target sort of the previous fused call (knn_query_typed).  The guess is the grid guess's
    // -- this call's meshes are the previous call's --: then every target lies in the cell it lay in and its record belongs
    // where it went last time, MM_BUF_TPOS[i].  A replayed sort computes the cell from THIS call's coordinates, stores
    // the record at that position if it lies inside the cell's range of MM_BUF_TSTART, and raises the eighth mismatch
    // word (mm_aborted) and the pinned word kMmCountsBadSlot otherwise: no count, no scan, no atomic; the lane kernel's work
    // items (MM_BUF_LANE_ITEMS), a function of the cell starts alone, are last call's too.
    // The pipeline asks its query to keep the sort while guessing is on (mm_knn_query_sorted_impl).  ok: the three
    // buffers and MM_BUF_TSORTED hold the completed sort of npts targets on the grid {dims, geom} with the lane kernel's
    // launch shape {Z, nstrips_total, max_items}; cleared by whatever else takes MM_BUF_TSORTED, by a replay that
    // missed and by a failed call.
    struct {
        bool ok = false;
        bool replayed = false;   // this attempt's sort was a replay
        i64 npts = 0;
        int dims[3] = {0, 0, 0};
        double geom[6] = {0, 0, 0, 0, 0, 0};   // lo, inv_h: what cell_of_point reads
        int Z = 0;
        i64 nstrips_total = 0, max_items = 0;
        long long replays = 0, records = 0, item_lists = 0;   // (mm_debug_target_replay: replayed sorts, recorded sorts, work
                                                              // lists built for a kept sort)
    } target_replay;
    // kNN queries whose targets fill only part of the grid (knn_query_typed): the verdict of the occupied-strip statistic
    struct {
        bool valid = false;
        i64 npts = 0, ncells = 0;
        bool dense = false;
    } lane_hint;
    int knn_kernels = 0;   // MM_KNN_RAN_* bits of the kNN kernels launched since the last mm_stage_reset (mm_last_knn_kernels)
    int *abort_flags = nullptr;   // non-null during a call over a guessed grid: d_counters + kMmAbortSlot (mm_aborted)
    hipStream_t copy_stream = nullptr;   // host-array entry points: uploads run beside the kernels (created on first use)
    hipEvent_t ev_copy[3] = {nullptr, nullptr, nullptr};
    int scratch_fill = -1;         // MM_SCRATCH_FILL, read when the context is created: the fill byte, -1: off
    long long fills_queued = 0;    // (mm_debug_scratch)
};

// MM_SCRATCH_FILL=<byte> in the environment (a diagnostic; default off, and then one branch on scratch_fill): contexts
// created under it fill what they hand out and have not written with that byte, on ctx->stream -- every scratch
// reservation (each carve, under MM_GUARD_ALLOC), a grow-only buffer when it is allocated (never when it is handed out
// again), mm_device_alloc and the library's other allocations that are not fully written before use.  A kernel that reads
// scratch before the call wrote it then computes something that depends on the byte.  DESIGN.md section 7.
int mm_fill_unwritten(mm_context *ctx, void *dst_d, size_t bytes);   // nothing when the fill is off
hipError_t mm_ctx_alloc(mm_context *ctx, void **out, size_t bytes);  // mm_raw_alloc on ctx->device, then mm_fill_unwritten

// The scratch of a call: the drivers state their arrays in an mm_scratch_layout and commit it (mm_scratch_layout.h, which
// also declares mm_round256 and the two primitives under commit(): reserve, then carve piece by piece; mm_context.hip
// defines them and no driver calls them itself).  All carve sizes are rounded up to 256 B.
// bytes to clear for a carve of `b` bytes: whole 256-byte units (the carve is rounded up to them, and an odd
// tail costs a second fill dispatch) -- except under MM_GUARD_ALLOC, where the carve ends with its array
static inline size_t mm_fill_span(size_t b) { return mm_guard_alloc() ? b : mm_round256(b); }

// Zero `bytes` bytes of device memory on ctx->stream with a kernel of the library's own (see mm_context.hip: the runtime's
// fill is queued behind a barrier).
int mm_zero_async(mm_context *ctx, void *dst_d, size_t bytes);

// n (<= 64) 64-bit words of device memory into the context's pinned mirror, by a kernel on ctx->stream.
int mm_mirror_async(mm_context *ctx, long long *dst_pinned, const long long *src_d, int n);

// A caller's array that kernels read or write 16 bytes at a time (longlong2 / double2: connectivity rows, operator rows,
// kNN rows).  The header promises such an array the alignment of its elements only, so the entry point takes it through
// this: an array that starts on 16 bytes is used as it is -- the kernels and the aligned caller's path are what they were
// --, any other is replaced by a copy of the library's own for the call (an allocation, a copy in on ctx->stream, for an
// output a copy back, a wait and a free: correct, not fast).  DESIGN.md section 1, "Caller pointers and alignment".
class mm_aligned16 {
public:
    mm_aligned16() = default;
    mm_aligned16(const mm_aligned16 &) = delete;
    mm_aligned16 &operator=(const mm_aligned16 &) = delete;
    ~mm_aligned16();   // waits for the stream before it frees a copy
    // bytes: a multiple of 16 (a guarded allocation ends with its array); a null array stays null; copy_in false: an
    // output of which the call writes every byte
    int take(mm_context *ctx, const void *caller, size_t bytes, bool copy_in = true);
    int give_back();   // the copy's bytes into the caller's array, on the stream (nothing to do without a copy)
    void *release();   // the copy (or null), which is now the caller's to free with mm_raw_free after a wait
    template <typename T>
    T *as() const { return static_cast<T *>(copy_ ? copy_ : const_cast<void *>(caller_)); }

private:
    mm_context *ctx_ = nullptr;
    const void *caller_ = nullptr;
    void *copy_ = nullptr;
    size_t bytes_ = 0;
};

// The small counter readback of a call, words [slot, slot + n) of d_counters (the table of slots is below).  begin: their
// device address, zeroed by mm_zero_async.  end: hipGetLastError for the launches in between, mm_mirror_async, one
// hipStreamSynchronize (after a failure too: the caller may free what its kernels used); the n words in the pinned mirror.
// Both return null after a failure, with the error set.
unsigned long long *mm_counters_begin(mm_context *ctx, int slot, int n);
const i64 *mm_counters_end(mm_context *ctx, int slot, int n);

// Cached buffer of at least `bytes` for `slot` (grows by reallocation, after a stream sync).
int mm_buffer_get(mm_context *ctx, int slot, size_t bytes, void **out);

// Stage timing helpers: no-ops unless profiling is on.
void mm_stage_reset(mm_context *ctx);
void mm_stage_begin(mm_context *ctx, int stage);
void mm_stage_end(mm_context *ctx, int stage);

// Slots of mm_context::d_counters (64 x i64, zeroed when the context is created) / its pinned mirror h_counters:
//   0 failed / missing points of the call    1 mm_layers' counter    8..15 the hex8 locate stage's 16 counters
//   16..23 mm_boundary.hip's and mm_surface.hip's counts and the bounding box of mm_cutoff_distance / mm_surface_distance
//   28..29 mm_surface_distance: the entries of its grid, the median exponent of the triangles' extents
//   32..47 the grid statistic                48..53 (h_counters) the sources' bounding box
// ("The last workgroup of a launch finishes the reduction" was tried for the bounding box and the scans and
// measured: on this multi-XCD part the device-scope fence every workgroup needs before it takes its ticket writes
// its XCD's L2 back -- the centroid kernel went from 0.26 to 0.72 ms, a scan's first kernel from 5 to 80 us.)
//   24..27 (eight ints) mismatch flags of a guessed grid (mm_aborted)   2..3 scratch of small readbacks
//   54 (h_counters) the one-pass build's per-cell counts differ from the guess (cursor_check_kernel), or a replayed
//      target sort found a target outside last call's cell (target_replay_kernel)
constexpr int kMmStatSlot = 32, kMmBoxSlot = 48, kMmAbortSlot = 24;   // (slots 0..15 are cleared by every locate stage)
constexpr int kMmCountsBadSlot = 54;

// A call over a GUESSED search grid (mm_interpolate_hex8): abort6 = eight ints; the first six are non-zero when this
// call's bounding box is not the one the grid was laid out from, the seventh when a one-pass build found other per-cell
// counts than the ones it placed its records by, the eighth when a replayed target sort found a target outside the cell
// it lay in last call (a call on a resident source has only that one: the pipeline clears the block itself).  The
// kernels that would be ruinously slow on a foreign grid -- or read stale records -- ask first.
__device__ __forceinline__ bool mm_aborted(const int *__restrict__ abort6)
{
    if (!abort6) return false;
    const int4 a = *reinterpret_cast<const int4 *>(abort6);
    const int4 b = *reinterpret_cast<const int4 *>(abort6 + 4);
    return (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) != 0;
}

// ---- internal launchers (device pointers, no synchronisation) -------------------------
int mm_launch_centroid(mm_context *ctx, i64 ndim, i64 nelem, i64 nper, const i64 *conn,
                       const double *points, double *out);
// hex8 centroids + per-workgroup bounding boxes partial[nblocks][6] of them (fused pipeline)
int mm_launch_centroid_bbox(mm_context *ctx, i64 nelem, const i64 *conn, const double *points, double *out,
                            double *partial, int nblocks);
// enc/w: operator rows (may be null when out is given); fields [ncomp][nnodes] + out [npoints][ncomp]:
// interpolated values formed at the acceptance point (the gather fused into the locate), or null
// lazy (nullable): nn holds only the k nearest of k_full; targets that exhaust them get their full
// list from the index (written to nn_full int32[npoints][k_full], rows of those targets only) and
// go through the reference-order kernel
struct mm_knn_index;
struct mm_lazy_lists {
    const mm_knn_index *index;
    i64 k_full;
    int *nn_full;
};
int mm_launch_locate_hex8(mm_context *ctx, i64 k, i64 npoints, const void *nn, bool nn_is_int32,
                          const i64 *conn, i64 nelem, int conn_is_exodus, i64 *enc, const double *nodes,
                          double *w, const double *pts, i64 *d_nfailed, int zero_failed,
                          const double *fields, i64 nnodes, i64 ncomp, double *out,
                          const mm_lazy_lists *lazy, const double *tsorted = nullptr);
// full-length int32 lists for a device-side list of targets (generic kernel, rows idx[i*k ...])
// on-demand list queries at least this long (graded meshes) take the tiled kernels; the locate stage then also walks
// the rest of those targets' candidates with its pass kernel before the reference-order kernel sees what is left
#define MM_LONG_LIST_MIN 32768
// list_len_hint: the list's length when the caller has read it back (long lists then take the tiled kernels, which carve
// the context's scratch pool anew), -1 when it is only known on the device
int mm_knn_query_list_impl(mm_context *ctx, const mm_knn_index *ix, const double *pts_d, i64 npts, i64 k,
                           int *idx_d, const int *list, const int *list_count, i64 list_len_hint);
int mm_launch_gather(mm_context *ctx, const double *fields, i64 nsrc, i64 ncomp, const i64 *ids,
                     const double *w, i64 npoints, i64 P, double *out, int out_point_major);
// (mm_context.hip) the status mm_last_status reports back to MM_OK
void mm_clear_status(void);
// (mm_scan.hip; device side: mm_scan.h) exclusive prefix sum of n ints on ctx->stream: start[0..n]; tile_sums: scratch of
// mm_scan_scratch_ints(n) ints (with_total: one more, for the grand total mm_scan_launch_tile_offsets can write)
size_t mm_scan_scratch_ints(i64 n, bool with_total = false);
int mm_exclusive_scan_int(mm_context *ctx, const int *counts, i64 n, int *start, int *tile_sums);
// (mm_radix_sort.hip) the stable LSD radix sort of 64-bit keys with 32-bit values: passes over the key bits [first_shift,
// end_shift), 8 at a time, ping-pong between (ka, va) and (kb, vb); *in_a = the result lies in (ka, va).  scratch:
// mm_radix_sort_scratch(n) bytes.
size_t mm_radix_sort_scratch(i64 n);
int mm_radix_sort_pairs(mm_context *ctx, unsigned long long *ka, unsigned long long *kb, unsigned *va, unsigned *vb, i64 n,
                        int first_shift, int end_shift, void *scratch, bool *in_a);
// (mm_knn.hip) the kNN index without the stage timers: build -- plain, over a guessed grid, in one pass over the mesh --,
// the check of a guess after the call's last synchronisation, and the queries
int mm_knn_build_impl(mm_context *ctx, const double *src_d, i64 nsrc, i64 ndim, mm_knn_index **out,
                      bool use_context_buffers, const double *box_partial_d, int box_nblocks, bool hex8_centroids = false);
int mm_knn_build_guessed(mm_context *ctx, const double *cen, i64 nelem, const double *box_partial, int box_nblocks,
                         mm_knn_index **out);
int mm_knn_build_one_pass(mm_context *ctx, const i64 *conn, const double *nodes, i64 nelem, double *box_partial,
                          int box_nblocks, mm_knn_index **out);
bool mm_knn_guess_confirmed(mm_context *ctx);
int mm_knn_query_impl(mm_context *ctx, const mm_knn_index *ix, const double *pts_d, i64 npts, i64 k, void *idx_d,
                      double *dist_d, bool idx_is_int32);
// keep_sort: the targets' sort is kept for the next call, or replayed from the last one (mm_context::target_replay)
int mm_knn_query_sorted_impl(mm_context *ctx, const mm_knn_index *ix, const double *pts_d, i64 npts, i64 k, int *idx_d,
                             const double **tsorted_out, bool keep_sort);

// The density-adaptive part of a kNN index (mm_knn_tree.inc.h): the sources in Morton order.
struct mm_knn_tree {
    double lo[3] = {0, 0, 0};      // corner of the bounding cube
    double size = 1.0;             // its edge
    double scale = 1.0;            // finest cells per unit length
    unsigned long long *keys = nullptr;   // [nsrc] sorted Morton keys
    double *xyz = nullptr;                // [nsrc + 1][4] records in that order
    unsigned char *level = nullptr;       // [nsrc] level of the leaf around each source
    int *coarse = nullptr;                // first source of every level-7 cell
    bool borrowed = false;
};

// kNN search grid over source points (device resident).
struct mm_knn_index {
    i64 nsrc = 0;
    int ndim = 3;
    int dims[3] = {1, 1, 1};       // cells per axis
    double lo[3] = {0, 0, 0};      // bounding-box minimum
    double h[3] = {1, 1, 1};       // cell edge per axis
    double inv_h[3] = {1, 1, 1};
    i64 ncells = 1;
    int *cell_start = nullptr;     // [ncells + 1] exclusive prefix of per-cell counts
    double *sorted_xyz = nullptr;  // [nsrc][4] records {x, y, z, original index bits} in cell order
    bool borrowed = false;         // arrays belong to the context's buffer cache (fused pipeline)
    mm_knn_index *fine = nullptr;  // next density level: a grid over the same sources with smaller cells (owned)
    mm_knn_tree *tree = nullptr;   // graded clouds: the adaptive index that serves them instead of density levels (owned)
    bool graded() const { return fine != nullptr || tree != nullptr; }
};

// An index under construction, or built for one call of the fused pipeline: destroyed on every way out but the one that
// releases it to the caller.  (Hidden visibility: one type in every unit, and the library exports nothing of it.)
struct __attribute__((visibility("hidden"))) mm_index_deleter {
    void operator()(mm_knn_index *ix) const { mm_knn_destroy(nullptr, ix); }
};
using IndexOwner = std::unique_ptr<mm_knn_index, mm_index_deleter>;
