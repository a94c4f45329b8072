// The scratch of one call, stated once: every array is named with its element count in ONE place, and commit() sums the
// sizes, reserves the pool and hands every pointer out.
//
//     mm_scratch_layout lay;
//     lay.add(&key_a, n);                        // typed: T **, element count
//     if (l->fine) lay.add(&down_list, npts);    // arrays that are not added stay as they were (null)
//     int rc = lay.commit(ctx, __func__);        // mm_scratch_begin(sum), one mm_scratch_take per entry, one error message
//
// Rules:
//  * entries are carved in the order added, each rounded up to 256 B; the reservation is exactly the sum of the rounded
//    sizes (mm_scratch_begin adds its own 4096).  Two entries added one after the other are therefore ADJACENT in the pool
//    when the first one's size is a multiple of 256 -- mm_scratch_adjacent() is the run-time check for code that relies on
//    it (not so under MM_GUARD_ALLOC, where every entry is an allocation of its own with its exact byte count);
//  * a zero-count entry takes one byte: a valid, distinct 256-byte slot, never null (a launch over zero elements may still
//    be handed the pointer);
//  * a helper contributes its arrays to its caller's layout: it takes the layout by reference and add()s, the caller
//    commits once;
//  * commit() starts the pool anew (mm_scratch_begin): what an earlier layout of the same context handed out is gone.
//
// Nothing here needs HIP: the four functions below are the whole interface to the context (mm_context.hip defines them;
// tests/host/scratch_layout_host.cpp stubs them).
#pragma once

#include <stddef.h>

#include "multimesh_hip.h"

struct mm_context;
int mm_scratch_begin(mm_context *ctx, size_t total);
void *mm_scratch_take(mm_context *ctx, size_t bytes);
void mm_set_error(int code, const char *fmt, ...);

static inline size_t mm_round256(size_t b) { return (b + 255) & ~(size_t)255; }

// b is the entry added right after a (of a_bytes bytes) and starts where a's rounded size ends
static inline bool mm_scratch_adjacent(const void *a, size_t a_bytes, const void *b)
{
    return (const char *)b == (const char *)a + mm_round256(a_bytes);
}

// (hidden: a header-only helper of the library, not one of its exported symbols)
struct __attribute__((visibility("hidden"))) mm_scratch_layout {
    static constexpr int kMaxEntries = 256;   // (the guard's piece limit: mm_scratch::guard_piece)
    struct entry {
        void **slot;
        size_t bytes;
    };
    entry e[kMaxEntries];
    int n = 0;
    bool overflow = false;

    void add_bytes(void **slot, size_t bytes)
    {
        *slot = nullptr;
        if (n >= kMaxEntries) {
            overflow = true;
            return;
        }
        e[n].slot = slot;
        e[n].bytes = bytes > 0 ? bytes : 1;
        ++n;
    }
    template <typename T>
    void add(T **slot, size_t count)
    {
        add_bytes(reinterpret_cast<void **>(slot), count * sizeof(T));
    }
    void add(void **slot, size_t bytes) { add_bytes(slot, bytes); }

    size_t total() const
    {
        size_t t = 0;
        for (int i = 0; i < n; ++i) t += mm_round256(e[i].bytes);
        return t;
    }

    // `who`: the entry point the error message names; `code`: MM_ERR_ALLOC, or MM_ERR_ARG at the sites that have always
    // reported a failed carve with MM_REQUIRE (the GLL locate's)
    int commit(mm_context *ctx, const char *who, int code = MM_ERR_ALLOC)
    {
        int rc = mm_scratch_begin(ctx, total());
        if (rc != MM_OK) return rc;
        bool ok = !overflow;
        for (int i = 0; i < n && ok; ++i) ok = (*e[i].slot = mm_scratch_take(ctx, e[i].bytes)) != nullptr;
        if (!ok) {
            mm_set_error(code, "%s: %s", who, "scratch carve failed");
            return code;
        }
        return MM_OK;
    }
};
