// Host test of multimesh_amd/csrc/mm_scratch_layout.h (tests/test_scratch_layout_host.py builds and runs this; no HIP,
// no GPU).  The context's pool is stubbed: addresses are handed out from a made-up base and never touched, so sizes
// beyond 4 GiB cost nothing; the stub follows mm_context.hip's two modes (one pool / one allocation per carve).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mm_scratch_layout.h"

struct mm_context {
    bool guard = false;
    size_t capacity = 0, used = 0, begun = 0;
    int begins = 0;
    std::vector<size_t> asked;   // byte counts mm_scratch_take was asked for since the last begin
    size_t cap_limit = 0;        // != 0: the pool pretends to hold only this much (a carve past it fails)
};

static const uintptr_t kBase = (uintptr_t)1 << 40;
static int g_code = 0;
static char g_msg[256] = "";

void mm_set_error(int code, const char *fmt, ...)
{
    g_code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
}

int mm_scratch_begin(mm_context *ctx, size_t total)
{
    ctx->begun = total;
    ctx->capacity = ctx->cap_limit ? ctx->cap_limit : mm_round256(total) + 4096;
    ctx->used = 0;
    ctx->asked.clear();
    ++ctx->begins;
    return MM_OK;
}

void *mm_scratch_take(mm_context *ctx, size_t bytes)
{
    if (ctx->used + mm_round256(bytes) > ctx->capacity) return nullptr;
    ctx->asked.push_back(bytes);
    void *p;
    if (ctx->guard) p = (void *)(kBase + ((uintptr_t)ctx->asked.size() << 36));   // an allocation of its own
    else p = (void *)(kBase + ctx->used);
    ctx->used += mm_round256(bytes);
    return p;
}

static int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

static size_t off(const void *p) { return (size_t)((uintptr_t)p - kBase); }

// a helper that contributes its arrays to its caller's layout, of the shape the GLL locate's visiting order has
struct Visit {
    long long *key_rank = nullptr;
    int *ord = nullptr, *counts = nullptr, *start = nullptr, *tile_sums = nullptr;
    void add(mm_scratch_layout &lay, int kavail, size_t npoints, size_t nelem)
    {
        if (kavail <= 0 || nelem == 0) return;
        lay.add(&key_rank, npoints);
        lay.add(&ord, npoints);
        lay.add(&counts, nelem + 2);
        lay.add(&start, nelem + 2);
        lay.add(&tile_sums, (nelem + 1 + 1023) / 1024);
    }
};

static void test_order_and_total()
{
    mm_context ctx;
    double *a;
    int *b, *c, *skipped = (int *)&ctx, *zero;
    char *d;
    void *raw;
    mm_scratch_layout lay;
    const size_t na = 3, nb = 64, nc = 65, nd = 1000, nraw = 257;
    lay.add(&a, na);
    lay.add(&b, nb);
    lay.add(&c, nc);
    skipped = nullptr;              // an array that is not added: the layout never sees it
    lay.add(&zero, 0);              // zero count: one byte, a slot of its own
    lay.add(&d, nd);
    lay.add(&raw, nraw);            // untyped: bytes
    const size_t sizes[6] = {na * sizeof(double), nb * sizeof(int), nc * sizeof(int), 1, nd, nraw};
    size_t sum = 0;
    for (size_t s : sizes) sum += mm_round256(s);
    CHECK(lay.total() == sum);
    CHECK(a == nullptr && d == nullptr);   // add() clears the slot until commit
    CHECK(lay.commit(&ctx, "test_entry") == MM_OK);
    CHECK(ctx.begins == 1 && ctx.begun == sum);   // exactly the sum: no slack terms
    const void *p[6] = {a, b, c, zero, d, raw};
    size_t expect = 0;
    for (int i = 0; i < 6; ++i) {
        CHECK(p[i] != nullptr);
        CHECK(off(p[i]) % 256 == 0);
        CHECK(off(p[i]) == expect);                       // add order, no overlap, no gaps beyond the rounding
        if (i) CHECK(off(p[i]) >= off(p[i - 1]) + sizes[i - 1]);
        expect += mm_round256(sizes[i]);
    }
    CHECK(ctx.used == sum);
    CHECK(skipped == nullptr);
    // adjacency: b's size is a multiple of 256, so c starts where b ends; a's is not a multiple but rounds up
    CHECK(mm_scratch_adjacent(b, nb * sizeof(int), c));
    CHECK(mm_scratch_adjacent(a, na * sizeof(double), b));
    CHECK(!mm_scratch_adjacent(a, na * sizeof(double), c));
}

static void test_nested()
{
    for (int with_visit = 0; with_visit < 2; ++with_visit) {
        mm_context ctx;
        double *boxes;
        Visit v;
        mm_scratch_layout lay;
        const size_t nelem = 5000, npoints = 777;
        lay.add(&boxes, nelem * 9);
        v.add(lay, with_visit ? 4 : 0, npoints, nelem);
        CHECK(lay.commit(&ctx, "nested") == MM_OK);
        size_t sum = mm_round256(nelem * 9 * sizeof(double));
        if (with_visit) {
            sum += mm_round256(npoints * sizeof(long long)) + mm_round256(npoints * sizeof(int)) +
                   2 * mm_round256((nelem + 2) * sizeof(int)) + mm_round256(5 * sizeof(int));
            CHECK(off(v.key_rank) == mm_round256(nelem * 9 * sizeof(double)));   // right behind the caller's own array
            CHECK(v.key_rank && v.ord && v.counts && v.start && v.tile_sums);
            CHECK(off(v.tile_sums) + mm_round256(5 * sizeof(int)) == sum);
        } else {
            CHECK(!v.key_rank && !v.ord && !v.counts && !v.start && !v.tile_sums);   // nothing to sort by: nothing added
        }
        CHECK(ctx.begun == sum && ctx.used == sum);
    }
}

static void test_large()
{
    mm_context ctx;
    double *big;
    int *mid, *tail;
    mm_scratch_layout lay;
    const size_t nbig = ((size_t)5 << 30) / sizeof(double) + 1;   // 5 GiB + 8 bytes
    const size_t nmid = ((size_t)1 << 32) + 3;                    // 16 GiB + 12 bytes
    lay.add(&big, nbig);
    lay.add(&mid, nmid);
    lay.add(&tail, 1);
    const size_t sum = mm_round256(nbig * sizeof(double)) + mm_round256(nmid * sizeof(int)) + 256;
    CHECK(sum > ((size_t)21 << 30));
    CHECK(lay.total() == sum);
    CHECK(lay.commit(&ctx, "large") == MM_OK);
    CHECK(off(big) == 0);
    CHECK(off(mid) == ((size_t)5 << 30) + 256);
    CHECK(off(tail) == ((size_t)5 << 30) + 256 + ((size_t)16 << 30) + 256);
    CHECK(ctx.begun == sum);
}

static void test_guarded()
{
    mm_context ctx;
    ctx.guard = true;
    double *a;
    int *b, *zero;
    unsigned char *c;
    mm_scratch_layout lay;
    lay.add(&a, 3);
    lay.add(&b, 65);
    lay.add(&zero, 0);
    lay.add(&c, 1001);
    CHECK(lay.commit(&ctx, "guarded") == MM_OK);
    // every entry is a request of its own for its EXACT byte count (an array then ends with its mapping)
    CHECK(ctx.asked.size() == 4);
    if (ctx.asked.size() == 4) {
        CHECK(ctx.asked[0] == 24 && ctx.asked[1] == 260 && ctx.asked[2] == 1 && ctx.asked[3] == 1001);
    }
    CHECK(a && b && zero && c && (void *)a != (void *)b && (void *)b != (void *)zero && (void *)zero != (void *)c);
    CHECK(!mm_scratch_adjacent(a, 24, b));   // code that relies on adjacency must find it missing here
}

static void test_failure()
{
    // a pool that is too small: one message, the code the site asks for, prefixed with the entry point
    for (int code : {MM_ERR_ALLOC, MM_ERR_ARG}) {
        mm_context ctx;
        ctx.cap_limit = 512;
        int *a, *b;
        mm_scratch_layout lay;
        lay.add(&a, 64);
        lay.add(&b, 1000);
        g_code = 0;
        const int rc = code == MM_ERR_ALLOC ? lay.commit(&ctx, "mm_entry_point") : lay.commit(&ctx, "mm_entry_point", code);
        CHECK(rc == code && g_code == code);
        CHECK(strcmp(g_msg, "mm_entry_point: scratch carve failed") == 0);
        CHECK(a != nullptr && b == nullptr);
    }
    // more entries than the layout (and the guard) tracks: refused at commit, not written past the table
    mm_context ctx;
    static int *slots[mm_scratch_layout::kMaxEntries + 1];
    mm_scratch_layout lay;
    for (int i = 0; i <= mm_scratch_layout::kMaxEntries; ++i) lay.add(&slots[i], 1);
    CHECK(lay.commit(&ctx, "many") == MM_ERR_ALLOC);
    // a second commit on the same context starts the pool anew
    mm_context ctx2;
    int *x, *y;
    mm_scratch_layout l1, l2;
    l1.add(&x, 10);
    l2.add(&y, 10);
    CHECK(l1.commit(&ctx2, "first") == MM_OK && l2.commit(&ctx2, "second") == MM_OK);
    CHECK(x == y && ctx2.begins == 2);
}

int main()
{
    test_order_and_total();
    test_nested();
    test_large();
    test_guarded();
    test_failure();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("scratch layout: all checks passed\n");
    return 0;
}
