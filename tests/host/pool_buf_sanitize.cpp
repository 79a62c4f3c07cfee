// CPU-only check of the scoped owner of pool buffers (kiez_amd/csrc/kz_pool_buf.h), built with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// by tests/test_host_sanitize.py against a fake pool that records every allocation and release:
//   * a function with several early returns, an early reset() and a move releases every buffer exactly once, on every path;
//   * the owners of one scope release in reverse declaration order (the release order the host code relies on);
//   * a failed allocation leaves the owner empty; alloc() on a full owner releases the old buffer first;
//   * the fake pool ends with zero live buffers.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../kiez_amd/csrc/kz_pool_buf.h"

static int fails = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            ++fails;                                         \
        }                                                    \
    } while (0)

// ---- the fake pool: real host memory (ASan sees a double release or a leak), every release logged --------------------------------
struct kz_ctx {
    int live = 0;
    int allocs = 0;
    int fail_at = -1;             // the allocation with this number fails (-1: none)
    std::vector<void*> released;  // in release order
};
int kz_pool_alloc(kz_ctx* ctx, size_t bytes, void** out) {
    *out = nullptr;
    if (ctx->allocs++ == ctx->fail_at) return 3;   // (KZ_ERR_NOMEM)
    *out = std::malloc(bytes ? bytes : 16);
    ++ctx->live;
    return 0;
}
void kz_pool_free(kz_ctx* ctx, void* ptr, size_t) {
    if (!ptr) return;
    ctx->released.push_back(ptr);
    --ctx->live;
    std::free(ptr);
}

static bool released_once(const kz_ctx& c, const void* p) {
    int n = 0;
    for (void* q : c.released) n += q == p;
    return n == 1;
}

// A host routine of the shape kz_knn_impl has: buffers taken one after the other, an early reset(), a buffer handed on by a move,
// and a return after every step.  `stop` picks the return.
static int routine(kz_ctx* ctx, int stop, std::vector<void*>* seen) {
    KzPoolBuf<double> c;
    KzPoolBuf<int> b;
    KzPoolBuf<float> a;
    int rc = a.alloc(ctx, 64);
    if (rc != 0) return rc;
    seen->push_back(a.get());
    if (stop == 0) return 1;
    rc = b.alloc(ctx, 128);
    if (rc != 0) return rc;
    seen->push_back(b.get());
    if (stop == 1) return 1;
    a.reset();   // (released early, as the host code does at a release point)
    CHECK(a.get() == nullptr, "reset() leaves the owner empty");
    if (stop == 2) return 1;
    {
        KzPoolBuf<int> left;
        rc = left.alloc(ctx, 32);
        if (rc != 0) return rc;
        seen->push_back(left.get());
        if (stop == 3) return 1;
        b = std::move(left);   // (the old b goes, left's buffer takes its place)
        CHECK(left.get() == nullptr, "a moved-from owner is empty");
    }
    if (stop == 4) return 1;
    rc = c.alloc(ctx, 8);
    if (rc != 0) return rc;
    seen->push_back(c.get());
    KzPoolBuf<double> d(std::move(c));
    CHECK(c.get() == nullptr && d.get() != nullptr, "move construction takes the buffer");
    if (stop == 5) return 1;
    return 0;
}

int main() {
    // every return of the routine, and every allocation failing in turn
    for (int stop = 0; stop <= 6; ++stop)
        for (int fail_at = -1; fail_at < 4; ++fail_at) {
            kz_ctx ctx;
            ctx.fail_at = fail_at;
            std::vector<void*> seen;
            (void)routine(&ctx, stop, &seen);
            CHECK(ctx.live == 0, "stop %d, fail_at %d: %d buffers still live", stop, fail_at, ctx.live);
            CHECK(ctx.released.size() == seen.size(), "stop %d, fail_at %d: %zu released, %zu taken", stop, fail_at, ctx.released.size(),
                  seen.size());
            for (void* p : seen) CHECK(released_once(ctx, p), "stop %d, fail_at %d: a buffer not released exactly once", stop, fail_at);
        }
    // release order of one scope: reverse declaration order
    {
        kz_ctx ctx;
        void *p1, *p2, *p3;
        {
            KzPoolBuf<char> third, second, first;
            (void)first.alloc(&ctx, 1);
            (void)second.alloc(&ctx, 1);
            (void)third.alloc(&ctx, 1);
            p1 = first.get();
            p2 = second.get();
            p3 = third.get();
        }
        CHECK(ctx.released.size() == 3 && ctx.released[0] == p1 && ctx.released[1] == p2 && ctx.released[2] == p3,
              "owners of a scope release in reverse declaration order");
        CHECK(ctx.live == 0, "%d buffers still live", ctx.live);
    }
    // a failed allocation leaves the owner empty; alloc() on a full owner releases the old buffer first; self move-assignment keeps it
    {
        kz_ctx ctx;
        KzPoolBuf<int> x;
        CHECK(x.alloc(&ctx, 16) == 0 && x.get() != nullptr, "allocation");
        void* old = x.get();
        ctx.fail_at = ctx.allocs;
        CHECK(x.alloc(&ctx, 16) == 3 && x.get() == nullptr, "a failed allocation leaves the owner empty");
        CHECK(released_once(ctx, old), "the old buffer is released before the new one is taken");
        CHECK(x.alloc(&ctx, 16) == 0 && x.get() != nullptr, "allocation after a failure");
        KzPoolBuf<int>& alias = x;
        x = std::move(alias);
        CHECK(x.get() != nullptr, "self move-assignment keeps the buffer");
        x.reset();
        x.reset();
        CHECK(ctx.live == 0 && ctx.released.size() == 2, "reset() twice releases once (%d live, %zu released)", ctx.live, ctx.released.size());
    }
    std::printf("%d failures\n", fails);
    return fails == 0 ? 0 : 1;
}
