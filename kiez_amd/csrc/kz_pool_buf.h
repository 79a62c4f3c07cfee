// Scoped owner of one transient buffer of the context's pool: the destructor hands the buffer back with kz_pool_free.  Release
// is stream-ordered exactly as kz_pool_free is (kz_runtime.hip): the owner neither synchronises nor remembers a size.  Owners
// are destroyed in reverse declaration order, so the declaration order of a scope is its release order.
// No HIP here: tests/host/pool_buf_sanitize.cpp compiles this header against a fake pool.
#pragma once
#include <cstddef>

struct kz_ctx;
int kz_pool_alloc(kz_ctx* ctx, size_t bytes, void** out);   // returns KZ_OK / KZ_ERR_NOMEM
void kz_pool_free(kz_ctx* ctx, void* ptr, size_t bytes);

template <class T>
class KzPoolBuf {
public:
    KzPoolBuf() = default;
    KzPoolBuf(const KzPoolBuf&) = delete;
    KzPoolBuf& operator=(const KzPoolBuf&) = delete;
    KzPoolBuf(KzPoolBuf&& o) noexcept : ctx_(o.ctx_), ptr_(o.ptr_) { o.ptr_ = nullptr; }
    KzPoolBuf& operator=(KzPoolBuf&& o) noexcept {
        if (this != &o) {
            reset();
            ctx_ = o.ctx_;
            ptr_ = o.ptr_;
            o.ptr_ = nullptr;
        }
        return *this;
    }
    ~KzPoolBuf() { reset(); }

    // releases what the owner held, then takes a buffer of at least `bytes` from the pool (null when that fails)
    int alloc(kz_ctx* ctx, size_t bytes) {
        reset();
        ctx_ = ctx;
        void* p = nullptr;
        const int rc = kz_pool_alloc(ctx, bytes, &p);
        ptr_ = static_cast<T*>(p);
        return rc;
    }
    T* get() const { return ptr_; }
    void reset() {
        if (ptr_) kz_pool_free(ctx_, ptr_, 0);
        ptr_ = nullptr;
    }

private:
    kz_ctx* ctx_ = nullptr;
    T* ptr_ = nullptr;
};
