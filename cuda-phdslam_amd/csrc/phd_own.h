/*
 * phd_own.h — move-only owners of what a context holds (host units only):
 * device memory, pinned host memory, events and streams.  Each releases in its
 * destructor; alloc / ensure / create return the C-ABI's status and set the
 * last error (fail, phd_ctx.h).  They convert to the raw handle, so launches
 * and runtime calls read as with raw pointers.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>

#include "phd_capi.h"

#pragma GCC visibility push(hidden)
/* sets the calling thread's last error (phd_last_error) and returns code; phd_capi_ctx.hip */
int fail(int code, const std::string& msg);
#pragma GCC visibility pop

namespace phd {

inline int own_status(hipError_t e, const char* what) {
    return e == hipSuccess ? PHD_OK : fail(PHD_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

/* one runtime handle H, released by Free unless it is borrowed */
template <class H, hipError_t (*Free)(H)>
class Owned {
  public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.h_), own_(o.own_) { o.h_ = H(); }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset(o.h_, o.own_);
            o.h_ = H();
        }
        return *this;
    }
    ~Owned() { reset(); }
    void reset(H h = H(), bool own = true) {
        if (h_ && own_) (void)Free(h_);
        h_ = h;
        own_ = own;
    }
    H get() const { return h_; }

  protected:
    H h_ = H();
    bool own_ = true;
};

inline hipError_t free_dev(void* p) { return hipFree(p); }
inline hipError_t free_pinned(void* p) { return hipHostFree(p); }

/* elements of T from hipMalloc (DevBuf) or hipHostMalloc (PinnedBuf); bytes() is
 * what the last alloc asked for */
template <class T, hipError_t (*Free)(void*)>
class Buf : public Owned<void*, Free> {
  public:
    int alloc(size_t count, unsigned pinned_flags = hipHostMallocDefault) {
        this->reset();
        void* p = nullptr;
        const bool dev = Free == free_dev;
        const hipError_t e = dev ? hipMalloc(&p, count * sizeof(T)) : hipHostMalloc(&p, count * sizeof(T), pinned_flags);
        if (e != hipSuccess) return own_status(e, dev ? "hipMalloc" : "hipHostMalloc");
        this->reset(p);
        bytes_ = count * sizeof(T);
        return PHD_OK;
    }
    /* grow-only; the contents are lost when it grows */
    int ensure(size_t count) { return get() && count * sizeof(T) <= bytes_ ? PHD_OK : alloc(count); }
    T* get() const { return (T*)this->h_; }
    operator T*() const { return get(); }
    size_t bytes() const { return get() ? bytes_ : 0; }

  private:
    size_t bytes_ = 0;
};
template <class T>
using DevBuf = Buf<T, free_dev>;
template <class T>
using PinnedBuf = Buf<T, free_pinned>;

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    int create(unsigned flags) {
        hipEvent_t e = nullptr;
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc == hipSuccess) reset(e);
        return own_status(rc, "hipEventCreateWithFlags");
    }
    operator hipEvent_t() const { return h_; }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    /* priority: NULL for the default one */
    int create(unsigned flags, const int* priority = nullptr) {
        hipStream_t s = nullptr;
        const hipError_t rc =
            priority ? hipStreamCreateWithPriority(&s, flags, *priority) : hipStreamCreateWithFlags(&s, flags);
        if (rc == hipSuccess) reset(s);
        return own_status(rc, "hipStreamCreate");
    }
    void borrow(hipStream_t s) { reset(s, false); }  // the caller's stream: never destroyed here
    bool owned() const { return own_; }
    operator hipStream_t() const { return h_; }
};

}  // namespace phd
