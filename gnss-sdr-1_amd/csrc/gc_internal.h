// gc_internal.h -- shared internals of libgnsscorr.so (context, error handling).
#ifndef GC_INTERNAL_H
#define GC_INTERNAL_H

#include "gnsscorr.h"
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>

// Experiment switches (measured-slower kernels and their tuning variables) exist only in builds made with
// `make EXTRA=-DGNSSCORR_EXPERIMENTS`: the product library reads no tuning variable from the environment and carries none of those
// kernels.  gc_build_has_experiments() (gnsscorr.h) tells a test which build it runs on.
#include <cstdlib>
#ifdef GNSSCORR_EXPERIMENTS
static inline const char* gc_exp_env(const char* name) { return std::getenv(name); }
#else
static inline const char* gc_exp_env(const char*) { return nullptr; }
#endif

// thread-local last-error text (gc_last_error)
void gc_set_error(const char* fmt, ...);
gc_status gc_fail(gc_status st, const char* fmt, ...);

#define GC_HIP(call)                                                                          \
    do                                                                                        \
        {                                                                                     \
            hipError_t e_ = (call);                                                           \
            if (e_ != hipSuccess)                                                             \
                return gc_fail(GC_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                    __FILE__, __LINE__);                                                      \
        }                                                                                     \
    while (0)

#define GC_REQUIRE(cond, ...)                              \
    do                                                     \
        {                                                  \
            if (!(cond)) return gc_fail(GC_ERR_INVALID, __VA_ARGS__); \
        }                                                  \
    while (0)

struct gc_ctx
{
    int device = -1;
    hipStream_t stream = nullptr;
    int n_cus = 0;
    size_t lds_max = 0;
    std::mutex mtx;  // serialises entry points that share this context's scratch
    // one reference for the creator (dropped by gc_ctx_destroy) + one per live handle created on the context:
    // the stream and the struct go away with the last of them, so handles may be destroyed in any order
    std::atomic<int> refs{1};
    // level-1 epoch batcher (gc_tracking.hip), created on first use, released with the context
    std::atomic<void*> l1_batcher{nullptr};
    void (*l1_batcher_free)(void*) = nullptr;
};

void gc_ctx_retain(gc_ctx* ctx);
void gc_ctx_release(gc_ctx* ctx);

// member of every handle struct: keeps the context alive for the handle's lifetime
struct gc_ctx_ref
{
    gc_ctx* p = nullptr;
    void bind(gc_ctx* c)
    {
        p = c;
        gc_ctx_retain(c);
    }
    ~gc_ctx_ref()
    {
        if (p) gc_ctx_release(p);
    }
};

// RAII device selection for entry points (contexts may live on different GPUs)
struct gc_device_guard
{
    int prev = -1;
    bool ok = true;
    explicit gc_device_guard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~gc_device_guard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Move-only owners of hipMalloc (gc_dev_buf<T>), hipHostMalloc (gc_host_buf<T>) and page-locked, device-mapped memory with its device
// view (gc_mapped_buf<T>), as members of a handle struct: the handle's destructor frees them, so a create function that fails half
// way and a destroy function need no list of frees.  Declare the handle's gc_ctx_ref BEFORE its buffers (members are destroyed in
// reverse order: the context outlives the frees) and delete the handle under a gc_device_guard of its device.  A buffer converts to
// T*, so launch sites read as they would with a plain pointer.  The Mem policy is a template argument so that a stub can stand in for
// the HIP runtime on the CPU (tests/owned_buf_selftest.cpp).
struct gc_device_mem
{
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t zero(void* p, size_t bytes) { return hipMemset(p, 0, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};

struct gc_pinned_mem
{
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t zero(void* p, size_t bytes) { return std::memset(p, 0, bytes), hipSuccess; }
    static void release(void* p) { (void)hipHostFree(p); }
};

struct gc_mapped_mem
{
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped); }
    static hipError_t zero(void* p, size_t bytes) { return std::memset(p, 0, bytes), hipSuccess; }
    static void release(void* p) { (void)hipHostFree(p); }
    static hipError_t device_view(void** dv, void* p) { return hipHostGetDevicePointer(dv, p, 0); }
};

template <typename T, typename Mem>
struct gc_owned_buf
{
    struct Release
    {
        void operator()(T* q) const { Mem::release(q); }
    };
    std::unique_ptr<T, Release> p;
    size_t cap = 0;  // elements held
    gc_owned_buf() = default;
    gc_owned_buf(gc_owned_buf&& o) noexcept : p(std::move(o.p)), cap(o.cap) { o.cap = 0; }
    gc_owned_buf& operator=(gc_owned_buf&& o) noexcept
    {
        p = std::move(o.p);
        cap = o.cap;
        o.cap = 0;
        return *this;
    }
    // n elements, uninitialised or zero-filled (synchronously); what was held before is freed first
    hipError_t alloc(size_t n, bool zero_fill = false)
    {
        reset();
        void* q = nullptr;
        const hipError_t e = Mem::alloc(&q, n * sizeof(T));
        if (e != hipSuccess) return e;
        p.reset(static_cast<T*>(q));
        cap = n;
        return zero_fill ? Mem::zero(q, n * sizeof(T)) : hipSuccess;
    }
    // room for n elements: grows only and keeps no contents (alloc); empty, with cap 0, when the allocation fails
    hipError_t reserve(size_t n) { return n <= cap ? hipSuccess : alloc(n); }
    void reset()
    {
        p.reset();
        cap = 0;
    }
    T* get() const { return p.get(); }
    operator T*() const { return p.get(); }
};

template <typename T>
using gc_dev_buf = gc_owned_buf<T, gc_device_mem>;
template <typename T>
using gc_host_buf = gc_owned_buf<T, gc_pinned_mem>;

// page-locked memory the device reads and writes in place: host pointer (the buffer itself) + device view `dev`
template <typename T, typename Mem = gc_mapped_mem>
struct gc_mapped_buf : gc_owned_buf<T, Mem>
{
    T* dev = nullptr;
    gc_mapped_buf() = default;
    gc_mapped_buf(gc_mapped_buf&& o) noexcept : gc_owned_buf<T, Mem>(std::move(o)), dev(o.dev) { o.dev = nullptr; }
    gc_mapped_buf& operator=(gc_mapped_buf&& o) noexcept
    {
        gc_owned_buf<T, Mem>::operator=(std::move(o));
        dev = o.dev;
        o.dev = nullptr;
        return *this;
    }
    // the memory alone; map() asks for the device view later (a caller that can do without the view when mapping fails)
    hipError_t alloc_host(size_t n)
    {
        dev = nullptr;
        return gc_owned_buf<T, Mem>::alloc(n);
    }
    hipError_t map()
    {
        void* dv = nullptr;
        const hipError_t e = Mem::device_view(&dv, this->get());
        dev = e == hipSuccess ? static_cast<T*>(dv) : nullptr;
        return e;
    }
    // memory and view, or nothing
    hipError_t alloc(size_t n)
    {
        hipError_t e = alloc_host(n);
        if (e == hipSuccess && (e = map()) != hipSuccess) reset();
        return e;
    }
    hipError_t reserve(size_t n) { return n <= this->cap ? hipSuccess : alloc(n); }
    void reset()
    {
        gc_owned_buf<T, Mem>::reset();
        dev = nullptr;
    }
};

static inline hipStream_t gc_pick_stream(gc_ctx* ctx, void* stream)
{
    return stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
}

#endif
