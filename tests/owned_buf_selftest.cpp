// owned_buf_selftest.cpp -- the buffer owners of gnss-sdr-1_amd/csrc/gc_internal.h (gc_owned_buf with reserve, gc_mapped_buf) on the
// host, with a stub memory policy in place of the HIP runtime: malloc / free behind a counter that makes the k-th call (allocation
// or device mapping) fail.  Handles shaped like the tracking host's (gc_tracking.hip, trk_closed_loop.hip) are created with every k
// their create path can reach: whatever was allocated before the failure is freed with the handle, nothing twice, nothing leaked;
// a reserve that fails leaves its buffer empty with capacity 0.  Built with -fsanitize=address,undefined by tests/test_owned_buf.py:
// a leak, a double free or a use after free ends the run.  Prints "ok <number of checks>".
#include "gc_internal.h"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

static int g_calls = 0, g_fail_at = 0, g_checks = 0;
static size_t g_live_at_alloc = 0;  // buffers alive when the last allocation was asked for
static std::set<void*> g_live;

#define CHECK(cond)                                                         \
    do                                                                      \
        {                                                                   \
            g_checks++;                                                     \
            if (!(cond))                                                    \
                {                                                           \
                    std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); \
                    std::exit(1);                                           \
                }                                                           \
        }                                                                   \
    while (0)

struct StubMem
{
    static bool fails() { return ++g_calls == g_fail_at; }
    static hipError_t alloc(void** p, size_t bytes)
    {
        g_live_at_alloc = g_live.size();
        if (fails()) return hipErrorOutOfMemory;
        *p = std::malloc(bytes ? bytes : 1);
        g_live.insert(*p);
        return hipSuccess;
    }
    static hipError_t zero(void* p, size_t bytes) { return std::memset(p, 0, bytes), hipSuccess; }
    static void release(void* p)
    {
        if (!p) return;
        CHECK(g_live.erase(p) == 1);
        std::free(p);
    }
    static hipError_t device_view(void** dv, void* p)
    {
        if (fails()) return hipErrorInvalidValue;
        *dv = static_cast<char*>(p) + 64;  // anything that is not the host pointer (never dereferenced)
        return hipSuccess;
    }
};
template <typename T>
using Buf = gc_owned_buf<T, StubMem>;
template <typename T>
using Mapped = gc_mapped_buf<T, StubMem>;

static void arm(int k)
{
    g_calls = 0;
    g_fail_at = k;
}

// gc_trk_batch: two tables at create, three buffers that grow with the launches
struct Batch
{
    Buf<int> d_chans;
    Buf<float> d_codes, d_partial, d_params, d_out;
    bool create() { return d_chans.alloc(4) == hipSuccess && d_codes.alloc(4 * 1023, true) == hipSuccess; }
    bool run(size_t n) { return d_params.reserve(n) == hipSuccess && d_out.reserve(3 * n) == hipSuccess && d_partial.reserve(6 * n) == hipSuccess; }
};

// gc_correlator's init(): the mapping of the window may fail without an error (the copy path needs no device view)
struct Correlator
{
    Buf<float> d_sig, d_code, d_stage, d_out, d_partial;
    Mapped<float> h_stage, h_out;
    Mapped<char> h_sig;
    bool zero_copy = true;
    bool init()
    {
        if (d_sig.alloc(1002) != hipSuccess || d_stage.alloc(1) != hipSuccess || d_out.alloc(8) != hipSuccess || d_partial.alloc(512) != hipSuccess ||
            h_stage.alloc_host(1) != hipSuccess || h_out.alloc_host(8) != hipSuccess)
            return false;
        hipError_t e = h_sig.alloc(8016);
        if (e == hipSuccess) e = h_stage.map();
        if (e == hipSuccess) e = h_out.map();
        zero_copy = e == hipSuccess;
        return true;
    }
};

// a lane of the level-1 batcher and the closed loop's engine: arrays of owners
struct Lane
{
    Mapped<int> h_chans, h_params;
    Mapped<char> h_out, h_span;
    Buf<float> d_partial;
    Buf<char> d_span;
    bool init() { return h_chans.alloc(256) == hipSuccess && h_params.alloc(256) == hipSuccess && h_out.alloc(256 * 64) == hipSuccess && d_partial.alloc(1024) == hipSuccess; }
};
struct Loop
{
    Buf<int> d_chans;
    Buf<float> d_codes, d_data_codes, d_recs;
    struct Slot
    {
        Buf<unsigned long long> d, h;
    } limits[8];
    bool create()
    {
        bool ok = d_chans.alloc(4, true) == hipSuccess && d_codes.alloc(4 * 1023) == hipSuccess;
        for (Slot& s : limits) ok = ok && s.d.alloc(4) == hipSuccess && s.h.alloc(4) == hipSuccess;
        return ok;
    }
};

template <class H, class F>
static int every_failure(F create)
{
    int reachable = 0;
    for (int k = 1;; k++)
        {
            arm(k);
            bool ok;
            {
                H h;
                ok = create(h);
                CHECK(ok || g_calls == k);  // a create path stops at the first refusal it cannot do without
            }
            CHECK(g_live.empty());
            if (g_calls < k) return reachable;  // the path made fewer calls than k: every call has failed once
            reachable++;
            (void)ok;
        }
}

int main()
{
    CHECK(every_failure<Batch>([](Batch& b) { return b.create() && b.run(10) && b.run(5) && b.run(20); }) == 2 + 3 + 3);
    CHECK(every_failure<Lane>([](Lane& l) { return l.init() && l.d_span.reserve(1 << 20) == hipSuccess && l.h_span.reserve(4 << 20) == hipSuccess; }) == 2 + 2 + 2 + 1 + 1 + 2);
    CHECK(every_failure<Loop>([](Loop& l) { return l.create() && l.d_recs.reserve(64) == hipSuccess && l.d_data_codes.alloc(4 * 1023) == hipSuccess; }) == 2 + 16 + 2);
    // the correlator: calls 1-6 are needed; 7-10 (the window, its view, the two other views) only decide the path
    for (int k = 1; k <= 11; k++)
        {
            arm(k);
            {
                Correlator c;
                const bool ok = c.init();
                CHECK(ok == (k > 6));
                if (ok) CHECK(c.zero_copy == (k > 10));
                if (ok && !c.zero_copy) CHECK(c.h_stage.get() && c.h_out.get() && c.d_sig.get());  // what the copy path uses
                if (k == 7 || k == 8) CHECK(!c.h_sig.get() && !c.h_sig.dev && c.h_sig.cap == 0);  // memory and view, or nothing
                if (k == 9) CHECK(c.h_stage.get() && !c.h_stage.dev);
                if (ok && c.zero_copy) CHECK(c.h_sig.dev && c.h_stage.dev && c.h_out.dev && static_cast<void*>(c.h_out.dev) != c.h_out.get());
            }
            CHECK(g_live.empty());
        }
    // reserve: grows only, frees before it allocates, empty with capacity 0 when the allocation fails
    arm(0);
    {
        Buf<double> b;
        CHECK(!b.get() && b.cap == 0);
        CHECK(b.reserve(10) == hipSuccess && b.cap == 10 && g_live.size() == 1);
        double* first = b;
        first[9] = 1.0;
        CHECK(b.reserve(4) == hipSuccess && b.get() == first && b.cap == 10 && g_calls == 1);
        CHECK(b.reserve(10) == hipSuccess && b.get() == first && g_calls == 1);
        CHECK(b.reserve(11) == hipSuccess && b.cap == 11 && g_calls == 2 && g_live.size() == 1 && g_live_at_alloc == 0);
        b[10] = 2.0;
        arm(1);
        CHECK(b.reserve(12) == hipErrorOutOfMemory && !b.get() && b.cap == 0 && g_live.empty() && g_live_at_alloc == 0);
        CHECK(b.reserve(1) == hipSuccess && b.cap == 1);
        CHECK(b.alloc(3, true) == hipSuccess && b.cap == 3 && b[0] == 0.0 && b[2] == 0.0 && g_live.size() == 1);
        b.reset();
        CHECK(!b.get() && b.cap == 0 && g_live.empty());
        Mapped<int> m;
        CHECK(m.reserve(8) == hipSuccess && m.cap == 8 && m.dev && g_live.size() == 1);
        int* view = m.dev;
        CHECK(m.reserve(8) == hipSuccess && m.dev == view);
        arm(2);  // the mapping of the grown buffer fails
        CHECK(m.reserve(9) == hipErrorInvalidValue && !m.get() && !m.dev && m.cap == 0 && g_live.empty());
    }
    // moves carry the memory, the capacity and the view; the source is left empty; what the target held is freed
    arm(0);
    {
        Mapped<int> a, b;
        CHECK(a.alloc(5) == hipSuccess && b.alloc(7) == hipSuccess && g_live.size() == 2);
        int* pa = a;
        int* va = a.dev;
        b = std::move(a);
        CHECK(b.get() == pa && b.dev == va && b.cap == 5 && !a.get() && !a.dev && a.cap == 0 && g_live.size() == 1);
        Mapped<int> c(std::move(b));
        CHECK(c.get() == pa && c.dev == va && c.cap == 5 && !b.get() && !b.dev && b.cap == 0);
        Lane l;
        CHECK(l.init());
        l = Lane();  // how a lane and a correlator drop what they hold
        CHECK(!l.h_chans.get() && !l.h_chans.dev && g_live.size() == 1);
    }
    CHECK(g_live.empty());
    std::printf("ok %d\n", g_checks);
    return 0;
}
