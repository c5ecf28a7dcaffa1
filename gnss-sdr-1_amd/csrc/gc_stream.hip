// gc_stream.hip -- gc_stream_*: the IQ block of one RF stream, pushed once per GPU and shared by every
// channel / acquisition that reads that stream (all channels of a GNSS-SDR flowgraph read one stream,
// src/core/receiver/gnss_flowgraph.cc:496-499; SURVEY.md section 8b/8e "shared IQ ring per RF stream").
//
// Layout: a ring of `capacity` samples in HBM followed by a mirror of its first `max_window` samples, so
// that any window of <= max_window samples is contiguous wherever it starts: sample a lives at a % capacity
// and, when that is < max_window, also at capacity + a % capacity.  Kernels index with absolute sample
// numbers (TrkChan::ring_len), 64 bits wide and counted from the ring's origin: 0, or what gc_stream_debug_set_origin (a test's
// handle) or a derived stage gave the empty ring, which then starts as if that many samples had been pushed and evicted.  Pushes run on the stream's own HIP stream through pinned staging slots and
// overlap with compute; a push waits only for kernels that may still read the samples it evicts.
//
// The allocation, front to back:
//
//   guard | ring: capacity | mirror: max_window | slack: GC_STREAM_SLACK | guard
//
// d_ring points at the ring.  The slack is two samples behind the mirror -- one aligned pair of samples, the unit in which the
// tracking kernels fetch a window (trk_device.hpp): a margin of one such pair behind the last position a window can touch, kept
// since the first ring.  No load needs it: a window starts below capacity and holds at most max_window samples, so its last
// sample lies at or below position capacity + max_window - 2 and the aligned pair that holds it ends inside the mirror; whole
// chunks are fetched inside [0, capacity) alone and ragged ends sample by sample (load_masked), and ring_window.h reads nothing
// behind the ring's end.  No writer stores there either: the slack stays zero for the ring's life
// (tests/test_ring_contract_gpu.py compares it after every update).
// The guard bands are storage no writer and no reader has any business in: each holds at least the largest tile of any
// producer (1024 outputs), rounded up to a multiple of 4096 bytes -- so that d_ring keeps the allocation's alignment -- and is
// filled with GC_STREAM_GUARD_BYTE at creation.  gc_stream_debug_guards compares them with that byte: a store of a producer
// kernel in front of the ring or past capacity + max_window + slack shows there instead of in a neighbouring allocation.
#include "gc_stream.h"
#include <algorithm>
#include <cstring>
#include <vector>

static void stream_release(gc_stream* s)
{
    if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
    (void)hipFree(s->d_base);
    for (int i = 0; i < gc_stream::kSlots; i++)
        {
            if (s->h_slot[i]) (void)hipHostFree(s->h_slot[i]);
            if (s->slot_done[i]) (void)hipEventDestroy(s->slot_done[i]);
        }
    for (hipEvent_t e : s->reader_events)
        if (e) (void)hipEventDestroy(e);
    if (s->pushed) (void)hipEventDestroy(s->pushed);
    if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
}

void gc_stream_keep(gc_stream* s) { s->refs.fetch_add(1); }

void gc_stream_drop(gc_stream* s)
{
    if (s->refs.fetch_sub(1) != 1) return;
    gc_device_guard g(s->ctx->device);
    {
        std::unique_lock<std::mutex> lk(s->mtx);
        s->readers.drain(lk);
    }
    stream_release(s);
    delete s;
}

gc_status gc_stream_begin_read(gc_stream* s, hipStream_t compute, uint64_t min_index, gc_stream_ticket* t)
{
    std::unique_lock<std::mutex> lk(s->mtx);
    const int slot = s->readers.reserve(lk, min_index, [s]() { return gc_stream_oldest(s); });
    if (slot < 0)
        return gc_fail(GC_ERR_STATE, "the reader fell behind the stream ring: it needs sample %llu, the oldest resident sample is %llu",
            (unsigned long long)min_index, (unsigned long long)gc_stream_oldest(s));
    // the range as of the reservation (reserve() returns with the lock held): nothing at or above the floor is evicted from here on
    t->slot = slot;
    t->oldest = gc_stream_oldest(s);
    t->head = s->head;
    if (s->has_pushed)
        {
            hipError_t e = hipStreamWaitEvent(compute, s->pushed, 0);
            if (e != hipSuccess)
                {
                    s->readers.cancel(slot);
                    t->slot = -1;
                    return gc_fail(GC_ERR_HIP, "hipStreamWaitEvent failed: %s", hipGetErrorString(e));
                }
        }
    return GC_OK;
}

gc_status gc_stream_end_read(gc_stream* s, hipStream_t compute, const gc_stream_ticket& t)
{
    if (t.slot < 0) return GC_OK;
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->readers.commit(t.slot, compute)) return gc_fail(GC_ERR_HIP, "hipEventRecord failed behind a launch that reads the stream ring");
    return GC_OK;
}

void gc_stream_cancel_read(gc_stream* s, const gc_stream_ticket& t)
{
    if (t.slot < 0) return;
    std::lock_guard<std::mutex> lk(s->mtx);
    s->readers.cancel(t.slot);
}

extern "C" {

gc_status gc_stream_create(gc_ctx* ctx, int iq_format, uint64_t capacity_samples, uint32_t max_window_samples, gc_stream** out)
{
    GC_REQUIRE(ctx && out, "gc_stream_create: NULL argument");
    *out = nullptr;
    GC_REQUIRE(iq_format == GC_IQ_F32 || iq_format == GC_IQ_I16 || iq_format == GC_IQ_I8, "gc_stream_create: unknown format %d", iq_format);
    GC_REQUIRE(max_window_samples > 0 && capacity_samples >= 2ull * max_window_samples,
        "gc_stream_create: capacity must be at least twice the longest window");
    GC_REQUIRE(capacity_samples <= 0x7fffffffull, "gc_stream_create: capacity must be below 2^31 samples");
    gc_device_guard g(ctx->device);
    gc_stream* s = new gc_stream();
    s->ctx = ctx;
    s->ctx_ref.bind(ctx);
    s->iq_format = iq_format;
    s->elem = gc_iq_sample_bytes(iq_format);
    s->capacity = capacity_samples;
    s->mirror = max_window_samples;
    s->slot_bytes = (size_t)4 << 20;
    s->guard_bytes = ((size_t)GC_STREAM_GUARD_SAMPLES * s->elem + 4095u) & ~(size_t)4095u;
    const size_t storage_bytes = (size_t)gc_stream_storage_samples(s) * s->elem;
    hipError_t e = hipMalloc(&s->d_base, s->guard_bytes + storage_bytes + s->guard_bytes);
    if (e == hipSuccess)
        {
            s->d_ring = s->d_base + s->guard_bytes;
            e = hipMemset(s->d_base, GC_STREAM_GUARD_BYTE, s->guard_bytes);
        }
    if (e == hipSuccess) e = hipMemset(s->d_ring, 0, storage_bytes);
    if (e == hipSuccess) e = hipMemset(s->d_ring + storage_bytes, GC_STREAM_GUARD_BYTE, s->guard_bytes);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->pushed, hipEventDisableTiming);
    for (int i = 0; i < gc_stream::kSlots && e == hipSuccess; i++)
        {
            e = hipHostMalloc(reinterpret_cast<void**>(&s->h_slot[i]), s->slot_bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s->slot_done[i], hipEventDisableTiming);
        }
    s->reader_events.assign(8, nullptr);
    for (auto& ev : s->reader_events)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) s->readers.init(s->reader_events);
    if (e != hipSuccess)
        {
            stream_release(s);
            delete s;
            return gc_fail(GC_ERR_HIP, "gc_stream_create: %s", hipGetErrorString(e));
        }
    *out = s;
    return GC_OK;
}

gc_status gc_stream_destroy(gc_stream* s)
{
    if (!s) return GC_OK;
    gc_stream_drop(s);  // batches that read the ring keep it alive until they are destroyed or re-pointed
    return GC_OK;
}

static gc_status stream_push(gc_stream* s, const void* host_iq, uint64_t n_samples, uint64_t* first_index, bool pinned);

gc_status gc_stream_push(gc_stream* s, const void* host_iq, uint64_t n_samples, uint64_t* first_index)
{
    return stream_push(s, host_iq, n_samples, first_index, false);
}

gc_status gc_stream_push_pinned(gc_stream* s, const void* pinned_host_iq, uint64_t n_samples, uint64_t* first_index)
{
    return stream_push(s, pinned_host_iq, n_samples, first_index, true);
}

gc_status gc_stream_broadcast_pinned(gc_stream* const* rings, int n_rings, const void* pinned_host_iq, uint64_t n_samples)
{
    GC_REQUIRE(rings && n_rings > 0 && pinned_host_iq, "gc_stream_broadcast_pinned: bad argument");
    // every ring has its own copy stream (and, on another GPU, its own DMA engines and link): the copies are enqueued back to
    // back and run concurrently; nothing is exchanged between the GPUs
    for (int i = 0; i < n_rings; i++)
        {
            GC_REQUIRE(rings[i], "gc_stream_broadcast_pinned: ring %d is NULL", i);
            GC_REQUIRE(rings[i]->iq_format == rings[0]->iq_format, "gc_stream_broadcast_pinned: ring %d has another sample format", i);
            gc_status st = stream_push(rings[i], pinned_host_iq, n_samples, nullptr, true);
            if (st != GC_OK) return st;
        }
    return GC_OK;
}

}  // extern "C"

gc_status gc_stream_produce(gc_stream* s, uint64_t n_samples, uint64_t* first_index, gc_ring_writer& w, bool kernel_fed)
{
    gc_device_guard g(s->ctx->device);
    std::lock_guard<std::mutex> one_push(s->push_mtx);
    std::unique_lock<std::mutex> lk(s->mtx);
    if (s->kernel_fed != kernel_fed)
        return gc_fail(GC_ERR_STATE, kernel_fed ? "the ring has no producer on the device" : "gc_stream_push: a signal conditioner or a ring decimator writes this ring");
    if (first_index) *first_index = s->head;
    if (n_samples == 0) return GC_OK;
    const uint64_t new_head = s->head + n_samples;
    const uint64_t new_oldest = new_head > s->capacity ? new_head - s->capacity : 0;
    // Launches that may still read samples this push evicts must finish first -- including launches whose reader slot is
    // reserved but which have not been enqueued yet (gc_reader_table.h).  From here on new readers see the post-push range.
    // The wait is done by the calling (producer) thread, not by the copy stream: a DMA queue that has to wait for a compute
    // signal takes the runtime's slow path (measured 316 us instead of 80 us per 3.2 MB push), and blocking here is also the
    // back-pressure that keeps the producer at most one ring ahead of the consumers.
    if (new_oldest > s->evicting_below) s->evicting_below = new_oldest;
    s->readers.wait_evictable(lk, new_oldest);
    uint64_t idx = s->head, left = n_samples;
    while (left > 0)
        {
            const uint64_t pos = idx % s->capacity;
            uint64_t len = std::min<uint64_t>(left, s->capacity - pos);
            gc_status st = w.write(s, idx, pos, &len);
            if (st != GC_OK) return st;
            if (pos < s->mirror && !w.writes_mirror())
                {
                    // the part that lands in the first max_window samples is repeated behind the ring (HBM to HBM)
                    const uint64_t mlen = std::min<uint64_t>(len, s->mirror - pos);
                    GC_HIP(hipMemcpyAsync(s->d_ring + (s->capacity + pos) * s->elem, s->d_ring + pos * s->elem, (size_t)mlen * s->elem,
                        hipMemcpyDeviceToDevice, s->copy_stream));
                }
            st = w.written(s);
            if (st != GC_OK) return st;
            idx += len;
            left -= len;
        }
    GC_HIP(hipEventRecord(s->pushed, s->copy_stream));
    s->has_pushed = true;
    s->head = new_head;
    return GC_OK;
}

namespace
{
// gc_stream_push / gc_stream_push_pinned: every piece is one H2D copy, from the caller's page-locked memory or through a staging slot
struct host_copy_writer : gc_ring_writer
{
    const char* src;
    bool pinned;
    int k = -1;
    host_copy_writer(const void* host_iq, bool pinned_) : src(static_cast<const char*>(host_iq)), pinned(pinned_) {}
    gc_status write(gc_stream* s, uint64_t, uint64_t pos, uint64_t* plen) override
    {
        uint64_t len = *plen;
        k = -1;
        if (pinned)
            {
                // page-locked caller memory: DMA straight from it (the caller keeps it until gc_stream_synchronize)
                GC_HIP(hipMemcpyAsync(s->d_ring + pos * s->elem, src, (size_t)len * s->elem, hipMemcpyHostToDevice, s->copy_stream));
            }
        else
            {
                len = std::min<uint64_t>(len, s->slot_bytes / s->elem);
                k = s->next_slot;
                s->next_slot = (k + 1) % gc_stream::kSlots;
                if (s->slot_busy[k]) GC_HIP(hipEventSynchronize(s->slot_done[k]));
                std::memcpy(s->h_slot[k], src, (size_t)len * s->elem);
                GC_HIP(hipMemcpyAsync(s->d_ring + pos * s->elem, s->h_slot[k], (size_t)len * s->elem, hipMemcpyHostToDevice, s->copy_stream));
            }
        src += (size_t)len * s->elem;
        *plen = len;
        return GC_OK;
    }
    gc_status written(gc_stream* s) override
    {
        if (k >= 0)
            {
                GC_HIP(hipEventRecord(s->slot_done[k], s->copy_stream));
                s->slot_busy[k] = true;
            }
        return GC_OK;
    }
};
}  // namespace

static gc_status stream_push(gc_stream* s, const void* host_iq, uint64_t n_samples, uint64_t* first_index, bool pinned)
{
    GC_REQUIRE(s && host_iq, "gc_stream_push: NULL argument");
    GC_REQUIRE(n_samples <= s->capacity, "gc_stream_push: at most capacity = %llu samples per push", (unsigned long long)s->capacity);
    host_copy_writer w(host_iq, pinned);
    return gc_stream_produce(s, n_samples, first_index, w, false);
}

extern "C" {

gc_status gc_stream_info(gc_stream* s, uint64_t* oldest_index, uint64_t* head_index, uint64_t* capacity_samples)
{
    GC_REQUIRE(s, "gc_stream_info: NULL handle");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (oldest_index) *oldest_index = gc_stream_oldest(s);
    if (head_index) *head_index = s->head;
    if (capacity_samples) *capacity_samples = s->capacity;
    return GC_OK;
}

gc_status gc_stream_accept_quantised_output(gc_stream* s)
{
    GC_REQUIRE(s, "gc_stream_accept_quantised_output: NULL handle");
    GC_REQUIRE(s->iq_format != GC_IQ_F32, "gc_stream_accept_quantised_output: a GC_IQ_F32 ring holds outputs as they are; nothing is quantised into it");
    std::lock_guard<std::mutex> no_push(s->push_mtx);
    std::lock_guard<std::mutex> lk(s->mtx);
    if (s->kernel_fed) return gc_fail(GC_ERR_STATE, "gc_stream_accept_quantised_output: the ring already has a producer on the device");
    if (s->head != s->origin) return gc_fail(GC_ERR_STATE, "gc_stream_accept_quantised_output: samples have been pushed into the ring already");
    s->quantised_output = true;
    return GC_OK;
}

gc_status gc_stream_read(gc_stream* s, uint64_t first_index, uint64_t n_samples, void* host_out)
{
    GC_REQUIRE(s && (host_out || n_samples == 0), "gc_stream_read: NULL argument");
    gc_device_guard g(s->ctx->device);
    // no push starts while the window is copied (a push in progress has finished its bookkeeping: its samples count as resident)
    std::lock_guard<std::mutex> no_push(s->push_mtx);
    {
        std::lock_guard<std::mutex> lk(s->mtx);
        if (first_index < gc_stream_oldest(s) || first_index + n_samples > s->head || first_index + n_samples < first_index)
            return gc_fail(GC_ERR_STATE, "gc_stream_read: samples [%llu, %llu) are not resident: the ring holds [%llu, %llu)",
                (unsigned long long)first_index, (unsigned long long)(first_index + n_samples), (unsigned long long)gc_stream_oldest(s),
                (unsigned long long)s->head);
    }
    GC_HIP(hipStreamSynchronize(s->copy_stream));
    char* dst = static_cast<char*>(host_out);
    uint64_t idx = first_index, left = n_samples;
    while (left > 0)
        {
            const uint64_t pos = idx % s->capacity;
            const uint64_t len = std::min<uint64_t>(left, s->capacity - pos);
            GC_HIP(hipMemcpy(dst, s->d_ring + pos * s->elem, (size_t)len * s->elem, hipMemcpyDeviceToHost));
            dst += (size_t)len * s->elem;
            idx += len;
            left -= len;
        }
    return GC_OK;
}

gc_status gc_stream_debug_read_storage(gc_stream* s, uint64_t first_position, uint64_t n_samples, void* host_out)
{
    GC_REQUIRE(s && (host_out || n_samples == 0), "gc_stream_debug_read_storage: NULL argument");
    const uint64_t total = gc_stream_storage_samples(s);
    GC_REQUIRE(first_position <= total && n_samples <= total - first_position,
        "gc_stream_debug_read_storage: positions [%llu, +%llu) are outside the ring's storage of %llu samples (ring, mirror and slack)",
        (unsigned long long)first_position, (unsigned long long)n_samples, (unsigned long long)total);
    gc_device_guard g(s->ctx->device);
    // as gc_stream_read: no push starts while the storage is copied, and what has been enqueued has landed
    std::lock_guard<std::mutex> no_push(s->push_mtx);
    GC_HIP(hipStreamSynchronize(s->copy_stream));
    if (n_samples) GC_HIP(hipMemcpy(host_out, s->d_ring + first_position * s->elem, (size_t)n_samples * s->elem, hipMemcpyDeviceToHost));
    return GC_OK;
}

gc_status gc_stream_debug_guards(gc_stream* s, int32_t* front_intact, int32_t* back_intact)
{
    GC_REQUIRE(s && front_intact && back_intact, "gc_stream_debug_guards: NULL argument");
    gc_device_guard g(s->ctx->device);
    std::lock_guard<std::mutex> no_push(s->push_mtx);
    GC_HIP(hipStreamSynchronize(s->copy_stream));
    std::vector<unsigned char> band(s->guard_bytes);
    const char* at[2] = {s->d_base, s->d_ring + (size_t)gc_stream_storage_samples(s) * s->elem};
    int32_t* intact[2] = {front_intact, back_intact};
    for (int i = 0; i < 2; i++)
        {
            GC_HIP(hipMemcpy(band.data(), at[i], band.size(), hipMemcpyDeviceToHost));
            *intact[i] = std::all_of(band.begin(), band.end(), [](unsigned char b) { return b == GC_STREAM_GUARD_BYTE; }) ? 1 : 0;
        }
    return GC_OK;
}

gc_status gc_stream_debug_set_origin(gc_stream* s, uint64_t origin)
{
    GC_REQUIRE(s, "gc_stream_debug_set_origin: NULL handle");
    GC_REQUIRE(origin <= GC_STREAM_MAX_ORIGIN, "gc_stream_debug_set_origin: origin %llu is above 2^62", (unsigned long long)origin);
    std::lock_guard<std::mutex> no_push(s->push_mtx);
    std::lock_guard<std::mutex> lk(s->mtx);
    if (s->kernel_fed) return gc_fail(GC_ERR_STATE, "gc_stream_debug_set_origin: the ring has a producer on the device");
    if (s->origin_set) return gc_fail(GC_ERR_STATE, "gc_stream_debug_set_origin: the ring has an origin already (%llu)", (unsigned long long)s->origin);
    if (s->head != 0) return gc_fail(GC_ERR_STATE, "gc_stream_debug_set_origin: samples have been pushed into the ring already");
    gc_stream_set_origin_locked(s, origin);
    return GC_OK;
}

gc_status gc_stream_synchronize(gc_stream* s)
{
    GC_REQUIRE(s, "gc_stream_synchronize: NULL handle");
    gc_device_guard g(s->ctx->device);
    GC_HIP(hipStreamSynchronize(s->copy_stream));
    return GC_OK;
}

}  // extern "C"
