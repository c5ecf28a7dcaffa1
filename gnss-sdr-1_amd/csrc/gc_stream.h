// gc_stream.h -- HBM ring of one RF stream (internal view; C ABI in gnsscorr.h).
#ifndef GC_STREAM_H
#define GC_STREAM_H
#include "gc_internal.h"
#include "gc_read_set.h"
#include "gc_reader_table.h"
#include <vector>

struct gc_hip_event_policy
{
    typedef hipEvent_t event_t;
    typedef hipStream_t stream_t;
    static bool query(hipEvent_t e) { return hipEventQuery(e) == hipSuccess; }
    static void synchronize(hipEvent_t e) { (void)hipEventSynchronize(e); }
    static bool record(hipEvent_t e, hipStream_t st) { return hipEventRecord(e, st) == hipSuccess; }
};

// bytes of one complex sample of a gc_iq_format
static inline size_t gc_iq_sample_bytes(int iq_format) { return iq_format == GC_IQ_F32 ? 8 : iq_format == GC_IQ_I16 ? 4 : 2; }

// samples behind the mirror that belong to the ring's storage and stay zero, samples each guard band holds at least, and the
// byte the bands are filled with (gc_stream.hip has the layout and what each is for)
static const uint64_t GC_STREAM_SLACK = 2;
static const uint64_t GC_STREAM_GUARD_SAMPLES = 1024;
static const int GC_STREAM_GUARD_BYTE = 0xA5;

struct gc_stream
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    int iq_format = GC_IQ_F32;
    size_t elem = 8;         // bytes per complex sample
    uint64_t capacity = 0;   // samples in the ring
    uint64_t mirror = 0;     // samples repeated behind the ring so that a window never has to wrap
    char* d_ring = nullptr;  // (capacity + mirror + GC_STREAM_SLACK) * elem bytes inside d_base, behind the front guard band
    char* d_base = nullptr;  // the allocation (hipFree takes this): guard band, ring storage, guard band (layout: gc_stream.hip)
    size_t guard_bytes = 0;  // bytes of each guard band: a multiple of 4096
    uint64_t head = 0;       // absolute index one past the newest sample
    uint64_t origin = 0;     // absolute index of the first sample the ring ever holds: 0, or what gc_stream_set_origin_locked set
    bool origin_set = false; // an origin has been given (once, to an empty ring): by gc_stream_debug_set_origin or by a derived stage
    hipStream_t copy_stream = nullptr;
    hipEvent_t pushed = nullptr;  // completion of the newest push
    bool has_pushed = false;
    // pinned staging for pageable caller buffers
    static const int kSlots = 4;
    size_t slot_bytes = 0;
    char* h_slot[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t slot_done[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool slot_busy[kSlots] = {false, false, false, false};
    int next_slot = 0;
    // launches that read the ring: reserved before their residency check, committed behind their enqueue (gc_reader_table.h)
    gc_reader_table<gc_hip_event_policy> readers;
    std::vector<hipEvent_t> reader_events;
    uint64_t evicting_below = 0;  // a push in progress is about to overwrite everything below this index
    std::mutex mtx;
    std::mutex push_mtx;  // one push at a time (a push may release mtx while it waits for readers)
    std::atomic<int> refs{1};  // the creator's reference + one per batch channel that reads the ring
    bool quantised_output = false;  // gc_stream_accept_quantised_output: a conditioner / ring decimator may quantise into this integer ring
    bool kernel_fed = false;   // a stage on the device -- conditioner, ring decimator or ring resampler -- writes the ring: gc_stream_push is
                               // refused.  Set by gc_ring_stage_claim alone, cleared by gc_ring_stage_release (gc_ring_stage.h)
};

// Who writes the samples of a push.  gc_stream_produce does the ring's bookkeeping -- one push at a time, the wait for launches that
// still read what the push evicts, the split at the wrap point, the mirror, the `pushed` event, the head -- and asks the writer to
// enqueue, on the ring's copy stream, whatever puts each contiguous piece in place: a copy from host memory (gc_stream_push) or a
// kernel (the signal conditioner).
struct gc_ring_writer
{
    virtual ~gc_ring_writer() {}
    // samples [idx, idx + *len) go to ring position pos (no wrap inside); the writer may shorten *len (> 0)
    virtual gc_status write(gc_stream* s, uint64_t idx, uint64_t pos, uint64_t* len) = 0;
    // the piece and its mirror part have been enqueued
    virtual gc_status written(gc_stream*) { return GC_OK; }
    // true: write() stores the part that falls in the first max_window samples behind the ring as well
    virtual bool writes_mirror() const { return false; }
};
// Appends n_samples (<= capacity) through `w`; first_index (optional) receives the absolute number of the first of them.
// `kernel_fed` says which kind of producer calls: the other kind is refused with GC_ERR_STATE.
gc_status gc_stream_produce(gc_stream* s, uint64_t n_samples, uint64_t* first_index, gc_ring_writer& w, bool kernel_fed);

void gc_stream_keep(gc_stream* s);
void gc_stream_drop(gc_stream* s);

// samples of storage at d_ring: ring, mirror and slack
static inline uint64_t gc_stream_storage_samples(const gc_stream* s) { return s->capacity + s->mirror + GC_STREAM_SLACK; }

// oldest absolute index still resident (a push in progress counts as done)
static inline uint64_t gc_stream_oldest(const gc_stream* s)
{
    const uint64_t o = s->head > s->capacity ? s->head - s->capacity : 0;
    return o > s->evicting_below ? o : s->evicting_below;
}

// largest origin a ring takes: head arithmetic and index * decimation products stay far below 2^64 behind it
static const uint64_t GC_STREAM_MAX_ORIGIN = 1ull << 62;
// The ring starts at `origin` as if that many samples had been pushed and evicted: head, the oldest resident sample and the first
// push's first_index are `origin`, whose storage position is origin % capacity.  The caller holds push_mtx and mtx and has checked
// that the ring is empty (head 0), has no producer and no origin yet.
static inline void gc_stream_set_origin_locked(gc_stream* s, uint64_t origin)
{
    s->origin = origin;
    s->origin_set = true;
    s->head = origin;
    s->evicting_below = origin;
}

// A reserved read of the ring: slot of the reader table + the resident range [oldest, head) at the moment of the reservation.
struct gc_stream_ticket
{
    int slot = -1;
    uint64_t oldest = 0, head = 0;
};
static const uint64_t GC_STREAM_FLOOR_OLDEST = ~0ull;
// Call BEFORE checking residency and enqueueing a kernel that reads the ring: reserves a reader slot with floor `min_index`
// (GC_STREAM_FLOOR_OLDEST: the oldest resident sample), so that no push evicts samples at or above the floor until the launch
// registered by gc_stream_end_read has finished; makes `compute` wait for the newest push; reports the resident range, which
// stays valid for [floor, head) until end_read / cancel_read.  GC_ERR_STATE (nothing reserved) if the floor is no longer resident.
gc_status gc_stream_begin_read(gc_stream* s, hipStream_t compute, uint64_t min_index, gc_stream_ticket* t);
// The kernel(s) of the ticket have been enqueued on `compute`.
gc_status gc_stream_end_read(gc_stream* s, hipStream_t compute, const gc_stream_ticket& t);
// Nothing was enqueued after all (validation or launch failure).
void gc_stream_cancel_read(gc_stream* s, const gc_stream_ticket& t);

// The reads of one launch, cancelled on every way out that does not commit them (gc_read_set.h).
struct gc_stream_read_ops
{
    typedef gc_stream ring_t;
    typedef hipStream_t stream_t;
    typedef gc_stream_ticket ticket_t;
    static constexpr uint64_t FLOOR_OLDEST = GC_STREAM_FLOOR_OLDEST;
    static gc_status begin(gc_stream* s, hipStream_t compute, uint64_t floor, gc_stream_ticket* t) { return gc_stream_begin_read(s, compute, floor, t); }
    static gc_status end(gc_stream* s, hipStream_t compute, const gc_stream_ticket& t) { return gc_stream_end_read(s, compute, t); }
    static void cancel(gc_stream* s, const gc_stream_ticket& t) { gc_stream_cancel_read(s, t); }
    static gc_status too_many_rings(int bound) { return gc_fail(GC_ERR_INVALID, "one launch reads at most %d distinct stream rings", bound); }
};
typedef gc_read_set<gc_stream_read_ops> gc_stream_read_set;

#endif
