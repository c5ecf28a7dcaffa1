// gc_ring_stage.h -- what the stages that write an RF ring on the device share on the host (gc_conditioner.hip,
// gc_ring_decimator.hip, gc_ring_resampler.hip): the producer's claim on the output ring and its release, where a contiguous piece
// of the ring goes, the state of a quantised (GC_IQ_I16 / GC_IQ_I8) output, and the whole life cycle of a ring DERIVED from
// another ring -- the decimator and the resampler differ in their arguments, their kernel and two index functions.
//
// A derived ring's update() is a reader of the source ring and the producer of the output ring at once: it takes a read ticket
// on the source with the floor the stage names (the oldest source sample output m0 reads, m0 = the output ring's head), which
// makes the output ring's copy stream wait for the newest source push and keeps later pushes from evicting what the launch reads,
// appends through gc_stream_produce with the stage's kernel writer, and commits the ticket behind the launches.
//
// Messages keep the public function's name in front: the shared checks take it as `who`.
#ifndef GC_RING_STAGE_H
#define GC_RING_STAGE_H
#include "cond_store_epilogue.h"
#include "gc_stream.h"

// ---- the producer of a ring ----

// why a ring cannot be claimed
enum
{
    GC_RING_HAS_PRODUCER = 1,  // a stage writes it already
    GC_RING_HAS_SAMPLES = 2    // its head is not 0
};
// Takes `out` for a producer on the device (gc_stream_push is refused from here on) unless it has one or holds samples: 0 and the
// ring is claimed, or the reasons and nothing has changed.  Which reason is reported, with what status, is the caller's.
unsigned gc_ring_stage_claim(gc_stream* out);
// The claimed and kept ring of a stage that goes away: waits for what the stage enqueued, gives the ring back to gc_stream_push
// and drops the stage's reference.
void gc_ring_stage_release(gc_stream* out);

// The piece of `len` samples at ring position `pos` of `s` (no wrap inside), for a writer that stores the mirror itself.
CondStoreDst gc_ring_stage_piece(const gc_stream* s, uint64_t pos, uint64_t len, float scale, unsigned long long* clipped);

// ---- a GC_IQ_I16 / GC_IQ_I8 output ring: the factor in front of the clamp and the count of clipped components ----

struct gc_quantised_output
{
    float scale = 1.0f;
    unsigned long long* d_clipped = nullptr;  // clipped components so far (HBM); nullptr for a GC_IQ_F32 ring
};
// the counter of an integer ring, zeroed; nothing for a GC_IQ_F32 ring
hipError_t gc_quantised_output_alloc(gc_quantised_output* q, const gc_stream* out);
void gc_quantised_output_free(gc_quantised_output* q);
// The checks of <stage>_set_output_scale, the arguments first: the scale, the handle (`out`: its output ring, nullptr for a NULL
// handle), the ring's format.  "Only before the first push / update" stays with the caller, under its own lock.
gc_status gc_quantised_output_check_scale(const char* who, float scale, const gc_stream* out);
// <stage>_output_info behind the caller's handle check and lock: waits for what has been enqueued when the count is asked for.
gc_status gc_quantised_output_info(const gc_quantised_output* q, gc_ctx* ctx, gc_stream* out, int32_t* out_format, float* scale, uint64_t* clipped_components);

// ---- a ring derived from another ring ----

struct gc_derived_ring
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    gc_stream* src = nullptr;   // holds a reference
    gc_stream* out = nullptr;   // holds a reference
    uint64_t src_consumed = 0;  // source head the newest update saw
    uint64_t out_head = 0;      // outputs appended so far
    bool updated = false;       // update has been called
    std::mutex mtx;             // one update at a time
};

// The stage's kernel writer -- one launch per contiguous piece of the output ring, mirror included -- and its index functions.
struct gc_derived_writer : gc_ring_writer
{
    bool writes_mirror() const override { return true; }
    virtual uint64_t floor_of(uint64_t m0) const = 0;        // the oldest source sample output m0 and the outputs behind it read
    virtual uint64_t available_at(uint64_t head) const = 0;  // outputs that the source samples below `head` complete
};

// The create checks every derived ring shares, in two halves around the stage's own checks of the rings' formats.  Before any of
// them come the stage's own arguments, before anything that needs a device or a ring.
// NULL arguments (`handle_out`: where create returns the handle), the same ring twice, a ring of another context
gc_status gc_derived_ring_check(const char* who, const gc_ctx* ctx, const gc_stream* src, const gc_stream* out, const void* handle_out);
// a source that no longer holds its first sample, an output ring that is not empty or has a producer; then `r` is bound: it keeps
// the context and both rings and is the output ring's producer until gc_derived_ring_release.
// A source with an origin other than 0 (gc_stream_debug_set_origin, or the output ring of such a stage) is taken only by a stage
// that passes its `index_rule` (nullptr: GC_ERR_STATE, the message names the origin) and only while nothing has been evicted
// since the origin.  The stage's first output is then the first m whose whole window -- `history` source samples in front of its
// newest one -- lies at or above the origin, index_rule->available_at(origin + history); the output ring receives that m as ITS
// origin and r->out_head starts there, so nothing in front of the source's origin is ever read.
static const uint64_t GC_DERIVED_MAX_SOURCE_ORIGIN = 1ull << 55;  // times the largest rate ratio (64) it stays below GC_STREAM_MAX_ORIGIN
gc_status gc_derived_ring_open(const char* who, gc_derived_ring* r, gc_ctx* ctx, gc_stream* src, gc_stream* out, const gc_derived_writer* index_rule = nullptr,
    uint64_t history = 0);
// after a failed gc_derived_ring_open as well; the stage frees what its kernels read AFTER it (it waits for them)
void gc_derived_ring_release(gc_derived_ring* r);
// <stage>_update behind the handle check.  who: the public function; noun: "decimator", "resampler".  More outputs than the ring
// holds are appended in order in several pieces (the older ones are evicted again, as by any producer).  When a piece fails
// after others were enqueued, those stay: the heads move, the ticket is committed behind them and the first error is returned.
gc_status gc_derived_ring_update(const char* who, const char* noun, gc_derived_ring* r, gc_derived_writer& w, uint64_t* first_out, uint64_t* n_out);
// <stage>_info behind the handle check
gc_status gc_derived_ring_info(gc_derived_ring* r, uint64_t* src_consumed, uint64_t* out_head);

#endif
