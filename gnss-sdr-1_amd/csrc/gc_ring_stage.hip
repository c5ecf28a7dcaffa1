// gc_ring_stage.hip -- the host side shared by the stages that write an RF ring on the device (gc_ring_stage.h).
#include "gc_ring_stage.h"
#include <algorithm>
#include <cmath>

unsigned gc_ring_stage_claim(gc_stream* out)
{
    std::lock_guard<std::mutex> no_push(out->push_mtx);
    std::lock_guard<std::mutex> lk(out->mtx);
    const unsigned why = (out->kernel_fed ? GC_RING_HAS_PRODUCER : 0u) | (out->head != 0 ? GC_RING_HAS_SAMPLES : 0u);
    if (why == 0) out->kernel_fed = true;
    return why;
}

void gc_ring_stage_release(gc_stream* out)
{
    (void)hipStreamSynchronize(out->copy_stream);
    {
        std::lock_guard<std::mutex> lk(out->mtx);
        out->kernel_fed = false;
    }
    gc_stream_drop(out);
}

CondStoreDst gc_ring_stage_piece(const gc_stream* s, uint64_t pos, uint64_t len, float scale, unsigned long long* clipped)
{
    CondStoreDst p;
    p.dst = s->d_ring + pos * s->elem;
    p.mirror_dst = s->d_ring + (s->capacity + pos) * s->elem;
    p.n_mirror = pos < s->mirror ? (unsigned)std::min<uint64_t>(len, s->mirror - pos) : 0u;
    p.scale = scale;
    p.clipped = clipped;
    return p;
}

hipError_t gc_quantised_output_alloc(gc_quantised_output* q, const gc_stream* out)
{
    if (out->iq_format == GC_IQ_F32) return hipSuccess;
    const hipError_t e = hipMalloc(&q->d_clipped, sizeof(unsigned long long));
    return e != hipSuccess ? e : hipMemset(q->d_clipped, 0, sizeof(unsigned long long));
}

void gc_quantised_output_free(gc_quantised_output* q)
{
    (void)hipFree(q->d_clipped);
    q->d_clipped = nullptr;
}

gc_status gc_quantised_output_check_scale(const char* who, float scale, const gc_stream* out)
{
    GC_REQUIRE(std::isfinite(scale) && scale > 0.0f, "%s: scale %g is not finite and positive", who, (double)scale);
    GC_REQUIRE(out, "%s: NULL handle", who);
    GC_REQUIRE(out->iq_format != GC_IQ_F32, "%s: a GC_IQ_F32 output ring has no scale", who);
    return GC_OK;
}

gc_status gc_quantised_output_info(const gc_quantised_output* q, gc_ctx* ctx, gc_stream* out, int32_t* out_format, float* scale, uint64_t* clipped_components)
{
    unsigned long long n = 0;
    if (q->d_clipped && clipped_components)
        {
            gc_device_guard g(ctx->device);
            GC_HIP(hipStreamSynchronize(out->copy_stream));
            GC_HIP(hipMemcpy(&n, q->d_clipped, sizeof n, hipMemcpyDeviceToHost));
        }
    if (out_format) *out_format = out->iq_format;
    if (scale) *scale = q->d_clipped ? q->scale : 1.0f;
    if (clipped_components) *clipped_components = n;
    return GC_OK;
}

gc_status gc_derived_ring_check(const char* who, const gc_ctx* ctx, const gc_stream* src, const gc_stream* out, const void* handle_out)
{
    GC_REQUIRE(ctx && src && out && handle_out, "%s: NULL argument", who);
    GC_REQUIRE(src != out, "%s: the source ring and the output ring are the same ring", who);
    GC_REQUIRE(src->ctx == ctx && out->ctx == ctx, "%s: a ring belongs to another context", who);
    return GC_OK;
}

gc_status gc_derived_ring_open(const char* who, gc_derived_ring* r, gc_ctx* ctx, gc_stream* src, gc_stream* out, const gc_derived_writer* index_rule,
    uint64_t history)
{
    uint64_t origin = 0;
    {
        std::lock_guard<std::mutex> lk(src->mtx);
        origin = src->origin;
        if (origin != 0 && !index_rule)
            return gc_fail(GC_ERR_STATE, "%s: the source ring starts at origin %llu: this stage reads a source that starts at sample 0 only", who,
                (unsigned long long)origin);
        if (origin == 0 && gc_stream_oldest(src) != 0)
            return gc_fail(GC_ERR_STATE, "%s: the source ring no longer holds sample 0 (its oldest sample is %llu)", who,
                (unsigned long long)gc_stream_oldest(src));
        if (gc_stream_oldest(src) != origin)
            return gc_fail(GC_ERR_STATE, "%s: the source ring no longer holds its origin, sample %llu (its oldest sample is %llu)", who,
                (unsigned long long)origin, (unsigned long long)gc_stream_oldest(src));
        GC_REQUIRE(origin <= GC_DERIVED_MAX_SOURCE_ORIGIN, "%s: the source ring's origin %llu is above 2^55", who, (unsigned long long)origin);
    }
    // origin 0: output 0, whose window reaches in front of the stream and reads zeros there, as ever.  Any other origin: the first
    // output whose whole window lies at or above it -- as many outputs as have their newest sample below origin + history come before
    const uint64_t first_out = origin != 0 ? index_rule->available_at(origin + history) : 0;
    {
        // (claim would report the head of such a ring as samples that have been pushed)
        std::lock_guard<std::mutex> lk(out->mtx);
        if (out->origin != 0 && out->head == out->origin && !out->kernel_fed)
            return gc_fail(GC_ERR_STATE, "%s: the output ring has an origin of its own (%llu): a derived ring receives its origin from the stage", who,
                (unsigned long long)out->origin);
    }
    const unsigned why = gc_ring_stage_claim(out);
    GC_REQUIRE(!(why & GC_RING_HAS_SAMPLES), "%s: samples have been pushed into the output ring already", who);
    if (why) return gc_fail(GC_ERR_STATE, "%s: the output ring already has a producer on the device", who);
    if (first_out != 0)
        {
            std::lock_guard<std::mutex> no_push(out->push_mtx);
            std::lock_guard<std::mutex> lk(out->mtx);
            gc_stream_set_origin_locked(out, first_out);
        }
    r->out_head = first_out;
    r->ctx = ctx;
    r->ctx_ref.bind(ctx);
    r->src = src;
    r->out = out;
    gc_stream_keep(src);
    gc_stream_keep(out);
    return GC_OK;
}

void gc_derived_ring_release(gc_derived_ring* r)
{
    if (r->out) gc_ring_stage_release(r->out);
    if (r->src) gc_stream_drop(r->src);
    r->out = r->src = nullptr;
}

gc_status gc_derived_ring_update(const char* who, const char* noun, gc_derived_ring* r, gc_derived_writer& w, uint64_t* first_out, uint64_t* n_out)
{
    std::lock_guard<std::mutex> one_update(r->mtx);
    r->updated = true;
    gc_device_guard g(r->ctx->device);
    const uint64_t m0 = r->out_head;
    if (first_out) *first_out = m0;
    gc_stream_read_set reads(r->out->copy_stream);
    gc_status st = reads.add(r->src, w.floor_of(m0));
    if (st != GC_OK) return st;  // the floor is no longer resident: nothing reserved, nothing changed
    const gc_stream_ticket& t = reads.ticket(0);
    const uint64_t m1 = w.available_at(t.head);
    if (m1 <= m0)
        {
            // nothing to produce
            r->src_consumed = t.head;
            return GC_OK;
        }
    uint64_t m = m0;
    while (m < m1)
        {
            const uint64_t n = std::min<uint64_t>(m1 - m, r->out->capacity);
            uint64_t first = 0;
            st = gc_stream_produce(r->out, n, &first, w, true);
            if (st == GC_OK && first != m)
                st = gc_fail(GC_ERR_STATE, "%s: the ring's head %llu is not the %s's output %llu", who, (unsigned long long)first, noun, (unsigned long long)m);
            if (st != GC_OK) break;
            m += n;
        }
    if (m == m0) return st;
    r->out_head = m;
    r->src_consumed = t.head;
    const gc_status st_end = reads.commit();
    if (n_out) *n_out = m - m0;
    return st != GC_OK ? st : st_end;
}

gc_status gc_derived_ring_info(gc_derived_ring* r, uint64_t* src_consumed, uint64_t* out_head)
{
    std::lock_guard<std::mutex> lk(r->mtx);
    if (src_consumed) *src_consumed = r->src_consumed;
    if (out_head) *out_head = r->out_head;
    return GC_OK;
}
