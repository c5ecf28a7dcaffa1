// gc_ring_notch.hip -- gc_ring_notch_*: a ring derived on the device from another ring at the same rate with continuous-wave
// interference notched out, the reference's Notch_Filter / Notch_Filter_Lite input filters.  The life cycle is the derived ring's
// (gc_ring_stage.h), shared with the decimator and the resampler; the notch's own are its arguments, its writer and its state.
//
// An update completes whole segments, but gc_stream_produce cuts its pieces at the output ring's wrap, not at segment borders.
// The writer therefore decides, in front of a piece, every segment the piece touches that has not been decided yet -- all of
// them are complete in the source -- and leaves one record per segment in HBM (ring_notch_kernels.h); the piece, and a later
// piece that begins in the middle of the last of those segments, are written from the records.
#include "gc_ring_stage.h"
#include "ring_notch_kernels.h"
#include <algorithm>
#include <cmath>
#include <vector>

struct gc_ring_notch
{
    gc_derived_ring ring;
    NotchParams params = {};
    RingNotchWork work = {};
    uint64_t seg_enqueued = 0;  // segments whose decision has been enqueued
};

namespace
{
RingNotchJob rnotch_job(const gc_ring_notch* d)
{
    RingNotchJob job;
    job.src = d->ring.src->d_ring;
    job.src_cap = (unsigned)d->ring.src->capacity;
    job.params = d->params;
    job.work = d->work;
    return job;
}

struct rnotch_writer : gc_derived_writer
{
    gc_ring_notch* d;
    explicit rnotch_writer(gc_ring_notch* d_) : d(d_) {}
    // sample m reads x[m - 1]
    uint64_t floor_of(uint64_t m0) const override { return m0 ? m0 - 1 : 0; }
    uint64_t available_at(uint64_t head) const override { return head / d->params.length * d->params.length; }
    gc_status write(gc_stream* s, uint64_t idx, uint64_t pos, uint64_t* len) override
    {
        const uint64_t L = d->params.length;
        const RingNotchJob job = rnotch_job(d);
        const uint64_t seg_end = (idx + *len + L - 1) / L;  // complete in the source: an update ends at a segment border
        if (seg_end > d->seg_enqueued)
            {
                GC_HIP(ring_notch_decide_launch(s->copy_stream, job, d->seg_enqueued, (unsigned)(seg_end - d->seg_enqueued)));
                d->seg_enqueued = seg_end;
            }
        GC_HIP(ring_notch_apply_launch(s->copy_stream, job, idx, (unsigned)*len, gc_ring_stage_piece(s, pos, *len, 1.0f, nullptr)));
        return GC_OK;
    }
};

void rnotch_release(gc_ring_notch* d)
{
    gc_derived_ring_release(&d->ring);  // waits for the kernels that read what follows
    RingNotchWork& w = d->work;
    (void)hipFree(w.state);
    (void)hipFree(const_cast<NotchC*>(w.twiddles));
    (void)hipFree(w.energies);
    (void)hipFree(w.bits);
    (void)hipFree(w.back);
    (void)hipFree(w.z);
    (void)hipFree(w.A);
    (void)hipFree(w.B);
    (void)hipFree(w.carry);
    delete d;
}

template <class T>
hipError_t rnotch_alloc(T** p, size_t n)
{
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * n);
    return e != hipSuccess ? e : hipMemset(*p, 0, sizeof(T) * n);
}
}  // namespace

extern "C" {

size_t gc_notch_conf_size(void) { return sizeof(gc_notch_conf); }

gc_status gc_ring_notch_create(gc_ctx* ctx, gc_stream* src_ring, const gc_notch_conf* conf, gc_stream* out_ring, gc_ring_notch** out)
{
    static const char who[] = "gc_ring_notch_create";
    if (out) *out = nullptr;
    // the arguments first, before anything that needs a device
    GC_REQUIRE(conf, "gc_ring_notch_create: NULL configuration");
    GC_REQUIRE(conf->mode == GC_NOTCH_FULL || conf->mode == GC_NOTCH_LITE, "gc_ring_notch_create: unknown mode %d", (int)conf->mode);
    GC_REQUIRE(conf->noise_floor == GC_NOTCH_FLOOR_REFERENCE || conf->noise_floor == GC_NOTCH_FLOOR_LINEAR, "gc_ring_notch_create: unknown noise floor %d",
        (int)conf->noise_floor);
    GC_REQUIRE(conf->length >= 2 && conf->length <= GC_NOTCH_MAX_LENGTH, "gc_ring_notch_create: length %u is outside 2..%d", conf->length, GC_NOTCH_MAX_LENGTH);
    GC_REQUIRE(conf->p_c_factor >= 0.0f && conf->p_c_factor < 1.0f, "gc_ring_notch_create: p_c_factor %g is outside [0, 1)", (double)conf->p_c_factor);
    GC_REQUIRE(conf->pfa > 0.0f && conf->pfa < 1.0f, "gc_ring_notch_create: pfa %g is outside (0, 1)", (double)conf->pfa);
    GC_REQUIRE(conf->threshold == 0.0f || (std::isfinite(conf->threshold) && conf->threshold > 0.0f),
        "gc_ring_notch_create: threshold %g is neither 0 (from pfa and length) nor finite and positive", (double)conf->threshold);
    GC_REQUIRE(conf->segments_est >= 1, "gc_ring_notch_create: segments_est is 0");
    GC_REQUIRE(conf->segments_coeff >= 1, "gc_ring_notch_create: segments_coeff is 0");
    float threshold = conf->threshold;
    if (threshold == 0.0f)
        {
            double q = 0.0;
            const gc_status stq = gc_chi2_upper_quantile(2.0 * (double)conf->length, (double)conf->pfa, &q);
            if (stq != GC_OK) return stq;
            threshold = (float)q;
        }
    gc_status st = gc_derived_ring_check(who, ctx, src_ring, out_ring, out);
    if (st != GC_OK) return st;
    GC_REQUIRE(src_ring->iq_format == GC_IQ_F32 && out_ring->iq_format == GC_IQ_F32, "gc_ring_notch_create: the source ring and the output ring must be GC_IQ_F32");
    GC_REQUIRE(src_ring->capacity > conf->length, "gc_ring_notch_create: the source ring holds %llu samples, not more than a segment of %u",
        (unsigned long long)src_ring->capacity, conf->length);
    gc_ring_notch* d = new gc_ring_notch();
    st = gc_derived_ring_open(who, &d->ring, ctx, src_ring, out_ring);
    if (st != GC_OK)
        {
            delete d;
            return st;
        }
    gc_device_guard g(ctx->device);
    d->params.threshold = threshold;
    d->params.p = conf->p_c_factor;
    d->params.dof = (float)(2u * conf->length);
    d->params.length = conf->length;
    d->params.segments_est = conf->segments_est;
    d->params.segments_reset = conf->segments_reset;
    d->params.segments_coeff = conf->segments_coeff;
    d->params.mode = conf->mode == GC_NOTCH_LITE ? NOTCH_MODE_LITE : NOTCH_MODE_FULL;
    d->params.noise_floor = conf->noise_floor == GC_NOTCH_FLOOR_LINEAR ? NOTCH_FLOOR_LINEAR : NOTCH_FLOOR_REFERENCE;
    // a piece holds at most capacity samples: capacity / L + 2 segments touch it, one more precedes a batch
    RingNotchWork& w = d->work;
    w.records = (unsigned)(out_ring->capacity / conf->length) + 4u;
    std::vector<NotchC> tw(conf->length);
    for (uint32_t j = 0; j < conf->length; j++) tw[j] = notch_twiddle(j, conf->length);
    NotchC* d_tw = nullptr;
    hipError_t e = rnotch_alloc(&w.state, 1);
    if (e == hipSuccess) e = rnotch_alloc(&d_tw, tw.size());
    w.twiddles = d_tw;
    if (e == hipSuccess) e = hipMemcpy(d_tw, tw.data(), sizeof(NotchC) * tw.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rnotch_alloc(&w.energies, w.records);
    if (e == hipSuccess) e = rnotch_alloc(&w.bits, w.records);
    if (e == hipSuccess) e = rnotch_alloc(&w.back, w.records);
    if (e == hipSuccess) e = rnotch_alloc(&w.z, w.records);
    if (e == hipSuccess) e = rnotch_alloc(&w.A, w.records);
    if (e == hipSuccess) e = rnotch_alloc(&w.B, w.records);
    if (e == hipSuccess) e = rnotch_alloc(&w.carry, w.records);
    if (e != hipSuccess)
        {
            rnotch_release(d);
            return gc_fail(GC_ERR_HIP, "gc_ring_notch_create: %s", hipGetErrorString(e));
        }
    *out = d;
    return GC_OK;
}

gc_status gc_ring_notch_destroy(gc_ring_notch* d)
{
    if (!d) return GC_OK;
    gc_device_guard g(d->ring.ctx->device);
    rnotch_release(d);
    return GC_OK;
}

gc_status gc_ring_notch_update(gc_ring_notch* d, uint64_t* first_out, uint64_t* n_out)
{
    if (first_out) *first_out = 0;
    if (n_out) *n_out = 0;
    GC_REQUIRE(d, "gc_ring_notch_update: NULL handle");
    rnotch_writer w(d);
    return gc_derived_ring_update("gc_ring_notch_update", "notch filter", &d->ring, w, first_out, n_out);
}

gc_status gc_ring_notch_info(gc_ring_notch* d, uint64_t* src_consumed, uint64_t* out_head)
{
    GC_REQUIRE(d, "gc_ring_notch_info: NULL handle");
    return gc_derived_ring_info(&d->ring, src_consumed, out_head);
}

gc_status gc_ring_notch_state(gc_ring_notch* d, uint64_t* segments_decided, uint64_t* segments_filtered, float* noise_power, uint32_t* n_segments,
    int32_t* active, float* threshold, float* last_re_im)
{
    GC_REQUIRE(d, "gc_ring_notch_state: NULL handle");
    std::lock_guard<std::mutex> one_update(d->ring.mtx);
    gc_device_guard g(d->ring.ctx->device);
    NotchState st;
    GC_HIP(hipStreamSynchronize(d->ring.out->copy_stream));
    GC_HIP(hipMemcpy(&st, d->work.state, sizeof st, hipMemcpyDeviceToHost));
    if (segments_decided) *segments_decided = st.decided;
    if (segments_filtered) *segments_filtered = st.filtered;
    if (noise_power) *noise_power = st.noise;
    if (n_segments) *n_segments = st.n;
    if (active) *active = (int32_t)st.active;
    if (threshold) *threshold = d->params.threshold;
    if (last_re_im)
        {
            last_re_im[0] = st.last.re;
            last_re_im[1] = st.last.im;
        }
    return GC_OK;
}

}  // extern "C"
