// gc_ring_decimator.hip -- gc_ring_decimator_*: a decimated ring derived on the device from another ring, and gc_acq_resampler_plan,
// the reference's rule for the acquisition resampler (src/core/receiver/gnss_flowgraph.cc:375-499).  The source ring is pushed once
// (or written by a gc_conditioner); tracking reads it at full rate, and update() makes a kernel (ring_decim_kernels.hip) append
// y[m] = sum_k h[k] x[mD - k] for every m the source's samples so far complete to the output ring, which acquisition searches at
// 1 / D of the rate.  Nothing crosses the host link a second time.
//
// update() is a reader of the source ring and the producer of the output ring at once: it takes a read ticket on the source with
// floor max(0, m0 D - (T - 1)) (m0 = the output ring's head), which makes the output ring's copy stream wait for the newest source
// push and keeps later pushes from evicting what the launch reads, appends through gc_stream_produce with a kernel writer, and
// commits the ticket behind the launches.  Output m is always source sample mD: the decimator starts at sample 0 of the source.
//
// The output ring may have any gc_iq_format: the kernel's store epilogue (cond_store_epilogue.h, the conditioner's) scales, clamps
// and rounds into a GC_IQ_I16 / GC_IQ_I8 ring and counts the clipped components in d_clipped.
#include "gc_stream.h"
#include "ring_decim_kernels.h"
#include <algorithm>
#include <cmath>
#include <vector>

struct gc_ring_decimator
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    gc_stream* src = nullptr;  // holds a reference
    gc_stream* out = nullptr;  // holds a reference
    uint32_t decimation = 1, n_taps = 1;
    float* d_taps = nullptr;
    uint64_t src_consumed = 0;  // source head the newest update saw
    uint64_t out_head = 0;      // outputs appended so far
    bool updated = false;       // gc_ring_decimator_update has been called: the output scale is fixed
    float out_scale = 1.0f;     // GC_IQ_I16 / GC_IQ_I8 output rings
    unsigned long long* d_clipped = nullptr;  // clipped components so far; nullptr for a GC_IQ_F32 ring
    std::mutex mtx;             // one update at a time
};

namespace
{
// one launch per contiguous piece of the output ring
struct rdec_writer : gc_ring_writer
{
    gc_ring_decimator* d;
    explicit rdec_writer(gc_ring_decimator* d_) : d(d_) {}
    bool writes_mirror() const override { return true; }
    gc_status write(gc_stream* s, uint64_t idx, uint64_t pos, uint64_t* len) override
    {
        RingDecimJob job;
        job.src = d->src->d_ring;
        job.src_cap = (unsigned)d->src->capacity;
        job.taps = d->d_taps;
        job.n_taps = (int)d->n_taps;
        job.decimation = (int)d->decimation;
        job.first_out = idx;
        job.n_out = (unsigned)*len;
        job.dst = s->d_ring + pos * s->elem;
        job.mirror_dst = s->d_ring + (s->capacity + pos) * s->elem;
        job.n_mirror = pos < s->mirror ? (unsigned)std::min<uint64_t>(*len, s->mirror - pos) : 0u;
        job.out_scale = d->out_scale;
        job.clipped = d->d_clipped;
        const int tile = ring_decim_tile_outputs(job.decimation, job.n_taps, job.n_out, std::max(1, d->ctx->n_cus));
        GC_HIP(ring_decim_launch(d->src->iq_format, s->iq_format, s->copy_stream, job, tile));
        return GC_OK;
    }
};

void rdec_release(gc_ring_decimator* d)
{
    if (d->out)
        {
            (void)hipStreamSynchronize(d->out->copy_stream);
            std::lock_guard<std::mutex> lk(d->out->mtx);
            d->out->kernel_fed = false;
        }
    (void)hipFree(d->d_taps);
    (void)hipFree(d->d_clipped);
    if (d->out) gc_stream_drop(d->out);
    if (d->src) gc_stream_drop(d->src);
}

// taps of the reference's low-pass for `decimation`; 0 when the design fails
int plan_taps(int64_t fs_in, uint32_t decimation)
{
    const double rfs = (double)fs_in / (double)decimation;
    int n = 0;
    if (gc_fir_low_pass(1.0, (double)fs_in, rfs / 2.1, rfs / 10.0, nullptr, 0, &n) != GC_OK) return 0;
    return n;
}
}  // namespace

extern "C" {

gc_status gc_ring_decimator_create(gc_ctx* ctx, gc_stream* src_ring, uint32_t decimation, const float* taps, uint32_t n_taps, gc_stream* out_ring,
    gc_ring_decimator** out)
{
    if (out) *out = nullptr;
    // the arguments first, before anything that needs a device
    GC_REQUIRE(taps, "gc_ring_decimator_create: NULL taps");
    GC_REQUIRE(decimation >= 1 && decimation <= GC_COND_MAX_DECIMATION, "gc_ring_decimator_create: decimation %u is outside 1..%d", decimation,
        GC_COND_MAX_DECIMATION);
    GC_REQUIRE(n_taps >= 1 && n_taps <= GC_COND_MAX_TAPS, "gc_ring_decimator_create: %u taps, outside 1..%d", n_taps, GC_COND_MAX_TAPS);
    for (uint32_t k = 0; k < n_taps; k++) GC_REQUIRE(std::isfinite(taps[k]), "gc_ring_decimator_create: tap %u is not finite", k);
    GC_REQUIRE(ctx && src_ring && out_ring && out, "gc_ring_decimator_create: NULL argument");
    GC_REQUIRE(src_ring != out_ring, "gc_ring_decimator_create: the source ring and the output ring are the same ring");
    GC_REQUIRE(src_ring->ctx == ctx && out_ring->ctx == ctx, "gc_ring_decimator_create: a ring belongs to another context");
    GC_REQUIRE(out_ring->iq_format == GC_IQ_F32 || out_ring->quantised_output,
        "gc_ring_decimator_create: the output ring must be GC_IQ_F32, or an integer ring opened with gc_stream_accept_quantised_output");
    {
        std::lock_guard<std::mutex> lk(src_ring->mtx);
        if (gc_stream_oldest(src_ring) != 0)
            return gc_fail(GC_ERR_STATE, "gc_ring_decimator_create: the source ring no longer holds sample 0 (its oldest sample is %llu)",
                (unsigned long long)gc_stream_oldest(src_ring));
    }
    {
        std::lock_guard<std::mutex> no_push(out_ring->push_mtx);
        std::lock_guard<std::mutex> lk(out_ring->mtx);
        GC_REQUIRE(out_ring->head == 0, "gc_ring_decimator_create: samples have been pushed into the output ring already");
        if (out_ring->kernel_fed) return gc_fail(GC_ERR_STATE, "gc_ring_decimator_create: the output ring already has a producer on the device");
        out_ring->kernel_fed = true;
    }
    gc_device_guard g(ctx->device);
    gc_ring_decimator* d = new gc_ring_decimator();
    d->ctx = ctx;
    d->ctx_ref.bind(ctx);
    d->src = src_ring;
    d->out = out_ring;
    gc_stream_keep(src_ring);
    gc_stream_keep(out_ring);
    d->decimation = decimation;
    d->n_taps = n_taps;
    hipError_t e = hipMalloc(&d->d_taps, sizeof(float) * n_taps);
    if (e == hipSuccess) e = hipMemcpy(d->d_taps, taps, sizeof(float) * n_taps, hipMemcpyHostToDevice);
    if (e == hipSuccess && out_ring->iq_format != GC_IQ_F32) e = hipMalloc(&d->d_clipped, sizeof(unsigned long long));
    if (e == hipSuccess && d->d_clipped) e = hipMemset(d->d_clipped, 0, sizeof(unsigned long long));
    if (e != hipSuccess)
        {
            rdec_release(d);
            delete d;
            return gc_fail(GC_ERR_HIP, "gc_ring_decimator_create: %s", hipGetErrorString(e));
        }
    *out = d;
    return GC_OK;
}

gc_status gc_ring_decimator_destroy(gc_ring_decimator* d)
{
    if (!d) return GC_OK;
    gc_device_guard g(d->ctx->device);
    rdec_release(d);
    delete d;
    return GC_OK;
}

gc_status gc_ring_decimator_update(gc_ring_decimator* d, uint64_t* first_out, uint64_t* n_out)
{
    if (first_out) *first_out = 0;
    if (n_out) *n_out = 0;
    GC_REQUIRE(d, "gc_ring_decimator_update: NULL handle");
    std::lock_guard<std::mutex> one_update(d->mtx);
    d->updated = true;
    gc_device_guard g(d->ctx->device);
    const uint64_t D = d->decimation, T = d->n_taps;
    const uint64_t m0 = d->out_head;
    if (first_out) *first_out = m0;
    const uint64_t floor = m0 * D >= T - 1 ? m0 * D - (T - 1) : 0;
    gc_stream_read_set reads(d->out->copy_stream);
    gc_status st = reads.add(d->src, floor);
    if (st != GC_OK) return st;  // the floor is no longer resident: nothing reserved, nothing changed
    const gc_stream_ticket& t = reads.ticket(0);
    const uint64_t m1 = (t.head + D - 1) / D;
    if (m1 <= m0)
        {
            // nothing to produce
            d->src_consumed = t.head;
            return GC_OK;
        }
    // more than the output ring holds: in order, in several pieces (the older ones are evicted again, as by any producer)
    uint64_t m = m0;
    while (m < m1)
        {
            const uint64_t n = std::min<uint64_t>(m1 - m, d->out->capacity);
            rdec_writer w(d);
            uint64_t first = 0;
            st = gc_stream_produce(d->out, n, &first, w, true);
            if (st == GC_OK && first != m)
                st = gc_fail(GC_ERR_STATE, "gc_ring_decimator_update: the ring's head %llu is not the decimator's output %llu", (unsigned long long)first,
                    (unsigned long long)m);
            if (st != GC_OK) break;
            m += n;
        }
    if (m == m0) return st;
    d->out_head = m;
    d->src_consumed = t.head;
    const gc_status st_end = reads.commit();
    if (n_out) *n_out = m - m0;
    return st != GC_OK ? st : st_end;
}

gc_status gc_ring_decimator_set_output_scale(gc_ring_decimator* d, float scale)
{
    // the arguments first, before anything that needs a device
    GC_REQUIRE(std::isfinite(scale) && scale > 0.0f, "gc_ring_decimator_set_output_scale: scale %g is not finite and positive", (double)scale);
    GC_REQUIRE(d, "gc_ring_decimator_set_output_scale: NULL handle");
    GC_REQUIRE(d->out->iq_format != GC_IQ_F32, "gc_ring_decimator_set_output_scale: a GC_IQ_F32 output ring has no scale");
    std::lock_guard<std::mutex> one_update(d->mtx);
    if (d->updated) return gc_fail(GC_ERR_STATE, "gc_ring_decimator_set_output_scale: the decimator has been updated already");
    d->out_scale = scale;
    return GC_OK;
}

gc_status gc_ring_decimator_output_info(gc_ring_decimator* d, int32_t* out_format, float* scale, uint64_t* clipped_components)
{
    GC_REQUIRE(d, "gc_ring_decimator_output_info: NULL handle");
    std::lock_guard<std::mutex> one_update(d->mtx);
    unsigned long long n = 0;
    if (d->d_clipped && clipped_components)
        {
            gc_device_guard g(d->ctx->device);
            GC_HIP(hipStreamSynchronize(d->out->copy_stream));
            GC_HIP(hipMemcpy(&n, d->d_clipped, sizeof n, hipMemcpyDeviceToHost));
        }
    if (out_format) *out_format = d->out->iq_format;
    if (scale) *scale = d->d_clipped ? d->out_scale : 1.0f;
    if (clipped_components) *clipped_components = n;
    return GC_OK;
}

gc_status gc_ring_decimator_info(gc_ring_decimator* d, uint64_t* src_consumed, uint64_t* out_head)
{
    GC_REQUIRE(d, "gc_ring_decimator_info: NULL handle");
    std::lock_guard<std::mutex> lk(d->mtx);
    if (src_consumed) *src_consumed = d->src_consumed;
    if (out_head) *out_head = d->out_head;
    return GC_OK;
}

gc_status gc_acq_resampler_plan(int64_t fs_in, uint32_t opt_acq_fs_hz, uint32_t* decimation, int64_t* resampled_fs, float* taps, int capacity, int* n_taps,
    uint32_t* latency_samples)
{
    if (decimation) *decimation = 1;
    if (resampled_fs) *resampled_fs = fs_in;
    if (n_taps) *n_taps = 0;
    if (latency_samples) *latency_samples = 0;
    GC_REQUIRE(fs_in > 0 && opt_acq_fs_hz > 0, "gc_acq_resampler_plan: the rates must be positive");
    // "Disabled acquisition resampler because the input sampling frequency is too low"
    if ((int64_t)opt_acq_fs_hz >= fs_in) return GC_OK;
    // the reference's rule: the largest divisor of fs_in that is not above floor(fs_in / opt) ... and this library's: on to the
    // next divisor while the kernel's limits (D <= 64, T <= 1024) are exceeded.  Together: the largest divisor that is not above
    // min(floor(fs_in / opt), 64) and whose filter fits -- one loop of at most 63 steps whatever the ratio of the rates
    int64_t dec = std::min<int64_t>(fs_in / (int64_t)opt_acq_fs_hz, GC_COND_MAX_DECIMATION);
    int T = 0;
    while (dec > 1)
        {
            if (fs_in % dec == 0 && dec <= GC_COND_MAX_DECIMATION)
                {
                    T = plan_taps(fs_in, (uint32_t)dec);
                    if (T >= 1 && T <= GC_COND_MAX_TAPS) break;
                }
            dec--;
        }
    if (dec <= 1) return GC_OK;
    const int64_t rfs = fs_in / dec;
    if (decimation) *decimation = (uint32_t)dec;
    if (resampled_fs) *resampled_fs = rfs;
    if (n_taps) *n_taps = T;
    if (latency_samples) *latency_samples = (uint32_t)((T - 1) / 2);
    if (!taps) return GC_OK;  // sizes alone
    GC_REQUIRE(T <= capacity, "gc_acq_resampler_plan: %d taps do not fit in %d", T, capacity);
    int n = 0;
    const double r = (double)fs_in / (double)dec;  // the reference's acq_fs: fs / decimation in double
    return gc_fir_low_pass(1.0, (double)fs_in, r / 2.1, r / 10.0, taps, capacity, &n);
}

}  // extern "C"
