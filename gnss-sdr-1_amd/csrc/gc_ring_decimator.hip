// gc_ring_decimator.hip -- gc_ring_decimator_*: a decimated ring derived on the device from another ring.  The source ring is
// pushed once (or written by a gc_conditioner); tracking reads it at full rate, and update() makes a kernel (ring_decim_kernels.hip)
// append y[m] = sum_k h[k] x[mD - k] for every m the source's samples so far complete to the output ring, which acquisition searches
// at 1 / D of the rate.  Nothing crosses the host link a second time.
//
// The life cycle is the derived ring's (gc_ring_stage.h); the decimator's own are its arguments, its writer and its index
// functions: output m is always source sample mD and reads back to max(0, mD - (T - 1)) -- on a source at origin 0 the decimator
// starts at output 0, whose window reaches in front of the stream; on a source with another origin at the first output whose whole
// window lies at or above it (gc_derived_ring_open).  The taps of the reference's acquisition resampler come from gc_acq_resampler_plan (gc_numerics.cpp).
//
// The output ring may have any gc_iq_format: the kernel's store epilogue (cond_store_epilogue.h, the conditioner's) scales, clamps
// and rounds into a GC_IQ_I16 / GC_IQ_I8 ring and counts the clipped components.
#include "gc_ring_stage.h"
#include "ring_decim_kernels.h"
#include <algorithm>
#include <cmath>

struct gc_ring_decimator
{
    gc_derived_ring ring;
    uint32_t decimation = 1, n_taps = 1;
    float* d_taps = nullptr;
    gc_quantised_output quant;  // the scale is fixed by the first update
};

namespace
{
struct rdec_writer : gc_derived_writer
{
    gc_ring_decimator* d;
    explicit rdec_writer(gc_ring_decimator* d_) : d(d_) {}
    uint64_t floor_of(uint64_t m0) const override { return m0 * d->decimation >= d->n_taps - 1 ? m0 * d->decimation - (d->n_taps - 1) : 0; }
    uint64_t available_at(uint64_t head) const override { return (head + d->decimation - 1) / d->decimation; }
    gc_status write(gc_stream* s, uint64_t idx, uint64_t pos, uint64_t* len) override
    {
        RingDecimJob job;
        job.src = d->ring.src->d_ring;
        job.src_cap = (unsigned)d->ring.src->capacity;
        job.taps = d->d_taps;
        job.n_taps = (int)d->n_taps;
        job.decimation = (int)d->decimation;
        job.first_out = idx;
        job.n_out = (unsigned)*len;
        job.out = gc_ring_stage_piece(s, pos, *len, d->quant.scale, d->quant.d_clipped);
        const int tile = ring_decim_tile_outputs(job.decimation, job.n_taps, job.n_out, std::max(1, d->ring.ctx->n_cus));
        GC_HIP(ring_decim_launch(d->ring.src->iq_format, s->iq_format, s->copy_stream, job, tile));
        return GC_OK;
    }
};

void rdec_release(gc_ring_decimator* d)
{
    gc_derived_ring_release(&d->ring);
    (void)hipFree(d->d_taps);
    gc_quantised_output_free(&d->quant);
    delete d;
}
}  // namespace

extern "C" {

gc_status gc_ring_decimator_create(gc_ctx* ctx, gc_stream* src_ring, uint32_t decimation, const float* taps, uint32_t n_taps, gc_stream* out_ring,
    gc_ring_decimator** out)
{
    static const char who[] = "gc_ring_decimator_create";
    if (out) *out = nullptr;
    // the arguments first, before anything that needs a device
    GC_REQUIRE(taps, "gc_ring_decimator_create: NULL taps");
    GC_REQUIRE(decimation >= 1 && decimation <= GC_COND_MAX_DECIMATION, "gc_ring_decimator_create: decimation %u is outside 1..%d", decimation,
        GC_COND_MAX_DECIMATION);
    GC_REQUIRE(n_taps >= 1 && n_taps <= GC_COND_MAX_TAPS, "gc_ring_decimator_create: %u taps, outside 1..%d", n_taps, GC_COND_MAX_TAPS);
    for (uint32_t k = 0; k < n_taps; k++) GC_REQUIRE(std::isfinite(taps[k]), "gc_ring_decimator_create: tap %u is not finite", k);
    gc_status st = gc_derived_ring_check(who, ctx, src_ring, out_ring, out);
    if (st != GC_OK) return st;
    GC_REQUIRE(out_ring->iq_format == GC_IQ_F32 || out_ring->quantised_output,
        "gc_ring_decimator_create: the output ring must be GC_IQ_F32, or an integer ring opened with gc_stream_accept_quantised_output");
    gc_ring_decimator* d = new gc_ring_decimator();
    d->decimation = decimation;
    d->n_taps = n_taps;
    const rdec_writer index_rule(d);
    st = gc_derived_ring_open(who, &d->ring, ctx, src_ring, out_ring, &index_rule, n_taps - 1);
    if (st != GC_OK)
        {
            delete d;
            return st;
        }
    gc_device_guard g(ctx->device);
    hipError_t e = hipMalloc(&d->d_taps, sizeof(float) * n_taps);
    if (e == hipSuccess) e = hipMemcpy(d->d_taps, taps, sizeof(float) * n_taps, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = gc_quantised_output_alloc(&d->quant, out_ring);
    if (e != hipSuccess)
        {
            rdec_release(d);
            return gc_fail(GC_ERR_HIP, "gc_ring_decimator_create: %s", hipGetErrorString(e));
        }
    *out = d;
    return GC_OK;
}

gc_status gc_ring_decimator_destroy(gc_ring_decimator* d)
{
    if (!d) return GC_OK;
    gc_device_guard g(d->ring.ctx->device);
    rdec_release(d);
    return GC_OK;
}

gc_status gc_ring_decimator_update(gc_ring_decimator* d, uint64_t* first_out, uint64_t* n_out)
{
    if (first_out) *first_out = 0;
    if (n_out) *n_out = 0;
    GC_REQUIRE(d, "gc_ring_decimator_update: NULL handle");
    rdec_writer w(d);
    return gc_derived_ring_update("gc_ring_decimator_update", "decimator", &d->ring, w, first_out, n_out);
}

gc_status gc_ring_decimator_set_output_scale(gc_ring_decimator* d, float scale)
{
    const gc_status st = gc_quantised_output_check_scale("gc_ring_decimator_set_output_scale", scale, d ? d->ring.out : nullptr);
    if (st != GC_OK) return st;
    std::lock_guard<std::mutex> one_update(d->ring.mtx);
    if (d->ring.updated) return gc_fail(GC_ERR_STATE, "gc_ring_decimator_set_output_scale: the decimator has been updated already");
    d->quant.scale = scale;
    return GC_OK;
}

gc_status gc_ring_decimator_output_info(gc_ring_decimator* d, int32_t* out_format, float* scale, uint64_t* clipped_components)
{
    GC_REQUIRE(d, "gc_ring_decimator_output_info: NULL handle");
    std::lock_guard<std::mutex> one_update(d->ring.mtx);
    return gc_quantised_output_info(&d->quant, d->ring.ctx, d->ring.out, out_format, scale, clipped_components);
}

gc_status gc_ring_decimator_info(gc_ring_decimator* d, uint64_t* src_consumed, uint64_t* out_head)
{
    GC_REQUIRE(d, "gc_ring_decimator_info: NULL handle");
    return gc_derived_ring_info(&d->ring, src_consumed, out_head);
}

}  // extern "C"
