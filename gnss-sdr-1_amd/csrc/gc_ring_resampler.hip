// gc_ring_resampler.hip -- gc_ring_resampler_*: a ring derived on the device from another ring at an ARBITRARY rate ratio, the third
// stage of the reference's signal conditioner (data_type_adapter -> input_filter -> resampler).  The life cycle is the derived
// ring's (gc_ring_stage.h), shared with gc_ring_decimator.hip; the resampler's own are its arguments, its writer and its index
// functions.  A tap bank for its polyphase mode comes from gc_resampler_design (gc_numerics.cpp).
//
// Which source sample an output is, is a closed form of the output's absolute number (resamp_index.h): the writer splits the first
// output of every contiguous piece into a 128-bit base and the kernel adds 64-bit offsets, so the result does not depend on how
// the source was pushed or how the updates were cut.
#include "gc_ring_stage.h"
#include "ring_resamp_kernels.h"
#include <algorithm>
#include <cmath>
#include <vector>

struct gc_ring_resampler
{
    gc_derived_ring ring;
    ResampRatio ratio = {RESAMP_IDENTITY, 0};
    int log2_phases = 0, taps = 1;
    float* d_bank = nullptr;  // polyphase: phases rows of ring_resamp_bank_pitch(taps) floats
};

namespace
{
struct rres_writer : gc_derived_writer
{
    gc_ring_resampler* d;
    explicit rres_writer(gc_ring_resampler* d_) : d(d_) {}
    uint64_t floor_of(uint64_t m0) const override { return resamp_floor(d->ratio, d->taps, m0); }
    uint64_t available_at(uint64_t head) const override { return resamp_available(d->ratio, head); }
    gc_status write(gc_stream* s, uint64_t idx, uint64_t pos, uint64_t* len) override
    {
        const ResampBase base = resamp_base(d->ratio, idx);
        RingResampJob job;
        job.src = d->ring.src->d_ring;
        job.src_cap = (unsigned)d->ring.src->capacity;
        job.kind = d->ratio.kind;
        job.step = d->ratio.step;
        job.q0 = base.q0;
        job.r0 = base.r0;
        job.n_out = (unsigned)*len;
        job.out = gc_ring_stage_piece(s, pos, *len, 1.0f, nullptr);
        job.bank = d->d_bank;
        job.log2_phases = d->log2_phases;
        job.taps = d->taps;
        if (d->ratio.kind != RESAMP_POLY)
            {
                GC_HIP(ring_resamp_direct_launch(d->ring.src->iq_format, s->copy_stream, job));
                return GC_OK;
            }
        const int tile = ring_resamp_tile_outputs(job.step, job.taps, 1 << job.log2_phases, job.n_out, std::max(1, d->ring.ctx->n_cus));
        GC_HIP(ring_resamp_poly_launch(d->ring.src->iq_format, s->copy_stream, job, tile));
        return GC_OK;
    }
};

void rres_release(gc_ring_resampler* d)
{
    gc_derived_ring_release(&d->ring);
    (void)hipFree(d->d_bank);
    delete d;
}

int log2_of(uint32_t v)
{
    int n = 0;
    while ((1u << n) < v) n++;
    return n;
}
}  // namespace

extern "C" {

size_t gc_resampler_conf_size(void) { return sizeof(gc_resampler_conf); }

gc_status gc_ring_resampler_create(gc_ctx* ctx, gc_stream* src_ring, const gc_resampler_conf* conf, gc_stream* out_ring, gc_ring_resampler** out)
{
    static const char who[] = "gc_ring_resampler_create";
    if (out) *out = nullptr;
    // the arguments first, before anything that needs a device
    GC_REQUIRE(conf, "gc_ring_resampler_create: NULL configuration");
    GC_REQUIRE(conf->mode == GC_RESAMP_DIRECT || conf->mode == GC_RESAMP_POLYPHASE, "gc_ring_resampler_create: unknown mode %d", (int)conf->mode);
    GC_REQUIRE(std::isfinite(conf->fs_in) && std::isfinite(conf->fs_out) && conf->fs_in > 0.0 && conf->fs_out > 0.0,
        "gc_ring_resampler_create: the rates must be finite and positive");
    const double rate_ratio = conf->fs_in / conf->fs_out;
    const bool poly = conf->mode == GC_RESAMP_POLYPHASE;
    if (!poly)
        GC_REQUIRE(rate_ratio >= 1.0 / 64.0 && rate_ratio <= 64.0, "gc_ring_resampler_create: fs_in / fs_out = %g is outside 1/64 .. 64", rate_ratio);
    else
        {
            GC_REQUIRE(rate_ratio >= 1.0 / 8.0 && rate_ratio <= 64.0, "gc_ring_resampler_create: fs_in / fs_out = %g is outside 1/8 .. 64 (polyphase mode)", rate_ratio);
            GC_REQUIRE(ring_resamp_power_of_two(conf->phases) && conf->phases <= GC_RRES_MAX_PHASES, "gc_ring_resampler_create: %u phases, not a power of two in 1..%d",
                conf->phases, GC_RRES_MAX_PHASES);
            GC_REQUIRE(conf->taps_per_phase >= 1 && conf->taps_per_phase <= GC_RRES_MAX_TAPS, "gc_ring_resampler_create: %u taps per phase, outside 1..%d",
                conf->taps_per_phase, GC_RRES_MAX_TAPS);
            GC_REQUIRE(conf->phases * conf->taps_per_phase <= GC_RRES_MAX_BANK, "gc_ring_resampler_create: a bank of %u x %u taps, more than %d", conf->phases,
                conf->taps_per_phase, GC_RRES_MAX_BANK);
            GC_REQUIRE(conf->bank, "gc_ring_resampler_create: NULL bank");
            for (uint32_t k = 0; k < conf->phases * conf->taps_per_phase; k++)
                GC_REQUIRE(std::isfinite(conf->bank[k]), "gc_ring_resampler_create: tap %u of phase %u is not finite", k % conf->taps_per_phase, k / conf->taps_per_phase);
        }
    const ResampRatio ratio = poly ? resamp_poly_ratio(conf->fs_in, conf->fs_out) : resamp_direct_ratio(conf->fs_in, conf->fs_out);
    GC_REQUIRE(ratio.kind == RESAMP_IDENTITY || ratio.step > 0, "gc_ring_resampler_create: the rate ratio rounds to a step of 0");
    if (poly)
        GC_REQUIRE(ring_resamp_tile_outputs(ratio.step, (int)conf->taps_per_phase, (int)conf->phases, 1u, 1) > 0,
            "gc_ring_resampler_create: the source window and the bank do not fit in a workgroup's LDS");
    gc_status st = gc_derived_ring_check(who, ctx, src_ring, out_ring, out);
    if (st != GC_OK) return st;
    if (poly)
        GC_REQUIRE(out_ring->iq_format == GC_IQ_F32, "gc_ring_resampler_create: polyphase mode writes a GC_IQ_F32 output ring only");
    else
        GC_REQUIRE(out_ring->iq_format == src_ring->iq_format,
            "gc_ring_resampler_create: direct mode moves samples as they are: the output ring must have the source ring's format");
    gc_ring_resampler* d = new gc_ring_resampler();
    d->ratio = ratio;
    if (poly)
        {
            d->log2_phases = log2_of(conf->phases);
            d->taps = (int)conf->taps_per_phase;
        }
    const rres_writer index_rule(d);
    st = gc_derived_ring_open(who, &d->ring, ctx, src_ring, out_ring, &index_rule, (uint64_t)(d->taps - 1));
    if (st != GC_OK)
        {
            delete d;
            return st;
        }
    gc_device_guard g(ctx->device);
    hipError_t e = hipSuccess;
    if (poly)
        {
            // rows at the pitch the kernel keeps them at in LDS
            const int pitch = ring_resamp_bank_pitch(d->taps);
            std::vector<float> rows((size_t)conf->phases * pitch, 0.0f);
            for (uint32_t p = 0; p < conf->phases; p++) std::copy(conf->bank + (size_t)p * d->taps, conf->bank + (size_t)(p + 1) * d->taps, rows.begin() + (size_t)p * pitch);
            e = hipMalloc(&d->d_bank, sizeof(float) * rows.size());
            if (e == hipSuccess) e = hipMemcpy(d->d_bank, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice);
        }
    if (e != hipSuccess)
        {
            rres_release(d);
            return gc_fail(GC_ERR_HIP, "gc_ring_resampler_create: %s", hipGetErrorString(e));
        }
    *out = d;
    return GC_OK;
}

gc_status gc_ring_resampler_destroy(gc_ring_resampler* d)
{
    if (!d) return GC_OK;
    gc_device_guard g(d->ring.ctx->device);
    rres_release(d);
    return GC_OK;
}

gc_status gc_ring_resampler_update(gc_ring_resampler* d, uint64_t* first_out, uint64_t* n_out)
{
    if (first_out) *first_out = 0;
    if (n_out) *n_out = 0;
    GC_REQUIRE(d, "gc_ring_resampler_update: NULL handle");
    rres_writer w(d);
    return gc_derived_ring_update("gc_ring_resampler_update", "resampler", &d->ring, w, first_out, n_out);
}

gc_status gc_ring_resampler_info(gc_ring_resampler* d, uint64_t* src_consumed, uint64_t* out_head)
{
    GC_REQUIRE(d, "gc_ring_resampler_info: NULL handle");
    return gc_derived_ring_info(&d->ring, src_consumed, out_head);
}

}  // extern "C"
