// gc_ring_resampler.hip -- gc_ring_resampler_*: a ring derived on the device from another ring at an ARBITRARY rate ratio, the third
// stage of the reference's signal conditioner (data_type_adapter -> input_filter -> resampler), and gc_resampler_design, a tap bank
// for its polyphase mode.  A sibling of gc_ring_decimator.hip with the same life cycle: update() is a reader of the source ring
// and the producer of the output ring at once -- a read ticket on the source with floor resamp_floor(m0) (m0 = the output ring's
// head), which makes the output ring's copy stream wait for the newest source push and keeps later pushes from evicting what the
// launch reads; gc_stream_produce with a kernel writer that stores the mirror itself; the ticket committed behind the launches.
//
// Which source sample an output is, is a closed form of the output's absolute number (resamp_index.h): the writer splits the first
// output of every contiguous piece into a 128-bit base and the kernel adds 64-bit offsets, so the result does not depend on how
// the source was pushed or how the updates were cut.
#include "gc_stream.h"
#include "ring_resamp_kernels.h"
#include <algorithm>
#include <cmath>
#include <vector>

struct gc_ring_resampler
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    gc_stream* src = nullptr;  // holds a reference
    gc_stream* out = nullptr;  // holds a reference
    ResampRatio ratio = {RESAMP_IDENTITY, 0};
    int log2_phases = 0, taps = 1;
    float* d_bank = nullptr;    // polyphase: phases rows of ring_resamp_bank_pitch(taps) floats
    uint64_t src_consumed = 0;  // source head the newest update saw
    uint64_t out_head = 0;      // outputs appended so far
    std::mutex mtx;             // one update at a time
};

namespace
{
// one launch per contiguous piece of the output ring
struct rres_writer : gc_ring_writer
{
    gc_ring_resampler* d;
    explicit rres_writer(gc_ring_resampler* d_) : d(d_) {}
    bool writes_mirror() const override { return true; }
    gc_status write(gc_stream* s, uint64_t idx, uint64_t pos, uint64_t* len) override
    {
        const ResampBase base = resamp_base(d->ratio, idx);
        RingResampJob job;
        job.src = d->src->d_ring;
        job.src_cap = (unsigned)d->src->capacity;
        job.kind = d->ratio.kind;
        job.step = d->ratio.step;
        job.q0 = base.q0;
        job.r0 = base.r0;
        job.n_out = (unsigned)*len;
        job.dst = s->d_ring + pos * s->elem;
        job.mirror_dst = s->d_ring + (s->capacity + pos) * s->elem;
        job.n_mirror = pos < s->mirror ? (unsigned)std::min<uint64_t>(*len, s->mirror - pos) : 0u;
        job.bank = d->d_bank;
        job.log2_phases = d->log2_phases;
        job.taps = d->taps;
        if (d->ratio.kind != RESAMP_POLY)
            {
                GC_HIP(ring_resamp_direct_launch(d->src->iq_format, s->copy_stream, job));
                return GC_OK;
            }
        const int tile = ring_resamp_tile_outputs(job.step, job.taps, 1 << job.log2_phases, job.n_out, std::max(1, d->ctx->n_cus));
        GC_HIP(ring_resamp_poly_launch(d->src->iq_format, s->copy_stream, job, tile));
        return GC_OK;
    }
};

void rres_release(gc_ring_resampler* d)
{
    if (d->out)
        {
            (void)hipStreamSynchronize(d->out->copy_stream);
            std::lock_guard<std::mutex> lk(d->out->mtx);
            d->out->kernel_fed = false;
        }
    (void)hipFree(d->d_bank);
    if (d->out) gc_stream_drop(d->out);
    if (d->src) gc_stream_drop(d->src);
}

bool power_of_two(uint32_t v) { return v != 0 && (v & (v - 1)) == 0; }

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
            GC_REQUIRE(power_of_two(conf->phases) && conf->phases <= GC_RRES_MAX_PHASES, "gc_ring_resampler_create: %u phases, not a power of two in 1..%d",
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
    GC_REQUIRE(ctx && src_ring && out_ring && out, "gc_ring_resampler_create: NULL argument");
    GC_REQUIRE(src_ring != out_ring, "gc_ring_resampler_create: the source ring and the output ring are the same ring");
    GC_REQUIRE(src_ring->ctx == ctx && out_ring->ctx == ctx, "gc_ring_resampler_create: a ring belongs to another context");
    if (poly)
        GC_REQUIRE(out_ring->iq_format == GC_IQ_F32, "gc_ring_resampler_create: polyphase mode writes a GC_IQ_F32 output ring only");
    else
        GC_REQUIRE(out_ring->iq_format == src_ring->iq_format,
            "gc_ring_resampler_create: direct mode moves samples as they are: the output ring must have the source ring's format");
    {
        std::lock_guard<std::mutex> lk(src_ring->mtx);
        if (gc_stream_oldest(src_ring) != 0)
            return gc_fail(GC_ERR_STATE, "gc_ring_resampler_create: the source ring no longer holds sample 0 (its oldest sample is %llu)",
                (unsigned long long)gc_stream_oldest(src_ring));
    }
    {
        std::lock_guard<std::mutex> no_push(out_ring->push_mtx);
        std::lock_guard<std::mutex> lk(out_ring->mtx);
        GC_REQUIRE(out_ring->head == 0, "gc_ring_resampler_create: samples have been pushed into the output ring already");
        if (out_ring->kernel_fed) return gc_fail(GC_ERR_STATE, "gc_ring_resampler_create: the output ring already has a producer on the device");
        out_ring->kernel_fed = true;
    }
    gc_device_guard g(ctx->device);
    gc_ring_resampler* d = new gc_ring_resampler();
    d->ctx = ctx;
    d->ctx_ref.bind(ctx);
    d->src = src_ring;
    d->out = out_ring;
    gc_stream_keep(src_ring);
    gc_stream_keep(out_ring);
    d->ratio = ratio;
    hipError_t e = hipSuccess;
    if (poly)
        {
            d->log2_phases = log2_of(conf->phases);
            d->taps = (int)conf->taps_per_phase;
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
            delete d;
            return gc_fail(GC_ERR_HIP, "gc_ring_resampler_create: %s", hipGetErrorString(e));
        }
    *out = d;
    return GC_OK;
}

gc_status gc_ring_resampler_destroy(gc_ring_resampler* d)
{
    if (!d) return GC_OK;
    gc_device_guard g(d->ctx->device);
    rres_release(d);
    delete d;
    return GC_OK;
}

gc_status gc_ring_resampler_update(gc_ring_resampler* d, uint64_t* first_out, uint64_t* n_out)
{
    if (first_out) *first_out = 0;
    if (n_out) *n_out = 0;
    GC_REQUIRE(d, "gc_ring_resampler_update: NULL handle");
    std::lock_guard<std::mutex> one_update(d->mtx);
    gc_device_guard g(d->ctx->device);
    const uint64_t m0 = d->out_head;
    if (first_out) *first_out = m0;
    gc_stream_read_set reads(d->out->copy_stream);
    gc_status st = reads.add(d->src, resamp_floor(d->ratio, d->taps, m0));
    if (st != GC_OK) return st;  // the floor is no longer resident: nothing reserved, nothing changed
    const gc_stream_ticket& t = reads.ticket(0);
    const uint64_t m1 = resamp_available(d->ratio, t.head);
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
            rres_writer w(d);
            uint64_t first = 0;
            st = gc_stream_produce(d->out, n, &first, w, true);
            if (st == GC_OK && first != m)
                st = gc_fail(GC_ERR_STATE, "gc_ring_resampler_update: the ring's head %llu is not the resampler's output %llu", (unsigned long long)first,
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

gc_status gc_ring_resampler_info(gc_ring_resampler* d, uint64_t* src_consumed, uint64_t* out_head)
{
    GC_REQUIRE(d, "gc_ring_resampler_info: NULL handle");
    std::lock_guard<std::mutex> lk(d->mtx);
    if (src_consumed) *src_consumed = d->src_consumed;
    if (out_head) *out_head = d->out_head;
    return GC_OK;
}

gc_status gc_resampler_design(double fs_in, double fs_out, uint32_t phases, float* bank, int capacity, int* taps_per_phase)
{
    if (taps_per_phase) *taps_per_phase = 0;
    GC_REQUIRE(std::isfinite(fs_in) && std::isfinite(fs_out) && fs_in > 0.0 && fs_out > 0.0, "gc_resampler_design: the rates must be finite and positive");
    GC_REQUIRE(power_of_two(phases) && phases <= GC_RRES_MAX_PHASES, "gc_resampler_design: %u phases, not a power of two in 1..%d", phases, GC_RRES_MAX_PHASES);
    const double P = (double)phases, low = std::min(fs_in, fs_out);
    int n = 0;
    gc_status st = gc_fir_low_pass(P, P * fs_in, low / 2.1, low / 10.0, nullptr, 0, &n);
    if (st != GC_OK) return st;
    const int64_t T = ((int64_t)n + phases - 1) / phases;
    GC_REQUIRE(T >= 1 && T <= GC_RRES_MAX_TAPS && (int64_t)phases * T <= GC_RRES_MAX_BANK,
        "gc_resampler_design: %lld taps per phase (%d prototype taps over %u phases) exceed %d per phase or %d in the bank", (long long)T, n, phases,
        GC_RRES_MAX_TAPS, GC_RRES_MAX_BANK);
    if (taps_per_phase) *taps_per_phase = (int)T;
    if (!bank) return GC_OK;  // T alone
    GC_REQUIRE((int64_t)phases * T <= capacity, "gc_resampler_design: %u x %lld taps do not fit in %d", phases, (long long)T, capacity);
    std::vector<float> g((size_t)phases * T, 0.0f);  // the prototype, zero-padded to phases * T
    st = gc_fir_low_pass(P, P * fs_in, low / 2.1, low / 10.0, g.data(), n, &n);
    if (st != GC_OK) return st;
    for (uint32_t p = 0; p < phases; p++)
        for (int64_t k = 0; k < T; k++) bank[(size_t)p * T + k] = g[(size_t)k * phases + p];
    return GC_OK;
}

}  // extern "C"
