// gc_conditioner.hip -- gc_conditioner_*: the signal conditioner in front of an RF stream ring.  Raw samples (any gc_iq_format or
// gc_raw_real_format, any intermediate frequency, any integer multiple of the channels' rate) are pushed here; a kernel (cond_kernels.hip) mixes them down,
// low-pass filters and decimates them into the output ring, which acquisition and tracking read like any other gc_stream.
//
// Raw samples live in a small ring of their own in HBM (raw sample n at n % raw_cap): a push copies its block behind the previous
// one, and the kernel finds the T - 1 older samples an output needs where earlier pushes left them.  Nothing is carried over on the
// host and nothing is moved on the device, so the outputs do not depend on how the input is cut into pushes.  The H2D copy and the
// kernel are enqueued on the OUTPUT ring's copy stream, in that order, inside the ring's own push bookkeeping (gc_stream_produce):
// readers of the ring wait for the kernel exactly as they wait for the copy of a plain push.
//
// Pulse blanking (gc_conditioner_set_pulse_blanking) acts on the raw ring between the two: once a chunk's copy is enqueued, the
// segments it completes get their energies, their decisions and -- the flagged ones -- zeros in place (cond_blank_kernels.hip), and
// the FIR launch covers the outputs whose newest input those segments decide.  The undecided tail (< L samples) waits in the raw
// ring for the next push, in front of the T - 1 samples of history.
//
// The output ring may have any gc_iq_format.  The kernel's store epilogue (cond_store_epilogue.h) scales, clamps and rounds into a
// GC_IQ_I16 / GC_IQ_I8 ring and counts the clipped components; a GC_IQ_F32 ring has neither a scale nor a counter.  The claim on
// the output ring, the geometry of a piece and that output state are shared with the derived rings (gc_ring_stage.h); the
// filter design and the blanker's quantile are host numerics (gc_numerics.cpp).
#include "cond_blank_kernels.h"
#include "cond_kernels.h"
#include "gc_ring_stage.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

struct gc_conditioner
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    gc_stream* out = nullptr;  // holds a reference
    gc_conditioner_conf conf;
    uint64_t phase_inc = 0;
    unsigned bits = 64;        // bits per raw sample (2 for GC_RAW_REAL_2BIT: counts of samples become bytes through raw_bytes())
    char* d_raw = nullptr;     // raw ring: raw_cap samples
    uint64_t raw_cap = 0;
    uint64_t chunk = 0;        // raw samples per H2D copy + launch
    float* d_taps = nullptr;
    uint64_t in_head = 0;      // raw samples pushed so far
    // pulse blanking: off until gc_conditioner_set_pulse_blanking
    bool blanking = false;
    gc_blanking_conf blank_conf;
    BlankParams blank_params;
    BlankState* d_blank_state = nullptr;
    float* d_blank_energy = nullptr;        // one chunk's segments
    unsigned char* d_blank_flags = nullptr;
    uint64_t blank_max_seg = 0;             // segments one chunk can complete
    // GC_IQ_I16 / GC_IQ_I8 output rings (gc_conditioner_set_output_scale, gc_conditioner_output_info)
    gc_quantised_output quant;
    // pinned staging for pageable caller buffers (as in gc_stream)
    static const int kSlots = 2;
    char* h_slot[kSlots] = {nullptr, nullptr};
    hipEvent_t slot_done[kSlots] = {nullptr, nullptr};
    bool slot_busy[kSlots] = {false, false};
    int next_slot = 0;
    std::mutex mtx;  // one push at a time
};

namespace
{
// bytes of n raw samples; n is a multiple of 4 wherever the format is GC_RAW_REAL_2BIT (pushes, ring positions and chunks all are)
inline size_t raw_bytes(const gc_conditioner* c, uint64_t n) { return (size_t)(n * c->bits / 8u); }
inline bool cond_real(int fmt) { return fmt == GC_RAW_REAL_F32 || fmt == GC_RAW_REAL_I16 || fmt == GC_RAW_REAL_I8 || fmt == GC_RAW_REAL_2BIT; }

// writes the outputs of one chunk of raw samples: one launch per contiguous piece of the output ring
struct cond_writer : gc_ring_writer
{
    gc_conditioner* c;
    explicit cond_writer(gc_conditioner* c_) : c(c_) {}
    bool writes_mirror() const override { return true; }
    gc_status write(gc_stream* s, uint64_t idx, uint64_t pos, uint64_t* len) override
    {
        CondJob job;
        job.raw = c->d_raw;
        job.raw_cap = (unsigned)c->raw_cap;
        job.taps = c->d_taps;
        job.n_taps = (int)c->conf.n_taps;
        job.decimation = (int)c->conf.decimation;
        job.phase_inc = c->phase_inc;
        job.first_out = idx;
        job.n_out = (unsigned)*len;
        job.out = gc_ring_stage_piece(s, pos, *len, c->quant.scale, c->quant.d_clipped);
        const int tile = cond_tile_outputs(job.decimation, job.n_taps, job.n_out, 2 * std::max(1, c->ctx->n_cus));
        GC_HIP(cond_launch(c->conf.in_format, s->iq_format, s->copy_stream, job, tile));
        return GC_OK;
    }
};

uint64_t cond_phase_inc(double translate_hz, double fs_in)
{
    // round(f / fs * 2^64) mod 2^64: quotient and scaling in IEEE double (the scaling is exact), ties to even
    const double v = std::nearbyint(std::ldexp(translate_hz / fs_in, 64));  // |v| <= 2^63
    return v < 0.0 ? (uint64_t)0 - (uint64_t)(-v) : (uint64_t)v;
}

gc_status cond_check_conf(const gc_conditioner_conf* conf, const float* taps)
{
    GC_REQUIRE(conf && taps, "gc_conditioner_create: NULL configuration or taps");
    GC_REQUIRE(conf->decimation >= 1 && conf->decimation <= GC_COND_MAX_DECIMATION, "gc_conditioner_create: decimation %u is outside 1..%d",
        conf->decimation, GC_COND_MAX_DECIMATION);
    GC_REQUIRE(conf->n_taps >= 1 && conf->n_taps <= GC_COND_MAX_TAPS, "gc_conditioner_create: %u taps, outside 1..%d", conf->n_taps, GC_COND_MAX_TAPS);
    GC_REQUIRE(conf->fs_in > 0.0 && std::isfinite(conf->fs_in), "gc_conditioner_create: fs_in must be positive");
    GC_REQUIRE(std::isfinite(conf->translate_hz) && std::fabs(conf->translate_hz) <= 0.5 * conf->fs_in,
        "gc_conditioner_create: |translate_hz| = %g exceeds fs_in / 2 = %g", std::fabs(conf->translate_hz), 0.5 * conf->fs_in);
    GC_REQUIRE(conf->in_format == GC_IQ_F32 || conf->in_format == GC_IQ_I16 || conf->in_format == GC_IQ_I8 || cond_real(conf->in_format),
        "gc_conditioner_create: unknown input format %d", conf->in_format);
    for (uint32_t k = 0; k < conf->n_taps; k++) GC_REQUIRE(std::isfinite(taps[k]), "gc_conditioner_create: tap %u is not finite", k);
    return GC_OK;
}

void cond_blank_free(gc_conditioner* c)
{
    (void)hipFree(c->d_blank_state);
    (void)hipFree(c->d_blank_energy);
    (void)hipFree(c->d_blank_flags);
    c->d_blank_state = nullptr;
    c->d_blank_energy = nullptr;
    c->d_blank_flags = nullptr;
    c->blanking = false;
}

// raw samples whose fate is known: all of them without blanking, whole segments with it
uint64_t cond_decided(const gc_conditioner* c, uint64_t in_head)
{
    return c->blanking ? in_head / c->blank_conf.length * c->blank_conf.length : in_head;
}

gc_status cond_check_blanking(const gc_blanking_conf* b)
{
    GC_REQUIRE(b, "gc_conditioner_set_pulse_blanking: NULL configuration");
    GC_REQUIRE(b->length >= 1 && b->length <= GC_COND_MAX_BLANK_LENGTH, "gc_conditioner_set_pulse_blanking: length %u is outside 1..%d", b->length,
        GC_COND_MAX_BLANK_LENGTH);
    GC_REQUIRE(b->pfa > 0.0f && b->pfa < 1.0f, "gc_conditioner_set_pulse_blanking: pfa %g is outside (0, 1)", (double)b->pfa);
    GC_REQUIRE(b->segments_est >= 1, "gc_conditioner_set_pulse_blanking: segments_est must be at least 1");
    GC_REQUIRE(b->threshold == 0.0f || (std::isfinite(b->threshold) && b->threshold > 0.0f),
        "gc_conditioner_set_pulse_blanking: threshold %g is neither 0 (from pfa and length) nor finite and positive", (double)b->threshold);
    return GC_OK;
}

void cond_release(gc_conditioner* c)
{
    if (c->out) gc_ring_stage_release(c->out);  // waits for the kernels that read what is freed below
    (void)hipFree(c->d_raw);
    (void)hipFree(c->d_taps);
    gc_quantised_output_free(&c->quant);
    cond_blank_free(c);
    for (int i = 0; i < gc_conditioner::kSlots; i++)
        {
            if (c->h_slot[i]) (void)hipHostFree(c->h_slot[i]);
            if (c->slot_done[i]) (void)hipEventDestroy(c->slot_done[i]);
        }
}

gc_status cond_push(gc_conditioner* c, const void* host_raw, uint64_t n_in, uint64_t* first_out, uint64_t* n_out, bool pinned)
{
    GC_REQUIRE(c && (host_raw || n_in == 0), "gc_conditioner_push: NULL argument");
    gc_stream* s = c->out;
    const uint64_t D = c->conf.decimation;
    GC_REQUIRE(c->conf.in_format != GC_RAW_REAL_2BIT || (n_in & 3u) == 0, "gc_conditioner_push: %llu samples of GC_RAW_REAL_2BIT are not whole bytes",
        (unsigned long long)n_in);
    std::lock_guard<std::mutex> one_push(c->mtx);
    const uint64_t out_before = (cond_decided(c, c->in_head) + D - 1) / D;
    const uint64_t out_after = (cond_decided(c, c->in_head + n_in) + D - 1) / D;
    GC_REQUIRE(out_after - out_before <= s->capacity, "gc_conditioner_push: the push makes %llu outputs, the ring holds %llu",
        (unsigned long long)(out_after - out_before), (unsigned long long)s->capacity);
    if (first_out) *first_out = out_before;
    if (n_out) *n_out = out_after - out_before;
    gc_device_guard g(c->ctx->device);
    const char* src = static_cast<const char*>(host_raw);
    uint64_t left = n_in;
    while (left > 0)
        {
            const uint64_t n = std::min(left, c->chunk);
            const char* from = src;
            int k = -1;
            if (!pinned)
                {
                    k = c->next_slot;
                    c->next_slot = (k + 1) % gc_conditioner::kSlots;
                    if (c->slot_busy[k]) GC_HIP(hipEventSynchronize(c->slot_done[k]));
                    std::memcpy(c->h_slot[k], src, raw_bytes(c, n));
                    from = c->h_slot[k];
                }
            // behind the previous block in the raw ring (two copies when the block crosses the ring's end); the samples it overwrites
            // are older than any output still to be made needs, and the copy stream orders it behind the kernels that read them
            const uint64_t pos = c->in_head % c->raw_cap;
            const uint64_t n1 = std::min(n, c->raw_cap - pos);
            GC_HIP(hipMemcpyAsync(c->d_raw + raw_bytes(c, pos), from, raw_bytes(c, n1), hipMemcpyHostToDevice, s->copy_stream));
            if (n1 < n) GC_HIP(hipMemcpyAsync(c->d_raw, from + raw_bytes(c, n1), raw_bytes(c, n - n1), hipMemcpyHostToDevice, s->copy_stream));
            if (k >= 0)
                {
                    GC_HIP(hipEventRecord(c->slot_done[k], s->copy_stream));
                    c->slot_busy[k] = true;
                }
            const uint64_t dec0 = cond_decided(c, c->in_head), dec1 = cond_decided(c, c->in_head + n);
            const uint64_t m0 = (dec0 + D - 1) / D, m1 = (dec1 + D - 1) / D;
            c->in_head += n;
            if (dec1 > dec0 && c->blanking)
                {
                    // the segments this chunk completes (the first may have begun in an earlier copy), before the FIR reads them
                    BlankJob job;
                    job.raw = c->d_raw;
                    job.raw_cap = (unsigned)c->raw_cap;
                    job.length = c->blank_conf.length;
                    job.seg0 = dec0 / c->blank_conf.length;
                    job.n_seg = (unsigned)((dec1 - dec0) / c->blank_conf.length);
                    job.energies = c->d_blank_energy;
                    job.flags = c->d_blank_flags;
                    job.state = c->d_blank_state;
                    job.params = c->blank_params;
                    if (job.n_seg > c->blank_max_seg) return gc_fail(GC_ERR_STATE, "gc_conditioner_push: %u segments in one chunk", job.n_seg);
                    GC_HIP(cond_blank_launch(c->conf.in_format, s->copy_stream, job));
                }
            if (m1 > m0)
                {
                    cond_writer w(c);
                    uint64_t first = 0;
                    gc_status st = gc_stream_produce(s, m1 - m0, &first, w, true);
                    if (st != GC_OK) return st;
                    if (first != m0) return gc_fail(GC_ERR_STATE, "gc_conditioner_push: the ring's head %llu is not the conditioner's output %llu",
                        (unsigned long long)first, (unsigned long long)m0);
                }
            src += raw_bytes(c, n);
            left -= n;
        }
    return GC_OK;
}
}  // namespace

extern "C" {

size_t gc_conditioner_conf_size(void) { return sizeof(gc_conditioner_conf); }

gc_status gc_conditioner_create(gc_ctx* ctx, const gc_conditioner_conf* conf, const float* taps, gc_stream* out_ring, gc_conditioner** out)
{
    if (out) *out = nullptr;
    // the configuration first, before anything that needs a device
    gc_status st = cond_check_conf(conf, taps);
    if (st != GC_OK) return st;
    GC_REQUIRE(ctx && out_ring && out, "gc_conditioner_create: NULL argument");
    GC_REQUIRE(out_ring->ctx == ctx, "gc_conditioner_create: the output ring belongs to another context");
    GC_REQUIRE(out_ring->iq_format == GC_IQ_F32 || out_ring->quantised_output,
        "gc_conditioner_create: the output ring must be GC_IQ_F32, or an integer ring opened with gc_stream_accept_quantised_output");
    gc_device_guard g(ctx->device);
    const unsigned why = gc_ring_stage_claim(out_ring);
    if (why & GC_RING_HAS_PRODUCER) return gc_fail(GC_ERR_STATE, "gc_conditioner_create: the ring already has a conditioner");
    if (why) return gc_fail(GC_ERR_STATE, "gc_conditioner_create: samples have been pushed into the ring already");
    gc_conditioner* c = new gc_conditioner();
    c->ctx = ctx;
    c->ctx_ref.bind(ctx);
    c->out = out_ring;
    gc_stream_keep(out_ring);
    c->conf = *conf;
    c->phase_inc = cond_phase_inc(conf->translate_hz, conf->fs_in);
    c->bits = cond_raw_bits(conf->in_format);
    const size_t slot_bytes = (size_t)4 << 20;
    c->chunk = (uint64_t)slot_bytes * 8u / c->bits;
    // a chunk, the T - 1 samples before it, and room for the largest tile's vector slack; a multiple of 8 samples (16 bytes in
    // every format) so that aligned vectors do not straddle the end
    // and the undecided tail of a blanked stream (< GC_COND_MAX_BLANK_LENGTH samples) in front of that history
    // the real formats: a multiple of 64 samples (16 bytes of the 2-bit format) and two such vectors of slack
    const uint64_t align = cond_raw_align(conf->in_format);
    c->raw_cap = (c->chunk + GC_COND_MAX_TAPS + GC_COND_MAX_BLANK_LENGTH + (uint64_t)4 * GC_COND_THREADS * GC_COND_MAX_DECIMATION + 8 * align + align - 1) &
                 ~(align - 1);
    hipError_t e = hipMalloc(&c->d_raw, raw_bytes(c, c->raw_cap));
    if (e == hipSuccess) e = hipMemset(c->d_raw, 0, raw_bytes(c, c->raw_cap));
    if (e == hipSuccess) e = hipMalloc(&c->d_taps, sizeof(float) * conf->n_taps);
    if (e == hipSuccess) e = hipMemcpy(c->d_taps, taps, sizeof(float) * conf->n_taps, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = gc_quantised_output_alloc(&c->quant, out_ring);
    for (int i = 0; i < gc_conditioner::kSlots && e == hipSuccess; i++)
        {
            e = hipHostMalloc(reinterpret_cast<void**>(&c->h_slot[i]), slot_bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->slot_done[i], hipEventDisableTiming);
        }
    if (e != hipSuccess)
        {
            cond_release(c);
            delete c;
            return gc_fail(GC_ERR_HIP, "gc_conditioner_create: %s", hipGetErrorString(e));
        }
    *out = c;
    return GC_OK;
}

gc_status gc_conditioner_destroy(gc_conditioner* c)
{
    if (!c) return GC_OK;
    gc_device_guard g(c->ctx->device);
    cond_release(c);
    delete c;
    return GC_OK;
}

gc_status gc_conditioner_push(gc_conditioner* c, const void* host_raw, uint64_t n_in, uint64_t* first_out, uint64_t* n_out)
{
    return cond_push(c, host_raw, n_in, first_out, n_out, false);
}

gc_status gc_conditioner_push_pinned(gc_conditioner* c, const void* pinned_host_raw, uint64_t n_in, uint64_t* first_out, uint64_t* n_out)
{
    return cond_push(c, pinned_host_raw, n_in, first_out, n_out, true);
}

gc_status gc_conditioner_info(gc_conditioner* c, uint64_t* in_head, uint64_t* out_head)
{
    GC_REQUIRE(c, "gc_conditioner_info: NULL handle");
    std::lock_guard<std::mutex> lk(c->mtx);
    const uint64_t D = c->conf.decimation;
    if (in_head) *in_head = c->in_head;
    if (out_head) *out_head = (cond_decided(c, c->in_head) + D - 1) / D;
    return GC_OK;
}

gc_status gc_conditioner_set_output_scale(gc_conditioner* c, float scale)
{
    const gc_status st = gc_quantised_output_check_scale("gc_conditioner_set_output_scale", scale, c ? c->out : nullptr);
    if (st != GC_OK) return st;
    std::lock_guard<std::mutex> one_push(c->mtx);
    if (c->in_head != 0) return gc_fail(GC_ERR_STATE, "gc_conditioner_set_output_scale: samples have been pushed already");
    c->quant.scale = scale;
    return GC_OK;
}

gc_status gc_conditioner_output_info(gc_conditioner* c, int32_t* out_format, float* scale, uint64_t* clipped_components)
{
    GC_REQUIRE(c, "gc_conditioner_output_info: NULL handle");
    std::lock_guard<std::mutex> one_push(c->mtx);
    return gc_quantised_output_info(&c->quant, c->ctx, c->out, out_format, scale, clipped_components);
}

size_t gc_blanking_conf_size(void) { return sizeof(gc_blanking_conf); }

gc_status gc_conditioner_set_pulse_blanking(gc_conditioner* c, const gc_blanking_conf* conf)
{
    // the configuration first, before anything that needs a device
    gc_status st = cond_check_blanking(conf);
    if (st != GC_OK) return st;
    GC_REQUIRE(c, "gc_conditioner_set_pulse_blanking: NULL handle");
    GC_REQUIRE(c->conf.in_format != GC_RAW_REAL_2BIT, "gc_conditioner_set_pulse_blanking: GC_RAW_REAL_2BIT samples cannot be blanked in place");
    // degrees of freedom of a segment's energy: two components per complex sample, one per real sample
    const uint32_t dof = cond_real(c->conf.in_format) ? conf->length : 2u * conf->length;
    float threshold = conf->threshold;
    if (threshold == 0.0f)
        {
            double q = 0.0;
            st = gc_chi2_upper_quantile((double)dof, (double)conf->pfa, &q);
            if (st != GC_OK) return st;
            threshold = (float)q;
        }
    std::lock_guard<std::mutex> one_push(c->mtx);
    if (c->in_head != 0) return gc_fail(GC_ERR_STATE, "gc_conditioner_set_pulse_blanking: samples have been pushed already");
    gc_device_guard g(c->ctx->device);
    cond_blank_free(c);
    c->blank_conf = *conf;
    c->blank_conf.threshold = threshold;
    c->blank_params.threshold = threshold;
    c->blank_params.dof = (float)dof;
    c->blank_params.segments_est = conf->segments_est;
    c->blank_params.segments_reset = conf->segments_reset;
    c->blank_max_seg = c->chunk / conf->length + 1;
    hipError_t e = hipMalloc(&c->d_blank_state, sizeof(BlankState));
    if (e == hipSuccess) e = hipMemset(c->d_blank_state, 0, sizeof(BlankState));
    if (e == hipSuccess) e = hipMalloc(&c->d_blank_energy, sizeof(float) * c->blank_max_seg);
    if (e == hipSuccess) e = hipMalloc(&c->d_blank_flags, c->blank_max_seg);
    if (e != hipSuccess)
        {
            cond_blank_free(c);
            return gc_fail(GC_ERR_HIP, "gc_conditioner_set_pulse_blanking: %s", hipGetErrorString(e));
        }
    c->blanking = true;
    return GC_OK;
}

gc_status gc_conditioner_blanking_info(gc_conditioner* c, uint64_t* segments_decided, uint64_t* segments_blanked, float* noise_power, uint32_t* n_segments,
    float* threshold)
{
    GC_REQUIRE(c, "gc_conditioner_blanking_info: NULL handle");
    std::lock_guard<std::mutex> one_push(c->mtx);
    if (!c->blanking) return gc_fail(GC_ERR_STATE, "gc_conditioner_blanking_info: pulse blanking is not configured");
    gc_device_guard g(c->ctx->device);
    BlankState st;
    GC_HIP(hipStreamSynchronize(c->out->copy_stream));
    GC_HIP(hipMemcpy(&st, c->d_blank_state, sizeof st, hipMemcpyDeviceToHost));
    if (segments_decided) *segments_decided = st.decided;
    if (segments_blanked) *segments_blanked = st.blanked;
    if (noise_power) *noise_power = st.noise;
    if (n_segments) *n_segments = st.n;
    if (threshold) *threshold = c->blank_params.threshold;
    return GC_OK;
}

}  // extern "C"
