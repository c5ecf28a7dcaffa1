// gc_conditioner.hip -- gc_conditioner_*: the signal conditioner in front of an RF stream ring.  Raw samples (any gc_iq_format, any
// intermediate frequency, any integer multiple of the channels' rate) are pushed here; a kernel (cond_kernels.hip) mixes them down,
// low-pass filters and decimates them into the output ring, which acquisition and tracking read like any other gc_stream.
//
// Raw samples live in a small ring of their own in HBM (raw sample n at n % raw_cap): a push copies its block behind the previous
// one, and the kernel finds the T - 1 older samples an output needs where earlier pushes left them.  Nothing is carried over on the
// host and nothing is moved on the device, so the outputs do not depend on how the input is cut into pushes.  The H2D copy and the
// kernel are enqueued on the OUTPUT ring's copy stream, in that order, inside the ring's own push bookkeeping (gc_stream_produce):
// readers of the ring wait for the kernel exactly as they wait for the copy of a plain push.
#include "cond_kernels.h"
#include "gc_stream.h"
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
    size_t elem = 8;           // bytes per raw sample
    char* d_raw = nullptr;     // raw ring: raw_cap samples
    uint64_t raw_cap = 0;
    uint64_t chunk = 0;        // raw samples per H2D copy + launch
    float* d_taps = nullptr;
    uint64_t in_head = 0;      // raw samples pushed so far
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
        job.dst = reinterpret_cast<float2*>(s->d_ring) + pos;
        job.mirror_dst = reinterpret_cast<float2*>(s->d_ring) + s->capacity + pos;
        job.n_mirror = pos < s->mirror ? (unsigned)std::min<uint64_t>(*len, s->mirror - pos) : 0u;
        const int tile = cond_tile_outputs(job.decimation, job.n_taps, job.n_out, 2 * std::max(1, c->ctx->n_cus));
        GC_HIP(cond_launch(c->conf.in_format, s->copy_stream, job, tile));
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
    GC_REQUIRE(conf->in_format == GC_IQ_F32 || conf->in_format == GC_IQ_I16 || conf->in_format == GC_IQ_I8, "gc_conditioner_create: unknown input format %d",
        conf->in_format);
    for (uint32_t k = 0; k < conf->n_taps; k++) GC_REQUIRE(std::isfinite(taps[k]), "gc_conditioner_create: tap %u is not finite", k);
    return GC_OK;
}

void cond_release(gc_conditioner* c)
{
    if (c->out)
        {
            (void)hipStreamSynchronize(c->out->copy_stream);
            {
                std::lock_guard<std::mutex> lk(c->out->mtx);
                c->out->kernel_fed = false;
            }
        }
    (void)hipFree(c->d_raw);
    (void)hipFree(c->d_taps);
    for (int i = 0; i < gc_conditioner::kSlots; i++)
        {
            if (c->h_slot[i]) (void)hipHostFree(c->h_slot[i]);
            if (c->slot_done[i]) (void)hipEventDestroy(c->slot_done[i]);
        }
    if (c->out) gc_stream_drop(c->out);
}

gc_status cond_push(gc_conditioner* c, const void* host_raw, uint64_t n_in, uint64_t* first_out, uint64_t* n_out, bool pinned)
{
    GC_REQUIRE(c && (host_raw || n_in == 0), "gc_conditioner_push: NULL argument");
    gc_stream* s = c->out;
    const uint64_t D = c->conf.decimation;
    std::lock_guard<std::mutex> one_push(c->mtx);
    const uint64_t out_before = (c->in_head + D - 1) / D;
    const uint64_t out_after = (c->in_head + n_in + D - 1) / D;
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
                    std::memcpy(c->h_slot[k], src, (size_t)n * c->elem);
                    from = c->h_slot[k];
                }
            // behind the previous block in the raw ring (two copies when the block crosses the ring's end); the samples it overwrites
            // are older than any output still to be made needs, and the copy stream orders it behind the kernels that read them
            const uint64_t pos = c->in_head % c->raw_cap;
            const uint64_t n1 = std::min(n, c->raw_cap - pos);
            GC_HIP(hipMemcpyAsync(c->d_raw + pos * c->elem, from, (size_t)n1 * c->elem, hipMemcpyHostToDevice, s->copy_stream));
            if (n1 < n) GC_HIP(hipMemcpyAsync(c->d_raw, from + (size_t)n1 * c->elem, (size_t)(n - n1) * c->elem, hipMemcpyHostToDevice, s->copy_stream));
            if (k >= 0)
                {
                    GC_HIP(hipEventRecord(c->slot_done[k], s->copy_stream));
                    c->slot_busy[k] = true;
                }
            const uint64_t m0 = (c->in_head + D - 1) / D, m1 = (c->in_head + n + D - 1) / D;
            c->in_head += n;
            if (m1 > m0)
                {
                    cond_writer w(c);
                    uint64_t first = 0;
                    gc_status st = gc_stream_produce(s, m1 - m0, &first, w, true);
                    if (st != GC_OK) return st;
                    if (first != m0) return gc_fail(GC_ERR_STATE, "gc_conditioner_push: the ring's head %llu is not the conditioner's output %llu",
                        (unsigned long long)first, (unsigned long long)m0);
                }
            src += (size_t)n * c->elem;
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
    GC_REQUIRE(out_ring->iq_format == GC_IQ_F32, "gc_conditioner_create: the output ring must be GC_IQ_F32");
    gc_device_guard g(ctx->device);
    {
        std::lock_guard<std::mutex> no_push(out_ring->push_mtx);
        std::lock_guard<std::mutex> lk(out_ring->mtx);
        if (out_ring->kernel_fed) return gc_fail(GC_ERR_STATE, "gc_conditioner_create: the ring already has a conditioner");
        if (out_ring->head != 0) return gc_fail(GC_ERR_STATE, "gc_conditioner_create: samples have been pushed into the ring already");
        out_ring->kernel_fed = true;
    }
    gc_conditioner* c = new gc_conditioner();
    c->ctx = ctx;
    c->ctx_ref.bind(ctx);
    c->out = out_ring;
    gc_stream_keep(out_ring);
    c->conf = *conf;
    c->phase_inc = cond_phase_inc(conf->translate_hz, conf->fs_in);
    c->elem = conf->in_format == GC_IQ_F32 ? 8 : conf->in_format == GC_IQ_I16 ? 4 : 2;
    const size_t slot_bytes = (size_t)4 << 20;
    c->chunk = slot_bytes / c->elem;
    // a chunk, the T - 1 samples before it, and room for the largest tile's vector slack; a multiple of 8 samples (16 bytes in
    // every format) so that aligned vectors do not straddle the end
    c->raw_cap = (c->chunk + GC_COND_MAX_TAPS + (uint64_t)4 * GC_COND_THREADS * GC_COND_MAX_DECIMATION + 64 + 7) & ~(uint64_t)7;
    hipError_t e = hipMalloc(&c->d_raw, (size_t)c->raw_cap * c->elem);
    if (e == hipSuccess) e = hipMemset(c->d_raw, 0, (size_t)c->raw_cap * c->elem);
    if (e == hipSuccess) e = hipMalloc(&c->d_taps, sizeof(float) * conf->n_taps);
    if (e == hipSuccess) e = hipMemcpy(c->d_taps, taps, sizeof(float) * conf->n_taps, hipMemcpyHostToDevice);
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
    if (out_head) *out_head = (c->in_head + D - 1) / D;
    return GC_OK;
}

gc_status gc_fir_low_pass(double gain, double fs, double cutoff_hz, double transition_hz, float* taps, int capacity, int* n_taps)
{
    if (n_taps) *n_taps = 0;
    GC_REQUIRE(fs > 0.0 && cutoff_hz > 0.0 && cutoff_hz <= 0.5 * fs && transition_hz > 0.0 && std::isfinite(gain) && std::isfinite(fs),
        "gc_fir_low_pass: need fs > 0, 0 < cutoff_hz <= fs / 2 and transition_hz > 0");
    // Hamming window: 53 dB of stop-band attenuation, length 53 fs / (22 transition), made odd
    const double want = 53.0 * fs / (22.0 * transition_hz);
    GC_REQUIRE(want < 1.0e6, "gc_fir_low_pass: the transition width asks for %.0f taps", want);
    int n = (int)want;
    if ((n & 1) == 0) n++;
    if (n_taps) *n_taps = n;
    if (!taps) return GC_OK;  // length query
    GC_REQUIRE(n <= capacity, "gc_fir_low_pass: %d taps do not fit in %d", n, capacity);
    const int M = (n - 1) / 2;
    const double pi = 3.14159265358979323846, w0 = 2.0 * pi * cutoff_hz / fs;
    std::vector<double> h((size_t)n);
    double sum = 0.0;
    for (int i = 0; i < n; i++)
        {
            const int k = i - M;
            const double win = n > 1 ? 0.54 - 0.46 * std::cos(2.0 * pi * i / (n - 1)) : 1.0;
            h[i] = (k == 0 ? w0 / pi : std::sin(k * w0) / (k * pi)) * win;
            sum += h[i];
        }
    for (int i = 0; i < n; i++) taps[i] = (float)(gain * h[i] / sum);
    return GC_OK;
}

}  // extern "C"
