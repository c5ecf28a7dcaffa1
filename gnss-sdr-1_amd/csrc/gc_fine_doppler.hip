// gc_fine_doppler.hip -- C ABI of the fine Doppler stage (gnsscorr.h; kernels in acq_fine_kernels.hip, rules in acq_fine_window.h).
#include "acq_fine_kernels.h"
#include "gc_internal.h"
#include "gc_stream.h"
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

static_assert((int)GC_FINE_ALIGN_REFERENCE == (int)FINE_ALIGN_REFERENCE && (int)GC_FINE_ALIGN_EXACT == (int)FINE_ALIGN_EXACT, "one alignment code");
static_assert(sizeof(gc_fine_doppler_result) == 32 && sizeof(gc_fine_doppler_request) == 16 && sizeof(gc_fine_doppler_conf) == 32, "gnsscorr.h layouts");

static const uint64_t FINE_MAX_WINDOW_BINS = 8192;

struct gc_fine_doppler
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;  // before the buffers: the context outlives their frees (gc_internal.h)
    gc_fine_doppler_conf conf;
    int n_slots = 0;
    uint32_t total = 0, next = 0, n_tiles = 0, stride = 0;
    std::vector<char> has_code;
    gc_dev_buf<float2> d_codes;
    gc_dev_buf<float2> d_block;  // the host entry point's samples
    gc_dev_buf<AcqFineRequest> d_req;
    gc_host_buf<AcqFineRequest> h_req;
    gc_dev_buf<float2> d_partial;
    gc_dev_buf<float> d_energy, d_spec;
    gc_dev_buf<gc_fine_doppler_result> d_results;
    gc_host_buf<gc_fine_doppler_result> h_results;
    std::vector<uint32_t> last_bins;  // window_bins of the last call's requests
};

// the requests of one call as the kernels take them; no device is touched
static gc_status fine_resolve(gc_fine_doppler* f, const char* who, const gc_fine_doppler_request* requests, int n_requests, std::vector<AcqFineRequest>& out)
{
    GC_REQUIRE(n_requests >= 1 && n_requests <= f->n_slots, "%s: n_requests = %d, the handle takes 1..%d", who, n_requests, f->n_slots);
    for (int i = 0; i < n_requests; i++)
        {
            const gc_fine_doppler_request& q = requests[i];
            GC_REQUIRE(q.slot < (uint32_t)f->n_slots, "%s: request %d names slot %u of %d", who, i, q.slot, f->n_slots);
            GC_REQUIRE(f->has_code[q.slot], "%s: request %d: slot %u has no code (gc_fine_doppler_set_code)", who, i, q.slot);
            GC_REQUIRE(q.delay_samples < f->conf.samples_per_code, "%s: request %d: delay_samples %u >= samples_per_code %u", who, i, q.delay_samples,
                f->conf.samples_per_code);
            GC_REQUIRE(fine_window_ok(f->conf.fs_in, q.coarse_doppler_hz, (double)f->conf.window_hz),
                "%s: request %d: |coarse_doppler_hz| + window_hz must be finite and below fs_in / 2 (%g, %g, %lld)", who, i, q.coarse_doppler_hz,
                (double)f->conf.window_hz, (long long)f->conf.fs_in);
        }
    out.resize(n_requests);
    for (int i = 0; i < n_requests; i++)
        {
            AcqFineRequest& r = out[i];
            r.slot = requests[i].slot;
            r.delay = requests[i].delay_samples;
            fine_window(f->conf.fs_in, f->next, requests[i].coarse_doppler_hz, (double)f->conf.window_hz, &r.k_lo, &r.count);
            GC_REQUIRE(r.count >= 1, "%s: request %d: no bin lies within %g Hz of %g Hz", who, i, (double)f->conf.window_hz, requests[i].coarse_doppler_hz);
            GC_REQUIRE(r.count <= f->stride, "%s: request %d: window of %u bins, %u expected at the most", who, i, r.count, f->stride);
        }
    return GC_OK;
}

// the caller holds the context mutex
static gc_status fine_enqueue(gc_fine_doppler* f, const void* src, unsigned src_cap, uint64_t first, int iq_format, const std::vector<AcqFineRequest>& req,
    hipStream_t st)
{
    const int n_requests = (int)req.size();
    std::memcpy(f->h_req, req.data(), sizeof(AcqFineRequest) * n_requests);
    GC_HIP(hipMemcpyAsync(f->d_req, f->h_req, sizeof(AcqFineRequest) * n_requests, hipMemcpyHostToDevice, st));
    AcqFineArgs a;
    a.src = src;
    a.src_cap = src_cap;
    a.first = first;
    a.codes = f->d_codes;
    a.req = f->d_req;
    a.partial = f->d_partial;
    a.energy = f->d_energy;
    a.spec = f->d_spec;
    a.results = f->d_results;
    a.fs = f->conf.fs_in;
    a.n = f->conf.samples_per_code;
    a.total = f->total;
    a.next = f->next;
    a.n_tiles = f->n_tiles;
    a.stride = f->stride;
    a.alignment = f->conf.alignment;
    hipError_t e = acq_fine_launch(st, a, iq_format, n_requests);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_fine_doppler: kernel launch failed: %s", hipGetErrorString(e));
    return GC_OK;
}

static gc_status fine_fetch(gc_fine_doppler* f, int n_requests, gc_fine_doppler_result* results, hipStream_t st)
{
    GC_HIP(hipMemcpyAsync(f->h_results, f->d_results, sizeof(gc_fine_doppler_result) * n_requests, hipMemcpyDeviceToHost, st));
    GC_HIP(hipStreamSynchronize(st));
    std::memcpy(results, f->h_results, sizeof(gc_fine_doppler_result) * n_requests);
    f->last_bins.resize(n_requests);
    for (int i = 0; i < n_requests; i++) f->last_bins[i] = f->h_req[i].count;
    return GC_OK;
}

extern "C" {

size_t gc_fine_doppler_conf_size(void) { return sizeof(gc_fine_doppler_conf); }

gc_status gc_fine_doppler_window(int64_t fs_in, uint32_t next, double coarse_hz, double window_hz, uint32_t* first_bin, uint32_t* bins)
{
    GC_REQUIRE(first_bin && bins, "gc_fine_doppler_window: NULL argument");
    GC_REQUIRE(fine_sizes_ok(fs_in, next), "gc_fine_doppler_window: fs_in %lld must be positive, next %u even and at most 2^24", (long long)fs_in, next);
    GC_REQUIRE(fine_window_ok(fs_in, coarse_hz, window_hz), "gc_fine_doppler_window: window_hz must be finite and positive and |coarse_hz| + window_hz < fs_in / 2");
    fine_window(fs_in, next, coarse_hz, window_hz, first_bin, bins);
    return GC_OK;
}

gc_status gc_fine_doppler_create(gc_ctx* ctx, const gc_fine_doppler_conf* conf, int n_slots, gc_fine_doppler** out)
{
    GC_REQUIRE(conf && out, "gc_fine_doppler_create: NULL argument");
    GC_REQUIRE(n_slots >= 1, "gc_fine_doppler_create: n_slots must be >= 1");
    GC_REQUIRE(conf->samples_per_code >= 1, "gc_fine_doppler_create: samples_per_code must be >= 1");
    GC_REQUIRE(conf->prn_replicas >= 1 && conf->prn_replicas <= 50, "gc_fine_doppler_create: prn_replicas %u outside 1..50", conf->prn_replicas);
    GC_REQUIRE(conf->zero_padding_factor >= 1 && conf->zero_padding_factor <= 16, "gc_fine_doppler_create: zero_padding_factor %u outside 1..16",
        conf->zero_padding_factor);
    const uint64_t next = (uint64_t)conf->samples_per_code * conf->prn_replicas * conf->zero_padding_factor;
    GC_REQUIRE(fine_sizes_ok(conf->fs_in, next), "gc_fine_doppler_create: fs_in %lld must be positive, Next = P N Z = %llu even and at most 2^24",
        (long long)conf->fs_in, (unsigned long long)next);
    GC_REQUIRE(fine_window_ok(conf->fs_in, 0.0, (double)conf->window_hz), "gc_fine_doppler_create: window_hz %g must be finite, positive and below fs_in / 2",
        (double)conf->window_hz);
    GC_REQUIRE(conf->alignment == GC_FINE_ALIGN_REFERENCE || conf->alignment == GC_FINE_ALIGN_EXACT, "gc_fine_doppler_create: unknown alignment %d",
        conf->alignment);
    const uint64_t max_bins = fine_window_max_bins(conf->fs_in, (uint32_t)next, (double)conf->window_hz);
    GC_REQUIRE(max_bins <= FINE_MAX_WINDOW_BINS, "gc_fine_doppler_create: a window of up to %llu bins, at most %llu are computed", (unsigned long long)max_bins,
        (unsigned long long)FINE_MAX_WINDOW_BINS);
    GC_REQUIRE(ctx, "gc_fine_doppler_create: NULL context");
    gc_device_guard g(ctx->device);
    std::unique_ptr<gc_fine_doppler> f(new gc_fine_doppler());  // behind the guard: freed on its device if an allocation fails
    f->ctx = ctx;
    f->ctx_ref.bind(ctx);
    f->conf = *conf;
    f->n_slots = n_slots;
    f->total = conf->samples_per_code * conf->prn_replicas;
    f->next = (uint32_t)next;
    f->n_tiles = (f->total + ACQ_FINE_TILE - 1) / ACQ_FINE_TILE;
    f->stride = (uint32_t)max_bins;
    f->has_code.assign(n_slots, 0);
    const size_t ns = (size_t)n_slots;
    hipError_t e = f->d_codes.alloc(ns * conf->samples_per_code);
    if (e == hipSuccess) e = f->d_block.alloc(f->total);
    if (e == hipSuccess) e = f->d_req.alloc(ns);
    if (e == hipSuccess) e = f->d_partial.alloc(ns * f->n_tiles * f->stride);
    if (e == hipSuccess) e = f->d_energy.alloc(ns * f->n_tiles);
    if (e == hipSuccess) e = f->d_spec.alloc(ns * f->stride);
    if (e == hipSuccess) e = f->d_results.alloc(ns);
    if (e == hipSuccess) e = f->h_req.alloc(ns);
    if (e == hipSuccess) e = f->h_results.alloc(ns);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_fine_doppler_create: allocation failed: %s", hipGetErrorString(e));
    *out = f.release();
    return GC_OK;
}

gc_status gc_fine_doppler_destroy(gc_fine_doppler* f)
{
    GC_REQUIRE(f, "gc_fine_doppler_destroy: NULL handle");
    gc_device_guard g(f->ctx->device);
    {
        std::lock_guard<std::mutex> lk(f->ctx->mtx);
        (void)hipStreamSynchronize(f->ctx->stream);
    }
    delete f;  // the buffers go with it, on their device; the mutex may go with the context
    return GC_OK;
}

gc_status gc_fine_doppler_set_code(gc_fine_doppler* f, int slot, const float* code)
{
    GC_REQUIRE(f && code, "gc_fine_doppler_set_code: NULL argument");
    GC_REQUIRE(slot >= 0 && slot < f->n_slots, "gc_fine_doppler_set_code: slot %d of %d", slot, f->n_slots);
    gc_device_guard g(f->ctx->device);
    std::lock_guard<std::mutex> lk(f->ctx->mtx);
    hipStream_t st = f->ctx->stream;
    const size_t n = f->conf.samples_per_code;
    GC_HIP(hipMemcpyAsync(f->d_codes + (size_t)slot * n, code, sizeof(float2) * n, hipMemcpyHostToDevice, st));
    GC_HIP(hipStreamSynchronize(st));
    f->has_code[slot] = 1;
    return GC_OK;
}

gc_status gc_fine_doppler_estimate_stream(gc_fine_doppler* f, gc_stream* s, uint64_t first_index, const gc_fine_doppler_request* requests, int n_requests,
    gc_fine_doppler_result* results)
{
    const char* who = "gc_fine_doppler_estimate_stream";
    GC_REQUIRE(f && s && requests && results, "%s: NULL argument", who);
    GC_REQUIRE(s->ctx->device == f->ctx->device, "%s: the stream lives on another GPU", who);
    std::vector<AcqFineRequest> req;
    gc_status rs = fine_resolve(f, who, requests, n_requests, req);
    if (rs != GC_OK) return rs;
    gc_device_guard g(f->ctx->device);
    std::lock_guard<std::mutex> lk(f->ctx->mtx);
    hipStream_t st = f->ctx->stream;
    // the block is protected against eviction from here (reserved before the residency check and the launch)
    gc_stream_read_set reads(st);
    rs = reads.add(s, first_index);
    if (rs != GC_OK) return rs;
    const gc_stream_ticket& t = reads.ticket(0);
    // (head - first_index, not first_index + total: the sum wraps for an index near 2^64)
    if (first_index > t.head || f->total > t.head - first_index)
        return gc_fail(GC_ERR_INVALID, "%s: block [%llu, +%u) is not inside the stream's resident samples [%llu, %llu)", who,
            (unsigned long long)first_index, f->total, (unsigned long long)t.oldest, (unsigned long long)t.head);
    rs = fine_enqueue(f, s->d_ring, (unsigned)s->capacity, first_index, s->iq_format, req, st);
    if (rs != GC_OK) return rs;
    rs = reads.commit();
    if (rs != GC_OK) return rs;
    return fine_fetch(f, n_requests, results, st);
}

gc_status gc_fine_doppler_estimate(gc_fine_doppler* f, const float* host_iq, const gc_fine_doppler_request* requests, int n_requests,
    gc_fine_doppler_result* results)
{
    const char* who = "gc_fine_doppler_estimate";
    GC_REQUIRE(f && host_iq && requests && results, "%s: NULL argument", who);
    std::vector<AcqFineRequest> req;
    gc_status rs = fine_resolve(f, who, requests, n_requests, req);
    if (rs != GC_OK) return rs;
    gc_device_guard g(f->ctx->device);
    std::lock_guard<std::mutex> lk(f->ctx->mtx);
    hipStream_t st = f->ctx->stream;
    GC_HIP(hipMemcpyAsync(f->d_block, host_iq, sizeof(float2) * f->total, hipMemcpyHostToDevice, st));
    rs = fine_enqueue(f, f->d_block, f->total, 0, GC_IQ_F32, req, st);
    if (rs != GC_OK) return rs;
    return fine_fetch(f, n_requests, results, st);
}

gc_status gc_fine_doppler_spectrum(gc_fine_doppler* f, int request_index, float* host_p)
{
    GC_REQUIRE(f && host_p, "gc_fine_doppler_spectrum: NULL argument");
    gc_device_guard g(f->ctx->device);
    std::lock_guard<std::mutex> lk(f->ctx->mtx);
    if (f->last_bins.empty()) return gc_fail(GC_ERR_STATE, "gc_fine_doppler_spectrum: no estimate call yet");
    GC_REQUIRE(request_index >= 0 && request_index < (int)f->last_bins.size(), "gc_fine_doppler_spectrum: request %d of %d in the last call", request_index,
        (int)f->last_bins.size());
    hipStream_t st = f->ctx->stream;
    GC_HIP(hipMemcpyAsync(host_p, f->d_spec + (size_t)request_index * f->stride, sizeof(float) * f->last_bins[request_index], hipMemcpyDeviceToHost, st));
    GC_HIP(hipStreamSynchronize(st));
    return GC_OK;
}

}  // extern "C"
