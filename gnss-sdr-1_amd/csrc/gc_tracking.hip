// gc_tracking.hip -- host side of the tracking path of libgnsscorr.so:
//   * gc_trk_batch_*   : batched, HBM-resident multi-channel / multi-epoch engine
//   * gc_correlator_*  : one object per channel with the method set of the
//                        reference's Cpu_Multicorrelator_Real_Codes
//                        (src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.h:45-69)
//                        and, with complex chips, of Cpu_Multicorrelator
//                        (src/algorithms/tracking/libs/cpu_multicorrelator.h:46-64)
#include "gc_internal.h"
#include "gc_l1_batcher.h"
#include "gc_stream.h"
#include "trk_batch_plan.h"
#include "trk_kernels.h"
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <vector>

// -----------------------------------------------------------------------------
// parameter marshalling: same float arithmetic as the reference's call site
// -----------------------------------------------------------------------------
extern "C" void gc_epoch_params_fill(gc_epoch_params* p, uint64_t sample_offset,
    float rem_carrier_phase_in_rad, float phase_step_rad, float phase_rate_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips,
    int signal_length_samples)
{
    // cpu_multicorrelator_real_codes.cc:141  lv_cmake(std::cos(rem), -std::sin(rem))
    p->sample_offset = sample_offset;
    p->phase0_re = std::cos(rem_carrier_phase_in_rad);
    p->phase0_im = -std::sin(rem_carrier_phase_in_rad);
    // :145/:149  std::exp(lv_32fc_t(0.0, -phase_step_rad)), std::exp(lv_32fc_t(0.0, -phase_rate_step_rad))
    const std::complex<float> inc = std::exp(std::complex<float>(0.0f, -phase_step_rad));
    const std::complex<float> rate = std::exp(std::complex<float>(0.0f, -phase_rate_step_rad));
    p->phase_inc_re = inc.real();
    p->phase_inc_im = inc.imag();
    p->phase_rate_re = rate.real();
    p->phase_rate_im = rate.imag();
    p->rem_code_phase_chips = rem_code_phase_chips;
    p->code_phase_step_chips = code_phase_step_chips;
    p->code_phase_rate_step_chips = code_phase_rate_step_chips;
    p->n_samples = signal_length_samples;
}

static_assert(TRK_MODE_PLAIN == 0 && TRK_MODE_HD_RESAMPLER == 1 && TRK_MODE_HD_FULL == 2 && TRK_MODE_COMPLEX_CODE == 3 && TRK_MODE_SC16 == 4,
    "TRK_FORMAT_TRAITS (trk_batch_plan.h) is indexed by TRK_MODE_*");

// -----------------------------------------------------------------------------
// batched engine
// -----------------------------------------------------------------------------
struct gc_trk_batch
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    int n_channels = 0, n_taps = 0, max_code_len = 0;
    // the batch's arithmetic, all of it (TRK_FORMAT_TRAITS): TRK_MODE_PLAIN, TRK_MODE_HD_FULL (gc_trk_batch_create), TRK_MODE_COMPLEX_CODE
    // (gc_trk_batch_set_complex_codes) or TRK_MODE_SC16 (gc_trk_batch_set_16sc: Cpu_Multicorrelator_16sc arithmetic)
    int mode = TRK_MODE_PLAIN;
    bool lds_sizing = true;  // size a launch's LDS by what a slice touches (gc_trk_batch_set_slices(b, -1) turns it off: A/B timing)
    int nominal_len = 0;
    int iq_format = GC_IQ_F32;
    int forced_slices = 0;
    std::vector<gc_stream*> streams;  // per channel: the ring it reads (gc_trk_batch_set_input_stream) or NULL
    bool has_read_floor = false;
    uint64_t read_floor = 0;  // oldest absolute index run_dev launches may read (gc_trk_batch_set_read_floor)
    std::vector<TrkChan> h_chans;
    bool chans_dirty = true;
    gc_dev_buf<TrkChan> d_chans;
    gc_dev_buf<float> d_codes;  // [channel][words per chip * max_code_len]
    gc_dev_buf<float2> d_partial;
    gc_dev_buf<gc_epoch_params> d_params;
    gc_dev_buf<float2> d_out;
};

static const TrkFormatTraits& batch_traits(const gc_trk_batch* b) { return TRK_FORMAT_TRAITS[b->mode]; }

// floats of the code table of one channel in LDS: the longest code and the margin, in the words of `mode`
static int table_floats(int mode, int code_len) { return TRK_FORMAT_TRAITS[mode].words_per_chip * (code_len + TRK_LDS_MARGIN_FLOATS); }

static gc_status batch_sync_chans(gc_trk_batch* b, hipStream_t st)
{
    if (!b->chans_dirty) return GC_OK;
    GC_HIP(hipMemcpyAsync(b->d_chans, b->h_chans.data(), sizeof(TrkChan) * b->n_channels, hipMemcpyHostToDevice, st));
    // the host vector may be edited again right after this call returns
    GC_HIP(hipStreamSynchronize(st));
    b->chans_dirty = false;
    return GC_OK;
}

// A zeroed code table at the stride of `mode`, every channel pointed at its row and without a code.  The table held before is
// freed once the new one exists.
static hipError_t batch_new_table(gc_trk_batch* b, int mode)
{
    const size_t stride = (size_t)TRK_FORMAT_TRAITS[mode].words_per_chip * b->max_code_len;
    gc_dev_buf<float> table;
    const hipError_t e = table.alloc((size_t)b->n_channels * stride);
    if (e != hipSuccess) return e;
    (void)hipMemset(table, 0, sizeof(float) * (size_t)b->n_channels * stride);
    b->d_codes = std::move(table);
    for (int i = 0; i < b->n_channels; i++)
        {
            b->h_chans[i].code = b->d_codes + (size_t)i * stride;
            b->h_chans[i].code_len = 0;
        }
    b->chans_dirty = true;
    return hipSuccess;
}

// the three code setters: `fn` is the public function, which fits the batch when the format's traits name it
static gc_status batch_upload_code(gc_trk_batch* b, const char* fn, int ch, const void* code, int code_length, const float* shifts_chips)
{
    GC_REQUIRE(b && code && shifts_chips, "%s: NULL argument", fn);
    GC_REQUIRE(ch >= 0 && ch < b->n_channels, "%s: channel %d out of range", fn, ch);
    GC_REQUIRE(code_length > 0 && code_length <= b->max_code_len, "%s: code_length %d not in 1..%d", fn, code_length, b->max_code_len);
    const TrkFormatTraits& f = batch_traits(b);
    if (std::strcmp(fn, f.code_setter) != 0) return gc_fail(GC_ERR_STATE, "%s: the batch holds %s codes (%s)", fn, f.name, f.code_setter);
    gc_device_guard g(b->ctx->device);
    std::lock_guard<std::mutex> lk(b->ctx->mtx);
    GC_HIP(hipStreamSynchronize(b->ctx->stream));  // launches on the context's stream may still read the old table
    const size_t words = (size_t)f.words_per_chip;
    GC_HIP(hipMemcpy(b->d_codes + (size_t)ch * words * b->max_code_len, code, sizeof(float) * words * code_length, hipMemcpyHostToDevice));
    b->h_chans[ch].code_len = code_length;
    return gc_trk_batch_set_shifts(b, ch, shifts_chips);
}

// the two mode switches: `target` on, or back to plain float chips.  Every channel needs its code again afterwards.  Complex chips
// change the table's stride (allocated again); 16-bit chips keep it and change the samples (through the input format, which drops
// the registered inputs).
static gc_status batch_switch_format(gc_trk_batch* b, const char* fn, int target, int on)
{
    GC_REQUIRE(b, "%s: NULL argument", fn);
    if ((b->mode == target) == (on != 0)) return GC_OK;
    const int to = on ? target : TRK_MODE_PLAIN;
    if (on && b->mode != TRK_MODE_PLAIN)
        {
            if (b->mode == TRK_MODE_HD_FULL) return gc_fail(GC_ERR_STATE, "%s: the %s correlator has no high-dynamics variant", fn, TRK_FORMAT_TRAITS[to].name);
            return gc_fail(GC_ERR_STATE, "%s: the batch holds %s codes", fn, batch_traits(b).name);
        }
    GC_REQUIRE(table_floats(to, b->max_code_len) <= TRK_LDS_TABLE_FLOATS, "%s: max_code_length %d too long for %s chips (max %d)", fn, b->max_code_len,
        TRK_FORMAT_TRAITS[to].name, TRK_LDS_TABLE_FLOATS / TRK_FORMAT_TRAITS[to].words_per_chip - TRK_LDS_MARGIN_FLOATS);
    if (target == TRK_MODE_COMPLEX_CODE)
        {
            gc_device_guard g(b->ctx->device);
            std::lock_guard<std::mutex> lk(b->ctx->mtx);
            GC_HIP(hipStreamSynchronize(b->ctx->stream));
            GC_HIP(batch_new_table(b, to));
        }
    else
        {
            b->mode = TRK_MODE_PLAIN;  // the format setter refuses anything but cshort to a 16-bit batch
            const gc_status s = gc_trk_batch_set_input_format(b, on ? GC_IQ_I16 : GC_IQ_F32);
            if (s != GC_OK) return s;
            for (auto& c : b->h_chans) c.code_len = 0;
            b->chans_dirty = true;
        }
    b->mode = to;
    return GC_OK;
}

extern "C" {

gc_status gc_trk_batch_create(gc_ctx* ctx, int n_channels, int n_taps, int max_code_length, int high_dyn,
    gc_trk_batch** out)
{
    GC_REQUIRE(ctx && out, "gc_trk_batch_create: NULL argument");
    *out = nullptr;
    GC_REQUIRE(n_channels > 0, "gc_trk_batch_create: n_channels must be > 0");
    GC_REQUIRE(n_taps >= 1 && n_taps <= GC_MAX_TAPS, "gc_trk_batch_create: n_taps must be in 1..%d", GC_MAX_TAPS);
    GC_REQUIRE(max_code_length > 0 && max_code_length + TRK_LDS_MARGIN_FLOATS <= TRK_LDS_TABLE_FLOATS,
        "gc_trk_batch_create: max_code_length must be in 1..%d", TRK_LDS_TABLE_FLOATS - TRK_LDS_MARGIN_FLOATS);
    gc_device_guard g(ctx->device);
    std::unique_ptr<gc_trk_batch> b(new gc_trk_batch());
    b->ctx = ctx;
    b->ctx_ref.bind(ctx);
    b->n_channels = n_channels;
    b->n_taps = n_taps;
    b->max_code_len = max_code_length;
    b->mode = high_dyn ? TRK_MODE_HD_FULL : TRK_MODE_PLAIN;
    b->h_chans.assign(n_channels, TrkChan{});
    b->streams.assign(n_channels, nullptr);
    if (b->d_chans.alloc(n_channels) != hipSuccess || batch_new_table(b.get(), b->mode) != hipSuccess)
        return gc_fail(GC_ERR_HIP, "gc_trk_batch_create: hipMalloc failed");
    *out = b.release();
    return GC_OK;
}

gc_status gc_trk_batch_destroy(gc_trk_batch* b)
{
    if (!b) return GC_OK;
    gc_device_guard g(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    for (gc_stream* r : b->streams)
        if (r) gc_stream_drop(r);
    delete b;
    return GC_OK;
}

gc_status gc_trk_batch_set_shifts(gc_trk_batch* b, int ch, const float* shifts_chips)
{
    GC_REQUIRE(b && shifts_chips, "gc_trk_batch_set_shifts: NULL argument");
    GC_REQUIRE(ch >= 0 && ch < b->n_channels, "gc_trk_batch_set_shifts: channel %d out of range", ch);
    for (int t = 0; t < b->n_taps; t++) b->h_chans[ch].shifts[t] = shifts_chips[t];
    b->chans_dirty = true;
    return GC_OK;
}

gc_status gc_trk_batch_set_code(gc_trk_batch* b, int ch, const float* code, int code_length, const float* shifts_chips)
{
    return batch_upload_code(b, "gc_trk_batch_set_code", ch, code, code_length, shifts_chips);
}

gc_status gc_trk_batch_set_code_complex(gc_trk_batch* b, int ch, const float* code_iq, int code_length, const float* shifts_chips)
{
    return batch_upload_code(b, "gc_trk_batch_set_code_complex", ch, code_iq, code_length, shifts_chips);
}

gc_status gc_trk_batch_set_code_16sc(gc_trk_batch* b, int ch, const int16_t* code_iq, int code_length, const float* shifts_chips)
{
    return batch_upload_code(b, "gc_trk_batch_set_code_16sc", ch, code_iq, code_length, shifts_chips);
}

gc_status gc_trk_batch_set_complex_codes(gc_trk_batch* b, int on) { return batch_switch_format(b, "gc_trk_batch_set_complex_codes", TRK_MODE_COMPLEX_CODE, on); }

gc_status gc_trk_batch_set_16sc(gc_trk_batch* b, int on) { return batch_switch_format(b, "gc_trk_batch_set_16sc", TRK_MODE_SC16, on); }

gc_status gc_trk_batch_set_input_dev(gc_trk_batch* b, int ch, const void* dev_iq, uint64_t n_samples)
{
    GC_REQUIRE(b && dev_iq, "gc_trk_batch_set_input_dev: NULL argument");
    GC_REQUIRE(ch >= 0 && ch < b->n_channels, "gc_trk_batch_set_input_dev: channel %d out of range", ch);
    const uintptr_t es = gc_iq_sample_bytes(b->iq_format);
    GC_REQUIRE((reinterpret_cast<uintptr_t>(dev_iq) % es) == 0, "gc_trk_batch_set_input_dev: IQ pointer must be aligned to one sample (%d bytes)", (int)es);
    b->h_chans[ch].iq = dev_iq;
    b->h_chans[ch].n_iq = n_samples;
    b->h_chans[ch].ring_len = 0;
    if (b->streams[ch]) gc_stream_drop(b->streams[ch]);
    b->streams[ch] = nullptr;
    b->chans_dirty = true;
    return GC_OK;
}

gc_status gc_trk_batch_set_input_stream(gc_trk_batch* b, int ch, gc_stream* s)
{
    GC_REQUIRE(b && s, "gc_trk_batch_set_input_stream: NULL argument");
    GC_REQUIRE(ch >= 0 && ch < b->n_channels, "gc_trk_batch_set_input_stream: channel %d out of range", ch);
    GC_REQUIRE(s->ctx->device == b->ctx->device, "gc_trk_batch_set_input_stream: the stream lives on another GPU");
    GC_REQUIRE(s->iq_format == b->iq_format, "gc_trk_batch_set_input_stream: stream format %d, batch format %d", s->iq_format, b->iq_format);
    gc_stream_keep(s);
    if (b->streams[ch]) gc_stream_drop(b->streams[ch]);
    b->h_chans[ch].iq = s->d_ring;
    b->h_chans[ch].n_iq = ~0ull;
    b->h_chans[ch].ring_len = (unsigned)s->capacity;
    b->streams[ch] = s;
    b->chans_dirty = true;
    return GC_OK;
}

gc_status gc_trk_batch_set_read_floor(gc_trk_batch* b, uint64_t oldest_index_read)
{
    GC_REQUIRE(b, "gc_trk_batch_set_read_floor: NULL argument");
    b->has_read_floor = true;
    b->read_floor = oldest_index_read;
    return GC_OK;
}

gc_status gc_trk_batch_set_input_format(gc_trk_batch* b, int iq_format)
{
    GC_REQUIRE(b, "gc_trk_batch_set_input_format: NULL argument");
    GC_REQUIRE(iq_format == GC_IQ_F32 || iq_format == GC_IQ_I16 || iq_format == GC_IQ_I8, "gc_trk_batch_set_input_format: unknown format %d", iq_format);
    if (!(batch_traits(b).iq_formats & (1u << iq_format))) return gc_fail(GC_ERR_STATE, "gc_trk_batch_set_input_format: 16-bit mode correlates lv_16sc_t input only");
    if (iq_format != b->iq_format)
        {
            // pointers registered so far were checked against the old sample size
            for (auto& c : b->h_chans)
                {
                    c.iq = nullptr;
                    c.n_iq = 0;
                    c.ring_len = 0;
                }
            for (gc_stream*& r : b->streams)
                {
                    if (r) gc_stream_drop(r);
                    r = nullptr;
                }
            b->chans_dirty = true;
        }
    b->iq_format = iq_format;
    return GC_OK;
}

// engine tuning knobs (not part of the reference surface)
gc_status gc_trk_batch_set_nominal_length(gc_trk_batch* b, int n_samples)
{
    GC_REQUIRE(b, "gc_trk_batch_set_nominal_length: NULL argument");
    b->nominal_len = n_samples;
    return GC_OK;
}

gc_status gc_trk_batch_set_slices(gc_trk_batch* b, int n_slices)
{
    GC_REQUIRE(b && n_slices >= -1 && n_slices <= 1024, "gc_trk_batch_set_slices: bad argument");
    b->lds_sizing = n_slices >= 0;
    b->forced_slices = n_slices > 0 ? n_slices : 0;
    return GC_OK;
}

// distinct rings the batch reads
static std::vector<gc_stream*> batch_streams(const gc_trk_batch* b)
{
    std::vector<gc_stream*> v;
    for (gc_stream* s : b->streams)
        if (s && std::find(v.begin(), v.end(), s) == v.end()) v.push_back(s);
    return v;
}

// floors / ends: oldest absolute index the launch reads from each ring of batch_streams(b) and one past the newest (NULL: unknown).
// The reader slots are reserved BEFORE the residency check and the enqueue, so a push on the producer's thread cannot evict
// what this launch was validated for (gc_reader_table.h).
static gc_status batch_launch(gc_trk_batch* b, int n_epochs, const gc_epoch_params* dev_params, void* dev_out,
    hipStream_t st, int max_len, const std::vector<uint64_t>* floors = nullptr, const std::vector<uint64_t>* ends = nullptr, float max_step = 0.0f)
{
    for (int i = 0; i < b->n_channels; i++)
        {
            GC_REQUIRE(b->h_chans[i].code_len > 0, "gc_trk_batch_run: channel %d has no code (gc_trk_batch_set_code)", i);
            GC_REQUIRE(b->h_chans[i].iq != nullptr, "gc_trk_batch_run: channel %d has no input (gc_trk_batch_set_input_dev)", i);
        }
    gc_status s = batch_sync_chans(b, st);
    if (s != GC_OK) return s;
    // slices per job and LDS of the launch (trk_batch_plan.h)
    static_assert(sizeof(TrkChan) % 4 == 0, "the plan walks the channel array in 4-byte words");
    const TrkChan& c0 = b->h_chans[0];
    const TrkBatchPlan plan = trk_batch_plan(b->forced_slices, b->lds_sizing, b->n_channels, n_epochs, b->ctx->n_cus, b->mode, trk_small_window_ok(b->mode, b->iq_format),
        max_len > 0 ? max_len : b->nominal_len, &c0.code_len, c0.shifts, (int)(sizeof(TrkChan) / 4), b->n_taps, max_step, table_floats(b->mode, b->max_code_len));
    if (plan.n_slices > 1)
        {
            const size_t need = (size_t)b->n_channels * n_epochs * plan.n_slices * b->n_taps;
            if (need > b->d_partial.cap)
                {
                    GC_HIP(hipStreamSynchronize(st));
                    GC_HIP(b->d_partial.reserve(need));
                }
        }
    const std::vector<gc_stream*> rings = batch_streams(b);
    gc_stream_read_set reads(st);
    for (size_t i = 0; i < rings.size(); i++)
        {
            // later pushes may evict everything below the floor while this launch is still running; the newest push must have landed
            const uint64_t floor = (floors && (*floors)[i] != ~0ull) ? (*floors)[i] : b->has_read_floor ? b->read_floor : GC_STREAM_FLOOR_OLDEST;
            const gc_status rs = reads.add(rings[i], floor);
            if (rs != GC_OK) return rs;
            const gc_stream_ticket& t = reads.ticket((int)i);
            // a floor above the head protects nothing: a later push would evict, unhindered, whatever the records of this launch read
            if (floor != GC_STREAM_FLOOR_OLDEST && floor > t.head)
                return gc_fail(GC_ERR_INVALID, "gc_trk_batch_run: the read floor %llu lies above the stream's resident samples [%llu, %llu)",
                    (unsigned long long)floor, (unsigned long long)t.oldest, (unsigned long long)t.head);
            if (ends && (*ends)[i] > t.head)
                return gc_fail(GC_ERR_INVALID, "gc_trk_batch_run: a window ends at sample %llu, the stream's resident samples are [%llu, %llu)",
                    (unsigned long long)(*ends)[i], (unsigned long long)t.oldest, (unsigned long long)t.head);
        }
    hipError_t e = trk_launch(b->n_taps, b->mode, b->iq_format, st, b->d_chans, dev_params, static_cast<float2*>(dev_out), b->d_partial,
        b->n_channels, n_epochs, plan.n_slices, plan.lds_floats, true);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "tracking kernel launch failed: %s", hipGetErrorString(e));
    return reads.commit();
}

gc_status gc_trk_batch_run_dev(gc_trk_batch* b, int n_epochs, const gc_epoch_params* dev_params, void* dev_out, void* stream)
{
    GC_REQUIRE(b && dev_params && dev_out, "gc_trk_batch_run_dev: NULL argument");
    GC_REQUIRE(n_epochs > 0, "gc_trk_batch_run_dev: n_epochs must be > 0");
    gc_device_guard g(b->ctx->device);
    std::lock_guard<std::mutex> lk(b->ctx->mtx);
    return batch_launch(b, n_epochs, dev_params, dev_out, gc_pick_stream(b->ctx, stream), 0);
}

gc_status gc_trk_batch_run(gc_trk_batch* b, int n_epochs, const gc_epoch_params* host_params, float* host_out)
{
    GC_REQUIRE(b && host_params && host_out, "gc_trk_batch_run: NULL argument");
    GC_REQUIRE(n_epochs > 0, "gc_trk_batch_run: n_epochs must be > 0");
    gc_device_guard g(b->ctx->device);
    std::lock_guard<std::mutex> lk(b->ctx->mtx);
    const size_t jobs = (size_t)b->n_channels * n_epochs;
    int max_len = 0;
    float max_step = 0.0f;
    const std::vector<gc_stream*> rings = batch_streams(b);
    std::vector<uint64_t> floors(rings.size(), ~0ull), ends(rings.size(), 0);
    for (size_t j = 0; j < jobs; j++)
        {
            const gc_epoch_params& p = host_params[j];
            const TrkChan& c = b->h_chans[j / n_epochs];
            GC_REQUIRE(p.n_samples >= 0, "gc_trk_batch_run: job %zu has negative n_samples", j);
            if (gc_stream* r = b->streams[j / n_epochs])
                {
                    uint64_t oldest = 0, head = 0;
                    gc_stream_info(r, &oldest, &head, nullptr);
                    GC_REQUIRE((uint64_t)p.n_samples <= r->mirror, "gc_trk_batch_run: job %zu is longer than the stream's max_window %llu", j,
                        (unsigned long long)r->mirror);
                    // (head - sample_offset, not sample_offset + n_samples: the sum wraps for an offset near 2^64)
                    GC_REQUIRE(p.sample_offset >= oldest && p.sample_offset <= head && (uint64_t)p.n_samples <= head - p.sample_offset,
                        "gc_trk_batch_run: job %zu window [%llu, +%d) is not inside the stream's resident samples [%llu, %llu)", j,
                        (unsigned long long)p.sample_offset, p.n_samples, (unsigned long long)oldest, (unsigned long long)head);
                    const size_t ri = std::find(rings.begin(), rings.end(), r) - rings.begin();
                    floors[ri] = std::min(floors[ri], p.sample_offset);
                    ends[ri] = std::max(ends[ri], p.sample_offset + (uint64_t)p.n_samples);
                }
            else
                {
                    GC_REQUIRE(p.sample_offset <= c.n_iq && (uint64_t)p.n_samples <= c.n_iq - p.sample_offset,
                        "gc_trk_batch_run: job %zu window [%llu, +%d) exceeds the channel's %llu samples", j,
                        (unsigned long long)p.sample_offset, p.n_samples, (unsigned long long)c.n_iq);
                }
            if (p.n_samples > max_len) max_len = p.n_samples;
            if (p.n_samples > 0) max_step = std::max(max_step, std::fabs(p.code_phase_step_chips) + std::fabs(p.code_phase_rate_step_chips) * (float)p.n_samples);
        }
    hipStream_t st = b->ctx->stream;
    GC_HIP(b->d_params.reserve(jobs));
    GC_HIP(b->d_out.reserve(jobs * b->n_taps));
    GC_HIP(hipMemcpyAsync(b->d_params, host_params, jobs * sizeof(gc_epoch_params), hipMemcpyHostToDevice, st));
    gc_status s = batch_launch(b, n_epochs, b->d_params, b->d_out, st, max_len, &floors, &ends, max_step);
    if (s != GC_OK) return s;
    // n_taps results per job: complex floats, or lv_16sc_t (4 bytes) in 16-bit mode
    GC_HIP(hipMemcpyAsync(host_out, b->d_out, jobs * b->n_taps * batch_traits(b).out_bytes, hipMemcpyDeviceToHost, st));
    GC_HIP(hipStreamSynchronize(st));
    return GC_OK;
}

}  // extern "C"

// -----------------------------------------------------------------------------
// Level 1: Cpu_Multicorrelator_Real_Codes image
// -----------------------------------------------------------------------------
struct gc_correlator
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    bool use_high_dynamics_resampler = true;  // reference ctor default (cpu_multicorrelator_real_codes.cc:49)
    int max_len = 0, n_corr = 0;
    // retained caller pointers (the reference stores pointers, .cc:79-98)
    const float* local_code_in = nullptr;
    float* shifts_chips = nullptr;
    int code_length_chips = 0;
    // what local_code_in points at: TRK_MODE_PLAIN float chips (Cpu_Multicorrelator_Real_Codes), TRK_MODE_COMPLEX_CODE (re, im) float
    // pairs (Cpu_Multicorrelator), or TRK_MODE_SC16 (re, im) int16 pairs with int16 input/output (Cpu_Multicorrelator_16sc)
    int code_mode = TRK_MODE_PLAIN;
    float* corr_out = nullptr;      // n_corr complex floats, or n_corr lv_16sc_t
    const float* sig_in = nullptr;  // complex floats, or lv_16sc_t
    int io_bytes = 8;               // of one sample of sig_in and of one result in corr_out: 8 (complex float) or 4 (lv_16sc_t)
    struct Staging
    {
        TrkChan chan;
        gc_epoch_params params;
    };
    // what init() makes and free() drops
    struct Work
    {
        bool inited = false;
        gc_dev_buf<float2> d_sig;
        gc_dev_buf<float> d_code;
        std::vector<float> code_shadow;  // last uploaded code contents
        gc_mapped_buf<Staging> h_stage;
        gc_dev_buf<Staging> d_stage;
        gc_dev_buf<float2> d_out;
        gc_mapped_buf<float2> h_out;
        gc_dev_buf<float2> d_partial;
        // zero-copy path: the window is copied into page-locked, device-mapped host memory and the kernel reads it (and the
        // descriptor) over PCIe and writes the result back the same way -- one launch and one synchronisation per call
        // instead of three copies around the launch
        bool zero_copy = true;
        gc_mapped_buf<char> h_sig;
    } w;
    static constexpr int partial_slices = 64;
};

// -----------------------------------------------------------------------------
// Level-1 epoch batcher: queue / lanes / waiters / window sharing / host-buffer registry live in gc_l1_batcher.h (header-only,
// no HIP types, exercised on the CPU under ThreadSanitizer by tests/l1_batcher_selftest.cpp); this is its HIP backend: a lane
// is a HIP stream with page-locked, device-mapped descriptor / result arrays, a launch is ONE trk_launch over the batch.
// -----------------------------------------------------------------------------
// host (mapped / registered) -> HBM copy of a shared window on the lane's stream: a kernel launch costs the calling thread
// less than a hipMemcpyAsync, and the tracking kernel behind it needs no other ordering
__global__ void l1_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16, int tail_bytes)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
    if (blockIdx.x == 0 && (int)threadIdx.x < tail_bytes)  // never reads past the end of the caller's memory
        reinterpret_cast<char*>(dst + n16)[threadIdx.x] = reinterpret_cast<const char*>(src + n16)[threadIdx.x];
}

struct L1HipBackend
{
    typedef TrkChan Chan;
    typedef gc_epoch_params Params;
    static constexpr int MAX_SLICES = 64;
    struct Lane
    {
        hipStream_t stream = nullptr;
        gc_mapped_buf<TrkChan> h_chans;  // page-locked, device-mapped arrays of maxb entries
        gc_mapped_buf<gc_epoch_params> h_params;
        gc_mapped_buf<char> h_out;
        gc_dev_buf<float2> d_partial;
        gc_dev_buf<char> d_span;  // windows shared by several requests of a batch, copied once
        size_t span_cap = 0;      // d_span.cap, where the batcher reads it
        gc_mapped_buf<char> h_span;     // where the leader stages unions of overlapping unregistered windows
        const char* dv_span = nullptr;  // h_span.dev, where the batcher reads it
    };
    int device = 0;
    struct Guard
    {
        gc_device_guard g;
        explicit Guard(L1HipBackend& b) : g(b.device) {}
    };
    bool lane_init(Lane& l, int maxb, int max_out_bytes)
    {
        const bool ok = hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) == hipSuccess && l.h_chans.alloc(maxb) == hipSuccess &&
                        l.h_params.alloc(maxb) == hipSuccess && l.h_out.alloc((size_t)max_out_bytes * maxb) == hipSuccess &&
                        l.d_partial.alloc((size_t)GC_MAX_TAPS * MAX_SLICES * maxb) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    }
    void lane_free(Lane& l)
    {
        if (l.stream)
            {
                (void)hipStreamSynchronize(l.stream);
                (void)hipStreamDestroy(l.stream);
            }
        l = Lane();
    }
    // grows the lane's shared-window buffer (the lane is idle: nothing reads the old one)
    bool span_reserve(Lane& lane, size_t need)
    {
        if (need <= lane.span_cap) return true;
        const bool ok = lane.d_span.reserve((need + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1)) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        lane.span_cap = lane.d_span.cap;
        return ok;
    }
    bool hspan_reserve(Lane& lane, size_t need)
    {
        if (need <= lane.h_span.cap) return true;
        const bool ok = lane.h_span.reserve((need + ((size_t)4 << 20)) & ~(((size_t)1 << 20) - 1)) == hipSuccess;  // page-locking is slow: grow in large steps
        if (!ok) (void)hipGetLastError();
        lane.dv_span = lane.h_span.dev;
        return ok;
    }
    // src_dev_view and dst are 16-byte aligned
    int copy(Lane& lane, const void* src_dev_view, void* dst, size_t bytes)
    {
        const size_t n16 = bytes / 16;
        const unsigned blocks = (unsigned)std::min<size_t>(256, (n16 + 255) / 256);
        hipLaunchKernelGGL(l1_copy_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, lane.stream, static_cast<const uint4*>(src_dev_view), static_cast<uint4*>(dst), n16,
            (int)(bytes - n16 * 16));
        return (int)hipGetLastError();
    }
    template <class Rq>
    int launch(Lane& lane, const Rq& k, int B, int lds_floats)
    {
        return (int)trk_launch(k.n_corr, k.mode, k.fmt, lane.stream, lane.h_chans.dev, lane.h_params.dev, reinterpret_cast<float2*>(lane.h_out.dev), lane.d_partial, B, 1,
            k.n_slices, lds_floats, false);
    }
    int wait(Lane& lane) { return (int)hipStreamSynchronize(lane.stream); }
    int oom_error() const { return (int)hipErrorOutOfMemory; }
    const char* error_string(int e) const { return hipGetErrorString((hipError_t)e); }
    void host_unregister(const void* base) { (void)hipHostUnregister(const_cast<void*>(base)); }
};

typedef gc_l1_batcher_t<L1HipBackend> gc_l1_batcher;
typedef gc_l1_batcher::Request L1Request;

// the backend lives beside the batcher that points at it
struct L1Holder
{
    L1HipBackend be;
    gc_l1_batcher* bat = nullptr;
    ~L1Holder() { delete bat; }
};

static void l1_batcher_free(void* p)
{
    L1Holder* h = static_cast<L1Holder*>(p);
    gc_device_guard g(h->be.device);
    delete h;
}

// the context's batcher (created by the first caller; NULL if its buffers cannot be set up: callers then use the direct path)
static gc_l1_batcher* l1_batcher_get(gc_ctx* ctx)
{
    auto usable = [](void* p) -> gc_l1_batcher* {
        L1Holder* h = static_cast<L1Holder*>(p);
        return h->bat->ok() ? h->bat : nullptr;
    };
    if (void* p = ctx->l1_batcher.load(std::memory_order_acquire)) return usable(p);
    std::lock_guard<std::mutex> lk(ctx->mtx);
    if (void* p = ctx->l1_batcher.load(std::memory_order_acquire)) return usable(p);
    L1Holder* h = new L1Holder();
    h->be.device = ctx->device;
    h->bat = new gc_l1_batcher(&h->be, (int)(sizeof(float2) * GC_MAX_TAPS));
    if (const char* e = gc_exp_env("GNSSCORR_L1_SECOND_LANE")) h->bat->min_second_lane = std::max(1, std::atoi(e));
    ctx->l1_batcher_free = &l1_batcher_free;
    ctx->l1_batcher.store(h, std::memory_order_release);
    return usable(h);
}

static gc_status l1_submit(gc_l1_batcher* b, L1Request* rq, void* own_pinned, const void* own_pinned_dev)
{
    if (b->submit(rq, own_pinned, own_pinned_dev) != gc_l1_batcher::ST_OK) return gc_fail(GC_ERR_HIP, "%s", rq->err);
    return GC_OK;
}

// the reference's scalar arguments of one call
struct L1Call
{
    float rem_carr, phase_step, phase_rate_step, rem_code, code_step, code_rate_step;
    int N;
};

// descriptor and parameter record of a level-1 call that reads its window at `iq` (NULL: the batcher decides -- registered memory,
// the call's page-locked copy, or a shared HBM copy)
static void correlator_fill(const gc_correlator* c, const L1Call& a, const void* iq, TrkChan* chan, gc_epoch_params* params)
{
    std::memset(chan, 0, sizeof *chan);
    chan->iq = iq;
    chan->n_iq = (unsigned long long)a.N;
    chan->code = c->w.d_code;
    chan->code_len = c->code_length_chips;
    for (int t = 0; t < c->n_corr; t++) chan->shifts[t] = c->shifts_chips[t];
    gc_epoch_params_fill(params, 0, a.rem_carr, a.phase_step, a.phase_rate_step, a.rem_code, a.code_step, a.code_rate_step, a.N);
}

static gc_status correlator_run(gc_correlator* c, int mode, const L1Call& a)
{
    GC_REQUIRE(c, "correlator: NULL handle");
    gc_correlator::Work& w = c->w;
    const int N = a.N;
    if (!w.inited) return gc_fail(GC_ERR_STATE, "correlator: init() has not been called");
    if (!c->local_code_in || !c->shifts_chips) return gc_fail(GC_ERR_STATE, "correlator: set_local_code_and_taps() has not been called");
    if (!c->corr_out || !c->sig_in) return gc_fail(GC_ERR_STATE, "correlator: set_input_output_vectors() has not been called");
    GC_REQUIRE(N >= 0 && N <= c->max_len, "correlator: signal_length_samples %d exceeds init() capacity %d", N, c->max_len);
    // the overload's arithmetic against the code and the vectors that were set: the high-dynamics modes correlate real chips
    const TrkFormatTraits& f = TRK_FORMAT_TRAITS[mode];
    if ((mode == TRK_MODE_HD_RESAMPLER || mode == TRK_MODE_HD_FULL ? TRK_MODE_PLAIN : mode) != c->code_mode)
        return gc_fail(GC_ERR_STATE, "correlator: the local code is %s; use the matching setters and Carrier_wipeoff overload", TRK_FORMAT_TRAITS[c->code_mode].name);
    if (f.out_bytes != c->io_bytes) return gc_fail(GC_ERR_STATE, "correlator: input/output vectors and local code must both be 16-bit or both float");
    const int L = c->code_length_chips;
    GC_REQUIRE(L > 0 && table_floats(mode, L) <= TRK_LDS_TABLE_FLOATS, "correlator: code_length_chips %d not supported (max %d)", L,
        TRK_LDS_TABLE_FLOATS / f.words_per_chip - TRK_LDS_MARGIN_FLOATS);
    const int iq_format = c->io_bytes == 4 ? GC_IQ_I16 : GC_IQ_F32;
    gc_device_guard g(c->ctx->device);
    static const bool batching = [] {
        const char* e = gc_exp_env("GNSSCORR_L1_BATCH");  // 0: every call is its own launch under the context mutex (round-1 behaviour)
        return !(e && e[0] == '0');
    }();
    gc_l1_batcher* bat = (w.zero_copy && batching) ? l1_batcher_get(c->ctx) : nullptr;
    // The object's own buffers (code table, page-locked window, staging) belong to the calling thread -- one correlator per
    // channel thread, like the reference's -- so with the batcher only the rare code upload takes the context mutex.
    std::unique_lock<std::mutex> lk(c->ctx->mtx, std::defer_lock);
    if (!bat) lk.lock();
    hipStream_t st = c->ctx->stream;
    const size_t LF = (size_t)f.words_per_chip * L;  // floats in the code table
    // code table: the caller's buffer is re-read on every call like the reference
    // does; it is re-uploaded only when its contents changed
    if (LF > w.d_code.cap || w.code_shadow.size() != LF || std::memcmp(w.code_shadow.data(), c->local_code_in, sizeof(float) * LF) != 0)
        {
            if (bat) lk.lock();
            GC_HIP(w.d_code.reserve(LF));
            // the previous upload may still be in flight from the pageable shadow buffer
            GC_HIP(hipStreamSynchronize(st));
            w.code_shadow.assign(c->local_code_in, c->local_code_in + LF);
            GC_HIP(hipMemcpyAsync(w.d_code, w.code_shadow.data(), sizeof(float) * LF, hipMemcpyHostToDevice, st));
            if (bat)
                {
                    GC_HIP(hipStreamSynchronize(st));  // batches run on the lanes' streams: the table must have landed
                    lk.unlock();
                }
        }
    const size_t sig_bytes = (size_t)c->io_bytes * N;
    const bool zc = w.zero_copy;
    if (N > 0 && !bat)
        {
            if (zc)
                std::memcpy(w.h_sig, c->sig_in, sig_bytes);
            else
                GC_HIP(hipMemcpyAsync(w.d_sig, c->sig_in, sig_bytes, hipMemcpyHostToDevice, st));
        }
    static const int one_wg_max = [] {
        const char* e = gc_exp_env("GNSSCORR_L1_ONE_WG_MAX");  // tuning knob: windows up to this length run in one workgroup
        return e ? std::atoi(e) : 2048;
    }();
    const int n_slices = trk_level1_slices(N, one_wg_max, gc_correlator::partial_slices);
    const size_t out_bytes = (size_t)c->io_bytes * c->n_corr;
    if (bat)
        {
            L1Request rq;
            correlator_fill(c, a, nullptr, &rq.chan, &rq.params);
            rq.n_corr = c->n_corr;
            rq.mode = mode;
            rq.fmt = iq_format;
            rq.n_slices = n_slices;
            rq.lds_floats = table_floats(mode, L);
            rq.host_sig = reinterpret_cast<const char*>(c->sig_in);
            rq.sig_bytes = sig_bytes;
            rq.out_host = c->corr_out;
            rq.out_bytes = out_bytes;
            return l1_submit(bat, &rq, w.h_sig, w.h_sig.dev);
        }
    gc_correlator::Staging* s = w.h_stage;
    correlator_fill(c, a, zc ? static_cast<const void*>(w.h_sig.dev) : w.d_sig.get(), &s->chan, &s->params);
    if (!zc) GC_HIP(hipMemcpyAsync(w.d_stage, s, sizeof *s, hipMemcpyHostToDevice, st));
    gc_correlator::Staging* stage_dev = zc ? w.h_stage.dev : w.d_stage.get();
    hipError_t e = trk_launch(c->n_corr, mode, iq_format, st, &stage_dev->chan, &stage_dev->params, zc ? w.h_out.dev : w.d_out.get(), w.d_partial, 1, 1, n_slices,
        table_floats(mode, L), false);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "tracking kernel launch failed: %s", hipGetErrorString(e));
    if (!zc) GC_HIP(hipMemcpyAsync(w.h_out, w.d_out, out_bytes, hipMemcpyDeviceToHost, st));
    GC_HIP(hipStreamSynchronize(st));
    std::memcpy(c->corr_out, w.h_out, out_bytes);
    return GC_OK;
}

// the three code setters: pointers retained, 4-byte words per chip by `code_mode`
static gc_status correlator_set_code(gc_correlator* c, const char* fn, int code_mode, int code_length_chips, const void* local_code_in, float* shifts_chips)
{
    GC_REQUIRE(c, "%s: NULL handle", fn);
    c->local_code_in = static_cast<const float*>(local_code_in);  // compared and uploaded as words
    c->shifts_chips = shifts_chips;
    c->code_length_chips = code_length_chips;
    c->code_mode = code_mode;
    return GC_OK;
}

static gc_status correlator_set_vectors(gc_correlator* c, const char* fn, int io_bytes, void* corr_out, const void* sig_in)
{
    GC_REQUIRE(c, "%s: NULL handle", fn);
    c->sig_in = static_cast<const float*>(sig_in);
    c->corr_out = static_cast<float*>(corr_out);
    c->io_bytes = io_bytes;
    return GC_OK;
}

extern "C" {

gc_status gc_correlator_create(gc_ctx* ctx, gc_correlator** out)
{
    GC_REQUIRE(ctx && out, "gc_correlator_create: NULL argument");
    gc_correlator* c = new gc_correlator();
    c->ctx = ctx;
    c->ctx_ref.bind(ctx);
    *out = c;
    return GC_OK;
}

gc_status gc_correlator_destroy(gc_correlator* c)
{
    if (!c) return GC_OK;
    gc_device_guard g(c->ctx->device);
    (void)hipStreamSynchronize(c->ctx->stream);
    delete c;
    return GC_OK;
}

gc_status gc_correlator_set_high_dynamics_resampler(gc_correlator* c, int use_high_dynamics_resampler)
{
    GC_REQUIRE(c, "gc_correlator_set_high_dynamics_resampler: NULL handle");
    c->use_high_dynamics_resampler = use_high_dynamics_resampler != 0;
    return GC_OK;
}

gc_status gc_correlator_init(gc_correlator* c, int max_signal_length_samples, int n_correlators)
{
    GC_REQUIRE(c, "gc_correlator_init: NULL handle");
    GC_REQUIRE(max_signal_length_samples > 0, "gc_correlator_init: max_signal_length_samples must be > 0");
    GC_REQUIRE(n_correlators >= 1 && n_correlators <= GC_MAX_TAPS, "gc_correlator_init: n_correlators must be in 1..%d", GC_MAX_TAPS);
    gc_device_guard g(c->ctx->device);
    std::lock_guard<std::mutex> lk(c->ctx->mtx);
    (void)hipStreamSynchronize(c->ctx->stream);
    c->w = gc_correlator::Work();  // an initialised object is released first
    gc_correlator::Work& w = c->w;
    c->max_len = max_signal_length_samples;
    c->n_corr = n_correlators;
    const size_t n_sig = (size_t)max_signal_length_samples + 2;
    GC_HIP(w.d_sig.alloc(n_sig));
    GC_HIP(w.d_stage.alloc(1));
    GC_HIP(w.d_out.alloc(GC_MAX_TAPS));
    GC_HIP(w.d_partial.alloc((size_t)GC_MAX_TAPS * gc_correlator::partial_slices));
    GC_HIP(w.h_stage.alloc_host(1));
    GC_HIP(w.h_out.alloc_host(GC_MAX_TAPS));
    {
        const char* e = gc_exp_env("GNSSCORR_L1_COPY");  // 1: stage the window in HBM with explicit copies instead
        w.zero_copy = !(e && e[0] == '1');
    }
    if (w.zero_copy)
        {
            hipError_t e = w.h_sig.alloc(sizeof(float2) * n_sig);
            if (e == hipSuccess) e = w.h_stage.map();
            if (e == hipSuccess) e = w.h_out.map();
            if (e != hipSuccess)
                {
                    (void)hipGetLastError();
                    w.zero_copy = false;  // the copy path needs none of these
                }
        }
    w.inited = true;
    return GC_OK;
}

gc_status gc_correlator_set_local_code_and_taps(gc_correlator* c, int code_length_chips, const float* local_code_in,
    float* shifts_chips)
{
    return correlator_set_code(c, "gc_correlator_set_local_code_and_taps", TRK_MODE_PLAIN, code_length_chips, local_code_in, shifts_chips);
}

gc_status gc_correlator_set_local_code_and_taps_complex(gc_correlator* c, int code_length_chips, const float* local_code_in_iq,
    float* shifts_chips)
{
    return correlator_set_code(c, "gc_correlator_set_local_code_and_taps_complex", TRK_MODE_COMPLEX_CODE, code_length_chips, local_code_in_iq, shifts_chips);
}

gc_status gc_correlator_set_local_code_and_taps_16sc(gc_correlator* c, int code_length_chips, const int16_t* local_code_in_iq,
    float* shifts_chips)
{
    return correlator_set_code(c, "gc_correlator_set_local_code_and_taps_16sc", TRK_MODE_SC16, code_length_chips, local_code_in_iq, shifts_chips);
}

gc_status gc_correlator_set_input_output_vectors_16sc(gc_correlator* c, int16_t* corr_out, const int16_t* sig_in)
{
    return correlator_set_vectors(c, "gc_correlator_set_input_output_vectors_16sc", 4, corr_out, sig_in);
}

gc_status gc_correlator_set_input_output_vectors(gc_correlator* c, float* corr_out, const float* sig_in)
{
    return correlator_set_vectors(c, "gc_correlator_set_input_output_vectors", 8, corr_out, sig_in);
}

gc_status gc_correlator_carrier_wipeoff_multicorrelator_resampler(gc_correlator* c,
    float rem_carrier_phase_in_rad, float phase_step_rad, float phase_rate_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips,
    int signal_length_samples)
{
    GC_REQUIRE(c, "gc_correlator_carrier_wipeoff_multicorrelator_resampler: NULL handle");
    const int mode = c->use_high_dynamics_resampler ? TRK_MODE_HD_FULL : TRK_MODE_PLAIN;
    return correlator_run(c, mode, {rem_carrier_phase_in_rad, phase_step_rad, phase_rate_step_rad, rem_code_phase_chips,
        code_phase_step_chips, code_phase_rate_step_chips, signal_length_samples});
}

gc_status gc_correlator_carrier_wipeoff_multicorrelator_resampler_6(gc_correlator* c,
    float rem_carrier_phase_in_rad, float phase_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips,
    int signal_length_samples)
{
    GC_REQUIRE(c, "gc_correlator_carrier_wipeoff_multicorrelator_resampler_6: NULL handle");
    const int mode = c->use_high_dynamics_resampler ? TRK_MODE_HD_RESAMPLER : TRK_MODE_PLAIN;
    return correlator_run(c, mode, {rem_carrier_phase_in_rad, phase_step_rad, 0.0f, rem_code_phase_chips,
        code_phase_step_chips, code_phase_rate_step_chips, signal_length_samples});
}

gc_status gc_correlator_carrier_wipeoff_multicorrelator_resampler_5(gc_correlator* c,
    float rem_carrier_phase_in_rad, float phase_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips,
    int signal_length_samples)
{
    GC_REQUIRE(c, "gc_correlator_carrier_wipeoff_multicorrelator_resampler_5: NULL handle");
    return correlator_run(c, c->code_mode == TRK_MODE_SC16 ? TRK_MODE_SC16 : TRK_MODE_COMPLEX_CODE, {rem_carrier_phase_in_rad, phase_step_rad, 0.0f, rem_code_phase_chips,
        code_phase_step_chips, 0.0f, signal_length_samples});
}

gc_status gc_ctx_register_host_buffer(gc_ctx* ctx, const void* base, size_t bytes)
{
    GC_REQUIRE(ctx && base && bytes > 0, "gc_ctx_register_host_buffer: bad argument");
    gc_device_guard g(ctx->device);
    gc_l1_batcher* b = l1_batcher_get(ctx);
    if (!b) return gc_fail(GC_ERR_HIP, "gc_ctx_register_host_buffer: the batcher's buffers could not be set up");
    void* dv = nullptr;
    hipError_t e = hipHostRegister(const_cast<void*>(base), bytes, hipHostRegisterMapped);
    if (e == hipSuccess)
        {
            e = hipHostGetDevicePointer(&dv, const_cast<void*>(base), 0);
            if (e != hipSuccess) (void)hipHostUnregister(const_cast<void*>(base));
        }
    if (e != hipSuccess)
        {
            (void)hipGetLastError();
            return gc_fail(GC_ERR_HIP, "gc_ctx_register_host_buffer: %s (the correlators keep staging their windows)", hipGetErrorString(e));
        }
    b->add_region(base, bytes, dv);
    return GC_OK;
}

gc_status gc_ctx_unregister_host_buffer(gc_ctx* ctx, const void* base)
{
    GC_REQUIRE(ctx && base, "gc_ctx_unregister_host_buffer: bad argument");
    gc_device_guard g(ctx->device);
    void* p = ctx->l1_batcher.load(std::memory_order_acquire);
    if (!p) return gc_fail(GC_ERR_STATE, "gc_ctx_unregister_host_buffer: nothing is registered");
    // live registrations only; returns once no queued or running call reads through the buffer's device view and it is unpinned
    if (!static_cast<L1Holder*>(p)->bat->remove_region(base)) return gc_fail(GC_ERR_STATE, "gc_ctx_unregister_host_buffer: %p is not registered", base);
    return GC_OK;
}

gc_status gc_correlator_batch_stats(gc_ctx* ctx, uint64_t* n_batches, uint64_t* n_requests, uint64_t* n_shared_windows, int* max_batch)
{
    GC_REQUIRE(ctx, "gc_correlator_batch_stats: NULL context");
    gc_l1_batcher::Stats st;
    if (void* p = ctx->l1_batcher.load(std::memory_order_acquire))
        {
            st = static_cast<L1Holder*>(p)->bat->stats();
            if (const char* e = gc_exp_env("GNSSCORR_L1_TRACE"))
                if (e[0] == '1' && st.n_batches)
                    std::fprintf(stderr, "gnsscorr level-1 batcher: %llu batches, %llu calls; per batch: prepare %.1f us, launch %.1f us, wait %.1f us, scatter %.1f us; per call in the batcher %.1f us\n",
                        st.n_batches, st.n_requests, st.t_prep / st.n_batches, st.t_launch / st.n_batches, st.t_sync / st.n_batches, st.t_scatter / st.n_batches,
                        st.t_queue / (st.n_requests ? st.n_requests : 1));
        }
    if (n_batches) *n_batches = st.n_batches;
    if (n_requests) *n_requests = st.n_requests;
    if (n_shared_windows) *n_shared_windows = st.n_shared;
    if (max_batch) *max_batch = st.max_batch;
    return GC_OK;
}

gc_status gc_correlator_free(gc_correlator* c)
{
    GC_REQUIRE(c, "gc_correlator_free: NULL handle");
    gc_device_guard g(c->ctx->device);
    std::lock_guard<std::mutex> lk(c->ctx->mtx);
    (void)hipStreamSynchronize(c->ctx->stream);
    c->w = gc_correlator::Work();  // the handle answers GC_ERR_STATE until the next init()
    return GC_OK;
}

}  // extern "C"
