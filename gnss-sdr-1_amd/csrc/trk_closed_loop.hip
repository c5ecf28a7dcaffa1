// trk_closed_loop.hip -- closed-loop DLL/PLL tracking entirely on the GPU.
//
// One workgroup per channel runs K code periods back to back: the multicorrelator of
// trk_device.hpp for the epoch, then -- on one lane -- the per-epoch scalar maths the
// reference block does on the host between two correlations:
//   cn0_and_tracking_lock_status   dll_pll_veml_tracking.cc:839-878  (lock_detectors.cc:71-111)
//   run_dll_pll                    dll_pll_veml_tracking.cc:914-973  (tracking_discriminators.cc:41-128,
//                                  tracking_loop_filter.cc:74-245, tracking_FLL_PLL_filter.cc:55-133)
//   update_tracking_vars           dll_pll_veml_tracking.cc:998-1070
//   pull-in alignment              dll_pll_veml_tracking.cc:1568-1600
// so that a launch needs no host round trip per millisecond.  The per-epoch
// record carries what the block puts in Gnss_Synchro and in its binary dump.  The whole state machine of
// general_work runs here: pull-in (1), wide tracking with secondary-code / preamble synchronisation (2,
// :1601-1773), extended coherent integration (3, :1774-1826) and narrow tracking (4, :1827-1896), with the
// data-component prompt correlator of pilot tracking (:899-910) and the high-dynamics rate smoothers (:1016-1064).
// One engine, three kinds of kernel over one shell (trk_loop_device.hpp: state, loop maths, channel shell, period loop, launch): the
// persistent kernel here, the mixed kernel of gc_trk_loop_set_mixed (trk_closed_loop_mixed.hip) and the GLONASS kernel of
// gc_trk_loop_start_glonass (trk_closed_loop_glonass.hip).  Which kinds may run side by side is trk_loop_kind.h's rule.
#include "gc_internal.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include "gc_stream.h"
#include "trk_batch_plan.h"
#include "trk_loop_kind.h"
#include "trk_loop_device.hpp"
#include "trk_glonass_loop_device.hpp"
#include <cstring>
#include <vector>

// THREADS per channel: 1024 when there are few channels (one workgroup per CU), 256 when there are many
// DATA: pilot tracking, every channel carries the data component's replica (chan.code2)
// HD:   Dll_Pll_Conf::high_dyn -- the high-dynamics resampler and rotator (carrier and code rate terms)
template <int NTAPS, int THREADS, int FMT, bool DATA, bool HD = false>
__global__ __launch_bounds__(THREADS) void trk_closed_loop_kernel(LoopChan* __restrict__ chans,
    gc_loop_record* __restrict__ recs, int n_epochs, int lds_table_floats, const unsigned long long* __restrict__ limits, int resident)
{
    extern __shared__ float lds[];
    __shared__ LoopChan s;
    __shared__ gc_epoch_params s_p;
    __shared__ float2 s_corr[GC_MAX_TAPS];
    __shared__ int s_go;
    loop_channel<THREADS>(s, chans, recs, n_epochs, limits, [&] { return s.n_taps != NTAPS; }, [&](gc_loop_record* crec, unsigned long long limit) {
        loop_periods<VemlLoopKind<NTAPS, DATA, HD>, THREADS, FMT>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
    });
}

#ifdef GNSSCORR_EXPERIMENTS
// -----------------------------------------------------------------------------
// Few channels on a big chip (the sharded receiver: 32 channels per GPU, BASELINE configs[4]): one workgroup per channel leaves
// 7 of 8 CUs idle and a code period costs its full 10 us whatever the load.  Here a channel-period is cut into S slices, one
// workgroup each (the batched kernel's slicing: trk_epoch's `slice` of `n_slices`), ONE launch per code period: a slice leaves
// its partial sums in global memory and draws a ticket; the workgroup that draws the last one adds the partials IN SLICE ORDER
// (deterministic: no float atomics), runs the period's scalar loop maths on one lane exactly as the persistent kernel does
// (loop_after_correlation), prepares the NEXT period's correlator scalars (loop_prepare) and writes the state back.  The kernel
// boundary is the only grid-wide synchronisation: no spinning, no co-residency assumption.  Records agree with the persistent
// kernel's to float rounding (the sums are associated differently); for a given slice count they are reproducible bit for bit.
// MEASURED SLOWER than the persistent kernel and therefore an experiments-build option only (gc_trk_loop_set_geometry refuses
// slices > 1 in the product library): 32 channels x 25 Msps, 13.4 us per code period with 4 or 8 slices (15.3 with 2, 16.4 with
// 16) against 11.4 us for one 1024-thread workgroup per channel -- of the launch's 12 us only ~2 are the slice's correlation; the
// rest is a chain of dependent round trips the persistent kernel does not have (descriptor and scalars from the previous launch,
// code window, first samples, write-through of the partials, ticket, state in, state out) around the same 2.6 us of one-lane maths.
// -----------------------------------------------------------------------------
// Hand-off of the partial sums: every byte is stored with sc1 (agent-scope relaxed atomic stores: write-through), the storing lane
// drains them (s_waitcnt vmcnt(0)) and then adds to the channel's ticket counter; the lane whose add returns S - 1 reads them with
// sc1 loads, which bypass its CU's L1.  That is the fence-free form MI355X_MICROARCH.md lists as measured valid on gfx950 (one
// storing lane per workgroup, the last adder told by the value its add returned); LOOP_SLICE_FENCES=1 adds the agent-scope
// release / acquire pair of acq_final_kernel around it (~3.4 us per period on the critical path).
#ifndef LOOP_SLICE_FENCES
#define LOOP_SLICE_FENCES 0
#endif
struct LoopPrep
{
    gc_epoch_params p;
    int go;
    int pad;
};

// the correlator scalars of the first period of a launch sequence (and its invalid record when there is nothing to correlate)
template <bool HD>
__global__ __launch_bounds__(64) void trk_loop_prepare_kernel(LoopChan* __restrict__ chans, LoopPrep* __restrict__ prep, gc_loop_record* __restrict__ recs, int n_epochs,
    const unsigned long long* __restrict__ limits)
{
    __shared__ LoopChan s;
    __shared__ gc_epoch_params s_p;
    const int ch = blockIdx.x, tid = threadIdx.x;
    loop_copy_state<64>(&s, &chans[ch]);
    __syncthreads();
    if (s.n_taps == 0) return;  // standby slot: the slice kernel writes its all-zero records
    if (tid == 0)
        {
            const unsigned long long limit = limits ? limits[ch] : s.chan.n_iq;
            const int go = loop_prepare<HD>(s, limit, s_p, &recs[(size_t)ch * n_epochs]);
            prep[ch].p = s_p;
            prep[ch].go = go;
        }
    __syncthreads();
    loop_copy_state<64>(&chans[ch], &s);
}

// code period `e` of every channel: blockIdx -> (channel, slice) with all slices of a channel on one XCD (they share the window)
template <int NTAPS, int THREADS, int FMT, bool DATA, bool HD>
__global__ __launch_bounds__(THREADS) void trk_closed_loop_slice_kernel(LoopChan* __restrict__ chans, gc_loop_record* __restrict__ recs, int n_epochs, int e,
    int n_channels, int n_slices, int lds_table_floats, const unsigned long long* __restrict__ limits, LoopPrep* __restrict__ prep, float2* __restrict__ partial,
    unsigned* __restrict__ tickets)
{
    extern __shared__ float lds[];
    __shared__ LoopChan s;  // the finishing workgroup's copy of the channel state (the others use .chan and .n_taps only)
    __shared__ gc_epoch_params s_p;
    __shared__ float2 s_corr[GC_MAX_TAPS];
    __shared__ int s_go, s_last;
    const int tid = threadIdx.x;
    // b = (group * n_slices + slice) * 8 + x, channel = group * 8 + x: equal b % 8 (one XCD under round-robin placement) for a channel's slices
    const int x = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int slice = q % n_slices, ch = (q / n_slices) * 8 + x;
    if (ch >= n_channels) return;
    constexpr int NOUT = NTAPS + (DATA ? 1 : 0);
    gc_loop_record* rec = &recs[(size_t)ch * n_epochs + e];
    if (tid == 0)
        {
            s.chan = chans[ch].chan;
            s.n_taps = chans[ch].n_taps;
            s_p = prep[ch].p;
            s_go = prep[ch].go;
        }
    __syncthreads();
    if (s.n_taps != NTAPS)
        {
            // a channel that has not been started (or was stopped): standby record, written by its first slice
            if (slice == 0) loop_standby_records<THREADS>(rec, 1);
            return;
        }
    if (s_go)
        {
            const float2 r = trk_epoch<LoopEpochPolicy<NTAPS, HD, FMT, THREADS, DATA>>(s.chan, s_p, slice, n_slices, lds_table_floats, lds, LOOP_ALIGN_PAIRS);
            if (tid < NOUT) s_corr[tid] = r;
        }
    __syncthreads();
    if (tid == 0)
        {
            // hand the partial sums over; the workgroup that draws the last ticket finishes the period (all in one lane:
            // stores -> release fence -> ticket, ticket -> acquire fence -> loads; the same protocol as acq_final_kernel)
            float* pv = reinterpret_cast<float*>(partial + ((size_t)ch * n_slices + slice) * GC_MAX_TAPS);
            if (s_go)
                for (int t = 0; t < NOUT; t++)
                    {
                        __hip_atomic_store(pv + 2 * t, s_corr[t].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(pv + 2 * t + 1, s_corr[t].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
#if LOOP_SLICE_FENCES
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#endif
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the sc1 (write-through) stores above have left for L2 / memory
            const unsigned ticket = __hip_atomic_fetch_add(tickets + ch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (ticket == (unsigned)n_slices - 1u) ? 1 : 0;
#if LOOP_SLICE_FENCES
            if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
        }
    __syncthreads();
    if (!s_last) return;
    // ---- the last slice to finish: the rest of general_work for this period ----
    // (the channel state and prep[] were written by the PREVIOUS launch: visible across the kernel boundary to plain loads)
    loop_copy_state<THREADS>(&s, &chans[ch]);
    __syncthreads();
    if (tid == 0)
        {
            const unsigned long long limit = limits ? limits[ch] : s.chan.n_iq;
            if (s_go)
                {
                    float2 taps[GC_MAX_TAPS];
                    for (int t = 0; t < NOUT; t++) taps[t] = make_float2(0.f, 0.f);
                    for (int sl = 0; sl < n_slices; sl++)  // slice order: the same sums whichever workgroup finishes last
                        {
                            const float* qv = reinterpret_cast<const float*>(partial + ((size_t)ch * n_slices + sl) * GC_MAX_TAPS);
                            for (int t = 0; t < NOUT; t++)
                                {
                                    taps[t].x += __hip_atomic_load(qv + 2 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    taps[t].y += __hip_atomic_load(qv + 2 * t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                }
                        }
                    for (int t = 0; t < NOUT; t++) s_corr[t] = taps[t];
                    loop_after_correlation<NTAPS, DATA>(s, s_corr, rec);
                }
            // the next period's scalars (a period that found nothing to correlate leaves the state where it was: the next one
            // is decided again, as the persistent kernel decides every period)
            if (e + 1 < n_epochs)
                {
                    const int go = loop_prepare<HD>(s, limit, s_p, rec + 1);
                    prep[ch].p = s_p;
                    prep[ch].go = go;
                }
            __hip_atomic_store(tickets + ch, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
        }
    __syncthreads();
    loop_copy_state<THREADS>(&chans[ch], &s);
}

#else
struct LoopPrep;
#endif  // GNSSCORR_EXPERIMENTS

__global__ void trk_loop_start_kernel(LoopChan* chans, int ch)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) loop_start(chans[ch]);
}

// -----------------------------------------------------------------------------
// host API
// -----------------------------------------------------------------------------
// an event made without timing, destroyed with the engine
struct LoopEvent
{
    hipEvent_t e = nullptr;
    hipError_t create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    ~LoopEvent() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

struct gc_trk_loop
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    int n_channels = 0, max_code_len = 0;
    LoopKind kind = {LOOP_VEML, 0, 0, 0};     // of the running channels, set by the start that finds no other channel running (trk_loop_kind.h)
    gc_dev_buf<LoopChan> d_chans;
    gc_dev_buf<float> d_codes;
    gc_dev_buf<float> d_data_codes;           // pilot tracking: data-component replicas, allocated on first use
    std::vector<LoopSync> sync;               // per channel (gc_trk_loop_set_sync); extend_symbols == 0: none installed
    std::vector<int> data_code_len;           // samples of the data replica uploaded for the channel (0: none)
    int mixed = 0;                            // gc_trk_loop_set_mixed: tap count and pilot mode per channel (the mixed kernel)
    gc_dev_buf<GloChan> d_glo;                // the state of LOOP_GLONASS channels, allocated on first use
    std::vector<int> code_len;                // per channel: samples of the replica it was started with
    std::vector<char> track_pilot;            // per channel: pilot mode it was started with
    gc_dev_buf<gc_loop_record> d_recs;
    int forced_threads = 0;  // gc_trk_loop_set_geometry: threads per workgroup of the persistent kernel (0: by channel count)
    int forced_slices = 0;   // gc_trk_loop_set_geometry: workgroups per channel-period (0: by channel count; 1: persistent kernel)
    gc_dev_buf<LoopPrep> d_prep;     // sliced launches: next period's correlator scalars per channel
    gc_dev_buf<float2> d_slice_partial;
    gc_dev_buf<unsigned> d_tickets;
    int iq_format = GC_IQ_F32;  // sample format of every channel's input (gc_trk_loop_set_input_format)
    std::vector<char> started;
    std::vector<const void*> iq;
    std::vector<unsigned long long> n_iq;
    // ring input (gc_trk_loop_set_input_stream)
    std::vector<gc_stream*> streams;          // per channel, or NULL
    std::vector<unsigned long long> pos_host; // last known stream position of the channel (from the records)
    std::vector<char> pos_known;
    std::vector<char> idle;                   // the channel's last record said state 0 (standby after loss of lock)
    // Per-launch ring limits travel through a small ring of slots (pinned host copy + device copy + an event recorded behind the
    // launch that reads the device copy): an asynchronous launch keeps its slot until it has finished, so back-to-back
    // push -> run_dev -> push -> run_dev never rewrites limits an earlier, still queued launch will read.
    static constexpr int LIMIT_SLOTS = 8;
    struct LimitSlot
    {
        gc_dev_buf<unsigned long long> d;
        gc_host_buf<unsigned long long> h;  // pinned
        LoopEvent done;
        bool used = false;
    } limits[LIMIT_SLOTS];
    int limit_next = 0;
    // the last launch of the engine, on whatever stream the caller chose: entry points that rewrite device state wait for it
    LoopEvent last_launch;
    bool launched = false;
};

// waits until no launch of the engine is in flight on any stream (the caller holds the context mutex)
static hipError_t loop_quiesce(gc_trk_loop* l)
{
    hipError_t e = hipStreamSynchronize(l->ctx->stream);
    if (e == hipSuccess && l->launched) e = hipEventSynchronize(l->last_launch);
    return e;
}

// The kind rule (trk_loop_kind.h) for a request on slot `ch` (-1: for no slot), with the engine's one scan of its running channels:
// `first` is the lowest running channel (-1: none), the one a refusal names
struct LoopAdmission
{
    LoopKindVerdict verdict;
    int first;
    bool others;  // a channel other than `ch` runs
};
static LoopAdmission loop_admission(const gc_trk_loop* l, int ch, const LoopKind& req)
{
    LoopAdmission a = {LOOP_ADMIT, -1, false};
    for (int i = l->n_channels - 1; i >= 0; i--)
        if (l->started[i])
            {
                a.first = i;
                a.others |= i != ch;
            }
    a.verdict = loop_kind_admit(l->kind, l->mixed != 0, a.others, a.first >= 0, req);
    return a;
}

// f(slot `ch` of the state buffer the engine's running channels live in): LoopChan*, or GloChan* for LOOP_GLONASS
template <class F>
static gc_status loop_with_slot(gc_trk_loop* l, int ch, F f)
{
    return l->kind.family == LOOP_GLONASS ? f(l->d_glo + ch) : f(l->d_chans + ch);
}

// a running channel keeps its state; only the input block changes (stream position restarts at 0)
template <class State>
static gc_status loop_rebind_input(State* d_slot, const void* dev_iq, uint64_t n_samples)
{
    State h;
    GC_HIP(hipMemcpy(&h, d_slot, sizeof h, hipMemcpyDeviceToHost));
    h.chan.iq = dev_iq;
    h.chan.n_iq = n_samples;
    h.chan.ring_len = 0;
    h.pos = 0;
    GC_HIP(hipMemcpy(d_slot, &h, sizeof h, hipMemcpyHostToDevice));
    return GC_OK;
}

// n_taps = 0 marks the slot as standby for the kernel; the rest of the state is rewritten by the next start
template <class State>
static gc_status loop_mark_standby(State* d_slot)
{
    const int zero = 0;
    GC_HIP(hipMemcpy(reinterpret_cast<char*>(d_slot) + offsetof(State, n_taps), &zero, sizeof zero, hipMemcpyHostToDevice));
    return GC_OK;
}

// The slot binding of both starts, once every check has passed (the ring-window check included: a refused start leaves the engine
// and a running slot as they were).  h carries the kind's own part of the state; this uploads the replica, fills in the slot's
// correlator descriptor and position, does the host's bookkeeping and uploads the state to its buffer.
template <class State>
static gc_status loop_bind_slot(gc_trk_loop* l, int ch, State& h, State* d_slot, const float* code, int code_length, int track_pilot, uint64_t sample_counter)
{
    const size_t at = (size_t)ch * l->max_code_len;
    GC_HIP(hipMemcpy(l->d_codes + at, code, sizeof(float) * code_length, hipMemcpyHostToDevice));
    l->code_len[ch] = code_length;
    l->track_pilot[ch] = (char)track_pilot;
    h.chan.iq = l->iq[ch];
    h.chan.n_iq = l->n_iq[ch];
    h.chan.code = l->d_codes + at;
    h.chan.code_len = code_length;
    h.chan.code2 = track_pilot ? l->d_data_codes + at : nullptr;
    h.chan.ring_len = l->streams[ch] ? (unsigned)l->streams[ch]->capacity : 0;
    // ring input is addressed with absolute stream sample numbers: the channel starts where its counter says
    h.pos = l->streams[ch] ? sample_counter : 0;
    l->pos_host[ch] = h.pos;
    l->pos_known[ch] = 1;
    l->idle[ch] = 0;
    GC_HIP(hipMemcpy(d_slot, &h, sizeof h, hipMemcpyHostToDevice));
    return GC_OK;
}

// what gc_trk_loop_start_glonass and gc_glonass_loop_pull_in both ask of a configuration (`who`: the caller, for the message)
static gc_status glo_conf_check(const gc_glonass_loop_conf* conf, const char* who)
{
    GC_REQUIRE(conf, "%s: NULL configuration", who);
    GC_REQUIRE(conf->fs_in >= 1000.0 && conf->fs_in <= 1e9 && conf->fs_in == std::floor(conf->fs_in), "%s: fs_in must be a whole number of samples per second in 1e3..1e9", who);
    GC_REQUIRE(conf->band_carrier_freq_hz > 0 && conf->band_carrier_freq_hz + conf->channel_offset_hz > 0, "%s: bad carrier frequency", who);
    GC_REQUIRE(std::isfinite(conf->acq_delay_samples) && std::isfinite(conf->acq_doppler_hz) && std::fabs(conf->acq_delay_samples) <= 1e9 && std::fabs(conf->acq_doppler_hz) <= 1e6,
        "%s: bad acquisition hand-over", who);
    GC_REQUIRE(conf->sample_counter >= conf->acq_samplestamp_samples, "%s: sample_counter lies before acq_samplestamp_samples", who);
    return GC_OK;
}

extern "C" {

gc_status gc_trk_loop_create(gc_ctx* ctx, int n_channels, int max_code_length, gc_trk_loop** out)
{
    GC_REQUIRE(ctx && out, "gc_trk_loop_create: NULL argument");
    *out = nullptr;
    GC_REQUIRE(n_channels > 0, "gc_trk_loop_create: n_channels must be > 0");
    GC_REQUIRE(max_code_length > 0 && max_code_length + TRK_LDS_MARGIN_FLOATS <= TRK_LDS_TABLE_FLOATS, "gc_trk_loop_create: max_code_length must be in 1..%d",
        TRK_LDS_TABLE_FLOATS - TRK_LDS_MARGIN_FLOATS);
    gc_device_guard g(ctx->device);
    std::unique_ptr<gc_trk_loop> l(new gc_trk_loop());
    l->ctx = ctx;
    l->ctx_ref.bind(ctx);
    l->n_channels = n_channels;
    l->max_code_len = max_code_length;
    if (l->d_chans.alloc(n_channels) != hipSuccess || l->d_codes.alloc((size_t)n_channels * max_code_length) != hipSuccess)
        return gc_fail(GC_ERR_HIP, "gc_trk_loop_create: hipMalloc failed");
    (void)hipMemset(l->d_chans, 0, sizeof(LoopChan) * n_channels);
    l->started.assign(n_channels, 0);
    l->sync.assign(n_channels, LoopSync());
    l->data_code_len.assign(n_channels, 0);
    l->code_len.assign(n_channels, 0);
    l->track_pilot.assign(n_channels, 0);
    l->iq.assign(n_channels, nullptr);
    l->n_iq.assign(n_channels, 0);
    l->streams.assign(n_channels, nullptr);
    l->pos_host.assign(n_channels, 0);
    l->pos_known.assign(n_channels, 0);
    l->idle.assign(n_channels, 0);
    bool ok = l->last_launch.create() == hipSuccess;
    for (gc_trk_loop::LimitSlot& s : l->limits)
        ok = ok && s.d.alloc(n_channels) == hipSuccess && s.h.alloc(n_channels) == hipSuccess && s.done.create() == hipSuccess;
    if (!ok) return gc_fail(GC_ERR_HIP, "gc_trk_loop_create: allocation failed");
    *out = l.release();
    return GC_OK;
}

gc_status gc_trk_loop_destroy(gc_trk_loop* l)
{
    if (!l) return GC_OK;
    gc_device_guard g(l->ctx->device);
    (void)loop_quiesce(l);
    for (gc_stream* r : l->streams)
        if (r) gc_stream_drop(r);
    delete l;
    return GC_OK;
}

gc_status gc_trk_loop_set_geometry(gc_trk_loop* l, int threads_per_workgroup, int slices_per_channel)
{
    GC_REQUIRE(l, "gc_trk_loop_set_geometry: NULL handle");
    GC_REQUIRE(threads_per_workgroup == 0 || threads_per_workgroup == 256 || threads_per_workgroup == 512 || threads_per_workgroup == 1024,
        "gc_trk_loop_set_geometry: threads_per_workgroup must be 0 (automatic), 256, 512 or 1024");
    GC_REQUIRE(slices_per_channel >= 0 && slices_per_channel <= 16, "gc_trk_loop_set_geometry: slices_per_channel must be in 0..16 (0: automatic)");
#ifndef GNSSCORR_EXPERIMENTS
    GC_REQUIRE(slices_per_channel <= 1, "gc_trk_loop_set_geometry: sliced code periods measured slower than one workgroup per channel and exist in "
                                        "experiments builds only (make exp)");
#endif
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    GC_REQUIRE(slices_per_channel <= 1 || !l->mixed, "gc_trk_loop_set_geometry: a mixed engine (gc_trk_loop_set_mixed) runs one workgroup per channel");
    l->forced_threads = threads_per_workgroup;
    l->forced_slices = slices_per_channel;
    return GC_OK;
}

gc_status gc_trk_loop_set_mixed(gc_trk_loop* l, int on)
{
    GC_REQUIRE(l, "gc_trk_loop_set_mixed: NULL handle");
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    const LoopAdmission adm = loop_admission(l, -1, {LOOP_MODE, 0, 0, 0});
    if (adm.verdict != LOOP_ADMIT) return gc_fail(GC_ERR_STATE, "gc_trk_loop_set_mixed: channel %d is running; set the mode before any gc_trk_loop_start", adm.first);
    GC_REQUIRE(!on || l->forced_slices <= 1, "gc_trk_loop_set_mixed: a mixed engine runs one workgroup per channel (gc_trk_loop_set_geometry slices %d)",
        l->forced_slices);
    l->mixed = on ? 1 : 0;
    return GC_OK;
}

gc_status gc_trk_loop_set_input_dev(gc_trk_loop* l, int ch, const void* dev_iq, uint64_t n_samples)
{
    GC_REQUIRE(l && dev_iq, "gc_trk_loop_set_input_dev: NULL argument");
    GC_REQUIRE(ch >= 0 && ch < l->n_channels, "gc_trk_loop_set_input_dev: channel %d out of range", ch);
    const uintptr_t es = gc_iq_sample_bytes(l->iq_format);
    GC_REQUIRE((reinterpret_cast<uintptr_t>(dev_iq) % es) == 0, "gc_trk_loop_set_input_dev: IQ pointer must be aligned to one sample (%d bytes)", (int)es);
    gc_device_guard g(l->ctx->device);
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    if (l->streams[ch]) gc_stream_drop(l->streams[ch]);
    l->streams[ch] = nullptr;
    l->iq[ch] = dev_iq;
    l->n_iq[ch] = n_samples;
    if (!l->started[ch]) return GC_OK;
    GC_HIP(loop_quiesce(l));
    return loop_with_slot(l, ch, [&](auto* d_slot) { return loop_rebind_input(d_slot, dev_iq, n_samples); });
}

gc_status gc_trk_loop_set_input_format(gc_trk_loop* l, int iq_format)
{
    GC_REQUIRE(l, "gc_trk_loop_set_input_format: NULL handle");
    GC_REQUIRE(iq_format == GC_IQ_F32 || iq_format == GC_IQ_I16 || iq_format == GC_IQ_I8, "gc_trk_loop_set_input_format: unknown format %d", iq_format);
    if (iq_format == l->iq_format) return GC_OK;
    for (int i = 0; i < l->n_channels; i++)
        if (l->started[i] || l->iq[i] != nullptr)
            return gc_fail(GC_ERR_STATE, "gc_trk_loop_set_input_format: set the format before binding inputs or starting channels");
    l->iq_format = iq_format;
    return GC_OK;
}

gc_status gc_trk_loop_set_input_stream(gc_trk_loop* l, int ch, gc_stream* s)
{
    GC_REQUIRE(l && s, "gc_trk_loop_set_input_stream: NULL argument");
    GC_REQUIRE(ch >= 0 && ch < l->n_channels, "gc_trk_loop_set_input_stream: channel %d out of range", ch);
    GC_REQUIRE(s->ctx->device == l->ctx->device, "gc_trk_loop_set_input_stream: the stream lives on another GPU");
    GC_REQUIRE(s->iq_format == l->iq_format, "gc_trk_loop_set_input_stream: stream format %d, engine format %d (gc_trk_loop_set_input_format)",
        s->iq_format, l->iq_format);
    if (l->started[ch]) return gc_fail(GC_ERR_STATE, "gc_trk_loop_set_input_stream: channel %d is running; bind the stream before gc_trk_loop_start", ch);
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    gc_stream_keep(s);
    if (l->streams[ch]) gc_stream_drop(l->streams[ch]);
    l->streams[ch] = s;
    l->iq[ch] = s->d_ring;
    l->n_iq[ch] = ~0ull;
    return GC_OK;
}

gc_status gc_trk_loop_set_sync(gc_trk_loop* l, int ch, const gc_loop_sync_conf* sync, const float* data_code, int data_code_length)
{
    GC_REQUIRE(l, "gc_trk_loop_set_sync: NULL handle");
    GC_REQUIRE(ch >= 0 && ch < l->n_channels, "gc_trk_loop_set_sync: channel %d out of range", ch);
    if (!sync)
        {
            std::lock_guard<std::mutex> lk(l->ctx->mtx);
            l->sync[ch] = LoopSync();
            l->data_code_len[ch] = 0;
            return GC_OK;
        }
    GC_REQUIRE(sync->extend_correlation_symbols >= 1, "gc_trk_loop_set_sync: extend_correlation_symbols must be >= 1");
    GC_REQUIRE(sync->secondary_code_length >= 0 && sync->secondary_code_length <= 128, "gc_trk_loop_set_sync: secondary_code_length must be in 0..128");
    GC_REQUIRE(sync->preamble_length_symbols >= 0 && sync->preamble_length_symbols <= 192, "gc_trk_loop_set_sync: preamble_length_symbols must be in 0..192");
    GC_REQUIRE(sync->symbols_per_bit >= 0, "gc_trk_loop_set_sync: symbols_per_bit must be >= 0");
    LoopSync y;
    std::memset(&y, 0, sizeof y);
    y.extend_symbols = sync->extend_correlation_symbols;
    y.track_pilot = sync->track_pilot ? 1 : 0;
    y.symbols_per_bit = sync->symbols_per_bit;
    y.secondary_len = sync->secondary_code_length;
    y.preamble_len = sync->preamble_length_symbols;
    y.bit_sync_min_time_s = sync->bit_sync_min_time_s;
    y.pll_bw_narrow_hz = sync->pll_bw_narrow_hz;
    y.dll_bw_narrow_hz = sync->dll_bw_narrow_hz;
    y.el_narrow_chips = sync->early_late_space_narrow_chips;
    y.vel_narrow_chips = sync->very_early_late_space_narrow_chips;
    for (int i = 0; i < y.secondary_len; i++)
        {
            const char ch_i = sync->secondary_code[i];
            GC_REQUIRE(ch_i == '0' || ch_i == '1', "gc_trk_loop_set_sync: secondary_code[%d] is not '0' or '1'", i);
            const int bit = y.secondary_len - 1 - i;  // newest symbol in bit 0
            if (ch_i == '1') y.sec_ones[bit >> 5] |= 1u << (bit & 31);
        }
    for (int i = 0; i < y.preamble_len; i++)
        {
            const int v = sync->preamble_symbols[i];
            GC_REQUIRE(v == 1 || v == -1, "gc_trk_loop_set_sync: preamble_symbols[%d] is not +1 / -1", i);
            const int bit = y.preamble_len - 1 - i;
            if (v == 1) y.pre_plus[bit >> 5] |= 1u << (bit & 31);
        }
    gc_device_guard g(l->ctx->device);
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    if (y.track_pilot)
        {
            GC_REQUIRE(data_code, "gc_trk_loop_set_sync: track_pilot needs the data component's replica");
            GC_REQUIRE(data_code_length > 0 && data_code_length <= l->max_code_len, "gc_trk_loop_set_sync: data_code_length %d not in 1..%d", data_code_length,
                l->max_code_len);
            if (!l->d_data_codes) GC_HIP(l->d_data_codes.alloc((size_t)l->n_channels * l->max_code_len));
            GC_HIP(loop_quiesce(l));
            GC_HIP(hipMemcpy(l->d_data_codes + (size_t)ch * l->max_code_len, data_code, sizeof(float) * data_code_length, hipMemcpyHostToDevice));
            l->data_code_len[ch] = data_code_length;  // must equal the tracking replica's length: checked at start
        }
    l->sync[ch] = y;
    return GC_OK;
}

gc_status gc_trk_loop_start(gc_trk_loop* l, int ch, const gc_loop_conf* conf, const float* code, int code_length)
{
    GC_REQUIRE(l && conf && code, "gc_trk_loop_start: NULL argument");
    GC_REQUIRE(ch >= 0 && ch < l->n_channels, "gc_trk_loop_start: channel %d out of range", ch);
    GC_REQUIRE(code_length > 0 && code_length <= l->max_code_len, "gc_trk_loop_start: code_length %d not in 1..%d", code_length, l->max_code_len);
    GC_REQUIRE(l->iq[ch] != nullptr, "gc_trk_loop_start: channel %d has no input (gc_trk_loop_set_input_dev)", ch);
    GC_REQUIRE(conf->cn0_samples >= 1 && conf->cn0_samples <= LOOP_MAX_CN0, "gc_trk_loop_start: cn0_samples must be in 1..%d", LOOP_MAX_CN0);
    GC_REQUIRE(conf->vector_length > 0 && conf->fs_in > 0 && conf->code_chip_rate_hz > 0, "gc_trk_loop_start: bad signal description");
    GC_REQUIRE((uint32_t)code_length == conf->code_length_chips * conf->code_samples_per_chip,
        "gc_trk_loop_start: code_length %d != code_length_chips * code_samples_per_chip", code_length);
    GC_REQUIRE(conf->high_dyn_smoother_length <= LOOP_MAX_SMOOTHER, "gc_trk_loop_start: high_dyn_smoother_length must be <= %d", LOOP_MAX_SMOOTHER);
    const int n_taps = conf->veml ? 5 : 3;
    gc_device_guard g(l->ctx->device);
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    LoopSync y = l->sync[ch];
    if (y.extend_symbols == 0)
        {
            // nothing installed: a signal whose bit synchronisation never happens (stays in state 2)
            y.extend_symbols = 1;
            y.symbols_per_bit = 2;
        }
    // the running channels of an engine are of one kind (trk_loop_kind.h): it is free again once every channel has been stopped
    const LoopKind req = {LOOP_VEML, n_taps, y.track_pilot, conf->high_dyn_smoother_length > 0 ? 1 : 0};
    const LoopAdmission adm = loop_admission(l, ch, req);
    if (adm.verdict == LOOP_REFUSE_GLONASS_RUNS)
        return gc_fail(GC_ERR_STATE, "gc_trk_loop_start: channel %d runs as a GLONASS channel (gc_trk_loop_start_glonass); stop it first", adm.first);
    GC_REQUIRE(adm.verdict != LOOP_REFUSE_TAPS, "gc_trk_loop_start: all channels of one loop engine use the same tap count (%d)", l->kind.n_taps);
    if (y.track_pilot)
        GC_REQUIRE(l->data_code_len[ch] == code_length, "gc_trk_loop_start: the data replica has %d samples, the tracking replica %d", l->data_code_len[ch],
            code_length);
    GC_REQUIRE(adm.verdict != LOOP_REFUSE_PILOT, "gc_trk_loop_start: all channels of one loop engine share the pilot mode (track_pilot = %d)", l->kind.pilot);
    GC_REQUIRE(adm.verdict != LOOP_REFUSE_HIGH_DYN, "gc_trk_loop_start: all channels of one loop engine share the high_dyn mode (%d)", l->kind.high_dyn);
    if (gc_stream* r = l->streams[ch])
        GC_REQUIRE(conf->vector_length <= r->mirror, "gc_trk_loop_start: vector_length %u exceeds the stream's max_window %llu", conf->vector_length,
            (unsigned long long)r->mirror);

    // every check has passed: from here on the engine and the slot change
    hipStream_t st = l->ctx->stream;
    GC_HIP(loop_quiesce(l));
    LoopChan h;
    std::memset(&h, 0, sizeof h);
    h.conf = *conf;
    h.sync = y;
    h.n_taps = n_taps;
    // tap shifts in code samples (dll_pll_veml_tracking.cc:372-390, :720-732)
    const float spc = (float)conf->code_samples_per_chip;
    if (conf->veml)
        {
            h.chan.shifts[0] = -conf->very_early_late_space_chips * spc;
            h.chan.shifts[1] = -conf->early_late_space_chips * spc;
            h.chan.shifts[2] = 0.0f;
            h.chan.shifts[3] = conf->early_late_space_chips * spc;
            h.chan.shifts[4] = conf->very_early_late_space_chips * spc;
        }
    else
        {
            h.chan.shifts[0] = -conf->early_late_space_chips * spc;
            h.chan.shifts[1] = 0.0f;
            h.chan.shifts[2] = conf->early_late_space_chips * spc;
        }
    const gc_status bs = loop_bind_slot(l, ch, h, l->d_chans + ch, code, code_length, y.track_pilot, conf->sample_counter);
    if (bs != GC_OK) return bs;
    hipLaunchKernelGGL(trk_loop_start_kernel, dim3(1), dim3(64), 0, st, l->d_chans, ch);
    GC_HIP(hipGetLastError());
    GC_HIP(hipStreamSynchronize(st));
    if (!adm.others) l->kind = req;  // the engine's kind changes together with its only running channel
    l->started[ch] = 1;
    return GC_OK;
}

}  // extern "C"

extern "C" gc_status gc_trk_loop_stop(gc_trk_loop* l, int ch)
{
    GC_REQUIRE(l, "gc_trk_loop_stop: NULL handle");
    GC_REQUIRE(ch >= 0 && ch < l->n_channels, "gc_trk_loop_stop: channel %d out of range", ch);
    gc_device_guard g(l->ctx->device);
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    if (!l->started[ch]) return GC_OK;
    GC_HIP(loop_quiesce(l));
    const gc_status s = loop_with_slot(l, ch, [](auto* d_slot) { return loop_mark_standby(d_slot); });
    if (s == GC_OK) l->started[ch] = 0;
    return s;
}

extern "C" size_t gc_glonass_loop_conf_size(void) { return sizeof(gc_glonass_loop_conf); }

// glonass_l1_ca_dll_pll_tracking_cc::start_tracking (:160-243) for channel `ch`: every argument is checked before anything touches
// a device -- the configuration first (it needs no handle), then the handle and the engine's state
extern "C" gc_status gc_trk_loop_start_glonass(gc_trk_loop* l, int ch, const gc_glonass_loop_conf* conf)
{
    const gc_status cc = glo_conf_check(conf, "gc_trk_loop_start_glonass");
    if (cc != GC_OK) return cc;
    GC_REQUIRE(conf->vector_length >= 1 && conf->vector_length <= (1u << 24), "gc_trk_loop_start_glonass: vector_length must be in 1..2^24");
    GC_REQUIRE(conf->cn0_samples >= 1 && conf->cn0_samples <= LOOP_MAX_CN0, "gc_trk_loop_start_glonass: cn0_samples must be in 1..%d", LOOP_MAX_CN0);
    GC_REQUIRE(conf->pll_bw_hz > 0 && conf->dll_bw_hz > 0, "gc_trk_loop_start_glonass: loop bandwidths must be > 0");
    GC_REQUIRE(conf->early_late_space_chips > 0 && conf->early_late_space_chips <= 16.0f, "gc_trk_loop_start_glonass: early_late_space_chips must be in (0, 16]");
    GloChan h;
    std::memset(&h, 0, sizeof h);
    h.conf = *conf;
    glo_loop_start(h);
    GC_REQUIRE(h.current_prn_length_samples >= 1 && (unsigned)h.current_prn_length_samples <= 2u * conf->vector_length,
        "gc_trk_loop_start_glonass: the code period is %d samples, outside 1..2 * vector_length (%u)", h.current_prn_length_samples, conf->vector_length);
    GC_REQUIRE(l, "gc_trk_loop_start_glonass: NULL handle");
    GC_REQUIRE(ch >= 0 && ch < l->n_channels, "gc_trk_loop_start_glonass: channel %d out of range", ch);
    GC_REQUIRE(l->max_code_len >= GLO_CODE_LENGTH, "gc_trk_loop_start_glonass: the engine's max_code_length %d is below the %d chips of the replica", l->max_code_len,
        GLO_CODE_LENGTH);
    GC_REQUIRE(l->iq[ch] != nullptr, "gc_trk_loop_start_glonass: channel %d has no input (gc_trk_loop_set_input_dev)", ch);
    gc_device_guard g(l->ctx->device);
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    const LoopKind req = {LOOP_GLONASS, 3, 0, 0};
    const LoopAdmission adm = loop_admission(l, ch, req);
    if (adm.verdict == LOOP_REFUSE_MIXED_GLONASS)
        return gc_fail(GC_ERR_STATE, "gc_trk_loop_start_glonass: a mixed engine (gc_trk_loop_set_mixed) has no GLONASS slots; run a GLONASS engine beside it");
    if (adm.verdict != LOOP_ADMIT)
        return gc_fail(GC_ERR_STATE, "gc_trk_loop_start_glonass: channel %d runs as a veml channel (gc_trk_loop_start); stop it first", adm.first);
    if (gc_stream* r = l->streams[ch])
        GC_REQUIRE(2ull * conf->vector_length <= r->mirror, "gc_trk_loop_start_glonass: 2 * vector_length (%u) exceeds the stream's max_window %llu", conf->vector_length,
            (unsigned long long)r->mirror);
    float chips[GLO_CODE_LENGTH];
    const gc_status cs = gc_glonass_l1_ca_code_gen_float(chips, 0);
    if (cs != GC_OK) return cs;
    GC_HIP(loop_quiesce(l));
    if (!l->d_glo)
        {
            GC_HIP(l->d_glo.alloc(l->n_channels));
            GC_HIP(hipMemset(l->d_glo, 0, sizeof(GloChan) * l->n_channels));
        }
    h.chan.shifts[0] = -conf->early_late_space_chips;
    h.chan.shifts[1] = 0.0f;
    h.chan.shifts[2] = conf->early_late_space_chips;
    h.n_taps = 3;
    const gc_status bs = loop_bind_slot(l, ch, h, l->d_glo + ch, chips, GLO_CODE_LENGTH, 0, conf->sample_counter);
    if (bs != GC_OK) return bs;
    l->kind = req;  // the engine's kind changes together with its first running channel
    l->started[ch] = 1;
    return GC_OK;
}

// the pull-in alignment of a start with `conf`, on the host: glo_loop_start and glo_loop_pull_in, the statements the kernel runs
extern "C" gc_status gc_glonass_loop_pull_in(const gc_glonass_loop_conf* conf, int32_t* samples_offset, uint64_t* sample_counter, double* acc_carrier_phase_rad)
{
    const gc_status cc = glo_conf_check(conf, "gc_glonass_loop_pull_in");
    if (cc != GC_OK) return cc;
    GloChan h;
    std::memset(&h, 0, sizeof h);
    h.conf = *conf;
    glo_loop_start(h);
    GC_REQUIRE(h.current_prn_length_samples >= 1, "gc_glonass_loop_pull_in: the code period is %d samples", h.current_prn_length_samples);
    const int offset = glo_loop_pull_in(h);
    if (samples_offset) *samples_offset = offset;
    if (sample_counter) *sample_counter = h.sample_counter;
    if (acc_carrier_phase_rad) *acc_carrier_phase_rad = h.acc_carrier_phase_rad;
    return GC_OK;
}

#ifdef GNSSCORR_EXPERIMENTS
// one launch per code period: `n_epochs` launches of n_channels x n_slices workgroups behind one prepare launch.  The slices run 256
// threads on the per-period window, whatever a.plan says: the dynamic LDS is this path's own.
static hipError_t loop_launch_slices(gc_trk_loop* l, const LoopLaunch& a, bool pilot, int n_slices, int lds_table_floats)
{
    constexpr int TH = 256;
    const size_t lds_bytes = (size_t)(trk_hdr_floats(TH) + lds_table_floats) * sizeof(float);
    const unsigned grid = (unsigned)(((a.n_channels + 7) / 8) * n_slices * 8);
    LoopChan* d_chans = static_cast<LoopChan*>(a.d_state);
    return trk_switch_format(l->iq_format, [&](auto fm) { return trk_switch_bool(l->kind.n_taps == 5, [&](auto veml) { return trk_switch_bool(pilot, [&](auto da) {
        return trk_switch_bool(l->kind.high_dyn != 0, [&](auto hd) {
            const auto kernel = trk_closed_loop_slice_kernel<veml() ? 5 : 3, TH, fm(), da(), hd()>;
            if (lds_bytes > 48 * 1024)
                {
                    hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
                    if (ea != hipSuccess) return ea;
                }
            hipLaunchKernelGGL((trk_loop_prepare_kernel<hd()>), dim3(a.n_channels), dim3(64), 0, a.st, d_chans, l->d_prep, a.dev_records, a.n_epochs, a.limits);
            for (int e = 0; e < a.n_epochs; e++)
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), lds_bytes, a.st, d_chans, a.dev_records, a.n_epochs, e, a.n_channels, n_slices, lds_table_floats, a.limits, l->d_prep,
                    l->d_slice_partial, l->d_tickets);
            return hipGetLastError();
        });
    }); }); });
}

// slice buffers of the engine, grown on demand
static hipError_t loop_slices_reserve(gc_trk_loop* l, int n_slices, hipStream_t st)
{
    hipError_t e = l->d_prep ? hipSuccess : l->d_prep.alloc(l->n_channels);
    if (e == hipSuccess && !l->d_tickets)
        {
            e = l->d_tickets.alloc(l->n_channels);
            if (e == hipSuccess) e = hipMemsetAsync(l->d_tickets, 0, sizeof(unsigned) * l->n_channels, st);
        }
    if (e == hipSuccess) e = l->d_slice_partial.reserve((size_t)GC_MAX_TAPS * l->n_channels * n_slices);
    return e;
}

#endif  // GNSSCORR_EXPERIMENTS

// The persistent kernel of a plain engine: sample format, threads | high-dynamics, taps and data | pilot down to the instance's launch
static hipError_t loop_launch_plain(const LoopLaunch& a, int n_taps, int iq_format, bool pilot, bool high_dyn)
{
    return trk_switch_format(iq_format, [&](auto fm) { return trk_switch_threads(a.plan.threads, high_dyn, [&](auto th, auto hd) {
        return trk_switch_bool(n_taps == 5, [&](auto veml) { return trk_switch_bool(pilot, [&](auto da) {
            return loop_launch_kernel(trk_closed_loop_kernel<veml() ? 5 : 3, th(), fm(), da(), hd()>, th(), a, a.plan.resident);
        }); });
    }); });
}

// Ring inputs of a launch: the distinct rings its running channels read and the floor of each -- the oldest sample a channel with
// a known position still needs; one channel with an unknown position pins it at the oldest resident sample.  Also presets the
// limits: a buffer's length, 0 for a standby ring channel (never started, stopped, or lost lock: it reads nothing and holds
// nothing back in the ring); those of running ring channels follow from the reservations.
struct LoopRings
{
    gc_stream* ring[gc_stream_read_set::MAX_RINGS];
    uint64_t floor[gc_stream_read_set::MAX_RINGS];
    int n = 0;
    bool any = false;  // a channel is bound to a ring, running or not
};
static gc_status loop_ring_floors(const gc_trk_loop* l, bool positions_known, unsigned long long* h_limits, LoopRings& rings)
{
    for (int i = 0; i < l->n_channels; i++)
        {
            gc_stream* r = l->streams[i];
            h_limits[i] = l->n_iq[i];
            if (!r) continue;
            rings.any = true;
            if (!l->started[i] || l->idle[i])
                {
                    h_limits[i] = 0;
                    continue;
                }
            const uint64_t floor = positions_known && l->pos_known[i] ? l->pos_host[i] : GC_STREAM_FLOOR_OLDEST;
            const int k = (int)(std::find(rings.ring, rings.ring + rings.n, r) - rings.ring);
            if (k == rings.n)
                {
                    if (rings.n == gc_stream_read_set::MAX_RINGS) return gc_stream_read_ops::too_many_rings(rings.n);
                    rings.ring[rings.n] = r;
                    rings.floor[rings.n++] = floor;
                }
            else if (floor + 1 < rings.floor[k] + 1)  // GC_STREAM_FLOOR_OLDEST (~0) + 1 wraps to 0: below every floor
                rings.floor[k] = floor;
        }
    return GC_OK;
}

static gc_status loop_launch(gc_trk_loop* l, int n_epochs, gc_loop_record* dev_records, hipStream_t st, bool positions_known)
{
    // channels that were never started (or were stopped) sit in standby: all-zero records, state 0
    if (std::find(l->started.begin(), l->started.end(), 1) == l->started.end())
        return gc_fail(GC_ERR_STATE, "gc_trk_loop_run: no channel has been started (gc_trk_loop_start)");
    // this launch's slot of the limits ring: free once the launch that used it last has finished
    const int slot = l->limit_next;
    gc_trk_loop::LimitSlot& lim = l->limits[slot];
    if (lim.used) GC_HIP(hipEventSynchronize(lim.done));
    unsigned long long* h_limits = lim.h;
    // ring inputs: this launch may use what has been pushed so far, and must not be overtaken by later pushes.  One reservation per
    // ring, taken before the residency check and the enqueue; the limits are the heads seen by those reservations.
    LoopRings rings;
    const gc_status fs = loop_ring_floors(l, positions_known, h_limits, rings);
    if (fs != GC_OK) return fs;
    gc_stream_read_set reads(st);
    for (int k = 0; k < rings.n; k++)
        {
            const gc_status rs = reads.add(rings.ring[k], rings.floor[k]);
            if (rs != GC_OK && rings.floor[k] != GC_STREAM_FLOOR_OLDEST)
                return gc_fail(GC_ERR_STATE, "gc_trk_loop_run: a channel (at sample %llu) fell behind the ring", (unsigned long long)rings.floor[k]);
            if (rs != GC_OK) return rs;
        }
    if (rings.any)
        {
            for (int i = 0; i < l->n_channels; i++)
                if (l->streams[i] && l->started[i] && !l->idle[i]) h_limits[i] = reads.ticket(l->streams[i]).head;
            hipError_t ce = hipMemcpyAsync(lim.d, h_limits, sizeof(unsigned long long) * l->n_channels, hipMemcpyHostToDevice, st);
            if (ce != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_trk_loop_run: %s", hipGetErrorString(ce));
        }
    const unsigned long long* limits = rings.any ? lim.d.get() : nullptr;
    // a GLONASS engine: its own kernel and state; its 511-chip replica always sits in LDS as the doubled resident image
    const bool glonass = l->kind.family == LOOP_GLONASS, pilot = l->kind.pilot > 0, high_dyn = l->kind.high_dyn != 0;
    const TrkLoopPlan plan = trk_loop_plan(l->n_channels, l->ctx->n_cus, high_dyn, l->forced_threads, l->mixed != 0, l->started.data(), l->code_len.data(),
        l->track_pilot.data(), glonass ? GLO_CODE_LENGTH : l->max_code_len, pilot);
    const LoopLaunch a = {glonass ? (void*)l->d_glo.get() : (void*)l->d_chans.get(), l->n_channels, n_epochs, dev_records, st, plan, limits};
    hipError_t le;
    if (glonass)
        le = glo_loop_launch(a, l->iq_format);
    else if (l->mixed)
        le = loop_launch_mixed(a, l->iq_format, high_dyn);
#ifdef GNSSCORR_EXPERIMENTS
    // workgroups per channel-period: 1 = the persistent one-workgroup-per-channel kernel (always, in the product library); an
    // experiments build cuts the period into slices on request (gc_trk_loop_set_geometry), one launch per period: measured slower
    else if (l->forced_slices > 1)
        {
            GC_HIP(loop_slices_reserve(l, l->forced_slices, st));
            le = loop_launch_slices(l, a, pilot, l->forced_slices, (l->max_code_len + 64) * (pilot ? 2 : 1));
        }
#endif
    else
        le = loop_launch_plain(a, l->kind.n_taps, l->iq_format, pilot, high_dyn);
    if (le != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_trk_loop_run: kernel launch failed: %s", hipGetErrorString(le));
    gc_status out = GC_OK;
    hipError_t ee = hipEventRecord(l->last_launch, st);
    l->launched = true;
    if (ee == hipSuccess && rings.any)
        {
            ee = hipEventRecord(lim.done, st);
            if (ee == hipSuccess)
                {
                    lim.used = true;
                    l->limit_next = (slot + 1) % gc_trk_loop::LIMIT_SLOTS;
                }
        }
    if (ee != hipSuccess)
        {
            // without its completion event the launch cannot be tracked: wait for it here
            (void)hipStreamSynchronize(st);
            out = gc_fail(GC_ERR_HIP, "gc_trk_loop_run: hipEventRecord failed: %s", hipGetErrorString(ee));
        }
    const gc_status cs = reads.commit();
    return out != GC_OK ? out : cs;
}

extern "C" {

gc_status gc_trk_loop_run_dev(gc_trk_loop* l, int n_epochs, gc_loop_record* dev_records, void* stream)
{
    GC_REQUIRE(l && dev_records, "gc_trk_loop_run_dev: NULL argument");
    GC_REQUIRE(n_epochs > 0, "gc_trk_loop_run_dev: n_epochs must be > 0");
    gc_device_guard g(l->ctx->device);
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    // the records stay in HBM: the channels' positions are unknown to the host from here on
    for (auto& k : l->pos_known) k = 0;
    return loop_launch(l, n_epochs, dev_records, gc_pick_stream(l->ctx, stream), false);
}

gc_status gc_trk_loop_run(gc_trk_loop* l, int n_epochs, gc_loop_record* host_records)
{
    GC_REQUIRE(l && host_records, "gc_trk_loop_run: NULL argument");
    GC_REQUIRE(n_epochs > 0, "gc_trk_loop_run: n_epochs must be > 0");
    gc_device_guard g(l->ctx->device);
    std::lock_guard<std::mutex> lk(l->ctx->mtx);
    hipStream_t st = l->ctx->stream;
    const size_t n = (size_t)l->n_channels * n_epochs;
    GC_HIP(l->d_recs.reserve(n));
    gc_status s = loop_launch(l, n_epochs, l->d_recs, st, true);
    if (s != GC_OK) return s;
    GC_HIP(hipMemcpyAsync(host_records, l->d_recs, n * sizeof(gc_loop_record), hipMemcpyDeviceToHost, st));
    GC_HIP(hipStreamSynchronize(st));
    // ring channels: Tracking_sample_counter of the last record IS the absolute position (it started at sample_counter)
    for (int i = 0; i < l->n_channels; i++)
        if (l->streams[i] && l->started[i])
            {
                const gc_loop_record& last = host_records[(size_t)i * n_epochs + (n_epochs - 1)];
                l->pos_host[i] = last.sample_counter;
                l->pos_known[i] = 1;
                l->idle[i] = last.state == 0;  // loss of lock: the channel waits for the next gc_trk_loop_start
            }
    return GC_OK;
}

}  // extern "C"
