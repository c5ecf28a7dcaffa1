// gc_acquisition.hip -- host side of the PCPS acquisition path of libgnsscorr.so.
// Mirrors pcps_acquisition (src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition.cc):
// constructor sizes (:63-190), set_local_code (:239-274), init (:313-368),
// acquisition_core (:668-770) -- batched over n_sats satellites that search the
// same input block.
#include "acq_caf_kernels.h"
#include "acq_engine_sizes.h"
#include "acq_kernels.h"
#include "acq_quicksync_kernels.h"
#include "acq_tong_kernels.h"
#include "gc_internal.h"
#include "gc_stream.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

// QuickSync engine (pcps_quicksync_acquisition_cc.cc).  fft_size is M = N / f (N = samples_per_code), consumed is L = f N.  The wipe-off
// table holds L samples per bin in NATURAL order (the fold kernel and the candidate check read it; no transform does), a dwell folds
// x * wipeoff into n_bins rows of M samples (acq_qs_fold_kernel, row-permuted into d_xw), runs the transforms and the CFAR statistic of
// the plain engine at size M -- the grid is overwritten by every dwell, nothing accumulates -- and resolves the f aliased delays on the
// device (acq_qs_verify_kernel).  The statistics kernel runs with its dwell: the candidate check reads its winner.
struct AcqQuickSync
{
    int fold = 0;                      // f
    uint32_t code_len = 0;             // N
    AcqFftPlan wipe_plan{};            // N1 = 1, N2 = L: the table builder writes natural order
    gc_dev_buf<float2> d_code_time;    // [sat][N]: the codes as handed in (d_code, :182)
    gc_dev_buf<float> d_cand_val;      // [sat][f]: d_corr_output_f of the last dwell
    gc_dev_buf<uint32_t> d_cand_delay; // [sat][f]: d_possible_delay
};

// Tong engine (pcps_tong_acquisition_cc.cc).  Every dwell adds |.|^2 / (N^4 * its own input power) to the grid (acq_launch_cols_tong) and
// is followed by the decision kernel, which walks each running satellite's counter ON THE DEVICE and freezes the satellites that have
// decided: their column workgroups return at once from then on, so grid, row maxima and result stay those of the deciding dwell.
// Nothing is pending behind a dwell, and no call decides on the host.  gc_acq_reset() only marks the restart: the next dwell enqueues it
// (counters, flags, results) in front of its own work, on its own stream.
struct AcqTong
{
    AcqTongParams p{};
    bool restart = true;
    gc_dev_buf<AcqTongState> d_state;   // [sat]
    gc_dev_buf<int> d_frozen;           // [sat]
    gc_host_buf<AcqTongState> h_state;  // pinned
};

// CAF engine (galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc).  A slot holds R = (1 or 2 components) x (1 or 2 hypotheses) replicas in
// the order IA, QA, IB, QB (d_codes is [sat][R][N]).  The inverse row pass runs over R * n_bins cells per satellite, the column pass
// (ACQ_EPI_MAG, unchanged) writes the R |.|^2 planes of a batch and their block maxima, acq_caf_select_kernel makes the per-bin choice of
// hypothesis and builds the grid rows, and acq_caf_decide_kernel -- once per dwell -- the result, the keep rule and the CAF filter.  With
// R = 1 the column pass writes the grid itself.  Every dwell stands alone; the one thing kept between dwells is
// gc_acq_result::test_statistics on the device.  gc_acq_reset() only marks the restart: the next dwell zeroes the results in front of its
// own work, on its own stream.
struct AcqCaf
{
    AcqCafParams p{};
    bool restart = true;
    gc_dev_buf<float> d_planes;   // [batch sat][R][n_bins][N] (R >= 2)
    gc_dev_buf<float> d_plv;      // their block maxima [batch sat][R][n_bins][n_blocks]
    gc_dev_buf<unsigned> d_pli;
    gc_dev_buf<float> d_caf, d_caf_i, d_caf_q;  // [sat][n_bins]
    gc_dev_buf<unsigned char> d_choice;
};

// What a dwell leaves to be done later (kinds whose traits say holds_back; the statistics of a plain or paired dwell).
struct AcqHeld
{
    // The statistics of a dwell (acq_final_kernel) are computed when somebody can see them -- a fetch -- or when the next dwell
    // would not reproduce their side effect, not after every dwell: the reference evaluates the statistic after each dwell
    // (pcps_acquisition.cc:747-755), but a caller that enqueues the dwells of a search back to back and fetches once only ever
    // reads the last one.  The one side effect, the scratch image of d_tmp_buffer, is overwritten completely by the column pass
    // of an ACCUMULATING dwell (last-bin magnitudes, :737), so a pending evaluation may be dropped in front of such a dwell and must
    // run in front of any other.
    bool final_pending = false;
    AcqFinalArgs final_args{};
    hipStream_t final_stream = nullptr;
    // Of a dwell that more dwells are expected to follow (dwell counter < max_dwells, plain statistic) only the input block is taken
    // at once (row-permuted into slot 0 of d_xw); its transforms are held back: if the next call is an accumulating dwell on the same
    // stream, BOTH blocks go through one forward row / column pass (2 * n_bins spectra into d_X), one inverse row pass over
    // 2 * n_bins spectra per satellite and one column pass that adds the two |.|^2 and writes the grid once
    // (ACQ_EPI_MAG2) -- the grid read-modify-write of the second dwell and the first dwell's grid write never happen.  Anything
    // else (a fetch, a grid read, a change of codes or of the Doppler grid) first runs the held-back passes alone, so every caller
    // sees what per-dwell processing would have produced; gc_acq_reset() drops them with the grid.  (A paired engine's inter-pass
    // buffer is the one a dwell pair would need, so it holds nothing back.)
    bool inv_pending = false;
    bool inv_accumulate = false;
    int inv_n_bins = 0;
    hipStream_t inv_stream = nullptr;
    bool fuse_dwells = true;  // $GNSSCORR_ACQ_FUSE=0: every dwell on its own
};

// Three experiments, off by default and compiled into the experiments build only (acq_inverse_experiment):
//  * overlap ($GNSSCORR_ACQ_OVERLAP=1): row pass (instruction- and LDS-bound, 3.8 TB/s) and column pass (bandwidth-bound, 5.6 TB/s) of
//    DIFFERENT satellite batches side by side -- rows on the caller's stream, columns on a stream of the engine, d_Q double-buffered,
//    events both ways.  Measured 0.42 instead of 0.355 ms per search: the row pass holds all the LDS of every CU (4 x 40 KB), so the
//    column workgroups do not become resident beside it and the eight cross-queue hand-overs only add latency
//  * roles ($GNSSCORR_ACQ_ROLES=1): with more than one satellite batch of dwell pairs, the row pass of batch b and the column pass of
//    batch b - 1 share ONE launch (acq_rows3_cols_kernel: of every four workgroups of a CU, 4 - ACQ_ROLE_COLS do rows and ACQ_ROLE_COLS
//    columns), d_Q double-buffered, no events.  Measured 0.44 (one column workgroup of four) and 0.33 (two) against 0.31 ms per search:
//    a column workgroup needs its CU-mates' loads in flight to hide its two load phases, and the row pass slows down with fewer than
//    three workgroups
//  * onchip ($GNSSCORR_ACQ_ONCHIP=1): N = 25 x 1000 plans run the inverse transform of a cell entirely on its CU
//    (acq_inv_fused_kernel, no inter-pass buffer).  Measured 0.525 ms per cfg4 search against 0.311 ms for the two-pass form:
//    DESIGN.md section 3.2
struct AcqExperiments
{
    bool overlap = false, roles = false, onchip = false;
    hipStream_t side = nullptr;
    hipEvent_t ev_rows[2] = {nullptr, nullptr}, ev_cols[2] = {nullptr, nullptr};
    size_t q_stride = 0;  // float2 elements between the two halves of d_Q (0: single buffer)
    ~AcqExperiments()
    {
        for (hipEvent_t ev : {ev_rows[0], ev_rows[1], ev_cols[0], ev_cols[1]})
            if (ev) (void)hipEventDestroy(ev);
        if (side) (void)hipStreamDestroy(side);
    }
};

struct gc_acq
{
    gc_ctx* ctx = nullptr;
    // Declared before every buffer, hence destroyed after them: the context outlives the frees.  The frees themselves run under the
    // gc_device_guard of whoever deletes the engine (gc_acq_destroy, a failing acq_create).
    gc_ctx_ref ctx_ref;
    gc_acq_conf conf{};
    AcqKind kind = ACQ_PLAIN;
    const AcqKindTraits& traits() const { return ACQ_KIND_TRAITS[kind]; }
    int n_sats = 0;
    AcqEngineSizes sz{};  // fixed at creation (acq_engine_sizes.h)
    uint32_t n_bins = 0;  // bins of the ACTIVE grid: sz.n_bins, or those of step two
    bool step_two = false;
    float center_step_two = 0.0f;
    uint32_t dwell_counter = 0;
    AcqFftPlan plan{};
    AcqRowsPlan rows{};  // the row kernel of `plan`
    int n_blocks = 0;
    // Paired engine: GC_ACQ_COMBINE_MAX / _SUM.  Every satellite slot holds TWO replicas (d_codes is [sat][2][N]); the inverse row pass
    // runs over 2 * n_bins cells per satellite -- the dwell's n_bins spectra against replica A, then the same spectra against replica B
    // -- and the column pass combines the two |.|^2 of a grid cell before it writes it once (ACQ_EPI_PMAX / _PSUM).
    int combine = 0;
    gc_dev_buf<float2> d_wN, d_wN2, d_wipe_main, d_wipe2;
    float2* d_wipe = nullptr;  // the active table: d_wipe_main or d_wipe2 (not owned)
    gc_dev_buf<float2> d_codes, d_xw, d_X, d_Q;
    gc_dev_buf<float> d_grid, d_tmp, d_blkv, d_power;
    gc_dev_buf<unsigned> d_blki;
    gc_dev_buf<float2> d_in, d_cvt;  // d_cvt: the converted input block (integer sample formats)
    int iq_format = GC_IQ_F32;
    gc_dev_buf<gc_acq_result> d_results;
    gc_host_buf<gc_acq_result> h_results;  // pinned
    gc_dev_buf<float> d_part_val;          // acq_final_kernel: second-peak candidates per row piece
    gc_dev_buf<unsigned> d_part_cnt;       // and its ticket counters
    std::vector<char> code_set;
    int64_t freq_offset_hz = 0;  // d_old_freq: intermediate frequency / GLONASS FDMA channel offset
    gc_dev_buf<AcqPhaseSeg> d_segs;  // closed-form segments of the rows' running phases (acq_phase_segments.h) [seg_cap]
    gc_dev_buf<int> d_seg_off;       // [n_bins_alloc + 1]
    size_t seg_cap = 0;
    // the wipe-off tables hold what freq_offset_hz / the step-two centre say: cleared before a rebuild starts, set when it has
    // completed; a search on tables in an unknown state is refused (GC_ERR_STATE) instead of run
    bool wipe_valid = false, wipe2_valid = false;
    bool grid_logically_zero = true;  // gc_acq_reset() since the last dwell: the grid reads as zeros
    AcqHeld held;
    AcqQuickSync qs;     // ACQ_QUICKSYNC
    AcqTong tong;        // ACQ_TONG
    AcqCaf caf;          // ACQ_CAF
    AcqExperiments exp;  // experiments build
};

// what most entry points begin with: the engine's device selected, then its context's mutex held
struct acq_locked
{
    gc_device_guard g;
    std::lock_guard<std::mutex> lk;
    explicit acq_locked(const gc_acq* a) : g(a->ctx->device), lk(a->ctx->mtx) {}
};

// What an entry point asks of the engine's kind (ACQ_KIND_TRAITS answers): GC_OK if `ok`, otherwise GC_ERR_INVALID and the message
// "<who>: an engine made by <its create function> <why><use>", `who` the public function and `use` the call that fits
static gc_status acq_ask(const gc_acq* a, const char* who, bool ok, const char* why, const char* use = "")
{
    if (ok) return GC_OK;
    return gc_fail(GC_ERR_INVALID, "%s: an engine made by %s %s%s", who, a->traits().create, why, use);
}

// is the engine of kind `k`; is `who` the gc_acq_set_local_code* entry point of its kind
#define ACQ_ASK_KIND(a, who, k) acq_ask(a, who, (a)->kind == (k), "cannot do this: it takes one made by ", ACQ_KIND_TRAITS[k].create)
#define ACQ_ASK_CODE_ENTRY(a, who) acq_ask(a, who, std::strcmp((a)->traits().code_entry, who) == 0, "takes its codes through ", (a)->traits().code_entry)

// the satellites [s0, s0 + ns) that share the inter-pass buffer in one pair of inverse launches
struct AcqBatch
{
    int s0, ns, index;
};

// body(batch) for the batches of `per_batch` satellites in turn, until one fails
template <typename Body>
static hipError_t acq_for_batches(int n_sats, int per_batch, Body body)
{
    hipError_t e = hipSuccess;
    int index = 0;
    for (int s0 = 0; s0 < n_sats && e == hipSuccess; s0 += per_batch, index++) e = body(AcqBatch{s0, std::min(per_batch, n_sats - s0), index});
    return e;
}

// the fields that the arguments of every kind's statistics / decision kernel share (AcqFinalArgs, AcqTongDecideArgs, AcqCafDecideArgs)
template <typename Args>
static void acq_fill_decision_args(const gc_acq* a, Args& d)
{
    d.blk_max_val = a->d_blkv;
    d.blk_max_idx = a->d_blki;
    d.results = a->d_results;
    d.n_bins = (int)a->n_bins;
    d.n_blocks = a->n_blocks;
    d.fft_size = (int)a->sz.fft_size;
    d.doppler_max = (int)a->conf.doppler_max;
    d.doppler_step = (int)a->conf.doppler_step;
}

// the restart mark of the kinds that have one (AcqTong, AcqCaf), or null
static bool* acq_restart_flag(gc_acq* a)
{
    return a->kind == ACQ_TONG ? &a->tong.restart : a->kind == ACQ_CAF ? &a->caf.restart : nullptr;
}

static hipError_t acq_flush_inverse(gc_acq* a, hipStream_t st);

// makes `st` wait for what has been enqueued on `other` so far
static hipError_t acq_order_after(hipStream_t st, hipStream_t other)
{
    if (st == other) return hipSuccess;
    hipEvent_t ev;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, other);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
    if (e == hipSuccess) (void)hipEventDestroy(ev);
    return e;
}

// Runs the pending statistics kernel, if any, on `st` -- or drops it, in front of a dwell that `accumulates` onto the same grid
// (n_bins) on the same stream: that dwell's column pass overwrites the scratch image the evaluation would have left
static hipError_t acq_flush_final(gc_acq* a, hipStream_t st, bool accumulates = false, int n_bins = 0)
{
    AcqHeld& h = a->held;
    if (!h.final_pending) return hipSuccess;
    h.final_pending = false;
    if (accumulates && h.final_args.n_bins == n_bins && h.final_stream == st) return hipSuccess;
    // the dwell it belongs to was enqueued on final_stream: same stream in every sensible use; otherwise order the two
    const hipError_t e = acq_order_after(st, h.final_stream);
    if (e != hipSuccess) return e;
    return acq_launch_final(st, h.final_args, a->n_sats);
}

// The wipe-off tables are kept in the row-permuted layout the forward row pass reads (P[bin][a][b] = wipe[bin][a + N1 * b]): the
// product x * wipeoff[bin] (pcps_acquisition.cc:717) is then the two-operand load of that pass -- A = the table, B = the permuted
// input block, shared by every bin -- instead of a kernel of its own that writes and re-reads n_bins x N products per dwell.
// A table is built out of place by ONE kernel in which every sample is independent: the float32 running phase of each row in closed form
// (acq_phase_segments.h, ~30 arithmetic-progression segments per row, computed here on the host; 25000 dependent additions on one
// lane per bin took 0.56 ms), (cos, sin) stored at the permuted position.  No scratch array, no device-to-device copy, no allocation
// in a set-up call unless a pathological increment needs more segments than the buffer holds.  The caller holds the context mutex.
static hipError_t acq_build_wipeoffs(gc_acq* a, const std::vector<float>& inc, float2* table, hipStream_t st)
{
    const int n = (int)inc.size();
    std::vector<AcqPhaseSeg> segs;
    std::vector<int> off(n + 1, 0);
    for (int d = 0; d < n; d++)
        {
            acq_phase_segments(inc[d], (int)a->sz.input_len, segs);
            off[d + 1] = (int)segs.size();
        }
    hipError_t e = hipSuccess;
    if (segs.size() > a->seg_cap)
        {
            e = hipStreamSynchronize(st);
            a->d_segs.reset();
            a->seg_cap = 0;
            if (e == hipSuccess) e = a->d_segs.alloc(segs.size());
            if (e != hipSuccess) return e;
            a->seg_cap = segs.size();
        }
    e = hipMemcpyAsync(a->d_segs, segs.data(), sizeof(AcqPhaseSeg) * segs.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(a->d_seg_off, off.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = acq_launch_wipeoff_segments(st, a->d_segs, a->d_seg_off, table, n, a->kind == ACQ_QUICKSYNC ? a->qs.wipe_plan : a->plan);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the host vectors go out of scope
    return e;
}

// d_grid_doppler_wipeoffs of the coarse grid: exp(-j*2*pi*(d_old_freq + doppler)/fs * n) with the reference's float32
// running phase (update_grid_doppler_wipeoffs :371-380, update_local_carrier :296-310); d_old_freq = freq_offset_hz
static hipError_t acq_build_main_wipeoffs(gc_acq* a, hipStream_t st)
{
    std::vector<float> inc(a->sz.n_bins);
    for (uint32_t d = 0; d < a->sz.n_bins; d++)
        {
            const int32_t doppler = -(int32_t)a->conf.doppler_max + (int32_t)a->conf.doppler_step * (int32_t)d;
            const float freq = (float)(a->freq_offset_hz + (int64_t)doppler);
            const float phase_step_rad = (float)(6.283185307179586 * freq / (float)a->conf.fs_in);
            inc[d] = -phase_step_rad;
        }
    a->wipe_valid = false;
    const hipError_t e = acq_build_wipeoffs(a, inc, a->d_wipe_main, st);
    a->wipe_valid = (e == hipSuccess);
    return e;
}

// behind every gc_acq_create* entry point, which has checked its own arguments, prepared `conf` as its engine sees it and filled `spec`
static gc_status acq_create(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, const AcqEngineSpec& spec, gc_acq** out)
{
    GC_REQUIRE(n_sats > 0, "gc_acq_create: n_sats must be > 0");
    GC_REQUIRE(conf->sampled_ms > 0 && conf->samples_per_ms > 0.0f, "gc_acq_create: bad sizes");
    GC_REQUIRE(conf->doppler_step > 0, "gc_acq_create: doppler_step must be > 0");
    gc_device_guard g(ctx->device);
    // declared behind the guard: whichever way this function is left, an engine that is not handed out is freed on its device
    std::unique_ptr<gc_acq> a(new gc_acq());
    a->ctx = ctx;
    a->ctx_ref.bind(ctx);
    a->conf = *conf;
    a->n_sats = n_sats;
    a->kind = spec.kind;
    a->combine = spec.combine;
    a->qs.fold = spec.fold;
    a->tong.p = spec.tong;
    a->caf.p = spec.caf;
    size_t q_budget = (size_t)140 << 20;
    if (const char* e = std::getenv("GNSSCORR_ACQ_Q_MB")) q_budget = (size_t)std::max(1, std::atoi(e)) << 20;
    const AcqEngineSizes& z = a->sz = acq_engine_sizes(*conf, spec, n_sats, q_budget);
    if (z.empty_grid) return gc_fail(GC_ERR_INVALID, "gc_acq_create: empty search grid");
    a->n_bins = z.n_bins;
    if (!acq_plan_make(&a->plan, (int)z.fft_size, 160 * 1024))  // the LDS of a CU
        return gc_fail(GC_ERR_INVALID, "gc_acq_create: fft_size %u has no supported factorisation", z.fft_size);
    a->rows = acq_rows_plan(a->plan);
    const size_t N = z.fft_size, ns = (size_t)n_sats, cells = ns * z.n_bins_alloc;
    a->n_blocks = acq_cols_blocks(a->plan);
    AcqExperiments& x = a->exp;
    if (const char* e = gc_exp_env("GNSSCORR_ACQ_FUSE")) a->held.fuse_dwells = std::atoi(e) != 0;
#ifdef GNSSCORR_EXPERIMENTS
    if (const char* e = gc_exp_env("GNSSCORR_ACQ_OVERLAP")) x.overlap = std::atoi(e) != 0;
    if (const char* e = gc_exp_env("GNSSCORR_ACQ_ROLES")) x.roles = std::atoi(e) != 0;
    if (const char* e = gc_exp_env("GNSSCORR_ACQ_ONCHIP")) x.onchip = std::atoi(e) != 0;
    x.roles = x.roles && a->held.fuse_dwells && acq_rows_cols_fusable(a->plan, a->rows);
    if (a->kind == ACQ_PAIRED || a->kind == ACQ_CAF) x.roles = x.overlap = x.onchip = false;  // the experiment launches know one replica per satellite only
    if (x.roles && n_sats > 1) x.q_stride = z.q_cells * N;  // second inter-pass buffer
    if (x.overlap && z.sats_per_batch < n_sats)
        {
            // more than one batch: a second buffer, so that the rows of batch b + 1 run beside the columns of batch b
            x.q_stride = z.q_cells * N;
            GC_HIP(hipStreamCreateWithFlags(&x.side, hipStreamNonBlocking));
            for (hipEvent_t* ev : {&x.ev_rows[0], &x.ev_rows[1], &x.ev_cols[0], &x.ev_cols[1]}) GC_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
        }
#endif
    GC_HIP(a->d_wN.alloc(N));
    GC_HIP(a->d_wN2.alloc((size_t)2 * a->plan.N2));
    GC_HIP(a->d_wipe_main.alloc((size_t)z.n_bins * z.input_len));
    a->d_wipe = a->d_wipe_main;
    if (conf->make_2_steps && conf->num_doppler_bins_step2 > 0) GC_HIP(a->d_wipe2.alloc((size_t)conf->num_doppler_bins_step2 * N));
    GC_HIP(a->d_xw.alloc((size_t)z.n_bins_alloc * N));
    GC_HIP(a->d_X.alloc((size_t)2 * z.n_bins_alloc * N));  // two dwells' spectra (AcqHeld)
    GC_HIP(a->d_Q.alloc((x.q_stride ? 2 : 1) * z.q_cells * N));
    a->seg_cap = (size_t)z.n_bins_alloc * 128;
    GC_HIP(a->d_segs.alloc(a->seg_cap));
    GC_HIP(a->d_seg_off.alloc((size_t)z.n_bins_alloc + 1));
    GC_HIP(a->d_blkv.alloc(cells * a->n_blocks));
    GC_HIP(a->d_blki.alloc(cells * a->n_blocks));
    GC_HIP(a->d_in.alloc(z.input_len));
    GC_HIP(a->d_cvt.alloc(z.input_len));
    if (a->kind == ACQ_QUICKSYNC)
        {
            a->qs.code_len = (uint32_t)conf->samples_per_code;
            a->qs.wipe_plan.N = a->qs.wipe_plan.N2 = (int)z.consumed;
            a->qs.wipe_plan.N1 = 1;
            GC_HIP(a->qs.d_code_time.alloc(ns * a->qs.code_len, true));
            GC_HIP(a->qs.d_cand_val.alloc(ns * spec.fold, true));
            GC_HIP(a->qs.d_cand_delay.alloc(ns * spec.fold, true));
        }
    if (a->kind == ACQ_TONG)
        {
            GC_HIP(a->tong.d_state.alloc(ns, true));
            GC_HIP(a->tong.d_frozen.alloc(ns, true));
            GC_HIP(a->tong.h_state.alloc(ns));
        }
    if (a->kind == ACQ_CAF)
        {
            if (z.replicas > 1)
                {
                    GC_HIP(a->caf.d_planes.alloc(z.q_cells * N));
                    GC_HIP(a->caf.d_plv.alloc(z.q_cells * a->n_blocks));
                    GC_HIP(a->caf.d_pli.alloc(z.q_cells * a->n_blocks));
                }
            GC_HIP(a->caf.d_caf.alloc(cells, true));
            GC_HIP(a->caf.d_caf_i.alloc(cells, true));
            GC_HIP(a->caf.d_caf_q.alloc(cells, true));
            GC_HIP(a->caf.d_choice.alloc(cells, true));
        }
    GC_HIP(a->d_results.alloc(ns, a->kind == ACQ_QUICKSYNC));  // the QuickSync candidate check reads its winner from here
    GC_HIP(a->d_part_val.alloc(ns * ACQ_FINAL_SPLIT * 2));
    GC_HIP(a->d_part_cnt.alloc(ns, true));
    GC_HIP(a->h_results.alloc(ns));
    a->code_set.assign(n_sats, 0);

    hipStream_t st = ctx->stream;
    // twiddle tables, rounded from float64
    {
        std::vector<float2> w(N);
        // inter-pass twiddles as the matrix T[k1][n2] = exp(-2*pi*j*k1*n2/N): unit-stride reads per row
        for (size_t k1 = 0; k1 < (size_t)a->plan.N1; k1++)
            for (size_t n2 = 0; n2 < (size_t)a->plan.N2; n2++)
                {
                    double ang = -2.0 * M_PI * (double)((k1 * n2) % N) / (double)N;
                    w[k1 * a->plan.N2 + n2] = make_float2((float)std::cos(ang), (float)std::sin(ang));
                }
        GC_HIP(hipMemcpy(a->d_wN, w.data(), N * sizeof(float2), hipMemcpyHostToDevice));
        // row-FFT twiddles: per-stage tables + plain table (acq_stage_twiddles)
        std::vector<float2> w2((size_t)2 * a->plan.N2);
        acq_stage_twiddles(a->plan, w2.data());
        GC_HIP(hipMemcpy(a->d_wN2, w2.data(), w2.size() * sizeof(float2), hipMemcpyHostToDevice));
    }
    // Doppler wipe-off grid: init() (:340-357) + update_local_carrier (:296-310)
    GC_HIP(acq_build_main_wipeoffs(a.get(), st));
    GC_HIP(hipStreamSynchronize(st));
    // the large zero fills last
    GC_HIP(a->d_grid.alloc(cells * N, true));
    GC_HIP(a->d_tmp.alloc(ns * N, true));
    GC_HIP(a->d_codes.alloc((size_t)z.replicas * ns * N, true));
    GC_HIP(a->d_power.alloc(1, true));
    *out = a.release();
    return GC_OK;
}

// a zero-padded replica to its place in d_codes; the caller holds the context mutex
static gc_status acq_load_padded(gc_acq* a, hipStream_t st, const std::vector<float2>& buf, size_t slot)
{
    const size_t N = a->sz.fft_size;
    GC_HIP(hipMemcpyAsync(a->d_in, buf.data(), N * sizeof(float2), hipMemcpyHostToDevice, st));
    // FFT, conjugate (:272-273), kept in the row-permuted layout the inverse rows pass reads
    hipError_t e = acq_launch_permute(st, a->d_in, nullptr, a->d_xw, a->plan, (int)N, 1, 0, 0, 0);
    if (e == hipSuccess) e = acq_launch_rows(st, false, a->plan, a->rows, 1, a->d_xw, AcqCellMap{1, 1}, nullptr, AcqCellMap{1, 1}, a->d_Q, a->d_wN2, a->d_wN);
    if (e == hipSuccess) e = acq_launch_cols(st, false, ACQ_EPI_COMPLEX_CONJ_PERM, a->plan, 1, a->d_Q, a->d_codes + slot * N, nullptr);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_set_local_code: %s", hipGetErrorString(e));
    GC_HIP(hipStreamSynchronize(st));  // buf goes out of scope
    return GC_OK;
}

// set_local_code (:252-273) of one replica: zero padded, FFT, conjugate, kept in d_codes[slot]; the caller holds the context mutex
static gc_status acq_load_code(gc_acq* a, hipStream_t st, const float* code, size_t slot)
{
    const size_t N = a->sz.fft_size;
    // [0 .. 0 c_0 .. c_L] layouts of set_local_code (:252-269)
    std::vector<float2> buf(N, make_float2(0.f, 0.f));
    const float2* c = reinterpret_cast<const float2*>(code);
    if (a->conf.bit_transition_flag)
        {
            size_t off = N / 2;
            std::memcpy(buf.data() + off, c, sizeof(float2) * off);
        }
    else if (a->sz.fft_size == a->sz.consumed)
        std::memcpy(buf.data(), c, sizeof(float2) * a->sz.consumed);
    else
        std::memcpy(buf.data() + (N - a->sz.consumed), c, sizeof(float2) * a->sz.consumed);
    return acq_load_padded(a, st, buf, slot);
}

extern "C" {

gc_status gc_acq_create(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, gc_acq** out)
{
    GC_REQUIRE(ctx && conf && out, "gc_acq_create: NULL argument");
    *out = nullptr;
    return acq_create(ctx, conf, n_sats, AcqEngineSpec{}, out);
}

gc_status gc_acq_create_paired(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, int combine, gc_acq** out)
{
    GC_REQUIRE(ctx && conf && out, "gc_acq_create_paired: NULL argument");
    *out = nullptr;
    GC_REQUIRE(combine == GC_ACQ_COMBINE_MAX || combine == GC_ACQ_COMBINE_SUM, "gc_acq_create_paired: unknown combiner %d", combine);
    AcqEngineSpec spec;
    spec.kind = ACQ_PAIRED;
    spec.combine = combine;
    return acq_create(ctx, conf, n_sats, spec, out);
}

gc_status gc_acq_create_quicksync(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, uint32_t folding_factor, gc_acq** out)
{
    GC_REQUIRE(ctx && conf && out, "gc_acq_create_quicksync: NULL argument");
    *out = nullptr;
    GC_REQUIRE(folding_factor >= 1 && folding_factor <= 100, "gc_acq_create_quicksync: folding factor %u is not in 1 .. 100", folding_factor);
    GC_REQUIRE(!conf->make_2_steps, "gc_acq_create_quicksync: the QuickSync search has no second step");
    GC_REQUIRE(conf->samples_per_code >= 1.0f && conf->samples_per_code < 16777216.0f, "gc_acq_create_quicksync: bad samples_per_code");
    const uint32_t n_code = (uint32_t)conf->samples_per_code;
    GC_REQUIRE(n_code / folding_factor >= 1, "gc_acq_create_quicksync: %u samples per code folded %u times leave no transform", n_code, folding_factor);
    GC_REQUIRE(conf->sampled_ms > 0 && conf->samples_per_ms > 0.0f, "gc_acq_create_quicksync: bad sizes");
    GC_REQUIRE((uint64_t)(conf->sampled_ms * conf->samples_per_ms) >= (uint64_t)n_code * folding_factor,
        "gc_acq_create_quicksync: a block of %u ms does not hold %u code periods of %u samples", conf->sampled_ms, folding_factor, n_code);
    // the engine's view of the configuration: the decision machine (max_dwells, bit_transition_flag, :503-527) belongs to the caller, every
    // dwell stands alone (:340-342) and is judged by max / M^4 / input_power (:422, :480); a doppler_step of 0 means 250 (:219-222)
    gc_acq_conf c = *conf;
    if (c.doppler_step == 0) c.doppler_step = 250;
    c.max_dwells = 1;
    c.bit_transition_flag = 0;
    c.use_CFAR_algorithm_flag = 1;
    c.num_doppler_bins_step2 = 0;
    AcqEngineSpec spec;
    spec.kind = ACQ_QUICKSYNC;
    spec.fold = (int)folding_factor;
    return acq_create(ctx, &c, n_sats, spec, out);
}

gc_status gc_acq_create_tong(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, uint32_t tong_init_val, uint32_t tong_max_val, uint32_t tong_max_dwells,
    gc_acq** out)
{
    GC_REQUIRE(ctx && conf && out, "gc_acq_create_tong: NULL argument");
    *out = nullptr;
    GC_REQUIRE(tong_init_val >= 1 && tong_init_val < tong_max_val, "gc_acq_create_tong: needs 1 <= tong_init_val (%u) < tong_max_val (%u)", tong_init_val,
        tong_max_val);
    GC_REQUIRE(tong_max_dwells >= 1, "gc_acq_create_tong: tong_max_dwells must be >= 1");
    GC_REQUIRE(!conf->bit_transition_flag, "gc_acq_create_tong: the Tong search has no bit transition mode");
    GC_REQUIRE(!conf->make_2_steps, "gc_acq_create_tong: the Tong search has no second step");
    GC_REQUIRE(conf->samples_per_code >= 1.0f && conf->samples_per_code < 16777216.0f, "gc_acq_create_tong: bad samples_per_code");
    // the engine's view of the configuration: one block of sampled_ms * samples_per_ms samples per dwell at that transform size, the
    // grid accumulates until gc_acq_reset(), the decision belongs to the device; a doppler_step of 0 means 250 (the adapters' default)
    gc_acq_conf c = *conf;
    if (c.doppler_step == 0) c.doppler_step = 250;
    c.ms_per_code = c.sampled_ms;
    c.max_dwells = tong_max_dwells;
    c.use_CFAR_algorithm_flag = 0;
    c.num_doppler_bins_step2 = 0;
    AcqEngineSpec spec;
    spec.kind = ACQ_TONG;
    spec.tong = AcqTongParams{INFINITY, tong_init_val, tong_max_val, tong_max_dwells};  // the threshold: gc_acq_tong_set_threshold
    return acq_create(ctx, &c, n_sats, spec, out);
}

gc_status gc_acq_tong_set_threshold(gc_acq* a, float threshold)
{
    GC_REQUIRE(a, "gc_acq_tong_set_threshold: NULL handle");
    if (ACQ_ASK_KIND(a, "gc_acq_tong_set_threshold", ACQ_TONG) != GC_OK) return GC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    a->tong.p.threshold = threshold;  // travels with the decision kernel of every later dwell
    return GC_OK;
}

gc_status gc_acq_create_caf(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, int both_components, int hypotheses, uint32_t caf_window_hz, int arithmetic,
    gc_acq** out)
{
    GC_REQUIRE(conf && out, "gc_acq_create_caf: NULL argument");
    *out = nullptr;
    // what needs no device is checked before the context is looked at
    GC_REQUIRE(both_components == 0 || both_components == 1, "gc_acq_create_caf: both_components %d is not 0 or 1", both_components);
    GC_REQUIRE(hypotheses == 1 || hypotheses == 2, "gc_acq_create_caf: hypotheses %d is not 1 or 2", hypotheses);
    GC_REQUIRE(arithmetic == GC_CAF_REFERENCE || arithmetic == GC_CAF_EXACT, "gc_acq_create_caf: unknown arithmetic %d", arithmetic);
    GC_REQUIRE(conf->doppler_step > 0, "gc_acq_create_caf: doppler_step must be > 0 (the block has no default)");
    GC_REQUIRE(!conf->make_2_steps, "gc_acq_create_caf: the CAF search has no second step");
    GC_REQUIRE(!(conf->bit_transition_flag && conf->max_dwells < 1), "gc_acq_create_caf: bit_transition_flag needs max_dwells >= 1");
    GC_REQUIRE(conf->samples_per_code >= 1.0f && conf->samples_per_code < 16777216.0f, "gc_acq_create_caf: bad samples_per_code");
    const uint64_t n_bins = 2 * (uint64_t)conf->doppler_max / conf->doppler_step + 1;
    GC_REQUIRE(n_bins <= ACQ_CAF_MAX_BINS, "gc_acq_create_caf: %llu Doppler bins, the engine takes at most %d", (unsigned long long)n_bins, ACQ_CAF_MAX_BINS);
    const uint64_t half = (uint64_t)caf_window_hz / (2 * (uint64_t)conf->doppler_step);
    if (caf_window_hz > 0)
        {
            // :689-704: H = 0 divides by zero (0.5 / H), fewer than 2 H + 1 bins read CAF_I out of range
            GC_REQUIRE(half >= 1, "gc_acq_create_caf: a CAF window of %u Hz holds no bin of %u Hz to either side", caf_window_hz, conf->doppler_step);
            GC_REQUIRE(n_bins >= 2 * half + 1, "gc_acq_create_caf: a CAF window of %llu bins to either side needs %llu Doppler bins, the grid has %llu",
                (unsigned long long)half, (unsigned long long)(2 * half + 1), (unsigned long long)n_bins);
        }
    GC_REQUIRE(ctx, "gc_acq_create_caf: NULL context");
    // the engine's view of the configuration: one block of sampled_ms * samples_per_ms samples per dwell at that transform size, every dwell
    // stands alone; the bit transition flag only steers the keep rule of the decision kernel
    gc_acq_conf c = *conf;
    c.ms_per_code = c.sampled_ms;
    c.bit_transition_flag = 0;
    c.max_dwells = 1;
    c.use_CFAR_algorithm_flag = 0;
    c.num_doppler_bins_override = 0;
    c.num_doppler_bins_step2 = 0;
    AcqEngineSpec spec;
    spec.kind = ACQ_CAF;
    spec.caf.both = both_components;
    spec.caf.hyp = hypotheses;
    spec.caf.half = (int)half;
    spec.caf.arithmetic = arithmetic;
    spec.caf.bit_transition = conf->bit_transition_flag ? 1 : 0;
    return acq_create(ctx, &c, n_sats, spec, out);
}

gc_status gc_acq_set_local_code_iq(gc_acq* a, int sat, const float* code_i, const float* code_q)
{
    GC_REQUIRE(a && code_i, "gc_acq_set_local_code_iq: NULL argument");
    if (ACQ_ASK_CODE_ENTRY(a, "gc_acq_set_local_code_iq") != GC_OK) return GC_ERR_INVALID;
    GC_REQUIRE(code_q || !a->caf.p.both, "gc_acq_set_local_code_iq: an engine that searches both components needs code_q");
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_set_local_code_iq: satellite slot %d out of range", sat);
    acq_locked lock(a);
    hipStream_t st = a->ctx->stream;
    const size_t N = a->sz.fft_size, R = (size_t)a->sz.replicas;
    const size_t flip = std::min(N, (size_t)(uint32_t)a->conf.samples_per_code);
    const float* comp[2] = {code_i, code_q};
    // slots IA, QA, IB, QB (:234-282); B: the first code period negated
    size_t slot = R * (size_t)sat;
    for (int h = 0; h < a->caf.p.hyp; h++)
        for (int c = 0; c <= a->caf.p.both; c++, slot++)
            {
                std::vector<float2> buf(N);
                std::memcpy(buf.data(), comp[c], N * sizeof(float2));
                if (h == 1)
                    for (size_t i = 0; i < flip; i++) buf[i] = make_float2(-buf[i].x, -buf[i].y);
                const gc_status s = acq_load_padded(a, st, buf, slot);  // synchronises
                if (s != GC_OK) return s;
            }
    a->code_set[sat] = 1;
    return GC_OK;
}

gc_status gc_acq_caf_vectors(gc_acq* a, int sat, float* caf, float* caf_i, float* caf_q, uint8_t* choice)
{
    GC_REQUIRE(a, "gc_acq_caf_vectors: NULL handle");
    if (ACQ_ASK_KIND(a, "gc_acq_caf_vectors", ACQ_CAF) != GC_OK) return GC_ERR_INVALID;
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_caf_vectors: satellite slot %d out of range", sat);
    acq_locked lock(a);
    const size_t n = a->n_bins, off = (size_t)sat * n;
    if (a->caf.restart)
        {
            // reset and not run: what the first dwell starts from
            if (caf) std::memset(caf, 0, n * sizeof(float));
            if (caf_i) std::memset(caf_i, 0, n * sizeof(float));
            if (caf_q) std::memset(caf_q, 0, n * sizeof(float));
            if (choice) std::memset(choice, 0, n);
            return GC_OK;
        }
    GC_HIP(hipStreamSynchronize(a->ctx->stream));
    if (caf) GC_HIP(hipMemcpy(caf, a->caf.d_caf + off, n * sizeof(float), hipMemcpyDeviceToHost));
    if (caf_i) GC_HIP(hipMemcpy(caf_i, a->caf.d_caf_i + off, n * sizeof(float), hipMemcpyDeviceToHost));
    if (caf_q) GC_HIP(hipMemcpy(caf_q, a->caf.d_caf_q + off, n * sizeof(float), hipMemcpyDeviceToHost));
    if (choice) GC_HIP(hipMemcpy(choice, a->caf.d_choice + off, n, hipMemcpyDeviceToHost));
    return GC_OK;
}

gc_status gc_acq_destroy(gc_acq* a)
{
    if (!a) return GC_OK;
    gc_device_guard g(a->ctx->device);
    // nothing is freed under work that is still running; the buffers then go with the struct, on their device (the guard above)
    (void)hipStreamSynchronize(a->ctx->stream);
    if (a->exp.side) (void)hipStreamSynchronize(a->exp.side);
    delete a;
    return GC_OK;
}

gc_status gc_acq_fft_size(const gc_acq* a, uint32_t* fft_size, uint32_t* consumed_samples, uint32_t* num_doppler_bins)
{
    GC_REQUIRE(a, "gc_acq_fft_size: NULL handle");
    if (fft_size) *fft_size = a->sz.fft_size;
    if (consumed_samples) *consumed_samples = a->sz.consumed;
    if (num_doppler_bins) *num_doppler_bins = a->n_bins;
    return GC_OK;
}

gc_status gc_acq_set_local_code(gc_acq* a, int sat, const float* code)
{
    GC_REQUIRE(a && code, "gc_acq_set_local_code: NULL argument");
    if (ACQ_ASK_CODE_ENTRY(a, "gc_acq_set_local_code") != GC_OK) return GC_ERR_INVALID;
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_set_local_code: satellite slot %d out of range", sat);
    acq_locked lock(a);
    hipStream_t st = a->ctx->stream;
    GC_HIP(acq_flush_inverse(a, st));  // a held-back dwell was searched with the codes of its time (and d_Q is the staging buffer below)
    gc_status s;
    if (a->kind == ACQ_QUICKSYNC)
        {
            // set_local_code (pcps_quicksync_acquisition_cc.cc:178-201): the code itself for the candidate check, and conj(FFT_M) of
            // its f pieces of M samples added in float32, first piece first, onto a zeroed buffer
            const size_t M = a->sz.fft_size;
            const float2* c = reinterpret_cast<const float2*>(code);
            std::vector<float2> cf(M, make_float2(0.f, 0.f));
            for (int i = 0; i < a->qs.fold; i++)
                for (size_t m = 0; m < M; m++) cf[m] = make_float2(cf[m].x + c[i * M + m].x, cf[m].y + c[i * M + m].y);
            GC_HIP(hipMemcpyAsync(a->qs.d_code_time + (size_t)sat * a->qs.code_len, code, sizeof(float2) * a->qs.code_len, hipMemcpyHostToDevice, st));
            s = acq_load_padded(a, st, cf, (size_t)sat);  // synchronises: `code` and cf are free afterwards
        }
    else
        s = acq_load_code(a, st, code, (size_t)sat);
    if (s != GC_OK) return s;
    a->code_set[sat] = 1;
    return GC_OK;
}

gc_status gc_acq_set_local_code_pair(gc_acq* a, int sat, const float* code_a, const float* code_b)
{
    GC_REQUIRE(a && code_a && code_b, "gc_acq_set_local_code_pair: NULL argument");
    if (ACQ_ASK_CODE_ENTRY(a, "gc_acq_set_local_code_pair") != GC_OK) return GC_ERR_INVALID;
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_set_local_code_pair: satellite slot %d out of range", sat);
    acq_locked lock(a);
    hipStream_t st = a->ctx->stream;
    GC_HIP(acq_flush_inverse(a, st));  // as gc_acq_set_local_code (a paired engine holds no dwell back: nothing to run)
    gc_status s = acq_load_code(a, st, code_a, (size_t)2 * sat);
    if (s == GC_OK) s = acq_load_code(a, st, code_b, (size_t)2 * sat + 1);
    if (s != GC_OK) return s;
    a->code_set[sat] = 1;
    return GC_OK;
}

gc_status gc_acq_set_frequency_offset(gc_acq* a, int64_t offset_hz)
{
    GC_REQUIRE(a, "gc_acq_set_frequency_offset: NULL handle");
    if (acq_ask(a, "gc_acq_set_frequency_offset", a->traits().frequency_offset, "has no frequency offset") != GC_OK) return GC_ERR_INVALID;
    acq_locked lock(a);
    if (offset_hz == a->freq_offset_hz && a->wipe_valid) return GC_OK;
    GC_HIP(acq_flush_inverse(a, a->ctx->stream));  // a held-back dwell was wiped off with the tables of its time
    GC_HIP(hipStreamSynchronize(a->ctx->stream));
    a->freq_offset_hz = offset_hz;
    // a failed rebuild leaves wipe_valid clear: searches are refused until a later call (with any offset) has rebuilt the tables
    const hipError_t e = acq_build_main_wipeoffs(a, a->ctx->stream);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_set_frequency_offset: %s", hipGetErrorString(e));
    return GC_OK;
}

gc_status gc_acq_reset(gc_acq* a)
{
    GC_REQUIRE(a, "gc_acq_reset: NULL handle");
    acq_locked lock(a);
    // grid reset (:917-924) and d_num_noncoherent_integrations_counter = 0.  The first dwell after a reset
    // STORES |.|^2 into every kept cell (accumulate = 0), so nothing has to be written here: a 131 MB memset per
    // search at cfg4 sizes, and it would have to be ordered against dwells enqueued on caller streams.
    a->dwell_counter = 0;
    a->grid_logically_zero = true;
    a->held.inv_pending = false;  // a held-back dwell goes with the grid it would have been added to
    if (bool* restart = acq_restart_flag(a)) *restart = true;  // enqueued in front of the next dwell, on its stream
    return GC_OK;
}

gc_status gc_acq_set_step_two(gc_acq* a, int enable, float doppler_center_hz)
{
    GC_REQUIRE(a, "gc_acq_set_step_two: NULL handle");
    if (acq_ask(a, "gc_acq_set_step_two", a->traits().step_two, "has no second step") != GC_OK) return GC_ERR_INVALID;
    acq_locked lock(a);
    hipStream_t st = a->ctx->stream;
    GC_HIP(acq_flush_inverse(a, st));  // a held-back dwell belongs to the grid that is active now
    if (!enable)
        {
            a->step_two = false;
            a->n_bins = a->sz.n_bins;
            a->d_wipe = a->d_wipe_main;
            a->dwell_counter = 0;
            return GC_OK;
        }
    if (!a->conf.make_2_steps || !a->d_wipe2) return gc_fail(GC_ERR_STATE, "gc_acq_set_step_two: the plan was created without make_2_steps");
    const uint32_t n2 = a->conf.num_doppler_bins_step2;
    // update_grid_doppler_wipeoffs_step2 (pcps_acquisition.cc:383-390) + update_local_carrier (:296-310)
    std::vector<float> inc(n2);
    for (uint32_t d = 0; d < n2; d++)
        {
            float doppler = (static_cast<float>(d) - static_cast<float>(std::floor(n2 / 2.0))) * a->conf.doppler_step2;
            float freq = doppler_center_hz + doppler;
            float phase_step_rad = (float)(6.283185307179586 * freq / (float)a->conf.fs_in);
            inc[d] = -phase_step_rad;
        }
    a->wipe2_valid = false;
    const hipError_t e = acq_build_wipeoffs(a, inc, a->d_wipe2, st);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_set_step_two: %s", hipGetErrorString(e));
    a->wipe2_valid = true;
    a->step_two = true;
    a->center_step_two = doppler_center_hz;
    a->n_bins = n2;
    a->d_wipe = a->d_wipe2;
    a->dwell_counter = 0;  // d_num_noncoherent_integrations_counter = 0 (:848)
    return GC_OK;
}

// FFT(x * wipeoff[d]) of `n_blocks` input blocks parked (row-permuted) in d_xw -> d_X[block][bin]: x * wipeoff[d]
// (pcps_acquisition.cc:717) is the two-operand load of the forward row pass (:721), shared by every satellite
static hipError_t acq_forward(gc_acq* a, hipStream_t st, int n_blocks)
{
    const int n_bins = (int)a->n_bins;
    hipError_t e = acq_launch_rows(st, false, a->plan, a->rows, n_blocks * n_bins, a->d_wipe, AcqCellMap{1, n_bins}, a->d_xw, AcqCellMap{n_bins, 1 << 30},
        a->d_Q, a->d_wN2, a->d_wN);
    if (e == hipSuccess) e = acq_launch_cols(st, false, ACQ_EPI_PERM, a->plan, n_blocks * n_bins, a->d_Q, a->d_X, nullptr);
    return e;
}

// Takes the input block `x` of a plain, paired, Tong or CAF dwell: its power if the statistic needs it (`scratch`: with the zeroed
// d_tmp_buffer image of every satellite, :680-688), the block zero padded to fft_size and row-permuted into slot `slot` of d_xw -- the
// caller's buffer is free when this has run -- and the forward transforms of the first `forward_blocks` slots (0: held back)
static hipError_t acq_take_block(gc_acq* a, hipStream_t st, const float2* x, bool power, bool scratch, int slot, int forward_blocks)
{
    const size_t N = a->sz.fft_size;
    hipError_t e = hipSuccess;
    if (power)
        e = acq_launch_input_power(st, x, (int)a->sz.consumed, (int)N, a->d_power, scratch ? a->d_tmp.get() : nullptr, scratch ? a->n_sats : 0, scratch ? N : 0);
    if (e == hipSuccess) e = acq_launch_permute(st, x, nullptr, a->d_xw + (size_t)slot * N, a->plan, (int)a->sz.consumed, 1, 0, 0, 0);
    if (e == hipSuccess && forward_blocks > 0) e = acq_forward(a, st, forward_blocks);
    return e;
}

// The inverse row pass of a batch into Q: * conj(FFT(code)) (pcps_acquisition.cc:724) and the row half of the IFFT (:727).  A satellite
// has R replicas, each multiplied with the first x_spectra spectra of d_X: cell (sat * R + replica) * x_spectra + i reads spectrum i and
// the code of slot sat * R + replica.  x_spectra is n_bins, or 2 * n_bins for a dwell pair ([sat][dwell][bin]).
static hipError_t acq_inverse_rows(gc_acq* a, hipStream_t st, const AcqBatch& b, int R, int x_spectra, float2* Q)
{
    return acq_launch_rows(st, true, a->plan, a->rows, b.ns * R * x_spectra, a->d_X, AcqCellMap{1, x_spectra}, a->d_codes + (size_t)b.s0 * R * a->sz.fft_size,
        AcqCellMap{x_spectra, 1 << 30}, Q, a->d_wN2, a->d_wN);
}

// What the inverse column pass of the batch that starts at satellite s0 writes: `cells` rows per satellite of grid and block maxima,
// the d_tmp_buffer image if `scratch`, delays from `offset` on (bit transition: the second half)
static AcqMagArgs acq_mag_args(const gc_acq* a, int s0, int cells, bool scratch, int offset)
{
    const size_t first = (size_t)s0 * cells, N = a->sz.fft_size;
    AcqMagArgs m;
    m.grid = a->d_grid + first * N;
    m.tmp = scratch ? a->d_tmp + (size_t)s0 * N : nullptr;
    m.blk_max_val = a->d_blkv + first * a->n_blocks;
    m.blk_max_idx = a->d_blki + first * a->n_blocks;
    m.offset = offset;
    m.eff = (int)a->sz.eff;
    m.n_bins = cells;
    m.tmp_bin = cells - 1;
    return m;
}

#ifdef GNSSCORR_EXPERIMENTS
// The inverse passes of acq_inverse in the forms of AcqExperiments, arguments as there.  False: no experiment applies to this call and
// the product passes run; true: one ran, *status tells how.
static bool acq_inverse_experiment(gc_acq* a, hipStream_t st, bool pair, bool accumulate, int per_batch, int x_spectra, int epi, int offset, hipError_t* status)
{
    const AcqExperiments& x = a->exp;
    const int n_bins = (int)a->n_bins;
    const bool batches = x.q_stride != 0 && per_batch < a->n_sats;
    if (x.onchip && acq_inv_fusable(a->plan))
        {
            // one launch, no satellite batches; a pair's two transforms run back to back on the cell's workgroup
            *status = acq_launch_inv_fused(st, a->plan, a->n_sats, n_bins, pair ? 2 : 1, accumulate, a->d_X, a->d_codes, a->d_wN2, a->d_wN,
                acq_mag_args(a, 0, n_bins, true, offset), a->ctx->n_cus);
            return true;
        }
    if (pair && x.roles && batches && !x.overlap)
        {
            // rows(0); rows(b) + columns(b - 1) in one launch, b = 1 ..; columns(last)
            AcqBatch prev{0, 0, 0};
            hipError_t e = acq_for_batches(a->n_sats, per_batch, [&](AcqBatch b) {
                float2* Q = a->d_Q + (size_t)(b.index & 1) * x.q_stride;
                hipError_t eb;
                if (b.index == 0)
                    eb = acq_inverse_rows(a, st, b, 1, x_spectra, Q);
                else
                    eb = acq_launch_rows_cols(st, a->plan, a->rows, b.ns * x_spectra, a->d_X, AcqCellMap{1, x_spectra}, a->d_codes + (size_t)b.s0 * a->sz.fft_size,
                        AcqCellMap{x_spectra, 1 << 30}, Q, a->d_wN2, a->d_wN, epi, prev.ns * n_bins, a->d_Q + (size_t)(prev.index & 1) * x.q_stride,
                        acq_mag_args(a, prev.s0, n_bins, true, offset));
                prev = b;
                return eb;
            });
            if (e == hipSuccess)
                {
                    const AcqMagArgs m = acq_mag_args(a, prev.s0, n_bins, true, offset);
                    e = acq_launch_cols(st, true, epi, a->plan, prev.ns * n_bins, a->d_Q + (size_t)(prev.index & 1) * x.q_stride, nullptr, &m);
                }
            *status = e;
            return true;
        }
    if (x.overlap && batches)
        {
            // rows on `st`, columns on the side stream, the halves of d_Q in turn
            int last = -1;
            hipError_t e = acq_for_batches(a->n_sats, per_batch, [&](AcqBatch b) {
                const int half = b.index & 1;
                float2* Q = a->d_Q + (size_t)half * x.q_stride;
                hipError_t eb = hipSuccess;
                if (b.index >= 2) eb = hipStreamWaitEvent(st, x.ev_cols[half], 0);  // the columns of batch b - 2 have read this half
                if (eb == hipSuccess) eb = acq_inverse_rows(a, st, b, 1, x_spectra, Q);
                if (eb == hipSuccess) eb = hipEventRecord(x.ev_rows[half], st);
                if (eb == hipSuccess) eb = hipStreamWaitEvent(x.side, x.ev_rows[half], 0);
                if (eb != hipSuccess) return eb;
                const AcqMagArgs m = acq_mag_args(a, b.s0, n_bins, true, offset);
                eb = acq_launch_cols(x.side, true, epi, a->plan, b.ns * n_bins, Q, nullptr, &m);
                if (eb == hipSuccess) eb = hipEventRecord(x.ev_cols[half], x.side);
                last = half;
                return eb;
            });
            // everything behind this call on `st` sees the finished grid (the side stream runs its column passes in order: the last one's event covers all)
            if (e == hipSuccess && last >= 0) e = hipStreamWaitEvent(st, x.ev_cols[last], 0);
            *status = e;
            return true;
        }
    return false;
}
#endif

// per satellite and bin: * conj(FFT(code)) (pcps_acquisition.cc:724), IFFT (:727), |.|^2 (+=) (:730-739) of the spectra in d_X, in
// batches of satellites; `pair`: d_X holds two dwells (slot 0, then slot 1 at n_bins spectra), summed into the grid in one pass.
// Plain, paired and QuickSync dwells; the statistics of the dwell become the pending ones.
static hipError_t acq_inverse(gc_acq* a, hipStream_t st, bool pair, bool accumulate)
{
    const int n_bins = (int)a->n_bins;
    const bool bt = a->conf.bit_transition_flag != 0;
    const int offset = bt ? (int)a->sz.eff : 0;
    // a paired engine (never `pair`: it holds no dwell back) runs the dwell's n_bins spectra against replica A, then against replica B
    const int reps = a->sz.replicas;
    const int x_spectra = (pair ? 2 : 1) * n_bins;
    const int per_batch = acq_inverse_sats_per_batch(a->sz.q_cells, reps * x_spectra, a->n_sats);
    int epi = pair ? (accumulate ? ACQ_EPI_MAG2_ACC : ACQ_EPI_MAG2) : (accumulate ? ACQ_EPI_MAG_ACC : ACQ_EPI_MAG);
    if (a->kind == ACQ_PAIRED && a->combine == GC_ACQ_COMBINE_MAX) epi = accumulate ? ACQ_EPI_PMAX_ACC : ACQ_EPI_PMAX;
    if (a->kind == ACQ_PAIRED && a->combine == GC_ACQ_COMBINE_SUM) epi = accumulate ? ACQ_EPI_PSUM_ACC : ACQ_EPI_PSUM;
    hipError_t e = hipSuccess;
#ifdef GNSSCORR_EXPERIMENTS
    if (!acq_inverse_experiment(a, st, pair, accumulate, per_batch, x_spectra, epi, offset, &e))
#endif
        e = acq_for_batches(a->n_sats, per_batch, [&](AcqBatch b) {
            const hipError_t er = acq_inverse_rows(a, st, b, reps, x_spectra, a->d_Q);
            if (er != hipSuccess) return er;
            const AcqMagArgs m = acq_mag_args(a, b.s0, n_bins, true, offset);
            return acq_launch_cols(st, true, epi, a->plan, b.ns * n_bins, a->d_Q, nullptr, &m);
        });
    if (e == hipSuccess)
        {
            AcqFinalArgs f;
            acq_fill_decision_args(a, f);
            f.grid = a->d_grid;
            f.tmp = a->d_tmp;
            f.input_power = (a->sz.use_cfar || bt) ? a->d_power.get() : nullptr;
            f.part_val = a->d_part_val;
            f.part_cnt = a->d_part_cnt;
            f.use_cfar = a->sz.use_cfar ? 1 : 0;
            f.samples_per_chip = (int)a->conf.samples_per_chip;
            f.samples_per_code = a->conf.samples_per_code;
            f.step_two = a->step_two ? 1 : 0;
            f.center_step_two = a->center_step_two;
            f.doppler_step2 = a->conf.doppler_step2;
            f.n_bins_step2 = (int)a->conf.num_doppler_bins_step2;
            a->held.final_args = f;
            a->held.final_stream = st;
            a->held.final_pending = true;
        }
    return e;
}

// runs the held-back inverse passes of the last dwell, if any, on `st` (its statistics become the pending ones)
static hipError_t acq_flush_inverse(gc_acq* a, hipStream_t st)
{
    AcqHeld& h = a->held;
    if (!h.inv_pending) return hipSuccess;
    h.inv_pending = false;
    hipError_t e = acq_order_after(st, h.inv_stream);
    // statistics of an earlier dwell still pending: the dwell held back here accumulates onto that grid (or it would have flushed them)
    if (e == hipSuccess) e = acq_flush_final(a, st, h.inv_accumulate, h.inv_n_bins);
    if (e == hipSuccess) e = acq_forward(a, st, 1);
    if (e == hipSuccess) e = acq_inverse(a, st, false, h.inv_accumulate);
    return e;
}

// One dwell of every satellite slot on `st`, x the float block, per kind:
// plain and paired (pcps_acquisition.cc:668-770)
static hipError_t acq_enqueue_pcps(gc_acq* a, const float2* x, hipStream_t st)
{
    AcqHeld& h = a->held;
    const int n_bins = (int)a->n_bins;
    a->dwell_counter++;
    hipError_t e = hipSuccess;
    const bool bt = a->conf.bit_transition_flag != 0;
    const bool accumulate = a->dwell_counter > 1;
    const bool summed = !a->sz.use_cfar && !bt;  // the statistic of several dwells, which needs no input power
    // a dwell is held back: this one joins it if it adds to the same grid, otherwise the held-back passes run first
    bool pair = false;
    if (h.inv_pending)
        {
            pair = accumulate && summed && h.inv_n_bins == n_bins && h.inv_stream == st;
            if (!pair) e = acq_flush_inverse(a, st);
        }
    if (e == hipSuccess) e = acq_flush_final(a, st, accumulate && summed, n_bins);
    if (e != hipSuccess) return e;
    // more dwells of this search are expected: everything behind the input permutation waits for the next one (AcqHeld)
    const bool hold = !pair && a->traits().holds_back && h.fuse_dwells && summed && a->dwell_counter < a->sz.max_dwells &&
        a->sz.q_cells >= (size_t)2 * n_bins && a->sz.n_bins_alloc >= 2;
    // the second block of a pair goes behind the first one's, and both blocks' forward transforms run in one pair of launches
    if (pair) h.inv_pending = false;
    e = acq_take_block(a, st, x, !summed, true, pair ? 1 : 0, pair ? 2 : hold ? 0 : 1);
    if (e != hipSuccess) return e;
    if (pair) return acq_inverse(a, st, true, h.inv_accumulate);
    if (!hold) return acq_inverse(a, st, false, accumulate);
    h.inv_pending = true;
    h.inv_accumulate = accumulate;
    h.inv_n_bins = n_bins;
    h.inv_stream = st;
    return hipSuccess;
}

// QuickSync (pcps_quicksync_acquisition_cc.cc:340-483), x the block of L samples
static hipError_t acq_enqueue_quicksync(gc_acq* a, const float2* x, hipStream_t st)
{
    const int n_bins = (int)a->n_bins, L = (int)a->sz.consumed, f = a->qs.fold;
    a->dwell_counter = 1;  // d_mag and d_test_statistics restart with every dwell (:340-342): nothing accumulates
    // input power over the L samples (:362-364)
    hipError_t e = acq_launch_input_power(st, x, L, L, a->d_power, nullptr, 0, 0);
    // x * wipeoff[bin] folded f * f times (:382-396) into the rows the forward transform reads, which then runs with no second operand
    if (e == hipSuccess) e = acq_qs_launch_fold(st, x, a->d_wipe, a->d_xw, n_bins, L, f * f, a->plan);
    if (e == hipSuccess) e = acq_launch_rows(st, false, a->plan, a->rows, n_bins, a->d_xw, AcqCellMap{1, n_bins}, nullptr, AcqCellMap{1, 1}, a->d_Q, a->d_wN2, a->d_wN);
    if (e == hipSuccess) e = acq_launch_cols(st, false, ACQ_EPI_PERM, a->plan, n_bins, a->d_Q, a->d_X, nullptr);
    // * conj(FFT_M(folded code)), IFFT_M, |.|^2 stored (:405-414); first maximum and max / M^4 / input_power (:420-422, :480)
    if (e == hipSuccess) e = acq_inverse(a, st, false, false);
    if (e == hipSuccess) e = acq_flush_final(a, st);
    if (e != hipSuccess) return e;
    // the f delays the folded index stands for, correlated in the time domain (:440-474); the winner is read on the device
    AcqQsVerifyArgs v;
    v.x = x;
    v.wipe = a->d_wipe;
    v.codes = a->qs.d_code_time;
    v.results = a->d_results;
    v.cand_val = a->qs.d_cand_val;
    v.cand_delay = a->qs.d_cand_delay;
    v.N = (int)a->qs.code_len;
    v.M = (int)a->sz.fft_size;
    v.L = L;
    v.f = f;
    v.n_bins = n_bins;
    return acq_qs_launch_verify(st, v, a->n_sats);
}

// Tong (pcps_tong_acquisition_cc.cc:310-415)
static hipError_t acq_enqueue_tong(gc_acq* a, const float2* x, hipStream_t st)
{
    const int n_bins = (int)a->n_bins;
    hipError_t e = hipSuccess;
    if (a->tong.restart)
        {
            // set_state(1) / the restart of general_work's state 0 (:230-252, :273-295); the first dwell STORES its cells, so the grid needs no clearing
            e = acq_tong_launch_restart(st, a->tong.d_state, a->tong.d_frozen, a->d_results, a->n_sats, a->tong.p);
            if (e != hipSuccess) return e;
            a->tong.restart = false;
            a->dwell_counter = 0;
        }
    const bool accumulate = a->dwell_counter > 0;
    a->dwell_counter++;
    // input power of this block (:325-327), the block row-permuted, FFT(x * wipeoff[bin]) (:336-341)
    e = acq_take_block(a, st, x, true, false, 0, 1);
    if (e != hipSuccess) return e;
    // * conj(FFT(code)), IFFT, |.|^2 * s (+=) (:345-360) in batches of satellites.  The row pass computes the cells of frozen satellites
    // as well; their column workgroups return at once
    e = acq_for_batches(a->n_sats, a->sz.sats_per_batch, [&](AcqBatch b) {
        const hipError_t er = acq_inverse_rows(a, st, b, 1, n_bins, a->d_Q);
        if (er != hipSuccess) return er;
        return acq_launch_cols_tong(st, accumulate, a->plan, b.ns * n_bins, a->d_Q, acq_mag_args(a, b.s0, n_bins, false, 0), a->tong.d_frozen + b.s0, a->d_power);
    });
    if (e != hipSuccess) return e;
    // maximum, result and decision of every running satellite (:363-415), with every dwell
    AcqTongDecideArgs d;
    acq_fill_decision_args(a, d);
    d.input_power = a->d_power;
    d.state = a->tong.d_state;
    d.frozen = a->tong.d_frozen;
    d.samples_per_code = (unsigned)a->conf.samples_per_code;
    d.p = a->tong.p;
    return acq_tong_launch_decide(st, d, a->n_sats);
}

// CAF (galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc:461-770)
static hipError_t acq_enqueue_caf(gc_acq* a, const float2* x, hipStream_t st)
{
    AcqCaf& c = a->caf;
    const size_t N = a->sz.fft_size;
    const int n_bins = (int)a->n_bins, R = a->sz.replicas;
    hipError_t e = hipSuccess;
    if (c.restart)
        {
            // set_state(1) (:336-349): d_test_statistics = 0 and the Gnss_Synchro fields cleared; every dwell overwrites grid and vectors
            e = hipMemsetAsync(a->d_results, 0, (size_t)a->n_sats * sizeof(gc_acq_result), st);
            if (e != hipSuccess) return e;
            c.restart = false;
        }
    a->dwell_counter = 1;  // nothing accumulates
    // input power of this block (:462-464), the block row-permuted, FFT(x * wipeoff[bin]) (:473-478)
    e = acq_take_block(a, st, x, true, false, 0, 1);
    if (e != hipSuccess) return e;
    const float fnf = (float)N * (float)N, fnf4 = fnf * fnf;
    // * conj(FFT(replica)), IFFT, |.|^2 (:480-524) of the R replicas of a batch of satellites
    e = acq_for_batches(a->n_sats, a->sz.sats_per_batch, [&](AcqBatch b) {
        hipError_t eb = acq_inverse_rows(a, st, b, R, n_bins, a->d_Q);
        if (eb != hipSuccess) return eb;
        // one plane: it is the satellite's grid row (R * n_bins = n_bins cells from s0 on); more: the planes of the batch
        const AcqMagArgs g = acq_mag_args(a, b.s0, n_bins, false, 0);
        AcqMagArgs m = acq_mag_args(a, b.s0, R * n_bins, false, 0);
        if (R > 1)
            {
                m.grid = c.d_planes;
                m.blk_max_val = c.d_plv;
                m.blk_max_idx = c.d_pli;
            }
        eb = acq_launch_cols(st, true, ACQ_EPI_MAG, a->plan, b.ns * R * n_bins, a->d_Q, nullptr, &m);
        if (eb != hipSuccess || R == 1) return eb;
        AcqCafSelectArgs s;
        s.planes = c.d_planes;
        s.pl_max_val = c.d_plv;
        s.pl_max_idx = c.d_pli;
        s.grid = g.grid;
        s.blk_max_val = g.blk_max_val;
        s.blk_max_idx = g.blk_max_idx;
        s.caf_i = c.d_caf_i + (size_t)b.s0 * n_bins;
        s.caf_q = c.d_caf_q + (size_t)b.s0 * n_bins;
        s.choice = c.d_choice + (size_t)b.s0 * n_bins;
        s.n_bins = n_bins;
        s.n_blocks = a->n_blocks;
        s.N = (int)N;
        s.both = c.p.both;
        s.hyp = c.p.hyp;
        s.arithmetic = c.p.arithmetic;
        s.fnf4 = fnf4;
        return acq_caf_launch_select(st, s, b.ns);
    });
    if (e != hipSuccess) return e;
    // d_mag, the keep rule, the result (:634-654), the CAF filter and its argmax (:685-770), with every dwell
    AcqCafDecideArgs d;
    acq_fill_decision_args(a, d);
    d.input_power = a->d_power;
    d.caf = c.d_caf;
    d.caf_i = c.d_caf_i;
    d.caf_q = c.d_caf_q;
    d.choice = c.d_choice;
    d.samples_per_code = (unsigned)a->conf.samples_per_code;
    d.bit_transition = c.p.bit_transition;
    d.both = c.p.both;
    d.single_plane = R == 1 ? 1 : 0;
    d.caf_half = c.p.half;
    d.arithmetic = c.p.arithmetic;
    d.fnf4 = fnf4;
    return acq_caf_launch_decide(st, d, a->n_sats);
}

// one dwell of every satellite slot on `st`; the caller holds the context mutex
static gc_status acq_enqueue(gc_acq* a, const void* dev_iq_in, int iq_format, hipStream_t st)
{
    for (int s = 0; s < a->n_sats; s++)
        if (!a->code_set[s]) return gc_fail(GC_ERR_STATE, "gc_acq_dwell: satellite slot %d has no local code", s);
    if (!(a->step_two ? a->wipe2_valid : a->wipe_valid))
        return gc_fail(GC_ERR_STATE, "gc_acq_dwell: the Doppler wipe-off tables are not valid (a rebuild failed): call gc_acq_set_frequency_offset / gc_acq_set_step_two again");
    const float2* dev_iq = static_cast<const float2*>(dev_iq_in);
    if (iq_format != GC_IQ_F32)
        {
            // d_cshort path of acquisition_core (:676-679): convert the block, then the float search
            hipError_t ec = acq_launch_convert(st, iq_format, dev_iq_in, a->d_cvt, (int)a->sz.consumed);
            if (ec != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_dwell: input conversion failed: %s", hipGetErrorString(ec));
            dev_iq = a->d_cvt;
        }
    static hipError_t (*const dwell_of_kind[])(gc_acq*, const float2*, hipStream_t) = {acq_enqueue_pcps, acq_enqueue_pcps, acq_enqueue_quicksync,
        acq_enqueue_tong, acq_enqueue_caf};  // in the order of AcqKind
    const hipError_t e = dwell_of_kind[a->kind](a, dev_iq, st);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_dwell: kernel launch failed: %s", hipGetErrorString(e));
    a->grid_logically_zero = false;
    return GC_OK;
}

gc_status gc_acq_set_input_format(gc_acq* a, int iq_format)
{
    GC_REQUIRE(a, "gc_acq_set_input_format: NULL handle");
    GC_REQUIRE(iq_format == GC_IQ_F32 || iq_format == GC_IQ_I16 || iq_format == GC_IQ_I8, "gc_acq_set_input_format: unknown format %d", iq_format);
    a->iq_format = iq_format;
    return GC_OK;
}

gc_status gc_acq_dwell_enqueue(gc_acq* a, const void* dev_iq, void* stream)
{
    GC_REQUIRE(a && dev_iq, "gc_acq_dwell_enqueue: NULL argument");
    acq_locked lock(a);
    return acq_enqueue(a, dev_iq, a->iq_format, gc_pick_stream(a->ctx, stream));
}

// results of the last dwell to the host; the caller holds the context mutex
static gc_status acq_fetch(gc_acq* a, gc_acq_result* host_results, hipStream_t st)
{
    const bool* restart = acq_restart_flag(a);
    if (restart && *restart)
        {
            // a Tong or CAF search that has been reset and not run: the results the restart will write
            std::memset(host_results, 0, sizeof(gc_acq_result) * a->n_sats);
            return GC_OK;
        }
    GC_HIP(acq_flush_inverse(a, st));
    GC_HIP(acq_flush_final(a, st));
    GC_HIP(hipMemcpyAsync(a->h_results, a->d_results, sizeof(gc_acq_result) * a->n_sats, hipMemcpyDeviceToHost, st));
    GC_HIP(hipStreamSynchronize(st));
    std::memcpy(host_results, a->h_results, sizeof(gc_acq_result) * a->n_sats);
    return GC_OK;
}

gc_status gc_acq_fetch_results(gc_acq* a, gc_acq_result* host_results, void* stream)
{
    GC_REQUIRE(a && host_results, "gc_acq_fetch_results: NULL argument");
    acq_locked lock(a);
    return acq_fetch(a, host_results, gc_pick_stream(a->ctx, stream));
}

gc_status gc_acq_flush(gc_acq* a, void* stream)
{
    GC_REQUIRE(a, "gc_acq_flush: NULL handle");
    acq_locked lock(a);
    hipStream_t st = gc_pick_stream(a->ctx, stream);
    GC_HIP(acq_flush_inverse(a, st));
    GC_HIP(acq_flush_final(a, st));
    return GC_OK;
}

gc_status gc_acq_dwell_dev(gc_acq* a, const void* dev_iq, gc_acq_result* host_results, void* stream)
{
    GC_REQUIRE(a && dev_iq && host_results, "gc_acq_dwell_dev: NULL argument");
    acq_locked lock(a);
    hipStream_t st = gc_pick_stream(a->ctx, stream);
    gc_status s = acq_enqueue(a, dev_iq, a->iq_format, st);
    if (s != GC_OK) return s;
    return acq_fetch(a, host_results, st);
}

gc_status gc_acq_dwell(gc_acq* a, const float* host_iq, gc_acq_result* host_results)
{
    GC_REQUIRE(a && host_iq && host_results, "gc_acq_dwell: NULL argument");
    acq_locked lock(a);
    hipStream_t st = a->ctx->stream;
    // the host entry point takes gr_complex, whatever the device-side format is; the copy, the search and
    // the read-back stay under one lock because d_in is also set_local_code's staging buffer
    GC_HIP(hipMemcpyAsync(a->d_in, host_iq, sizeof(float2) * a->sz.consumed, hipMemcpyHostToDevice, st));
    gc_status s = acq_enqueue(a, a->d_in, GC_IQ_F32, st);
    if (s != GC_OK) return s;
    return acq_fetch(a, host_results, st);
}

// {state, tong_count, dwell_count} of every satellite to the host; the caller holds the context mutex
static gc_status acq_tong_fetch_status(gc_acq* a, struct gc_acq_tong_status* out, hipStream_t st)
{
    static_assert(sizeof(struct gc_acq_tong_status) == sizeof(AcqTongState), "gc_acq_tong_status is the device record");
    if (a->tong.restart)
        {
            const struct gc_acq_tong_status fresh = {GC_ACQ_TONG_RUNNING, a->tong.p.init_val, 0};
            for (int s = 0; s < a->n_sats; s++) out[s] = fresh;
            return GC_OK;
        }
    GC_HIP(hipMemcpyAsync(a->tong.h_state, a->tong.d_state, sizeof(AcqTongState) * a->n_sats, hipMemcpyDeviceToHost, st));
    GC_HIP(hipStreamSynchronize(st));
    std::memcpy(out, a->tong.h_state, sizeof(AcqTongState) * a->n_sats);
    return GC_OK;
}

// `n` dwells (`tong`: as far as the Tong engine's tong_max_dwells leave room) on consecutive blocks of the ring from first_index on, back
// to back on the context stream -- no host decision, no synchronisation between them -- then one fetch (and the Tong status, if asked
// for); `who`: the public function
static gc_status acq_search_stream(gc_acq* a, const char* who, gc_stream* s, uint64_t first_index, uint32_t n, bool tong, gc_acq_result* host_results,
    struct gc_acq_tong_status* host_status)
{
    GC_REQUIRE(s->ctx->device == a->ctx->device, "%s: the stream lives on another GPU", who);
    GC_REQUIRE(s->iq_format == a->iq_format, "%s: stream format %d, acquisition format %d (gc_acq_set_input_format)", who, s->iq_format, a->iq_format);
    GC_REQUIRE(a->sz.consumed <= s->mirror, "%s: the block of %u samples is longer than the stream's max_window", who, a->sz.consumed);
    acq_locked lock(a);
    hipStream_t st = a->ctx->stream;
    if (tong)
        {
            const uint32_t done = a->tong.restart ? 0u : a->dwell_counter;
            n = std::min(n, done < a->tong.p.max_dwells ? a->tong.p.max_dwells - done : 0u);
        }
    // all blocks are protected against eviction from here (reserved before the residency check and the launches) and checked before
    // the first one is enqueued
    gc_stream_read_set reads(st);
    gc_status rs = reads.add(s, first_index);
    if (rs != GC_OK) return rs;
    const gc_stream_ticket& t = reads.ticket(0);
    const uint64_t span = (uint64_t)n * a->sz.consumed;
    // (head - first_index, not first_index + span: the sum wraps for an index near 2^64)
    if (first_index > t.head || span > t.head - first_index)
        return gc_fail(GC_ERR_INVALID, "%s: blocks [%llu, +%llu) are not inside the stream's resident samples [%llu, %llu)", who,
            (unsigned long long)first_index, (unsigned long long)span, (unsigned long long)t.oldest, (unsigned long long)t.head);
    for (uint32_t k = 0; k < n; k++)
        {
            const uint64_t at = first_index + (uint64_t)k * a->sz.consumed;
            rs = acq_enqueue(a, s->d_ring + (at % s->capacity) * s->elem, a->iq_format, st);
            if (rs != GC_OK) return rs;
        }
    rs = reads.commit();
    if (rs != GC_OK) return rs;
    rs = acq_fetch(a, host_results, st);
    if (rs == GC_OK && host_status) rs = acq_tong_fetch_status(a, host_status, st);
    return rs;
}

gc_status gc_acq_dwell_stream(gc_acq* a, gc_stream* s, uint64_t first_index, gc_acq_result* host_results)
{
    GC_REQUIRE(a && s && host_results, "gc_acq_dwell_stream: NULL argument");
    return acq_search_stream(a, "gc_acq_dwell_stream", s, first_index, 1, false, host_results, nullptr);
}

gc_status gc_acq_tong_status(gc_acq* a, struct gc_acq_tong_status* out)
{
    GC_REQUIRE(a && out, "gc_acq_tong_status: NULL argument");
    if (ACQ_ASK_KIND(a, "gc_acq_tong_status", ACQ_TONG) != GC_OK) return GC_ERR_INVALID;
    acq_locked lock(a);
    return acq_tong_fetch_status(a, out, a->ctx->stream);
}

gc_status gc_acq_tong_search_stream(gc_acq* a, gc_stream* s, uint64_t first_index, uint32_t max_new_dwells, gc_acq_result* host_results,
    struct gc_acq_tong_status* host_status)
{
    GC_REQUIRE(a && s && host_results, "gc_acq_tong_search_stream: NULL argument");
    if (ACQ_ASK_KIND(a, "gc_acq_tong_search_stream", ACQ_TONG) != GC_OK) return GC_ERR_INVALID;
    return acq_search_stream(a, "gc_acq_tong_search_stream", s, first_index, max_new_dwells, true, host_results, host_status);
}

// calculate_threshold of the Tong and QuickSync adapters: the quantile of Exp(lambda) in closed form over `per_bin` cells in each bin,
// the bins counted like init() counts them
static float acq_exp_threshold(double pfa, uint32_t per_bin, double lambda, uint32_t doppler_max, uint32_t doppler_step)
{
    uint32_t bins = 0;
    for (int64_t d = -(int64_t)doppler_max; d <= (int64_t)doppler_max; d += (int64_t)doppler_step) bins++;
    const uint32_t ncells = per_bin * bins;
    const double exponent = 1.0 / (double)ncells;
    const double val = std::pow(1.0 - pfa, exponent);
    return (float)(-std::log(1.0 - val) / lambda);
}

gc_status gc_tong_threshold(float pfa, uint32_t vector_length, uint32_t doppler_max, uint32_t doppler_step, float* out)
{
    GC_REQUIRE(out, "gc_tong_threshold: NULL argument");
    GC_REQUIRE(vector_length >= 1 && doppler_step >= 1, "gc_tong_threshold: bad sizes");
    *out = acq_exp_threshold(pfa, vector_length, (double)vector_length, doppler_max, doppler_step);
    return GC_OK;
}

gc_status gc_acq_get_grid(gc_acq* a, int sat, float* host_grid)
{
    GC_REQUIRE(a && host_grid, "gc_acq_get_grid: NULL argument");
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_get_grid: satellite slot %d out of range", sat);
    acq_locked lock(a);
    const size_t n = (size_t)a->n_bins * a->sz.fft_size;
    if (a->grid_logically_zero)
        {
            std::memset(host_grid, 0, n * sizeof(float));
            return GC_OK;
        }
    GC_HIP(acq_flush_inverse(a, a->ctx->stream));
    GC_HIP(hipStreamSynchronize(a->ctx->stream));
    GC_HIP(hipMemcpy(host_grid, a->d_grid + (size_t)sat * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return GC_OK;
}

// row-permuted P[a][b] = v[a + N1 b]  ->  natural order
static void acq_unpermute(const AcqFftPlan& plan, const float2* p, float* out)
{
    for (int a = 0; a < plan.N1; a++)
        for (int b = 0; b < plan.N2; b++)
            {
                const float2 v = p[(size_t)a * plan.N2 + b];
                out[2 * ((size_t)a + (size_t)plan.N1 * b)] = v.x;
                out[2 * ((size_t)a + (size_t)plan.N1 * b) + 1] = v.y;
            }
}

gc_status gc_acq_peek(gc_acq* a, int what, int index, float* host_out)
{
    GC_REQUIRE(a && host_out, "gc_acq_peek: NULL argument");
    acq_locked lock(a);
    hipStream_t st = a->ctx->stream;
    const size_t N = a->sz.fft_size;
    GC_HIP(acq_flush_inverse(a, st));
    GC_HIP(hipStreamSynchronize(st));
    if (what == GC_ACQ_PEEK_ROW_MAX)
        {
            GC_REQUIRE(index >= 0 && index < a->n_sats, "gc_acq_peek: satellite slot %d out of range", index);
            const size_t n = (size_t)a->n_bins * a->n_blocks;
            std::vector<float> v(n);
            std::vector<unsigned> ix(n);
            GC_HIP(hipMemcpy(v.data(), a->d_blkv + (size_t)index * n, n * sizeof(float), hipMemcpyDeviceToHost));
            GC_HIP(hipMemcpy(ix.data(), a->d_blki + (size_t)index * n, n * sizeof(unsigned), hipMemcpyDeviceToHost));
            for (uint32_t d = 0; d < a->n_bins; d++)
                {
                    float best = -1.0f;
                    unsigned bi = 0xffffffffu;
                    for (int b = 0; b < a->n_blocks; b++)
                        {
                            const size_t e = (size_t)d * a->n_blocks + b;
                            if (ix[e] == 0xffffffffu) continue;
                            if (v[e] > best || (v[e] == best && ix[e] < bi))
                                {
                                    best = v[e];
                                    bi = ix[e];
                                }
                        }
                    host_out[2 * d] = best;
                    host_out[2 * d + 1] = (float)bi;
                }
            return GC_OK;
        }
    const float2* src = nullptr;
    if (what == GC_ACQ_PEEK_WIPEOFF || what == GC_ACQ_PEEK_SPECTRUM)
        {
            GC_REQUIRE(index >= 0 && (uint32_t)index < a->n_bins, "gc_acq_peek: Doppler bin %d out of range", index);
            src = (what == GC_ACQ_PEEK_WIPEOFF ? a->d_wipe : a->d_X) + (size_t)index * N;
        }
    else if (what == GC_ACQ_PEEK_CODE)
        {
            // paired engine: index = 2 * sat + replica; CAF engine: index = R * sat + replica
            GC_REQUIRE(index >= 0 && index < a->sz.replicas * a->n_sats, "gc_acq_peek: code slot %d out of range", index);
            src = a->d_codes + (size_t)index * N;
        }
    else
        return gc_fail(GC_ERR_INVALID, "gc_acq_peek: unknown item %d", what);
    if (a->kind == ACQ_QUICKSYNC && what == GC_ACQ_PEEK_WIPEOFF)
        {
            // the QuickSync table: L samples per bin, in natural order already
            GC_HIP(hipMemcpy(host_out, a->d_wipe + (size_t)index * a->sz.consumed, (size_t)a->sz.consumed * sizeof(float2), hipMemcpyDeviceToHost));
            return GC_OK;
        }
    std::vector<float2> p(N);
    GC_HIP(hipMemcpy(p.data(), src, N * sizeof(float2), hipMemcpyDeviceToHost));
    acq_unpermute(a->plan, p.data(), host_out);  // all three live in the row-permuted layout
    return GC_OK;
}

gc_status gc_acq_quicksync_candidates(gc_acq* a, int sat, uint32_t* possible_delay, float* corr_output_f)
{
    GC_REQUIRE(a && possible_delay && corr_output_f, "gc_acq_quicksync_candidates: NULL argument");
    if (ACQ_ASK_KIND(a, "gc_acq_quicksync_candidates", ACQ_QUICKSYNC) != GC_OK) return GC_ERR_INVALID;
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_quicksync_candidates: satellite slot %d out of range", sat);
    acq_locked lock(a);
    GC_HIP(hipStreamSynchronize(a->ctx->stream));
    GC_HIP(hipMemcpy(possible_delay, a->qs.d_cand_delay + (size_t)sat * a->qs.fold, (size_t)a->qs.fold * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GC_HIP(hipMemcpy(corr_output_f, a->qs.d_cand_val + (size_t)sat * a->qs.fold, (size_t)a->qs.fold * sizeof(float), hipMemcpyDeviceToHost));
    return GC_OK;
}

gc_status gc_quicksync_default_folding_factor(uint32_t code_length, uint32_t* out)
{
    GC_REQUIRE(out, "gc_quicksync_default_folding_factor: NULL argument");
    GC_REQUIRE(code_length >= 1, "gc_quicksync_default_folding_factor: empty code");
    // gps_l1_ca_pcps_quicksync_acquisition.cc: ceil(sqrt(log2(code_length)))
    *out = (uint32_t)std::ceil(std::sqrt(std::log2((double)code_length)));
    return GC_OK;
}

gc_status gc_quicksync_threshold(float pfa, uint32_t code_length, uint32_t folding_factor, uint32_t doppler_max, uint32_t doppler_step, float* out)
{
    GC_REQUIRE(out, "gc_quicksync_threshold: NULL argument");
    GC_REQUIRE(folding_factor >= 1 && doppler_step >= 1 && code_length >= folding_factor, "gc_quicksync_threshold: bad sizes");
    *out = acq_exp_threshold(pfa, code_length / folding_factor, (double)code_length / (double)folding_factor, doppler_max, doppler_step);
    return GC_OK;
}

}  // extern "C"
