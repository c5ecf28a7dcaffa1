// gc_acquisition.hip -- host side of the PCPS acquisition path of libgnsscorr.so.
// Mirrors pcps_acquisition (src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition.cc):
// constructor sizes (:63-190), set_local_code (:239-274), init (:313-368),
// acquisition_core (:668-770) -- batched over n_sats satellites that search the
// same input block.
#include "acq_caf_kernels.h"
#include "acq_kernels.h"
#include "acq_quicksync_kernels.h"
#include "acq_tong_kernels.h"
#include "gc_internal.h"
#include "gc_stream.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

struct gc_acq
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    gc_acq_conf conf{};
    int n_sats = 0;
    uint32_t fft_size = 0, consumed = 0, eff = 0, n_bins = 0;  // n_bins: bins of the ACTIVE grid
    uint32_t n_bins_main = 0, n_bins_alloc = 0;
    bool step_two = false;
    float center_step_two = 0.0f;
    float2* d_wipe_main = nullptr;
    float2* d_wipe2 = nullptr;
    bool use_cfar = false;
    uint32_t max_dwells = 1;
    uint32_t dwell_counter = 0;
    AcqFftPlan plan{};
    int n_blocks = 0;
    int sats_per_batch = 1;
    float2* d_wN = nullptr;
    float2* d_wN2 = nullptr;
    float2* d_wipe = nullptr;
    float2* d_codes = nullptr;
    float2* d_xw = nullptr;
    float2* d_X = nullptr;
    float2* d_Q = nullptr;
    float* d_grid = nullptr;
    float* d_tmp = nullptr;
    float* d_blkv = nullptr;
    unsigned* d_blki = nullptr;
    float* d_power = nullptr;
    float2* d_in = nullptr;
    float2* d_cvt = nullptr;  // converted input block (integer sample formats)
    int iq_format = GC_IQ_F32;
    gc_acq_result* d_results = nullptr;
    gc_acq_result* h_results = nullptr;  // pinned
    float* d_part_val = nullptr;      // acq_final_kernel: second-peak candidates per row piece
    unsigned* d_part_cnt = nullptr;   // and its ticket counters
    std::vector<char> code_set;
    int64_t freq_offset_hz = 0;  // d_old_freq: intermediate frequency / GLONASS FDMA channel offset
    AcqPhaseSeg* d_segs = nullptr;  // closed-form segments of the rows' running phases (acq_phase_segments.h) [seg_cap]
    int* d_seg_off = nullptr;       // [n_bins_alloc + 1]
    size_t seg_cap = 0;
    // the wipe-off tables hold what freq_offset_hz / the step-two centre say: cleared before a rebuild starts, set when it has
    // completed; a search on tables in an unknown state is refused (GC_ERR_STATE) instead of run
    bool wipe_valid = false, wipe2_valid = false;
    bool grid_logically_zero = true;  // gc_acq_reset() since the last dwell: the grid reads as zeros
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
    // sees what per-dwell processing would have produced; gc_acq_reset() drops them with the grid.
    bool inv_pending = false;
    bool inv_accumulate = false;
    int inv_n_bins = 0;
    hipStream_t inv_stream = nullptr;
    bool fuse_dwells = true;  // $GNSSCORR_ACQ_FUSE=0: every dwell on its own
    // Experiment, off by default ($GNSSCORR_ACQ_OVERLAP=1): row pass (instruction- and LDS-bound, 3.8 TB/s) and column pass (bandwidth-
    // bound, 5.6 TB/s) of DIFFERENT satellite batches side by side -- rows on the caller's stream, columns on a stream of the engine,
    // d_Q double-buffered, events both ways.  Measured 0.42 instead of 0.355 ms per search: the row pass holds all the LDS of every CU
    // (4 x 40 KB), so the column workgroups do not become resident beside it and the eight cross-queue hand-overs only add latency
    bool overlap = false;
    // Experiment, off by default ($GNSSCORR_ACQ_ROLES=1): with more than one satellite batch of dwell pairs, the row pass of batch b and
    // the column pass of batch b - 1 share ONE launch (acq_rows3_cols_kernel: of every four workgroups of a CU, 4 - ACQ_ROLE_COLS do rows
    // and ACQ_ROLE_COLS columns), d_Q double-buffered, no events.  Measured 0.44 (one column workgroup of four) and 0.33 (two) against
    // 0.31 ms per search: a column workgroup needs its CU-mates' loads in flight to hide its two load phases, and the row pass slows down
    // with fewer than three workgroups
    bool roles = false;
    // Experiment, off by default ($GNSSCORR_ACQ_ONCHIP=1, experiments build): N = 25 x 1000 plans run the inverse transform of a cell
    // entirely on its CU (acq_inv_fused_kernel, no inter-pass buffer).  Measured 0.525 ms per cfg4 search against 0.311 ms for the
    // two-pass form: DESIGN.md section 3.2
    bool onchip = false;
    hipStream_t side = nullptr;
    hipEvent_t ev_rows[2] = {nullptr, nullptr}, ev_cols[2] = {nullptr, nullptr};
    size_t q_stride = 0;      // float2 elements between the two halves of d_Q (0: single buffer)
    // Paired engine (gc_acq_create_paired): 0, or GC_ACQ_COMBINE_MAX / _SUM.  Every satellite slot holds TWO replicas (d_codes is
    // [sat][2][N]); the inverse row pass runs over 2 * n_bins cells per satellite -- the dwell's n_bins spectra against replica A, then
    // the same spectra against replica B -- and the column pass combines the two |.|^2 of a grid cell before it writes it once
    // (ACQ_EPI_PMAX / _PSUM).  The inter-pass buffer is the one a held-back dwell pair would need, so dwells are never held back.
    int combine = 0;
    int replicas() const { return caf ? caf_p.replicas() : (combine ? 2 : 1); }
    // QuickSync engine (gc_acq_create_quicksync, pcps_quicksync_acquisition_cc.cc): 0, or the folding factor f.  fft_size is M = N / f
    // (N = samples_per_code), consumed is L = f N.  The wipe-off table holds L samples per bin in NATURAL order (the fold kernel and
    // the candidate check read it; no transform does), a dwell folds x * wipeoff into n_bins rows of M samples (acq_qs_fold_kernel,
    // row-permuted into d_xw), runs the transforms and the CFAR statistic of the plain engine at size M -- the grid is overwritten
    // by every dwell, nothing accumulates -- and resolves the f aliased delays on the device (acq_qs_verify_kernel).  Dwells are
    // never held back and the statistics kernel runs with its dwell: the candidate check reads its winner.
    int fold = 0;
    uint32_t qs_code_len = 0;          // N
    AcqFftPlan wipe_plan{};            // N1 = 1, N2 = L: the table builder writes natural order
    float2* d_code_time = nullptr;     // [sat][N]: the codes as handed in (d_code, :182)
    float* d_cand_val = nullptr;       // [sat][f]: d_corr_output_f of the last dwell
    uint32_t* d_cand_delay = nullptr;  // [sat][f]: d_possible_delay
    size_t input_len() const { return fold ? consumed : fft_size; }  // samples of d_in / d_cvt and of a wipe-off row
    // Tong engine (gc_acq_create_tong, pcps_tong_acquisition_cc.cc): fft_size = consumed = sampled_ms * samples_per_ms, the bin grid is
    // inclusive.  Every dwell adds |.|^2 / (N^4 * its own input power) to the grid (acq_launch_cols_tong) and is followed by the
    // decision kernel, which walks each running satellite's counter ON THE DEVICE and freezes the satellites that have decided: their
    // column workgroups return at once from then on, so grid, row maxima and result stay those of the deciding dwell.  Dwells are
    // never held back, nothing is pending behind one, and no call decides on the host.  gc_acq_reset() only marks the restart: the
    // next dwell enqueues it (counters, flags, results) in front of its own work, on its own stream.
    bool tong = false;
    AcqTongParams tong_p{};
    bool tong_restart = true;
    AcqTongState* d_tong_state = nullptr;  // [sat]
    int* d_tong_frozen = nullptr;          // [sat]
    AcqTongState* h_tong_state = nullptr;  // pinned
    // CAF engine (gc_acq_create_caf, galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc): fft_size = consumed = sampled_ms * samples_per_ms, the
    // bin grid is inclusive, a slot holds R = (1 or 2 components) x (1 or 2 hypotheses) replicas in the order IA, QA, IB, QB (d_codes is
    // [sat][R][N]).  The inverse row pass runs over R * n_bins cells per satellite, the column pass (ACQ_EPI_MAG, unchanged) writes the
    // R |.|^2 planes of a batch and their block maxima, acq_caf_select_kernel makes the per-bin choice of hypothesis and builds the grid
    // rows, and acq_caf_decide_kernel -- once per dwell -- the result, the keep rule and the CAF filter.  With R = 1 the column pass
    // writes the grid itself.  Every dwell stands alone; the one thing kept between dwells is gc_acq_result::test_statistics on the
    // device.  gc_acq_reset() only marks the restart: the next dwell zeroes the results in front of its own work, on its own stream.
    struct CafParams
    {
        int both = 0, hyp = 1, half = 0, arithmetic = 0, bit_transition = 0;
        int replicas() const { return (1 + both) * hyp; }
    };
    bool caf = false;
    CafParams caf_p{};
    bool caf_restart = true;
    float* d_planes = nullptr;      // [batch sat][R][n_bins][N] (R >= 2)
    float* d_plv = nullptr;         // their block maxima [batch sat][R][n_bins][n_blocks]
    unsigned* d_pli = nullptr;
    float* d_caf = nullptr;         // [sat][n_bins]
    float* d_caf_i = nullptr;
    float* d_caf_q = nullptr;
    unsigned char* d_choice = nullptr;
};

static hipError_t acq_flush_inverse(gc_acq* a, hipStream_t st);

// runs the pending statistics kernel, if any, on `st`
static hipError_t acq_flush_final(gc_acq* a, hipStream_t st)
{
    if (!a->final_pending) return hipSuccess;
    a->final_pending = false;
    // the dwell it belongs to was enqueued on final_stream: same stream in every sensible use; otherwise order the two
    if (a->final_stream != st)
        {
            hipEvent_t ev;
            hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(ev, a->final_stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
            if (e == hipSuccess) (void)hipEventDestroy(ev);
            if (e != hipSuccess) return e;
        }
    return acq_launch_final(st, a->final_args, a->n_sats);
}

static void acq_release(gc_acq* a)
{
    (void)hipFree(a->d_wN);
    (void)hipFree(a->d_wN2);
    (void)hipFree(a->d_wipe_main);
    (void)hipFree(a->d_wipe2);
    (void)hipFree(a->d_segs);
    (void)hipFree(a->d_seg_off);
    (void)hipFree(a->d_codes);
    (void)hipFree(a->d_xw);
    (void)hipFree(a->d_X);
    (void)hipFree(a->d_Q);
    (void)hipFree(a->d_grid);
    (void)hipFree(a->d_tmp);
    (void)hipFree(a->d_blkv);
    (void)hipFree(a->d_blki);
    (void)hipFree(a->d_power);
    (void)hipFree(a->d_in);
    (void)hipFree(a->d_cvt);
    (void)hipFree(a->d_results);
    (void)hipFree(a->d_part_val);
    (void)hipFree(a->d_part_cnt);
    (void)hipFree(a->d_code_time);
    (void)hipFree(a->d_cand_val);
    (void)hipFree(a->d_cand_delay);
    (void)hipFree(a->d_tong_state);
    (void)hipFree(a->d_tong_frozen);
    (void)hipFree(a->d_planes);
    (void)hipFree(a->d_plv);
    (void)hipFree(a->d_pli);
    (void)hipFree(a->d_caf);
    (void)hipFree(a->d_caf_i);
    (void)hipFree(a->d_caf_q);
    (void)hipFree(a->d_choice);
    if (a->h_tong_state) (void)hipHostFree(a->h_tong_state);
    if (a->h_results) (void)hipHostFree(a->h_results);
    for (int i = 0; i < 2; i++)
        {
            if (a->ev_rows[i]) (void)hipEventDestroy(a->ev_rows[i]);
            if (a->ev_cols[i]) (void)hipEventDestroy(a->ev_cols[i]);
        }
    if (a->side) (void)hipStreamDestroy(a->side);
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
            acq_phase_segments(inc[d], (int)a->input_len(), segs);
            off[d + 1] = (int)segs.size();
        }
    hipError_t e = hipSuccess;
    if (segs.size() > a->seg_cap)
        {
            e = hipStreamSynchronize(st);
            (void)hipFree(a->d_segs);
            a->d_segs = nullptr;
            a->seg_cap = 0;
            if (e == hipSuccess) e = hipMalloc(&a->d_segs, segs.size() * sizeof(AcqPhaseSeg));
            if (e != hipSuccess) return e;
            a->seg_cap = segs.size();
        }
    e = hipMemcpyAsync(a->d_segs, segs.data(), sizeof(AcqPhaseSeg) * segs.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(a->d_seg_off, off.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = acq_launch_wipeoff_segments(st, a->d_segs, a->d_seg_off, table, n, a->fold ? a->wipe_plan : a->plan);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the host vectors go out of scope
    return e;
}

// d_grid_doppler_wipeoffs of the coarse grid: exp(-j*2*pi*(d_old_freq + doppler)/fs * n) with the reference's float32
// running phase (update_grid_doppler_wipeoffs :371-380, update_local_carrier :296-310); d_old_freq = freq_offset_hz
static hipError_t acq_build_main_wipeoffs(gc_acq* a, hipStream_t st)
{
    std::vector<float> inc(a->n_bins_main);
    for (uint32_t d = 0; d < a->n_bins_main; d++)
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

#define ACQ_TRY(call)                                                                                  \
    do                                                                                                 \
        {                                                                                              \
            hipError_t e_ = (call);                                                                    \
            if (e_ != hipSuccess)                                                                      \
                {                                                                                      \
                    acq_release(a);                                                                    \
                    delete a;                                                                          \
                    return gc_fail(GC_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));         \
                }                                                                                      \
        }                                                                                              \
    while (0)

// gc_acq_create (combine = 0), gc_acq_create_paired, gc_acq_create_quicksync (fold = f, conf prepared by the entry point) and
// gc_acq_create_tong (tong = its three counters, conf prepared by the entry point); gc_acq_create_caf (caf = its parameters, likewise)
static gc_status acq_create(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, int combine, int fold, gc_acq** out, const AcqTongParams* tong = nullptr,
    const gc_acq::CafParams* caf = nullptr)
{
    GC_REQUIRE(n_sats > 0, "gc_acq_create: n_sats must be > 0");
    GC_REQUIRE(conf->sampled_ms > 0 && conf->samples_per_ms > 0.0f, "gc_acq_create: bad sizes");
    GC_REQUIRE(conf->doppler_step > 0, "gc_acq_create: doppler_step must be > 0");
    gc_device_guard g(ctx->device);
    gc_acq* a = new gc_acq();
    a->ctx = ctx;
    a->ctx_ref.bind(ctx);
    a->conf = *conf;
    a->n_sats = n_sats;
    a->combine = combine;
    a->fold = fold;
    // pcps_acquisition.cc:77-85, :113-117
    const bool bt = conf->bit_transition_flag != 0;
    a->consumed = (uint32_t)(conf->sampled_ms * conf->samples_per_ms * (bt ? 2 : 1));
    a->fft_size = (conf->sampled_ms == conf->ms_per_code) ? a->consumed : a->consumed * 2;
    a->max_dwells = conf->max_dwells;
    if (bt)
        {
            a->fft_size = a->consumed * 2;
            a->max_dwells = 1;
        }
    a->eff = bt ? a->fft_size / 2 : a->fft_size;
    // :152-159 CFAR statistic only for a single dwell
    a->use_cfar = (a->max_dwells == 1) ? (conf->use_CFAR_algorithm_flag != 0) : false;
    // :326
    a->n_bins = (uint32_t)std::ceil((double)((int32_t)conf->doppler_max - (int32_t)(-(int32_t)conf->doppler_max)) / (double)conf->doppler_step);
    if (fold)
        {
            // pcps_quicksync_acquisition_cc.cc:95 (d_fft_size), :226-231 (the grid includes +doppler_max), :362-364 (f code periods per dwell)
            a->qs_code_len = (uint32_t)conf->samples_per_code;
            a->fft_size = a->qs_code_len / (uint32_t)fold;
            a->consumed = a->qs_code_len * (uint32_t)fold;
            a->eff = a->fft_size;
            a->n_bins = 2 * conf->doppler_max / conf->doppler_step + 1;
            a->wipe_plan.N = a->wipe_plan.N2 = (int)a->consumed;
            a->wipe_plan.N1 = 1;
        }
    if (tong)
        {
            // pcps_tong_acquisition_cc.cc:107 (d_fft_size, no zero padding whatever the code length), :200-205 (the grid includes +doppler_max)
            a->tong = true;
            a->tong_p = *tong;
            a->fft_size = a->eff = a->consumed;
            a->n_bins = 2 * conf->doppler_max / conf->doppler_step + 1;
        }
    if (caf)
        {
            // galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc:100 (d_fft_size, no zero padding of the engine's own), :300-307 (the grid includes +doppler_max)
            a->caf = true;
            a->caf_p = *caf;
            a->fft_size = a->eff = a->consumed;
            a->n_bins = 2 * conf->doppler_max / conf->doppler_step + 1;
        }
    if (conf->num_doppler_bins_override > 0) a->n_bins = conf->num_doppler_bins_override;
    a->n_bins_main = a->n_bins;
    a->n_bins_alloc = a->n_bins;
    if (conf->make_2_steps && conf->num_doppler_bins_step2 > a->n_bins_alloc) a->n_bins_alloc = conf->num_doppler_bins_step2;
    if (a->n_bins == 0 || a->fft_size == 0)
        {
            delete a;
            return gc_fail(GC_ERR_INVALID, "gc_acq_create: empty search grid");
        }
    const size_t lds_limit = 160 * 1024;
    if (!acq_plan_make(&a->plan, (int)a->fft_size, lds_limit))
        {
            delete a;
            return gc_fail(GC_ERR_INVALID, "gc_acq_create: fft_size %u has no supported factorisation", a->fft_size);
        }
    const size_t N = a->fft_size;
    a->n_blocks = acq_cols_blocks(a->plan);
    // scratch Q: a batch of satellites stays within ~140 MB (it lives in the 256 MB Infinity Cache between the two passes), and the
    // batches are equal: a launch's workgroups run in rounds of (CUs x workgroups per CU), so the time of a pass steps with the
    // round count -- 11 + 11 + 10 satellites x 41 bins cost 3 + 3 + 2 rounds of the row pass, 16 + 16 cost 4 + 4 with fewer, larger
    // launches (measured 0.53 -> 0.50 ms per search)
    // (a paired engine's row pass writes 2 * n_bins_alloc cells per satellite; one satellite's pair always fits, whatever the budget says)
    size_t per_sat = (size_t)a->replicas() * a->n_bins_alloc * N * sizeof(float2);
    size_t q_budget = (size_t)140 << 20;
    if (const char* e = std::getenv("GNSSCORR_ACQ_Q_MB")) q_budget = (size_t)std::max(1, std::atoi(e)) << 20;
    a->sats_per_batch = (int)(q_budget / per_sat);
    if (a->sats_per_batch < 1) a->sats_per_batch = 1;
    if (a->sats_per_batch > n_sats) a->sats_per_batch = n_sats;
    {
        const int n_batches = (n_sats + a->sats_per_batch - 1) / a->sats_per_batch;
        a->sats_per_batch = (n_sats + n_batches - 1) / n_batches;
    }
    size_t q_cells = (size_t)a->sats_per_batch * a->replicas() * a->n_bins_alloc;

    ACQ_TRY(hipMalloc(&a->d_wN, N * sizeof(float2)));
    ACQ_TRY(hipMalloc(&a->d_wN2, (size_t)2 * a->plan.N2 * sizeof(float2)));
    ACQ_TRY(hipMalloc(&a->d_wipe_main, (size_t)a->n_bins_main * a->input_len() * sizeof(float2)));
    a->d_wipe = a->d_wipe_main;
    if (conf->make_2_steps && conf->num_doppler_bins_step2 > 0)
        ACQ_TRY(hipMalloc(&a->d_wipe2, (size_t)conf->num_doppler_bins_step2 * N * sizeof(float2)));
    ACQ_TRY(hipMalloc(&a->d_codes, (size_t)a->replicas() * n_sats * N * sizeof(float2)));
    ACQ_TRY(hipMalloc(&a->d_xw, (size_t)a->n_bins_alloc * N * sizeof(float2)));
    ACQ_TRY(hipMalloc(&a->d_X, (size_t)2 * a->n_bins_alloc * N * sizeof(float2)));  // two dwells' spectra (see inv_pending)
    if (const char* e = gc_exp_env("GNSSCORR_ACQ_FUSE")) a->fuse_dwells = std::atoi(e) != 0;
    if (const char* e = gc_exp_env("GNSSCORR_ACQ_OVERLAP")) a->overlap = std::atoi(e) != 0;
    if (const char* e = gc_exp_env("GNSSCORR_ACQ_ROLES")) a->roles = std::atoi(e) != 0;
    if (const char* e = gc_exp_env("GNSSCORR_ACQ_ONCHIP")) a->onchip = std::atoi(e) != 0;
#ifdef GNSSCORR_EXPERIMENTS
    a->roles = a->roles && a->fuse_dwells && acq_rows_cols_fusable(a->plan);
#else
    a->roles = a->overlap = a->onchip = false;
#endif
    if (a->combine || a->caf) a->roles = a->overlap = a->onchip = false;  // the experiment launches know one replica per satellite only
    if (a->roles && n_sats > 1) a->q_stride = q_cells * N;  // second inter-pass buffer
    if (a->overlap && a->sats_per_batch < n_sats)
        {
            // more than one batch: a second buffer, so that the rows of batch b + 1 run beside the columns of batch b
            a->q_stride = q_cells * N;
            ACQ_TRY(hipStreamCreateWithFlags(&a->side, hipStreamNonBlocking));
            for (int i = 0; i < 2; i++)
                {
                    ACQ_TRY(hipEventCreateWithFlags(&a->ev_rows[i], hipEventDisableTiming));
                    ACQ_TRY(hipEventCreateWithFlags(&a->ev_cols[i], hipEventDisableTiming));
                }
        }
    ACQ_TRY(hipMalloc(&a->d_Q, (a->q_stride ? 2 : 1) * q_cells * N * sizeof(float2)));
    a->seg_cap = (size_t)a->n_bins_alloc * 128;
    ACQ_TRY(hipMalloc(&a->d_segs, a->seg_cap * sizeof(AcqPhaseSeg)));
    ACQ_TRY(hipMalloc(&a->d_seg_off, ((size_t)a->n_bins_alloc + 1) * sizeof(int)));
    ACQ_TRY(hipMalloc(&a->d_grid, (size_t)n_sats * a->n_bins_alloc * N * sizeof(float)));
    ACQ_TRY(hipMalloc(&a->d_tmp, (size_t)n_sats * N * sizeof(float)));
    ACQ_TRY(hipMalloc(&a->d_blkv, (size_t)n_sats * a->n_bins_alloc * a->n_blocks * sizeof(float)));
    ACQ_TRY(hipMalloc(&a->d_blki, (size_t)n_sats * a->n_bins_alloc * a->n_blocks * sizeof(unsigned)));
    ACQ_TRY(hipMalloc(&a->d_power, sizeof(float)));
    ACQ_TRY(hipMalloc(&a->d_in, a->input_len() * sizeof(float2)));
    ACQ_TRY(hipMalloc(&a->d_cvt, a->input_len() * sizeof(float2)));
    if (fold)
        {
            ACQ_TRY(hipMalloc(&a->d_code_time, (size_t)n_sats * a->qs_code_len * sizeof(float2)));
            ACQ_TRY(hipMalloc(&a->d_cand_val, (size_t)n_sats * fold * sizeof(float)));
            ACQ_TRY(hipMalloc(&a->d_cand_delay, (size_t)n_sats * fold * sizeof(uint32_t)));
            ACQ_TRY(hipMemset(a->d_code_time, 0, (size_t)n_sats * a->qs_code_len * sizeof(float2)));
            ACQ_TRY(hipMemset(a->d_cand_val, 0, (size_t)n_sats * fold * sizeof(float)));
            ACQ_TRY(hipMemset(a->d_cand_delay, 0, (size_t)n_sats * fold * sizeof(uint32_t)));
        }
    if (tong)
        {
            ACQ_TRY(hipMalloc(&a->d_tong_state, (size_t)n_sats * sizeof(AcqTongState)));
            ACQ_TRY(hipMalloc(&a->d_tong_frozen, (size_t)n_sats * sizeof(int)));
            ACQ_TRY(hipMemset(a->d_tong_state, 0, (size_t)n_sats * sizeof(AcqTongState)));
            ACQ_TRY(hipMemset(a->d_tong_frozen, 0, (size_t)n_sats * sizeof(int)));
            ACQ_TRY(hipHostMalloc(reinterpret_cast<void**>(&a->h_tong_state), (size_t)n_sats * sizeof(AcqTongState), hipHostMallocDefault));
        }
    if (caf)
        {
            const size_t R = (size_t)a->replicas(), rows = (size_t)a->sats_per_batch * R * a->n_bins_alloc, vec = (size_t)n_sats * a->n_bins_alloc;
            if (R > 1)
                {
                    ACQ_TRY(hipMalloc(&a->d_planes, rows * N * sizeof(float)));
                    ACQ_TRY(hipMalloc(&a->d_plv, rows * a->n_blocks * sizeof(float)));
                    ACQ_TRY(hipMalloc(&a->d_pli, rows * a->n_blocks * sizeof(unsigned)));
                }
            ACQ_TRY(hipMalloc(&a->d_caf, vec * sizeof(float)));
            ACQ_TRY(hipMalloc(&a->d_caf_i, vec * sizeof(float)));
            ACQ_TRY(hipMalloc(&a->d_caf_q, vec * sizeof(float)));
            ACQ_TRY(hipMalloc(&a->d_choice, vec));
            ACQ_TRY(hipMemset(a->d_caf, 0, vec * sizeof(float)));
            ACQ_TRY(hipMemset(a->d_caf_i, 0, vec * sizeof(float)));
            ACQ_TRY(hipMemset(a->d_caf_q, 0, vec * sizeof(float)));
            ACQ_TRY(hipMemset(a->d_choice, 0, vec));
        }
    ACQ_TRY(hipMalloc(&a->d_results, (size_t)n_sats * sizeof(gc_acq_result)));
    if (fold) ACQ_TRY(hipMemset(a->d_results, 0, (size_t)n_sats * sizeof(gc_acq_result)));  // the candidate check reads its winner from here
    ACQ_TRY(hipMalloc(&a->d_part_val, (size_t)n_sats * ACQ_FINAL_PIECES * 2 * sizeof(float)));
    ACQ_TRY(hipMalloc(&a->d_part_cnt, (size_t)n_sats * sizeof(unsigned)));
    ACQ_TRY(hipMemset(a->d_part_cnt, 0, (size_t)n_sats * sizeof(unsigned)));
    ACQ_TRY(hipHostMalloc(reinterpret_cast<void**>(&a->h_results), (size_t)n_sats * sizeof(gc_acq_result), hipHostMallocDefault));
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
        ACQ_TRY(hipMemcpy(a->d_wN, w.data(), N * sizeof(float2), hipMemcpyHostToDevice));
        // row-FFT twiddles: per-stage tables + plain table (acq_stage_twiddles)
        std::vector<float2> w2((size_t)2 * a->plan.N2);
        acq_stage_twiddles(a->plan, w2.data());
        ACQ_TRY(hipMemcpy(a->d_wN2, w2.data(), w2.size() * sizeof(float2), hipMemcpyHostToDevice));
    }
    // Doppler wipe-off grid: init() (:340-357) + update_local_carrier (:296-310)
    {
        hipError_t e = acq_build_main_wipeoffs(a, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        ACQ_TRY(e);
    }
    ACQ_TRY(hipMemsetAsync(a->d_grid, 0, (size_t)n_sats * a->n_bins_alloc * N * sizeof(float), st));
    ACQ_TRY(hipMemsetAsync(a->d_tmp, 0, (size_t)n_sats * N * sizeof(float), st));
    ACQ_TRY(hipMemsetAsync(a->d_codes, 0, (size_t)a->replicas() * n_sats * N * sizeof(float2), st));
    ACQ_TRY(hipMemsetAsync(a->d_power, 0, sizeof(float), st));
    ACQ_TRY(hipStreamSynchronize(st));
    *out = a;
    return GC_OK;
}

static gc_status acq_load_padded(gc_acq* a, hipStream_t st, const std::vector<float2>& buf, size_t slot);

// set_local_code (:252-273) of one replica: zero padded, FFT, conjugate, kept in d_codes[slot]; the caller holds the context mutex
static gc_status acq_load_code(gc_acq* a, hipStream_t st, const float* code, size_t slot)
{
    const size_t N = a->fft_size;
    // [0 .. 0 c_0 .. c_L] layouts of set_local_code (:252-269)
    std::vector<float2> buf(N, make_float2(0.f, 0.f));
    const float2* c = reinterpret_cast<const float2*>(code);
    if (a->conf.bit_transition_flag)
        {
            size_t off = N / 2;
            std::memcpy(buf.data() + off, c, sizeof(float2) * off);
        }
    else if (a->fft_size == a->consumed)
        std::memcpy(buf.data(), c, sizeof(float2) * a->consumed);
    else
        std::memcpy(buf.data() + (N - a->consumed), c, sizeof(float2) * a->consumed);
    return acq_load_padded(a, st, buf, slot);
}

static gc_status acq_load_padded(gc_acq* a, hipStream_t st, const std::vector<float2>& buf, size_t slot)
{
    const size_t N = a->fft_size;
    GC_HIP(hipMemcpyAsync(a->d_in, buf.data(), N * sizeof(float2), hipMemcpyHostToDevice, st));
    // FFT, conjugate (:272-273), kept in the row-permuted layout the inverse rows pass reads
    hipError_t e = acq_launch_permute(st, a->d_in, nullptr, a->d_xw, a->plan, (int)N, 1, 0, 0, 0);
    if (e == hipSuccess) e = acq_launch_rows(st, false, a->plan, 1, a->d_xw, AcqCellMap{1, 1}, nullptr, AcqCellMap{1, 1}, a->d_Q, a->d_wN2, a->d_wN);
    if (e == hipSuccess) e = acq_launch_cols(st, false, ACQ_EPI_COMPLEX_CONJ_PERM, a->plan, 1, a->d_Q, a->d_codes + slot * N, nullptr);
    if (e != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_set_local_code: %s", hipGetErrorString(e));
    GC_HIP(hipStreamSynchronize(st));  // buf goes out of scope
    return GC_OK;
}

extern "C" {

gc_status gc_acq_create(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, gc_acq** out)
{
    GC_REQUIRE(ctx && conf && out, "gc_acq_create: NULL argument");
    *out = nullptr;
    return acq_create(ctx, conf, n_sats, 0, 0, out);
}

gc_status gc_acq_create_paired(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, int combine, gc_acq** out)
{
    GC_REQUIRE(ctx && conf && out, "gc_acq_create_paired: NULL argument");
    *out = nullptr;
    GC_REQUIRE(combine == GC_ACQ_COMBINE_MAX || combine == GC_ACQ_COMBINE_SUM, "gc_acq_create_paired: unknown combiner %d", combine);
    return acq_create(ctx, conf, n_sats, combine, 0, out);
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
    return acq_create(ctx, &c, n_sats, 0, (int)folding_factor, out);
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
    AcqTongParams p;
    p.threshold = INFINITY;
    p.init_val = tong_init_val;
    p.max_val = tong_max_val;
    p.max_dwells = tong_max_dwells;
    return acq_create(ctx, &c, n_sats, 0, 0, out, &p);
}

gc_status gc_acq_tong_set_threshold(gc_acq* a, float threshold)
{
    GC_REQUIRE(a, "gc_acq_tong_set_threshold: NULL handle");
    GC_REQUIRE(a->tong, "gc_acq_tong_set_threshold: not a Tong engine (gc_acq_create_tong)");
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    a->tong_p.threshold = threshold;  // travels with the decision kernel of every later dwell
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
    gc_acq::CafParams p;
    p.both = both_components;
    p.hyp = hypotheses;
    p.half = (int)half;
    p.arithmetic = arithmetic;
    p.bit_transition = conf->bit_transition_flag ? 1 : 0;
    return acq_create(ctx, &c, n_sats, 0, 0, out, nullptr, &p);
}

gc_status gc_acq_set_local_code_iq(gc_acq* a, int sat, const float* code_i, const float* code_q)
{
    GC_REQUIRE(a && code_i, "gc_acq_set_local_code_iq: NULL argument");
    GC_REQUIRE(a->caf, "gc_acq_set_local_code_iq: not a CAF engine (gc_acq_create_caf)");
    GC_REQUIRE(code_q || !a->caf_p.both, "gc_acq_set_local_code_iq: an engine that searches both components needs code_q");
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_set_local_code_iq: satellite slot %d out of range", sat);
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = a->ctx->stream;
    const size_t N = a->fft_size, R = (size_t)a->replicas();
    const size_t flip = std::min(N, (size_t)(uint32_t)a->conf.samples_per_code);
    const float* comp[2] = {code_i, code_q};
    // slots IA, QA, IB, QB (:234-282); B: the first code period negated
    size_t slot = R * (size_t)sat;
    for (int h = 0; h < a->caf_p.hyp; h++)
        for (int c = 0; c <= a->caf_p.both; c++, slot++)
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
    GC_REQUIRE(a->caf, "gc_acq_caf_vectors: not a CAF engine (gc_acq_create_caf)");
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_caf_vectors: satellite slot %d out of range", sat);
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    const size_t n = a->n_bins, off = (size_t)sat * n;
    if (a->caf_restart)
        {
            // reset and not run: what the first dwell starts from
            if (caf) std::memset(caf, 0, n * sizeof(float));
            if (caf_i) std::memset(caf_i, 0, n * sizeof(float));
            if (caf_q) std::memset(caf_q, 0, n * sizeof(float));
            if (choice) std::memset(choice, 0, n);
            return GC_OK;
        }
    GC_HIP(hipStreamSynchronize(a->ctx->stream));
    if (caf) GC_HIP(hipMemcpy(caf, a->d_caf + off, n * sizeof(float), hipMemcpyDeviceToHost));
    if (caf_i) GC_HIP(hipMemcpy(caf_i, a->d_caf_i + off, n * sizeof(float), hipMemcpyDeviceToHost));
    if (caf_q) GC_HIP(hipMemcpy(caf_q, a->d_caf_q + off, n * sizeof(float), hipMemcpyDeviceToHost));
    if (choice) GC_HIP(hipMemcpy(choice, a->d_choice + off, n, hipMemcpyDeviceToHost));
    return GC_OK;
}

gc_status gc_acq_destroy(gc_acq* a)
{
    if (!a) return GC_OK;
    gc_device_guard g(a->ctx->device);
    (void)hipStreamSynchronize(a->ctx->stream);
    if (a->side) (void)hipStreamSynchronize(a->side);
    acq_release(a);
    delete a;
    return GC_OK;
}

gc_status gc_acq_fft_size(const gc_acq* a, uint32_t* fft_size, uint32_t* consumed_samples, uint32_t* num_doppler_bins)
{
    GC_REQUIRE(a, "gc_acq_fft_size: NULL handle");
    if (fft_size) *fft_size = a->fft_size;
    if (consumed_samples) *consumed_samples = a->consumed;
    if (num_doppler_bins) *num_doppler_bins = a->n_bins;
    return GC_OK;
}

gc_status gc_acq_set_local_code(gc_acq* a, int sat, const float* code)
{
    GC_REQUIRE(a && code, "gc_acq_set_local_code: NULL argument");
    GC_REQUIRE(!a->combine, "gc_acq_set_local_code: a paired engine takes two replicas per slot (gc_acq_set_local_code_pair)");
    GC_REQUIRE(!a->caf, "gc_acq_set_local_code: a CAF engine takes its components through gc_acq_set_local_code_iq");
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_set_local_code: satellite slot %d out of range", sat);
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = a->ctx->stream;
    GC_HIP(acq_flush_inverse(a, st));  // a held-back dwell was searched with the codes of its time (and d_Q is the staging buffer below)
    if (a->fold)
        {
            // set_local_code (pcps_quicksync_acquisition_cc.cc:178-201): the code itself for the candidate check, and conj(FFT_M) of
            // its f pieces of M samples added in float32, first piece first, onto a zeroed buffer
            const size_t M = a->fft_size;
            const float2* c = reinterpret_cast<const float2*>(code);
            std::vector<float2> cf(M, make_float2(0.f, 0.f));
            for (int i = 0; i < a->fold; i++)
                for (size_t m = 0; m < M; m++) cf[m] = make_float2(cf[m].x + c[i * M + m].x, cf[m].y + c[i * M + m].y);
            GC_HIP(hipMemcpyAsync(a->d_code_time + (size_t)sat * a->qs_code_len, code, sizeof(float2) * a->qs_code_len, hipMemcpyHostToDevice, st));
            const gc_status sq = acq_load_padded(a, st, cf, (size_t)sat);  // synchronises: `code` and cf are free afterwards
            if (sq != GC_OK) return sq;
            a->code_set[sat] = 1;
            return GC_OK;
        }
    const gc_status s = acq_load_code(a, st, code, (size_t)sat);
    if (s != GC_OK) return s;
    a->code_set[sat] = 1;
    return GC_OK;
}

gc_status gc_acq_set_local_code_pair(gc_acq* a, int sat, const float* code_a, const float* code_b)
{
    GC_REQUIRE(a && code_a && code_b, "gc_acq_set_local_code_pair: NULL argument");
    GC_REQUIRE(!a->tong, "gc_acq_set_local_code_pair: a Tong engine takes one replica per slot (gc_acq_set_local_code)");
    GC_REQUIRE(!a->caf, "gc_acq_set_local_code_pair: a CAF engine takes its components through gc_acq_set_local_code_iq");
    GC_REQUIRE(a->combine, "gc_acq_set_local_code_pair: not a paired engine (gc_acq_create_paired)");
    GC_REQUIRE(!a->fold, "gc_acq_set_local_code_pair: a QuickSync engine takes one code period per slot (gc_acq_set_local_code)");
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_set_local_code_pair: satellite slot %d out of range", sat);
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
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
    GC_REQUIRE(!a->fold, "gc_acq_set_frequency_offset: the QuickSync search has no frequency offset");
    GC_REQUIRE(!a->tong, "gc_acq_set_frequency_offset: the Tong search has no frequency offset");
    GC_REQUIRE(!a->caf, "gc_acq_set_frequency_offset: the CAF search has no frequency offset");
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
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
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    // grid reset (:917-924) and d_num_noncoherent_integrations_counter = 0.  The first dwell after a reset
    // STORES |.|^2 into every kept cell (accumulate = 0), so nothing has to be written here: a 131 MB memset per
    // search at cfg4 sizes, and it would have to be ordered against dwells enqueued on caller streams.
    a->dwell_counter = 0;
    a->grid_logically_zero = true;
    a->inv_pending = false;  // a held-back dwell goes with the grid it would have been added to
    a->tong_restart = true;  // Tong engine: counters, frozen flags and results restart in front of the next dwell, on its stream
    a->caf_restart = true;   // CAF engine: the kept statistic and the results are zeroed in front of the next dwell, on its stream
    return GC_OK;
}

gc_status gc_acq_set_step_two(gc_acq* a, int enable, float doppler_center_hz)
{
    GC_REQUIRE(a, "gc_acq_set_step_two: NULL handle");
    GC_REQUIRE(!a->fold, "gc_acq_set_step_two: the QuickSync search has no second step");
    GC_REQUIRE(!a->tong, "gc_acq_set_step_two: the Tong search has no second step");
    GC_REQUIRE(!a->caf, "gc_acq_set_step_two: the CAF search has no second step");
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = a->ctx->stream;
    GC_HIP(acq_flush_inverse(a, st));  // a held-back dwell belongs to the grid that is active now
    if (!enable)
        {
            a->step_two = false;
            a->n_bins = a->n_bins_main;
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

// per satellite and bin: * conj(FFT(code)) (pcps_acquisition.cc:724), IFFT (:727), |.|^2 (+=) (:730-739) of the spectra in d_X, in
// batches of satellites; `pair`: d_X holds two dwells (slot 0, then slot 1 at n_bins spectra), summed into the grid in one pass
static hipError_t acq_inverse(gc_acq* a, hipStream_t st, bool pair, bool accumulate)
{
    const size_t N = a->fft_size;
    const int n_bins = (int)a->n_bins;
    const bool bt = a->conf.bit_transition_flag != 0;
    // a paired engine (never `pair`: it holds no dwell back) runs the dwell's n_bins spectra against replica A, then against replica B
    const int reps = a->replicas();
    const int spectra = (pair ? 2 : reps) * n_bins;  // row-pass cells per satellite
    const int q_cells = a->sats_per_batch * reps * (int)a->n_bins_alloc;
    int per_batch = q_cells / spectra;
    {
        const int n_batches = (a->n_sats + per_batch - 1) / per_batch;
        per_batch = (a->n_sats + n_batches - 1) / n_batches;  // equal batches
    }
    hipError_t e = hipSuccess;
    auto mag_args = [&](int s0) {
        AcqMagArgs m;
        m.grid = a->d_grid + (size_t)s0 * n_bins * N;
        m.tmp = a->d_tmp + (size_t)s0 * N;
        m.blk_max_val = a->d_blkv + (size_t)s0 * n_bins * a->n_blocks;
        m.blk_max_idx = a->d_blki + (size_t)s0 * n_bins * a->n_blocks;
        m.offset = bt ? (int)a->eff : 0;
        m.eff = (int)a->eff;
        m.n_bins = n_bins;
        m.tmp_bin = n_bins - 1;
        return m;
    };
#ifdef GNSSCORR_EXPERIMENTS
    if (a->onchip && acq_inv_fusable(a->plan))
        {
            // N = 25 x 1000: the whole inverse transform of every cell in ONE launch that keeps a cell's values on the CU (no
            // inter-pass buffer, no satellite batches); a pair's two transforms run back to back on the cell's workgroup
            const AcqMagArgs m = mag_args(0);
            e = acq_launch_inv_fused(st, a->plan, a->n_sats, n_bins, pair ? 2 : 1, accumulate, a->d_X, a->d_codes, a->d_wN2, a->d_wN, m, a->ctx->n_cus);
        }
    else if (pair && a->roles && a->q_stride != 0 && per_batch < a->n_sats && !a->overlap)
        {
            // rows(0); rows(b) + columns(b - 1) in one launch, b = 1 ..; columns(last)
            const int epi = accumulate ? ACQ_EPI_MAG2_ACC : ACQ_EPI_MAG2;
            int b = 0, prev_s0 = 0, prev_ns = 0;
            for (int s0 = 0; s0 < a->n_sats && e == hipSuccess; s0 += per_batch, b++)
                {
                    const int ns = std::min(per_batch, a->n_sats - s0);
                    float2* Q = a->d_Q + (size_t)(b & 1) * a->q_stride;
                    if (b == 0)
                        e = acq_launch_rows(st, true, a->plan, ns * spectra, a->d_X, AcqCellMap{1, spectra}, a->d_codes + (size_t)s0 * N,
                            AcqCellMap{spectra, 1 << 30}, Q, a->d_wN2, a->d_wN);
                    else
                        e = acq_launch_rows_cols(st, a->plan, ns * spectra, a->d_X, AcqCellMap{1, spectra}, a->d_codes + (size_t)s0 * N,
                            AcqCellMap{spectra, 1 << 30}, Q, a->d_wN2, a->d_wN, epi, prev_ns * n_bins, a->d_Q + (size_t)((b - 1) & 1) * a->q_stride,
                            mag_args(prev_s0));
                    prev_s0 = s0;
                    prev_ns = ns;
                }
            if (e == hipSuccess)
                {
                    const AcqMagArgs m = mag_args(prev_s0);
                    e = acq_launch_cols(st, true, epi, a->plan, prev_ns * n_bins, a->d_Q + (size_t)((b - 1) & 1) * a->q_stride, nullptr, &m);
                }
        }
    else
#endif
    {
    const bool two_streams = a->overlap && a->q_stride != 0 && per_batch < a->n_sats;
    int b = 0;
    for (int s0 = 0; s0 < a->n_sats && e == hipSuccess; s0 += per_batch, b++)
        {
            const int ns = std::min(per_batch, a->n_sats - s0);
            float2* Q = a->d_Q + (two_streams ? (size_t)(b & 1) * a->q_stride : 0);
            hipStream_t cst = two_streams ? a->side : st;
            if (two_streams && b >= 2) e = hipStreamWaitEvent(st, a->ev_cols[b & 1], 0);  // the columns of batch b - 2 have read this half
            // cell -> (spectrum, replica): [sat][dwell][bin] x d_codes[sat] for a dwell pair, [sat][replica][bin] x d_codes[sat][replica] paired
            const int x_spectra = spectra / reps, code_cells = spectra / reps;
            if (e == hipSuccess)
                e = acq_launch_rows(st, true, a->plan, ns * spectra, a->d_X, AcqCellMap{1, x_spectra}, a->d_codes + (size_t)s0 * reps * N,
                    AcqCellMap{code_cells, 1 << 30}, Q, a->d_wN2, a->d_wN);
            if (e == hipSuccess && two_streams) e = hipEventRecord(a->ev_rows[b & 1], st);
            if (e == hipSuccess && two_streams) e = hipStreamWaitEvent(cst, a->ev_rows[b & 1], 0);
            if (e != hipSuccess) break;
            const AcqMagArgs m = mag_args(s0);
            int epi = pair ? (accumulate ? ACQ_EPI_MAG2_ACC : ACQ_EPI_MAG2) : (accumulate ? ACQ_EPI_MAG_ACC : ACQ_EPI_MAG);
            if (a->combine == GC_ACQ_COMBINE_MAX) epi = accumulate ? ACQ_EPI_PMAX_ACC : ACQ_EPI_PMAX;
            if (a->combine == GC_ACQ_COMBINE_SUM) epi = accumulate ? ACQ_EPI_PSUM_ACC : ACQ_EPI_PSUM;
            e = acq_launch_cols(cst, true, epi, a->plan, ns * n_bins, Q, nullptr, &m);
            if (e == hipSuccess && two_streams) e = hipEventRecord(a->ev_cols[b & 1], cst);
        }
    // everything behind this call on `st` sees the finished grid (the side stream runs its column passes in order: the last one's event covers all)
    if (e == hipSuccess && two_streams && b > 0) e = hipStreamWaitEvent(st, a->ev_cols[(b - 1) & 1], 0);
    }
    if (e == hipSuccess)
        {
            AcqFinalArgs f;
            f.grid = a->d_grid;
            f.tmp = a->d_tmp;
            f.blk_max_val = a->d_blkv;
            f.blk_max_idx = a->d_blki;
            f.input_power = (a->use_cfar || bt) ? a->d_power : nullptr;
            f.results = a->d_results;
            f.part_val = a->d_part_val;
            f.part_cnt = a->d_part_cnt;
            f.n_bins = n_bins;
            f.n_blocks = a->n_blocks;
            f.fft_size = (int)N;
            f.doppler_max = (int)a->conf.doppler_max;
            f.doppler_step = (int)a->conf.doppler_step;
            f.use_cfar = a->use_cfar ? 1 : 0;
            f.samples_per_chip = (int)a->conf.samples_per_chip;
            f.samples_per_code = a->conf.samples_per_code;
            f.step_two = a->step_two ? 1 : 0;
            f.center_step_two = a->center_step_two;
            f.doppler_step2 = a->conf.doppler_step2;
            f.n_bins_step2 = (int)a->conf.num_doppler_bins_step2;
            a->final_args = f;
            a->final_stream = st;
            a->final_pending = true;
        }
    return e;
}

// FFT(x * wipeoff[d]) of `n_blocks` input blocks parked (row-permuted) in d_xw -> d_X[block][bin]: x * wipeoff[d]
// (pcps_acquisition.cc:717) is the two-operand load of the forward row pass (:721), shared by every satellite
static hipError_t acq_forward(gc_acq* a, hipStream_t st, int n_blocks)
{
    const int n_bins = (int)a->n_bins;
    hipError_t e = acq_launch_rows(st, false, a->plan, n_blocks * n_bins, a->d_wipe, AcqCellMap{1, n_bins}, a->d_xw, AcqCellMap{n_bins, 1 << 30},
        a->d_Q, a->d_wN2, a->d_wN);
    if (e == hipSuccess) e = acq_launch_cols(st, false, ACQ_EPI_PERM, a->plan, n_blocks * n_bins, a->d_Q, a->d_X, nullptr);
    return e;
}

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

// runs the held-back inverse passes of the last dwell, if any, on `st` (its statistics become the pending ones)
static hipError_t acq_flush_inverse(gc_acq* a, hipStream_t st)
{
    if (!a->inv_pending) return hipSuccess;
    a->inv_pending = false;
    hipError_t e = acq_order_after(st, a->inv_stream);
    // statistics of an earlier dwell still pending: the dwell held back here accumulates onto that grid (or it would have flushed them)
    if (e == hipSuccess && a->final_pending)
        {
            const bool reproduces = a->inv_accumulate && a->final_args.n_bins == a->inv_n_bins && a->final_stream == st;
            if (reproduces)
                a->final_pending = false;
            else
                e = acq_flush_final(a, st);
        }
    if (e == hipSuccess) e = acq_forward(a, st, 1);
    if (e == hipSuccess) e = acq_inverse(a, st, false, a->inv_accumulate);
    return e;
}

// one QuickSync dwell (pcps_quicksync_acquisition_cc.cc:340-483) of every satellite slot on `st`, x the float block of L samples
static hipError_t acq_enqueue_quicksync(gc_acq* a, const float2* x, hipStream_t st)
{
    const int n_bins = (int)a->n_bins, L = (int)a->consumed;
    a->dwell_counter = 1;  // d_mag and d_test_statistics restart with every dwell (:340-342): nothing accumulates
    // input power over the L samples (:362-364)
    hipError_t e = acq_launch_input_power(st, x, L, L, a->d_power, nullptr, 0, 0);
    // x * wipeoff[bin] folded f * f times (:382-396) into the rows the forward transform reads, which then runs with no second operand
    if (e == hipSuccess) e = acq_qs_launch_fold(st, x, a->d_wipe, a->d_xw, n_bins, L, a->fold * a->fold, a->plan);
    if (e == hipSuccess) e = acq_launch_rows(st, false, a->plan, n_bins, a->d_xw, AcqCellMap{1, n_bins}, nullptr, AcqCellMap{1, 1}, a->d_Q, a->d_wN2, a->d_wN);
    if (e == hipSuccess) e = acq_launch_cols(st, false, ACQ_EPI_PERM, a->plan, n_bins, a->d_Q, a->d_X, nullptr);
    // * conj(FFT_M(folded code)), IFFT_M, |.|^2 stored (:405-414); first maximum and max / M^4 / input_power (:420-422, :480)
    if (e == hipSuccess) e = acq_inverse(a, st, false, false);
    if (e == hipSuccess) e = acq_flush_final(a, st);
    // the f delays the folded index stands for, correlated in the time domain (:440-474); the winner is read on the device
    if (e == hipSuccess)
        {
            AcqQsVerifyArgs v;
            v.x = x;
            v.wipe = a->d_wipe;
            v.codes = a->d_code_time;
            v.results = a->d_results;
            v.cand_val = a->d_cand_val;
            v.cand_delay = a->d_cand_delay;
            v.N = (int)a->qs_code_len;
            v.M = (int)a->fft_size;
            v.L = L;
            v.f = a->fold;
            v.n_bins = n_bins;
            e = acq_qs_launch_verify(st, v, a->n_sats);
        }
    return e;
}

// one Tong dwell (pcps_tong_acquisition_cc.cc:310-415) of every satellite slot on `st`, x the float block of N samples
static hipError_t acq_enqueue_tong(gc_acq* a, const float2* x, hipStream_t st)
{
    const size_t N = a->fft_size;
    const int n_bins = (int)a->n_bins;
    hipError_t e = hipSuccess;
    if (a->tong_restart)
        {
            // set_state(1) / the restart of general_work's state 0 (:230-252, :273-295); the first dwell STORES its cells, so the grid needs no clearing
            e = acq_tong_launch_restart(st, a->d_tong_state, a->d_tong_frozen, a->d_results, a->n_sats, a->tong_p);
            if (e != hipSuccess) return e;
            a->tong_restart = false;
            a->dwell_counter = 0;
        }
    const bool accumulate = a->dwell_counter > 0;
    a->dwell_counter++;
    // input power of this block (:325-327), the block row-permuted, FFT(x * wipeoff[bin]) (:336-341)
    e = acq_launch_input_power(st, x, (int)a->consumed, (int)N, a->d_power, nullptr, 0, 0);
    if (e == hipSuccess) e = acq_launch_permute(st, x, nullptr, a->d_xw, a->plan, (int)a->consumed, 1, 0, 0, 0);
    if (e == hipSuccess) e = acq_forward(a, st, 1);
    // * conj(FFT(code)), IFFT, |.|^2 * s (+=) (:345-360) in batches of satellites.  The row pass computes the cells of frozen satellites
    // as well; their column workgroups return at once
    for (int s0 = 0; s0 < a->n_sats && e == hipSuccess; s0 += a->sats_per_batch)
        {
            const int ns = std::min(a->sats_per_batch, a->n_sats - s0);
            e = acq_launch_rows(st, true, a->plan, ns * n_bins, a->d_X, AcqCellMap{1, n_bins}, a->d_codes + (size_t)s0 * N, AcqCellMap{n_bins, 1 << 30}, a->d_Q,
                a->d_wN2, a->d_wN);
            if (e != hipSuccess) break;
            AcqMagArgs m;
            m.grid = a->d_grid + (size_t)s0 * n_bins * N;
            m.tmp = nullptr;
            m.blk_max_val = a->d_blkv + (size_t)s0 * n_bins * a->n_blocks;
            m.blk_max_idx = a->d_blki + (size_t)s0 * n_bins * a->n_blocks;
            m.offset = 0;
            m.eff = (int)a->eff;
            m.n_bins = n_bins;
            m.tmp_bin = n_bins - 1;
            e = acq_launch_cols_tong(st, accumulate, a->plan, ns * n_bins, a->d_Q, m, a->d_tong_frozen + s0, a->d_power);
        }
    // maximum, result and decision of every running satellite (:363-415), with every dwell
    if (e == hipSuccess)
        {
            AcqTongDecideArgs d;
            d.blk_max_val = a->d_blkv;
            d.blk_max_idx = a->d_blki;
            d.input_power = a->d_power;
            d.results = a->d_results;
            d.state = a->d_tong_state;
            d.frozen = a->d_tong_frozen;
            d.n_bins = n_bins;
            d.n_blocks = a->n_blocks;
            d.fft_size = (int)N;
            d.doppler_max = (int)a->conf.doppler_max;
            d.doppler_step = (int)a->conf.doppler_step;
            d.samples_per_code = (unsigned)a->conf.samples_per_code;
            d.p = a->tong_p;
            e = acq_tong_launch_decide(st, d, a->n_sats);
        }
    return e;
}

// one CAF dwell (galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc:461-770) of every satellite slot on `st`, x the float block of N samples
static hipError_t acq_enqueue_caf(gc_acq* a, const float2* x, hipStream_t st)
{
    const size_t N = a->fft_size;
    const int n_bins = (int)a->n_bins, R = a->replicas();
    hipError_t e = hipSuccess;
    if (a->caf_restart)
        {
            // set_state(1) (:336-349): d_test_statistics = 0 and the Gnss_Synchro fields cleared; every dwell overwrites grid and vectors
            e = hipMemsetAsync(a->d_results, 0, (size_t)a->n_sats * sizeof(gc_acq_result), st);
            if (e != hipSuccess) return e;
            a->caf_restart = false;
        }
    a->dwell_counter = 1;  // nothing accumulates
    // input power of this block (:462-464), the block row-permuted, FFT(x * wipeoff[bin]) (:473-478)
    e = acq_launch_input_power(st, x, (int)a->consumed, (int)N, a->d_power, nullptr, 0, 0);
    if (e == hipSuccess) e = acq_launch_permute(st, x, nullptr, a->d_xw, a->plan, (int)a->consumed, 1, 0, 0, 0);
    if (e == hipSuccess) e = acq_forward(a, st, 1);
    const float fnf = (float)N * (float)N, fnf4 = fnf * fnf;
    // * conj(FFT(replica)), IFFT, |.|^2 (:480-524) of the R replicas of a batch of satellites: cell = (sat * R + replica) * n_bins + bin
    // reads spectrum cell % n_bins and code cell / n_bins of the batch's [sat][R] slots
    for (int s0 = 0; s0 < a->n_sats && e == hipSuccess; s0 += a->sats_per_batch)
        {
            const int ns = std::min(a->sats_per_batch, a->n_sats - s0);
            e = acq_launch_rows(st, true, a->plan, ns * R * n_bins, a->d_X, AcqCellMap{1, n_bins}, a->d_codes + (size_t)s0 * R * N, AcqCellMap{n_bins, 1 << 30},
                a->d_Q, a->d_wN2, a->d_wN);
            if (e != hipSuccess) break;
            float* g_grid = a->d_grid + (size_t)s0 * n_bins * N;
            float* g_blkv = a->d_blkv + (size_t)s0 * n_bins * a->n_blocks;
            unsigned* g_blki = a->d_blki + (size_t)s0 * n_bins * a->n_blocks;
            AcqMagArgs m;
            m.grid = R > 1 ? a->d_planes : g_grid;  // one plane: it is the grid row
            m.tmp = nullptr;
            m.blk_max_val = R > 1 ? a->d_plv : g_blkv;
            m.blk_max_idx = R > 1 ? a->d_pli : g_blki;
            m.offset = 0;
            m.eff = (int)a->eff;
            m.n_bins = R * n_bins;
            m.tmp_bin = R * n_bins - 1;
            e = acq_launch_cols(st, true, ACQ_EPI_MAG, a->plan, ns * R * n_bins, a->d_Q, nullptr, &m);
            if (e != hipSuccess || R == 1) continue;
            AcqCafSelectArgs s;
            s.planes = a->d_planes;
            s.pl_max_val = a->d_plv;
            s.pl_max_idx = a->d_pli;
            s.grid = g_grid;
            s.blk_max_val = g_blkv;
            s.blk_max_idx = g_blki;
            s.caf_i = a->d_caf_i + (size_t)s0 * n_bins;
            s.caf_q = a->d_caf_q + (size_t)s0 * n_bins;
            s.choice = a->d_choice + (size_t)s0 * n_bins;
            s.n_bins = n_bins;
            s.n_blocks = a->n_blocks;
            s.N = (int)N;
            s.both = a->caf_p.both;
            s.hyp = a->caf_p.hyp;
            s.arithmetic = a->caf_p.arithmetic;
            s.fnf4 = fnf4;
            e = acq_caf_launch_select(st, s, ns);
        }
    // d_mag, the keep rule, the result (:634-654), the CAF filter and its argmax (:685-770), with every dwell
    if (e == hipSuccess)
        {
            AcqCafDecideArgs d;
            d.blk_max_val = a->d_blkv;
            d.blk_max_idx = a->d_blki;
            d.input_power = a->d_power;
            d.results = a->d_results;
            d.caf = a->d_caf;
            d.caf_i = a->d_caf_i;
            d.caf_q = a->d_caf_q;
            d.choice = a->d_choice;
            d.n_bins = n_bins;
            d.n_blocks = a->n_blocks;
            d.fft_size = (int)N;
            d.doppler_max = (int)a->conf.doppler_max;
            d.doppler_step = (int)a->conf.doppler_step;
            d.samples_per_code = (unsigned)a->conf.samples_per_code;
            d.bit_transition = a->caf_p.bit_transition;
            d.both = a->caf_p.both;
            d.single_plane = R == 1 ? 1 : 0;
            d.caf_half = a->caf_p.half;
            d.arithmetic = a->caf_p.arithmetic;
            d.fnf4 = fnf4;
            e = acq_caf_launch_decide(st, d, a->n_sats);
        }
    return e;
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
            hipError_t ec = acq_launch_convert(st, iq_format, dev_iq_in, a->d_cvt, (int)a->consumed);
            if (ec != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_dwell: input conversion failed: %s", hipGetErrorString(ec));
            dev_iq = a->d_cvt;
        }
    if (a->tong)
        {
            const hipError_t et = acq_enqueue_tong(a, dev_iq, st);
            if (et != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_dwell: kernel launch failed: %s", hipGetErrorString(et));
            a->grid_logically_zero = false;
            return GC_OK;
        }
    if (a->caf)
        {
            const hipError_t ec = acq_enqueue_caf(a, dev_iq, st);
            if (ec != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_dwell: kernel launch failed: %s", hipGetErrorString(ec));
            a->grid_logically_zero = false;
            return GC_OK;
        }
    if (a->fold)
        {
            const hipError_t eq = acq_enqueue_quicksync(a, dev_iq, st);
            if (eq != hipSuccess) return gc_fail(GC_ERR_HIP, "gc_acq_dwell: kernel launch failed: %s", hipGetErrorString(eq));
            a->grid_logically_zero = false;
            return GC_OK;
        }
    const size_t N = a->fft_size;
    const int n_bins = (int)a->n_bins;
    a->dwell_counter++;
    hipError_t e = hipSuccess;
    const bool bt = a->conf.bit_transition_flag != 0;
    const bool accumulate = a->dwell_counter > 1;
    const bool plain = !a->use_cfar && !bt;
    // a dwell is held back: this one joins it if it adds to the same grid, otherwise the held-back passes run first
    bool pair = false;
    if (a->inv_pending)
        {
            pair = accumulate && plain && a->inv_n_bins == n_bins && a->inv_stream == st;
            if (!pair) e = acq_flush_inverse(a, st);
        }
    if (e == hipSuccess && a->final_pending)
        {
            // an accumulating dwell on the same grid overwrites the scratch the pending evaluation would have left: drop it
            const bool reproduces = accumulate && plain && a->final_args.n_bins == n_bins && a->final_stream == st;
            if (reproduces)
                a->final_pending = false;
            else
                e = acq_flush_final(a, st);
        }
    if (e == hipSuccess && (a->use_cfar || bt))
        e = acq_launch_input_power(st, dev_iq, (int)a->consumed, (int)N, a->d_power, a->d_tmp, a->n_sats, N);
    // the input block, zero padded to fft_size (:680-688), row-permuted once: the caller's buffer is free when this has run.  The
    // second block of a pair goes behind the first one's
    if (e == hipSuccess) e = acq_launch_permute(st, dev_iq, nullptr, a->d_xw + (pair ? N : 0), a->plan, (int)a->consumed, 1, 0, 0, 0);
    if (e == hipSuccess)
        {
            const int q_cells = a->sats_per_batch * (int)a->n_bins_alloc;
            if (pair)
                {
                    // both blocks' forward transforms in one pair of launches, then both dwells' inverse passes
                    a->inv_pending = false;
                    e = acq_forward(a, st, 2);
                    if (e == hipSuccess) e = acq_inverse(a, st, true, a->inv_accumulate);
                }
            else if (a->fuse_dwells && !a->combine && plain && a->dwell_counter < a->max_dwells && q_cells >= 2 * n_bins && a->n_bins_alloc >= 2)
                {
                    // more dwells of this search are expected: hold everything behind the input permutation back (see gc_acq::inv_pending)
                    a->inv_pending = true;
                    a->inv_accumulate = accumulate;
                    a->inv_n_bins = n_bins;
                    a->inv_stream = st;
                }
            else
                {
                    e = acq_forward(a, st, 1);
                    if (e == hipSuccess) e = acq_inverse(a, st, false, accumulate);
                }
        }
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
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    return acq_enqueue(a, dev_iq, a->iq_format, gc_pick_stream(a->ctx, stream));
}

// results of the last dwell to the host; the caller holds the context mutex
static gc_status acq_fetch(gc_acq* a, gc_acq_result* host_results, hipStream_t st)
{
    if ((a->tong && a->tong_restart) || (a->caf && a->caf_restart))
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
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    return acq_fetch(a, host_results, gc_pick_stream(a->ctx, stream));
}

gc_status gc_acq_flush(gc_acq* a, void* stream)
{
    GC_REQUIRE(a, "gc_acq_flush: NULL handle");
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = gc_pick_stream(a->ctx, stream);
    GC_HIP(acq_flush_inverse(a, st));
    GC_HIP(acq_flush_final(a, st));
    return GC_OK;
}

gc_status gc_acq_dwell_dev(gc_acq* a, const void* dev_iq, gc_acq_result* host_results, void* stream)
{
    GC_REQUIRE(a && dev_iq && host_results, "gc_acq_dwell_dev: NULL argument");
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = gc_pick_stream(a->ctx, stream);
    gc_status s = acq_enqueue(a, dev_iq, a->iq_format, st);
    if (s != GC_OK) return s;
    return acq_fetch(a, host_results, st);
}

gc_status gc_acq_dwell(gc_acq* a, const float* host_iq, gc_acq_result* host_results)
{
    GC_REQUIRE(a && host_iq && host_results, "gc_acq_dwell: NULL argument");
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = a->ctx->stream;
    // the host entry point takes gr_complex, whatever the device-side format is; the copy, the search and
    // the read-back stay under one lock because d_in is also set_local_code's staging buffer
    GC_HIP(hipMemcpyAsync(a->d_in, host_iq, sizeof(float2) * a->consumed, hipMemcpyHostToDevice, st));
    gc_status s = acq_enqueue(a, a->d_in, GC_IQ_F32, st);
    if (s != GC_OK) return s;
    return acq_fetch(a, host_results, st);
}

gc_status gc_acq_dwell_stream(gc_acq* a, gc_stream* s, uint64_t first_index, gc_acq_result* host_results)
{
    GC_REQUIRE(a && s && host_results, "gc_acq_dwell_stream: NULL argument");
    GC_REQUIRE(s->ctx->device == a->ctx->device, "gc_acq_dwell_stream: the stream lives on another GPU");
    GC_REQUIRE(s->iq_format == a->iq_format, "gc_acq_dwell_stream: stream format %d, acquisition format %d (gc_acq_set_input_format)",
        s->iq_format, a->iq_format);
    GC_REQUIRE(a->consumed <= s->mirror, "gc_acq_dwell_stream: the block of %u samples is longer than the stream's max_window", a->consumed);
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = a->ctx->stream;
    // the block is protected against eviction from here (reserved before the residency check and the launch)
    gc_stream_read_set reads(st);
    gc_status rs = reads.add(s, first_index);
    if (rs != GC_OK) return rs;
    const gc_stream_ticket& t = reads.ticket(0);
    if (first_index + a->consumed > t.head)
        return gc_fail(GC_ERR_INVALID, "gc_acq_dwell_stream: block [%llu, +%u) is not inside the stream's resident samples [%llu, %llu)",
            (unsigned long long)first_index, a->consumed, (unsigned long long)t.oldest, (unsigned long long)t.head);
    rs = acq_enqueue(a, s->d_ring + (first_index % s->capacity) * s->elem, a->iq_format, st);
    if (rs != GC_OK) return rs;
    rs = reads.commit();
    if (rs != GC_OK) return rs;
    return acq_fetch(a, host_results, st);
}

// {state, tong_count, dwell_count} of every satellite to the host; the caller holds the context mutex
static gc_status acq_tong_fetch_status(gc_acq* a, struct gc_acq_tong_status* out, hipStream_t st)
{
    static_assert(sizeof(struct gc_acq_tong_status) == sizeof(AcqTongState), "gc_acq_tong_status is the device record");
    if (a->tong_restart)
        {
            for (int s = 0; s < a->n_sats; s++)
                {
                    out[s].state = GC_ACQ_TONG_RUNNING;
                    out[s].tong_count = a->tong_p.init_val;
                    out[s].dwell_count = 0;
                }
            return GC_OK;
        }
    GC_HIP(hipMemcpyAsync(a->h_tong_state, a->d_tong_state, sizeof(AcqTongState) * a->n_sats, hipMemcpyDeviceToHost, st));
    GC_HIP(hipStreamSynchronize(st));
    std::memcpy(out, a->h_tong_state, sizeof(AcqTongState) * a->n_sats);
    return GC_OK;
}

gc_status gc_acq_tong_status(gc_acq* a, struct gc_acq_tong_status* out)
{
    GC_REQUIRE(a && out, "gc_acq_tong_status: NULL argument");
    GC_REQUIRE(a->tong, "gc_acq_tong_status: not a Tong engine (gc_acq_create_tong)");
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    return acq_tong_fetch_status(a, out, a->ctx->stream);
}

gc_status gc_acq_tong_search_stream(gc_acq* a, gc_stream* s, uint64_t first_index, uint32_t max_new_dwells, gc_acq_result* host_results,
    struct gc_acq_tong_status* host_status)
{
    GC_REQUIRE(a && s && host_results, "gc_acq_tong_search_stream: NULL argument");
    GC_REQUIRE(a->tong, "gc_acq_tong_search_stream: not a Tong engine (gc_acq_create_tong)");
    GC_REQUIRE(s->ctx->device == a->ctx->device, "gc_acq_tong_search_stream: the stream lives on another GPU");
    GC_REQUIRE(s->iq_format == a->iq_format, "gc_acq_tong_search_stream: stream format %d, acquisition format %d (gc_acq_set_input_format)",
        s->iq_format, a->iq_format);
    GC_REQUIRE(a->consumed <= s->mirror, "gc_acq_tong_search_stream: the block of %u samples is longer than the stream's max_window", a->consumed);
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = a->ctx->stream;
    const uint32_t done = a->tong_restart ? 0u : a->dwell_counter;
    const uint32_t left = done < a->tong_p.max_dwells ? a->tong_p.max_dwells - done : 0u;
    const uint32_t n = std::min(max_new_dwells, left);
    // all blocks are protected against eviction from here and checked before the first one is enqueued
    gc_stream_read_set reads(st);
    gc_status rs = reads.add(s, first_index);
    if (rs != GC_OK) return rs;
    const gc_stream_ticket& t = reads.ticket(0);
    const uint64_t span = (uint64_t)n * a->consumed;
    if (first_index + span > t.head)
        return gc_fail(GC_ERR_INVALID, "gc_acq_tong_search_stream: blocks [%llu, +%llu) are not inside the stream's resident samples [%llu, %llu)",
            (unsigned long long)first_index, (unsigned long long)span, (unsigned long long)t.oldest, (unsigned long long)t.head);
    // back to back on one stream: no host decision, no synchronisation between the dwells
    for (uint32_t k = 0; k < n; k++)
        {
            const uint64_t at = first_index + (uint64_t)k * a->consumed;
            rs = acq_enqueue(a, s->d_ring + (at % s->capacity) * s->elem, a->iq_format, st);
            if (rs != GC_OK) return rs;
        }
    rs = reads.commit();
    if (rs != GC_OK) return rs;
    rs = acq_fetch(a, host_results, st);
    if (rs == GC_OK && host_status) rs = acq_tong_fetch_status(a, host_status, st);
    return rs;
}

gc_status gc_tong_threshold(float pfa, uint32_t vector_length, uint32_t doppler_max, uint32_t doppler_step, float* out)
{
    GC_REQUIRE(out, "gc_tong_threshold: NULL argument");
    GC_REQUIRE(vector_length >= 1 && doppler_step >= 1, "gc_tong_threshold: bad sizes");
    // calculate_threshold of the adapters: the bins counted like init() counts them; the quantile of Exp(lambda) in closed form
    uint32_t bins = 0;
    for (int64_t d = -(int64_t)doppler_max; d <= (int64_t)doppler_max; d += (int64_t)doppler_step) bins++;
    const uint32_t ncells = vector_length * bins;
    const double exponent = 1.0 / (double)ncells;
    const double val = std::pow(1.0 - pfa, exponent);
    const double lambda = (double)vector_length;
    *out = (float)(-std::log(1.0 - val) / lambda);
    return GC_OK;
}

gc_status gc_acq_get_grid(gc_acq* a, int sat, float* host_grid)
{
    GC_REQUIRE(a && host_grid, "gc_acq_get_grid: NULL argument");
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_get_grid: satellite slot %d out of range", sat);
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    const size_t n = (size_t)a->n_bins * a->fft_size;
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
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    hipStream_t st = a->ctx->stream;
    const size_t N = a->fft_size;
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
            GC_REQUIRE(index >= 0 && index < a->replicas() * a->n_sats, "gc_acq_peek: code slot %d out of range", index);
            src = a->d_codes + (size_t)index * N;
        }
    else
        return gc_fail(GC_ERR_INVALID, "gc_acq_peek: unknown item %d", what);
    if (a->fold && what == GC_ACQ_PEEK_WIPEOFF)
        {
            // the QuickSync table: L samples per bin, in natural order already
            GC_HIP(hipMemcpy(host_out, a->d_wipe + (size_t)index * a->consumed, (size_t)a->consumed * sizeof(float2), hipMemcpyDeviceToHost));
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
    GC_REQUIRE(a->fold, "gc_acq_quicksync_candidates: not a QuickSync engine (gc_acq_create_quicksync)");
    GC_REQUIRE(sat >= 0 && sat < a->n_sats, "gc_acq_quicksync_candidates: satellite slot %d out of range", sat);
    gc_device_guard g(a->ctx->device);
    std::lock_guard<std::mutex> lk(a->ctx->mtx);
    GC_HIP(hipStreamSynchronize(a->ctx->stream));
    GC_HIP(hipMemcpy(possible_delay, a->d_cand_delay + (size_t)sat * a->fold, (size_t)a->fold * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GC_HIP(hipMemcpy(corr_output_f, a->d_cand_val + (size_t)sat * a->fold, (size_t)a->fold * sizeof(float), hipMemcpyDeviceToHost));
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
    // calculate_threshold of the adapters: the bins counted like init() counts them
    uint32_t bins = 0;
    for (int32_t d = -(int32_t)doppler_max; d <= (int32_t)doppler_max; d += (int32_t)doppler_step) bins++;
    const uint32_t ncells = (code_length / folding_factor) * bins;
    const double exponent = 1.0 / (double)ncells;
    const double val = std::pow(1.0 - (double)pfa, exponent);
    const double lambda = (double)code_length / (double)folding_factor;
    *out = (float)(-std::log(1.0 - val) / lambda);
    return GC_OK;
}

}  // extern "C"
