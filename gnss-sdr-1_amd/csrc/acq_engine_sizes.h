// acq_engine_sizes.h -- the kinds of acquisition engine (gc_acquisition.hip), what each accepts (ACQ_KIND_TRAITS) and the sizes each
// allocates from: a gc_acq_create* entry point fills an AcqEngineSpec, acq_engine_sizes() does the arithmetic, acq_create allocates.
// Host only, no HIP header: tests/acq_engine_sizes_selftest.cpp runs the rules on the CPU.
#ifndef ACQ_ENGINE_SIZES_H
#define ACQ_ENGINE_SIZES_H
#include "acq_tong_decide.h"
#include "gnsscorr.h"
#include <cmath>
#include <cstddef>
#include <cstdint>

enum AcqKind
{
    ACQ_PLAIN,      // gc_acq_create: pcps_acquisition.cc
    ACQ_PAIRED,     // gc_acq_create_paired: two replicas per slot, combined per grid cell
    ACQ_QUICKSYNC,  // gc_acq_create_quicksync: pcps_quicksync_acquisition_cc.cc
    ACQ_TONG,       // gc_acq_create_tong: pcps_tong_acquisition_cc.cc
    ACQ_CAF         // gc_acq_create_caf: galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc
};

struct AcqKindTraits
{
    const char* create;      // the kind's create function, for messages
    const char* code_entry;  // the one entry point that loads a slot's code(s)
    bool inclusive_grid;     // the Doppler grid includes +doppler_max: 2 * max / step + 1 bins against ceil(2 * max / step)
    bool step_two;           // gc_acq_set_step_two
    bool frequency_offset;   // gc_acq_set_frequency_offset
    bool holds_back;         // the transforms of a dwell may wait for the next one (AcqHeld)
};

static const AcqKindTraits ACQ_KIND_TRAITS[] = {
    /* ACQ_PLAIN     */ {"gc_acq_create", "gc_acq_set_local_code", false, true, true, true},
    /* ACQ_PAIRED    */ {"gc_acq_create_paired", "gc_acq_set_local_code_pair", false, true, true, false},
    /* ACQ_QUICKSYNC */ {"gc_acq_create_quicksync", "gc_acq_set_local_code", true, false, false, false},
    /* ACQ_TONG      */ {"gc_acq_create_tong", "gc_acq_set_local_code", true, false, false, false},
    /* ACQ_CAF       */ {"gc_acq_create_caf", "gc_acq_set_local_code_iq", true, false, false, false},
};

struct AcqCafParams
{
    int both = 0, hyp = 1, half = 0, arithmetic = 0, bit_transition = 0;
    int replicas() const { return (1 + both) * hyp; }
};

// what an entry point hands to acq_create; only the member of `kind` is read
struct AcqEngineSpec
{
    AcqKind kind = ACQ_PLAIN;
    int combine = 0;       // ACQ_PAIRED: GC_ACQ_COMBINE_MAX / _SUM
    int fold = 0;          // ACQ_QUICKSYNC: the folding factor f
    AcqTongParams tong{};  // ACQ_TONG
    AcqCafParams caf{};    // ACQ_CAF
};

struct AcqEngineSizes
{
    bool empty_grid = false;  // no Doppler bin or no sample: nothing below is meaningful
    uint32_t fft_size = 0;    // transform size
    uint32_t consumed = 0;    // input samples a dwell reads
    uint32_t eff = 0;         // delays searched of fft_size
    uint32_t input_len = 0;   // samples of the input staging buffers and of a wipe-off row
    uint32_t n_bins = 0;      // Doppler bins of the main grid
    uint32_t n_bins_alloc = 0;  // of the larger of main and step-two grid
    uint32_t max_dwells = 1;
    bool use_cfar = false;
    int replicas = 1;         // code replicas per satellite slot
    int sats_per_batch = 1;   // satellites whose inverse row pass shares the inter-pass buffer
    size_t q_cells = 0;       // rows of fft_size samples of that buffer
};

static inline AcqEngineSizes acq_engine_sizes(const gc_acq_conf& conf, const AcqEngineSpec& spec, int n_sats, size_t q_budget_bytes)
{
    AcqEngineSizes z;
    // pcps_acquisition.cc:77-85, :113-117
    const bool bt = conf.bit_transition_flag != 0;
    z.consumed = (uint32_t)(conf.sampled_ms * conf.samples_per_ms * (bt ? 2 : 1));
    z.fft_size = (conf.sampled_ms == conf.ms_per_code) ? z.consumed : z.consumed * 2;
    z.max_dwells = conf.max_dwells;
    if (bt)
        {
            z.fft_size = z.consumed * 2;
            z.max_dwells = 1;
        }
    z.eff = bt ? z.fft_size / 2 : z.fft_size;
    // :152-159 CFAR statistic only for a single dwell
    z.use_cfar = (z.max_dwells == 1) ? (conf.use_CFAR_algorithm_flag != 0) : false;
    if (spec.kind == ACQ_PAIRED) z.replicas = 2;
    if (spec.kind == ACQ_CAF) z.replicas = spec.caf.replicas();
    // pcps_tong_acquisition_cc.cc:107, galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc:100 (d_fft_size): no zero padding whatever the code length
    if (spec.kind == ACQ_TONG || spec.kind == ACQ_CAF) z.fft_size = z.eff = z.consumed;
    if (spec.kind == ACQ_QUICKSYNC)
        {
            // pcps_quicksync_acquisition_cc.cc:95 (d_fft_size = N / f), :362-364 (f code periods of N samples per dwell)
            z.fft_size = z.eff = (uint32_t)conf.samples_per_code / (uint32_t)spec.fold;
            z.consumed = (uint32_t)conf.samples_per_code * (uint32_t)spec.fold;
        }
    // the QuickSync wipe-off table and input hold the whole dwell, everybody else's one transform
    z.input_len = spec.kind == ACQ_QUICKSYNC ? z.consumed : z.fft_size;
    if (ACQ_KIND_TRAITS[spec.kind].inclusive_grid)
        // pcps_quicksync_acquisition_cc.cc:226-231, pcps_tong_acquisition_cc.cc:200-205, ..._caf_cc.cc:300-307: the grid includes +doppler_max
        z.n_bins = 2 * conf.doppler_max / conf.doppler_step + 1;
    else
        // pcps_acquisition.cc:326
        z.n_bins = (uint32_t)std::ceil((double)((int32_t)conf.doppler_max - (int32_t)(-(int32_t)conf.doppler_max)) / (double)conf.doppler_step);
    if (conf.num_doppler_bins_override > 0) z.n_bins = conf.num_doppler_bins_override;
    z.n_bins_alloc = z.n_bins;
    if (conf.make_2_steps && conf.num_doppler_bins_step2 > z.n_bins_alloc) z.n_bins_alloc = conf.num_doppler_bins_step2;
    if (z.n_bins == 0 || z.fft_size == 0)
        {
            z.empty_grid = true;
            return z;
        }
    // scratch Q: a batch of satellites stays within the budget (~140 MB: it lives in the 256 MB Infinity Cache between the two passes),
    // and the batches are equal: a launch's workgroups run in rounds of (CUs x workgroups per CU), so the time of a pass steps with the
    // round count -- 11 + 11 + 10 satellites x 41 bins cost 3 + 3 + 2 rounds of the row pass, 16 + 16 cost 4 + 4 with fewer, larger
    // launches (measured 0.53 -> 0.50 ms per search).  The row pass writes replicas * n_bins_alloc cells per satellite; one satellite
    // always fits, whatever the budget says
    const size_t per_sat = (size_t)z.replicas * z.n_bins_alloc * z.fft_size * 2 * sizeof(float);
    z.sats_per_batch = (int)(q_budget_bytes / per_sat);
    if (z.sats_per_batch < 1) z.sats_per_batch = 1;
    if (z.sats_per_batch > n_sats) z.sats_per_batch = n_sats;
    const int n_batches = (n_sats + z.sats_per_batch - 1) / z.sats_per_batch;
    z.sats_per_batch = (n_sats + n_batches - 1) / n_batches;
    z.q_cells = (size_t)z.sats_per_batch * z.replicas * z.n_bins_alloc;
    return z;
}

// Satellites per batch of the plain / paired / QuickSync inverse passes, whose row pass runs `spectra` cells per satellite through
// the q_cells rows: replicas * (active bins), or 2 * bins for a held-back dwell pair -- which halves the batch.  Equal batches again.
// (The Tong and CAF dwells step by AcqEngineSizes::sats_per_batch itself.)
static inline int acq_inverse_sats_per_batch(size_t q_cells, int spectra, int n_sats)
{
    int per_batch = (int)q_cells / spectra;
    const int n_batches = (n_sats + per_batch - 1) / per_batch;
    return (n_sats + n_batches - 1) / n_batches;
}

#endif
