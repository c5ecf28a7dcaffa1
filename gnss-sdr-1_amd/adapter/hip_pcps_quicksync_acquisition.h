/*!
 * \file hip_pcps_quicksync_acquisition.h
 * \brief Image of pcps_quicksync_acquisition_cc (src/algorithms/acquisition/gnuradio_blocks/pcps_quicksync_acquisition_cc.{h,cc})
 * over a QuickSync engine of libgnsscorr.so (gc_acq_create_quicksync), and the two AcquisitionInterface adapters in front of it:
 *   GpsL1CaPcpsQuickSyncAcquisitionHip             gps_l1_ca_pcps_quicksync_acquisition.cc
 *   GalileoE1PcpsQuickSyncAmbiguousAcquisitionHip  galileo_e1_pcps_quicksync_ambiguous_acquisition.cc
 *
 * Contracts kept:
 *   - d_fft_size = samples_per_code / folding_factor (:95); a dwell reads samples_per_code * folding_factor samples of an item of
 *     sampled_ms * samples_per_ms samples; the Doppler bins run from -doppler_max to +doppler_max INCLUSIVE, a step of 0 means 250
 *     (:219-231);
 *   - every dwell stands alone: d_mag, d_input_power and d_test_statistics restart at the top of state 1 (:340-343), so the
 *     `d_test_statistics < d_mag / d_input_power || !d_bit_transition_flag` condition (:438) always holds and the synchro fields are
 *     those of the dwell's winner; statistic = max |.|^2 / M^4 / input_power (:422, :480);
 *   - decision (:503-527): without bit_transition_flag positive as soon as the statistic exceeds the threshold, negative when the
 *     dwell count reaches max_dwells; with it, the decision is taken at dwell max_dwells only.  The "events" port carries 1
 *     (ACQ_SUCCESS) or 2 (ACQ_FAIL) from states 2 and 3;
 *   - the sample counter advances by sampled_ms * samples_per_ms per item in every state (:309, :345, :561, :593);
 *   - general_work(noutput, ninput_items, input_items, ..) becomes work(in, ninput_items[0]) on items of item_length() samples,
 *     consume_each(n) the return value.
 * Documented departures:
 *   - the block never initialises `complex_acumulator[100]` (:442) and adds the candidate correlations onto whatever the stack
 *     holds; here they start at zero;
 *   - the reference's adapters copy sampled_ms / folding_factor (GPS) or sampled_ms / (4 folding_factor) (Galileo) code periods into
 *     a buffer of ONE period (code_, gps :70, :243-247; galileo :259-263) -- a heap overrun whenever that count exceeds one -- and
 *     the block reads one period of it (:182).  The adapters here pass one period;
 *   - `dump` is accepted and ignored (the block writes the folded |.|^2 row per bin; gc_acq_get_grid gives the same rows).
 * The pure host-side pieces -- bin count, key rounding, the decision machine -- are free of the library and are checked without a
 * GPU by `quicksync_selftest --host`.
 */
#ifndef GNSSCORR_HIP_PCPS_QUICKSYNC_ACQUISITION_H_
#define GNSSCORR_HIP_PCPS_QUICKSYNC_ACQUISITION_H_

#include "acquisition_adapter_base.h"
#include "acquisition_block_base.h"
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gnsscorr
{
//! init() (:219-231): a step of 0 becomes 250; both ends of the range count
inline uint32_t quicksync_doppler_bins(uint32_t doppler_max, uint32_t& doppler_step)
{
    if (doppler_step == 0) doppler_step = 250;
    return inclusive_doppler_bins(doppler_max, doppler_step);
}

//! coherent_integration_time_ms rounded to a multiple of `multiple` ms as the adapters round it (gps :71-87 with multiple = f,
//! galileo :79-96 with multiple = 4 f): shorter values become one multiple, others are rounded down
inline unsigned int quicksync_coherent_ms(unsigned int sampled_ms, unsigned int multiple)
{
    if (sampled_ms % multiple == 0) return sampled_ms;
    return sampled_ms < multiple ? multiple : (sampled_ms / multiple) * multiple;
}

//! the decision of state 1 (:503-527) on the statistic of the dwell that has just run; returns the next state (1, 2 or 3)
inline int32_t quicksync_decide(float test_statistics, float threshold, uint32_t well_count, uint32_t max_dwells, bool bit_transition_flag)
{
    if (!bit_transition_flag)
        {
            if (test_statistics > threshold) return 2;  // Positive acquisition
            if (well_count == max_dwells) return 3;     // Negative acquisition
            return 1;
        }
    if (well_count == max_dwells) return test_statistics > threshold ? 2 : 3;  // d_max_dwells = 2
    return 1;
}
}  // namespace gnsscorr

class hip_pcps_quicksync_acquisition : public hip_acquisition_item_block
{
public:
    // general_work (:272-603): search state 1 (:315-536), positive 2, negative 3; set_state(1) restarts AND sets d_active (:261).  An item is
    // sampled_ms * samples_per_ms samples, not d_fft_size
    hip_pcps_quicksync_acquisition(uint32_t folding_factor, uint32_t sampled_ms, uint32_t max_dwells, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms,
        int32_t samples_per_code, bool bit_transition_flag, bool dump, const std::string& dump_filename)
        : hip_acquisition_item_block(Policy{1, 1, 2, 3, true}, sampled_ms, max_dwells, doppler_max, fs_in, samples_per_ms, samples_per_code, dump, dump_filename,
              folding_factor ? static_cast<uint32_t>(samples_per_code) / folding_factor : 0U, sampled_ms * static_cast<uint32_t>(samples_per_ms)),
          d_folding_factor(folding_factor), d_bit_transition_flag(bit_transition_flag)
    {
        d_code.assign(static_cast<size_t>(d_samples_per_code), gr_complex(0.0f, 0.0f));
        d_possible_delay.assign(folding_factor, 0U);
        d_corr_output_f.assign(folding_factor, 0.0f);
    }

    /*! set_local_code (:178-201): ONE code period of samples_per_code samples */
    void set_local_code(std::complex<float>* code)
    {
        std::memcpy(d_code.data(), code, sizeof(gr_complex) * d_code.size());
        d_have_code = true;
        if (d_acq != nullptr) d_status = load_code();
    }

    uint32_t folding_factor() const { return d_folding_factor; }
    uint32_t max_dwells() const { return d_max_dwells; }
    //! d_possible_delay / d_corr_output_f of the last dwell (logged by the block at :549-552)
    const std::vector<uint32_t>& possible_delay() const { return d_possible_delay; }
    const std::vector<float>& corr_output_f() const { return d_corr_output_f; }

private:
    // init (:204-245): counts the bins, creates the engine whose wipe-off table is the block's volk_gnsssdr_s32f_sincos_32fc grid of
    // samples_per_code * folding_factor samples per bin.  A restart leaves the engine alone: every dwell stands alone
    gc_status create_engine() override
    {
        d_num_doppler_bins = gnsscorr::quicksync_doppler_bins(d_doppler_max, d_doppler_step);
        gc_acq_conf c = conf(1.023e6, d_max_dwells);
        c.bit_transition_flag = d_bit_transition_flag ? 1 : 0;
        return make_engine([&](gc_ctx* ctx, gc_acq** acq) { return gc_acq_create_quicksync(ctx, &c, 1, d_folding_factor, acq); });
    }

    gc_status load_code() override { return gc_acq_set_local_code(d_acq.get(), 0, reinterpret_cast<const float*>(d_code.data())); }

    // state 1 (:315-536): one dwell on one item, whatever n_items says; the counter and the dwell count advance BEFORE the dwell.  An
    // engine error leaves the decision rule with a statistic of 0
    int search(const gr_complex* in, gc_stream*, uint64_t, int) override
    {
        const float fft_normalization_factor = static_cast<float>(d_fft_size) * static_cast<float>(d_fft_size);
        d_input_power = 0.0;
        d_mag = 0.0;
        d_test_statistics = 0.0;
        count_items(1);
        d_dwell_count++;
        gc_acq_result r;
        std::memset(&r, 0, sizeof r);
        d_status = d_acq ? gc_acq_dwell(d_acq.get(), reinterpret_cast<const float*>(in), &r) : GC_ERR_STATE;
        d_last = r;
        if (d_status == GC_OK)
            {
                d_input_power = r.input_power;
                const float magt = r.mag / (fft_normalization_factor * fft_normalization_factor);
                if (d_mag < magt)
                    {
                        d_mag = magt;
                        d_gnss_synchro->Acq_delay_samples = r.acq_delay_samples;
                        d_gnss_synchro->Acq_doppler_hz = r.acq_doppler_hz;
                        d_gnss_synchro->Acq_samplestamp_samples = d_sample_counter;
                        d_gnss_synchro->Acq_doppler_step = d_doppler_step;
                        d_test_statistics = d_mag / d_input_power;
                        // the candidates are fetched only when the dwell's winner is taken
                        (void)gc_acq_quicksync_candidates(d_acq.get(), 0, d_possible_delay.data(), d_corr_output_f.data());
                    }
            }
        d_state = gnsscorr::quicksync_decide(d_status == GC_OK ? d_test_statistics : 0.0f, d_threshold, d_dwell_count, d_max_dwells, d_bit_transition_flag);
        return 1;
    }

    uint32_t d_folding_factor;
    bool d_bit_transition_flag;
    std::vector<gr_complex> d_code;
    std::vector<uint32_t> d_possible_delay;
    std::vector<float> d_corr_output_f;
};

/*! GpsL1CaPcpsQuickSyncAcquisition (gps_l1_ca_pcps_quicksync_acquisition.cc:40-292) and GalileoE1PcpsQuickSyncAmbiguousAcquisition
 *  (galileo_e1_pcps_quicksync_ambiguous_acquisition.cc:41-309) over hip_pcps_quicksync_acquisition.  Keys of both: doppler_max,
 *  coherent_integration_time_ms (default 4 / 8, rounded to a multiple of f / 4 f ms), folding_factor (default
 *  ceil(sqrt(log2(code_length))) / 2), bit_transition_flag (forces max_dwells = 2), max_dwells, <role><ch>.pfa and <role>.pfa (the
 *  threshold rule gc_quicksync_threshold), Acquisition<ch>.cboc (Galileo), dump, dump_filename.  code_length =
 *  round(fs / (1.023e6 / 1023)) with samples_per_ms = code_length (GPS), round(fs / (1.023e6 / 4092)) with samples_per_ms =
 *  round(code_length / 4) (Galileo); vector_length = sampled_ms * samples_per_ms, of which the block reads code_length * f. */
template <bool GALILEO>
class PcpsQuickSyncAcquisitionHip : public AcquisitionAdapterBase<hip_pcps_quicksync_acquisition>
{
public:
    PcpsQuickSyncAcquisitionHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : AcquisitionAdapterBase<hip_pcps_quicksync_acquisition>(configuration, role, in_streams, out_streams, GALILEO ? 4000000 : 2048000)
    {
        dump_ = configuration_->property(role + ".dump", false);
        doppler_max_ = configuration_->property(role + ".doppler_max", 5000);
        sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", GALILEO ? 8 : 4);
        code_length_ = static_cast<unsigned int>(std::round(static_cast<double>(fs_in_) / (1.023e6 / (GALILEO ? 4092.0 : 1023.0))));
        const int samples_per_ms = GALILEO ? static_cast<int>(std::round(code_length_ / 4.0)) : static_cast<int>(code_length_);
        uint32_t default_f = 2;
        if (!GALILEO) gc_quicksync_default_folding_factor(code_length_, &default_f);
        folding_factor_ = configuration_->property(role + ".folding_factor", default_f);
        if (folding_factor_ == 0) folding_factor_ = default_f;
        sampled_ms_ = gnsscorr::quicksync_coherent_ms(sampled_ms_, GALILEO ? folding_factor_ * 4 : folding_factor_);
        vector_length_ = sampled_ms_ * samples_per_ms;
        bit_transition_flag_ = configuration_->property(role + ".bit_transition_flag", false);
        max_dwells_ = bit_transition_flag_ ? 2U : static_cast<unsigned int>(configuration_->property(role + ".max_dwells", 1));
        dump_filename_ = configuration_->property(role + ".dump_filename", std::string(GALILEO ? "../data/acquisition.dat" : "./data/acquisition.dat"));
        acquisition_ = std::make_shared<hip_pcps_quicksync_acquisition>(folding_factor_, sampled_ms_, max_dwells_, doppler_max_, fs_in_, samples_per_ms,
            static_cast<int32_t>(code_length_), bit_transition_flag_, dump_, dump_filename_);
    }

    std::string implementation() override { return GALILEO ? "Galileo_E1_PCPS_QuickSync_Ambiguous_Acquisition_HIP" : "GPS_L1_CA_PCPS_QuickSync_Acquisition_HIP"; }

    void set_threshold(float threshold) override
    {
        const float pfa = pfa_for_channel();
        threshold_ = threshold;
        if (pfa != 0.0f) gc_quicksync_threshold(pfa, code_length_, folding_factor_, doppler_max_, doppler_step_ ? doppler_step_ : 250, &threshold_);
        acquisition_->set_threshold(threshold_);
    }

    void set_local_code() override
    {
        std::vector<gr_complex> code(code_length_ + 8);
        if (GALILEO)
            gnsscorr::e1_code_sampled(configuration_, channel_, gnss_synchro_, fs_in_, code.data());
        else
            gc_gps_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(code.data()), gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
        acquisition_->set_local_code(code.data());  // one period (see the file comment)
    }

    unsigned int code_length() const { return code_length_; }
    unsigned int folding_factor() const { return folding_factor_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int max_dwells() const { return max_dwells_; }

private:
    std::string dump_filename_;
    unsigned int sampled_ms_ = 4;
    unsigned int max_dwells_ = 1;
    uint32_t folding_factor_ = 2;
    bool bit_transition_flag_ = false;
    bool dump_ = false;
};

using GpsL1CaPcpsQuickSyncAcquisitionHip = PcpsQuickSyncAcquisitionHip<false>;
using GalileoE1PcpsQuickSyncAmbiguousAcquisitionHip = PcpsQuickSyncAcquisitionHip<true>;

#endif  // GNSSCORR_HIP_PCPS_QUICKSYNC_ACQUISITION_H_
