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

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include "hip_multicorrelator_real_codes.h"  // gnsscorr::shared_context()
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
    uint32_t n = 0;
    for (auto doppler = -static_cast<int32_t>(doppler_max); doppler <= static_cast<int32_t>(doppler_max); doppler += static_cast<int32_t>(doppler_step)) n++;
    return n;
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

class hip_pcps_quicksync_acquisition
{
public:
    hip_pcps_quicksync_acquisition(uint32_t folding_factor, uint32_t sampled_ms, uint32_t max_dwells, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms,
        int32_t samples_per_code, bool bit_transition_flag, bool dump, const std::string& dump_filename)
        : d_fs_in(fs_in), d_samples_per_ms(samples_per_ms), d_samples_per_code(samples_per_code), d_sampled_ms(sampled_ms), d_max_dwells(max_dwells), d_doppler_max(doppler_max), d_folding_factor(folding_factor), d_bit_transition_flag(bit_transition_flag), d_dump(dump), d_dump_filename(dump_filename)
    {
        d_fft_size = folding_factor ? static_cast<uint32_t>(d_samples_per_code) / folding_factor : 0U;
        d_code.assign(static_cast<size_t>(d_samples_per_code), gr_complex(0.0f, 0.0f));
        d_possible_delay.assign(folding_factor, 0U);
        d_corr_output_f.assign(folding_factor, 0.0f);
    }

    ~hip_pcps_quicksync_acquisition()
    {
        if (d_acq != nullptr) gc_acq_destroy(d_acq);
    }

    hip_pcps_quicksync_acquisition(const hip_pcps_quicksync_acquisition&) = delete;
    hip_pcps_quicksync_acquisition& operator=(const hip_pcps_quicksync_acquisition&) = delete;

    inline void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    inline uint32_t mag() const { return d_mag; }
    inline void set_active(bool active) { d_active = active; }
    inline void set_channel(uint32_t channel) { d_channel = channel; }
    inline void set_threshold(float threshold) { d_threshold = threshold; }
    inline void set_doppler_max(uint32_t doppler_max) { d_doppler_max = doppler_max; }
    inline void set_doppler_step(uint32_t doppler_step) { d_doppler_step = doppler_step; }

    /*! set_local_code (:178-201): ONE code period of samples_per_code samples */
    void set_local_code(std::complex<float>* code)
    {
        std::memcpy(d_code.data(), code, sizeof(gr_complex) * d_code.size());
        d_have_code = true;
        if (d_acq != nullptr) d_status = gc_acq_set_local_code(d_acq, 0, reinterpret_cast<const float*>(d_code.data()));
    }

    /*! init (:204-245): clears the synchro fields, counts the bins, (re)creates the engine whose wipe-off table is the block's
     *  volk_gnsssdr_s32f_sincos_32fc grid of samples_per_code * folding_factor samples per bin */
    void init()
    {
        d_gnss_synchro->Flag_valid_acquisition = false;
        d_gnss_synchro->Flag_valid_symbol_output = false;
        d_gnss_synchro->Flag_valid_pseudorange = false;
        d_gnss_synchro->Flag_valid_word = false;
        d_gnss_synchro->Acq_delay_samples = 0.0;
        d_gnss_synchro->Acq_doppler_hz = 0.0;
        d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
        d_gnss_synchro->Acq_doppler_step = 0U;
        d_mag = 0.0;
        d_input_power = 0.0;
        d_num_doppler_bins = gnsscorr::quicksync_doppler_bins(d_doppler_max, d_doppler_step);
        if (d_acq != nullptr)
            {
                gc_acq_destroy(d_acq);
                d_acq = nullptr;
            }
        gc_acq_conf c;
        std::memset(&c, 0, sizeof c);
        c.fs_in = d_fs_in;
        c.sampled_ms = d_sampled_ms;
        c.ms_per_code = d_sampled_ms;
        c.samples_per_ms = static_cast<float>(d_samples_per_ms);
        c.samples_per_code = static_cast<float>(d_samples_per_code);
        c.samples_per_chip = static_cast<uint32_t>(std::ceil(static_cast<double>(d_fs_in) / 1.023e6));
        c.doppler_max = d_doppler_max;
        c.doppler_step = d_doppler_step;
        c.max_dwells = d_max_dwells;
        c.bit_transition_flag = d_bit_transition_flag ? 1 : 0;
        gc_ctx* ctx = gnsscorr::shared_context();
        d_status = ctx ? gc_acq_create_quicksync(ctx, &c, 1, d_folding_factor, &d_acq) : GC_ERR_NO_DEVICE;
        if (d_status == GC_OK && d_have_code) d_status = gc_acq_set_local_code(d_acq, 0, reinterpret_cast<const float*>(d_code.data()));
    }

    void set_state(int32_t state)
    {
        d_state = state;
        if (d_state == 1)
            {
                restart();
                d_active = true;  // :261
            }
    }

    /*! general_work (:272-603) on items of item_length() samples.  Returns the number of items consumed. */
    int work(const gr_complex* in, int ninput_items)
    {
        switch (d_state)
            {
            case 0:
                if (d_active)
                    {
                        restart();
                        d_state = 1;
                    }
                d_sample_counter += static_cast<uint64_t>(item_length()) * static_cast<uint64_t>(ninput_items);
                return ninput_items;
            case 1:
                dwell(in);
                return 1;
            case 2:
            case 3:
                d_active = false;
                d_events.push_back(d_state == 2 ? 1 : 2);
                d_state = 0;
                d_sample_counter += static_cast<uint64_t>(item_length()) * static_cast<uint64_t>(ninput_items);
                return ninput_items;
            }
        return 0;
    }

    //! messages published on the "events" port: 1 = ACQ_SUCCESS, 2 = ACQ_FAIL
    const std::vector<int>& events() const { return d_events; }
    void clear_events() { d_events.clear(); }
    float test_statistics() const { return d_test_statistics; }
    float input_power() const { return d_input_power; }
    const gc_acq_result& last_result() const { return d_last; }
    uint32_t fft_size() const { return d_fft_size; }
    uint32_t folding_factor() const { return d_folding_factor; }
    uint32_t item_length() const { return d_sampled_ms * static_cast<uint32_t>(d_samples_per_ms); }
    uint32_t num_doppler_bins() const { return d_num_doppler_bins; }
    uint32_t max_dwells() const { return d_max_dwells; }
    uint32_t dwell_count() const { return d_well_count; }
    int32_t state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    gc_status last_status() const { return d_status; }
    //! d_possible_delay / d_corr_output_f of the last dwell (logged by the block at :549-552)
    const std::vector<uint32_t>& possible_delay() const { return d_possible_delay; }
    const std::vector<float>& corr_output_f() const { return d_corr_output_f; }

private:
    // "restart acquisition variables" (set_state(1) :251-262 and state 0 :296-306)
    void restart()
    {
        d_gnss_synchro->Acq_delay_samples = 0.0;
        d_gnss_synchro->Acq_doppler_hz = 0.0;
        d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
        d_gnss_synchro->Acq_doppler_step = 0U;
        d_well_count = 0;
        d_mag = 0.0;
        d_input_power = 0.0;
        d_test_statistics = 0.0;
    }

    // state 1 (:315-536): one dwell on one item
    void dwell(const gr_complex* in)
    {
        const float fft_normalization_factor = static_cast<float>(d_fft_size) * static_cast<float>(d_fft_size);
        d_input_power = 0.0;
        d_mag = 0.0;
        d_test_statistics = 0.0;
        d_sample_counter += static_cast<uint64_t>(item_length());
        d_well_count++;
        gc_acq_result r;
        std::memset(&r, 0, sizeof r);
        d_status = d_acq ? gc_acq_dwell(d_acq, reinterpret_cast<const float*>(in), &r) : GC_ERR_STATE;
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
                        (void)gc_acq_quicksync_candidates(d_acq, 0, d_possible_delay.data(), d_corr_output_f.data());
                    }
            }
        d_state = gnsscorr::quicksync_decide(d_status == GC_OK ? d_test_statistics : 0.0f, d_threshold, d_well_count, d_max_dwells, d_bit_transition_flag);
    }

    int64_t d_fs_in;
    int32_t d_samples_per_ms, d_samples_per_code;
    uint32_t d_sampled_ms, d_max_dwells, d_doppler_max, d_folding_factor;
    bool d_bit_transition_flag, d_dump;
    std::string d_dump_filename;
    uint32_t d_fft_size = 0U, d_num_doppler_bins = 0U, d_doppler_step = 0U, d_channel = 0U, d_well_count = 0U;
    uint64_t d_sample_counter = 0ULL;
    int32_t d_state = 0;
    bool d_active = false, d_have_code = false;
    float d_threshold = 0.0f, d_mag = 0.0f, d_input_power = 0.0f, d_test_statistics = 0.0f;
    gc_acq* d_acq = nullptr;
    gc_status d_status = GC_OK;
    gc_acq_result d_last{};
    Gnss_Synchro* d_gnss_synchro = nullptr;
    std::vector<gr_complex> d_code;
    std::vector<uint32_t> d_possible_delay;
    std::vector<float> d_corr_output_f;
    std::vector<int> d_events;
};

/*! GpsL1CaPcpsQuickSyncAcquisition (gps_l1_ca_pcps_quicksync_acquisition.cc:40-292) and GalileoE1PcpsQuickSyncAmbiguousAcquisition
 *  (galileo_e1_pcps_quicksync_ambiguous_acquisition.cc:41-309) over hip_pcps_quicksync_acquisition.  Keys of both: doppler_max,
 *  coherent_integration_time_ms (default 4 / 8, rounded to a multiple of f / 4 f ms), folding_factor (default
 *  ceil(sqrt(log2(code_length))) / 2), bit_transition_flag (forces max_dwells = 2), max_dwells, <role><ch>.pfa and <role>.pfa (the
 *  threshold rule gc_quicksync_threshold), Acquisition<ch>.cboc (Galileo), dump, dump_filename.  code_length =
 *  round(fs / (1.023e6 / 1023)) with samples_per_ms = code_length (GPS), round(fs / (1.023e6 / 4092)) with samples_per_ms =
 *  round(code_length / 4) (Galileo); vector_length = sampled_ms * samples_per_ms, of which the block reads code_length * f. */
template <bool GALILEO>
class PcpsQuickSyncAcquisitionHip : public AcquisitionInterface
{
public:
    PcpsQuickSyncAcquisitionHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : configuration_(configuration), role_(role), in_streams_(in_streams), out_streams_(out_streams)
    {
        item_type_ = configuration_->property(role + ".item_type", std::string("gr_complex"));
        int64_t fs_in_deprecated = configuration_->property("GNSS-SDR.internal_fs_hz", static_cast<int64_t>(GALILEO ? 4000000 : 2048000));
        fs_in_ = configuration_->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
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

    std::string role() override { return role_; }
    std::string implementation() override { return GALILEO ? "Galileo_E1_PCPS_QuickSync_Ambiguous_Acquisition_HIP" : "GPS_L1_CA_PCPS_QuickSync_Acquisition_HIP"; }
    size_t item_size() override { return sizeof(gr_complex); }

    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) override
    {
        gnss_synchro_ = p_gnss_synchro;
        acquisition_->set_gnss_synchro(gnss_synchro_);
    }

    void set_channel(unsigned int channel) override
    {
        channel_ = channel;
        acquisition_->set_channel(channel_);
    }

    void set_channel_fsm(std::shared_ptr<ChannelFsm> channel_fsm) override { channel_fsm_ = channel_fsm; }

    void set_threshold(float threshold) override
    {
        float pfa = configuration_->property(role_ + std::to_string(channel_) + ".pfa", 0.0f);
        if (pfa == 0.0f) pfa = configuration_->property(role_ + ".pfa", 0.0f);
        threshold_ = threshold;
        if (pfa != 0.0f) gc_quicksync_threshold(pfa, code_length_, folding_factor_, doppler_max_, doppler_step_ ? doppler_step_ : 250, &threshold_);
        acquisition_->set_threshold(threshold_);
    }

    void set_doppler_max(unsigned int doppler_max) override
    {
        doppler_max_ = doppler_max;
        acquisition_->set_doppler_max(doppler_max_);
    }

    void set_doppler_step(unsigned int doppler_step) override
    {
        doppler_step_ = doppler_step;
        acquisition_->set_doppler_step(doppler_step_);
    }

    void init() override { acquisition_->init(); }

    void set_local_code() override
    {
        std::vector<gr_complex> code(code_length_ + 8);
        if (GALILEO)
            {
                const bool cboc = configuration_->property("Acquisition" + std::to_string(channel_) + ".cboc", false);
                const char* sig = (gnss_synchro_->Signal[0] == '1' && gnss_synchro_->Signal[1] == 'C') ? "1C" : "1B";
                gc_galileo_e1_code_gen_complex_sampled(reinterpret_cast<float*>(code.data()), sig, cboc ? 1 : 0, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
            }
        else
            gc_gps_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(code.data()), gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
        acquisition_->set_local_code(code.data());  // one period (see the file comment)
    }

    void set_state(int state) override { acquisition_->set_state(state); }
    signed int mag() override { return acquisition_->mag(); }
    void reset() override { acquisition_->set_active(true); }
    void stop_acquisition() override {}
    void set_resampler_latency(uint32_t) override {}

    //! the block (get_left_block() is a stream_to_vector in front of it in the reference)
    std::shared_ptr<hip_pcps_quicksync_acquisition> block() { return acquisition_; }
    unsigned int vector_length() const { return vector_length_; }
    unsigned int code_length() const { return code_length_; }
    unsigned int folding_factor() const { return folding_factor_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int max_dwells() const { return max_dwells_; }
    float threshold() const { return threshold_; }

private:
    ConfigurationInterface* configuration_;
    std::shared_ptr<hip_pcps_quicksync_acquisition> acquisition_;
    std::string item_type_;
    std::string role_;
    std::string dump_filename_;
    unsigned int in_streams_;
    unsigned int out_streams_;
    unsigned int vector_length_ = 0;
    unsigned int code_length_ = 0;
    unsigned int channel_ = 0;
    unsigned int doppler_max_ = 0;
    unsigned int doppler_step_ = 0;
    unsigned int sampled_ms_ = 4;
    unsigned int max_dwells_ = 1;
    uint32_t folding_factor_ = 2;
    bool bit_transition_flag_ = false;
    bool dump_ = false;
    float threshold_ = 0.0f;
    int64_t fs_in_ = 0;
    std::shared_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_ = nullptr;
};

using GpsL1CaPcpsQuickSyncAcquisitionHip = PcpsQuickSyncAcquisitionHip<false>;
using GalileoE1PcpsQuickSyncAmbiguousAcquisitionHip = PcpsQuickSyncAcquisitionHip<true>;

#endif  // GNSSCORR_HIP_PCPS_QUICKSYNC_ACQUISITION_H_
