/*!
 * \file hip_e5a_noncoherent_iq_acquisition_caf.h
 * \brief Image of galileo_e5a_noncoherentIQ_acquisition_caf_cc
 * (src/algorithms/acquisition/gnuradio_blocks/galileo_e5a_noncoherent_iq_acquisition_caf_cc.{h,cc}) over a CAF engine of
 * libgnsscorr.so (gc_acq_create_caf), and the AcquisitionInterface adapter in front of it:
 *   GalileoE5aNoncoherentIQAcquisitionCafHip   galileo_e5a_noncoherent_iq_acquisition_caf.cc
 *
 * Contracts kept:
 *   - d_fft_size = sampled_ms * samples_per_ms (:100); with Zero_padding > 0 the adapter has forced sampled_ms to 2 and the block
 *     searches ONE hypothesis (d_sampled_ms = 1, :92-95) with the replica [code, zeros]; otherwise 2 or 3 ms search the (1,1,1) and
 *     the first-period-negated replica of each component (:258-280), all of it on the device;
 *   - the Doppler bins run from -doppler_max to +doppler_max INCLUSIVE (:300-307);
 *   - states 1 and 2 (:405-804) fill one block of d_fft_size samples and search it: here one item of item_length() samples is one
 *     dwell.  d_well_count counts them; after max_dwells dwells the search is positive when the kept statistic exceeds the
 *     threshold (:785-795).  With bit_transition_flag the kept statistic and the cell of Gnss_Synchro only move when a dwell beats
 *     them (:645-653); with CAF_window_hz > 0 the Doppler is the CAF argmax of EVERY dwell (:768-770);
 *   - the sample counter advances by d_fft_size per item in every state and the stamp of a kept dwell is the counter AFTER its
 *     block (:424, :436, :649);
 *   - states 3 and 4 publish 1 (ACQ_SUCCESS) / 2 (ACQ_FAIL) on "events", clear d_active and return to state 0;
 *   - general_work becomes work(in, n_items) on host items, or work_ring(ring, first_index, n_items) on items in a gc_stream ring.
 * Documented departures:
 *   - `dump` is accepted and NOT implemented: the block writes raw grids into the hard-coded relative directory ../data (:662,
 *     :777); gc_acq_get_grid and gc_acq_caf_vectors read the same grids and vectors through the ABI;
 *   - `arithmetic` (an extension key of the adapter, "reference" by default) chooses between the block as written and the block as
 *     meant: see GC_CAF_REFERENCE / GC_CAF_EXACT in gnsscorr.h for the two places they differ (the magt_QB read at :523 and the
 *     wrapped CAF weights at :701, :725, :735);
 *   - a configuration the block would crash on (CAF_window_hz below 2 * doppler_step: a division by zero; a window wider than the
 *     grid: reads out of range; doppler_step 0: an endless loop) fails the search instead: last_status() is GC_ERR_INVALID.
 * The pure host-side pieces -- keys and defaults, replica layouts, the threshold rule -- are checked without a GPU by
 * `caf_selftest --host`.
 */
#ifndef GNSSCORR_HIP_E5A_NONCOHERENT_IQ_ACQUISITION_CAF_H_
#define GNSSCORR_HIP_E5A_NONCOHERENT_IQ_ACQUISITION_CAF_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include "hip_multicorrelator_real_codes.h"  // gnsscorr::shared_context()
#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

class hip_e5a_noncoherent_iq_acquisition_caf
{
public:
    hip_e5a_noncoherent_iq_acquisition_caf(uint32_t sampled_ms, uint32_t max_dwells, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms, int32_t samples_per_code,
        bool bit_transition_flag, bool dump, const std::string& dump_filename, bool both_signal_components, int32_t CAF_window_hz, int32_t Zero_padding,
        int32_t arithmetic = GC_CAF_REFERENCE)
        : d_fs_in(fs_in), d_samples_per_ms(samples_per_ms), d_samples_per_code(samples_per_code), d_max_dwells(max_dwells), d_doppler_max(doppler_max), d_bit_transition_flag(bit_transition_flag), d_dump(dump), d_dump_filename(dump_filename), d_both_signal_components(both_signal_components), d_CAF_window_hz(CAF_window_hz), d_arithmetic(arithmetic)
    {
        d_sampled_ms = Zero_padding > 0 ? 1U : sampled_ms;  // :92-99: the number of code periods the hypotheses are made for
        d_fft_size = sampled_ms * static_cast<uint32_t>(d_samples_per_ms);
        d_code_i.assign(d_fft_size, gr_complex(0.0f, 0.0f));
        d_code_q.assign(d_fft_size, gr_complex(0.0f, 0.0f));
    }

    ~hip_e5a_noncoherent_iq_acquisition_caf()
    {
        if (d_acq != nullptr) gc_acq_destroy(d_acq);
    }

    hip_e5a_noncoherent_iq_acquisition_caf(const hip_e5a_noncoherent_iq_acquisition_caf&) = delete;
    hip_e5a_noncoherent_iq_acquisition_caf& operator=(const hip_e5a_noncoherent_iq_acquisition_caf&) = delete;

    inline void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    inline uint32_t mag() const { return d_mag; }
    inline void set_active(bool active) { d_active = active; }
    inline void set_channel(uint32_t channel) { d_channel = channel; }
    inline void set_threshold(float threshold) { d_threshold = threshold; }
    inline void set_doppler_max(uint32_t doppler_max) { d_doppler_max = doppler_max; }
    inline void set_doppler_step(uint32_t doppler_step) { d_doppler_step = doppler_step; }

    /*! set_local_code (:234-282): d_fft_size samples of each component; codeQ is read with both components only */
    void set_local_code(std::complex<float>* codeI, std::complex<float>* codeQ)
    {
        std::memcpy(d_code_i.data(), codeI, sizeof(gr_complex) * d_fft_size);
        if (d_both_signal_components) std::memcpy(d_code_q.data(), codeQ, sizeof(gr_complex) * d_fft_size);
        d_have_code = true;
        if (d_acq != nullptr) load_code();
    }

    /*! init (:285-333): clears the synchro fields, counts the bins, (re)creates the engine (wipe-off grid, CAF vectors) */
    void init()
    {
        d_gnss_synchro->Flag_valid_acquisition = false;
        d_gnss_synchro->Flag_valid_symbol_output = false;
        d_gnss_synchro->Flag_valid_pseudorange = false;
        d_gnss_synchro->Flag_valid_word = false;
        d_gnss_synchro->Acq_delay_samples = 0.0;
        d_gnss_synchro->Acq_doppler_hz = 0.0;
        d_gnss_synchro->Acq_doppler_step = 0U;
        d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
        d_mag = 0.0;
        d_input_power = 0.0;
        d_num_doppler_bins = 0;
        if (d_doppler_step > 0)
            for (int64_t doppler = -static_cast<int64_t>(d_doppler_max); doppler <= static_cast<int64_t>(d_doppler_max); doppler += d_doppler_step) d_num_doppler_bins++;
        if (d_acq != nullptr)
            {
                gc_acq_destroy(d_acq);
                d_acq = nullptr;
            }
        gc_acq_conf c;
        std::memset(&c, 0, sizeof c);
        c.fs_in = d_fs_in;
        c.sampled_ms = d_fft_size / static_cast<uint32_t>(d_samples_per_ms);
        c.ms_per_code = c.sampled_ms;
        c.samples_per_ms = static_cast<float>(d_samples_per_ms);
        c.samples_per_code = static_cast<float>(d_samples_per_code);
        c.samples_per_chip = static_cast<uint32_t>(std::ceil(static_cast<double>(d_fs_in) / 1.023e7));
        c.doppler_max = d_doppler_max;
        c.doppler_step = d_doppler_step;
        c.max_dwells = d_max_dwells;
        c.bit_transition_flag = d_bit_transition_flag ? 1 : 0;
        gc_ctx* ctx = gnsscorr::shared_context();
        d_status = ctx ? gc_acq_create_caf(ctx, &c, 1, d_both_signal_components ? 1 : 0, d_sampled_ms > 1 ? 2 : 1, d_CAF_window_hz > 0 ? static_cast<uint32_t>(d_CAF_window_hz) : 0U,
                             d_arithmetic, &d_acq)
                       : GC_ERR_NO_DEVICE;
        if (d_status == GC_OK && d_have_code) load_code();
    }

    void set_state(int32_t state)
    {
        d_state = state;
        if (d_state == 1) restart();
    }

    /*! general_work (:360-860) on host items of item_length() samples.  Returns the number of items consumed. */
    int work(const gr_complex* in, int ninput_items) { return step(in, nullptr, 0, ninput_items); }

    /*! the same on items that lie in `ring` from absolute sample first_index on (a GC_IQ_F32 ring) */
    int work_ring(gc_stream* ring, uint64_t first_index, int n_items) { return step(nullptr, ring, first_index, n_items); }

    //! messages published on the "events" port: 1 = ACQ_SUCCESS, 2 = ACQ_FAIL
    const std::vector<int>& events() const { return d_events; }
    void clear_events() { d_events.clear(); }
    float test_statistics() const { return d_test_statistics; }
    float input_power() const { return d_input_power; }
    float threshold() const { return d_threshold; }
    const gc_acq_result& last_result() const { return d_last; }
    uint32_t fft_size() const { return d_fft_size; }
    uint32_t item_length() const { return d_fft_size; }
    uint32_t num_doppler_bins() const { return d_num_doppler_bins; }
    uint32_t hypotheses() const { return d_sampled_ms > 1 ? 2U : 1U; }
    bool both_signal_components() const { return d_both_signal_components; }
    uint32_t well_count() const { return d_well_count; }
    int32_t state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    gc_status last_status() const { return d_status; }
    gc_acq* engine() { return d_acq; }
    const std::vector<gr_complex>& code_i() const { return d_code_i; }
    const std::vector<gr_complex>& code_q() const { return d_code_q; }

private:
    void load_code()
    {
        d_status = gc_acq_set_local_code_iq(d_acq, 0, reinterpret_cast<const float*>(d_code_i.data()),
            d_both_signal_components ? reinterpret_cast<const float*>(d_code_q.data()) : nullptr);
    }

    // "restart acquisition variables" (set_state(1) :339-349 and state 0 :389-398): gc_acq_reset zeroes the kept statistic
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
        if (d_acq != nullptr) d_status = gc_acq_reset(d_acq);
    }

    int step(const gr_complex* in, gc_stream* ring, uint64_t first_index, int n_items)
    {
        switch (d_state)
            {
            case 0:
                if (d_active)
                    {
                        restart();
                        d_state = 1;
                    }
                d_sample_counter += static_cast<uint64_t>(d_fft_size) * static_cast<uint64_t>(n_items);
                return n_items;
            case 1:
            case 2:
                return n_items > 0 ? dwell(in, ring, first_index) : 0;
            case 3:
            case 4:
                d_active = false;
                d_events.push_back(d_state == 3 ? 1 : 2);
                d_state = 0;
                d_sample_counter += static_cast<uint64_t>(d_fft_size) * static_cast<uint64_t>(n_items);
                return n_items;
            }
        return 0;
    }

    // states 1 + 2 (:405-804): one block, one dwell.  Returns the items consumed (1)
    int dwell(const gr_complex* in, gc_stream* ring, uint64_t first_index)
    {
        gc_acq_result r;
        std::memset(&r, 0, sizeof r);
        d_sample_counter += static_cast<uint64_t>(d_fft_size);
        d_well_count++;
        if (d_acq == nullptr)
            {
                if (d_status == GC_OK) d_status = GC_ERR_STATE;
            }
        else if (ring != nullptr)
            d_status = gc_acq_dwell_stream(d_acq, ring, first_index, &r);
        else
            d_status = gc_acq_dwell(d_acq, reinterpret_cast<const float*>(in), &r);
        if (d_status != GC_OK)
            {
                // nothing ran: the item is consumed and the search fails, so that a broken engine cannot hold a channel for ever
                d_state = 4;
                return 1;
            }
        d_last = r;
        d_mag = r.mag;
        d_input_power = r.input_power;
        // the keep rule ran on the device (:645-653): the kept statistic moved if and only if this dwell's cell was taken
        const bool taken = r.mag > 0.0f && (!d_bit_transition_flag || d_test_statistics < r.test_statistics);
        d_test_statistics = r.test_statistics;
        d_gnss_synchro->Acq_delay_samples = r.acq_delay_samples;
        d_gnss_synchro->Acq_doppler_hz = r.acq_doppler_hz;  // the CAF argmax of this dwell when the filter is on (:768-770)
        if (taken)
            {
                d_gnss_synchro->Acq_samplestamp_samples = d_sample_counter;
                d_gnss_synchro->Acq_doppler_step = d_doppler_step;
            }
        if (d_well_count == d_max_dwells)
            d_state = d_test_statistics > d_threshold ? 3 : 4;  // :785-795
        else
            d_state = 1;
        return 1;
    }

    int64_t d_fs_in;
    int32_t d_samples_per_ms, d_samples_per_code;
    uint32_t d_max_dwells, d_doppler_max;
    bool d_bit_transition_flag, d_dump;
    std::string d_dump_filename;
    bool d_both_signal_components;
    int32_t d_CAF_window_hz, d_arithmetic;
    uint32_t d_sampled_ms = 1U, d_fft_size = 0U, d_num_doppler_bins = 0U, d_doppler_step = 250U, d_channel = 0U, d_well_count = 0U;
    uint64_t d_sample_counter = 0ULL;
    int32_t d_state = 0;
    bool d_active = false, d_have_code = false;
    float d_threshold = 0.0f, d_mag = 0.0f, d_input_power = 0.0f, d_test_statistics = 0.0f;
    gc_acq* d_acq = nullptr;
    gc_status d_status = GC_OK;
    gc_acq_result d_last{};
    Gnss_Synchro* d_gnss_synchro = nullptr;
    std::vector<gr_complex> d_code_i, d_code_q;
    std::vector<int> d_events;
};

/*! GalileoE5aNoncoherentIQAcquisitionCaf (galileo_e5a_noncoherent_iq_acquisition_caf.cc:47-305) over
 *  hip_e5a_noncoherent_iq_acquisition_caf.  Keys and defaults: doppler_max (5000), CAF_window_hz (0), Zero_padding (0),
 *  coherent_integration_time_ms (1; capped at 3; forced to 2 with Zero_padding), max_dwells (1), bit_transition_flag (false),
 *  <role><ch>.pfa and <role>.pfa (the threshold rule: gc_tong_threshold on vector_length), dump, dump_filename, Channel.signal ("5X":
 *  both components), and the extension key arithmetic ("reference" | "exact").  code_length = round(fs / 1.023e7 * 10230),
 *  vector_length = code_length * sampled_ms. */
class GalileoE5aNoncoherentIQAcquisitionCafHip : public AcquisitionInterface
{
public:
    GalileoE5aNoncoherentIQAcquisitionCafHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : configuration_(configuration), role_(role), in_streams_(in_streams), out_streams_(out_streams)
    {
        item_type_ = configuration_->property(role + ".item_type", std::string("gr_complex"));
        int64_t fs_in_deprecated = configuration_->property("GNSS-SDR.internal_fs_hz", static_cast<int64_t>(32000000));
        fs_in_ = configuration_->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
        dump_ = configuration_->property(role + ".dump", false);
        doppler_max_ = configuration_->property(role + ".doppler_max", 5000);
        CAF_window_hz_ = configuration_->property(role + ".CAF_window_hz", 0);
        Zero_padding = configuration_->property(role + ".Zero_padding", 0);
        sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", 1);
        if (sampled_ms_ > 3) sampled_ms_ = 3;      // :74-79
        if (Zero_padding > 0) sampled_ms_ = 2;     // :80-85: 1 ms of code + 1 ms of zeros
        max_dwells_ = configuration_->property(role + ".max_dwells", 1);
        dump_filename_ = configuration_->property(role + ".dump_filename", std::string("../data/acquisition.dat"));
        bit_transition_flag_ = configuration_->property(role + ".bit_transition_flag", false);
        const std::string arithmetic = configuration_->property(role + ".arithmetic", std::string("reference"));
        arithmetic_ = arithmetic == "reference" ? GC_CAF_REFERENCE : (arithmetic == "exact" ? GC_CAF_EXACT : -1);  // unknown: the engine refuses it
        code_length_ = static_cast<unsigned int>(std::round(static_cast<double>(fs_in_) / 1.023e7 * 10230.0));  // :92
        vector_length_ = code_length_ * sampled_ms_;
        codeI_.assign(vector_length_, gr_complex(0.0f, 0.0f));
        codeQ_.assign(vector_length_, gr_complex(0.0f, 0.0f));
        const std::string sig = configuration_->property("Channel.signal", std::string("5X"));
        both_signal_components = sig.size() >= 2 && sig[0] == '5' && sig[1] == 'X';
        acquisition_ = std::make_shared<hip_e5a_noncoherent_iq_acquisition_caf>(sampled_ms_, max_dwells_, doppler_max_, fs_in_, static_cast<int32_t>(code_length_),
            static_cast<int32_t>(code_length_), bit_transition_flag_, dump_, dump_filename_, both_signal_components, CAF_window_hz_, Zero_padding, arithmetic_);
    }

    std::string role() override { return role_; }
    std::string implementation() override { return "Galileo_E5a_Noncoherent_IQ_Acquisition_CAF_HIP"; }
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
        // calculate_threshold (:288-305) is the Tong adapters' closed form: ncells = vector_length * inclusive bins, lambda = vector_length
        if (pfa != 0.0f) gc_tong_threshold(pfa, vector_length_, doppler_max_, doppler_step_, &threshold_);
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

    /*! set_local_code (:222-276): "5X" takes 5I and 5Q, any other signal its own code as the I component; sampled_ms code periods, or
     *  one period with zeros behind it when Zero_padding is set */
    void set_local_code() override
    {
        std::vector<gr_complex> codeI(code_length_ + 8), codeQ(code_length_ + 8);
        const bool x = gnss_synchro_->Signal[0] == '5' && gnss_synchro_->Signal[1] == 'X';
        if (x)
            {
                gc_galileo_e5_a_code_gen_complex_sampled(reinterpret_cast<float*>(codeI.data()), "5I", gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
                gc_galileo_e5_a_code_gen_complex_sampled(reinterpret_cast<float*>(codeQ.data()), "5Q", gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
            }
        else
            {
                const char sig[3] = {gnss_synchro_->Signal[0], gnss_synchro_->Signal[1], '\0'};
                gc_galileo_e5_a_code_gen_complex_sampled(reinterpret_cast<float*>(codeI.data()), sig, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
            }
        std::fill(codeI_.begin(), codeI_.end(), gr_complex(0.0f, 0.0f));
        std::fill(codeQ_.begin(), codeQ_.end(), gr_complex(0.0f, 0.0f));
        const unsigned int periods = Zero_padding == 0 ? sampled_ms_ : 1U;
        for (unsigned int i = 0; i < periods; i++)
            {
                std::memcpy(&codeI_[static_cast<size_t>(i) * code_length_], codeI.data(), sizeof(gr_complex) * code_length_);
                if (x) std::memcpy(&codeQ_[static_cast<size_t>(i) * code_length_], codeQ.data(), sizeof(gr_complex) * code_length_);
            }
        acquisition_->set_local_code(codeI_.data(), codeQ_.data());
    }

    void set_state(int state) override { acquisition_->set_state(state); }
    signed int mag() override { return acquisition_->mag(); }
    void reset() override { acquisition_->set_active(true); }
    void stop_acquisition() override {}
    void set_resampler_latency(uint32_t) override {}

    //! the block (get_left_block() in the reference)
    std::shared_ptr<hip_e5a_noncoherent_iq_acquisition_caf> block() { return acquisition_; }
    unsigned int vector_length() const { return vector_length_; }
    unsigned int code_length() const { return code_length_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int max_dwells() const { return max_dwells_; }
    unsigned int doppler_max() const { return doppler_max_; }
    int caf_window_hz() const { return CAF_window_hz_; }
    int zero_padding() const { return Zero_padding; }
    bool bit_transition_flag() const { return bit_transition_flag_; }
    bool both_components() const { return both_signal_components; }
    int arithmetic() const { return arithmetic_; }
    float threshold() const { return threshold_; }

private:
    ConfigurationInterface* configuration_;
    std::shared_ptr<hip_e5a_noncoherent_iq_acquisition_caf> acquisition_;
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
    unsigned int sampled_ms_ = 1;
    unsigned int max_dwells_ = 1;
    int CAF_window_hz_ = 0;
    int Zero_padding = 0;
    int arithmetic_ = GC_CAF_REFERENCE;
    bool bit_transition_flag_ = false;
    bool both_signal_components = false;
    bool dump_ = false;
    float threshold_ = 0.0f;
    int64_t fs_in_ = 0;
    std::vector<gr_complex> codeI_, codeQ_;
    std::shared_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_ = nullptr;
};

#endif  // GNSSCORR_HIP_E5A_NONCOHERENT_IQ_ACQUISITION_CAF_H_
