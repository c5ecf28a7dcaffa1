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

#include "acquisition_adapter_base.h"
#include "acquisition_block_base.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

class hip_e5a_noncoherent_iq_acquisition_caf : public hip_acquisition_item_block
{
public:
    // general_work (:360-860): search states 1 and 2 (:405-804), positive 3, negative 4; set_state(1) restarts and leaves d_active alone
    // (:339-349).  d_doppler_step starts at 250, not 0
    hip_e5a_noncoherent_iq_acquisition_caf(uint32_t sampled_ms, uint32_t max_dwells, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms, int32_t samples_per_code,
        bool bit_transition_flag, bool dump, const std::string& dump_filename, bool both_signal_components, int32_t CAF_window_hz, int32_t Zero_padding,
        int32_t arithmetic = GC_CAF_REFERENCE)
        : hip_acquisition_item_block(Policy{1, 2, 3, 4, false}, sampled_ms, max_dwells, doppler_max, fs_in, samples_per_ms, samples_per_code, dump, dump_filename,
              sampled_ms * static_cast<uint32_t>(samples_per_ms), sampled_ms * static_cast<uint32_t>(samples_per_ms), 250U),
          d_bit_transition_flag(bit_transition_flag), d_both_signal_components(both_signal_components), d_CAF_window_hz(CAF_window_hz), d_arithmetic(arithmetic)
    {
        d_hypothesis_ms = Zero_padding > 0 ? 1U : sampled_ms;  // :92-99: the number of code periods the hypotheses are made for
        d_code_i.assign(d_fft_size, gr_complex(0.0f, 0.0f));
        d_code_q.assign(d_fft_size, gr_complex(0.0f, 0.0f));
    }

    /*! set_local_code (:234-282): d_fft_size samples of each component; codeQ is read with both components only */
    void set_local_code(std::complex<float>* codeI, std::complex<float>* codeQ)
    {
        std::memcpy(d_code_i.data(), codeI, sizeof(gr_complex) * d_fft_size);
        if (d_both_signal_components) std::memcpy(d_code_q.data(), codeQ, sizeof(gr_complex) * d_fft_size);
        d_have_code = true;
        if (d_acq != nullptr) d_status = load_code();
    }

    /*! general_work on items that lie in `ring` from absolute sample first_index on (a GC_IQ_F32 ring); work(in, n) of the base is the
     *  same on host items of item_length() samples */
    int work_ring(gc_stream* ring, uint64_t first_index, int n_items) { return step(nullptr, ring, first_index, n_items); }

    uint32_t hypotheses() const { return d_hypothesis_ms > 1 ? 2U : 1U; }
    bool both_signal_components() const { return d_both_signal_components; }
    uint32_t well_count() const { return d_dwell_count; }
    const std::vector<gr_complex>& code_i() const { return d_code_i; }
    const std::vector<gr_complex>& code_q() const { return d_code_q; }

private:
    // init (:285-333): counts the bins, creates the engine (wipe-off grid, CAF vectors).  A step of 0 has 0 bins: the engine refuses
    gc_status create_engine() override
    {
        d_num_doppler_bins = gnsscorr::inclusive_doppler_bins(d_doppler_max, d_doppler_step);
        gc_acq_conf c = conf(1.023e7, d_max_dwells);
        c.bit_transition_flag = d_bit_transition_flag ? 1 : 0;
        return make_engine([&](gc_ctx* ctx, gc_acq** acq) {
            return gc_acq_create_caf(ctx, &c, 1, d_both_signal_components ? 1 : 0, hypotheses(), d_CAF_window_hz > 0 ? static_cast<uint32_t>(d_CAF_window_hz) : 0U, d_arithmetic, acq);
        });
    }

    gc_status load_code() override
    {
        return gc_acq_set_local_code_iq(d_acq.get(), 0, reinterpret_cast<const float*>(d_code_i.data()),
            d_both_signal_components ? reinterpret_cast<const float*>(d_code_q.data()) : nullptr);
    }

    // "restart acquisition variables" (set_state(1) :339-349 and state 0 :389-398): gc_acq_reset zeroes the kept statistic
    void on_restart() override { reset_engine(); }

    // states 1 + 2 (:405-804): one block, one dwell; the counter and the dwell count advance BEFORE the dwell.  Returns the items
    // consumed (1)
    int search(const gr_complex* in, gc_stream* ring, uint64_t first_index, int n_items) override
    {
        if (n_items <= 0) return 0;
        gc_acq_result r;
        std::memset(&r, 0, sizeof r);
        count_items(1);
        d_dwell_count++;
        if (d_acq == nullptr)
            {
                if (d_status == GC_OK) d_status = GC_ERR_STATE;  // an earlier error status (init's) is kept
            }
        else if (ring != nullptr)
            d_status = gc_acq_dwell_stream(d_acq.get(), ring, first_index, &r);
        else
            d_status = gc_acq_dwell(d_acq.get(), reinterpret_cast<const float*>(in), &r);
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
        if (d_dwell_count == d_max_dwells)
            d_state = d_test_statistics > d_threshold ? 3 : 4;  // :785-795
        else
            d_state = 1;
        return 1;
    }

    bool d_bit_transition_flag, d_both_signal_components;
    int32_t d_CAF_window_hz, d_arithmetic;
    uint32_t d_hypothesis_ms = 1U;
    std::vector<gr_complex> d_code_i, d_code_q;
};

/*! GalileoE5aNoncoherentIQAcquisitionCaf (galileo_e5a_noncoherent_iq_acquisition_caf.cc:47-305) over
 *  hip_e5a_noncoherent_iq_acquisition_caf.  Keys and defaults: doppler_max (5000), CAF_window_hz (0), Zero_padding (0),
 *  coherent_integration_time_ms (1; capped at 3; forced to 2 with Zero_padding), max_dwells (1), bit_transition_flag (false),
 *  <role><ch>.pfa and <role>.pfa (the threshold rule: gc_tong_threshold on vector_length), dump, dump_filename, Channel.signal ("5X":
 *  both components), and the extension key arithmetic ("reference" | "exact").  code_length = round(fs / 1.023e7 * 10230),
 *  vector_length = code_length * sampled_ms. */
class GalileoE5aNoncoherentIQAcquisitionCafHip : public AcquisitionAdapterBase<hip_e5a_noncoherent_iq_acquisition_caf>
{
public:
    GalileoE5aNoncoherentIQAcquisitionCafHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : AcquisitionAdapterBase<hip_e5a_noncoherent_iq_acquisition_caf>(configuration, role, in_streams, out_streams, 32000000)
    {
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

    std::string implementation() override { return "Galileo_E5a_Noncoherent_IQ_Acquisition_CAF_HIP"; }

    void set_threshold(float threshold) override
    {
        const float pfa = pfa_for_channel();
        threshold_ = threshold;
        // calculate_threshold (:288-305) is the Tong adapters' closed form: ncells = vector_length * inclusive bins, lambda = vector_length
        if (pfa != 0.0f) gc_tong_threshold(pfa, vector_length_, doppler_max_, doppler_step_, &threshold_);
        acquisition_->set_threshold(threshold_);
    }

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
        gnsscorr::tile_code(codeI.data(), code_length_, periods, codeI_.data());
        if (x) gnsscorr::tile_code(codeQ.data(), code_length_, periods, codeQ_.data());
        acquisition_->set_local_code(codeI_.data(), codeQ_.data());
    }

    unsigned int code_length() const { return code_length_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int max_dwells() const { return max_dwells_; }
    unsigned int doppler_max() const { return doppler_max_; }
    int caf_window_hz() const { return CAF_window_hz_; }
    int zero_padding() const { return Zero_padding; }
    bool bit_transition_flag() const { return bit_transition_flag_; }
    bool both_components() const { return both_signal_components; }
    int arithmetic() const { return arithmetic_; }

private:
    std::string dump_filename_;
    unsigned int sampled_ms_ = 1;
    unsigned int max_dwells_ = 1;
    int CAF_window_hz_ = 0;
    int Zero_padding = 0;
    int arithmetic_ = GC_CAF_REFERENCE;
    bool bit_transition_flag_ = false;
    bool both_signal_components = false;
    bool dump_ = false;
    std::vector<gr_complex> codeI_, codeQ_;
};

#endif  // GNSSCORR_HIP_E5A_NONCOHERENT_IQ_ACQUISITION_CAF_H_
