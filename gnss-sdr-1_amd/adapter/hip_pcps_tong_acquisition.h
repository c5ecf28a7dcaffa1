/*!
 * \file hip_pcps_tong_acquisition.h
 * \brief Image of pcps_tong_acquisition_cc (src/algorithms/acquisition/gnuradio_blocks/pcps_tong_acquisition_cc.{h,cc}) over a Tong
 * engine of libgnsscorr.so (gc_acq_create_tong), and the two AcquisitionInterface adapters in front of it:
 *   GpsL1CaPcpsTongAcquisitionHip             gps_l1_ca_pcps_tong_acquisition.cc
 *   GalileoE1PcpsTongAmbiguousAcquisitionHip  galileo_e1_pcps_tong_ambiguous_acquisition.cc
 *
 * Contracts kept:
 *   - d_fft_size = sampled_ms * samples_per_ms (:107), no zero padding; the Doppler bins run from -doppler_max to +doppler_max
 *     INCLUSIVE (:200-205); set_local_code takes d_fft_size samples (the adapters tile the code period);
 *   - state 1 (:303-419): every item is one dwell -- the grid gets this dwell's |.|^2 / (N^4 * its input power) on top, d_mag is the
 *     largest cell, and the Tong counter walks against threshold * dwell_count; positive at tong_max_val, negative at 0 or at
 *     tong_max_dwells.  All of it runs on the device (the engine's decision kernel); this class reads the outcome;
 *   - the sample counter advances by d_fft_size per item in every state (:297, :314, :437, :467) and the stamp of a winner is the
 *     counter AFTER its block (:314, :373);
 *   - states 2 and 3 publish 1 (ACQ_SUCCESS) / 2 (ACQ_FAIL) on "events", clear d_active and return to state 0;
 *   - general_work(noutput, ninput_items, input_items, ..) becomes work(in, ninput_items[0]) on host items of item_length() samples, or
 *     work_ring(ring, first_index, n_items) on items that lie in a gc_stream ring: there state 1 hands ALL available items (up to the
 *     dwells left) to ONE gc_acq_tong_search_stream call -- no host decision between the dwells -- and consumes the items up to
 *     and including the deciding one, as the block would have.
 * Documented departures:
 *   - `dump` is accepted and ignored (gc_acq_get_grid gives the grid);
 *   - a doppler_step of 0 (set_doppler_step never called) is taken as 250; the block's loop would not end.
 * The pure host-side pieces -- bin count, key handling, threshold rule -- are checked without a GPU by `tong_selftest --host`.
 */
#ifndef GNSSCORR_HIP_PCPS_TONG_ACQUISITION_H_
#define GNSSCORR_HIP_PCPS_TONG_ACQUISITION_H_

#include "acquisition_adapter_base.h"
#include "acquisition_block_base.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gnsscorr
{
//! init() (:198-205): both ends of the range count; a step of 0 means 250
inline uint32_t tong_doppler_bins(uint32_t doppler_max, uint32_t doppler_step) { return inclusive_doppler_bins(doppler_max, doppler_step ? doppler_step : 250); }
}  // namespace gnsscorr

class hip_pcps_tong_acquisition : public hip_acquisition_item_block
{
public:
    // general_work (:263-489): search state 1 (:303-419), positive 2, negative 3; set_state(1) restarts and leaves d_active alone (:233-251)
    hip_pcps_tong_acquisition(uint32_t sampled_ms, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms, int32_t samples_per_code, uint32_t tong_init_val,
        uint32_t tong_max_val, uint32_t tong_max_dwells, bool dump, const std::string& dump_filename)
        : hip_acquisition_item_block(Policy{1, 1, 2, 3, false}, sampled_ms, tong_max_dwells, doppler_max, fs_in, samples_per_ms, samples_per_code, dump, dump_filename,
              sampled_ms * static_cast<uint32_t>(samples_per_ms), sampled_ms * static_cast<uint32_t>(samples_per_ms)),
          d_tong_init_val(tong_init_val), d_tong_max_val(tong_max_val), d_tong_count(tong_init_val)
    {
        d_code.assign(d_fft_size, gr_complex(0.0f, 0.0f));
    }

    void set_threshold(float threshold) override
    {
        d_threshold = threshold;
        if (d_acq != nullptr) d_status = gc_acq_tong_set_threshold(d_acq.get(), d_threshold);
    }

    /*! set_local_code (:174-182): d_fft_size samples */
    void set_local_code(std::complex<float>* code)
    {
        std::memcpy(d_code.data(), code, sizeof(gr_complex) * d_code.size());
        d_have_code = true;
        if (d_acq != nullptr) d_status = load_code();
    }

    /*! general_work (:263-489) on items that lie in `ring` from absolute sample first_index on (a GC_IQ_F32 ring, or the format given
     *  to the engine); work(in, n) of the base is the same on host items of item_length() samples */
    int work_ring(gc_stream* ring, uint64_t first_index, int n_items) { return step(nullptr, ring, first_index, n_items); }

    uint32_t tong_count() const { return d_tong_count; }

private:
    // init (:185-227): counts the bins, creates the engine (wipe-off grid and zeroed data grid)
    gc_status create_engine() override
    {
        if (d_doppler_step == 0) d_doppler_step = 250;
        d_num_doppler_bins = gnsscorr::tong_doppler_bins(d_doppler_max, d_doppler_step);
        const gc_acq_conf c = conf(1.023e6, d_max_dwells);
        const gc_status status = make_engine([&](gc_ctx* ctx, gc_acq** acq) { return gc_acq_create_tong(ctx, &c, 1, d_tong_init_val, d_tong_max_val, d_max_dwells, acq); });
        return status == GC_OK ? gc_acq_tong_set_threshold(d_acq.get(), d_threshold) : status;
    }

    gc_status load_code() override { return gc_acq_set_local_code(d_acq.get(), 0, reinterpret_cast<const float*>(d_code.data())); }

    // "restart acquisition variables" (set_state(1) :233-251 and state 0 :275-292): the engine's grid reads as zero after gc_acq_reset
    void on_restart() override
    {
        d_tong_count = d_tong_init_val;
        reset_engine();
    }

    // state 1 (:303-419): one dwell on a host item, or all the dwells the ring's items allow in one call.  The counter and the dwell
    // count advance AFTER the call, by the dwells the device ran
    int search(const gr_complex* in, gc_stream* ring, uint64_t first_index, int n_items) override
    {
        if (n_items <= 0) return 0;
        gc_acq_result r;
        struct gc_acq_tong_status st;
        std::memset(&r, 0, sizeof r);
        std::memset(&st, 0, sizeof st);
        const uint32_t before = d_dwell_count;
        if (d_acq == nullptr)
            d_status = GC_ERR_STATE;
        else if (ring != nullptr)
            d_status = gc_acq_tong_search_stream(d_acq.get(), ring, first_index, static_cast<uint32_t>(n_items), &r, &st);
        else
            {
                d_status = gc_acq_dwell(d_acq.get(), reinterpret_cast<const float*>(in), &r);
                if (d_status == GC_OK) d_status = gc_acq_tong_status(d_acq.get(), &st);
            }
        if (d_status != GC_OK)
            {
                // nothing ran: the item is consumed and the search fails, so that a broken engine cannot hold a channel for ever
                count_items(1);
                d_dwell_count++;
                d_state = 3;
                return 1;
            }
        // the device stopped at the deciding dwell: the dwells behind it (enqueued blindly) moved nothing and are not consumed
        const uint32_t ran = st.dwell_count - before;
        d_last = r;
        d_dwell_count = st.dwell_count;
        d_tong_count = st.tong_count;
        d_sample_counter += static_cast<uint64_t>(d_fft_size) * ran;
        d_input_power = r.input_power;
        d_mag = r.mag;
        d_test_statistics = r.test_statistics;
        if (r.mag > 0.0f)
            {
                // :368-375 in the last dwell run (every earlier winner of this search has been overwritten by it)
                d_gnss_synchro->Acq_delay_samples = r.acq_delay_samples;
                d_gnss_synchro->Acq_doppler_hz = r.acq_doppler_hz;
                d_gnss_synchro->Acq_samplestamp_samples = d_sample_counter;
                d_gnss_synchro->Acq_doppler_step = d_doppler_step;
            }
        d_state = st.state == GC_ACQ_TONG_POSITIVE ? 2 : (st.state == GC_ACQ_TONG_NEGATIVE ? 3 : 1);
        return static_cast<int>(ran);
    }

    uint32_t d_tong_init_val, d_tong_max_val, d_tong_count;
    std::vector<gr_complex> d_code;
};

/*! GpsL1CaPcpsTongAcquisition (gps_l1_ca_pcps_tong_acquisition.cc:40-290) and GalileoE1PcpsTongAmbiguousAcquisition
 *  (galileo_e1_pcps_tong_ambiguous_acquisition.cc:41-300) over hip_pcps_tong_acquisition.  Keys of both: doppler_max,
 *  coherent_integration_time_ms (GPS: default 1; Galileo: default 4, rounded down to a multiple of 4), tong_init_val (1), tong_max_val (2),
 *  tong_max_dwells (tong_max_val + 1), <role><ch>.pfa and <role>.pfa (the threshold rule gc_tong_threshold), Acquisition<ch>.cboc
 *  (Galileo), dump, dump_filename.  code_length = round(fs / (1.023e6 / 1023)), vector_length = code_length * sampled_ms (GPS);
 *  code_length = round(fs / (1.023e6 / 4092)), vector_length = code_length * (sampled_ms / 4), samples_per_ms = code_length / 4
 *  (Galileo).  The local code is the code period tiled over vector_length. */
template <bool GALILEO>
class PcpsTongAcquisitionHip : public AcquisitionAdapterBase<hip_pcps_tong_acquisition>
{
public:
    PcpsTongAcquisitionHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : AcquisitionAdapterBase<hip_pcps_tong_acquisition>(configuration, role, in_streams, out_streams, GALILEO ? 4000000 : 2048000)
    {
        dump_ = configuration_->property(role + ".dump", false);
        doppler_max_ = configuration_->property(role + ".doppler_max", 5000);
        sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", GALILEO ? 4 : 1);
        if (GALILEO && sampled_ms_ % 4 != 0) sampled_ms_ = (sampled_ms_ / 4) * 4;
        tong_init_val_ = configuration_->property(role + ".tong_init_val", 1);
        tong_max_val_ = configuration_->property(role + ".tong_max_val", 2);
        tong_max_dwells_ = configuration_->property(role + ".tong_max_dwells", static_cast<int>(tong_max_val_ + 1));
        dump_filename_ = configuration_->property(role + ".dump_filename", std::string(GALILEO ? "../data/acquisition.dat" : "./data/acquisition.dat"));
        code_length_ = static_cast<unsigned int>(std::round(static_cast<double>(fs_in_) / (1.023e6 / (GALILEO ? 4092.0 : 1023.0))));
        vector_length_ = GALILEO ? code_length_ * (sampled_ms_ / 4) : code_length_ * sampled_ms_;
        const int samples_per_ms = GALILEO ? static_cast<int>(code_length_ / 4) : static_cast<int>(code_length_);
        acquisition_ = std::make_shared<hip_pcps_tong_acquisition>(sampled_ms_, doppler_max_, fs_in_, samples_per_ms, static_cast<int32_t>(code_length_), tong_init_val_,
            tong_max_val_, tong_max_dwells_, dump_, dump_filename_);
    }

    std::string implementation() override { return GALILEO ? "Galileo_E1_PCPS_Tong_Ambiguous_Acquisition_HIP" : "GPS_L1_CA_PCPS_Tong_Acquisition_HIP"; }

    void set_threshold(float threshold) override
    {
        const float pfa = pfa_for_channel();
        threshold_ = threshold;
        if (pfa != 0.0f) gc_tong_threshold(pfa, vector_length_, doppler_max_, doppler_step_ ? doppler_step_ : 250, &threshold_);
        acquisition_->set_threshold(threshold_);
    }

    void set_local_code() override
    {
        std::vector<gr_complex> code(code_length_ + 8), tiled(vector_length_);
        if (GALILEO)
            gnsscorr::e1_code_sampled(configuration_, channel_, gnss_synchro_, fs_in_, code.data());
        else
            gc_gps_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(code.data()), gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
        gnsscorr::tile_code(code.data(), code_length_, vector_length_ / code_length_, tiled.data());
        if (!tiled.empty()) acquisition_->set_local_code(tiled.data());
    }

    unsigned int code_length() const { return code_length_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int tong_init_val() const { return tong_init_val_; }
    unsigned int tong_max_val() const { return tong_max_val_; }
    unsigned int tong_max_dwells() const { return tong_max_dwells_; }

private:
    std::string dump_filename_;
    unsigned int sampled_ms_ = 1;
    unsigned int tong_init_val_ = 1, tong_max_val_ = 2, tong_max_dwells_ = 3;
    bool dump_ = false;
};

using GpsL1CaPcpsTongAcquisitionHip = PcpsTongAcquisitionHip<false>;
using GalileoE1PcpsTongAmbiguousAcquisitionHip = PcpsTongAcquisitionHip<true>;

#endif  // GNSSCORR_HIP_PCPS_TONG_ACQUISITION_H_
