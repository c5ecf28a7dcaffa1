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

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include "hip_multicorrelator_real_codes.h"  // gnsscorr::shared_context()
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gnsscorr
{
//! init() (:198-205): both ends of the range count
inline uint32_t tong_doppler_bins(uint32_t doppler_max, uint32_t doppler_step)
{
    if (doppler_step == 0) doppler_step = 250;
    uint32_t n = 0;
    for (int64_t doppler = -static_cast<int64_t>(doppler_max); doppler <= static_cast<int64_t>(doppler_max); doppler += doppler_step) n++;
    return n;
}
}  // namespace gnsscorr

class hip_pcps_tong_acquisition
{
public:
    hip_pcps_tong_acquisition(uint32_t sampled_ms, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms, int32_t samples_per_code, uint32_t tong_init_val,
        uint32_t tong_max_val, uint32_t tong_max_dwells, bool dump, const std::string& dump_filename)
        : d_fs_in(fs_in), d_samples_per_ms(samples_per_ms), d_samples_per_code(samples_per_code), d_sampled_ms(sampled_ms), d_doppler_max(doppler_max), d_tong_init_val(tong_init_val), d_tong_max_val(tong_max_val), d_tong_max_dwells(tong_max_dwells), d_tong_count(tong_init_val), d_dump(dump), d_dump_filename(dump_filename)
    {
        d_fft_size = d_sampled_ms * static_cast<uint32_t>(d_samples_per_ms);
        d_code.assign(d_fft_size, gr_complex(0.0f, 0.0f));
    }

    ~hip_pcps_tong_acquisition()
    {
        if (d_acq != nullptr) gc_acq_destroy(d_acq);
    }

    hip_pcps_tong_acquisition(const hip_pcps_tong_acquisition&) = delete;
    hip_pcps_tong_acquisition& operator=(const hip_pcps_tong_acquisition&) = delete;

    inline void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    inline uint32_t mag() const { return d_mag; }
    inline void set_active(bool active) { d_active = active; }
    inline void set_channel(uint32_t channel) { d_channel = channel; }
    inline void set_doppler_max(uint32_t doppler_max) { d_doppler_max = doppler_max; }
    inline void set_doppler_step(uint32_t doppler_step) { d_doppler_step = doppler_step; }
    inline void set_threshold(float threshold)
    {
        d_threshold = threshold;
        if (d_acq != nullptr) d_status = gc_acq_tong_set_threshold(d_acq, d_threshold);
    }

    /*! set_local_code (:174-182): d_fft_size samples */
    void set_local_code(std::complex<float>* code)
    {
        std::memcpy(d_code.data(), code, sizeof(gr_complex) * d_code.size());
        d_have_code = true;
        if (d_acq != nullptr) d_status = gc_acq_set_local_code(d_acq, 0, reinterpret_cast<const float*>(d_code.data()));
    }

    /*! init (:185-227): clears the synchro fields, counts the bins, (re)creates the engine (wipe-off grid and zeroed data grid) */
    void init()
    {
        d_gnss_synchro->Flag_valid_acquisition = false;
        d_gnss_synchro->Flag_valid_symbol_output = false;
        d_gnss_synchro->Flag_valid_pseudorange = false;
        d_gnss_synchro->Flag_valid_word = false;
        d_gnss_synchro->Acq_doppler_step = 0U;
        d_gnss_synchro->Acq_delay_samples = 0.0;
        d_gnss_synchro->Acq_doppler_hz = 0.0;
        d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
        d_mag = 0.0;
        d_input_power = 0.0;
        if (d_doppler_step == 0) d_doppler_step = 250;
        d_num_doppler_bins = gnsscorr::tong_doppler_bins(d_doppler_max, d_doppler_step);
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
        c.max_dwells = d_tong_max_dwells;
        gc_ctx* ctx = gnsscorr::shared_context();
        d_status = ctx ? gc_acq_create_tong(ctx, &c, 1, d_tong_init_val, d_tong_max_val, d_tong_max_dwells, &d_acq) : GC_ERR_NO_DEVICE;
        if (d_status == GC_OK) d_status = gc_acq_tong_set_threshold(d_acq, d_threshold);
        if (d_status == GC_OK && d_have_code) d_status = gc_acq_set_local_code(d_acq, 0, reinterpret_cast<const float*>(d_code.data()));
    }

    void set_state(int32_t state)
    {
        d_state = state;
        if (d_state == 1) restart();
    }

    /*! general_work (:263-489) on host items of item_length() samples.  Returns the number of items consumed. */
    int work(const gr_complex* in, int ninput_items) { return step(in, nullptr, 0, ninput_items); }

    /*! the same on items that lie in `ring` from absolute sample first_index on (a GC_IQ_F32 ring, or the format given to the engine) */
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
    uint32_t dwell_count() const { return d_dwell_count; }
    uint32_t tong_count() const { return d_tong_count; }
    int32_t state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    gc_status last_status() const { return d_status; }
    gc_acq* engine() { return d_acq; }

private:
    // "restart acquisition variables" (set_state(1) :233-251 and state 0 :275-292): the engine's grid reads as zero after gc_acq_reset
    void restart()
    {
        d_gnss_synchro->Acq_delay_samples = 0.0;
        d_gnss_synchro->Acq_doppler_hz = 0.0;
        d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
        d_gnss_synchro->Acq_doppler_step = 0U;
        d_dwell_count = 0;
        d_tong_count = d_tong_init_val;
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
                return n_items > 0 ? dwells(in, ring, first_index, n_items) : 0;
            case 2:
            case 3:
                d_active = false;
                d_events.push_back(d_state == 2 ? 1 : 2);
                d_state = 0;
                d_sample_counter += static_cast<uint64_t>(d_fft_size) * static_cast<uint64_t>(n_items);
                return n_items;
            }
        return 0;
    }

    // state 1 (:303-419): one dwell on a host item, or all the dwells the ring's items allow in one call.  Returns the items consumed
    int dwells(const gr_complex* in, gc_stream* ring, uint64_t first_index, int n_items)
    {
        gc_acq_result r;
        struct gc_acq_tong_status st;
        std::memset(&r, 0, sizeof r);
        std::memset(&st, 0, sizeof st);
        const uint32_t before = d_dwell_count;
        if (d_acq == nullptr)
            d_status = GC_ERR_STATE;
        else if (ring != nullptr)
            d_status = gc_acq_tong_search_stream(d_acq, ring, first_index, static_cast<uint32_t>(n_items), &r, &st);
        else
            {
                d_status = gc_acq_dwell(d_acq, reinterpret_cast<const float*>(in), &r);
                if (d_status == GC_OK) d_status = gc_acq_tong_status(d_acq, &st);
            }
        if (d_status != GC_OK)
            {
                // nothing ran: the item is consumed and the search fails, so that a broken engine cannot hold a channel for ever
                d_sample_counter += static_cast<uint64_t>(d_fft_size);
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

    int64_t d_fs_in;
    int32_t d_samples_per_ms, d_samples_per_code;
    uint32_t d_sampled_ms, d_doppler_max, d_tong_init_val, d_tong_max_val, d_tong_max_dwells, d_tong_count;
    bool d_dump;
    std::string d_dump_filename;
    uint32_t d_fft_size = 0U, d_num_doppler_bins = 0U, d_doppler_step = 0U, d_channel = 0U, d_dwell_count = 0U;
    uint64_t d_sample_counter = 0ULL;
    int32_t d_state = 0;
    bool d_active = false, d_have_code = false;
    float d_threshold = 0.0f, d_mag = 0.0f, d_input_power = 0.0f, d_test_statistics = 0.0f;
    gc_acq* d_acq = nullptr;
    gc_status d_status = GC_OK;
    gc_acq_result d_last{};
    Gnss_Synchro* d_gnss_synchro = nullptr;
    std::vector<gr_complex> d_code;
    std::vector<int> d_events;
};

/*! GpsL1CaPcpsTongAcquisition (gps_l1_ca_pcps_tong_acquisition.cc:40-290) and GalileoE1PcpsTongAmbiguousAcquisition
 *  (galileo_e1_pcps_tong_ambiguous_acquisition.cc:41-300) over hip_pcps_tong_acquisition.  Keys of both: doppler_max,
 *  coherent_integration_time_ms (GPS: default 1; Galileo: default 4, rounded down to a multiple of 4), tong_init_val (1), tong_max_val (2),
 *  tong_max_dwells (tong_max_val + 1), <role><ch>.pfa and <role>.pfa (the threshold rule gc_tong_threshold), Acquisition<ch>.cboc
 *  (Galileo), dump, dump_filename.  code_length = round(fs / (1.023e6 / 1023)), vector_length = code_length * sampled_ms (GPS);
 *  code_length = round(fs / (1.023e6 / 4092)), vector_length = code_length * (sampled_ms / 4), samples_per_ms = code_length / 4
 *  (Galileo).  The local code is the code period tiled over vector_length. */
template <bool GALILEO>
class PcpsTongAcquisitionHip : public AcquisitionInterface
{
public:
    PcpsTongAcquisitionHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : configuration_(configuration), role_(role), in_streams_(in_streams), out_streams_(out_streams)
    {
        item_type_ = configuration_->property(role + ".item_type", std::string("gr_complex"));
        int64_t fs_in_deprecated = configuration_->property("GNSS-SDR.internal_fs_hz", static_cast<int64_t>(GALILEO ? 4000000 : 2048000));
        fs_in_ = configuration_->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
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

    std::string role() override { return role_; }
    std::string implementation() override { return GALILEO ? "Galileo_E1_PCPS_Tong_Ambiguous_Acquisition_HIP" : "GPS_L1_CA_PCPS_Tong_Acquisition_HIP"; }
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
        if (pfa != 0.0f) gc_tong_threshold(pfa, vector_length_, doppler_max_, doppler_step_ ? doppler_step_ : 250, &threshold_);
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
        std::vector<gr_complex> code(code_length_ + 8), tiled(vector_length_);
        if (GALILEO)
            {
                const bool cboc = configuration_->property("Acquisition" + std::to_string(channel_) + ".cboc", false);
                const char* sig = (gnss_synchro_->Signal[0] == '1' && gnss_synchro_->Signal[1] == 'C') ? "1C" : "1B";
                gc_galileo_e1_code_gen_complex_sampled(reinterpret_cast<float*>(code.data()), sig, cboc ? 1 : 0, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
            }
        else
            gc_gps_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(code.data()), gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
        for (unsigned int i = 0; i < vector_length_ / code_length_; i++) std::memcpy(&tiled[static_cast<size_t>(i) * code_length_], code.data(), sizeof(gr_complex) * code_length_);
        if (!tiled.empty()) acquisition_->set_local_code(tiled.data());
    }

    void set_state(int state) override { acquisition_->set_state(state); }
    signed int mag() override { return acquisition_->mag(); }
    void reset() override { acquisition_->set_active(true); }
    void stop_acquisition() override {}
    void set_resampler_latency(uint32_t) override {}

    //! the block (get_left_block() is a stream_to_vector in front of it in the reference)
    std::shared_ptr<hip_pcps_tong_acquisition> block() { return acquisition_; }
    unsigned int vector_length() const { return vector_length_; }
    unsigned int code_length() const { return code_length_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int tong_init_val() const { return tong_init_val_; }
    unsigned int tong_max_val() const { return tong_max_val_; }
    unsigned int tong_max_dwells() const { return tong_max_dwells_; }
    float threshold() const { return threshold_; }

private:
    ConfigurationInterface* configuration_;
    std::shared_ptr<hip_pcps_tong_acquisition> acquisition_;
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
    unsigned int tong_init_val_ = 1, tong_max_val_ = 2, tong_max_dwells_ = 3;
    bool dump_ = false;
    float threshold_ = 0.0f;
    int64_t fs_in_ = 0;
    std::shared_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_ = nullptr;
};

using GpsL1CaPcpsTongAcquisitionHip = PcpsTongAcquisitionHip<false>;
using GalileoE1PcpsTongAmbiguousAcquisitionHip = PcpsTongAcquisitionHip<true>;

#endif  // GNSSCORR_HIP_PCPS_TONG_ACQUISITION_H_
