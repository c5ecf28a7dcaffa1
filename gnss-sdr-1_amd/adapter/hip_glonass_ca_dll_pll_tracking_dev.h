/*!
 * \file hip_glonass_ca_dll_pll_tracking_dev.h
 * \brief The Glonass_L1_Ca_Dll_Pll_Tracking_cc / Glonass_L2_Ca_Dll_Pll_Tracking_cc block on the DEVICE loop
 * (gc_trk_loop_start_glonass): one work() call pushes the new input items into an HBM ring and runs every code period that is
 * complete in it -- correlations and the block's own loop maths in one launch -- then hands out the pull-in item and one
 * Gnss_Synchro per valid period.  Same configuration keys, same slot -> frequency-channel map and the same per-period results as
 * hip_glonass_ca_dll_pll_tracking (the host-loop image, one level-1 correlator launch and one host round trip per millisecond);
 * the loop itself lives in csrc/trk_closed_loop_glonass.hip.  TrackingInterface adapters: GlonassL1CaDllPllTrackingDevHip /
 * GlonassL2CaDllPllTrackingDevHip.
 */
#ifndef GNSSCORR_HIP_GLONASS_CA_DLL_PLL_TRACKING_DEV_H_
#define GNSSCORR_HIP_GLONASS_CA_DLL_PLL_TRACKING_DEV_H_

#include "hip_glonass_ca_dll_pll_tracking.h"
#include <algorithm>
#include <cstring>
#include <mutex>

namespace gnsscorr
{
//! what the GLONASS block's constructor is given
struct GlonassTrkConf
{
    int band = 1;
    int64_t fs_in = 0;
    uint32_t vector_length = 0;
    float pll_bw_hz = 50.0f, dll_bw_hz = 2.0f, early_late_space_chips = 0.5f;
    int cn0_samples = 20, cn0_min = 25, max_lock_fail = 50;
    double carrier_lock_th = 0.85;
};

/*! The item the block writes when it aligns to the code (glonass_l1_ca_dll_pll_tracking_cc.cc:570-590): the device loop does the
 *  same alignment before its first period and emits no record for it, so the item comes from gc_glonass_loop_pull_in, which runs
 *  the loop's own start and pull-in statements on the host. */
inline gc_status glonass_pull_in_item(const gc_glonass_loop_conf& c, const Gnss_Synchro& acq, Gnss_Synchro* item)
{
    uint64_t sample_counter = 0;
    double acc_carrier_phase_rad = 0.0;
    const gc_status st = gc_glonass_loop_pull_in(&c, nullptr, &sample_counter, &acc_carrier_phase_rad);
    if (st != GC_OK) return st;
    Gnss_Synchro s = acq;
    s.Tracking_sample_counter = sample_counter;
    s.Carrier_phase_rads = acc_carrier_phase_rad;
    s.Carrier_Doppler_hz = c.acq_doppler_hz;
    s.fs = static_cast<int64_t>(c.fs_in);
    s.correlation_length_ms = 1;
    *item = s;
    return GC_OK;
}

/*! start_tracking of one GLONASS channel of a device loop; `sample_counter` is the stream position the channel starts consuming
 *  at (the block's d_sample_counter).  *pull_in receives the item of the alignment. */
inline gc_status glonass_loop_start_channel(gc_trk_loop* loop, int ch, const GlonassTrkConf& t, const std::map<uint32_t, int32_t>& prn_to_channel, const Gnss_Synchro& acq,
    uint64_t sample_counter, Gnss_Synchro* pull_in)
{
    const auto slot = prn_to_channel.find(acq.PRN);
    if (slot == prn_to_channel.end()) return GC_ERR_INVALID;
    const GlonassBand band = glonass_band(t.band);
    gc_glonass_loop_conf c;
    std::memset(&c, 0, sizeof c);
    c.fs_in = static_cast<double>(t.fs_in);
    c.band_carrier_freq_hz = band.freq_hz;
    c.channel_offset_hz = band.dfreq_hz * slot->second;
    c.carrier_lock_th = t.carrier_lock_th;
    c.acq_delay_samples = acq.Acq_delay_samples;
    c.acq_doppler_hz = acq.Acq_doppler_hz;
    c.acq_samplestamp_samples = acq.Acq_samplestamp_samples;
    c.sample_counter = sample_counter;
    c.vector_length = t.vector_length;
    c.cn0_samples = t.cn0_samples;
    c.cn0_min = t.cn0_min;
    c.max_lock_fail = t.max_lock_fail;
    c.pll_bw_hz = t.pll_bw_hz;
    c.dll_bw_hz = t.dll_bw_hz;
    c.early_late_space_chips = t.early_late_space_chips;
    Gnss_Synchro item;
    gc_status st = glonass_pull_in_item(c, acq, &item);
    if (st == GC_OK) st = gc_trk_loop_start_glonass(loop, ch, &c);
    if (st == GC_OK && pull_in) *pull_in = item;
    return st;
}

//! what a period hands to the telemetry decoder (:752-764), from the device loop's record
inline Gnss_Synchro glonass_synchro_from_record(const gc_loop_record& r, const Gnss_Synchro& acq, int64_t fs_in)
{
    Gnss_Synchro s = acq;
    s.Prompt_I = static_cast<double>(r.prompt_data[0]);
    s.Prompt_Q = static_cast<double>(r.prompt_data[1]);
    s.Tracking_sample_counter = r.sample_counter;
    s.Code_phase_samples = r.rem_code_phase_samples;
    s.Carrier_phase_rads = r.acc_carrier_phase_rad;
    s.Carrier_Doppler_hz = r.carrier_doppler_hz;
    s.CN0_dB_hz = r.cn0_db_hz;
    s.Flag_valid_symbol_output = true;
    s.correlation_length_ms = 1;
    s.fs = fs_in;
    return s;
}
}  // namespace gnsscorr

class hip_glonass_ca_dll_pll_tracking_dev
{
public:
    /*! ring_periods: code periods of input the HBM ring holds (a work() call may bring at most that many) */
    hip_glonass_ca_dll_pll_tracking_dev(int band, int64_t fs_in, uint32_t vector_length, float pll_bw_hz, float dll_bw_hz, float early_late_space_chips, int cn0_samples = 20,
        int cn0_min = 25, int max_lock_fail = 50, double carrier_lock_th = 0.85, int device = 0, int ring_periods = 64)
        : d_ring_periods(ring_periods), d_glonass_prn(gnsscorr::glonass_default_channels())
    {
        d_conf.band = band;
        d_conf.fs_in = fs_in;
        d_conf.vector_length = vector_length;
        d_conf.pll_bw_hz = pll_bw_hz;
        d_conf.dll_bw_hz = dll_bw_hz;
        d_conf.early_late_space_chips = early_late_space_chips;
        d_conf.cn0_samples = cn0_samples;
        d_conf.cn0_min = cn0_min;
        d_conf.max_lock_fail = max_lock_fail;
        d_conf.carrier_lock_th = carrier_lock_th;
        d_status = gc_ctx_create(device, &d_ctx);
        if (d_status == GC_OK) d_status = gc_stream_create(d_ctx, GC_IQ_F32, static_cast<uint64_t>(vector_length) * ring_periods, 2 * vector_length, &d_ring);
        if (d_status == GC_OK) d_status = gc_trk_loop_create(d_ctx, 1, 511, &d_loop);
        if (d_status == GC_OK) d_status = gc_trk_loop_set_input_stream(d_loop, 0, d_ring);
        d_records.resize(ring_periods + 2);
    }

    ~hip_glonass_ca_dll_pll_tracking_dev()
    {
        if (d_loop) gc_trk_loop_destroy(d_loop);
        if (d_ring) gc_stream_destroy(d_ring);
        if (d_ctx) gc_ctx_destroy(d_ctx);
    }
    hip_glonass_ca_dll_pll_tracking_dev(const hip_glonass_ca_dll_pll_tracking_dev&) = delete;
    hip_glonass_ca_dll_pll_tracking_dev& operator=(const hip_glonass_ca_dll_pll_tracking_dev&) = delete;

    void set_channel(uint32_t channel) { d_channel = channel; }
    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_acquisition_gnss_synchro = p_gnss_synchro; }
    //! the slot -> frequency channel map comes from the almanac in a live receiver
    void set_glonass_channel_map(const std::map<uint32_t, int32_t>& prn_to_channel) { d_glonass_prn = prn_to_channel; }

    //! start_tracking (:160-243) on the device
    void start_tracking()
    {
        std::lock_guard<std::mutex> l(d_setlock);
        if (d_status != GC_OK) return;
        d_status = gnsscorr::glonass_loop_start_channel(d_loop, 0, d_conf, d_glonass_prn, *d_acquisition_gnss_synchro, d_sample_counter, &d_pull_in_item);
        d_state = d_status == GC_OK ? 1 : 0;
        d_pull_in = d_status == GC_OK;
    }

    void stop_tracking()
    {
        std::lock_guard<std::mutex> l(d_setlock);
        if (d_state != 0 && d_loop) gc_trk_loop_stop(d_loop, 0);
        d_state = 0;
    }

    //! forecast: like the reference block, two code periods
    int required_input_items() const { return static_cast<int>(d_conf.vector_length) * 2; }

    /*! general_work: `in` points at the first unconsumed item, ninput_items are available, at most max_out Gnss_Synchro fit in
     *  `out`.  Returns the items consumed; *produced = Gnss_Synchro written: the pull-in item first, then one per valid period. */
    int work(const gr_complex* in, int ninput_items, Gnss_Synchro* out, int max_out, int* produced)
    {
        std::lock_guard<std::mutex> l(d_setlock);
        *produced = 0;
        if (d_state == 0 || d_status != GC_OK)
            {
                // standby: the items pass by (they are not needed in HBM), the counters move on
                d_sample_counter += static_cast<uint64_t>(ninput_items);
                d_pushed = std::max(d_pushed, d_sample_counter);
                return ninput_items;
            }
        // 1. the items that are not in the ring yet (the scheduler shows again what was not consumed last time)
        const uint64_t have = d_pushed - d_sample_counter;  // already pushed, not yet consumed
        uint64_t fresh = static_cast<uint64_t>(ninput_items) > have ? static_cast<uint64_t>(ninput_items) - have : 0;
        const uint64_t room = static_cast<uint64_t>(d_conf.vector_length) * d_ring_periods - have;
        fresh = std::min(fresh, room);
        if (fresh > 0)
            {
                if (d_ring_head != d_pushed)
                    {
                        // items went by in standby: the ring's numbering continues at the stream position (zeros fill the gap)
                        d_status = skip_to(d_pushed);
                        if (d_status != GC_OK) return 0;
                    }
                d_status = gc_stream_push(d_ring, in + have, fresh, nullptr);
                if (d_status != GC_OK) return 0;
                d_pushed += fresh;
                d_ring_head = d_pushed;
            }
        if (d_pull_in && max_out > 0)
            {
                out[(*produced)++] = d_pull_in_item;
                d_pull_in = false;
            }
        // 2. every complete code period in one launch
        const int n_periods = std::min<int>(std::min<int>(max_out - *produced, static_cast<int>(d_records.size())),
            static_cast<int>((d_pushed - d_sample_counter) / d_conf.vector_length) + 1);
        if (n_periods <= 0) return 0;
        d_status = gc_trk_loop_run(d_loop, n_periods, d_records.data());
        if (d_status != GC_OK) return 0;
        // 3. records -> Gnss_Synchro; the launch stops at the first period that is not complete
        uint64_t position = d_sample_counter;
        for (int k = 0; k < n_periods; k++)
            {
                const gc_loop_record& r = d_records[k];
                if (r.valid == 0) break;  // nothing was correlated: out of input
                position = r.sample_counter;
                d_state = r.state;
                d_last = r;
                out[(*produced)++] = gnsscorr::glonass_synchro_from_record(r, *d_acquisition_gnss_synchro, d_conf.fs_in);
                if (r.state == 0)
                    {
                        d_events.push_back(3);  // loss of lock (:741)
                        gc_trk_loop_stop(d_loop, 0);
                        break;
                    }
            }
        const int consumed = static_cast<int>(position - d_sample_counter);
        d_sample_counter = position;
        return consumed;
    }

    bool tracking_enabled() const { return d_state != 0; }
    int32_t state() const { return d_state; }
    double carrier_doppler_hz() const { return d_last.carrier_doppler_hz; }
    double code_freq_chips() const { return d_last.code_freq_chips; }
    double cn0_db_hz() const { return d_last.cn0_db_hz; }
    double carrier_lock_test() const { return d_last.carrier_lock_test; }
    uint64_t sample_counter() const { return d_sample_counter; }
    const gc_loop_record& last_record() const { return d_last; }
    const std::vector<int>& events() const { return d_events; }
    gc_status last_status() const { return d_status; }

private:
    //! appends zeros until the ring's head is at absolute sample `index`
    gc_status skip_to(uint64_t index)
    {
        std::vector<gr_complex> zeros(std::min<uint64_t>(index - d_ring_head, 1u << 16));
        while (d_ring_head < index)
            {
                const uint64_t n = std::min<uint64_t>(index - d_ring_head, zeros.size());
                gc_status s = gc_stream_push(d_ring, zeros.data(), n, nullptr);
                if (s != GC_OK) return s;
                d_ring_head += n;
            }
        return GC_OK;
    }

    gnsscorr::GlonassTrkConf d_conf;
    int d_ring_periods;
    std::map<uint32_t, int32_t> d_glonass_prn;
    std::mutex d_setlock;
    gc_ctx* d_ctx = nullptr;
    gc_stream* d_ring = nullptr;
    gc_trk_loop* d_loop = nullptr;
    gc_status d_status = GC_OK;
    Gnss_Synchro* d_acquisition_gnss_synchro = nullptr;
    Gnss_Synchro d_pull_in_item{};
    bool d_pull_in = false;
    uint32_t d_channel = 0;
    int32_t d_state = 0;
    uint64_t d_sample_counter = 0;  // absolute index of the first unconsumed item (the block's d_sample_counter)
    uint64_t d_pushed = 0;          // absolute index one past the last item seen
    uint64_t d_ring_head = 0;       // absolute index one past the last item in the ring
    std::vector<gc_loop_record> d_records;
    gc_loop_record d_last{};
    std::vector<int> d_events;
};

//! TrackingInterface adapter on the device loop: the configuration keys of glonass_l1_ca_dll_pll_tracking.cc:46-130 ("2G": the same)
template <int BAND>
class GlonassCaDllPllTrackingDevHip : public TrackingInterface
{
public:
    GlonassCaDllPllTrackingDevHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : role_(role), in_streams_(in_streams), out_streams_(out_streams)
    {
        int fs_in_deprecated = configuration->property("GNSS-SDR.internal_fs_hz", 2048000);
        const int fs_in = configuration->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
        const float pll_bw_hz = configuration->property(role + ".pll_bw_hz", 50.0f);
        const float dll_bw_hz = configuration->property(role + ".dll_bw_hz", 2.0f);
        const float early_late_space_chips = configuration->property(role + ".early_late_space_chips", 0.5f);
        vector_length_ = std::round(fs_in / (0.511e6 / 511.0));
        tracking_ = std::make_shared<hip_glonass_ca_dll_pll_tracking_dev>(BAND, fs_in, vector_length_, pll_bw_hz, dll_bw_hz, early_late_space_chips,
            configuration->property(role + ".cn0_samples", 20), configuration->property(role + ".cn0_min", 25), configuration->property(role + ".max_lock_fail", 50),
            configuration->property(role + ".carrier_lock_th", 0.85));
    }

    std::string role() override { return role_; }
    std::string implementation() override { return BAND == 2 ? "GLONASS_L2_CA_DLL_PLL_Tracking_Dev_HIP" : "GLONASS_L1_CA_DLL_PLL_Tracking_Dev_HIP"; }
    size_t item_size() override { return sizeof(gr_complex); }
    void start_tracking() override { tracking_->start_tracking(); }
    void stop_tracking() override { tracking_->stop_tracking(); }
    void set_channel(unsigned int channel) override { tracking_->set_channel(channel); }
    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) override { tracking_->set_gnss_synchro(p_gnss_synchro); }
    std::shared_ptr<hip_glonass_ca_dll_pll_tracking_dev> block() { return tracking_; }
    unsigned int vector_length() const { return vector_length_; }

private:
    std::shared_ptr<hip_glonass_ca_dll_pll_tracking_dev> tracking_;
    std::string role_;
    unsigned int in_streams_, out_streams_;
    unsigned int vector_length_ = 0;
};

using GlonassL1CaDllPllTrackingDevHip = GlonassCaDllPllTrackingDevHip<1>;
using GlonassL2CaDllPllTrackingDevHip = GlonassCaDllPllTrackingDevHip<2>;

#endif  // GNSSCORR_HIP_GLONASS_CA_DLL_PLL_TRACKING_DEV_H_
