/*!
 * \file hip_glonass_ca_dll_pll_tracking_dev.h
 * \brief The Glonass_L1_Ca_Dll_Pll_Tracking_cc / Glonass_L2_Ca_Dll_Pll_Tracking_cc block on the DEVICE loop
 * (gc_trk_loop_start_glonass): one work() call pushes the new input items into an HBM ring and runs every code period that is
 * complete in it -- correlations and the block's own loop maths in one launch -- then hands out the pull-in item and one
 * Gnss_Synchro per valid period (hip_device_loop_block, tracking_block_base.h, under the GLONASS policy).  Same configuration keys,
 * same slot -> frequency-channel map and the same per-period results as hip_glonass_ca_dll_pll_tracking (the host-loop image, one
 * level-1 correlator launch and one host round trip per millisecond); the loop itself lives in csrc/trk_closed_loop_glonass.hip.
 * TrackingInterface adapters: GlonassL1CaDllPllTrackingDevHip / GlonassL2CaDllPllTrackingDevHip.
 */
#ifndef GNSSCORR_HIP_GLONASS_CA_DLL_PLL_TRACKING_DEV_H_
#define GNSSCORR_HIP_GLONASS_CA_DLL_PLL_TRACKING_DEV_H_

#include "hip_glonass_ca_dll_pll_tracking.h"
#include "tracking_block_base.h"
#include <cstring>

namespace gnsscorr
{
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

inline GlonassTrkConf glonass_trk_conf(int band, int64_t fs_in, uint32_t vector_length, float pll_bw_hz, float dll_bw_hz, float early_late_space_chips, int cn0_samples, int cn0_min,
    int max_lock_fail, double carrier_lock_th)
{
    GlonassTrkConf c;
    c.band = band;
    c.fs_in = fs_in;
    c.vector_length = vector_length;
    c.pll_bw_hz = pll_bw_hz;
    c.dll_bw_hz = dll_bw_hz;
    c.early_late_space_chips = early_late_space_chips;
    c.cn0_samples = cn0_samples;
    c.cn0_min = cn0_min;
    c.max_lock_fail = max_lock_fail;
    c.carrier_lock_th = carrier_lock_th;
    return c;
}
}  // namespace gnsscorr

class hip_glonass_ca_dll_pll_tracking_dev : public hip_device_loop_block
{
public:
    /*! ring_periods: code periods of input the HBM ring holds (a work() call may bring at most that many) */
    explicit hip_glonass_ca_dll_pll_tracking_dev(const gnsscorr::GlonassTrkConf& conf, int device = 0, int ring_periods = 64)
        : hip_device_loop_block(gnsscorr::kGlonassLoopPolicy, conf.vector_length, gnsscorr::kGlonassCaCodeLengthChips, device, ring_periods), d_conf(conf), d_glonass_prn(gnsscorr::glonass_default_channels())
    {
    }
    //! the host-loop block's argument list
    hip_glonass_ca_dll_pll_tracking_dev(int band, int64_t fs_in, uint32_t vector_length, float pll_bw_hz, float dll_bw_hz, float early_late_space_chips, int cn0_samples = 20,
        int cn0_min = 25, int max_lock_fail = 50, double carrier_lock_th = 0.85, int device = 0, int ring_periods = 64)
        : hip_glonass_ca_dll_pll_tracking_dev(gnsscorr::glonass_trk_conf(band, fs_in, vector_length, pll_bw_hz, dll_bw_hz, early_late_space_chips, cn0_samples, cn0_min, max_lock_fail, carrier_lock_th),
              device, ring_periods)
    {
    }

    //! the slot -> frequency channel map comes from the almanac in a live receiver
    void set_glonass_channel_map(const std::map<uint32_t, int32_t>& prn_to_channel) { d_glonass_prn = prn_to_channel; }

protected:
    //! start_tracking (:160-243) on the device
    gc_status start_channel(uint64_t sample_counter, Gnss_Synchro* pull_in) override
    {
        return gnsscorr::glonass_loop_start_channel(d_loop, 0, d_conf, d_glonass_prn, *d_acquisition_gnss_synchro, sample_counter, pull_in);
    }
    Gnss_Synchro to_synchro(const gc_loop_record& r) const override { return gnsscorr::glonass_synchro_from_record(r, *d_acquisition_gnss_synchro, d_conf.fs_in); }

private:
    gnsscorr::GlonassTrkConf d_conf;
    std::map<uint32_t, int32_t> d_glonass_prn;
};

//! TrackingInterface adapters on the device loop: the configuration keys of glonass_l1_ca_dll_pll_tracking.cc:46-130 ("2G": the same)
template <int BAND>
using GlonassCaDllPllTrackingDevHip = GlonassCaDllPllTrackingAdapter<BAND, hip_glonass_ca_dll_pll_tracking_dev>;
using GlonassL1CaDllPllTrackingDevHip = GlonassCaDllPllTrackingDevHip<1>;
using GlonassL2CaDllPllTrackingDevHip = GlonassCaDllPllTrackingDevHip<2>;

#endif  // GNSSCORR_HIP_GLONASS_CA_DLL_PLL_TRACKING_DEV_H_
