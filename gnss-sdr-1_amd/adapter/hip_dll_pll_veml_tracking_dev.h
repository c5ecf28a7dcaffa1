/*!
 * \file hip_dll_pll_veml_tracking_dev.h
 * \brief The dll_pll_veml_tracking block on the DEVICE loop (gc_trk_loop): one work() call pushes the new input items into an
 * HBM ring and runs every code period that is complete in it -- correlations, synchronisation, extended integration and loop
 * maths in one launch -- then hands out one Gnss_Synchro per valid period (hip_device_loop_block, tracking_block_base.h, under the
 * veml policy; this header holds what a start and a record mean for the veml loop).  GNU Radio's general_work may produce several
 * output items per call (noutput_items), so the block keeps the reference interface while the per-millisecond host round trip
 * of the CPU block (and of hip_dll_pll_veml_tracking, which calls the level-1 correlator once per period) disappears.
 *
 * Same configuration (Dll_Pll_Conf), same signals and the same per-period results as hip_dll_pll_veml_tracking /
 * dll_pll_veml_tracking (src/algorithms/tracking/gnuradio_blocks/dll_pll_veml_tracking.cc); the state machine itself lives in
 * trk_closed_loop.hip.
 */
#ifndef GNSSCORR_HIP_DLL_PLL_VEML_TRACKING_DEV_H_
#define GNSSCORR_HIP_DLL_PLL_VEML_TRACKING_DEV_H_

#include "gnss_sdr_types.h"
#include "tracking_block_base.h"
#include "tracking_loop_maths.h"
#include "tracking_signals.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace gnsscorr
{
/*! start_tracking (:549-747) of one channel of a device loop: replicas, synchronisation data, loop start.  `sample_counter` is the
 *  stream position the channel starts consuming at (the block's d_sample_counter). */
inline gc_status loop_start_channel(gc_trk_loop* loop, int ch, const Dll_Pll_Conf& trk_parameters, const TrkSignalInfo& sig, const Gnss_Synchro& acq,
    uint64_t sample_counter, float bit_sync_min_time_s = 10.0f)
{
    const uint32_t prn = acq.PRN;
    const int code_len = static_cast<int>(sig.code_length_chips * sig.code_samples_per_chip);
    std::vector<float> code(code_len), data_code(code_len);
    const bool pilot = trk_parameters.track_pilot && sig.has_pilot;
    // the replica the loop runs on, and the data component's when the loop runs on the pilot (:566-705)
    gc_status st = trk_generate_replicas(sig.system, sig.signal, prn, pilot, code.data(), data_code.data());
    if (st != GC_OK) return st;
    gc_loop_sync_conf y;
    st = gc_loop_sync_for_signal(trk_parameters.system, trk_parameters.signal, prn, pilot ? 1 : 0, std::max(1, trk_parameters.extend_correlation_symbols), &y);
    if (st != GC_OK) return st;
    y.bit_sync_min_time_s = bit_sync_min_time_s;
    y.pll_bw_narrow_hz = trk_parameters.pll_bw_narrow_hz;
    y.dll_bw_narrow_hz = trk_parameters.dll_bw_narrow_hz;
    y.early_late_space_narrow_chips = trk_parameters.early_late_space_narrow_chips;
    y.very_early_late_space_narrow_chips = trk_parameters.very_early_late_space_narrow_chips;
    st = gc_trk_loop_set_sync(loop, ch, &y, pilot ? data_code.data() : nullptr, code_len);
    if (st != GC_OK) return st;
    gc_loop_conf c;
    std::memset(&c, 0, sizeof c);
    c.fs_in = trk_parameters.fs_in;
    c.signal_carrier_freq_hz = sig.carrier_freq_hz;
    c.code_chip_rate_hz = sig.code_chip_rate_hz;
    c.code_period_s = sig.code_period_s;
    c.carrier_lock_th = trk_parameters.carrier_lock_th;
    c.acq_delay_samples = acq.Acq_delay_samples;
    c.acq_doppler_hz = acq.Acq_doppler_hz;
    c.acq_samplestamp_samples = acq.Acq_samplestamp_samples;
    c.sample_counter = sample_counter;
    c.code_length_chips = sig.code_length_chips;
    c.code_samples_per_chip = sig.code_samples_per_chip;
    c.vector_length = trk_parameters.vector_length;
    c.pull_in_time_s = trk_parameters.pull_in_time_s;
    c.veml = sig.veml ? 1 : 0;
    c.pll_filter_order = trk_parameters.pll_filter_order;
    c.dll_filter_order = trk_parameters.dll_filter_order;
    c.enable_fll_pull_in = trk_parameters.enable_fll_pull_in ? 1 : 0;
    c.enable_fll_steady_state = trk_parameters.enable_fll_steady_state ? 1 : 0;
    c.cn0_samples = trk_parameters.cn0_samples;
    c.cn0_min = trk_parameters.cn0_min;
    c.max_lock_fail = trk_parameters.max_lock_fail;
    c.pll_bw_hz = trk_parameters.pll_bw_hz;
    c.dll_bw_hz = trk_parameters.dll_bw_hz;
    c.fll_bw_hz = trk_parameters.fll_bw_hz;
    c.early_late_space_chips = trk_parameters.early_late_space_chips;
    c.very_early_late_space_chips = trk_parameters.very_early_late_space_chips;
    c.high_dyn_smoother_length = trk_parameters.high_dyn ? std::min(16u, std::max(1u, trk_parameters.smoother_length)) : 0u;
    return gc_trk_loop_start(loop, ch, &c, code.data(), code_len);
}

//! what a valid period hands to the telemetry decoder (:1693-1725, :1898-1906), from the device loop's record
inline Gnss_Synchro synchro_from_record(const gc_loop_record& r, const Gnss_Synchro& acq, const TrkSignalInfo& sig, bool interchange_iq, double fs_in)
{
    Gnss_Synchro s = acq;
    s.Prompt_I = static_cast<double>(interchange_iq ? r.prompt_data[1] : r.prompt_data[0]);
    s.Prompt_Q = static_cast<double>(interchange_iq ? r.prompt_data[0] : r.prompt_data[1]);
    s.Code_phase_samples = r.rem_code_phase_samples;
    s.Carrier_phase_rads = r.acc_carrier_phase_rad;
    s.Carrier_Doppler_hz = r.carrier_doppler_hz;
    s.CN0_dB_hz = r.cn0_db_hz;
    s.correlation_length_ms = sig.correlation_length_ms;
    s.Flag_valid_symbol_output = true;
    s.fs = static_cast<int64_t>(fs_in);
    s.Tracking_sample_counter = r.sample_counter;
    return s;
}
}  // namespace gnsscorr

//! one channel with a ring of its own: hip_device_loop_block under the veml policy
class hip_dll_pll_veml_tracking_dev : public hip_device_loop_block
{
public:
    /*! ring_periods: code periods of input the HBM ring holds (a work() call may bring at most that many) */
    explicit hip_dll_pll_veml_tracking_dev(const Dll_Pll_Conf& conf_, int device = 0, int ring_periods = 64)
        : hip_dll_pll_veml_tracking_dev(conf_, gnsscorr::trk_signal_find(conf_.system, std::string(conf_.signal)), device, ring_periods)
    {
    }

    //! the reference waits 10 s before looking for the telemetry preamble (:1648); tests shorten it
    void set_bit_sync_min_time_s(float t) { d_bit_sync_min_time_s = t; }

protected:
    //! start_tracking (:549-747): replicas, synchronisation data and the loop start on the device
    gc_status start_channel(uint64_t sample_counter, Gnss_Synchro*) override
    {
        return gnsscorr::loop_start_channel(d_loop, 0, trk_parameters, *d_sig, *d_acquisition_gnss_synchro, sample_counter, d_bit_sync_min_time_s);
    }
    Gnss_Synchro to_synchro(const gc_loop_record& r) const override
    {
        return gnsscorr::synchro_from_record(r, *d_acquisition_gnss_synchro, *d_sig, trk_parameters.track_pilot && d_sig->interchange_iq_with_pilot, trk_parameters.fs_in);
    }

private:
    //! sig == NULL (not a signal of the block): nothing is created, last_status() is GC_ERR_INVALID and start_tracking does nothing
    hip_dll_pll_veml_tracking_dev(const Dll_Pll_Conf& conf_, const gnsscorr::TrkSignalInfo* sig, int device, int ring_periods)
        : hip_device_loop_block(gnsscorr::kVemlLoopPolicy, conf_.vector_length, sig ? static_cast<int>(sig->code_length_chips * sig->code_samples_per_chip) : 0, device, ring_periods,
              sig ? GC_OK : GC_ERR_INVALID),
          trk_parameters(conf_), d_sig(sig)
    {
        if (d_sig == nullptr) return;
        if (!d_sig->has_pilot) trk_parameters.track_pilot = false;
        if (trk_parameters.extend_correlation_symbols < 1) trk_parameters.extend_correlation_symbols = 1;
    }

    Dll_Pll_Conf trk_parameters;
    const gnsscorr::TrkSignalInfo* d_sig;
    float d_bit_sync_min_time_s = 10.0f;
};

#endif  // GNSSCORR_HIP_DLL_PLL_VEML_TRACKING_DEV_H_
