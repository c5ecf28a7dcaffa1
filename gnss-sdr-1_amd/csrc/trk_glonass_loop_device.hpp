// trk_glonass_loop_device.hpp -- the device side of the GLONASS L1 / L2 C/A closed loop (trk_closed_loop_glonass.hip): the
// per-channel state and, on one lane, the scalar maths of the reference's own GLONASS block
//   glonass_l1_ca_dll_pll_tracking_cc.cc   start_tracking :160-243, general_work :549-777
// (glonass_l2_ca_dll_pll_tracking_cc.cc is the same with the L2 carrier constants), followed statement by statement with the same
// double / float promotions as the host image adapter/hip_glonass_ca_dll_pll_tracking.h.  It is not the veml loop:
//   * second-order Tracking_2nd_PLL_filter / Tracking_2nd_DLL_filter (tracking_2nd_PLL_filter.cc:40-88, tracking_2nd_DLL_filter.cc:40-76);
//   * the FDMA channel offset is part of the carrier NCO (d_carrier_frequency_hz) and not of the Doppler (d_carrier_doppler_hz);
//   * the block length is round()-ed every period with the code NCO command folded in, and the period CORRELATES the length of the
//     previous update while it CONSUMES the new one (d_sample_counter += d_current_prn_length_samples runs after the update);
//   * the C/N0 window stores cn0_samples prompts, estimates on the period after the buffer filled and does not store that prompt.
// Deviation, explicit: the reference reads past the 2 * vector_length items its scheduler guarantees when a block length ever
// exceeds that.  Here a new block length outside [1, 2 * vector_length] ends tracking: the period's record is written as the block
// would (valid, with the offending length), the channel goes to state 0, counts a lost-lock event and consumes nothing.
// Second deviation: a start is the start of a FRESH block object.  The block's start_tracking leaves d_cn0_estimation_counter, the
// prompt buffer, d_CN0_SNV_dB_Hz and d_carrier_lock_test as the previous run of the same object left them, so a restarted block
// places its first C/N0 estimate by the old window's fill; here every start clears the window and reports C/N0 0 / lock test 1 until
// the first estimate, whatever the slot tracked before -- a slot is handed from satellite to satellite and carries nothing over.
// Compiled with -ffp-contract=off (csrc/Makefile): the filter and discriminator expressions round once per operation.
#pragma once
#include "trk_loop_device.hpp"

#define GLO_CODE_LENGTH 511
#define GLO_CODE_RATE_HZ 0.511e6   // GLONASS_L1_CA_CODE_RATE_HZ (L2 C/A: the same)
#define GLO_CODE_LENGTH_CHIPS 511.0

// per-channel persistent state (device memory between launches, LDS during one); a buffer of its own beside the veml LoopChan's
struct GloChan
{
    gc_glonass_loop_conf conf;
    TrkChan chan;       // iq, code table, taps
    int n_taps;         // 3: started; 0: standby slot
    int state;          // 0 standby, 1 pull-in pending, 2 tracking
    unsigned long long pos;             // stream index of the next unread sample
    unsigned long long sample_counter;  // d_sample_counter
    unsigned long long acq_sample_stamp;
    double glonass_freq_ch;             // band carrier + FDMA offset of the slot
    double acq_code_phase_samples, acq_carrier_doppler_hz;
    double code_freq_chips, code_phase_step_chips;
    double carrier_frequency_hz, carrier_doppler_hz;
    double carrier_phase_step_rad, carrier_doppler_phase_step_rad;
    double rem_code_phase_samples, rem_code_phase_chips, rem_carr_phase_rad, acc_carrier_phase_rad;
    int current_prn_length_samples;
    int cn0_estimation_counter, carrier_lock_fail_counter, lost_lock_events;
    double carrier_lock_test, cn0_db_hz;
    // Tracking_2nd_DLL_filter / Tracking_2nd_PLL_filter
    float dll_tau1, dll_tau2, dll_pdi, dll_old_nco, dll_old_error;
    float pll_tau1, pll_tau2, pll_pdi, pll_old_nco, pll_old_error;
    float2 prompt_buffer[LOOP_MAX_CN0];
};

#define GLO_HD __host__ __device__

// natural frequency from the noise bandwidth, then the two time constants (tracking_2nd_DLL_filter.cc:40-50)
static GLO_HD inline void glo_loop_coefficients(float* tau1, float* tau2, float lbw, float zeta, float k)
{
    const float Wn = lbw * 8.0 * zeta / (4.0 * zeta * zeta + 1.0);
    *tau1 = k / (Wn * Wn);
    *tau2 = 2.0 * zeta / Wn;
}

// get_code_nco / get_carrier_nco (tracking_2nd_DLL_filter.cc:66-76, tracking_2nd_PLL_filter.cc:78-88): float state, the
// integrator term in double
static GLO_HD inline float glo_filter_step(float tau1, float tau2, float pdi, float& old_nco, float& old_error, float discriminator)
{
    const float nco = old_nco + (tau2 / tau1) * (discriminator - old_error) + (discriminator + old_error) * (pdi / (2.0 * tau1));
    old_nco = nco;
    old_error = discriminator;
    return nco;
}

// start_tracking (:160-243): runs on the host (gc_trk_loop_start_glonass) before the state is uploaded.  s.conf is filled in.
static GLO_HD inline void glo_loop_start(GloChan& s)
{
    const gc_glonass_loop_conf& c = s.conf;
    const double fs_in = (double)(long long)c.fs_in;  // the block's d_fs_in is an int64_t
    s.acq_code_phase_samples = c.acq_delay_samples;
    s.acq_carrier_doppler_hz = c.acq_doppler_hz;
    s.acq_sample_stamp = c.acq_samplestamp_samples;
    s.sample_counter = c.sample_counter;
    const long long acq_trk_diff_samples = (long long)s.sample_counter - (long long)s.acq_sample_stamp;
    const double acq_trk_diff_seconds = (float)acq_trk_diff_samples / (float)(long long)c.fs_in;
    s.glonass_freq_ch = c.band_carrier_freq_hz + c.channel_offset_hz;
    // code-rate aiding from the acquisition Doppler, against the slot's own carrier
    const double radial_velocity = (s.glonass_freq_ch + s.acq_carrier_doppler_hz) / s.glonass_freq_ch;
    s.code_freq_chips = radial_velocity * GLO_CODE_RATE_HZ;
    s.code_phase_step_chips = s.code_freq_chips / fs_in;
    const double T_prn_mod_seconds = (1 / s.code_freq_chips) * GLO_CODE_LENGTH_CHIPS;
    const double T_prn_mod_samples = T_prn_mod_seconds * fs_in;
    s.current_prn_length_samples = (int)round(T_prn_mod_samples);
    // code phase drift between the acquisition stamp and now
    const double T_prn_true_seconds = GLO_CODE_LENGTH_CHIPS / GLO_CODE_RATE_HZ;
    const double T_prn_true_samples = T_prn_true_seconds * fs_in;
    const double N_prn_diff = acq_trk_diff_seconds / T_prn_true_seconds;
    double corrected = fmod(s.acq_code_phase_samples + (T_prn_true_seconds - T_prn_mod_seconds) * N_prn_diff * fs_in, T_prn_true_samples);
    if (corrected < 0) corrected = T_prn_mod_samples + corrected;
    s.acq_code_phase_samples = corrected;
    // the carrier NCO carries the FDMA offset, the Doppler bookkeeping does not
    s.carrier_frequency_hz = s.acq_carrier_doppler_hz + c.channel_offset_hz;
    s.carrier_doppler_hz = s.acq_carrier_doppler_hz;
    s.carrier_phase_step_rad = LOOP_PI_2 * s.carrier_frequency_hz / fs_in;
    s.carrier_doppler_phase_step_rad = LOOP_PI_2 * s.carrier_doppler_hz / fs_in;
    glo_loop_coefficients(&s.dll_tau1, &s.dll_tau2, c.dll_bw_hz, 0.7f, 1.0f);
    glo_loop_coefficients(&s.pll_tau1, &s.pll_tau2, c.pll_bw_hz, 0.7f, 0.25f);
    s.dll_pdi = s.pll_pdi = 0.001f;
    s.dll_old_nco = s.dll_old_error = s.pll_old_nco = s.pll_old_error = 0.0f;
    s.carrier_lock_fail_counter = 0;
    s.rem_code_phase_samples = 0.0;
    s.rem_carr_phase_rad = 0.0;
    s.rem_code_phase_chips = 0.0;
    s.acc_carrier_phase_rad = 0.0;
    s.cn0_estimation_counter = 0;
    s.carrier_lock_test = 1.0;
    s.cn0_db_hz = 0.0;
    s.lost_lock_events = 0;
    s.state = 1;
}

// The pull-in alignment (:570-590; state 1 -> 2): skips samples_offset samples so that the next block starts on a code period.  The
// kernel runs it before a channel's first period; gc_glonass_loop_pull_in runs the same statements on the host for the item the
// block writes at that point.  Returns samples_offset.
static GLO_HD inline int glo_loop_pull_in(GloChan& s)
{
    const int acq_to_trk_delay_samples = (int)(s.sample_counter - s.acq_sample_stamp);
    const double shift_correction = (float)s.current_prn_length_samples - fmodf((float)acq_to_trk_delay_samples, (float)s.current_prn_length_samples);
    const int samples_offset = (int)round(s.acq_code_phase_samples + shift_correction);
    s.sample_counter = s.sample_counter + (unsigned long long)(long long)samples_offset;
    s.pos = s.pos + (unsigned long long)(long long)samples_offset;
    s.acc_carrier_phase_rad -= s.carrier_doppler_phase_step_rad * samples_offset;
    s.state = 2;
    return samples_offset;
}

// What general_work does before the correlation of a period, by one lane: the pull-in alignment (no record), the decision whether
// the whole block lies below `limit`, and the correlator's scalars narrowed to float where
// Hip_Multicorrelator::Carrier_wipeoff_multicorrelator_resampler (5 arguments: no rate terms) narrows them.  Returns 0 (and writes
// the period's invalid record) when there is nothing to correlate: standby, or the input is exhausted.
static __device__ __forceinline__ int glo_loop_prepare(GloChan& s, unsigned long long limit, gc_epoch_params& s_p, gc_loop_record* rec)
{
    if (s.state == 1) glo_loop_pull_in(s);
    const unsigned long long n = (unsigned long long)s.current_prn_length_samples;
    const int go = s.state == 2 && s.pos + n <= limit && s.pos + n >= s.pos;
    if (go)
        {
            const float rem_carr = (float)s.rem_carr_phase_rad;
            const float pstep = (float)s.carrier_phase_step_rad;
            s_p.sample_offset = s.pos;
            s_p.phase0_re = cosf(rem_carr);
            s_p.phase0_im = -sinf(rem_carr);
            s_p.phase_inc_re = cosf(pstep);
            s_p.phase_inc_im = -sinf(pstep);
            s_p.phase_rate_re = 1.0f;
            s_p.phase_rate_im = -0.0f;
            s_p.rem_code_phase_chips = (float)s.rem_code_phase_chips;
            s_p.code_phase_step_chips = (float)s.code_phase_step_chips;
            s_p.code_phase_rate_step_chips = 0.0f;
            s_p.n_samples = s.current_prn_length_samples;
        }
    else
        loop_invalid_record(rec, s.state, s.sample_counter);
    return go;
}

// everything general_work does with one period's correlator outputs E, P, L (:592-777)
static __device__ __forceinline__ void glo_loop_after_correlation(GloChan& s, const float2* taps, gc_loop_record* rec)
{
    const gc_glonass_loop_conf& c = s.conf;
    const double fs_in = (double)(long long)c.fs_in;
    const float2 E = taps[0], P = taps[1], L = taps[2];
    {
        unsigned* w = reinterpret_cast<unsigned*>(rec);
        for (unsigned i = 0; i < sizeof(gc_loop_record) / 4; i++) w[i] = 0u;
    }
    // PLL: two-quadrant arctan, in cycles
    const double carr_error_hz = ((P.x != 0.0f) ? (double)atanf(P.y / P.x) : 0.0) / LOOP_PI_2;
    const double carr_error_filt_hz = glo_filter_step(s.pll_tau1, s.pll_tau2, s.pll_pdi, s.pll_old_nco, s.pll_old_error, (float)carr_error_hz);
    s.carrier_frequency_hz += carr_error_filt_hz;
    s.carrier_doppler_hz += carr_error_filt_hz;
    s.code_freq_chips = GLO_CODE_RATE_HZ + ((s.carrier_doppler_hz * GLO_CODE_RATE_HZ) / s.glonass_freq_ch);
    // DLL: the filtered code error becomes a time shift of the next block
    const double pe = cabs_d(E), pl = cabs_d(L);
    const double code_error_chips = (pe + pl == 0.0) ? 0.0 : 0.5 * (pe - pl) / (pe + pl);
    const double code_error_filt_chips = glo_filter_step(s.dll_tau1, s.dll_tau2, s.dll_pdi, s.dll_old_nco, s.dll_old_error, (float)code_error_chips);
    const double T_chip_seconds = 1.0 / s.code_freq_chips;
    const double T_prn_seconds = T_chip_seconds * GLO_CODE_LENGTH_CHIPS;
    const double code_error_filt_secs = (T_prn_seconds * code_error_filt_chips * T_chip_seconds);
    const double T_prn_samples = T_prn_seconds * fs_in;
    const double K_blk_samples = T_prn_samples + s.rem_code_phase_samples + code_error_filt_secs * fs_in;
    const double rounded = round(K_blk_samples);
    // (a length no int32 holds is out of range whatever its value)
    const int new_length = rounded >= -2147483648.0 && rounded <= 2147483647.0 ? (int)rounded : -1;
    s.current_prn_length_samples = new_length;
    // NCO commands for the next block
    s.carrier_doppler_phase_step_rad = LOOP_PI_2 * s.carrier_doppler_hz / fs_in;
    s.carrier_phase_step_rad = LOOP_PI_2 * s.carrier_frequency_hz / fs_in;
    s.rem_carr_phase_rad = s.rem_carr_phase_rad + s.carrier_phase_step_rad * new_length;
    s.rem_carr_phase_rad = fmod(s.rem_carr_phase_rad, LOOP_PI_2);
    s.acc_carrier_phase_rad -= s.carrier_doppler_phase_step_rad * new_length;
    s.code_phase_step_chips = s.code_freq_chips / fs_in;
    s.rem_code_phase_samples = K_blk_samples - new_length;
    s.rem_code_phase_chips = s.code_freq_chips * (s.rem_code_phase_samples / fs_in);
    // C/N0 and lock detector
    if (s.cn0_estimation_counter < c.cn0_samples)
        {
            s.prompt_buffer[s.cn0_estimation_counter] = P;
            s.cn0_estimation_counter++;
        }
    else
        {
            s.cn0_estimation_counter = 0;
            s.cn0_db_hz = (double)loop_cn0_svn_estimator(s.prompt_buffer, c.cn0_samples, 0.001);
            s.carrier_lock_test = (double)loop_carrier_lock_detector(s.prompt_buffer, c.cn0_samples);
            if (s.carrier_lock_test < c.carrier_lock_th || s.cn0_db_hz < c.cn0_min)
                s.carrier_lock_fail_counter++;
            else if (s.carrier_lock_fail_counter > 0)
                s.carrier_lock_fail_counter--;
            if (s.carrier_lock_fail_counter > c.max_lock_fail)
                {
                    s.lost_lock_events++;  // message 3 on the "events" port
                    s.carrier_lock_fail_counter = 0;
                    s.state = 0;
                }
        }
    unsigned long long consumed = (unsigned long long)(long long)new_length;
    if (new_length < 1 || (unsigned)new_length > 2u * c.vector_length)
        {
            // the explicit deviation (see the top of this file)
            if (s.state != 0) s.lost_lock_events++;
            s.state = 0;
            consumed = 0;
        }
    s.sample_counter += consumed;
    s.pos += consumed;
    for (int t = 0; t < 3; t++)
        {
            rec->corr[2 * t] = rec->accu[2 * t] = taps[t].x;
            rec->corr[2 * t + 1] = rec->accu[2 * t + 1] = taps[t].y;
        }
    rec->prompt_data[0] = P.x;
    rec->prompt_data[1] = P.y;
    rec->sample_counter = s.sample_counter;
    rec->acc_carrier_phase_rad = s.acc_carrier_phase_rad;
    rec->rem_code_phase_samples = s.rem_code_phase_samples;
    rec->carrier_doppler_hz = (float)s.carrier_doppler_hz;
    rec->code_freq_chips = (float)s.code_freq_chips;
    rec->carr_phase_error_hz = (float)carr_error_hz;
    rec->carr_error_filt_hz = (float)carr_error_filt_hz;
    rec->code_error_chips = (float)code_error_chips;
    rec->code_error_filt_chips = (float)code_error_filt_chips;
    rec->cn0_db_hz = (float)s.cn0_db_hz;
    rec->carrier_lock_test = (float)s.carrier_lock_test;
    rec->state = s.state;
    rec->valid = 1;
    rec->current_prn_length_samples = new_length;
}

// the GLONASS loop as loop_periods takes it: E / P / L on the real replica, no data component, no rate terms
struct GloLoopKind
{
    using State = GloChan;
    static constexpr int NTAPS = 3;
    static constexpr bool DATA = false, HD = false;
    static __device__ __forceinline__ int prepare(GloChan& s, unsigned long long limit, gc_epoch_params& s_p, gc_loop_record* rec) { return glo_loop_prepare(s, limit, s_p, rec); }
    static __device__ __forceinline__ void after_correlation(GloChan& s, const float2* taps, gc_loop_record* rec) { glo_loop_after_correlation(s, taps, rec); }
};

// the GLONASS kernel's launch (trk_closed_loop_glonass.hip)
hipError_t glo_loop_launch(const LoopLaunch& a, int iq_format);
