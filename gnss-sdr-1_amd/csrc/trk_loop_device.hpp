// trk_loop_device.hpp -- the device side of the closed-loop tracking engine (trk_closed_loop.hip): the per-channel state, the
// loop maths of general_work on one lane, and what the persistent kernel (trk_closed_loop.hip), the mixed kernel
// (trk_closed_loop_mixed.hip) and the GLONASS kernel (trk_closed_loop_glonass.hip) share: the channel shell, the period loop over a
// loop kind, and the launch.
#pragma once
#include <type_traits>
#include "gc_internal.h"
#include "trk_device.hpp"
#include "trk_loop_plan.h"

#define LOOP_MAX_CN0 64
#ifndef LOOP_NT
#define LOOP_NT 0  // nontemporal IQ loads: off -- the channels of a launch re-read one RF stream from the caches, period after period
#endif
#ifndef LOOP_WHOLE
#define LOOP_WHOLE 0  // ragged first / last chunks fetched whole where they lie inside the buffer (trk_device.hpp): off -- a lone
                      // workgroup per channel on cache-resident samples gains nothing from it and pays for the masks (0.713 vs 0.689 ms for
                      // 256 channels x 64 periods)
#endif
#ifndef LOOP_ALIGN_PAIRS
#define LOOP_ALIGN_PAIRS 1  // chunk grid of a window: the 16-byte one (the batched kernel's 128-byte grid makes nearly every period start with
                            // a ragged chunk: 0.710 vs 0.689 ms)
#endif
#define LOOP_MAX_SMOOTHER 16
#define LOOP_PI_2 6.283185307179586

// code loop filter without the last integrator (the block constructs it with include_last_integrator = false)
struct DevLoopFilter
{
    float b[4], a[3];
    int nb, na;
    float in[4], out[4];
    int idx;
};

struct DevPll
{
    int order;
    float w, x, a2, a3, b3, w0p, w0p2, w0p3, w0f, w0f2;
};

// gc_loop_sync_conf in device form: the bit patterns are stored newest-symbol-first (bit k = k-th newest symbol), the
// order of the sign shift register they are compared with
struct LoopSync
{
    int extend_symbols, track_pilot, symbols_per_bit, secondary_len, preamble_len;
    float bit_sync_min_time_s, pll_bw_narrow_hz, dll_bw_narrow_hz, el_narrow_chips, vel_narrow_chips;
    unsigned sec_ones[4];   // bit k set: secondary_code[len-1-k] == '1'
    unsigned pre_plus[6];   // bit k set: preamble_symbols[len-1-k] == +1
};

// per-channel persistent state (device memory between launches, LDS during one)
struct LoopChan
{
    gc_loop_conf conf;
    LoopSync sync;
    unsigned hist[6];       // signs of the last prompts, newest in bit 0 (1 = negative real part): d_Prompt_circular_buffer /
                            // d_symbol_history, of which only the signs are ever read
    int hist_count;
    float2 accu[5];         // d_VE_accu, d_E_accu, d_P_accu, d_L_accu, d_VL_accu
    float2 prompt_data;     // d_Prompt_Data
    int current_symbol, extend_count;
    // high dynamics (:1016-1033, :1047-1064): histories of (NCO step, block length), newest last, 2 * smoother_length deep
    double carr_hist[2 * LOOP_MAX_SMOOTHER][2], code_hist[2 * LOOP_MAX_SMOOTHER][2];
    int carr_hist_n, code_hist_n;
    double carrier_phase_rate_step_rad, code_phase_rate_step_chips;
    TrkChan chan;       // iq, code table, taps
    int n_taps;
    int state;          // 0 standby, 1 pull-in, 2 tracking
    int cloop, pull_in_transitory;
    unsigned long long pos;             // stream index of the next unread sample
    unsigned long long sample_counter;  // d_sample_counter
    unsigned long long acq_sample_stamp;
    double acq_code_phase_samples, acq_carrier_doppler_hz;
    double carrier_doppler_hz, code_freq_chips;
    double carrier_phase_step_rad, code_phase_step_chips;
    double rem_code_phase_samples, rem_code_phase_chips, acc_carrier_phase_rad;
    float rem_carr_phase_rad;
    int current_prn_length_samples;
    double current_correlation_time_s;
    double carr_phase_error_hz, carr_freq_error_hz, carr_error_filt_hz, code_error_chips, code_error_filt_chips;
    float2 P_accu_old;
    DevLoopFilter dll;
    DevPll pll;
    float2 prompt_buffer[LOOP_MAX_CN0];
    int cn0_estimation_counter, carrier_lock_fail_counter;
    double carrier_lock_test, cn0_db_hz;
    int lost_lock_events;
};

// ---- loop filter design: tracking_loop_filter.cc:104-245 (include_last_integrator == false) ----
static __device__ __forceinline__ void dll_design(DevLoopFilter& f, int order, float bw, float T)
{
    const float zeta = 1.0 / sqrt(2.0);
    float g1, g2, g3, wn;
    f.nb = f.na = 0;
    switch (order)
        {
        case 1:
            wn = bw * 4.0;
            g1 = wn;
            f.b[0] = g1;
            f.nb = 1;
            break;
        case 3:
            {
                wn = bw / 0.7845;
                const float a3 = 1.1, b3 = 2.4;
                g1 = wn * wn * wn;
                g2 = a3 * wn * wn;
                g3 = b3 * wn;
                f.b[0] = g3 + T / 2.0 * (g2 + T / 2.0 * g1);
                f.b[1] = g1 * T * T / 2.0 - 2.0 * g3;
                f.b[2] = g3 + T / 2.0 * (-g2 + T / 2.0 * g1);
                f.nb = 3;
                f.a[0] = 2.0f;
                f.a[1] = -1.0f;
                f.na = 2;
                break;
            }
        default:
            wn = bw * (8.0 * zeta) / (4.0 * zeta * zeta + 1.0);
            g1 = wn * wn;
            g2 = wn * 2.0 * zeta;
            f.b[0] = (g1 * T / 2.0 + g2);
            f.b[1] = g1 * T / 2.0 - g2;
            f.nb = 2;
            f.a[0] = 1.0f;
            f.na = 1;
            break;
        }
}

static __device__ __forceinline__ void dll_initialize(DevLoopFilter& f)
{
    for (int i = 0; i < 4; i++) f.in[i] = f.out[i] = 0.0f;
    f.idx = 3;
}

static __device__ __forceinline__ float dll_apply(DevLoopFilter& f, float v)
{
    float result = 0.0f;
    for (int i = 0; i < f.na; ++i) result += f.a[i] * f.out[(f.idx + i) % 4];
    f.idx--;
    if (f.idx < 0) f.idx += 4;
    f.in[f.idx] = v;
    for (int i = 0; i < f.nb; ++i) result += f.b[i] * f.in[(f.idx + i) % 4];
    f.out[f.idx] = result;
    return result;
}

// ---- carrier loop filter: tracking_FLL_PLL_filter.cc:55-133 ----
static __device__ __forceinline__ void pll_set_params(DevPll& p, float fll_bw_hz, float pll_bw_hz, int order)
{
    p.order = order;
    p.w = p.x = p.a3 = p.b3 = p.w0p3 = p.w0f2 = 0.0f;
    if (order == 3)
        {
            p.b3 = 2.400f;
            p.a3 = 1.100f;
            p.a2 = 1.414f;
            p.w0p = pll_bw_hz / 0.7845;
            p.w0p2 = p.w0p * p.w0p;
            p.w0p3 = p.w0p2 * p.w0p;
            p.w0f = fll_bw_hz / 0.53;
            p.w0f2 = p.w0f * p.w0f;
        }
    else
        {
            p.a2 = 1.414f;
            p.w0p = pll_bw_hz / 0.53;
            p.w0p2 = p.w0p * p.w0p;
            p.w0f = fll_bw_hz / 0.25;
        }
}

// set_params on a running filter (:1754): new coefficients, integrators untouched
static __device__ __forceinline__ void pll_retune(DevPll& p, float fll_bw_hz, float pll_bw_hz, int order)
{
    const float w = p.w, x = p.x;
    pll_set_params(p, fll_bw_hz, pll_bw_hz, order);
    p.w = w;
    p.x = x;
}

static __device__ __forceinline__ float pll_get_carrier_error(DevPll& p, float fll, float pll, float T)
{
    float carrier_error_hz;
    if (p.order == 3)
        {
            p.w = p.w + T * (p.w0p3 * pll + p.w0f2 * fll);
            p.x = p.x + T * (0.5 * p.w + p.a2 * p.w0f * fll + p.a3 * p.w0p2 * pll);
            carrier_error_hz = 0.5 * p.x + p.b3 * p.w0p * pll;
        }
    else
        {
            const float w_new = p.w + pll * p.w0p2 * T + fll * p.w0f * T;
            carrier_error_hz = 0.5 * (w_new + p.w) + p.a2 * p.w0p * pll;
            p.w = w_new;
        }
    return carrier_error_hz;
}

static __device__ double cabs_d(float2 v) { return (double)hypotf(v.x, v.y); }  // std::abs(gr_complex) is float hypot

// start_tracking (dll_pll_veml_tracking.cc:549-747), loop part
static __device__ void loop_start(LoopChan& s)
{
    const gc_loop_conf& c = s.conf;
    s.acq_code_phase_samples = c.acq_delay_samples;
    s.acq_carrier_doppler_hz = c.acq_doppler_hz;
    s.acq_sample_stamp = c.acq_samplestamp_samples;
    s.sample_counter = c.sample_counter;
    s.carrier_doppler_hz = s.acq_carrier_doppler_hz;
    s.carrier_phase_step_rad = LOOP_PI_2 * s.carrier_doppler_hz / c.fs_in;
    pll_set_params(s.pll, c.fll_bw_hz, c.pll_bw_hz, c.pll_filter_order);
    if (s.pll.order == 3)
        {
            s.pll.x = 2.0 * (float)s.acq_carrier_doppler_hz;
            s.pll.w = 0;
        }
    else
        {
            s.pll.w = (float)s.acq_carrier_doppler_hz;
            s.pll.x = 0;
        }
    dll_design(s.dll, c.dll_filter_order, c.dll_bw_hz, (float)c.code_period_s);
    dll_initialize(s.dll);
    s.carrier_lock_fail_counter = 0;
    s.rem_code_phase_samples = 0.0;
    s.rem_carr_phase_rad = 0.0f;
    s.rem_code_phase_chips = 0.0;
    s.acc_carrier_phase_rad = 0.0;
    s.cn0_estimation_counter = 0;
    s.carrier_lock_test = 1.0;
    s.cn0_db_hz = 0.0;
    s.current_correlation_time_s = c.code_period_s;
    s.code_freq_chips = c.code_chip_rate_hz;
    s.code_phase_step_chips = s.code_freq_chips / c.fs_in;
    s.current_prn_length_samples = (int)c.vector_length;
    s.P_accu_old = make_float2(0.f, 0.f);
    s.carr_phase_error_hz = s.carr_freq_error_hz = s.carr_error_filt_hz = s.code_error_chips = s.code_error_filt_chips = 0.0;
    s.state = 1;
    s.cloop = 1;
    s.pull_in_transitory = 1;
    s.lost_lock_events = 0;
    for (int t = 0; t < 5; t++) s.accu[t] = make_float2(0.f, 0.f);
    s.prompt_data = make_float2(0.f, 0.f);
    s.current_symbol = 0;
    s.extend_count = 0;
    s.hist_count = 0;
    for (int i = 0; i < 6; i++) s.hist[i] = 0u;
    s.carrier_phase_rate_step_rad = s.code_phase_rate_step_chips = 0.0;
    s.carr_hist_n = s.code_hist_n = 0;
}

// cn0_svn_estimator (lock_detectors.cc:71-90) over `length` prompts
static __device__ __forceinline__ float loop_cn0_svn_estimator(const float2* prompt_buffer, int length, double coh_integration_time_s)
{
    double Psig = 0.0, Ptot = 0.0;
    for (int i = 0; i < length; i++)
        {
            const float2 v = prompt_buffer[i];
            Psig += fabs((double)v.x);
            Ptot += (double)v.y * (double)v.y + (double)v.x * (double)v.x;
        }
    Psig /= (double)length;
    Psig = Psig * Psig;
    Ptot /= (double)length;
    const double SNR = Psig / (Ptot - Psig);
    return (float)(10.0 * log10(SNR) - 10.0 * log10(coh_integration_time_s));
}

// carrier_lock_detector (lock_detectors.cc:94-111)
static __device__ __forceinline__ float loop_carrier_lock_detector(const float2* prompt_buffer, int length)
{
    float sum_I = 0.f, sum_Q = 0.f;
    for (int i = 0; i < length; i++)
        {
            sum_I += prompt_buffer[i].x;
            sum_Q += prompt_buffer[i].y;
        }
    const float NBP = sum_I * sum_I + sum_Q * sum_Q, NBD = sum_I * sum_I - sum_Q * sum_Q;
    return NBD / NBP;
}

// cn0_and_tracking_lock_status (:839-878); false = loss of lock
static __device__ __forceinline__ bool loop_lock_status(LoopChan& s, double coh_integration_time_s)
{
    const gc_loop_conf& c = s.conf;
    if (s.cn0_estimation_counter < c.cn0_samples)
        {
            s.prompt_buffer[s.cn0_estimation_counter] = s.accu[2];
            s.cn0_estimation_counter++;
            return true;
        }
    s.cn0_estimation_counter = 0;
    s.cn0_db_hz = (double)loop_cn0_svn_estimator(s.prompt_buffer, c.cn0_samples, coh_integration_time_s);
    s.carrier_lock_test = (double)loop_carrier_lock_detector(s.prompt_buffer, c.cn0_samples);
    if (!s.pull_in_transitory)
        {
            if (s.carrier_lock_test < c.carrier_lock_th || s.cn0_db_hz < c.cn0_min)
                s.carrier_lock_fail_counter++;
            else if (s.carrier_lock_fail_counter > 0)
                s.carrier_lock_fail_counter--;
        }
    if (s.carrier_lock_fail_counter > c.max_lock_fail)
        {
            s.lost_lock_events++;  // message 3 on the "events" port
            s.carrier_lock_fail_counter = 0;
            return false;
        }
    return true;
}

// clear_tracking_vars (:976-995)
static __device__ __forceinline__ void loop_clear_tracking_vars(LoopChan& s)
{
    s.prompt_data = make_float2(0.f, 0.f);
    s.P_accu_old = make_float2(0.f, 0.f);
    s.carr_phase_error_hz = s.carr_freq_error_hz = s.carr_error_filt_hz = 0.0;
    s.code_error_chips = s.code_error_filt_chips = 0.0;
    s.current_symbol = 0;
    s.hist_count = 0;
    for (int i = 0; i < 6; i++) s.hist[i] = 0u;
    s.carrier_phase_rate_step_rad = s.code_phase_rate_step_chips = 0.0;
    s.carr_hist_n = s.code_hist_n = 0;
}

// run_dll_pll (:914-973) on the accumulators
static __device__ __forceinline__ void loop_run_dll_pll(LoopChan& s, bool veml)
{
    const gc_loop_conf& c = s.conf;
    const float2 VE = s.accu[0], E = s.accu[1], P = s.accu[2], L = s.accu[3], VL = s.accu[4];
    if (s.cloop)
        s.carr_phase_error_hz = ((P.x != 0.0f) ? (double)atanf(P.y / P.x) : 0.0) / LOOP_PI_2;
    else
        s.carr_phase_error_hz = (double)atan2f(P.y, P.x) / LOOP_PI_2;
    if ((s.pull_in_transitory && c.enable_fll_pull_in) || c.enable_fll_steady_state)
        {
            const double dot = s.P_accu_old.x * P.x + s.P_accu_old.y * P.y;
            const double cross = s.P_accu_old.x * P.y - P.x * s.P_accu_old.y;
            s.carr_freq_error_hz = atan2(cross, dot) / (s.current_correlation_time_s - 0.0) / LOOP_PI_2;
            s.P_accu_old = P;
            if (s.pull_in_transitory && c.enable_fll_pull_in)
                s.carr_error_filt_hz = pll_get_carrier_error(s.pll, (float)s.carr_freq_error_hz, 0.0f, (float)s.current_correlation_time_s);
            else
                s.carr_error_filt_hz = pll_get_carrier_error(s.pll, (float)s.carr_freq_error_hz, (float)s.carr_phase_error_hz, (float)s.current_correlation_time_s);
        }
    else
        s.carr_error_filt_hz = pll_get_carrier_error(s.pll, 0.0f, (float)s.carr_phase_error_hz, (float)s.current_correlation_time_s);
    s.carrier_doppler_hz = s.carr_error_filt_hz;
    if (veml)
        {
            // std::sqrt(std::norm(VE) + std::norm(E)) on gr_complex (tracking_discriminators.cc:121-122): a float sum and a float root
            const double pe = (double)sqrtf((VE.x * VE.x + VE.y * VE.y) + (E.x * E.x + E.y * E.y));
            const double pl = (double)sqrtf((VL.x * VL.x + VL.y * VL.y) + (L.x * L.x + L.y * L.y));
            s.code_error_chips = (pe + pl == 0.0) ? 0.0 : (pe - pl) / (pe + pl);
        }
    else
        {
            const double pe = cabs_d(E), pl = cabs_d(L);
            s.code_error_chips = (pe + pl == 0.0) ? 0.0 : 0.5 * (pe - pl) / (pe + pl);
        }
    s.code_error_filt_chips = dll_apply(s.dll, (float)s.code_error_chips);
    s.code_freq_chips = (1.0 + (s.carrier_doppler_hz / c.signal_carrier_freq_hz)) * c.code_chip_rate_hz - s.code_error_filt_chips;
}

// the rate smoother of both NCOs (:1016-1033, :1047-1064): once 2 * smoother_length (value, samples) pairs are held, the
// rate is (mean of the newer half - mean of the older half) / samples of the newer half
static __device__ __forceinline__ double loop_smoothed_rate(double (*hist)[2], int& count, int sl, double value, double samples, double current)
{
    const int cap = 2 * sl;
    if (count == cap)
        {
            for (int k = 1; k < cap; k++)
                {
                    hist[k - 1][0] = hist[k][0];
                    hist[k - 1][1] = hist[k][1];
                }
            count--;
        }
    hist[count][0] = value;
    hist[count][1] = samples;
    count++;
    if (count < cap) return current;
    double cp1 = 0.0, cp2 = 0.0, ns = 0.0;
    for (int k = 0; k < sl; k++)
        {
            cp1 += hist[k][0];
            cp2 += hist[cap - k - 1][0];
            ns += hist[cap - k - 1][1];
        }
    cp1 /= (double)sl;
    cp2 /= (double)sl;
    return (cp2 - cp1) / ns;
}

// update_tracking_vars (:998-1070)
static __device__ __forceinline__ void loop_update_tracking_vars(LoopChan& s)
{
    const gc_loop_conf& c = s.conf;
    const int sl = (int)c.high_dyn_smoother_length;
    const double T_prn_samples = (1.0 / s.code_freq_chips) * (double)c.code_length_chips * c.fs_in;
    const double K_blk_samples = T_prn_samples + s.rem_code_phase_samples;
    s.current_prn_length_samples = (int)floor(K_blk_samples);
    s.carrier_phase_step_rad = LOOP_PI_2 * s.carrier_doppler_hz / c.fs_in;
    const double n = (double)s.current_prn_length_samples;
    if (sl > 0) s.carrier_phase_rate_step_rad = loop_smoothed_rate(s.carr_hist, s.carr_hist_n, sl, s.carrier_phase_step_rad, n, s.carrier_phase_rate_step_rad);
    s.rem_carr_phase_rad += (float)(s.carrier_phase_step_rad * n + 0.5 * s.carrier_phase_rate_step_rad * n * n);
    s.rem_carr_phase_rad = fmodf(s.rem_carr_phase_rad, (float)LOOP_PI_2);
    s.acc_carrier_phase_rad -= (s.carrier_phase_step_rad * n + 0.5 * s.carrier_phase_rate_step_rad * n * n);
    s.code_phase_step_chips = s.code_freq_chips / c.fs_in;
    if (sl > 0) s.code_phase_rate_step_chips = loop_smoothed_rate(s.code_hist, s.code_hist_n, sl, s.code_phase_step_chips, n, s.code_phase_rate_step_chips);
    s.rem_code_phase_samples = K_blk_samples - n;
    s.rem_code_phase_chips = s.code_freq_chips * s.rem_code_phase_samples / c.fs_in;
}

// save_correlation_results (:1072-1125): accumulate with the secondary-code sign
static __device__ __forceinline__ void loop_save_correlation_results(LoopChan& s, const float2* taps, bool veml)
{
    const LoopSync& y = s.sync;
    float sign = 1.0f;
    if (y.secondary_len > 0)
        {
            // sec_ones is stored newest-first: character i of the string is bit (len - 1 - i)
            const int bit = y.secondary_len - 1 - s.current_symbol;
            if ((y.sec_ones[bit >> 5] >> (bit & 31)) & 1u) sign = -1.0f;
            s.current_symbol = (s.current_symbol + 1) % y.secondary_len;
        }
    else
        {
            s.current_symbol++;
            s.current_symbol = y.symbols_per_bit > 0 ? s.current_symbol % y.symbols_per_bit : 0;
        }
    for (int t = 0; t < 5; t++)
        {
            if (!veml && (t == 0 || t == 4)) continue;
            const float2 v = taps[veml ? t : t - 1];
            if (sign > 0.0f)
                {
                    s.accu[t].x += v.x;
                    s.accu[t].y += v.y;
                }
            else
                {
                    s.accu[t].x -= v.x;
                    s.accu[t].y -= v.y;
                }
        }
    s.cloop = y.track_pilot ? 0 : 1;
}

// pushes the sign of the prompt into the history; true when the last `len` signs match `pattern`
// (exactly == all bits equal; or, for the secondary code, all bits opposite as well)
static __device__ __forceinline__ bool loop_push_and_match(LoopChan& s, float prompt_re, int len, const unsigned* pattern, bool either_polarity)
{
    const unsigned neg = prompt_re < 0.0f ? 1u : 0u;
    for (int w = 5; w > 0; w--) s.hist[w] = (s.hist[w] << 1) | (s.hist[w - 1] >> 31);
    s.hist[0] = (s.hist[0] << 1) | neg;
    if (s.hist_count < len) s.hist_count++;
    if (s.hist_count < len) return false;
    int diff = 0;
    for (int w = 0; w * 32 < len; w++)
        {
            const int nb = min(32, len - w * 32);
            const unsigned mask = nb == 32 ? 0xffffffffu : ((1u << nb) - 1u);
            diff += __popc((s.hist[w] ^ pattern[w]) & mask);
        }
    return either_polarity ? (diff == 0 || diff == len) : diff == len;
}

static __device__ __forceinline__ void loop_write_record(const LoopChan& s, gc_loop_record* rec, int valid, int integrating, int extend_count)
{
    for (int t = 0; t < 5; t++)
        {
            rec->accu[2 * t] = s.accu[t].x;
            rec->accu[2 * t + 1] = s.accu[t].y;
        }
    rec->extend_count = extend_count;
    rec->integrating = integrating;
    rec->valid = valid;
}

// ---- the pieces every kernel of the engine is built from (State: LoopChan or GloChan) ----
// the workgroup's word-wise copy of one channel's state, global memory -> LDS or back
template <int THREADS, class State>
static __device__ __forceinline__ void loop_copy_state(State* to, const State* from)
{
    static_assert(sizeof(State) % 4 == 0, "the channel state is copied in 4-byte words");
    const int tid = threadIdx.x;
    const unsigned* src = reinterpret_cast<const unsigned*>(from);
    unsigned* dst = reinterpret_cast<unsigned*>(to);
    for (unsigned i = tid; i < sizeof(State) / 4; i += THREADS) dst[i] = src[i];
}

// a channel that has not been started (or was stopped): the workgroup writes all-zero records, standby
template <int THREADS>
static __device__ __forceinline__ void loop_standby_records(gc_loop_record* crec, int n_epochs)
{
    const int tid = threadIdx.x;
    for (int e = 0; e < n_epochs; e++)
        {
            unsigned* w = reinterpret_cast<unsigned*>(&crec[e]);
            for (unsigned i = tid; i < sizeof(gc_loop_record) / 4; i += THREADS) w[i] = 0u;
        }
}

// nothing to correlate: an invalid record marks the epoch, by one lane (records are written in place, field by field: no stack copies)
static __device__ __forceinline__ void loop_invalid_record(gc_loop_record* rec, int state, unsigned long long sample_counter)
{
    unsigned* w = reinterpret_cast<unsigned*>(rec);
    for (unsigned i = 0; i < sizeof(gc_loop_record) / 4; i++) w[i] = 0u;
    rec->state = state;
    rec->sample_counter = sample_counter;
}

// everything general_work does with one code period's correlator outputs (states 2, 3, 4; :1601-1896)
template <int NTAPS, bool DATA>
static __device__ __forceinline__ void loop_after_correlation(LoopChan& s, const float2* taps, gc_loop_record* rec)
{
    const gc_loop_conf& c = s.conf;
    const LoopSync& y = s.sync;
    const bool veml = NTAPS == 5;
    const float2 P = taps[NTAPS / 2];
    {
        unsigned* w = reinterpret_cast<unsigned*>(rec);
        for (unsigned i = 0; i < sizeof(gc_loop_record) / 4; i++) w[i] = 0u;
    }
    for (int t = 0; t < NTAPS; t++)
        {
            rec->corr[2 * t] = taps[t].x;
            rec->corr[2 * t + 1] = taps[t].y;
        }
    s.prompt_data = DATA ? taps[NTAPS] : P;
    const int ext = y.extend_symbols > 1 ? y.extend_symbols : 1;
    if (s.state == 2)
        {
            // single correlation step variables (:1604-1612)
            for (int t = 0; t < 5; t++) s.accu[t] = make_float2(0.f, 0.f);
            for (int t = 0; t < NTAPS; t++) s.accu[veml ? t : t + 1] = taps[t];
            if (!loop_lock_status(s, c.code_period_s))
                {
                    loop_clear_tracking_vars(s);
                    s.state = 0;
                    loop_write_record(s, rec, 0, 0, 0);
                }
            else
                {
                    loop_run_dll_pll(s, veml);
                    loop_update_tracking_vars(s);
                    loop_write_record(s, rec, 1, 0, s.extend_count);  // log_data(false), :1627
                    bool next_state;
                    if (y.secondary_len > 0)
                        {
                            // acquire_secondary (:800-836) over the last secondary_len prompts: '0' <-> positive prompt or the
                            // exact opposite.  A negative prompt on a '0' counts +1: sign bit == 1 and code bit == 0 differ.
                            next_state = loop_push_and_match(s, P.x, y.secondary_len, y.sec_ones, true);
                        }
                    else if (y.symbols_per_bit > 1)
                        {
                            // preamble search after bit_sync_min_time_s of tracking (:1645-1685)
                            next_state = false;
                            const float t_trk = (float)((double)(float)(s.sample_counter - s.acq_sample_stamp) / c.fs_in);
                            if (t_trk > y.bit_sync_min_time_s && y.preamble_len > 0)
                                {
                                    // corr == length  <=>  every symbol's clipped sign equals the preamble's: negative
                                    // (bit 1) where the preamble is -1 (pre_plus bit 0): all bits differ
                                    next_state = loop_push_and_match(s, P.x, y.preamble_len, y.pre_plus, false);
                                }
                        }
                    else
                        next_state = true;
                    if (next_state)
                        {
                            for (int t = 0; t < 5; t++) s.accu[t] = make_float2(0.f, 0.f);
                            s.hist_count = 0;
                            for (int i = 0; i < 6; i++) s.hist[i] = 0u;
                            s.current_symbol = 0;
                            if (ext > 1)
                                {
                                    s.extend_count = 0;
                                    s.current_correlation_time_s = (double)((float)ext * (float)c.code_period_s);
                                    s.state = 3;
                                    // narrow loop filters and taps (:1751-1766)
                                    dll_design(s.dll, c.dll_filter_order, y.dll_bw_narrow_hz, (float)s.current_correlation_time_s);
                                    pll_retune(s.pll, c.fll_bw_hz, y.pll_bw_narrow_hz, c.pll_filter_order);
                                    const float spc = (float)c.code_samples_per_chip;
                                    if (veml)
                                        {
                                            s.chan.shifts[0] = -y.vel_narrow_chips * spc;
                                            s.chan.shifts[1] = -y.el_narrow_chips * spc;
                                            s.chan.shifts[3] = y.el_narrow_chips * spc;
                                            s.chan.shifts[4] = y.vel_narrow_chips * spc;
                                        }
                                    else
                                        {
                                            s.chan.shifts[0] = -y.el_narrow_chips * spc;
                                            s.chan.shifts[2] = y.el_narrow_chips * spc;
                                        }
                                }
                            else
                                s.state = 4;
                        }
                }
        }
    else if (s.state == 3)
        {
            loop_update_tracking_vars(s);
            loop_save_correlation_results(s, taps, veml);
            s.extend_count++;
            if (s.extend_count == ext - 1)
                {
                    s.extend_count = 0;
                    s.state = 4;
                }
            loop_write_record(s, rec, 1, 1, s.extend_count);  // log_data(true), :1824
        }
    else  // state 4
        {
            loop_save_correlation_results(s, taps, veml);
            if (!loop_lock_status(s, c.code_period_s * (double)ext))
                {
                    loop_clear_tracking_vars(s);
                    s.state = 0;
                    loop_write_record(s, rec, 0, 0, 0);
                }
            else
                {
                    loop_run_dll_pll(s, veml);
                    loop_update_tracking_vars(s);
                    loop_write_record(s, rec, 1, 0, s.extend_count);  // log_data(false), :1880
                    for (int t = 0; t < 5; t++) s.accu[t] = make_float2(0.f, 0.f);
                    if (ext > 1) s.state = 3;
                }
        }
    s.sample_counter += (unsigned long long)s.current_prn_length_samples;
    s.pos += (unsigned long long)s.current_prn_length_samples;
    rec->prompt_data[0] = s.prompt_data.x;
    rec->prompt_data[1] = s.prompt_data.y;
    rec->sample_counter = s.sample_counter;
    rec->acc_carrier_phase_rad = s.acc_carrier_phase_rad;
    rec->rem_code_phase_samples = s.rem_code_phase_samples;
    rec->carrier_doppler_hz = (float)s.carrier_doppler_hz;
    rec->code_freq_chips = (float)s.code_freq_chips;
    rec->carr_phase_error_hz = (float)s.carr_phase_error_hz;
    rec->carr_error_filt_hz = (float)s.carr_error_filt_hz;
    rec->code_error_chips = (float)s.code_error_chips;
    rec->code_error_filt_chips = (float)s.code_error_filt_chips;
    rec->cn0_db_hz = (float)s.cn0_db_hz;
    rec->carrier_lock_test = (float)s.carrier_lock_test;
    rec->state = s.state;
    rec->current_prn_length_samples = s.current_prn_length_samples;
}

// What general_work does BEFORE the correlation of a code period (:1552-1600, :886-897), by one lane: end of the pull-in
// transitory, the pull-in sample skip (state 1 -> 2), the decision whether a whole block is available below `limit`, and the
// correlator's scalars narrowed to float exactly where do_correlation_step narrows them.  Returns 0 (and writes the period's
// invalid record) when there is nothing to correlate: standby, or the input is exhausted.
template <bool HD>
static __device__ __forceinline__ int loop_prepare(LoopChan& s, unsigned long long limit, gc_epoch_params& s_p, gc_loop_record* rec)
{
    const gc_loop_conf& c = s.conf;
    int go = 1;
    if (s.pull_in_transitory)
        {
            if (c.pull_in_time_s < (s.sample_counter - s.acq_sample_stamp) / (unsigned long long)(int)c.fs_in) s.pull_in_transitory = 0;
        }
    if (s.state == 1)
        {
            // pull-in (:1568-1600): skip samples until the incoming code is aligned with the replica
            const long long acq_trk_diff_samples = (long long)s.sample_counter - (long long)s.acq_sample_stamp;
            const double delta = (double)acq_trk_diff_samples - s.acq_code_phase_samples;
            s.code_freq_chips = c.code_chip_rate_hz;
            s.code_phase_step_chips = s.code_freq_chips / c.fs_in;
            const double T_prn_mod_samples = (1.0 / s.code_freq_chips) * (double)c.code_length_chips * c.fs_in;
            s.acq_code_phase_samples = T_prn_mod_samples - fmod(delta, T_prn_mod_samples);
            s.current_prn_length_samples = (int)round(T_prn_mod_samples);
            const int samples_offset = (int)round(s.acq_code_phase_samples);
            s.acc_carrier_phase_rad -= s.carrier_phase_step_rad * (double)samples_offset;
            s.state = 2;
            s.sample_counter += samples_offset;
            s.pos += samples_offset;
        }
    if (s.state < 2 || s.pos + c.vector_length > limit) go = 0;  // standby, or the input block is exhausted
    if (go)
        {
            // do_correlation_step (:886-897): the scalars are narrowed to float exactly there
            const float spc = (float)c.code_samples_per_chip;
            const float rem_carr = s.rem_carr_phase_rad;
            const float pstep = (float)s.carrier_phase_step_rad;
            s_p.sample_offset = s.pos;
            s_p.phase0_re = cosf(rem_carr);
            s_p.phase0_im = -sinf(rem_carr);
            s_p.phase_inc_re = cosf(pstep);
            s_p.phase_inc_im = -sinf(pstep);
            const float prate = HD ? (float)s.carrier_phase_rate_step_rad : 0.0f;
            s_p.phase_rate_re = cosf(prate);
            s_p.phase_rate_im = -sinf(prate);
            s_p.rem_code_phase_chips = (float)s.rem_code_phase_chips * spc;
            s_p.code_phase_step_chips = (float)s.code_phase_step_chips * spc;
            s_p.code_phase_rate_step_chips = HD ? (float)s.code_phase_rate_step_chips * spc : 0.0f;
            s_p.n_samples = (int)c.vector_length;
        }
    else
        loop_invalid_record(rec, s.state, s.sample_counter);
    return go;
}

// A kind of loop, as loop_periods takes it: the state type, the correlator's shape and the one-lane maths around it.  The veml
// kinds are these; the GLONASS one is GloLoopKind (trk_glonass_loop_device.hpp).
template <int NTAPS_, bool DATA_, bool HD_>
struct VemlLoopKind
{
    using State = LoopChan;
    static constexpr int NTAPS = NTAPS_;
    static constexpr bool DATA = DATA_, HD = HD_;
    static __device__ __forceinline__ int prepare(LoopChan& s, unsigned long long limit, gc_epoch_params& s_p, gc_loop_record* rec) { return loop_prepare<HD>(s, limit, s_p, rec); }
    static __device__ __forceinline__ void after_correlation(LoopChan& s, const float2* taps, gc_loop_record* rec) { loop_after_correlation<NTAPS, DATA>(s, taps, rec); }
};

// what the closed-loop kernels instantiate trk_epoch with (trk_device.hpp): real float replicas, one high-dynamics switch for the
// resampler and the rotator, and the settings measured above (LOOP_NT, LOOP_WHOLE)
template <int NTAPS_, bool HD_, int FMT_, int THREADS_, bool DATA_>
struct LoopEpochPolicy
{
    static constexpr int NTAPS = NTAPS_, FMT = FMT_, THREADS = THREADS_;
    static constexpr bool HDR = HD_, HDC = HD_, DATA = DATA_;
    static constexpr bool CC = false, SC16 = false, CHIPS = false;
    static constexpr bool NT = (LOOP_NT != 0);
    static constexpr bool WHOLE = (LOOP_WHOLE != 0);
    static constexpr bool GTAB = false;  // the launch's LDS holds the longest code's table (trk_loop_plan.h)
};

// The n_epochs code periods of one channel whose state `s` the workgroup holds in LDS (crec: the channel's first record): the
// body shared by the persistent kernel (one kind per launch), the mixed kernel (one per channel) and the GLONASS kernel.
template <class KIND, int THREADS, int FMT>
static __device__ __forceinline__ void loop_periods(typename KIND::State& s, gc_epoch_params& s_p, float2* s_corr, int& s_go, float* lds, gc_loop_record* crec,
    int n_epochs, int lds_table_floats, unsigned long long limit, int resident)
{
    constexpr int NTAPS = KIND::NTAPS;
    constexpr bool DATA = KIND::DATA, HD = KIND::HD;
    const int tid = threadIdx.x;
    // The replica does not change during a launch and this workgroup has the CU's LDS to itself: the doubled image
    // R[i] = code[i mod L] is loaded ONCE and every period addresses its window inside it, instead of re-reading the window from
    // global memory period after period (one round trip and a barrier per period)
    if (resident)
        {
            trk_fill_resident<THREADS>(lds, s.chan.code, DATA ? s.chan.code2 : nullptr, s.chan.code_len);
            __syncthreads();
        }

    for (int e = 0; e < n_epochs; e++)
        {
            gc_loop_record* rec = &crec[e];
            if (tid == 0)
                {
                    const int go = KIND::prepare(s, limit, s_p, rec);
                    s_go = go;
                }
            __syncthreads();
            if (!s_go) continue;  // uniform: every later epoch of this launch is skipped the same way

            const float2 r = trk_epoch<LoopEpochPolicy<NTAPS, HD, FMT, THREADS, DATA>>(s.chan, s_p, 0, 1, lds_table_floats, lds, LOOP_ALIGN_PAIRS, resident != 0);
            if (tid < NTAPS + (DATA ? 1 : 0)) s_corr[tid] = r;
            __syncthreads();

            if (tid == 0) KIND::after_correlation(s, s_corr, rec);
            // the next iteration's barrier orders these writes before any other thread reads s / s_p again
        }
}

// One channel of a launch, the shell of the persistent, the mixed and the GLONASS kernel: the workgroup loads slot blockIdx.x into
// `s` (LDS); a stand-by slot gets its all-zero records and nothing else; otherwise body(crec, limit) runs the periods -- crec is the
// channel's first record, limit the samples available to this launch: the channel's buffer length, or (ring input) the stream's
// head -- and the state goes back.  standby() is evaluated once the state is loaded.
template <int THREADS, class State, class Standby, class Body>
static __device__ __forceinline__ void loop_channel(State& s, State* chans, gc_loop_record* recs, int n_epochs, const unsigned long long* limits, Standby standby, Body body)
{
    const int ch = blockIdx.x;
    loop_copy_state<THREADS>(&s, &chans[ch]);
    __syncthreads();
    gc_loop_record* crec = &recs[(size_t)ch * n_epochs];
    if (standby())
        {
            loop_standby_records<THREADS>(crec, n_epochs);
            return;
        }
    const unsigned long long limit = limits ? limits[ch] : s.chan.n_iq;
    body(crec, limit);
    __syncthreads();
    loop_copy_state<THREADS>(&chans[ch], &s);
}

// ---- launches (host) ----
// One launch of n_channels workgroups over the engine's state buffer; plan.lds_bytes is the launch's dynamic LDS
struct LoopLaunch
{
    void* d_state;  // LoopChan or GloChan slots: the kernel's first parameter says which
    int n_channels, n_epochs;
    gc_loop_record* dev_records;
    hipStream_t st;
    TrkLoopPlan plan;
    const unsigned long long* limits;
};

// launches `kernel` with `threads` per workgroup; extra: the kernel's parameters behind `limits`
template <class State, class... Extra>
static hipError_t loop_launch_kernel(void (*kernel)(State*, gc_loop_record*, int, int, const unsigned long long*, Extra...), int threads, const LoopLaunch& a, Extra... extra)
{
    if (a.plan.lds_bytes > 48 * 1024)
        {
            hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.plan.lds_bytes);
            if (ea != hipSuccess) return ea;
        }
    hipLaunchKernelGGL(kernel, dim3(a.n_channels), dim3(threads), a.plan.lds_bytes, a.st, static_cast<State*>(a.d_state), a.dev_records, a.n_epochs, a.plan.lds_table_floats,
        a.limits, extra...);
    return hipGetLastError();
}

// The runtime axes of a launch are each switched once, with trk_switch_format / trk_switch_threads / trk_switch_bool (trk_kernels.h).

// the mixed kernel's launch (trk_closed_loop_mixed.hip)
hipError_t loop_launch_mixed(const LoopLaunch& a, int iq_format, bool high_dyn);
