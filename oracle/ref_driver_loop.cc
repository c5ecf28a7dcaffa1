/*
 * ref_driver_loop.cc -- C-linkage callers for the reference's loop filters that compile from their own
 * sources (test infrastructure).  tracking_FLL_PLL_filter.cc (the carrier loop filter of dll_pll_veml_tracking,
 * dll_pll_veml_tracking.cc:344,564,939-950,1752), tracking_2nd_DLL_filter.cc and tracking_2nd_PLL_filter.cc (the
 * code / carrier filters of the GLONASS and carrier-aided blocks) include nothing but their own headers; they are
 * compiled from /root/reference where they lie (oracle/Makefile target `ref` -> _ref/libref_loop.so).  This file
 * only gives their methods C names.
 *
 * The code loop filter of dll_pll_veml_tracking (tracking_loop_filter.cc, :340 with include_last_integrator = false, re-designed at
 * :1750-1751), its discriminators (tracking_discriminators.cc, :914-973) and its lock detectors (lock_detectors.cc, :839-878) want
 * <glog/logging.h> and <gnuradio/gr_complex.h>: oracle/shim/ holds a stand-in for each (a LOG that writes nowhere, gr_complex as
 * std::complex<float>), written by this project, and the three files compile unchanged behind it.  Complex values cross the C
 * boundary as (re, im) float pairs.
 */
#include "lock_detectors.h"
#include "tracking_2nd_DLL_filter.h"
#include "tracking_2nd_PLL_filter.h"
#include "tracking_FLL_PLL_filter.h"
#include "tracking_discriminators.h"
#include "tracking_loop_filter.h"
#include <vector>

extern "C" {
void* ref_fll_pll_new() { return new Tracking_FLL_PLL_filter(); }
void ref_fll_pll_delete(void* f) { delete static_cast<Tracking_FLL_PLL_filter*>(f); }
void ref_fll_pll_set_params(void* f, float fll_bw_hz, float pll_bw_hz, int order)
{
    static_cast<Tracking_FLL_PLL_filter*>(f)->set_params(fll_bw_hz, pll_bw_hz, order);
}
void ref_fll_pll_initialize(void* f, float doppler_hz) { static_cast<Tracking_FLL_PLL_filter*>(f)->initialize(doppler_hz); }
float ref_fll_pll_get_carrier_error(void* f, float fll, float pll, float t)
{
    return static_cast<Tracking_FLL_PLL_filter*>(f)->get_carrier_error(fll, pll, t);
}

void* ref_dll2_new(float pdi) { return new Tracking_2nd_DLL_filter(pdi); }
void ref_dll2_delete(void* f) { delete static_cast<Tracking_2nd_DLL_filter*>(f); }
void ref_dll2_set_bw(void* f, float bw) { static_cast<Tracking_2nd_DLL_filter*>(f)->set_DLL_BW(bw); }
void ref_dll2_set_pdi(void* f, float pdi) { static_cast<Tracking_2nd_DLL_filter*>(f)->set_pdi(pdi); }
void ref_dll2_initialize(void* f) { static_cast<Tracking_2nd_DLL_filter*>(f)->initialize(); }
float ref_dll2_get_code_nco(void* f, float e) { return static_cast<Tracking_2nd_DLL_filter*>(f)->get_code_nco(e); }

void* ref_pll2_new(float pdi) { return new Tracking_2nd_PLL_filter(pdi); }
void ref_pll2_delete(void* f) { delete static_cast<Tracking_2nd_PLL_filter*>(f); }
void ref_pll2_set_bw(void* f, float bw) { static_cast<Tracking_2nd_PLL_filter*>(f)->set_PLL_BW(bw); }
void ref_pll2_set_pdi(void* f, float pdi) { static_cast<Tracking_2nd_PLL_filter*>(f)->set_pdi(pdi); }
void ref_pll2_initialize(void* f) { static_cast<Tracking_2nd_PLL_filter*>(f)->initialize(); }
float ref_pll2_get_carrier_nco(void* f, float e) { return static_cast<Tracking_2nd_PLL_filter*>(f)->get_carrier_nco(e); }

void* ref_lf_new(float update_interval, float noise_bandwidth, int order) { return new Tracking_loop_filter(update_interval, noise_bandwidth, order, false); }
void ref_lf_delete(void* f) { delete static_cast<Tracking_loop_filter*>(f); }
void ref_lf_initialize(void* f) { static_cast<Tracking_loop_filter*>(f)->initialize(); }
void ref_lf_set_noise_bandwidth(void* f, float bw) { static_cast<Tracking_loop_filter*>(f)->set_noise_bandwidth(bw); }
void ref_lf_set_update_interval(void* f, float t) { static_cast<Tracking_loop_filter*>(f)->set_update_interval(t); }
float ref_lf_apply(void* f, float v) { return static_cast<Tracking_loop_filter*>(f)->apply(v); }

static gr_complex cx(const float* v) { return gr_complex(v[0], v[1]); }
double ref_fll_four_quadrant_atan(const float* s1, const float* s2, double t1, double t2) { return fll_four_quadrant_atan(cx(s1), cx(s2), t1, t2); }
double ref_pll_four_quadrant_atan(const float* s1) { return pll_four_quadrant_atan(cx(s1)); }
double ref_pll_cloop_two_quadrant_atan(const float* s1) { return pll_cloop_two_quadrant_atan(cx(s1)); }
double ref_dll_nc_e_minus_l_normalized(const float* e, const float* l) { return dll_nc_e_minus_l_normalized(cx(e), cx(l)); }
double ref_dll_nc_vemlp_normalized(const float* ve, const float* e, const float* l, const float* vl)
{
    return dll_nc_vemlp_normalized(cx(ve), cx(e), cx(l), cx(vl));
}

float ref_cn0_svn_estimator(const float* prompts, int length, double coh_integration_time_s)
{
    std::vector<gr_complex> b(length);
    for (int i = 0; i < length; i++) b[i] = cx(prompts + 2 * i);
    return cn0_svn_estimator(b.data(), length, coh_integration_time_s);
}
float ref_carrier_lock_detector(const float* prompts, int length)
{
    std::vector<gr_complex> b(length);
    for (int i = 0; i < length; i++) b[i] = cx(prompts + 2 * i);
    return carrier_lock_detector(b.data(), length);
}
}
