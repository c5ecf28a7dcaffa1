// C names for the drop-in layer's own loop filters (gnss-sdr-1_amd/adapter/tracking_loop_maths.h: Tracking_FLL_PLL_filter;
// adapter/hip_glonass_ca_dll_pll_tracking.h: Tracking_2nd_DLL_filter / Tracking_2nd_PLL_filter), so that
// tests/test_loop_filter_pin.py can run the committed scripts of tests/golden/ref_loop_filters.npz (outputs of the REFERENCE's
// filters compiled in oracle/_ref) through them, and those of tests/golden/ref_loop_maths.npz through its Tracking_loop_filter,
// discriminators and lock detectors.  Host-only code, built by the test with g++.
#include "tracking_loop_maths.h"
#ifdef WITH_SECOND_ORDER
#include "hip_glonass_ca_dll_pll_tracking.h"
#endif

extern "C" {
int fp_run(int order, float fll_bw, float pll_bw, float narrow_bw, float doppler, int n_switch, int n, const float* fll, const float* pll,
    const float* T, float* out)
{
    Tracking_FLL_PLL_filter f;
    f.set_params(fll_bw, pll_bw, order);
    f.initialize(doppler);
    for (int k = 0; k < n; k++)
        {
            if (k == n_switch) f.set_params(fll_bw, narrow_bw, order);
            out[k] = f.get_carrier_error(fll[k], pll[k], T[k]);
        }
    return 0;
}
// The code loop filter script of tests/golden/ref_loop_maths.npz: constructed without the last integrator, initialised, re-designed at
// n_switch by set_update_interval then set_noise_bandwidth (the block's order), history kept.
int lf_run(int order, float bw, float t_wide, float narrow_bw, float t_narrow, int n_switch, int n, const float* in, float* out)
{
    Tracking_loop_filter f(t_wide, bw, order, false);
    f.initialize();
    for (int k = 0; k < n; k++)
        {
            if (k == n_switch)
                {
                    f.set_update_interval(t_narrow);
                    f.set_noise_bandwidth(narrow_bw);
                }
            out[k] = f.apply(in[k]);
        }
    return 0;
}

// taps: n x 6 complex floats, VE E P L VL and the previous prompt; out: n x 5 doubles, FLL, four-quadrant PLL, two-quadrant PLL,
// E-minus-L, VEMLP
int disc_run(int n, const float* taps, const double* T, double* out)
{
    for (int k = 0; k < n; k++)
        {
            const float* t = taps + 12 * k;
            const gr_complex_t VE(t[0], t[1]), E(t[2], t[3]), P(t[4], t[5]), L(t[6], t[7]), VL(t[8], t[9]), Pold(t[10], t[11]);
            out[5 * k + 0] = fll_four_quadrant_atan(Pold, P, 0.0, T[k]);
            out[5 * k + 1] = pll_four_quadrant_atan(P);
            out[5 * k + 2] = pll_cloop_two_quadrant_atan(P);
            out[5 * k + 3] = dll_nc_e_minus_l_normalized(E, L);
            out[5 * k + 4] = dll_nc_vemlp_normalized(VE, E, L, VL);
        }
    return 0;
}

// buffers: n x length complex floats
int lock_run(int n, int length, const float* buffers, const double* T, float* cn0, float* lock_test)
{
    for (int k = 0; k < n; k++)
        {
            const gr_complex_t* b = reinterpret_cast<const gr_complex_t*>(buffers + 2 * (size_t)k * length);
            cn0[k] = cn0_svn_estimator(b, length, T[k]);
            lock_test[k] = carrier_lock_detector(b, length);
        }
    return 0;
}
#ifdef WITH_SECOND_ORDER
int s2_run(int which, float bw, float pdi, float bw2, float pdi2, int n, const float* e, float* out)
{
    if (which == 0)
        {
            Tracking_2nd_DLL_filter f(pdi);
            f.set_DLL_BW(bw);
            f.initialize();
            for (int k = 0; k < n; k++)
                {
                    if (k == n / 2)
                        {
                            f.set_pdi(pdi2);
                            f.set_DLL_BW(bw2);
                        }
                    out[k] = f.get_code_nco(e[k]);
                }
        }
    else
        {
            Tracking_2nd_PLL_filter f(pdi);
            f.set_PLL_BW(bw);
            f.initialize();
            for (int k = 0; k < n; k++)
                {
                    if (k == n / 2)
                        {
                            f.set_pdi(pdi2);
                            f.set_PLL_BW(bw2);
                        }
                    out[k] = f.get_carrier_nco(e[k]);
                }
        }
    return 0;
}
#endif
}
