// gc_numerics.cpp -- the host numerics of libgnsscorr.so's conditioner family, none of which needs a device: the windowed-sinc
// low-pass design (gc_fir_low_pass, the counterpart of gr::filter::firdes::low_pass), the chi-squared quantile behind the pulse
// blanker's threshold (gc_chi2_upper_quantile), the reference's rule for the acquisition resampler (gc_acq_resampler_plan,
// src/core/receiver/gnss_flowgraph.cc:375-499) and the tap bank of the ring resampler's polyphase mode (gc_resampler_design).
#include "cond_kernels.h"
#include "gc_internal.h"
#include "ring_resamp_kernels.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace
{
// log of the gamma function's regularised incomplete pair: P by its series (x < a + 1), Q by Lentz's continued fraction otherwise
double chi2_gamma_q(double a, double x)
{
    if (x <= 0.0) return 1.0;
    const double lead = std::exp(a * std::log(x) - x - std::lgamma(a));
    if (x < a + 1.0)
        {
            double term = 1.0 / a, sum = term;
            for (int k = 1; k < 1000000; k++)
                {
                    term *= x / (a + k);
                    sum += term;
                    if (term < sum * 1e-17) break;
                }
            return 1.0 - lead * sum;
        }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, cc = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int k = 1; k < 1000000; k++)
        {
            const double an = -(double)k * ((double)k - a);
            b += 2.0;
            d = an * d + b;
            if (std::fabs(d) < tiny) d = tiny;
            cc = b + an / cc;
            if (std::fabs(cc) < tiny) cc = tiny;
            d = 1.0 / d;
            const double del = d * cc;
            h *= del;
            if (std::fabs(del - 1.0) < 1e-16) break;
        }
    return lead * h;
}

// taps of the reference's low-pass for `decimation`; 0 when the design fails
int plan_taps(int64_t fs_in, uint32_t decimation)
{
    const double rfs = (double)fs_in / (double)decimation;
    int n = 0;
    if (gc_fir_low_pass(1.0, (double)fs_in, rfs / 2.1, rfs / 10.0, nullptr, 0, &n) != GC_OK) return 0;
    return n;
}
}  // namespace

extern "C" {

gc_status gc_chi2_upper_quantile(double dof, double pfa, double* out)
{
    if (out) *out = 0.0;
    GC_REQUIRE(out, "gc_chi2_upper_quantile: NULL result");
    GC_REQUIRE(dof > 0.0 && std::isfinite(dof), "gc_chi2_upper_quantile: dof %g is not positive", dof);
    GC_REQUIRE(pfa > 0.0 && pfa < 1.0, "gc_chi2_upper_quantile: pfa %g is outside (0, 1)", pfa);
    // Q(a, x) = pfa for x = q / 2, a = dof / 2: Newton steps on Q (dQ/dx = -x^(a-1) e^-x / Gamma(a)) kept inside a bracket that
    // every evaluation tightens, bisection whenever a step leaves it
    const double a = 0.5 * dof;
    double lo = 0.0, hi = a + 1.0;
    while (chi2_gamma_q(a, hi) > pfa) hi *= 2.0;
    double x = 0.5 * (lo + hi);
    for (int it = 0; it < 300; it++)
        {
            const double f = chi2_gamma_q(a, x) - pfa;
            if (f > 0.0)
                lo = x;
            else
                hi = x;
            const double pdf = std::exp((a - 1.0) * std::log(x) - x - std::lgamma(a));
            double xn = x + f / pdf;
            if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
            const bool done = std::fabs(xn - x) <= 2e-16 * x || hi - lo <= 2e-16 * hi;
            x = xn;
            if (done) break;
        }
    *out = 2.0 * x;
    return GC_OK;
}

gc_status gc_fir_low_pass(double gain, double fs, double cutoff_hz, double transition_hz, float* taps, int capacity, int* n_taps)
{
    if (n_taps) *n_taps = 0;
    GC_REQUIRE(fs > 0.0 && cutoff_hz > 0.0 && cutoff_hz <= 0.5 * fs && transition_hz > 0.0 && std::isfinite(gain) && std::isfinite(fs),
        "gc_fir_low_pass: need fs > 0, 0 < cutoff_hz <= fs / 2 and transition_hz > 0");
    // Hamming window: 53 dB of stop-band attenuation, length 53 fs / (22 transition), made odd
    const double want = 53.0 * fs / (22.0 * transition_hz);
    GC_REQUIRE(want < 1.0e6, "gc_fir_low_pass: the transition width asks for %.0f taps", want);
    int n = (int)want;
    if ((n & 1) == 0) n++;
    if (n_taps) *n_taps = n;
    if (!taps) return GC_OK;  // length query
    GC_REQUIRE(n <= capacity, "gc_fir_low_pass: %d taps do not fit in %d", n, capacity);
    const int M = (n - 1) / 2;
    const double pi = 3.14159265358979323846, w0 = 2.0 * pi * cutoff_hz / fs;
    std::vector<double> h((size_t)n);
    double sum = 0.0;
    for (int i = 0; i < n; i++)
        {
            const int k = i - M;
            const double win = n > 1 ? 0.54 - 0.46 * std::cos(2.0 * pi * i / (n - 1)) : 1.0;
            h[i] = (k == 0 ? w0 / pi : std::sin(k * w0) / (k * pi)) * win;
            sum += h[i];
        }
    for (int i = 0; i < n; i++) taps[i] = (float)(gain * h[i] / sum);
    return GC_OK;
}

gc_status gc_acq_resampler_plan(int64_t fs_in, uint32_t opt_acq_fs_hz, uint32_t* decimation, int64_t* resampled_fs, float* taps, int capacity, int* n_taps,
    uint32_t* latency_samples)
{
    if (decimation) *decimation = 1;
    if (resampled_fs) *resampled_fs = fs_in;
    if (n_taps) *n_taps = 0;
    if (latency_samples) *latency_samples = 0;
    GC_REQUIRE(fs_in > 0 && opt_acq_fs_hz > 0, "gc_acq_resampler_plan: the rates must be positive");
    // "Disabled acquisition resampler because the input sampling frequency is too low"
    if ((int64_t)opt_acq_fs_hz >= fs_in) return GC_OK;
    // the reference's rule: the largest divisor of fs_in that is not above floor(fs_in / opt) ... and this library's: on to the
    // next divisor while the kernel's limits (D <= 64, T <= 1024) are exceeded.  Together: the largest divisor that is not above
    // min(floor(fs_in / opt), 64) and whose filter fits -- one loop of at most 63 steps whatever the ratio of the rates
    int64_t dec = std::min<int64_t>(fs_in / (int64_t)opt_acq_fs_hz, GC_COND_MAX_DECIMATION);
    int T = 0;
    while (dec > 1)
        {
            if (fs_in % dec == 0 && dec <= GC_COND_MAX_DECIMATION)
                {
                    T = plan_taps(fs_in, (uint32_t)dec);
                    if (T >= 1 && T <= GC_COND_MAX_TAPS) break;
                }
            dec--;
        }
    if (dec <= 1) return GC_OK;
    const int64_t rfs = fs_in / dec;
    if (decimation) *decimation = (uint32_t)dec;
    if (resampled_fs) *resampled_fs = rfs;
    if (n_taps) *n_taps = T;
    if (latency_samples) *latency_samples = (uint32_t)((T - 1) / 2);
    if (!taps) return GC_OK;  // sizes alone
    GC_REQUIRE(T <= capacity, "gc_acq_resampler_plan: %d taps do not fit in %d", T, capacity);
    int n = 0;
    const double r = (double)fs_in / (double)dec;  // the reference's acq_fs: fs / decimation in double
    return gc_fir_low_pass(1.0, (double)fs_in, r / 2.1, r / 10.0, taps, capacity, &n);
}


gc_status gc_resampler_design(double fs_in, double fs_out, uint32_t phases, float* bank, int capacity, int* taps_per_phase)
{
    if (taps_per_phase) *taps_per_phase = 0;
    GC_REQUIRE(std::isfinite(fs_in) && std::isfinite(fs_out) && fs_in > 0.0 && fs_out > 0.0, "gc_resampler_design: the rates must be finite and positive");
    GC_REQUIRE(ring_resamp_power_of_two(phases) && phases <= GC_RRES_MAX_PHASES, "gc_resampler_design: %u phases, not a power of two in 1..%d", phases, GC_RRES_MAX_PHASES);
    const double P = (double)phases, low = std::min(fs_in, fs_out);
    int n = 0;
    gc_status st = gc_fir_low_pass(P, P * fs_in, low / 2.1, low / 10.0, nullptr, 0, &n);
    if (st != GC_OK) return st;
    const int64_t T = ((int64_t)n + phases - 1) / phases;
    GC_REQUIRE(T >= 1 && T <= GC_RRES_MAX_TAPS && (int64_t)phases * T <= GC_RRES_MAX_BANK,
        "gc_resampler_design: %lld taps per phase (%d prototype taps over %u phases) exceed %d per phase or %d in the bank", (long long)T, n, phases,
        GC_RRES_MAX_TAPS, GC_RRES_MAX_BANK);
    if (taps_per_phase) *taps_per_phase = (int)T;
    if (!bank) return GC_OK;  // T alone
    GC_REQUIRE((int64_t)phases * T <= capacity, "gc_resampler_design: %u x %lld taps do not fit in %d", phases, (long long)T, capacity);
    std::vector<float> g((size_t)phases * T, 0.0f);  // the prototype, zero-padded to phases * T
    st = gc_fir_low_pass(P, P * fs_in, low / 2.1, low / 10.0, g.data(), n, &n);
    if (st != GC_OK) return st;
    for (uint32_t p = 0; p < phases; p++)
        for (int64_t k = 0; k < T; k++) bank[(size_t)p * T + k] = g[(size_t)k * phases + p];
    return GC_OK;
}

}  // extern "C"
