// acq_caf_filter.h -- the CAF Doppler filter of galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc (:685-765), for host and device.
//
// The block smooths the per-bin peaks of the I and of the Q component over H = CAF_window_hz / (2 * doppler_step) bins to either side
// with a triangular weight 1 - wf * distance, wf = 0.5f / H, in three sections:
//
//   head    d < H              i = 0 .. H + d            denominator 1 + H + d - wf H (H + 1) / 2 - wf d (d + 1) / 2
//   middle  H <= d < n - H     i = d - H .. d + H        denominator 1 + 2 H - 2 wf H (H + 1) / 2
//   tail    d >= n - H         i = d - H .. n - 1        denominator 1 + H + (n - d - 1) - wf H (H + 1) / 2 - wf (n - d - 1) (n - d) / 2
//
// every sum a float32 running sum in index order, CAF[d] = I sum / denominator + Q sum / denominator.  The block takes the
// distance as static_cast<unsigned int>(d - i) WITHOUT abs in three of the six sums -- the I sums of the head and of the middle
// section and the Q sum of the middle section -- so that for i > d the difference wraps to 2^32 - (i - d) and the weight becomes
// 1 - wf * 4.29e9.  ACQ_CAF_REFERENCE reproduces that (with explicit unsigned arithmetic: defined behaviour), ACQ_CAF_EXACT takes
// |d - i| in all six.  acq_caf_at() is the statement for one d: acq_caf_decide_kernel runs it with one lane per bin,
// tests/acq_caf_filter_selftest.cpp on the CPU.  Built with -ffp-contract=off: one rounding per operation, everywhere.
//
// The caller guarantees H >= 1 and n_bins >= 2 H + 1 (gc_acq_create_caf refuses anything else: the block reads out of range or
// divides by zero there).
#ifndef ACQ_CAF_FILTER_H
#define ACQ_CAF_FILTER_H
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CAF_HD __host__ __device__
#else
#define CAF_HD
#endif

enum
{
    ACQ_CAF_REFERENCE = 0,
    ACQ_CAF_EXACT = 1
};

// the weight of sample i in the sum of bin d; `wraps`: the block's unsigned difference without abs
static CAF_HD inline float acq_caf_weight(float wf, int d, int i, bool wraps)
{
    const uint32_t dist = wraps ? (uint32_t)d - (uint32_t)i : (uint32_t)(d >= i ? d - i : i - d);
    return 1.0f - wf * (float)dist;
}

// CAF[d] of the vectors caf_i and caf_q (caf_q may be null: I only), n_bins entries each
static CAF_HD inline float acq_caf_at(const float* caf_i, const float* caf_q, int n_bins, int H, int d, int arithmetic)
{
    const bool ref = arithmetic == ACQ_CAF_REFERENCE;
    const float wf = 0.5f / (float)H;
    int lo, hi;  // i = lo .. hi - 1
    float den;
    bool wraps_i, wraps_q;
    if (d < H)
        {
            lo = 0;
            hi = H + d + 1;
            den = (float)(1 + H + d) - wf * (float)H * (float)(H + 1) / 2.0f - wf * (float)d * (float)(d + 1) / 2.0f;
            wraps_i = ref;
            wraps_q = false;
        }
    else if (d < n_bins - H)
        {
            lo = d - H;
            hi = d + H + 1;
            den = (float)(1 + 2 * H) - 2.0f * wf * (float)H * (float)(H + 1) / 2.0f;
            wraps_i = ref;
            wraps_q = ref;
        }
    else
        {
            lo = d - H;
            hi = n_bins;
            const int r = n_bins - d - 1;
            den = (float)(1 + H + r) - wf * (float)H * (float)(H + 1) / 2.0f - wf * (float)r * (float)(r + 1) / 2.0f;
            wraps_i = false;
            wraps_q = false;
        }
    float acc = 0.0f;
    for (int i = lo; i < hi; i++) acc += caf_i[i] * acq_caf_weight(wf, d, i, wraps_i);
    acc /= den;
    if (caf_q)
        {
            float q = 0.0f;
            for (int i = lo; i < hi; i++) q += caf_q[i] * acq_caf_weight(wf, d, i, wraps_q);
            q /= den;
            acc += q;
        }
    return acc;
}

#endif
