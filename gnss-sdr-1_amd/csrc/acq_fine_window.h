// acq_fine_window.h -- the rules of the fine Doppler stage (pcps_acquisition_fine_doppler_cc.cc:400-479), for host and device.
//
// With N samples per code period, P code periods and a zero-padding factor Z the block transforms Next = P N Z points, of which
// the first P N are x[n] * r'[n mod N] (r': the local code rotated to the acquired delay s), takes the first largest |Y[k]|^2 and
// accepts its frequency when it lies within 1 kHz of the coarse Doppler.  Only those bins are computed here, so four statements of
// the block are kept in one place and shared by the kernels (acq_fine_kernels.hip), the entry points (gc_fine_doppler.hip) and
// tests/acq_fine_window_selftest.cpp:
//
//   fine_freq          the float32 frequency table, filled from double arithmetic on float32 operands (:135-146)
//   fine_window        {k : |(double)f[k] - fc| < window_hz} as one circular run (k_lo, count) of array indices; membership is
//                      decided on the float32 table value.  Precondition |fc| + window_hz < fs / 2: the run never reaches Nyquist
//   fine_replica_src   r'[i] = code[fine_replica_src(i, N, s, alignment)].  FINE_ALIGN_REFERENCE is the block's
//                      std::rotate(r, r + (N - s), r + N - 1) (:405-409): its last iterator leaves the final element where it is,
//                      so the code is one sample late for every s >= 2; FINE_ALIGN_EXACT is (i - s) mod N
//   fine_phase_index   (k n) mod Next in 64-bit integers: a twiddle's phase is always 2 pi index / Next of a reduced index
//
// Plain C++, no HIP types.  Built with -ffp-contract=off like the rest of the library.
#ifndef ACQ_FINE_WINDOW_H
#define ACQ_FINE_WINDOW_H
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FINE_HD __host__ __device__
#else
#define FINE_HD
#endif

enum
{
    FINE_ALIGN_REFERENCE = 0,
    FINE_ALIGN_EXACT = 1
};

static const uint32_t FINE_MAX_NEXT = 1u << 24;  // the table casts k to float: every index must be a float32 integer

// f[k], k < Next (Next even)
static FINE_HD inline float fine_freq(uint32_t k, int64_t fs, uint32_t next)
{
    const float fsf = (float)fs;
    const float nf = (float)next;
    if (k < next / 2) return (float)(((double)fsf / 2.0 * (double)(float)k) / ((double)nf / 2.0));
    return (float)(((double)(-fsf) / 2.0 * (double)(float)(next - k)) / ((double)nf / 2.0));
}

// array index of the signed bin j, -Next/2 <= j < Next/2 (f is non-decreasing in j)
static FINE_HD inline uint32_t fine_bin_of(int64_t j, uint32_t next)
{
    return (uint32_t)(j < 0 ? j + (int64_t)next : j);
}

static FINE_HD inline bool fine_in_window(int64_t j, int64_t fs, uint32_t next, double fc, double window_hz)
{
    const double d = (double)fine_freq(fine_bin_of(j, next), fs, next) - fc;
    return (d < 0.0 ? -d : d) < window_hz;
}

// what every entry point checks before it touches a device
static inline bool fine_sizes_ok(int64_t fs, uint64_t next)
{
    return fs > 0 && next >= 2 && (next & 1u) == 0 && next <= FINE_MAX_NEXT;
}
static inline bool fine_window_ok(int64_t fs, double fc, double window_hz)
{
    // written so that NaN and infinities fail
    if (!(window_hz > 0.0) || !(window_hz < 1e300) || !(fc > -1e300 && fc < 1e300)) return false;
    return (fc < 0.0 ? -fc : fc) + window_hz < (double)fs / 2.0;
}

// The window as a circular run: k = (k_lo + b) mod Next, b < count, in ascending frequency.  count may be 0 when the bins are
// wider than the window and none falls inside.  Requires fine_sizes_ok and fine_window_ok.
static inline void fine_window(int64_t fs, uint32_t next, double fc, double window_hz, uint32_t* k_lo, uint32_t* count)
{
    const int64_t half = (int64_t)(next / 2);
    const double df = (double)fs / (double)next;
    int64_t j = (int64_t)((fc - window_hz) / df) - 4;
    if (j < -half) j = -half;
    // the estimate is a few bins low at the most; walk down while it is inside (float32 rounding of the table), then up to the first member
    while (j > -half && fine_in_window(j, fs, next, fc, window_hz)) j--;
    while (j < half && !fine_in_window(j, fs, next, fc, window_hz))
        {
            if ((double)fine_freq(fine_bin_of(j, next), fs, next) - fc >= window_hz)
                {
                    *k_lo = fine_bin_of(j, next);
                    *count = 0;
                    return;
                }
            j++;
        }
    const int64_t first = j;
    while (j < half && fine_in_window(j, fs, next, fc, window_hz)) j++;
    *k_lo = fine_bin_of(first < half ? first : 0, next);
    *count = (uint32_t)(j - first);
}

// an upper bound of fine_window's count over every admissible fc
static inline uint64_t fine_window_max_bins(int64_t fs, uint32_t next, double window_hz)
{
    return (uint64_t)(2.0 * window_hz * (double)next / (double)fs) + 3;
}

static FINE_HD inline uint32_t fine_replica_src(uint32_t i, uint32_t n, uint32_t s, int alignment)
{
    if (alignment == FINE_ALIGN_EXACT) return i >= s ? i - s : i + n - s;
    if (s == 0 || i == n - 1) return i;
    return i < s - 1 ? n - s + i : i - (s - 1);
}

static FINE_HD inline uint32_t fine_phase_index(uint32_t k, uint64_t n, uint32_t next)
{
    return (uint32_t)(((uint64_t)k * n) % (uint64_t)next);
}

#endif
