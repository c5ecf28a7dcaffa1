// trk_batch_plan.h -- the open-loop tracking launches' decisions, as pure host functions: what depends on the arithmetic of a launch
// (the code format's traits), how an epoch is cut in slices and how much LDS a launch gets.  These decide speed, never results.
// Compiles without HIP (tests/trk_batch_plan_selftest.cpp prints the plan of any argument tuple; tests/test_trk_batch_plan.py holds
// a table worked out by hand against it).
#ifndef TRK_BATCH_PLAN_H
#define TRK_BATCH_PLAN_H
#include <algorithm>
#include <cmath>
#include <cstddef>

static constexpr int TRK_LDS_TABLE_FLOATS = 16000;  // code table in LDS: the 64 KB default dynamic-LDS limit minus the header
static constexpr int TRK_LDS_MARGIN_FLOATS = 64;    // table words behind the code itself
static constexpr int TRK_WINDOW_TARGET = 4096;      // floats of LDS per workgroup that still leave 8 waves per SIMD (9 workgroups of ~17 KB per CU)
static constexpr int TRK_CHUNK_SAMPLES = 512;       // samples a workgroup takes per step: slices are whole chunks

// The arithmetic of a batch or of a level-1 code, indexed by the kernel's TRK_MODE_* (trk_kernels.h; gc_tracking.hip asserts the
// order).  IQ formats as bits 1 << gc_iq_format (F32 1, I16 2, I8 4): trk_launch (trk_kernels.hip) instantiates a kernel for exactly
// these (mode, format) pairs and refuses the others.  No batch has TRK_MODE_HD_RESAMPLER; the level-1 object that selects it (the
// 6-argument overload) correlates complex float input only.
struct TrkFormatTraits
{
    int words_per_chip;       // 4-byte words of the code table per chip
    unsigned iq_formats;      // sample formats it correlates
    int out_bytes;            // bytes of one tap's result
    bool has_high_dyn;        // a high-dynamics variant of the format exists
    bool sliced_window;       // a slice's launch may hold a window of the table in LDS instead of all of it
    const char* name;         // for messages
    const char* code_setter;  // the batch's code setter that fits
};
static constexpr TrkFormatTraits TRK_FORMAT_TRAITS[5] = {
    {1, 7u, 8, true, true, "real", "gc_trk_batch_set_code"},                         // TRK_MODE_PLAIN
    {1, 1u, 8, true, false, "real", "gc_trk_batch_set_code"},                        // TRK_MODE_HD_RESAMPLER: the resampler's window is the
    {1, 7u, 8, true, false, "real", "gc_trk_batch_set_code"},                        // TRK_MODE_HD_FULL:      whole epoch whatever the slice
    {2, 7u, 8, false, true, "complex float", "gc_trk_batch_set_code_complex"},       // TRK_MODE_COMPLEX_CODE
    {1, 2u, 4, false, false, "16-bit complex", "gc_trk_batch_set_code_16sc"},        // TRK_MODE_SC16
};

struct TrkBatchPlan
{
    int n_slices;    // workgroups per job
    int lds_floats;  // code window of the launch
};

// forced_slices / lds_sizing: gc_trk_batch_set_slices (> 0: that many; sizing off: the whole table).  len: the longest window of the
// launch (or the nominal one).  Channel i has code_len[i * stride] chips and the tap shifts shifts[i * stride + t], t < n_taps: two
// members of one array of channel descriptors, `stride` 4-byte words each.  max_step: the largest |code step| of the records in chips
// per sample, 0 when the host cannot see them.  small_window_ok: trk_small_window_ok(format, iq_format).
// table_floats: the batch's whole table.  n_cus <= 0: 256.
static inline TrkBatchPlan trk_batch_plan(int forced_slices, bool lds_sizing, int n_channels, int n_epochs, int n_cus, int format, bool small_window_ok, int len,
    const int* code_len, const float* shifts, int stride, int n_taps, float max_step, int table_floats)
{
    TrkBatchPlan p = {1, table_floats};
    if (forced_slices > 0)
        p.n_slices = forced_slices;
    else
        {
            // aim at >= 8 workgroups per CU; never cut an epoch below 4 chunks (2048 samples) per slice
            const long long jobs = (long long)n_channels * n_epochs;
            const long long want = 8LL * (n_cus > 0 ? n_cus : 256);
            if (jobs < want && len > 0)
                {
                    const int chunks = (len + TRK_CHUNK_SAMPLES - 1) / TRK_CHUNK_SAMPLES;
                    const int s = (int)((want + jobs - 1) / jobs);
                    p.n_slices = std::max(1, std::min(std::min(s, std::max(chunks / 4, 1)), 64));
                }
        }
    // LDS of the launch: what one slice of a nominal epoch touches, not the capacity of the longest code (Galileo E1: 33 KB per
    // workgroup = 4 waves per SIMD; half a period per slice: 17 KB = 8).  Known on the host: the nominal window length, the code
    // lengths, the tap shifts; a code period per nominal window gives the chips per sample.  A record that exceeds the bound (a code
    // step far off nominal, a longer window) is served by the kernel from the whole table in LDS when it fits the launch's LDS, from
    // global memory otherwise (trk_epoch, GTAB): the bound decides speed, never results.
    const TrkFormatTraits& f = TRK_FORMAT_TRAITS[format];
    if (len < 4096 || !lds_sizing || !f.sliced_window || !small_window_ok) return p;  // (short windows: nothing to gain)
    int l_max = 0;
    float spread = 0.0f;
    for (int i = 0; i < n_channels; i++)
        {
            const float* sh = shifts + (size_t)i * stride;
            l_max = std::max(l_max, code_len[(size_t)i * stride]);
            spread = std::max(spread, *std::max_element(sh, sh + n_taps) - *std::min_element(sh, sh + n_taps));
        }
    // a long real code: at least as many slices as windows of the target size
    if (forced_slices == 0 && l_max + TRK_LDS_MARGIN_FLOATS > TRK_WINDOW_TARGET + 128 && f.words_per_chip == 1)
        p.n_slices = std::max(p.n_slices, (l_max + TRK_WINDOW_TARGET - 1) / TRK_WINDOW_TARGET);
    if (p.n_slices > 1)
        {
            const int chunks = (len + 16 + TRK_CHUNK_SAMPLES - 1) / TRK_CHUNK_SAMPLES;  // + the alignment lead-in of at most 8 sample pairs
            const int cps = (chunks + p.n_slices - 1) / p.n_slices;
            // chips per sample: the largest |code step| of the records when the caller's parameter array is on the host
            // (gc_trk_batch_run), else one code period per nominal window (device-resident records: a batch whose windows
            // span several code periods should state so with gc_trk_batch_set_slices(b, -1))
            const double chips_per_sample = max_step > 0.0f ? (double)max_step : (double)l_max / (double)len;
            // (in double: a huge or garbage step must not overflow an int on its way to "the whole table")
            const double need = (double)f.words_per_chip * (std::ceil((double)cps * (double)TRK_CHUNK_SAMPLES * chips_per_sample * 1.002 + (double)spread) + (double)TRK_LDS_MARGIN_FLOATS);
            // (a table that fits the 8-waves budget whole is left whole: nothing to gain, and windows of several code periods keep
            // the LDS modulo path; so is one whose bound is not finite, not positive or not below the table)
            if (std::isfinite(need) && need > 0.0 && need < (double)table_floats && table_floats > TRK_WINDOW_TARGET + 128) p.lds_floats = std::max(((int)need + 63) & ~63, 1024);
        }
    return p;
}

// A level-1 call is one epoch: cut in slices so that the launch covers many CUs.  The count depends on the window length alone, so
// a call gives the same sums whether it runs alone or inside a batch.  one_wg_max: windows up to this length run in one workgroup
// (measured: beyond ~2000 samples several workgroups + the partial-sum launch win); partial_slices: what the partial buffer holds.
static inline int trk_level1_slices(int N, int one_wg_max, int partial_slices)
{
    const int chunks = (N + 1 + TRK_CHUNK_SAMPLES - 1) / TRK_CHUNK_SAMPLES;
    const int n_slices = N <= one_wg_max ? 1 : std::max(chunks / 2, 1);
    return std::min(n_slices, partial_slices);
}

#endif
