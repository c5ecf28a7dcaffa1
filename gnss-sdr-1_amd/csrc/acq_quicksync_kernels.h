// acq_quicksync_kernels.h -- the two kernels the QuickSync search (pcps_quicksync_acquisition_cc.cc) adds to the PCPS engine:
// the fold in front of the M-point transforms and the time-domain check of the f aliased delays behind the statistics kernel.
#ifndef ACQ_QUICKSYNC_KERNELS_H
#define ACQ_QUICKSYNC_KERNELS_H
#include "acq_kernels.h"

// y[bin][(m % N1) * N2 + m / N1] = sum_{t < terms} x[t M + m] * wipe[bin][t M + m], m < M = plan.N (:382-396): float32 products
// and sums, t ascending from 0 for every output whatever the launch geometry; stored in the row-permuted layout the forward row
// pass reads.  x and the wipe-off rows (natural order, L samples each) are read up to index terms * M - 1 <= L - 1.
hipError_t acq_qs_launch_fold(hipStream_t st, const float2* x, const float2* wipe, float2* y, int n_bins, int L, int terms, const AcqFftPlan& plan);

struct AcqQsVerifyArgs
{
    const float2* x;      // the dwell's block, L samples
    const float2* wipe;   // [n_bins][L], natural order
    const float2* codes;  // [sat][N]: one code period per satellite, as handed to set_local_code (not conjugated, :462)
    gc_acq_result* results;  // in: indext, doppler_index of the folded search; out: acq_delay_samples
    float* cand_val;         // [sat][f]: d_corr_output_f
    uint32_t* cand_delay;    // [sat][f]: d_possible_delay
    int N, M, L, f, n_bins;
};
// candidate i < f of satellite s: p = k* + i M, a = sum_{j < min(N, L - p)} x[p + j] wipe[b*][p + j] code[s][j] (:445-470), (b*, k*)
// read from results[s] on the device; then the first maximum of |a|^2 over i gives results[s].acq_delay_samples (:471-474)
hipError_t acq_qs_launch_verify(hipStream_t st, const AcqQsVerifyArgs& a, int n_sats);

#endif
