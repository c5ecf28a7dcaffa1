// acq_tong_kernels.h -- device-side pieces of the Tong engine (gc_acq_create_tong; pcps_tong_acquisition_cc.cc) beside the
// transforms of acq_kernels.h: the per-dwell decision kernel and the restart of a search.  The column pass of a Tong dwell is
// acq_launch_cols_tong (acq_kernels.h).
#ifndef ACQ_TONG_KERNELS_H
#define ACQ_TONG_KERNELS_H
#include "acq_tong_decide.h"
#include "gnsscorr.h"
#include <hip/hip_runtime.h>

struct AcqTongDecideArgs
{
    const float* blk_max_val;     // [sat][bin][n_blocks]: block row maxima of the column pass
    const unsigned* blk_max_idx;
    const float* input_power;     // of this dwell
    gc_acq_result* results;       // [sat]
    AcqTongState* state;          // [sat]
    int* frozen;                  // [sat]: set when the state leaves "running"
    int n_bins, n_blocks, fft_size;
    int doppler_max, doppler_step;
    unsigned samples_per_code;
    AcqTongParams p;
};

// one launch per dwell, behind the column passes: d_mag and its cell of every RUNNING satellite (rows ascending, first maximum of a
// row, a later row only with a strictly larger value, nothing wins against 0 or with NaN), gc_acq_result, the decision step
hipError_t acq_tong_launch_decide(hipStream_t st, const AcqTongDecideArgs& a, int n_sats);

// start of a search: state = {running, init_val, 0}, frozen = 0, results zeroed
hipError_t acq_tong_launch_restart(hipStream_t st, AcqTongState* state, int* frozen, gc_acq_result* results, int n_sats, AcqTongParams p);

#endif
