// acq_caf_kernels.h -- device-side pieces of the CAF engine (gc_acq_create_caf; galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc)
// beside the transforms of acq_kernels.h.  The inverse column pass of a CAF dwell is acq_launch_cols with the ACQ_EPI_MAG epilogue,
// writing the |.|^2 planes of a satellite's R replicas ([sat][R][n_bins][N], replicas in the order IA, QA, IB, QB) and their block
// maxima; acq_caf_launch_select makes the block's per-bin choice of hypothesis and builds the grid row, acq_caf_launch_decide the
// per-dwell result and the CAF filter.
#ifndef ACQ_CAF_KERNELS_H
#define ACQ_CAF_KERNELS_H
#include "acq_caf_filter.h"
#include "gnsscorr.h"
#include <hip/hip_runtime.h>

#define ACQ_CAF_MAX_BINS 4096  // CAF_I and CAF_Q of a satellite wait in LDS (32 KB) while the filter runs

struct AcqCafSelectArgs
{
    const float* planes;           // [sat][R][n_bins][N] of this launch's satellites
    const float* pl_max_val;       // [sat][R][n_bins][n_blocks]: block maxima of the plane rows (column pass)
    const unsigned* pl_max_idx;
    float* grid;                   // [sat][n_bins][N]
    float* blk_max_val;            // [sat][n_bins][n_blocks]: block maxima of the grid rows, as a column pass leaves them
    unsigned* blk_max_idx;
    float* caf_i;                  // [sat][n_bins]
    float* caf_q;
    unsigned char* choice;         // [sat][n_bins]: bit 0 = I took B, bit 1 = Q took B
    int n_bins, n_blocks, N;
    int both, hyp;                 // R = (1 + both) * hyp
    int arithmetic;                // ACQ_CAF_REFERENCE: nQB = IB[kQB] / fnf4 (:523)
    float fnf4;
};

// one launch per satellite batch, behind its column pass: n_blocks workgroups per (satellite, bin), each of which recomputes the
// row's choice from the block maxima and streams its share of the chosen row(s) into the grid row.  R >= 2 only
hipError_t acq_caf_launch_select(hipStream_t st, const AcqCafSelectArgs& a, int n_sats);

struct AcqCafDecideArgs
{
    const float* blk_max_val;      // [sat][n_bins][n_blocks] of the grid rows
    const unsigned* blk_max_idx;
    const float* input_power;      // of this dwell
    gc_acq_result* results;        // [sat]: test_statistics is the kept statistic between dwells
    float* caf;                    // [sat][n_bins]
    float* caf_i;                  // written here when single_plane (the grid row is the only plane), read otherwise
    float* caf_q;
    unsigned char* choice;
    int n_bins, n_blocks, fft_size;
    int doppler_max, doppler_step;
    unsigned samples_per_code;
    int bit_transition;
    int both, single_plane;
    int caf_half;                  // H, 0: no filter
    int arithmetic;
    float fnf4;
};

// one launch per dwell, behind the last batch: one workgroup per satellite
hipError_t acq_caf_launch_decide(hipStream_t st, const AcqCafDecideArgs& a, int n_sats);

#endif
