// ring_decim_kernels.h -- launcher of the ring-to-ring FIR decimator: reads one gc_stream ring (any format) by absolute sample
// number, low-pass filters and decimates into a piece of a ring of any gc_iq_format and its mirror.  The conditioner's definition
// with no mixer, its accumulation (cond_fir_accum.h) and its store epilogue (cond_store_epilogue.h): for the same samples the two
// kernels produce the same bits in every output format.
#ifndef RING_DECIM_KERNELS_H
#define RING_DECIM_KERNELS_H
#include "cond_kernels.h"

#define GC_RDEC_THREADS 256

// One piece of outputs that is contiguous in the output ring.
struct RingDecimJob
{
    const void* src;               // source ring (HBM, 16-byte aligned): sample n lives at n % src_cap; src_cap is arbitrary
    unsigned src_cap;
    const float* taps;             // n_taps floats (HBM), read with uniform (scalar) loads
    int n_taps;
    int decimation;
    unsigned long long first_out;  // absolute number m of the first output of the piece
    unsigned n_out;                // outputs in the piece
    CondStoreDst out;              // where the piece goes: ring position first_out % capacity, its mirror, the scale and the
                                   // decimator's count of clipped components (gc_ring_stage_piece)
};

// Outputs per workgroup (64, 128 or 256): the largest that fits in GC_COND_LDS_SAMPLES and still gives `want_groups` workgroups.
// Results never depend on it.
int ring_decim_tile_outputs(int decimation, int n_taps, unsigned n_out, int want_groups);
// Enqueues the decimator for one piece on `st`.  iq_format: format of the source ring; out_format: format of the output ring.  The
// input window of every tile,
// [m0 D - (T - 1), (m0 + tile - 1) D] clipped at sample 0, must be resident in the source ring (at most src_cap samples).
hipError_t ring_decim_launch(int iq_format, int out_format, hipStream_t st, const RingDecimJob& job, int tile_outputs);

#endif
