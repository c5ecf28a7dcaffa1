// cond_kernels.h -- launcher of the signal conditioner kernel: frequency-translating FIR decimator (mix down, low-pass, decimate)
// from a ring of raw samples into a piece of an RF stream ring (gc_stream) and its mirror.
#ifndef COND_KERNELS_H
#define COND_KERNELS_H
#include "cond_store_epilogue.h"

#define GC_COND_MAX_DECIMATION 64
#define GC_COND_MAX_TAPS 1024
#define GC_COND_THREADS 256
#define GC_COND_LDS_SAMPLES 8192  // float2 entries of one workgroup's input tile (64 KiB)

// One piece of outputs that is contiguous in the output ring.
struct CondJob
{
    const void* raw;               // raw ring (HBM): raw sample n lives at n % raw_cap; raw_cap is a multiple of cond_raw_align()
                                   // samples (a whole number of 16-byte vectors in the format) and the allocation is 16-byte
                                   // aligned, so an aligned 16-byte vector never straddles the wrap
    unsigned raw_cap;
    const float* taps;             // n_taps floats (HBM), read with uniform (scalar) loads
    int n_taps;
    int decimation;
    unsigned long long phase_inc;  // turns per input sample in units of 2^-64; 0 = no mixer
    unsigned long long first_out;  // absolute number m of the first output of the piece
    unsigned n_out;                // outputs in the piece
    CondStoreDst out;              // where the piece goes: ring position first_out % capacity, its mirror, the scale and the
                                   // conditioner's count of clipped components (gc_ring_stage_piece)
};

// Outputs per workgroup for a launch (a multiple of 64, at most 1024): as many as fit in GC_COND_LDS_SAMPLES, fewer when the
// launch would not reach `want_groups` workgroups.  Results never depend on it.
int cond_tile_outputs(int decimation, int n_taps, unsigned n_out, int want_groups);
// Samples the raw ring's capacity must be a multiple of: 8 for the gc_iq_format values (16 bytes of the narrowest), 64 for the
// gc_raw_real_format values (16 bytes of 2-bit samples); 0 for an unknown format.  A launch needs twice that as slack: a tile's
// inputs plus one vector on each side must fit in the ring without lapping it.
unsigned cond_raw_align(int iq_format);
// Bits per raw sample: 64 / 32 / 16 for gr_complex / cshort / cbyte, 32 / 16 / 8 / 2 for the real formats; 0 for an unknown format.
unsigned cond_raw_bits(int iq_format);
// Enqueues the conditioner for one piece on `st`.  iq_format: format of the raw ring (gc_iq_format or gc_raw_real_format);
// out_format: gc_iq_format of the output ring.
hipError_t cond_launch(int iq_format, int out_format, hipStream_t st, const CondJob& job, int tile_outputs);

#endif
