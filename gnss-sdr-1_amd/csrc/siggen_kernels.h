// siggen_kernels.h -- launcher of the signal generator's kernel: a multi-satellite scene (code x data x secondary code x carrier
// per satellite, plus Gaussian noise) synthesised straight into a piece of a gc_stream ring and its mirror.  A sample's bits are a
// closed form of its absolute number (siggen_phase.h): nothing is carried from launch to launch.
#ifndef SIGGEN_KERNELS_H
#define SIGGEN_KERNELS_H
#include "cond_store_epilogue.h"
#include "siggen_phase.h"

#define GC_SIGGEN_THREADS 256
#define GC_SIGGEN_RUN 4                // samples per thread and tile: 1024 samples per tile
#define GC_SIGGEN_LDS_FLOATS 15360     // table entries of one launch that the LDS placement holds (60 KiB)

// one component of a satellite on the device
struct SiggenComp
{
    unsigned table_off;      // first entry of its table in SiggenJob::tables
    unsigned secondary_off;  // first symbol of its secondary code in SiggenJob::secondary
    unsigned secondary_len;  // 0: none
    unsigned periods_per_symbol;  // 0: no data
    unsigned period_offset;
    int axis;                // 0: real part, 1: imaginary part
    float gain;
    unsigned reserved;
};

// one satellite on the device (HBM; read with a wave-uniform index)
struct SiggenSat
{
    unsigned long long code_step_q, code_phase0_q, carr_step_q, carr_phase0_q;
    float amplitude;
    unsigned table_len;
    unsigned n_comp;
    unsigned reserved;
    SiggenComp comp[2];
};

// One piece of samples that is contiguous in the output ring.
struct SiggenJob
{
    const SiggenSat* sats;        // n_sats descriptors (HBM)
    const float* tables;          // every component's table, one behind the other (HBM)
    const signed char* secondary; // every secondary code, +-1 (HBM)
    unsigned n_sats;
    unsigned n_table_floats;      // entries in `tables`
    int tables_in_lds;            // 1: every workgroup copies `tables` into LDS first (n_table_floats <= GC_SIGGEN_LDS_FLOATS)
    float sigma;                  // 0: no noise is drawn
    unsigned long long seed;
    unsigned long long t_first;   // scenario sample of the piece's first output
    unsigned n_out;               // outputs in the piece
    unsigned ring_pos;            // ring position of the piece's first output (its parity aligns the 16-byte stores)
    CondStoreDst out;             // where the piece goes, in the output ring's format, and its mirror (gc_ring_stage_piece)
};

// Enqueue one piece on `st`; out_format: the output ring's gc_iq_format.  n_groups: workgroups to launch at most (each takes
// tiles of GC_SIGGEN_THREADS * GC_SIGGEN_RUN samples in turn).  Results never depend on it.
hipError_t siggen_launch(int out_format, hipStream_t st, const SiggenJob& job, int n_groups);

#endif
