// cond_blank_kernels.h -- launcher of the signal conditioner's pulse blanking (segment energies, decisions, apply) on the raw ring.
#ifndef COND_BLANK_KERNELS_H
#define COND_BLANK_KERNELS_H
#include "cond_blank_decide.h"
#include "gnsscorr.h"
#include <hip/hip_runtime.h>

#define GC_COND_MAX_BLANK_LENGTH 4096
#define GC_BLANK_THREADS 256

// The segments [seg0, seg0 + n_seg) of the raw stream, all of whose samples are in the raw ring (segment s = raw samples
// [s L, (s + 1) L), raw sample n at n % raw_cap).
struct BlankJob
{
    void* raw;                // raw ring (HBM), as in CondJob; flagged segments are zeroed in place
    unsigned raw_cap;         // multiple of 8 samples and > length + 16 (gc_iq_format), of 64 and > length + 128 (real formats)
    unsigned length;          // L, 1..GC_COND_MAX_BLANK_LENGTH
    unsigned long long seg0;  // absolute number of the first segment
    unsigned n_seg;
    float* energies;          // n_seg floats (HBM scratch): energy of segment seg0 + i
    unsigned char* flags;     // n_seg bytes (HBM scratch): 1 = blanked
    BlankState* state;        // HBM, carried from launch to launch
    BlankParams params;
};

// Lanes that share one segment (a power of two, 1..64): a function of the format and L alone, like the whole summation order.
// 0 for a format that is not blanked (GC_RAW_REAL_2BIT, unknown values).
int cond_blank_lanes(int iq_format, unsigned length);
// Enqueues the three stages for the job on `st`: energies, decisions (one wave), apply.  iq_format: format of the raw ring.
hipError_t cond_blank_launch(int iq_format, hipStream_t st, const BlankJob& job);

#endif
