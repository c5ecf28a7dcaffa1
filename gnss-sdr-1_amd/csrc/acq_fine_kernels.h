// acq_fine_kernels.h -- the two kernels of the fine Doppler stage (acq_fine_kernels.hip; rules in acq_fine_window.h).
#ifndef ACQ_FINE_KERNELS_H
#define ACQ_FINE_KERNELS_H
#include "gnsscorr.h"
#include "acq_fine_window.h"
#include <hip/hip_runtime.h>

#define ACQ_FINE_TILE 1024  // samples of one workgroup of the partial kernel
#define ACQ_FINE_SEED 32    // the twiddle recurrence is re-seeded from the exact phase index every so many samples

// one request as the kernels see it: the window already resolved by the host rule
struct AcqFineRequest
{
    uint32_t slot, delay, k_lo, count;
};

struct AcqFineArgs
{
    const void* src;           // ring of complex samples: sample n lives at n % src_cap
    unsigned src_cap;
    unsigned long long first;  // absolute number of x[0]; [first, first + total) is resident
    const float2* codes;       // [n_slots][n]
    const AcqFineRequest* req;
    float2* partial;           // [request][tile][stride]
    float* energy;             // [request][tile]
    float* spec;               // [request][stride]
    gc_fine_doppler_result* results;
    long long fs;
    uint32_t n, total, next, n_tiles, stride;
    int alignment;
};

// n_tiles = ceil(total / ACQ_FINE_TILE) workgroups per request; iq_format: the ring's gc_iq_format
hipError_t acq_fine_launch(hipStream_t st, const AcqFineArgs& a, int iq_format, int n_requests);

#endif
