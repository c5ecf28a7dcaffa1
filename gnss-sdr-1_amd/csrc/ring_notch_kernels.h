// ring_notch_kernels.h -- launchers of the notch filter ring stage's passes: from a GC_IQ_F32 gc_stream ring, read by absolute
// sample number, into a piece of another GC_IQ_F32 ring and its mirror at the same rate.  The arithmetic is notch_decide.h's.
#ifndef RING_NOTCH_KERNELS_H
#define RING_NOTCH_KERNELS_H
#include "cond_store_epilogue.h"
#include "notch_decide.h"

#define GC_NOTCH_THREADS 256
#define GC_NOTCH_MAX_LENGTH 1024

// What the stage keeps in HBM.  Segment s has the record s % records: the passes of one batch of segments write them, and the
// pieces of the output ring that hold those segments read them, also a piece that begins in the middle of a segment of an
// earlier batch.
struct RingNotchWork
{
    NotchState* state;
    const NotchC* twiddles;  // length entries (notch_twiddle)
    float* energies;         // E[s]
    unsigned char* bits;     // NOTCH_SEG_*
    unsigned* back;          // lite, filtered segments: how many segments back the coefficient in use was computed
    NotchC* z;               // lite, filtered segments: the coefficient in use
    NotchC* A;               // filtered segments: the composite map of the segment
    NotchC* B;
    NotchC* carry;           // filtered segments: last in front of the segment
    unsigned records;
};

struct RingNotchJob
{
    const void* src;   // source ring (HBM, GC_IQ_F32): sample n lives at n % src_cap; src_cap is arbitrary
    unsigned src_cap;
    NotchParams params;
    RingNotchWork work;
};

// Decides segments [seg0, seg0 + n_seg) in order and carries last through them: energies, decisions, composites, the walk.  Four
// launches chained on `st`; the samples [seg0 L - 1 (clipped at 0), (seg0 + n_seg) L) must be resident in the source ring, and
// n_seg < records.
hipError_t ring_notch_decide_launch(hipStream_t st, const RingNotchJob& job, unsigned long long seg0, unsigned n_seg);
// Writes outputs [idx, idx + n_out), contiguous in the output ring, from the records of their segments (all decided, at most
// records - 1 segments back from the newest decided one); the samples from the first of those segments' first sample, less one,
// must be resident.  Two launches: unfiltered samples are copied sample by sample, filtered segments run the recursion.
hipError_t ring_notch_apply_launch(hipStream_t st, const RingNotchJob& job, unsigned long long idx, unsigned n_out, const CondStoreDst& out);

#endif
