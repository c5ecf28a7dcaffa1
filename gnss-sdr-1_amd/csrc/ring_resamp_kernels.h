// ring_resamp_kernels.h -- launchers of the ring resampler's two kernels: from one gc_stream ring, read by absolute sample number,
// into a piece of another ring and its mirror at an arbitrary rate ratio.  Direct mode gathers samples as they are (the reference's
// Direct_Resampler); polyphase mode filters with one of P tap rows per output.  The index arithmetic is resamp_index.h's.
#ifndef RING_RESAMP_KERNELS_H
#define RING_RESAMP_KERNELS_H
#include "cond_store_epilogue.h"
#include "resamp_index.h"

#define GC_RRES_THREADS 256
#define GC_RRES_MAX_PHASES 256
#define GC_RRES_MAX_TAPS 1024
#define GC_RRES_MAX_BANK 8192        // phases * taps per phase: 32 KiB of LDS
#define GC_RRES_LDS_BYTES 65536      // source window + tap bank of one workgroup

static inline bool ring_resamp_power_of_two(uint32_t v) { return v != 0 && (v & (v - 1)) == 0; }

// One piece of outputs that is contiguous in the output ring.
struct RingResampJob
{
    const void* src;           // source ring (HBM, 16-byte aligned): sample n lives at n % src_cap; src_cap is arbitrary
    unsigned src_cap;
    int kind;                  // RESAMP_IDENTITY / RESAMP_DOWN / RESAMP_UP (direct) or RESAMP_POLY
    unsigned long long step;   // step of the direct kinds, INC of RESAMP_POLY
    unsigned long long q0, r0; // resamp_base() of the piece's first output
    unsigned n_out;            // outputs in the piece
    CondStoreDst out;          // where the piece goes, in the output ring's format, and its mirror (gc_ring_stage_piece); neither
                               // kernel scales or counts
    // RESAMP_POLY
    const float* bank;         // phases rows of ring_resamp_bank_pitch(taps) floats (HBM): row p holds H[p][0 .. taps - 1]
    int log2_phases;
    int taps;
};

// floats per row of the bank, in HBM and in LDS: odd, so that lanes with different phases spread over the LDS banks
static RESAMP_HD inline int ring_resamp_bank_pitch(int taps) { return taps | 1; }
// source samples the LDS window of a tile of `tile` outputs must hold: n_last - n_first + taps at most
static inline unsigned long long ring_resamp_window(unsigned long long inc, int taps, int tile)
{
    return (((unsigned long long)(tile - 1) * inc + 0xffffffffull) >> 32) + (unsigned long long)taps;
}
// Outputs per workgroup in polyphase mode: 256, halved down to 16 until the window and the bank fit in GC_RRES_LDS_BYTES and, from
// 256 down to 64, until the launch has `want_groups` workgroups.  0 when nothing fits.  Results never depend on it.
int ring_resamp_tile_outputs(unsigned long long inc, int taps, int phases, unsigned n_out, int want_groups);
// Enqueue one piece on `st`.  The source samples of the piece, [n_first (less taps - 1 in polyphase mode, clipped at 0), n_last],
// must be resident in the source ring.  Direct: the rings have the same format `iq_format`.  Polyphase: iq_format is the source
// ring's, the output ring is GC_IQ_F32.
hipError_t ring_resamp_direct_launch(int iq_format, hipStream_t st, const RingResampJob& job);
hipError_t ring_resamp_poly_launch(int iq_format, hipStream_t st, const RingResampJob& job, int tile_outputs);

#endif
