// cond_store_epilogue.h -- the store epilogue every FIR decimator of the library shares (cond_kernels.hip, ring_decim_kernels.hip),
// and the description of a piece of the output ring that every stage's job carries (the ring resampler's too):
// a tile's accumulated outputs go to a piece of the output ring and, for the first n_mirror outputs of the piece, to the same
// place behind the ring.  OUT is the ring's gc_iq_format.
//
//   GC_IQ_F32   the float2 as it is: one 8-byte store per output (and one more for the mirror).
//   GC_IQ_I16 / GC_IQ_I8   each component c becomes   v = c * scale (one float32 product);  v = MAX if v > MAX, MIN if v < MIN;
//               q = (intN) rintf(v) (ties to even);  a NaN stores 0.  A component with v > MAX or v < MIN -- strict, before the
//               rounding, never a NaN -- counts as clipped.
//
// cshort: an output is one dword, stored by the lane that accumulated it.  cbyte: an output is two bytes, so the lanes put their
// outputs into the LDS tile -- free once every wave has finished its accumulation, hence the barrier in front -- and the workgroup
// stores the tile's byte range as dwords: element k of the tile lies at base + 2 k, the dword stores start at the first 4-byte
// boundary and take two neighbouring outputs each; only an element in front of that boundary and one left over at the end go out
// as 2-byte stores.  The ring position of a piece and the length of its mirror part can be odd, and the ring's capacity too, so the
// boundary is found for dst and for mirror_dst separately.  Which lane ACCUMULATES which output is not changed.
//
// Clipped components are counted once per output (the mirror copy is not counted again; lanes past the end of a short tile count
// nothing): summed over the wave with cross-lane moves, over the workgroup through LDS, and added to the producer's 64-bit counter
// in HBM with one atomicAdd per workgroup -- none when the workgroup's count is zero.
//
// Every thread of the workgroup must call cond_store_tile when OUT is not GC_IQ_F32 (it holds barriers).
#ifndef COND_STORE_EPILOGUE_H
#define COND_STORE_EPILOGUE_H
#include "gnsscorr.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

// where a piece of outputs that is contiguous in the output ring goes: embedded in every stage's job, filled by the host's
// gc_ring_stage_piece (gc_ring_stage.h)
struct CondStoreDst
{
    void* dst;                    // where output 0 of the piece goes, in the ring's format
    void* mirror_dst;             // the same position behind the ring
    unsigned n_mirror;            // the first n_mirror outputs of the piece are stored to mirror_dst as well
    float scale;                  // GC_IQ_I16 / GC_IQ_I8 only
    unsigned long long* clipped;  // GC_IQ_I16 / GC_IQ_I8 only: running count of clipped components (HBM)
};

template <int OUT>
struct CondOutRange;
template <>
struct CondOutRange<GC_IQ_I16>
{
    static constexpr float MINV = -32768.0f, MAXV = 32767.0f;
};
template <>
struct CondOutRange<GC_IQ_I8>
{
    static constexpr float MINV = -128.0f, MAXV = 127.0f;
};

// one component: scale, clamp, round; n_clipped goes up when the clamp acted
template <int OUT>
static __device__ __forceinline__ int cond_quantise(const float c, const float scale, unsigned& n_clipped)
{
    float v = c * scale;
    if (v > CondOutRange<OUT>::MAXV)
        {
            v = CondOutRange<OUT>::MAXV;
            n_clipped++;
        }
    else if (v < CondOutRange<OUT>::MINV)
        {
            v = CondOutRange<OUT>::MINV;
            n_clipped++;
        }
    return v != v ? 0 : (int)rintf(v);
}

// `count` cbyte outputs from the LDS stage to base (2-byte aligned): dwords from the first 4-byte boundary on
template <int THREADS>
static __device__ __forceinline__ void cond_store_cbyte_range(const unsigned short* stage, char* base, const int count)
{
    if (count <= 0) return;
    const int tid = threadIdx.x;
    const int head = (int)(((uintptr_t)base >> 1) & 1u);  // 1: element 0 lies in the upper half of a dword
    const int n_dw = (count - head) >> 1;
    for (int d = tid; d < n_dw; d += THREADS)
        {
            const int k = head + 2 * d;
            const unsigned w = (unsigned)stage[k] | ((unsigned)stage[k + 1] << 16);
            *reinterpret_cast<unsigned*>(base + 2 * (size_t)k) = w;
        }
    // the ragged ends: at most one element in front of the first boundary and one behind the last whole dword
    if (tid == 0 && head) *reinterpret_cast<unsigned short*>(base) = stage[0];
    const int last = head + 2 * n_dw;
    if (tid == THREADS - 1 && last < count) *reinterpret_cast<unsigned short*>(base + 2 * (size_t)last) = stage[last];
}

// acc[r] is output tid + r * THREADS of the tile; the tile has tn outputs, the first of them is output o0 of the piece.  lds: the
// tile's LDS (at least 2 tn bytes), overwritten when OUT is GC_IQ_I8.
template <int OUT, int R, int THREADS>
static __device__ __forceinline__ void cond_store_tile(float2* lds, const float2 (&acc)[R], const int tn, const unsigned o0, const CondStoreDst& out)
{
    const int tid = threadIdx.x;
    if constexpr (OUT == GC_IQ_F32)
        {
            float2* dst = static_cast<float2*>(out.dst);
            float2* mirror_dst = static_cast<float2*>(out.mirror_dst);
#pragma unroll
            for (int r = 0; r < R; r++)
                {
                    const int jj = tid + r * THREADS;
                    if (jj >= tn) continue;
                    const unsigned o = o0 + (unsigned)jj;
                    dst[o] = acc[r];
                    if (o < out.n_mirror) mirror_dst[o] = acc[r];  // the mirror is written here: no HBM-to-HBM copy follows
                }
        }
    else
        {
            static_assert(OUT == GC_IQ_I16 || OUT == GC_IQ_I8, "unknown output format");
            static_assert(THREADS % 64 == 0, "whole waves");
            __shared__ unsigned cond_clip_wave[THREADS / 64];
            unsigned n_clipped = 0;
            unsigned q[R];
#pragma unroll
            for (int r = 0; r < R; r++)
                {
                    q[r] = 0;
                    if (tid + r * THREADS >= tn) continue;
                    const int re = cond_quantise<OUT>(acc[r].x, out.scale, n_clipped);
                    const int im = cond_quantise<OUT>(acc[r].y, out.scale, n_clipped);
                    q[r] = OUT == GC_IQ_I16 ? (((unsigned)re & 0xffffu) | ((unsigned)im << 16)) : (((unsigned)re & 0xffu) | (((unsigned)im & 0xffu) << 8));
                }
            if constexpr (OUT == GC_IQ_I16)
                {
                    unsigned* dst = static_cast<unsigned*>(out.dst);
                    unsigned* mirror_dst = static_cast<unsigned*>(out.mirror_dst);
#pragma unroll
                    for (int r = 0; r < R; r++)
                        {
                            const int jj = tid + r * THREADS;
                            if (jj >= tn) continue;
                            const unsigned o = o0 + (unsigned)jj;
                            dst[o] = q[r];
                            if (o < out.n_mirror) mirror_dst[o] = q[r];
                        }
                }
            // the wave's count, then the workgroup's
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) n_clipped += __shfl_down(n_clipped, off, 64);
            if constexpr (OUT == GC_IQ_I8) __syncthreads();  // every wave is done reading the tile's inputs
            if ((tid & 63) == 0) cond_clip_wave[tid >> 6] = n_clipped;
            if constexpr (OUT == GC_IQ_I8)
                {
                    unsigned short* stage = reinterpret_cast<unsigned short*>(lds);
#pragma unroll
                    for (int r = 0; r < R; r++)
                        {
                            const int jj = tid + r * THREADS;
                            if (jj < tn) stage[jj] = (unsigned short)q[r];
                        }
                }
            __syncthreads();
            if (tid == 0)
                {
                    unsigned total = 0;
#pragma unroll
                    for (int w = 0; w < THREADS / 64; w++) total += cond_clip_wave[w];
                    if (total != 0) atomicAdd(out.clipped, (unsigned long long)total);
                }
            if constexpr (OUT == GC_IQ_I8)
                {
                    const unsigned short* stage = reinterpret_cast<const unsigned short*>(lds);
                    cond_store_cbyte_range<THREADS>(stage, static_cast<char*>(out.dst) + 2 * (size_t)o0, tn);
                    const int n_m = out.n_mirror > o0 ? (int)min((unsigned)tn, out.n_mirror - o0) : 0;
                    cond_store_cbyte_range<THREADS>(stage, static_cast<char*>(out.mirror_dst) + 2 * (size_t)o0, n_m);
                }
        }
}

#endif
