// ring_window.h -- how a kernel reads a gc_stream ring of complex samples (gfx950): the 16-byte vector traits of the three
// gc_iq_format values, and the loader of a window of consecutive samples, addressed by absolute sample number, into LDS.
//
// A window [a0, a0 + count) is, apart from the zeros in front of sample 0, at most two contiguous pieces of the ring: the split is
// found once per workgroup (one modulo, uniform: src_cap, a0 and count must be), and each piece is loaded with 16-byte loads from
// its first 16-byte boundary on, with single-sample loads for the < 16 bytes at either ragged end -- the ring's capacity need not
// be a multiple of anything, and nothing past the ring's end (its mirror) is read.  Where entry i of the window goes is the
// caller's: put(i, x) is a functor passed by value and inlined (ring_decim_kernels.hip: the polyphase image; ring_resamp_kernels.hip:
// a flat window).  The conditioner's raw ring is aligned and read differently (cond_kernels.hip); it takes the traits alone.
#ifndef RING_WINDOW_H
#define RING_WINDOW_H
#include "gnsscorr.h"
#include <hip/hip_runtime.h>

typedef float ring_f32x4 __attribute__((ext_vector_type(4)));
typedef short ring_i16x8 __attribute__((ext_vector_type(8)));
typedef signed char ring_i8x16 __attribute__((ext_vector_type(16)));
typedef float ring_f32x2 __attribute__((ext_vector_type(2)));
typedef short ring_i16x2 __attribute__((ext_vector_type(2)));
typedef signed char ring_i8x2 __attribute__((ext_vector_type(2)));

// 16 bytes of samples (N of them, ELEM bytes each), one sample, and one sample as bits
template <int FMT>
struct RingRaw;
template <>
struct RingRaw<GC_IQ_F32>
{
    typedef ring_f32x4 vec;
    typedef ring_f32x2 one;
    typedef uint2 bits;
    static constexpr int N = 2, ELEM = 8;
};
template <>
struct RingRaw<GC_IQ_I16>
{
    typedef ring_i16x8 vec;
    typedef ring_i16x2 one;
    typedef unsigned bits;
    static constexpr int N = 4, ELEM = 4;
};
template <>
struct RingRaw<GC_IQ_I8>
{
    typedef ring_i8x16 vec;
    typedef ring_i8x2 one;
    typedef unsigned short bits;
    static constexpr int N = 8, ELEM = 2;
};

// n samples that are contiguous in the ring from position pos become entries i0 .. i0 + n - 1 of the window
template <int FMT, int THREADS, class Put>
static __device__ __forceinline__ void ring_window_load_piece(const char* ring, unsigned pos, int i0, int n, Put put)
{
    typedef typename RingRaw<FMT>::vec vec;
    typedef typename RingRaw<FMT>::one one;
    constexpr int S = RingRaw<FMT>::N, ELEM = RingRaw<FMT>::ELEM;
    const int tid = threadIdx.x;
    if (n <= 0) return;
    const int head = min((int)((0u - pos) & (unsigned)(S - 1)), n);  // samples in front of the first 16-byte boundary
    const int n_vec = (n - head) / S;
    const int tail0 = head + n_vec * S;
    const vec* vp = reinterpret_cast<const vec*>(ring + (size_t)(pos + (unsigned)head) * ELEM);
    for (int v = tid; v < n_vec; v += THREADS)
        {
            const vec raw = vp[v];
            const int i = i0 + head + v * S;
#pragma unroll
            for (int e = 0; e < S; e++) put(i + e, float2{(float)raw[2 * e], (float)raw[2 * e + 1]});
        }
    const int n_ragged = head + (n - tail0);  // < 2 S <= 16
    if (tid < n_ragged)
        {
            const int k = tid < head ? tid : tail0 + (tid - head);
            const one raw = *reinterpret_cast<const one*>(ring + (size_t)(pos + (unsigned)k) * ELEM);
            put(i0 + k, float2{(float)raw[0], (float)raw[1]});
        }
}

// Samples [a0, a0 + count) of the ring `src` (sample n at n % src_cap; a0 < 0: zeros in front of sample 0) become entries
// 0 .. count - 1 of the window.  What lies at or above sample 0 must be resident: at most src_cap samples.  Every thread of the
// workgroup (THREADS of them) calls it; the caller's barrier follows.
template <int FMT, int THREADS, class Put>
static __device__ __forceinline__ void ring_window_load(const void* src, unsigned src_cap, long long a0, int count, Put put)
{
    const int tid = threadIdx.x;
    const int n_zero = a0 < 0 ? (int)min((long long)count, -a0) : 0;
    for (int i = tid; i < n_zero; i += THREADS) put(i, float2{0.0f, 0.0f});
    // the split: [lo, lo + n) is resident (n <= src_cap), so it wraps at most once
    const unsigned long long lo = a0 < 0 ? 0ull : (unsigned long long)a0;
    const int n = count - n_zero;
    const unsigned pos = (unsigned)(lo % src_cap);
    const int n1 = (int)min((unsigned)n, src_cap - pos);
    const char* ring = static_cast<const char*>(src);
    ring_window_load_piece<FMT, THREADS>(ring, pos, n_zero, n1, put);
    ring_window_load_piece<FMT, THREADS>(ring, 0u, n_zero + n1, n - n1, put);
}

#endif
