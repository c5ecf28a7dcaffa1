// cond_blank_kernels.hip -- pulse blanking on the conditioner's raw ring (gfx950): the device image of the reference's
// Pulse_Blanking_Filter (src/algorithms/input_filter/gnuradio_blocks/pulse_blanking_cc.cc).  Three launches per chunk of raw samples,
// on the output ring's copy stream, between the H2D copy and the FIR decimator:
//
//   1. energies   E[s] = sum over the segment of re^2 + im^2 (x^2 for the real formats; float32, plain cast).  G lanes share a
//                 segment (G: a power of two fixed by the format and L).  The segment is covered by ALIGNED 16-byte vectors of
//                 the ring, counted from the one that holds its first sample; lane g takes vectors g, g + G, ... and adds the
//                 samples of each that belong to the segment in ascending order; the G partial sums meet in a fixed xor
//                 butterfly.  An aligned vector never straddles the ring's wrap (raw_cap is a multiple of 8 samples, of 64 for
//                 the real formats), and the alignment of sample n is n % S whatever the pushes were: the order of the sum is a
//                 function of the segment alone, so E[s] has the same bits however the stream was cut into pushes and chunks.
//   2. decisions  one wave walks the new segments with the state (noise floor, n, last_filtered, counters) in HBM
//                 (cond_blank_decide.h: 64 segments per step in steady mode, the dependent float32 mean by one walk otherwise).
//   3. apply      zeroes the flagged segments in the ring, whole vectors inside, single samples at ragged edges; the FIR kernel
//                 then reads zeros.  Segments that are not flagged are not written.
#include "cond_blank_kernels.h"

typedef float blank_f32x4 __attribute__((ext_vector_type(4)));
typedef short blank_i16x8 __attribute__((ext_vector_type(8)));
typedef signed char blank_i8x16 __attribute__((ext_vector_type(16)));
typedef short blank_i16x2 __attribute__((ext_vector_type(2)));
typedef signed char blank_i8x2 __attribute__((ext_vector_type(2)));

// 16 bytes of raw samples / one raw sample
template <int FMT>
struct BlankRaw;
template <>
struct BlankRaw<GC_IQ_F32>
{
    typedef blank_f32x4 vec;
    typedef float2 one;
    static constexpr int N = 2, ELEM = 8;
};
template <>
struct BlankRaw<GC_IQ_I16>
{
    typedef blank_i16x8 vec;
    typedef blank_i16x2 one;
    static constexpr int N = 4, ELEM = 4;
};
template <>
struct BlankRaw<GC_IQ_I8>
{
    typedef blank_i8x16 vec;
    typedef blank_i8x2 one;
    static constexpr int N = 8, ELEM = 2;
};
// real samples: one component each, E = sum of x^2 (the 2-bit packed format is not blanked: see include/gnsscorr.h)
template <>
struct BlankRaw<GC_RAW_REAL_F32>
{
    typedef blank_f32x4 vec;
    typedef float one;
    static constexpr int N = 4, ELEM = 4;
};
template <>
struct BlankRaw<GC_RAW_REAL_I16>
{
    typedef blank_i16x8 vec;
    typedef short one;
    static constexpr int N = 8, ELEM = 2;
};
template <>
struct BlankRaw<GC_RAW_REAL_I8>
{
    typedef blank_i8x16 vec;
    typedef signed char one;
    static constexpr int N = 16, ELEM = 1;
};
static constexpr bool blank_is_real(int fmt) { return fmt >= GC_RAW_REAL_F32; }

// where a thread's segment lies: samples [a, b), aligned vectors 0 .. nvec - 1 from ring position pos0
struct BlankSpan
{
    unsigned long long a, b, av;
    unsigned nvec, pos0;
};

template <int S>
static __device__ __forceinline__ BlankSpan blank_span(const BlankJob& job, unsigned sl)
{
    BlankSpan sp;
    sp.a = (job.seg0 + sl) * (unsigned long long)job.length;
    sp.b = sp.a + job.length;
    sp.av = sp.a & ~(unsigned long long)(S - 1);
    sp.nvec = (unsigned)((sp.b - sp.av + (S - 1)) / S);
    sp.pos0 = (unsigned)(sp.av % job.raw_cap);
    return sp;
}

template <int FMT>
__global__ __launch_bounds__(GC_BLANK_THREADS) void cond_blank_energy_kernel(const BlankJob job, const int G)
{
    typedef typename BlankRaw<FMT>::vec vec;
    constexpr int S = BlankRaw<FMT>::N;
    const unsigned per_group = GC_BLANK_THREADS / (unsigned)G;
    const unsigned sl = blockIdx.x * per_group + threadIdx.x / (unsigned)G;  // segment of the job
    const unsigned g = threadIdx.x % (unsigned)G;
    float acc = 0.0f;
    if (sl < job.n_seg)
        {
            const BlankSpan sp = blank_span<S>(job, sl);
            for (unsigned v = g; v < sp.nvec; v += (unsigned)G)
                {
                    unsigned pos = sp.pos0 + v * S;  // L + two vectors of slack < raw_cap (cond_blank_launch): at most one wrap
                    if (pos >= job.raw_cap) pos -= job.raw_cap;
                    const vec raw = *reinterpret_cast<const vec*>(static_cast<const char*>(job.raw) + (size_t)pos * BlankRaw<FMT>::ELEM);
                    const unsigned long long nv = sp.av + (unsigned long long)v * S;
#pragma unroll
                    for (int e = 0; e < S; e++)
                        {
                            const unsigned long long n = nv + e;
                            if (n < sp.a || n >= sp.b) continue;
                            if constexpr (blank_is_real(FMT))
                                {
                                    const float x = (float)raw[e];
                                    acc += x * x;
                                }
                            else
                                {
                                    const float re = (float)raw[2 * e], im = (float)raw[2 * e + 1];
                                    acc += re * re + im * im;
                                }
                        }
                }
        }
    // fixed tree over the G lanes of the segment (every lane of the wave takes part)
    for (int m = G >> 1; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
    if (sl < job.n_seg && g == 0) job.energies[sl] = acc;
}

__global__ __launch_bounds__(64) void cond_blank_decide_kernel(const BlankJob job)
{
    const unsigned lane = threadIdx.x;
    const BlankParams p = job.params;
    BlankState st = *job.state;  // the same in every lane
    const unsigned count = job.n_seg;
    unsigned i = 0;
    float e = lane < count ? job.energies[lane] : 0.0f;
    while (i < count)
        {
            const unsigned cnt = min(64u, count - i);
            // the next 64 energies, in flight while these are decided (used when all 64 stand)
            const float e_next = i + 64u + lane < count ? job.energies[i + 64u + lane] : 0.0f;
            unsigned long long flags = 0ull;
            unsigned done = 0;
            if (st.n >= p.segments_est)
                {
                    flags = __ballot(lane < cnt && blank_lane_flag(e, st.noise, p.threshold));
                    done = blank_wave_commit(st, p, flags, cnt);
                }
            else
                {
                    // the running mean is a dependent chain: every lane walks it on the same values (one lane's work)
                    while (done < cnt && st.n < p.segments_est)
                        {
                            const float ej = __shfl(e, (int)done);
                            flags |= (unsigned long long)blank_seq_step(st, p, ej) << done;
                            done++;
                        }
                }
            if (lane < done) job.flags[i + lane] = (unsigned char)((flags >> lane) & 1ull);
            i += done;
            if (done == 64u)
                e = e_next;
            else
                e = i + lane < count ? job.energies[i + lane] : 0.0f;
        }
    if (lane == 0) *job.state = st;
}

template <int FMT>
__global__ __launch_bounds__(GC_BLANK_THREADS) void cond_blank_apply_kernel(const BlankJob job, const int G)
{
    typedef typename BlankRaw<FMT>::vec vec;
    typedef typename BlankRaw<FMT>::one one;
    constexpr int S = BlankRaw<FMT>::N;
    const unsigned per_group = GC_BLANK_THREADS / (unsigned)G;
    const unsigned sl = blockIdx.x * per_group + threadIdx.x / (unsigned)G;
    const unsigned g = threadIdx.x % (unsigned)G;
    if (sl >= job.n_seg || job.flags[sl] == 0) return;
    const BlankSpan sp = blank_span<S>(job, sl);
    for (unsigned v = g; v < sp.nvec; v += (unsigned)G)
        {
            unsigned pos = sp.pos0 + v * S;
            if (pos >= job.raw_cap) pos -= job.raw_cap;
            char* at = static_cast<char*>(job.raw) + (size_t)pos * BlankRaw<FMT>::ELEM;
            const unsigned long long nv = sp.av + (unsigned long long)v * S;
            if (nv >= sp.a && nv + S <= sp.b)
                *reinterpret_cast<vec*>(at) = vec(0);
            else
                {
#pragma unroll
                    for (int e = 0; e < S; e++)
                        {
                            const unsigned long long n = nv + e;
                            if (n >= sp.a && n < sp.b) reinterpret_cast<one*>(at)[e] = one{};
                        }
                }
        }
}

// samples in a 16-byte vector; 0: the format is not blanked
static unsigned blank_vec_samples(int iq_format)
{
    switch (iq_format)
        {
        case GC_IQ_F32: return 2u;
        case GC_IQ_I16:
        case GC_RAW_REAL_F32: return 4u;
        case GC_IQ_I8:
        case GC_RAW_REAL_I16: return 8u;
        case GC_RAW_REAL_I8: return 16u;
        default: return 0u;
        }
}

int cond_blank_lanes(int iq_format, unsigned length)
{
    const unsigned S = blank_vec_samples(iq_format);
    if (S == 0) return 0;
    const unsigned vecs = (length + S - 1) / S;
    int G = 1;
    while (G < 64 && (unsigned)G < vecs) G *= 2;
    return G;
}

template <int FMT>
static void cond_blank_launch_fmt(hipStream_t st, const BlankJob& job, int G)
{
    const unsigned per_group = GC_BLANK_THREADS / (unsigned)G;
    const dim3 grid((job.n_seg + per_group - 1) / per_group);
    hipLaunchKernelGGL((cond_blank_energy_kernel<FMT>), grid, dim3(GC_BLANK_THREADS), 0, st, job, G);
    hipLaunchKernelGGL(cond_blank_decide_kernel, dim3(1), dim3(64), 0, st, job);
    hipLaunchKernelGGL((cond_blank_apply_kernel<FMT>), grid, dim3(GC_BLANK_THREADS), 0, st, job, G);
}

hipError_t cond_blank_launch(int iq_format, hipStream_t st, const BlankJob& job)
{
    if (job.n_seg == 0) return hipSuccess;
    // the raw ring's alignment and the slack of one vector on each side of a segment, per format as in cond_launch
    const unsigned align = blank_is_real(iq_format) ? 64u : 8u;
    if (blank_vec_samples(iq_format) == 0 || job.length < 1 || job.length > GC_COND_MAX_BLANK_LENGTH || job.raw_cap % align != 0 ||
        job.length + 2u * align >= job.raw_cap)
        return hipErrorInvalidValue;
    const int G = cond_blank_lanes(iq_format, job.length);
    switch (iq_format)
        {
        case GC_IQ_F32: cond_blank_launch_fmt<GC_IQ_F32>(st, job, G); break;
        case GC_IQ_I16: cond_blank_launch_fmt<GC_IQ_I16>(st, job, G); break;
        case GC_IQ_I8: cond_blank_launch_fmt<GC_IQ_I8>(st, job, G); break;
        case GC_RAW_REAL_F32: cond_blank_launch_fmt<GC_RAW_REAL_F32>(st, job, G); break;
        case GC_RAW_REAL_I16: cond_blank_launch_fmt<GC_RAW_REAL_I16>(st, job, G); break;
        case GC_RAW_REAL_I8: cond_blank_launch_fmt<GC_RAW_REAL_I8>(st, job, G); break;
        default: return hipErrorInvalidValue;
        }
    return hipGetLastError();
}
