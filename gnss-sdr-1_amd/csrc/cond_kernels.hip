// cond_kernels.hip -- the signal conditioner's kernel (gfx950): frequency-translating FIR decimator, the device image of the
// reference's Freq_Xlating_Fir_Filter input filter (src/algorithms/input_filter/adapters/freq_xlating_fir_filter.cc):
//
//   y[m] = sum_{k=0}^{T-1} h[k] * x[mD - k] * exp(-j 2 pi phi(mD - k)),   phi(n) = ((n * inc) mod 2^64) >> 32  [2^-32 turns]
//
// One workgroup produces a tile of outputs.  It loads the (tile - 1) D + T raw samples the tile needs with 16-byte loads, converts
// (plain cast) and mixes each of them ONCE, and stores them to LDS in polyphase order: input i of the tile at row i % D, column
// i / D.  Output j, tap k reads input j D + (T - 1 - k), i.e. row (T - 1 - k) % D -- the same for every lane -- and column
// j + (T - 1 - k) / D: the 64 lanes of a wave read 64 consecutive float2 for any D (ds_read_b64, no bank conflict; a flat layout
// would be read with a stride of 2 D dwords, a D-way conflict for D = 2, 4, 8 ...).  Rows are an odd number of float2 long, which
// spreads the D rows a wave's mixed samples are written to over the banks.  The taps are read with uniform (scalar) loads; every
// output accumulates in float32 in tap order k = 0 .. T-1, so an output's bits do not depend on the tile it falls in.
//
// Real raw samples (gc_raw_real_format: float32, int16, int8, 2 bits packed four to a byte) have a front end of their own up to the
// barrier: a 16-byte vector holds 4, 8, 16 or 64 of them, a sample is one field of one of its four dwords (shift and sign
// extension in registers), and the mixer is two products, z = (x cos, -(x sin)) -- what the complex front end gives for (x, 0).
// A lane walks its vector from a start that depends on the lane, so that the 16 lanes that share a ds_write_b64 pass spread over the
// banks (cond_front_real).  The accumulation and the stores are shared code (cond_fir_accum.h, cond_store_epilogue.h); OUT is the
// output ring's format, and the GC_IQ_F32 instantiation stores the accumulators as they are.
#include "cond_kernels.h"
#include "cond_fir_accum.h"
#include "cond_store_epilogue.h"
#include "ring_window.h"

// real formats: BITS per sample, N = 128 / BITS samples in a vector of four dwords
typedef unsigned cond_u32x4 __attribute__((ext_vector_type(4)));
template <int FMT>
struct CondRawReal;
template <>
struct CondRawReal<GC_RAW_REAL_F32>
{
    static constexpr int BITS = 32, N = 4;
};
template <>
struct CondRawReal<GC_RAW_REAL_I16>
{
    static constexpr int BITS = 16, N = 8;
};
template <>
struct CondRawReal<GC_RAW_REAL_I8>
{
    static constexpr int BITS = 8, N = 16;
};
template <>
struct CondRawReal<GC_RAW_REAL_2BIT>
{
    static constexpr int BITS = 2, N = 64;
};
static constexpr bool cond_is_real(int fmt) { return fmt >= GC_RAW_REAL_F32; }

// (cos, sin) of 2 pi phase / 2^32.  The argument reduction is exact: the nearest quarter turn comes from the top bits, the signed
// remainder (|r| <= 2^29) is an angle in [-pi/4, pi/4] that float32 holds to 2^-24 of its size (<= 4.7e-8 rad).  Taylor
// polynomials to x^9 / x^8: truncation below 2.5e-8 on that interval.
static __device__ __forceinline__ float2 cond_cos_sin(unsigned phase)
{
    const unsigned q = (phase + 0x20000000u) >> 30;
    const int r = (int)(phase - (q << 30));
    const float x = (float)r * 1.4629180792671596e-9f;  // (pi / 2) / 2^30
    const float x2 = x * x;
    float s = fmaf(x2, 2.7557319224e-6f, -1.9841269841e-4f);
    s = fmaf(s, x2, 8.3333333333e-3f);
    s = fmaf(s, x2, -1.6666666667e-1f);
    s = fmaf(x * x2, s, x);
    float c = fmaf(x2, 2.4801587302e-5f, -1.3888888889e-3f);
    c = fmaf(c, x2, 4.1666666667e-2f);
    c = fmaf(c, x2, -0.5f);
    c = fmaf(c, x2, 1.0f);
    switch (q & 3u)
        {
        case 0: return float2{c, s};
        case 1: return float2{-s, c};
        case 2: return float2{-c, -s};
        default: return float2{s, -c};
        }
}

// The complex formats' front end: loads, converts and mixes the tile's inputs [a0, a0 + count) into the polyphase LDS image.
template <int FMT, bool MIX>
static __device__ __forceinline__ void cond_front_complex(const CondJob& job, float2* cond_lds, const long long a0, const int count, const int D,
    const int rowlen)
{
    typedef typename RingRaw<FMT>::vec vec;
    constexpr int S = RingRaw<FMT>::N;
    const int tid = threadIdx.x;
    // whole 16-byte vectors from the boundary below a0; those below sample 0 read as zeros
    const long long av = a0 & ~(long long)(S - 1);
    const int n_vec = (int)((a0 + count - av + S - 1) / S);
    const unsigned long long avp = av < 0 ? 0ull : (unsigned long long)av;
    const unsigned base = (unsigned)(avp % job.raw_cap);
    for (int v = tid; v < n_vec; v += GC_COND_THREADS)
        {
            const long long nv = av + (long long)v * S;
            vec raw = vec(0);
            if (nv >= 0)
                {
                    unsigned pos = base + (unsigned)(nv - (long long)avp);  // count + S < raw_cap: at most one wrap
                    if (pos >= job.raw_cap) pos -= job.raw_cap;
                    raw = *reinterpret_cast<const vec*>(static_cast<const char*>(job.raw) + (size_t)pos * RingRaw<FMT>::ELEM);
                }
#pragma unroll
            for (int e = 0; e < S; e++)
                {
                    const int i = (int)(nv + e - a0);
                    if (i < 0 || i >= count) continue;
                    float2 x = float2{(float)raw[2 * e], (float)raw[2 * e + 1]};
                    if (MIX && nv >= 0)
                        {
                            const unsigned phase = (unsigned)((((unsigned long long)(nv + e)) * job.phase_inc) >> 32);
                            const float2 cs = cond_cos_sin(phase);
                            // x * (cos - j sin)
                            x = float2{fmaf(x.x, cs.x, x.y * cs.y), fmaf(x.y, cs.x, -(x.x * cs.y))};
                        }
                    const unsigned row = (unsigned)i % (unsigned)D, col = (unsigned)i / (unsigned)D;
                    cond_lds[row * (unsigned)rowlen + col] = x;
                }
        }
}

// The real formats' front end.  Sample e of a vector is the field of BITS bits at bit e BITS of its four dwords.  A lane takes the S
// samples of its vector in the order e = e0, e0 + 1, ..., S - 1, 0, ..., e0 - 1 with e0 = lane (S >= 16) or lane S / 16 (S < 16):
// a ds_write_b64 is served 16 consecutive lanes at a time over 32 banks, and with e0 = 0 those lanes' float2 indices for D = 1 are
// S apart -- all on one bank pair for S = 16 and 64.  With the skew they are S l + (e0(l) + t) % S: 16 distinct residues mod 16,
// no conflict for D = 1; for D = 2, 4, 8 the 16 lanes spread over D rows of odd length: 2 lanes on a bank pair, up to 4 for
// S = 64 (profiles/tools/cond_lds_bank_model.py; DESIGN.md section 3.3 has the table).  Row and column of the polyphase image and the mixer's phase advance by one sample per
// step -- two divisions and one 64-bit product per vector, none per sample.
template <int FMT, bool MIX>
static __device__ __forceinline__ void cond_front_real(const CondJob& job, float2* cond_lds, const long long a0, const int count, const int D,
    const int rowlen)
{
    constexpr int S = CondRawReal<FMT>::N, BITS = CondRawReal<FMT>::BITS;
    const int tid = threadIdx.x;
    const long long av = a0 & ~(long long)(S - 1);
    const int n_vec = (int)((a0 + count - av + S - 1) / S);
    const unsigned long long avp = av < 0 ? 0ull : (unsigned long long)av;
    const unsigned base = (unsigned)(avp % job.raw_cap);
    const int e0 = S >= 16 ? (tid & (S - 1)) : (((tid & 15) * S) >> 4);
    for (int v = tid; v < n_vec; v += GC_COND_THREADS)
        {
            const long long nv = av + (long long)v * S;
            if (nv < 0)
                {
                    // before the stream began: zeros, unmixed
                    for (int e = 0; e < S; e++)
                        {
                            const int i = (int)(nv + e - a0);
                            if (i >= 0 && i < count) cond_lds[((unsigned)i % (unsigned)D) * (unsigned)rowlen + (unsigned)i / (unsigned)D] = float2{0.0f, 0.0f};
                        }
                    continue;
                }
            unsigned pos = base + (unsigned)(nv - (long long)avp);  // count + 2 S < raw_cap: at most one wrap
            if (pos >= job.raw_cap) pos -= job.raw_cap;
            const cond_u32x4 raw = *reinterpret_cast<const cond_u32x4*>(static_cast<const char*>(job.raw) + (size_t)(pos / S) * 16);
            const int i0 = (int)(nv - a0);  // tile index of the vector's first sample, > -S
            // (row, col) of tile index max(i, 0): of the vector's first sample, and of the sample this lane starts with
            const unsigned u0 = (unsigned)max(i0, 0), us = (unsigned)max(i0 + e0, 0);
            const unsigned col0 = u0 / (unsigned)D, row0 = u0 - col0 * (unsigned)D;
            unsigned col = us / (unsigned)D, row = us - col * (unsigned)D;
            int e = e0, i = i0 + e0;
            unsigned long long ph = MIX ? (unsigned long long)(nv + e0) * job.phase_inc : 0ull;
#pragma unroll 2
            for (int t = 0; t < S; t++)
                {
                    if (i >= 0 && i < count)
                        {
                            const unsigned bit = (unsigned)e * BITS, word = bit >> 5;
                            const unsigned w = word == 0 ? raw.x : word == 1 ? raw.y : word == 2 ? raw.z : raw.w;
                            const float x = BITS == 32 ? __uint_as_float(w) : (float)((int)(w << ((32 - BITS) - (bit & 31u))) >> (32 - BITS));
                            float2 z = float2{x, 0.0f};
                            if (MIX)
                                {
                                    const float2 cs = cond_cos_sin((unsigned)(ph >> 32));
                                    // (x, 0) * (cos - j sin)
                                    z = float2{x * cs.x, -(x * cs.y)};
                                }
                            cond_lds[row * (unsigned)rowlen + col] = z;
                        }
                    // the next sample of the vector; after the last one, its first
                    e++;
                    i++;
                    ph += job.phase_inc;
                    if (++row == (unsigned)D)
                        {
                            row = 0;
                            col++;
                        }
                    if (e == S)
                        {
                            e = 0;
                            i = i0;
                            ph -= (unsigned long long)S * job.phase_inc;
                            row = row0;
                            col = col0;
                        }
                    if (i <= 0) row = col = 0;  // tile index 0 is (0, 0); below it nothing is stored
                }
        }
}

template <int FMT, int OUT, int R, bool MIX>
__global__ __launch_bounds__(GC_COND_THREADS) void cond_fir_decim_kernel(const CondJob job, const int tile, const int rowlen)
{
    extern __shared__ float2 cond_lds[];
    const int tid = threadIdx.x;
    const int D = job.decimation, T = job.n_taps;
    const unsigned o0 = blockIdx.x * (unsigned)tile;  // first output of the tile, counted in the piece
    const int tn = (int)min((unsigned)tile, job.n_out - o0);
    const long long a0 = (long long)(job.first_out + o0) * D - (T - 1);  // absolute number of the tile's first input (< 0: zeros)
    const int count = (tn - 1) * D + T;
    if constexpr (cond_is_real(FMT))
        cond_front_real<FMT, MIX>(job, cond_lds, a0, count, D, rowlen);
    else
        cond_front_complex<FMT, MIX>(job, cond_lds, a0, count, D, rowlen);
    __syncthreads();

    // lanes past the end of a short tile read the last output's samples and store nothing
    int j[R];
#pragma unroll
    for (int r = 0; r < R; r++) j[r] = min(tid + r * GC_COND_THREADS, tn - 1);
    float2 acc[R];
    cond_fir_accumulate<R>(cond_lds, rowlen, D, T, job.taps, j, acc);
    cond_store_tile<OUT, R, GC_COND_THREADS>(cond_lds, acc, tn, o0, job.out);
}

static int cond_rowlen(int decimation, int n_taps, int tile) { return cond_fir_rowlen(decimation, n_taps, tile); }

int cond_tile_outputs(int decimation, int n_taps, unsigned n_out, int want_groups)
{
    int tile = 1024;
    while (tile > 64 && decimation * cond_rowlen(decimation, n_taps, tile) > GC_COND_LDS_SAMPLES) tile /= 2;
    while (tile > GC_COND_THREADS && (n_out + (unsigned)tile - 1) / (unsigned)tile < (unsigned)want_groups) tile /= 2;
    return tile;
}

template <int FMT, int OUT, int R>
static void cond_launch_r(bool mix, dim3 grid, size_t lds_bytes, hipStream_t st, const CondJob& job, int tile, int rowlen)
{
    if (mix)
        hipLaunchKernelGGL((cond_fir_decim_kernel<FMT, OUT, R, true>), grid, dim3(GC_COND_THREADS), lds_bytes, st, job, tile, rowlen);
    else
        hipLaunchKernelGGL((cond_fir_decim_kernel<FMT, OUT, R, false>), grid, dim3(GC_COND_THREADS), lds_bytes, st, job, tile, rowlen);
}

template <int FMT, int OUT>
static void cond_launch_out(dim3 grid, size_t lds_bytes, hipStream_t st, const CondJob& job, int tile, int rowlen)
{
    const bool mix = job.phase_inc != 0;
    if (tile <= GC_COND_THREADS)
        cond_launch_r<FMT, OUT, 1>(mix, grid, lds_bytes, st, job, tile, rowlen);
    else if (tile <= 2 * GC_COND_THREADS)
        cond_launch_r<FMT, OUT, 2>(mix, grid, lds_bytes, st, job, tile, rowlen);
    else
        cond_launch_r<FMT, OUT, 4>(mix, grid, lds_bytes, st, job, tile, rowlen);
}

template <int FMT>
static bool cond_launch_fmt(int out_format, dim3 grid, size_t lds_bytes, hipStream_t st, const CondJob& job, int tile, int rowlen)
{
    switch (out_format)
        {
        case GC_IQ_F32: cond_launch_out<FMT, GC_IQ_F32>(grid, lds_bytes, st, job, tile, rowlen); return true;
        case GC_IQ_I16: cond_launch_out<FMT, GC_IQ_I16>(grid, lds_bytes, st, job, tile, rowlen); return true;
        case GC_IQ_I8: cond_launch_out<FMT, GC_IQ_I8>(grid, lds_bytes, st, job, tile, rowlen); return true;
        default: return false;
        }
}

unsigned cond_raw_align(int iq_format)
{
    switch (iq_format)
        {
        case GC_IQ_F32:
        case GC_IQ_I16:
        case GC_IQ_I8: return 8u;
        case GC_RAW_REAL_F32:
        case GC_RAW_REAL_I16:
        case GC_RAW_REAL_I8:
        case GC_RAW_REAL_2BIT: return 64u;
        default: return 0u;
        }
}

unsigned cond_raw_bits(int iq_format)
{
    switch (iq_format)
        {
        case GC_IQ_F32: return 64u;
        case GC_IQ_I16:
        case GC_RAW_REAL_F32: return 32u;
        case GC_IQ_I8:
        case GC_RAW_REAL_I16: return 16u;
        case GC_RAW_REAL_I8: return 8u;
        case GC_RAW_REAL_2BIT: return 2u;
        default: return 0u;
        }
}

hipError_t cond_launch(int iq_format, int out_format, hipStream_t st, const CondJob& job, int tile)
{
    if (job.n_out == 0) return hipSuccess;
    const unsigned align = cond_raw_align(iq_format);
    if (job.decimation < 1 || job.decimation > GC_COND_MAX_DECIMATION || job.n_taps < 1 || job.n_taps > GC_COND_MAX_TAPS || tile < 64 ||
        tile > 4 * GC_COND_THREADS || align == 0 || job.raw_cap % align != 0)
        return hipErrorInvalidValue;
    if (out_format != GC_IQ_F32 && (job.out.clipped == nullptr || !(job.out.scale > 0.0f))) return hipErrorInvalidValue;
    const int rowlen = cond_rowlen(job.decimation, job.n_taps, tile);
    const size_t lds_samples = (size_t)job.decimation * rowlen;
    // a tile's inputs (plus one vector of slack on each side) must fit in the raw ring without lapping it
    if (lds_samples > GC_COND_LDS_SAMPLES || (size_t)tile * job.decimation + job.n_taps + 2 * align >= job.raw_cap) return hipErrorInvalidValue;
    const dim3 grid((job.n_out + (unsigned)tile - 1) / (unsigned)tile);
    const size_t lds_bytes = lds_samples * sizeof(float2);
    bool ok = false;
    switch (iq_format)
        {
        case GC_IQ_F32: ok = cond_launch_fmt<GC_IQ_F32>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        case GC_IQ_I16: ok = cond_launch_fmt<GC_IQ_I16>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        case GC_IQ_I8: ok = cond_launch_fmt<GC_IQ_I8>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        case GC_RAW_REAL_F32: ok = cond_launch_fmt<GC_RAW_REAL_F32>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        case GC_RAW_REAL_I16: ok = cond_launch_fmt<GC_RAW_REAL_I16>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        case GC_RAW_REAL_I8: ok = cond_launch_fmt<GC_RAW_REAL_I8>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        case GC_RAW_REAL_2BIT: ok = cond_launch_fmt<GC_RAW_REAL_2BIT>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        default: return hipErrorInvalidValue;
        }
    if (!ok) return hipErrorInvalidValue;
    return hipGetLastError();
}
