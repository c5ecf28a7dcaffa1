// ring_resamp_kernels.hip -- the ring resampler's kernels (gfx950): one gc_stream ring derived from another at an arbitrary rate
// ratio.  Which source sample an output is, is resamp_index.h's closed form of the output's absolute number, split by the host into
// a 128-bit base (q0, r0) per launch and 64-bit offsets per lane; nothing is carried from launch to launch.
//
//   direct     out[m] = x[n_m], bits as they are (the reference's Direct_Resampler: nearest earlier sample, no filter).  A gather:
//              one workgroup of 256 lanes per 256 outputs; the tile's first source sample is reduced to a ring position with one
//              64-bit modulo, uniform, and each lane adds its distance from it and folds once.
//   polyphase  y[m] = sum_{k=0}^{T-1} H[p_m][k] x[n_m - k],  x[n] = 0 for n < 0, plain cast, H[p][0] x first and then one fmaf per
//              tap in k order.  The tile's source window [n_first - (T - 1), n_last] is, apart from the zeros in front of sample
//              0, at most two contiguous pieces of the ring: ring_window.h's loader, which the ring decimator shares, reads
//              nothing behind the ring's end, so any capacity works.  Window (float2) and bank (odd row pitch) lie in LDS; after one barrier lane j
//              accumulates output j with its own phase row.  An output's bits are a function of its T source samples and its tap
//              row alone.
#include "ring_resamp_kernels.h"
#include "ring_window.h"
#include <algorithm>

template <int FMT>
__global__ __launch_bounds__(GC_RRES_THREADS) void ring_resamp_direct_kernel(const RingResampJob job)
{
    typedef typename RingRaw<FMT>::bits bits;
    const unsigned o0 = blockIdx.x * (unsigned)GC_RRES_THREADS;  // first output of the tile, counted in the piece
    const unsigned j = o0 + threadIdx.x;
    // the wrap split: once per tile
    const unsigned long long n_tile = resamp_offset_index(job.kind, job.step, job.q0, job.r0, o0);
    const unsigned pos_tile = (unsigned)(n_tile % job.src_cap);
    if (j >= job.n_out) return;
    const unsigned long long n = resamp_offset_index(job.kind, job.step, job.q0, job.r0, j);
    // the piece's source samples are resident: n - n_tile < src_cap < 2^31, so one fold
    unsigned pos = pos_tile + (unsigned)(n - n_tile);
    if (pos >= job.src_cap) pos -= job.src_cap;
    const bits v = static_cast<const bits*>(job.src)[pos];
    static_cast<bits*>(job.out.dst)[j] = v;
    if (j < job.out.n_mirror) static_cast<bits*>(job.out.mirror_dst)[j] = v;
}

// entry i of the window to its place: the window is flat
struct RresLinearPut
{
    float2* win;
    __device__ __forceinline__ void operator()(int i, float2 x) const { win[i] = x; }
};

// the accumulation of cond_fir_accum.h with a tap row per lane: h[0] x first, then one fmaf per tap in the order k = 1 .. T-1.
// x points at the window entry of source sample n_m; tap k reads the entry k in front of it.
static __device__ __forceinline__ float2 rres_accumulate(const float2* x, const float* h, const int T)
{
    float2 acc;
    {
        const float2 v = x[0];
        acc = float2{h[0] * v.x, h[0] * v.y};
    }
    for (int k = 1; k < T; k++)
        {
            const float2 v = x[-k];
            acc.x = fmaf(h[k], v.x, acc.x);
            acc.y = fmaf(h[k], v.y, acc.y);
        }
    return acc;
}

template <int FMT>
__global__ __launch_bounds__(GC_RRES_THREADS) void ring_resamp_poly_kernel(const RingResampJob job, const int tile, const int win_cap)
{
    extern __shared__ __attribute__((aligned(16))) float2 rres_lds[];
    float2* win = rres_lds;                                        // win_cap entries
    float* bank = reinterpret_cast<float*>(rres_lds + win_cap);    // phases rows of pitch floats
    const int tid = threadIdx.x;
    const int T = job.taps, pitch = ring_resamp_bank_pitch(T);
    const unsigned o0 = blockIdx.x * (unsigned)tile;  // first output of the tile, counted in the piece
    const int tn = (int)min((unsigned)tile, job.n_out - o0);
    const unsigned long long n_first = resamp_offset_index(RESAMP_POLY, job.step, job.q0, job.r0, o0);
    const unsigned long long n_last = resamp_offset_index(RESAMP_POLY, job.step, job.q0, job.r0, o0 + (unsigned)(tn - 1));
    const long long a0 = (long long)n_first - (T - 1);  // absolute number of the window's first entry (< 0: zeros)
    const int count = (int)(n_last - n_first) + T;       // <= win_cap (ring_resamp_window)
    ring_window_load<FMT, GC_RRES_THREADS>(job.src, job.src_cap, a0, count, RresLinearPut{win});
    const int n_bank = pitch << job.log2_phases;
    for (int i = tid; i < n_bank; i += GC_RRES_THREADS) bank[i] = job.bank[i];
    __syncthreads();
    if (tid >= tn) return;

    const unsigned j = o0 + (unsigned)tid;
    const unsigned long long nm = resamp_offset_index(RESAMP_POLY, job.step, job.q0, job.r0, j);
    const unsigned p = resamp_offset_phase(job.step, job.log2_phases, job.r0, j);
    const float2 y = rres_accumulate(win + (int)(nm - n_first) + (T - 1), bank + p * (unsigned)pitch, T);
    static_cast<float2*>(job.out.dst)[j] = y;
    if (j < job.out.n_mirror) static_cast<float2*>(job.out.mirror_dst)[j] = y;
}

static size_t rres_lds_bytes(unsigned long long inc, int taps, int phases, int tile)
{
    return (size_t)ring_resamp_window(inc, taps, tile) * sizeof(float2) + (size_t)phases * ring_resamp_bank_pitch(taps) * sizeof(float);
}

int ring_resamp_tile_outputs(unsigned long long inc, int taps, int phases, unsigned n_out, int want_groups)
{
    int tile = GC_RRES_THREADS;
    while (tile > 16 && rres_lds_bytes(inc, taps, phases, tile) > GC_RRES_LDS_BYTES) tile /= 2;
    if (rres_lds_bytes(inc, taps, phases, tile) > GC_RRES_LDS_BYTES) return 0;
    while (tile > 64 && (n_out + (unsigned)tile - 1) / (unsigned)tile < (unsigned)want_groups) tile /= 2;
    return tile;
}

// the last output's distance from the first, in source samples; false when the offsets leave 64 bits or the distance the ring
static bool rres_span(const RingResampJob& job, unsigned long long* span)
{
    const ResampRatio r = {job.kind, job.step};
    const ResampBase b = {job.q0, job.r0};
    if (job.kind != RESAMP_IDENTITY && job.step == 0) return false;
    if (!resamp_offsets_fit(r, b, job.n_out)) return false;
    *span = resamp_offset_index(job.kind, job.step, job.q0, job.r0, job.n_out - 1) - resamp_offset_index(job.kind, job.step, job.q0, job.r0, 0);
    return true;
}

hipError_t ring_resamp_direct_launch(int iq_format, hipStream_t st, const RingResampJob& job)
{
    if (job.n_out == 0) return hipSuccess;
    if (job.kind < RESAMP_IDENTITY || job.kind > RESAMP_UP || job.src_cap == 0 || job.src == nullptr || job.out.dst == nullptr ||
        (job.out.n_mirror > 0 && job.out.mirror_dst == nullptr) || job.out.n_mirror > job.n_out)
        return hipErrorInvalidValue;
    // what the piece reads, [n_first, n_last], must not lap the source ring
    unsigned long long span = 0;
    if (!rres_span(job, &span) || span >= job.src_cap) return hipErrorInvalidValue;
    const dim3 grid((job.n_out + GC_RRES_THREADS - 1) / GC_RRES_THREADS), block(GC_RRES_THREADS);
    switch (iq_format)
        {
        case GC_IQ_F32: hipLaunchKernelGGL((ring_resamp_direct_kernel<GC_IQ_F32>), grid, block, 0, st, job); break;
        case GC_IQ_I16: hipLaunchKernelGGL((ring_resamp_direct_kernel<GC_IQ_I16>), grid, block, 0, st, job); break;
        case GC_IQ_I8: hipLaunchKernelGGL((ring_resamp_direct_kernel<GC_IQ_I8>), grid, block, 0, st, job); break;
        default: return hipErrorInvalidValue;
        }
    return hipGetLastError();
}

hipError_t ring_resamp_poly_launch(int iq_format, hipStream_t st, const RingResampJob& job, int tile)
{
    if (job.n_out == 0) return hipSuccess;
    const int phases = 1 << job.log2_phases;
    if (job.kind != RESAMP_POLY || job.log2_phases < 0 || phases > GC_RRES_MAX_PHASES || job.taps < 1 || job.taps > GC_RRES_MAX_TAPS ||
        phases * job.taps > GC_RRES_MAX_BANK || tile < 16 || tile > GC_RRES_THREADS || (tile & (tile - 1)) != 0 || job.src_cap == 0 || job.src == nullptr ||
        job.bank == nullptr || job.out.dst == nullptr || (job.out.n_mirror > 0 && job.out.mirror_dst == nullptr) || job.out.n_mirror > job.n_out)
        return hipErrorInvalidValue;
    const size_t lds_bytes = rres_lds_bytes(job.step, job.taps, phases, tile);
    if (lds_bytes > GC_RRES_LDS_BYTES) return hipErrorInvalidValue;
    // what the piece reads, [max(0, n_first - (T - 1)), n_last], must not lap the source ring
    unsigned long long span = 0;
    if (!rres_span(job, &span)) return hipErrorInvalidValue;
    const unsigned long long history = std::min<unsigned long long>((unsigned long long)(job.taps - 1), job.q0);
    if (span + history >= job.src_cap) return hipErrorInvalidValue;
    const dim3 grid((job.n_out + (unsigned)tile - 1) / (unsigned)tile), block(GC_RRES_THREADS);
    const int win_cap = (int)ring_resamp_window(job.step, job.taps, tile);
    switch (iq_format)
        {
        case GC_IQ_F32: hipLaunchKernelGGL((ring_resamp_poly_kernel<GC_IQ_F32>), grid, block, lds_bytes, st, job, tile, win_cap); break;
        case GC_IQ_I16: hipLaunchKernelGGL((ring_resamp_poly_kernel<GC_IQ_I16>), grid, block, lds_bytes, st, job, tile, win_cap); break;
        case GC_IQ_I8: hipLaunchKernelGGL((ring_resamp_poly_kernel<GC_IQ_I8>), grid, block, lds_bytes, st, job, tile, win_cap); break;
        default: return hipErrorInvalidValue;
        }
    return hipGetLastError();
}
