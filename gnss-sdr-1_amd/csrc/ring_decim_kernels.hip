// ring_decim_kernels.hip -- FIR decimator from a gc_stream ring into a gc_stream ring (gfx950): the device image of the
// fir_filter_ccf the reference puts in front of its acquisition blocks when GNSS-SDR.use_acquisition_resampler is set
// (src/core/receiver/gnss_flowgraph.cc:375-499):
//
//   y[m] = sum_{k=0}^{T-1} h[k] * x[mD - k]        x[n] = 0 for n < 0, plain cast, float32 products and sums, k ascending
//
// One workgroup produces a tile of outputs.  Its input window [m0 D - (T - 1), (m0 + tile - 1) D] is, apart from the zeros in front
// of sample 0, at most two contiguous pieces of the source ring: ring_window.h's loader finds the split once per tile and reads
// nothing past the ring's end (its mirror), whatever the ring's capacity.
// Samples go to LDS in the conditioner's polyphase order, are accumulated by the conditioner's code (cond_fir_accum.h) and stored by
// its epilogue (cond_store_epilogue.h; OUT is the output ring's format), so an output's bits are a function of the source samples alone.
#include "ring_decim_kernels.h"
#include "cond_fir_accum.h"
#include "cond_store_epilogue.h"
#include "ring_window.h"
#include <algorithm>

// input i of the tile to its polyphase place
struct RdecPolyphasePut
{
    float2* lds;
    unsigned rowlen, D;
    __device__ __forceinline__ void operator()(int i, float2 x) const
    {
        const unsigned row = (unsigned)i % D, col = (unsigned)i / D;
        lds[row * rowlen + col] = x;
    }
};

template <int FMT, int OUT>
__global__ __launch_bounds__(GC_RDEC_THREADS) void ring_decim_kernel(const RingDecimJob job, const int tile, const int rowlen)
{
    extern __shared__ float2 rdec_lds[];
    const int tid = threadIdx.x;
    const int D = job.decimation, T = job.n_taps;
    const unsigned o0 = blockIdx.x * (unsigned)tile;  // first output of the tile, counted in the piece
    const int tn = (int)min((unsigned)tile, job.n_out - o0);
    const long long a0 = (long long)(job.first_out + o0) * D - (T - 1);  // absolute number of the tile's first input (< 0: zeros)
    const int count = (tn - 1) * D + T;
    ring_window_load<FMT, GC_RDEC_THREADS>(job.src, job.src_cap, a0, count, RdecPolyphasePut{rdec_lds, (unsigned)rowlen, (unsigned)D});
    __syncthreads();
    // the integer epilogues hold barriers: there the lanes past the end of a short tile stay, read the last output's samples and
    // store nothing
    if constexpr (OUT == GC_IQ_F32)
        if (tid >= tn) return;

    int j[1] = {min(tid, tn - 1)};
    float2 acc[1];
    cond_fir_accumulate<1>(rdec_lds, rowlen, D, T, job.taps, j, acc);
    cond_store_tile<OUT, 1, GC_RDEC_THREADS>(rdec_lds, acc, tn, o0, job.out);
}

int ring_decim_tile_outputs(int decimation, int n_taps, unsigned n_out, int want_groups)
{
    int tile = GC_RDEC_THREADS;
    while (tile > 64 && (decimation * cond_fir_rowlen(decimation, n_taps, tile) > GC_COND_LDS_SAMPLES ||
                            (n_out + (unsigned)tile - 1) / (unsigned)tile < (unsigned)want_groups))
        tile /= 2;
    return tile;
}

template <int FMT>
static bool ring_decim_launch_fmt(int out_format, dim3 grid, size_t lds_bytes, hipStream_t st, const RingDecimJob& job, int tile, int rowlen)
{
    switch (out_format)
        {
        case GC_IQ_F32: hipLaunchKernelGGL((ring_decim_kernel<FMT, GC_IQ_F32>), grid, dim3(GC_RDEC_THREADS), lds_bytes, st, job, tile, rowlen); return true;
        case GC_IQ_I16: hipLaunchKernelGGL((ring_decim_kernel<FMT, GC_IQ_I16>), grid, dim3(GC_RDEC_THREADS), lds_bytes, st, job, tile, rowlen); return true;
        case GC_IQ_I8: hipLaunchKernelGGL((ring_decim_kernel<FMT, GC_IQ_I8>), grid, dim3(GC_RDEC_THREADS), lds_bytes, st, job, tile, rowlen); return true;
        default: return false;
        }
}

hipError_t ring_decim_launch(int iq_format, int out_format, hipStream_t st, const RingDecimJob& job, int tile)
{
    if (job.n_out == 0) return hipSuccess;
    if (job.decimation < 1 || job.decimation > GC_COND_MAX_DECIMATION || job.n_taps < 1 || job.n_taps > GC_COND_MAX_TAPS ||
        (tile != 64 && tile != 128 && tile != 256) || job.src_cap == 0 || job.src == nullptr || job.taps == nullptr)
        return hipErrorInvalidValue;
    if (out_format != GC_IQ_F32 && (job.out.clipped == nullptr || !(job.out.scale > 0.0f))) return hipErrorInvalidValue;
    const int rowlen = cond_fir_rowlen(job.decimation, job.n_taps, tile);
    const size_t lds_samples = (size_t)job.decimation * rowlen;
    // the longest window of the launch, clipped at sample 0, must not lap the source ring
    const unsigned long long widest = (unsigned long long)(std::min<unsigned>((unsigned)tile, job.n_out) - 1) * job.decimation + job.n_taps;
    const unsigned long long last_in = (job.first_out + job.n_out - 1) * (unsigned long long)job.decimation;
    if (lds_samples > GC_COND_LDS_SAMPLES || std::min(widest, last_in + 1) > job.src_cap) return hipErrorInvalidValue;
    const dim3 grid((job.n_out + (unsigned)tile - 1) / (unsigned)tile);
    const size_t lds_bytes = lds_samples * sizeof(float2);
    bool ok = false;
    switch (iq_format)
        {
        case GC_IQ_F32: ok = ring_decim_launch_fmt<GC_IQ_F32>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        case GC_IQ_I16: ok = ring_decim_launch_fmt<GC_IQ_I16>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        case GC_IQ_I8: ok = ring_decim_launch_fmt<GC_IQ_I8>(out_format, grid, lds_bytes, st, job, tile, rowlen); break;
        default: return hipErrorInvalidValue;
        }
    if (!ok) return hipErrorInvalidValue;
    return hipGetLastError();
}
