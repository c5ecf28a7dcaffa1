// trk_closed_loop_mixed.hip -- the closed-loop engine's mixed kernel (gc_trk_loop_set_mixed): one workgroup per channel, each channel
// with its own tap count, pilot mode, code length and code period, all in one launch.  The per-period body is trk_loop_device.hpp's,
// the same as the persistent kernel's (trk_closed_loop.hip).
#include "trk_loop_device.hpp"

// Mixed engines (gc_trk_loop_set_mixed): every channel slot carries its own tap count, pilot mode, code length and period.
// One workgroup per channel as above; after the state copy the workgroup branches once, uniformly, into the body of its
// channel's <3 | 5 taps, data | pilot>.  The kernel's registers are those of its worst body (mixed engines).
template <int THREADS, int FMT, bool HD = false>
__global__ __launch_bounds__(THREADS) void trk_closed_loop_mixed_kernel(LoopChan* __restrict__ chans,
    gc_loop_record* __restrict__ recs, int n_epochs, int lds_table_floats, const unsigned long long* __restrict__ limits, int resident)
{
    extern __shared__ float lds[];
    __shared__ LoopChan s;
    __shared__ gc_epoch_params s_p;
    __shared__ float2 s_corr[GC_MAX_TAPS];
    __shared__ int s_go;
    const int ch = blockIdx.x;
    const int tid = threadIdx.x;
    {
        const unsigned* src = reinterpret_cast<const unsigned*>(&chans[ch]);
        unsigned* dst = reinterpret_cast<unsigned*>(&s);
        for (unsigned i = tid; i < sizeof(LoopChan) / 4; i += THREADS) dst[i] = src[i];
    }
    __syncthreads();
    // the channel's kind, the same for every lane of the workgroup: a scalar branch
    const int kind = __builtin_amdgcn_readfirstlane(s.n_taps == 0 ? 0 : (s.n_taps == 5 ? 2 : 1) + (s.sync.track_pilot ? 2 : 0));
    gc_loop_record* crec = &recs[(size_t)ch * n_epochs];
    if (kind == 0)
        {
            // standby slot (n_taps == 0): all-zero records, nothing else
            for (int e = 0; e < n_epochs; e++)
                {
                    unsigned* w = reinterpret_cast<unsigned*>(&crec[e]);
                    for (unsigned i = tid; i < sizeof(gc_loop_record) / 4; i += THREADS) w[i] = 0u;
                }
            return;
        }
    const unsigned long long limit = limits ? limits[ch] : s.chan.n_iq;
    if (kind == 1) loop_periods<3, THREADS, FMT, false, HD>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
    else if (kind == 2) loop_periods<5, THREADS, FMT, false, HD>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
    else if (kind == 3) loop_periods<3, THREADS, FMT, true, HD>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
    else loop_periods<5, THREADS, FMT, true, HD>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
    __syncthreads();
    {
        unsigned* dst = reinterpret_cast<unsigned*>(&chans[ch]);
        const unsigned* src = reinterpret_cast<const unsigned*>(&s);
        for (unsigned i = tid; i < sizeof(LoopChan) / 4; i += THREADS) dst[i] = src[i];
    }
}

// the mixed kernel of a mixed engine (gc_trk_loop_set_mixed); high-dynamics engines take 256 threads like the persistent kernel
template <int TH, int FM, bool HD>
static hipError_t loop_launch_mixed_t(LoopChan* d_chans, int n_channels, int n_epochs, gc_loop_record* dev_records, hipStream_t st, int lds_table_floats,
    const unsigned long long* limits, int resident)
{
    const size_t lds_bytes = (size_t)(trk_hdr_floats(TH) + lds_table_floats) * sizeof(float);
    if (lds_bytes > 48 * 1024)
        {
            hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&trk_closed_loop_mixed_kernel<TH, FM, HD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                (int)lds_bytes);
            if (ea != hipSuccess) return ea;
        }
    hipLaunchKernelGGL((trk_closed_loop_mixed_kernel<TH, FM, HD>), dim3(n_channels), dim3(TH), lds_bytes, st, d_chans, dev_records, n_epochs,
        lds_table_floats, limits, resident);
    return hipGetLastError();
}

template <int FM>
static hipError_t loop_launch_mixed_f(LoopChan* d_chans, int n_channels, int high_dyn, int threads, int n_epochs, gc_loop_record* dev_records, hipStream_t st,
    int lds_table_floats, const unsigned long long* limits, int resident)
{
    if (high_dyn) return loop_launch_mixed_t<256, FM, true>(d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, limits, resident);
    if (threads == 1024) return loop_launch_mixed_t<1024, FM, false>(d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, limits, resident);
    if (threads == 512) return loop_launch_mixed_t<512, FM, false>(d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, limits, resident);
    return loop_launch_mixed_t<256, FM, false>(d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, limits, resident);
}

hipError_t loop_launch_mixed(LoopChan* d_chans, int n_channels, int iq_format, int high_dyn, int threads, int n_epochs, gc_loop_record* dev_records,
    hipStream_t st, int lds_table_floats, const unsigned long long* limits, int resident)
{
    if (iq_format == GC_IQ_I16)
        return loop_launch_mixed_f<GC_IQ_I16>(d_chans, n_channels, high_dyn, threads, n_epochs, dev_records, st, lds_table_floats, limits, resident);
    if (iq_format == GC_IQ_I8)
        return loop_launch_mixed_f<GC_IQ_I8>(d_chans, n_channels, high_dyn, threads, n_epochs, dev_records, st, lds_table_floats, limits, resident);
    return loop_launch_mixed_f<GC_IQ_F32>(d_chans, n_channels, high_dyn, threads, n_epochs, dev_records, st, lds_table_floats, limits, resident);
}
