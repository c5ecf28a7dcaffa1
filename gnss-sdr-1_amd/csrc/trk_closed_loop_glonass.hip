// trk_closed_loop_glonass.hip -- closed-loop GLONASS L1 / L2 C/A tracking on the GPU (gc_trk_loop_start_glonass).
//
// One workgroup per channel runs n_epochs code periods back to back, like trk_closed_loop_kernel: the E / P / L multicorrelator of
// trk_device.hpp over the period's block, then -- on one lane -- the scalar maths of the reference's GLONASS block
// (trk_glonass_loop_device.hpp).  The replica is real: the reference's complex chips are (+-1, 0), so every tap equals the
// complex-chip result up to the sign of a zero.  The 511-chip replica always sits in LDS as the doubled resident image
// (2 * 511 + 64 floats, loaded once per launch); there is no per-period window mode.  The block length changes from period to
// period (round()-ed with the code NCO command folded in), so the correlator's n_samples is the channel's own
// current_prn_length_samples, at most 2 * vector_length.
#include "trk_glonass_loop_device.hpp"

template <int THREADS, int FMT>
__global__ __launch_bounds__(THREADS) void trk_closed_loop_glonass_kernel(GloChan* __restrict__ chans, gc_loop_record* __restrict__ recs, int n_epochs,
    int lds_table_floats, const unsigned long long* __restrict__ limits)
{
    extern __shared__ float lds[];
    __shared__ GloChan s;
    __shared__ gc_epoch_params s_p;
    __shared__ float2 s_corr[GC_MAX_TAPS];
    __shared__ int s_go;
    const int ch = blockIdx.x;
    const int tid = threadIdx.x;
    {
        // cooperative copy of the channel state into LDS
        const unsigned* src = reinterpret_cast<const unsigned*>(&chans[ch]);
        unsigned* dst = reinterpret_cast<unsigned*>(&s);
        for (unsigned i = tid; i < sizeof(GloChan) / 4; i += THREADS) dst[i] = src[i];
    }
    __syncthreads();
    gc_loop_record* crec = &recs[(size_t)ch * n_epochs];
    if (s.n_taps != 3)
        {
            // a channel that has not been started (or was stopped): standby records, nothing else
            for (int e = 0; e < n_epochs; e++)
                {
                    unsigned* w = reinterpret_cast<unsigned*>(&crec[e]);
                    for (unsigned i = tid; i < sizeof(gc_loop_record) / 4; i += THREADS) w[i] = 0u;
                }
            return;
        }
    // samples available to this launch: the channel's buffer length, or (ring input) the stream's head
    const unsigned long long limit = limits ? limits[ch] : s.chan.n_iq;
    trk_fill_resident<THREADS>(lds, s.chan.code, nullptr, s.chan.code_len);
    __syncthreads();
    for (int e = 0; e < n_epochs; e++)
        {
            gc_loop_record* rec = &crec[e];
            if (tid == 0) s_go = glo_loop_prepare(s, limit, s_p, rec);
            __syncthreads();
            if (!s_go) continue;  // uniform: the state did not change, so every later epoch of this launch is skipped the same way

            const float2 r = trk_epoch<3, false, false, FMT, false, false, THREADS, false, LOOP_PF, false, LOOP_NT != 0, LOOP_WHOLE != 0>(s.chan, s_p, 0, 1, lds_table_floats, lds,
                LOOP_ALIGN_PAIRS, true);
            if (tid < 3) s_corr[tid] = r;
            __syncthreads();

            if (tid == 0) glo_loop_after_correlation(s, s_corr, rec);
            // the next iteration's barrier orders these writes before any other thread reads s / s_p again
        }
    __syncthreads();
    {
        unsigned* dst = reinterpret_cast<unsigned*>(&chans[ch]);
        const unsigned* src = reinterpret_cast<const unsigned*>(&s);
        for (unsigned i = tid; i < sizeof(GloChan) / 4; i += THREADS) dst[i] = src[i];
    }
}

template <int TH, int FM>
static hipError_t glo_launch_k(GloChan* d_chans, int n_channels, int n_epochs, gc_loop_record* dev_records, hipStream_t st, int lds_table_floats, size_t lds_bytes,
    const unsigned long long* limits)
{
    hipLaunchKernelGGL((trk_closed_loop_glonass_kernel<TH, FM>), dim3(n_channels), dim3(TH), lds_bytes, st, d_chans, dev_records, n_epochs, lds_table_floats, limits);
    return hipGetLastError();
}
template <int FM>
static hipError_t glo_launch_t(int threads, GloChan* d_chans, int n_channels, int n_epochs, gc_loop_record* dev_records, hipStream_t st, int lds_table_floats,
    size_t lds_bytes, const unsigned long long* limits)
{
    if (threads == 1024) return glo_launch_k<1024, FM>(d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, lds_bytes, limits);
    if (threads == 512) return glo_launch_k<512, FM>(d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, lds_bytes, limits);
    return glo_launch_k<256, FM>(d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, lds_bytes, limits);
}

hipError_t glo_loop_launch(GloChan* d_chans, int n_channels, int iq_format, int threads, int n_epochs, gc_loop_record* dev_records, hipStream_t st,
    int lds_table_floats, size_t lds_bytes, const unsigned long long* limits)
{
    if (iq_format == GC_IQ_I16) return glo_launch_t<GC_IQ_I16>(threads, d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, lds_bytes, limits);
    if (iq_format == GC_IQ_I8) return glo_launch_t<GC_IQ_I8>(threads, d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, lds_bytes, limits);
    return glo_launch_t<GC_IQ_F32>(threads, d_chans, n_channels, n_epochs, dev_records, st, lds_table_floats, lds_bytes, limits);
}
