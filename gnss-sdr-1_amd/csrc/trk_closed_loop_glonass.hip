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
    loop_channel<THREADS>(s, chans, recs, n_epochs, limits, [&] { return s.n_taps != 3; }, [&](gc_loop_record* crec, unsigned long long limit) {
        loop_periods<GloLoopKind, THREADS, FMT>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, 1);
    });
}

hipError_t glo_loop_launch(const LoopLaunch& a, int iq_format)
{
    return trk_switch_format(iq_format, [&](auto fm) {
        return trk_switch_threads(a.plan.threads, false, [&](auto th, auto) { return loop_launch_kernel(trk_closed_loop_glonass_kernel<th(), fm()>, th(), a); });
    });
}
