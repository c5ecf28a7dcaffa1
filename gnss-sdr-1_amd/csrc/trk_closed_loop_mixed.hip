// trk_closed_loop_mixed.hip -- the closed-loop engine's mixed kernel (gc_trk_loop_set_mixed): one workgroup per channel, each channel
// with its own tap count, pilot mode, code length and code period, all in one launch.  The per-period body is trk_loop_device.hpp's,
// the same as the persistent kernel's (trk_closed_loop.hip).
#include "trk_loop_device.hpp"

// Mixed engines (gc_trk_loop_set_mixed): every channel slot carries its own tap count, pilot mode, code length and period.
// One workgroup per channel in the engine's shell (loop_channel); once the state is loaded the workgroup branches, uniformly, into
// the period loop of its channel's <3 | 5 taps, data | pilot>.  The kernel's registers are those of its worst body (mixed engines).
template <int THREADS, int FMT, bool HD = false>
__global__ __launch_bounds__(THREADS) void trk_closed_loop_mixed_kernel(LoopChan* __restrict__ chans,
    gc_loop_record* __restrict__ recs, int n_epochs, int lds_table_floats, const unsigned long long* __restrict__ limits, int resident)
{
    extern __shared__ float lds[];
    __shared__ LoopChan s;
    __shared__ gc_epoch_params s_p;
    __shared__ float2 s_corr[GC_MAX_TAPS];
    __shared__ int s_go;
    int kind;  // of the channel, the same for every lane of the workgroup: a scalar branch
    loop_channel<THREADS>(
        s, chans, recs, n_epochs, limits,
        [&] {
            kind = __builtin_amdgcn_readfirstlane(s.n_taps == 0 ? 0 : (s.n_taps == 5 ? 2 : 1) + (s.sync.track_pilot ? 2 : 0));
            return kind == 0;  // standby slot (n_taps == 0)
        },
        [&](gc_loop_record* crec, unsigned long long limit) {
            if (kind == 1) loop_periods<VemlLoopKind<3, false, HD>, THREADS, FMT>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
            else if (kind == 2) loop_periods<VemlLoopKind<5, false, HD>, THREADS, FMT>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
            else if (kind == 3) loop_periods<VemlLoopKind<3, true, HD>, THREADS, FMT>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
            else loop_periods<VemlLoopKind<5, true, HD>, THREADS, FMT>(s, s_p, s_corr, s_go, lds, crec, n_epochs, lds_table_floats, limit, resident);
        });
}

// the mixed kernel of a mixed engine (gc_trk_loop_set_mixed); high-dynamics engines take 256 threads like the persistent kernel
hipError_t loop_launch_mixed(const LoopLaunch& a, int iq_format, bool high_dyn)
{
    return trk_switch_format(iq_format, [&](auto fm) {
        return trk_switch_threads(a.plan.threads, high_dyn, [&](auto th, auto hd) {
            return loop_launch_kernel(trk_closed_loop_mixed_kernel<th(), fm(), hd()>, th(), a, a.plan.resident);
        });
    });
}
