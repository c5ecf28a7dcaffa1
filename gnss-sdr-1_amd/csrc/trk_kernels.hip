// trk_kernels.hip -- batched tracking multicorrelator for gfx950 (MI355X).
//
// One kernel fuses what the reference does in two volk_gnsssdr passes per
// channel-epoch (cpu_multicorrelator_real_codes.cc:129-152):
//   code NCO    volk_gnsssdr_32f_xn_resampler_32f_xn_generic
//               (kernels/volk_gnsssdr/volk_gnsssdr_32f_xn_resampler_32f_xn.h:77-94)
//               / ..._high_dynamics_resampler_32f_xn_generic (…:81-107)
//   carrier NCO + E/P/L dot products
//               volk_gnsssdr_32fc_32f_rotator_dot_prod_32fc_xn_generic (…:81-113)
//               / ..._high_dynamic_rotator_dot_prod_32fc_xn_generic (…:82-116)
// The resampled replica (4*n_taps bytes per sample in the reference) is never
// materialised: chip indices are computed per sample with the generic kernel's
// float32 operation order (no FMA contraction in that expression: this file is
// built with -ffp-contract=off and uses fmaf() explicitly where fusing is
// wanted) and looked up in an LDS-resident window of the code table.
//
// Work decomposition: one 256-thread workgroup (4 wave64) per
// (channel, epoch, slice).  Each lane streams 16-byte (2 complex sample) loads,
// 1 KiB per wave-instruction, coalesced; per-lane partial sums for every tap are
// reduced with wave shuffles, then across the 4 waves through LDS.  No MFMA:
// 8 bytes of IQ per ~45 VALU operations is an HBM/VALU-bound complex MAC stream.
#include "gc_internal.h"
#include "trk_batch_plan.h"  // TRK_FORMAT_TRAITS: the sample formats of each mode
#include "trk_device.hpp"

#ifndef TRK_WAVES
#define TRK_WAVES 8  // minimum waves per SIMD the register allocator must leave room for (<= 64 VGPRs)
#endif
static __device__ __forceinline__ short sat16(int v) { return (short)min(max(v, -32768), 32767); }

#ifndef TRK_CHIPS_WAVES
#define TRK_CHIPS_WAVES 4  // the chip-domain loop holds a lane's eight samples and the next segment's loads
#endif
// what the batched kernel instantiates trk_epoch with (trk_device.hpp)
template <int NTAPS_, bool HDR_, bool HDC_, int FMT_, bool CC_, bool SC16_, bool CHIPS_>
struct TrkBatchPolicy
{
    static constexpr int NTAPS = NTAPS_, FMT = FMT_;
    static constexpr bool HDR = HDR_, HDC = HDC_, CC = CC_, SC16 = SC16_, CHIPS = CHIPS_;
    static constexpr int THREADS = TRK_THREADS;
    static constexpr bool DATA = false;        // the data component's correlator is the closed loop's
    static constexpr bool NT = (TRK_NT != 0);  // every window streams once from HBM
    static constexpr bool WHOLE = true;        // the ragged ends of a window take prefetched 16-byte loads like its interior
    static constexpr bool GTAB = !CHIPS;       // launches sized below the table (trk_batch_plan.h); the chip-domain loop keeps the whole table in LDS
};

template <int NTAPS, bool HDR, bool HDC, int FMT, bool CC = false, bool SC16 = false, bool CHIPS = false>
__global__ __launch_bounds__(TRK_THREADS, CHIPS ? TRK_CHIPS_WAVES : TRK_WAVES) void trk_multicorrelator_kernel(
    const TrkChan* __restrict__ chans, const gc_epoch_params* __restrict__ params,
    float2* __restrict__ out, float2* __restrict__ partial,
    int n_channels, int n_epochs, int n_slices, int lds_table_floats, int align_pairs)
{
    extern __shared__ float lds[];

    // XCD-aware job mapping: workgroups are dealt round-robin over the 8 XCDs, so
    // blocks with equal (blockIdx % 8) share an L2.  All channels of one epoch
    // (which read the same IQ window when they share an RF stream) are given the
    // same residue.
    const int b = blockIdx.x;
    int slice, ch, epoch;
    if (n_epochs == 1)
        {
            // one epoch per channel (level-1 calls and their batches): no epoch dimension to spread over the XCDs
            slice = b % n_slices;
            ch = b / n_slices;
            epoch = 0;
        }
    else
        {
            const int x = b & 7;
            int q = b >> 3;
            slice = q % n_slices;
            q /= n_slices;
            ch = q % n_channels;
            epoch = (q / n_channels) * 8 + x;
            if (epoch >= n_epochs) return;
        }
    const int job = ch * n_epochs + epoch;

    const TrkChan cd = chans[ch];
    const gc_epoch_params p = params[job];
    const float2 r = trk_epoch<TrkBatchPolicy<NTAPS, HDR, HDC, FMT, CC, SC16, CHIPS>>(cd, p, slice, n_slices, lds_table_floats, lds, align_pairs);
    if (threadIdx.x < NTAPS)
        {
            if (n_slices == 1)
                {
                    if (SC16)  // lv_16sc_t results: the exact integer sums, saturated once
                        reinterpret_cast<short2*>(out)[(size_t)job * NTAPS + threadIdx.x] = make_short2(sat16(__float_as_int(r.x)), sat16(__float_as_int(r.y)));
                    else
                        out[(size_t)job * NTAPS + threadIdx.x] = r;
                }
            else
                partial[((size_t)job * n_slices + slice) * NTAPS + threadIdx.x] = r;
        }
}

// sums the per-slice partials in slice order (deterministic)
__global__ void trk_finish_kernel(const float2* __restrict__ partial, float2* __restrict__ out,
    int n_items /* jobs*n_taps */, int n_taps, int n_slices, int sc16)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    int job = i / n_taps, t = i % n_taps;
    if (sc16)
        {
            int sr = 0, si = 0;
            for (int s = 0; s < n_slices; s++)
                {
                    float2 v = partial[((size_t)job * n_slices + s) * n_taps + t];
                    sr += __float_as_int(v.x);
                    si += __float_as_int(v.y);
                }
            reinterpret_cast<short2*>(out)[i] = make_short2(sat16(sr), sat16(si));
            return;
        }
    float sr = 0.f, si = 0.f;
    for (int s = 0; s < n_slices; s++)
        {
            float2 v = partial[((size_t)job * n_slices + s) * n_taps + t];
            sr += v.x;
            si += v.y;
        }
    out[i] = make_float2(sr, si);
}

// -----------------------------------------------------------------------------
// launcher
// -----------------------------------------------------------------------------
// Experiments build only: $GNSSCORR_TRK_LOOP = samples | chips selects the form of the plain float loop.  The chip-domain form
// (trk_chips.hpp) gives the same results and measured slower on MI355X in every mode of the bench
#ifdef GNSSCORR_EXPERIMENTS
static bool trk_chip_domain()
{
    static const bool on = [] {
        const char* e = gc_exp_env("GNSSCORR_TRK_LOOP");
        return e && e[0] == 'c';
    }();
    return on;
}
static size_t trk_chips_lds_bytes(int lds_table_floats)
{
    return (size_t)(TRK_HDR_FLOATS + ((lds_table_floats + 3) & ~3) + TRK_THREADS / 64 * TRK_CHIPS_WAVE_FLOATS) * sizeof(float);
}
#endif
// whether trk_launch's kernel for (mode, format) serves records that fit neither the launch's LDS window nor the whole table in it
// (the global-table path of trk_epoch): the host sizes a launch's LDS below the table only then
bool trk_small_window_ok(int mode, int iq_format)
{
#ifdef GNSSCORR_EXPERIMENTS
    if (mode == TRK_MODE_PLAIN && iq_format == GC_IQ_F32 && trk_chip_domain()) return false;  // the chip-domain loop keeps the whole table in LDS
#endif
    (void)mode;
    (void)iq_format;
    return true;
}

// the kernel's arithmetic switches per TRK_MODE_*; the sample formats of each come from TRK_FORMAT_TRAITS (trk_batch_plan.h)
struct TrkModeSwitches
{
    bool hdr, hdc, cc, sc16;
};
static constexpr TrkModeSwitches TRK_MODE_SWITCHES[5] = {
    {false, false, false, false},  // TRK_MODE_PLAIN
    {true, false, false, false},   // TRK_MODE_HD_RESAMPLER
    {true, true, false, false},    // TRK_MODE_HD_FULL
    {false, false, true, false},   // TRK_MODE_COMPLEX_CODE
    {false, false, false, true},   // TRK_MODE_SC16: lv_16sc_t in, lv_16sc_t out
};

// f(std::integral_constant<int, v>) for v in [LO, HI]; hipErrorInvalidValue outside
template <int LO, int HI, class F>
static hipError_t trk_switch_int(int v, F f)
{
    if constexpr (LO > HI)
        return hipErrorInvalidValue;
    else
        return v == LO ? f(std::integral_constant<int, LO>()) : trk_switch_int<LO + 1, HI>(v, f);
}

hipError_t trk_launch(int n_taps, int mode, int iq_format, hipStream_t st, const TrkChan* chans,
    const gc_epoch_params* params, float2* out, float2* partial,
    int n_channels, int n_epochs, int n_slices, int lds_table_floats, bool line_aligned)
{
    const int align_pairs = line_aligned ? TRK_ALIGN_PAIRS : 1;
    const int epochs8 = n_epochs == 1 ? 1 : (n_epochs + 7) / 8 * 8;
    dim3 grid((unsigned)((size_t)epochs8 * n_channels * n_slices));
    size_t lds_bytes = (size_t)(TRK_HDR_FLOATS + lds_table_floats) * sizeof(float);
    // one kernel per tap count and (mode, format) pair of TRK_FORMAT_TRAITS: the pairs no caller can reach are not compiled
    hipError_t e = trk_switch_int<1, GC_MAX_TAPS>(n_taps, [&](auto nt) {
        return trk_switch_int<TRK_MODE_PLAIN, TRK_MODE_SC16>(mode, [&](auto md) {
            return trk_switch_format(iq_format, [&](auto fm) -> hipError_t {
                constexpr int NTAPS = decltype(nt)::value, MODE = decltype(md)::value, FMT = decltype(fm)::value;
                if constexpr ((TRK_FORMAT_TRAITS[MODE].iq_formats & (1u << FMT)) == 0)
                    return hipErrorInvalidValue;
                else
                    {
                        constexpr TrkModeSwitches m = TRK_MODE_SWITCHES[MODE];
#ifdef GNSSCORR_EXPERIMENTS
                        if constexpr (MODE == TRK_MODE_PLAIN && FMT == GC_IQ_F32)
                            if (trk_chip_domain() && trk_chips_lds_bytes(lds_table_floats) <= 64 * 1024)
                                {
                                    hipLaunchKernelGGL((trk_multicorrelator_kernel<NTAPS, false, false, GC_IQ_F32, false, false, true>), grid, dim3(TRK_THREADS),
                                        trk_chips_lds_bytes(lds_table_floats), st, chans, params, out, partial, n_channels, n_epochs, n_slices, lds_table_floats, align_pairs);
                                    return hipGetLastError();
                                }
#endif
                        hipLaunchKernelGGL((trk_multicorrelator_kernel<NTAPS, m.hdr, m.hdc, FMT, m.cc, m.sc16>), grid, dim3(TRK_THREADS), lds_bytes, st,
                            chans, params, out, partial, n_channels, n_epochs, n_slices, lds_table_floats, align_pairs);
                        return hipGetLastError();
                    }
            });
        });
    });
    if (e != hipSuccess) return e;
    if (n_slices > 1)
        {
            int n_items = n_channels * n_epochs * n_taps;
            hipLaunchKernelGGL(trk_finish_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st,
                partial, out, n_items, n_taps, n_slices, mode == TRK_MODE_SC16 ? 1 : 0);
            e = hipGetLastError();
        }
    return e;
}
