// acq_quicksync_kernels.hip -- fold and candidate check of the QuickSync search (pcps_quicksync_acquisition_cc.cc:366-474).
// Everything between the two -- the M-point transforms, |.|^2, the row maxima and the statistic -- is the PCPS engine's
// (acq_kernels.hip) at fft size M = N / f.
#include "acq_quicksync_kernels.h"

// volk_32fc_x2_multiply_32fc: plain float32 products and sums (the library is built with -ffp-contract=off)
static __device__ __forceinline__ float2 qs_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// ---- fold (:382-396) ----
// Memory bound: per bin the wipe-off row is read once (8 L bytes), the block x (8 L bytes, the same for every bin) comes from the
// caches, 8 M bytes are written.  A workgroup owns ACQ_QS_TB consecutive columns b of the row-permuted output, i.e. the contiguous
// samples m = N1 b0 .. N1 (b0 + nb) - 1 (m = a + N1 b): every term t reads one contiguous run of x and of the row, the sums go to
// LDS and leave it as N1 contiguous runs of the output (the gather of acq_wipeoff_segments_kernel).  One lane owns one output (two
// neighbours where 16-byte loads are possible) and adds its terms with t ascending: the bits do not depend on the geometry.
#define ACQ_QS_TB 64
__global__ __launch_bounds__(256) void acq_qs_fold_kernel(const float2* __restrict__ x, const float2* __restrict__ wipe, float2* __restrict__ y,
    int L, int M, int terms, int N1, int N2)
{
    extern __shared__ float2 tile[];  // [ACQ_QS_TB * N1]
    const int bin = blockIdx.y;
    const int b0 = blockIdx.x * ACQ_QS_TB;
    const int nb = min(ACQ_QS_TB, N2 - b0);
    const int base = N1 * b0, count = N1 * nb;  // base is even; base + count <= M
    const float2* __restrict__ w = wipe + (size_t)bin * L;
    // 16-byte loads: M even (every t M + base is even, and so is count: the last tile ends at M) and both rows 16-byte aligned
    const bool wide = (M & 1) == 0 && ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(w)) & 15) == 0;
    if (wide)
        {
            for (int i = 2 * threadIdx.x; i < count; i += 512)
                {
                    const int m = base + i;
                    float2 s0 = make_float2(0.f, 0.f), s1 = make_float2(0.f, 0.f);
#pragma unroll 4
                    for (int t = 0; t < terms; t++)
                        {
                            const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)t * M + m);
                            const float4 wv = *reinterpret_cast<const float4*>(w + (size_t)t * M + m);
                            const float2 p0 = qs_cmul(make_float2(xv.x, xv.y), make_float2(wv.x, wv.y));
                            const float2 p1 = qs_cmul(make_float2(xv.z, xv.w), make_float2(wv.z, wv.w));
                            s0 = make_float2(s0.x + p0.x, s0.y + p0.y);
                            s1 = make_float2(s1.x + p1.x, s1.y + p1.y);
                        }
                    tile[i] = s0;
                    tile[i + 1] = s1;
                }
        }
    else
        {
            for (int i = threadIdx.x; i < count; i += 256)
                {
                    const int m = base + i;
                    float2 s = make_float2(0.f, 0.f);
#pragma unroll 4
                    for (int t = 0; t < terms; t++)
                        {
                            const float2 p = qs_cmul(x[(size_t)t * M + m], w[(size_t)t * M + m]);
                            s = make_float2(s.x + p.x, s.y + p.y);
                        }
                    tile[i] = s;
                }
        }
    __syncthreads();
    const int j = threadIdx.x & (ACQ_QS_TB - 1);
    for (int a = threadIdx.x / ACQ_QS_TB; a < N1; a += 256 / ACQ_QS_TB)
        if (j < nb) y[(size_t)bin * M + (size_t)a * N2 + b0 + j] = tile[a + N1 * j];
}

hipError_t acq_qs_launch_fold(hipStream_t st, const float2* x, const float2* wipe, float2* y, int n_bins, int L, int terms, const AcqFftPlan& plan)
{
    const size_t lds = sizeof(float2) * ACQ_QS_TB * (size_t)plan.N1;
    if (lds > 48 * 1024 || terms < 1 || (long long)terms * plan.N > (long long)L) return hipErrorInvalidValue;
    dim3 grid((plan.N2 + ACQ_QS_TB - 1) / ACQ_QS_TB, n_bins);
    hipLaunchKernelGGL(acq_qs_fold_kernel, grid, dim3(256), lds, st, x, wipe, y, L, plan.N, terms, plan.N1, plan.N2);
    return hipGetLastError();
}

// ---- candidate check (:440-474) ----
// One workgroup per (satellite, candidate).  Fixed reduction order: lane `tid` adds its terms j = tid, tid + 1024, ... ascending;
// the 64 lanes of a wave are combined by the shuffle tree with offsets 32, 16, 8, 4, 2, 1 (lane l takes lane l + offset); lane 0 of
// the workgroup adds the sixteen wave sums, wave 0 first.  No float atomics: two runs give the same bits.  (The block adds the N
// products one after the other; the difference is float32 rounding of a sum of N terms.)
// Latency bound -- n_sats * f workgroups, each a dependent chain of loads: 1024 lanes and the loads of ACQ_QS_VERIFY_U terms in
// flight per lane before the first one is used (256 lanes with one load at a time took 33.5 us for 32 x 4 candidates of N = 25000).
#define ACQ_QS_VERIFY_THREADS 1024
#define ACQ_QS_VERIFY_U 4
__global__ __launch_bounds__(ACQ_QS_VERIFY_THREADS) void acq_qs_verify_kernel(AcqQsVerifyArgs a)
{
    const int sat = blockIdx.x, cand = blockIdx.y;
    const int tid = threadIdx.x;
    __shared__ float2 sw[ACQ_QS_VERIFY_THREADS / 64];
    // the folded winner, as the statistics kernel left it in device memory; clamped so that a result that was never written cannot
    // take a read out of the arrays
    const unsigned k = min(a.results[sat].indext, (unsigned)(a.M - 1));
    const unsigned bin = min(a.results[sat].doppler_index, (unsigned)(a.n_bins - 1));
    const int p = (int)k + cand * a.M;            // < f M <= L
    const int n = min(a.N, a.L - p);              // = N for f >= 2; f = 1: the block ends N - k* samples behind p
    const float2* __restrict__ xs = a.x + p;
    const float2* __restrict__ ws = a.wipe + (size_t)bin * a.L + p;
    const float2* __restrict__ cs = a.codes + (size_t)sat * a.N;
    float2 acc = make_float2(0.f, 0.f);
    for (int j0 = tid; j0 < n; j0 += ACQ_QS_VERIFY_U * ACQ_QS_VERIFY_THREADS)
        {
            float2 xv[ACQ_QS_VERIFY_U], wv[ACQ_QS_VERIFY_U], cv[ACQ_QS_VERIFY_U];
#pragma unroll
            for (int u = 0; u < ACQ_QS_VERIFY_U; u++)
                {
                    const int j = j0 + u * ACQ_QS_VERIFY_THREADS;
                    const bool in = j < n;
                    xv[u] = in ? xs[j] : make_float2(0.f, 0.f);
                    wv[u] = in ? ws[j] : make_float2(0.f, 0.f);
                    cv[u] = in ? cs[j] : make_float2(0.f, 0.f);
                }
#pragma unroll
            for (int u = 0; u < ACQ_QS_VERIFY_U; u++)
                {
                    if (j0 + u * ACQ_QS_VERIFY_THREADS >= n) continue;
                    const float2 t = qs_cmul(qs_cmul(xv[u], wv[u]), cv[u]);
                    acc = make_float2(acc.x + t.x, acc.y + t.y);
                }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            const float ox = __shfl_down(acc.x, off, 64), oy = __shfl_down(acc.y, off, 64);
            acc = make_float2(acc.x + ox, acc.y + oy);
        }
    if ((tid & 63) == 0) sw[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        {
            float2 s = sw[0];
            for (int w = 1; w < ACQ_QS_VERIFY_THREADS / 64; w++) s = make_float2(s.x + sw[w].x, s.y + sw[w].y);
            a.cand_val[(size_t)sat * a.f + cand] = s.x * s.x + s.y * s.y;  // volk_32fc_magnitude_squared_32f (:470)
            a.cand_delay[(size_t)sat * a.f + cand] = (uint32_t)p;
        }
}

// second step: one lane per satellite takes the first maximum of its f values (volk_gnsssdr_32f_index_max_32u, :471) and fills the result
__global__ __launch_bounds__(64) void acq_qs_pick_kernel(AcqQsVerifyArgs a, int n_sats)
{
    const int sat = blockIdx.x * 64 + threadIdx.x;
    if (sat >= n_sats) return;
    int best = 0;
    float bv = a.cand_val[(size_t)sat * a.f];
    for (int i = 1; i < a.f; i++)
        {
            const float v = a.cand_val[(size_t)sat * a.f + i];
            if (v > bv)
                {
                    bv = v;
                    best = i;
                }
        }
    a.results[sat].acq_delay_samples = (double)a.cand_delay[(size_t)sat * a.f + best];  // :474
}

hipError_t acq_qs_launch_verify(hipStream_t st, const AcqQsVerifyArgs& a, int n_sats)
{
    if (a.f < 1 || a.M < 1 || (long long)a.f * a.M > (long long)a.L || n_sats < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(acq_qs_verify_kernel, dim3(n_sats, a.f), dim3(ACQ_QS_VERIFY_THREADS), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(acq_qs_pick_kernel, dim3((n_sats + 63) / 64), dim3(64), 0, st, a, n_sats);
    return hipGetLastError();
}
