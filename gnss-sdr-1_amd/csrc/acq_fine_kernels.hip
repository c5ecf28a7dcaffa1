// acq_fine_kernels.hip -- fine Doppler stage (pcps_acquisition_fine_doppler_cc.cc:400-479): the code-wiped spectrum of P code periods
// at the bins of the acceptance window only, as a direct sum.  No transform: a request reads count (159 for +-1 kHz at Z = 8,
// P = 10) of the Next = P N Z bins.
//
//   acq_fine_partial_kernel   one workgroup per (tile of ACQ_FINE_TILE samples, request): the tile of the ring, addressed by absolute
//                             sample number, times the rotated code, into LDS; then every lane owns one bin and walks the tile with
//                             broadcast LDS reads.  The twiddle exp(-j 2 pi k n / Next) is a recurrence of ACQ_FINE_SEED steps,
//                             started each time from the reduced integer phase index ((k n) mod Next, advanced by (k SEED) mod Next
//                             with one conditional subtraction, so it stays exact); the step itself comes from a double sincospi.
//                             Leaves sum y w^n per bin and sum |y|^2 of the tile.
//   acq_fine_finish_kernel    one workgroup per request: adds the tiles in tile order, p = |Y|^2, first maximum in array-index
//                             order, the result record; p stays in HBM for gc_fine_doppler_spectrum.
//
// Every sum has a fixed order that depends on the request and the samples alone, never on the ring position, the sample format or
// the other requests of the launch; there are no atomics.
#include "acq_fine_kernels.h"
#include "ring_window.h"

#define ACQ_FINE_THREADS 192  // three waves: 159 bins of the usual window in one pass
#define ACQ_FINE_FINISH_THREADS 256
static_assert(ACQ_FINE_TILE % ACQ_FINE_SEED == 0, "a tile is a whole number of recurrence runs");

// entry i of the tile is sample n0 + i of the block: times r'[(n0 + i) mod N]
struct FinePut
{
    float2* y;
    const float2* code;
    uint32_t m0, n, s;  // m0 = n0 mod N
    int alignment;
    __device__ __forceinline__ void operator()(int i, float2 x) const
    {
        const uint32_t m = (m0 + (uint32_t)i) % n;
        const float2 c = code[fine_replica_src(m, n, s, alignment)];
        y[i] = float2{x.x * c.x - x.y * c.y, x.x * c.y + x.y * c.x};
    }
};

template <int THREADS>
static __device__ __forceinline__ float fine_block_sum(float v, float* sh)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sh[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; w++) t += sh[w];
    return t;
}

template <int FMT>
__global__ __launch_bounds__(ACQ_FINE_THREADS) void acq_fine_partial_kernel(AcqFineArgs a)
{
    __shared__ __attribute__((aligned(16))) float2 y[ACQ_FINE_TILE];
    __shared__ float wave_sum[ACQ_FINE_THREADS / 64];
    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const AcqFineRequest q = a.req[r];
    const uint32_t n0 = tile * ACQ_FINE_TILE;
    const int len = (int)min((uint32_t)ACQ_FINE_TILE, a.total - n0);
    const int padded = (len + ACQ_FINE_SEED - 1) / ACQ_FINE_SEED * ACQ_FINE_SEED;  // <= ACQ_FINE_TILE
    ring_window_load<FMT, ACQ_FINE_THREADS>(a.src, a.src_cap, (long long)(a.first + n0), len,
        FinePut{y, a.codes + (size_t)q.slot * a.n, n0 % a.n, a.n, q.delay, a.alignment});
    for (int i = len + tid; i < padded; i += ACQ_FINE_THREADS) y[i] = float2{0.0f, 0.0f};
    __syncthreads();

    float e = 0.0f;
    for (int i = tid; i < len; i += ACQ_FINE_THREADS) e += y[i].x * y[i].x + y[i].y * y[i].y;
    e = fine_block_sum<ACQ_FINE_THREADS>(e, wave_sum);
    if (tid == 0) a.energy[(size_t)r * a.n_tiles + tile] = e;

    const float nextf = (float)a.next;
    float2* out = a.partial + ((size_t)r * a.n_tiles + tile) * a.stride;
    for (uint32_t b = tid; b < q.count; b += ACQ_FINE_THREADS)
        {
            uint32_t k = q.k_lo + b;
            if (k >= a.next) k -= a.next;
            uint32_t idx = fine_phase_index(k, n0, a.next);
            const uint32_t inc = fine_phase_index(k, ACQ_FINE_SEED, a.next);
            double sd, cd;
            sincospi(2.0 * (double)k / (double)a.next, &sd, &cd);
            const float sr = (float)cd, si = -(float)sd;  // one step: exp(-j 2 pi k / Next)
            float ar = 0.0f, ai = 0.0f;
            for (int c = 0; c < padded; c += ACQ_FINE_SEED)
                {
                    float sn, cs;
                    sincospif(2.0f * (float)idx / nextf, &sn, &cs);  // idx < 2^24: exact in float32
                    float wr = cs, wi = -sn;
#pragma unroll
                    for (int j = 0; j < ACQ_FINE_SEED; j++)
                        {
                            const float2 v = y[c + j];
                            ar = fmaf(v.x, wr, ar);
                            ar = fmaf(-v.y, wi, ar);
                            ai = fmaf(v.x, wi, ai);
                            ai = fmaf(v.y, wr, ai);
                            const float nr = fmaf(wr, sr, -(wi * si));
                            wi = fmaf(wr, si, wi * sr);
                            wr = nr;
                        }
                    idx += inc;
                    if (idx >= a.next) idx -= a.next;
                }
            out[b] = float2{ar, ai};
        }
}

struct FineKey
{
    float p;
    uint32_t k, b;
};
static __device__ __forceinline__ FineKey fine_key_max(FineKey x, FineKey y)
{
    return (y.p > x.p || (y.p == x.p && y.k < x.k)) ? y : x;
}

__global__ __launch_bounds__(ACQ_FINE_FINISH_THREADS) void acq_fine_finish_kernel(AcqFineArgs a)
{
    constexpr int NW = ACQ_FINE_FINISH_THREADS / 64;
    __shared__ float wave_sum[NW];
    __shared__ float sp[NW];
    __shared__ uint32_t sk[NW], sb[NW];
    const int tid = threadIdx.x;
    const uint32_t r = blockIdx.x;
    const AcqFineRequest q = a.req[r];

    // mean = sum |y|^2: a lane takes every 256th tile in order, then one fixed tree
    float e = 0.0f;
    for (uint32_t t = tid; t < a.n_tiles; t += ACQ_FINE_FINISH_THREADS) e += a.energy[(size_t)r * a.n_tiles + t];
    e = fine_block_sum<ACQ_FINE_FINISH_THREADS>(e, wave_sum);

    FineKey best = {-1.0f, 0xffffffffu, 0u};
    for (uint32_t b = tid; b < q.count; b += ACQ_FINE_FINISH_THREADS)
        {
            const float2* p = a.partial + (size_t)r * a.n_tiles * a.stride + b;
            float yr = 0.0f, yi = 0.0f;
            for (uint32_t t = 0; t < a.n_tiles; t++)
                {
                    const float2 v = p[(size_t)t * a.stride];
                    yr += v.x;
                    yi += v.y;
                }
            const float pw = yr * yr + yi * yi;
            a.spec[(size_t)r * a.stride + b] = pw;
            uint32_t k = q.k_lo + b;
            if (k >= a.next) k -= a.next;
            best = fine_key_max(best, FineKey{pw, k, b});
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            FineKey o;
            o.p = __shfl_down(best.p, off, 64);
            o.k = __shfl_down(best.k, off, 64);
            o.b = __shfl_down(best.b, off, 64);
            best = fine_key_max(best, o);
        }
    if ((tid & 63) == 0)
        {
            sp[tid >> 6] = best.p;
            sk[tid >> 6] = best.k;
            sb[tid >> 6] = best.b;
        }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < NW; w++) best = fine_key_max(best, FineKey{sp[w], sk[w], sb[w]});
    if (best.k == 0xffffffffu)
        {
            // nothing compared (NaN samples): the window's first bin, flagged as an edge
            best.b = 0;
            best.k = q.k_lo;
            best.p = a.spec[(size_t)r * a.stride];
        }
    gc_fine_doppler_result res;
    res.doppler_hz = (double)fine_freq(best.k, a.fs, a.next);
    res.bin = best.k;
    res.status = (best.b == 0 || best.b == q.count - 1) ? GC_FINE_EDGE : GC_FINE_REFINED;
    res.peak = best.p;
    res.mean = e;
    res.window_first_bin = q.k_lo;
    res.window_bins = q.count;
    a.results[r] = res;
}

hipError_t acq_fine_launch(hipStream_t st, const AcqFineArgs& a, int iq_format, int n_requests)
{
    if (n_requests <= 0 || a.n == 0 || a.total == 0 || a.src_cap == 0 || a.n_tiles != (a.total + ACQ_FINE_TILE - 1) / ACQ_FINE_TILE) return hipErrorInvalidValue;
    const dim3 grid(a.n_tiles, (unsigned)n_requests), block(ACQ_FINE_THREADS);
    switch (iq_format)
        {
        case GC_IQ_F32:
            hipLaunchKernelGGL(acq_fine_partial_kernel<GC_IQ_F32>, grid, block, 0, st, a);
            break;
        case GC_IQ_I16:
            hipLaunchKernelGGL(acq_fine_partial_kernel<GC_IQ_I16>, grid, block, 0, st, a);
            break;
        case GC_IQ_I8:
            hipLaunchKernelGGL(acq_fine_partial_kernel<GC_IQ_I8>, grid, block, 0, st, a);
            break;
        default:
            return hipErrorInvalidValue;
        }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(acq_fine_finish_kernel, dim3((unsigned)n_requests), dim3(ACQ_FINE_FINISH_THREADS), 0, st, a);
    return hipGetLastError();
}
