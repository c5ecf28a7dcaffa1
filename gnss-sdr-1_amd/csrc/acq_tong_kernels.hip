// acq_tong_kernels.hip -- the decision kernel of the Tong engine (pcps_tong_acquisition_cc.cc:363-415).
#include "acq_tong_kernels.h"

#define ACQ_TONG_THREADS 256

struct TongKey
{
    float v;
    unsigned long long k;  // row * N + index: orders equal values like the block's scan
};
static __device__ __forceinline__ TongKey tong_key_max(TongKey a, TongKey b)
{
    return (b.v > a.v || (b.v == a.v && b.k < a.k)) ? b : a;
}

// One workgroup per satellite.  The block visits the rows in ascending order, takes the FIRST maximum of each and lets a later row
// win only with a strictly larger value, starting from d_mag = 0 (:363-375): the winner is the largest value, ties go to the
// smallest (row, index), and a grid without a positive value -- all zero, or NaN where the input power was 0 -- leaves d_mag at 0
// and the cell fields of the previous dwell as they were (zero at the start of a search).
__global__ __launch_bounds__(ACQ_TONG_THREADS) void acq_tong_decide_kernel(AcqTongDecideArgs a)
{
    const int sat = blockIdx.x;
    if (__builtin_amdgcn_readfirstlane(a.frozen[sat]) != 0) return;  // decided in an earlier dwell: nothing of it moves any more
    const int tid = threadIdx.x;
    constexpr int NW = ACQ_TONG_THREADS / 64;
    __shared__ float sv[NW];
    __shared__ unsigned long long sk[NW];
    TongKey b = {-1.0f, ~0ull};
    const int total = a.n_bins * a.n_blocks;
    for (int i = tid; i < total; i += ACQ_TONG_THREADS)
        {
            const size_t e = (size_t)sat * total + i;
            const unsigned idx = a.blk_max_idx[e];
            const float val = a.blk_max_val[e];
            if (idx == 0xffffffffu) continue;  // block without a value that compares (no kept samples, or NaN only)
            TongKey c = {val, (unsigned long long)(i / a.n_blocks) * (unsigned long long)a.fft_size + idx};
            b = tong_key_max(b, c);
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            TongKey o;
            o.v = __shfl_down(b.v, off, 64);
            o.k = __shfl_down(b.k, off, 64);
            b = tong_key_max(b, o);
        }
    if ((tid & 63) == 0)
        {
            sv[tid >> 6] = b.v;
            sk[tid >> 6] = b.k;
        }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < NW; w++)
        {
            TongKey c = {sv[w], sk[w]};
            b = tong_key_max(b, c);
        }
    gc_acq_result r = a.results[sat];
    float mag = 0.0f;
    if (b.v > 0.0f)
        {
            mag = b.v;
            const unsigned row = (unsigned)(b.k / (unsigned long long)a.fft_size);
            const unsigned tim = (unsigned)(b.k % (unsigned long long)a.fft_size);
            r.indext = tim;
            r.doppler_index = row;
            r.doppler_hz = -a.doppler_max + a.doppler_step * (int)row;
            r.acq_doppler_hz = (double)r.doppler_hz;
            r.acq_delay_samples = (double)(tim % a.samples_per_code);  // integer remainder (:371)
        }
    r.mag = mag;
    r.test_statistics = mag;  // :393
    r.input_power = *a.input_power;
    r.second_peak = 0.0f;
    r.second_peak_full_row = 0.0f;
    a.results[sat] = r;
    AcqTongState st = a.state[sat];
    if (acq_tong_step(st, a.p, mag) != ACQ_TONG_RUNNING) a.frozen[sat] = 1;
    a.state[sat] = st;
}

__global__ __launch_bounds__(64) void acq_tong_restart_kernel(AcqTongState* __restrict__ state, int* __restrict__ frozen,
    gc_acq_result* __restrict__ results, int n_sats, AcqTongParams p)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_sats) return;
    AcqTongState st;
    acq_tong_restart(st, p);
    state[s] = st;
    frozen[s] = 0;
    gc_acq_result r;
    r.indext = 0;
    r.doppler_hz = 0;
    r.doppler_index = 0;
    r.test_statistics = 0.0f;
    r.mag = 0.0f;
    r.input_power = 0.0f;
    r.second_peak = 0.0f;
    r.second_peak_full_row = 0.0f;
    r.acq_delay_samples = 0.0;
    r.acq_doppler_hz = 0.0;
    results[s] = r;
}

hipError_t acq_tong_launch_decide(hipStream_t st, const AcqTongDecideArgs& a, int n_sats)
{
    if (n_sats <= 0 || a.samples_per_code == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(acq_tong_decide_kernel, dim3(n_sats), dim3(ACQ_TONG_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t acq_tong_launch_restart(hipStream_t st, AcqTongState* state, int* frozen, gc_acq_result* results, int n_sats, AcqTongParams p)
{
    if (n_sats <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(acq_tong_restart_kernel, dim3((n_sats + 63) / 64), dim3(64), 0, st, state, frozen, results, n_sats, p);
    return hipGetLastError();
}
