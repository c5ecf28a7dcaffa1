// acq_caf_kernels.hip -- the selection and the decision kernel of the CAF engine
// (galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc:489-632 and :634-770).
#include "acq_caf_kernels.h"

#define ACQ_CAF_THREADS 256

struct CafMax
{
    float v;
    unsigned i;
};
// the larger value; of equal values the smaller index (volk_gnsssdr_32f_index_max_32u keeps the first maximum); NaN never wins
static __device__ __forceinline__ CafMax caf_max(CafMax a, CafMax b)
{
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
static __device__ __forceinline__ CafMax caf_wave_max(CafMax b)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            CafMax o;
            o.v = __shfl_down(b.v, off, 64);
            o.i = __shfl_down(b.i, off, 64);
            b = caf_max(b, o);
        }
    return b;
}

// Workgroup (x, y): share x of grid row y = (satellite, bin) of this launch.  Wave w reduces the block maxima of replica w's plane
// row to (mX, kX); every lane then makes the block's two choices (:533, :543) from those four pairs -- REFERENCE arithmetic with the
// one gathered load IB[kQB] (:523) -- and the workgroup streams its share of the chosen I row (+ the chosen Q row, float32, I first:
// :550-605) into the grid row, 16 bytes per lane where the rows are 16-byte aligned.  At most 8 N bytes read and 4 N written per
// row; no flag, no atomic, no other launch for the choice: the few block maxima are read again by every workgroup of the row.
template <bool VEC>
__global__ __launch_bounds__(ACQ_CAF_THREADS) void acq_caf_select_kernel(AcqCafSelectArgs a)
{
    const int xblk = blockIdx.x, row = blockIdx.y;
    const int sat = row / a.n_bins, bin = row - sat * a.n_bins;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = (1 + a.both) * a.hyp;
    const size_t N = (size_t)a.N;
    __shared__ float sv[4];
    __shared__ unsigned si[4];
    __shared__ float rv[ACQ_CAF_THREADS / 64];
    __shared__ unsigned ri[ACQ_CAF_THREADS / 64];
    if (wave < R)
        {
            const size_t e0 = (((size_t)sat * R + wave) * a.n_bins + bin) * a.n_blocks;
            CafMax b = {-1.0f, 0xffffffffu};
            for (int i = lane; i < a.n_blocks; i += 64)
                {
                    CafMax c = {a.pl_max_val[e0 + i], a.pl_max_idx[e0 + i]};
                    if (c.i != 0xffffffffu) b = caf_max(b, c);
                }
            b = caf_wave_max(b);
            if (lane == 0)
                {
                    // a row without a value that compares (NaN only): nothing to normalise, index 0 keeps the gathered load in range
                    if (b.i == 0xffffffffu) b = CafMax{0.0f, 0u};
                    sv[wave] = b.v;
                    si[wave] = b.i;
                }
        }
    __syncthreads();
    // replicas in the order IA, QA, IB, QB
    const int rQA = a.both ? 1 : -1, rIB = (a.hyp == 2) ? (a.both ? 2 : 1) : -1, rQB = (a.hyp == 2 && a.both) ? 3 : -1;
    const float* plane0 = a.planes + (size_t)sat * R * a.n_bins * N + (size_t)bin * N;
    const size_t rstride = (size_t)a.n_bins * N;
    bool iB = false, qB = false;
    if (rIB >= 0)
        {
            const float nIA = sv[0] / a.fnf4, nIB = sv[rIB] / a.fnf4;
            iB = !(nIA >= nIB);
        }
    if (rQB >= 0)
        {
            const float nQA = sv[rQA] / a.fnf4;
            const float mQB = (a.arithmetic == ACQ_CAF_REFERENCE) ? plane0[rIB * rstride + si[rQB]] : sv[rQB];
            const float nQB = mQB / a.fnf4;
            qB = !(nQA >= nQB);
        }
    const int ri_ = iB ? rIB : 0, rq_ = a.both ? (qB ? rQB : rQA) : -1;
    if (xblk == 0 && tid == 0)
        {
            const size_t e = (size_t)sat * a.n_bins + bin;
            a.caf_i[e] = sv[ri_];
            a.caf_q[e] = rq_ >= 0 ? sv[rq_] : 0.0f;  // the chosen Q plane's OWN maximum, under REFERENCE as well (:560)
            a.choice[e] = (unsigned char)((iB ? 1 : 0) | (qB ? 2 : 0));
        }
    const float* pi = plane0 + ri_ * rstride;
    const float* pq = rq_ >= 0 ? plane0 + rq_ * rstride : nullptr;
    float* g = a.grid + (size_t)row * N;
    // share of this workgroup: `chunk` consecutive samples, a multiple of 4
    const int chunk = (((a.N + a.n_blocks - 1) / a.n_blocks) + 3) & ~3;
    const int lo = xblk * chunk, hi = min(a.N, lo + chunk);
    CafMax best = {-1.0f, 0xffffffffu};
    if (VEC)
        {
            // N % 4 == 0: every row starts 16-byte aligned and so does every share
            for (int i = lo + 4 * tid; i < hi; i += 4 * ACQ_CAF_THREADS)
                {
                    float4 v = *reinterpret_cast<const float4*>(pi + i);
                    if (pq)
                        {
                            const float4 q = *reinterpret_cast<const float4*>(pq + i);
                            v.x += q.x;
                            v.y += q.y;
                            v.z += q.z;
                            v.w += q.w;
                        }
                    *reinterpret_cast<float4*>(g + i) = v;
                    best = caf_max(best, CafMax{v.x, (unsigned)i});
                    best = caf_max(best, CafMax{v.y, (unsigned)i + 1});
                    best = caf_max(best, CafMax{v.z, (unsigned)i + 2});
                    best = caf_max(best, CafMax{v.w, (unsigned)i + 3});
                }
        }
    else
        {
            for (int i = lo + tid; i < hi; i += ACQ_CAF_THREADS)
                {
                    float v = pi[i];
                    if (pq) v += pq[i];
                    g[i] = v;
                    best = caf_max(best, CafMax{v, (unsigned)i});
                }
        }
    best = caf_wave_max(best);
    if (lane == 0)
        {
            rv[wave] = best.v;
            ri[wave] = best.i;
        }
    __syncthreads();
    if (tid == 0)
        {
            CafMax b = {rv[0], ri[0]};
            for (int w = 1; w < ACQ_CAF_THREADS / 64; w++) b = caf_max(b, CafMax{rv[w], ri[w]});
            a.blk_max_val[(size_t)row * a.n_blocks + xblk] = b.v;
            a.blk_max_idx[(size_t)row * a.n_blocks + xblk] = b.i;
        }
}

struct CafRowKey
{
    float v;       // m_b / fnf4
    unsigned bin;
    unsigned idx;
};
// the block walks the bins in ascending order and a later bin wins only with a strictly larger value (:635)
static __device__ __forceinline__ CafRowKey caf_row_max(CafRowKey a, CafRowKey b)
{
    return (b.v > a.v || (b.v == a.v && b.bin < a.bin)) ? b : a;
}

// One workgroup per satellite, one lane per bin (bins beyond 256 in further rounds).  Every lane reduces the block maxima of its
// grid rows to (k_b, m_b) and compares m_b / fnf4 as the block does; lane 0 applies the keep rule and writes the result; the
// filter then runs from LDS, one acq_caf_at() of 2 H + 1 terms per lane, and its first maximum overwrites the Doppler (:768-770).
__global__ __launch_bounds__(ACQ_CAF_THREADS) void acq_caf_decide_kernel(AcqCafDecideArgs a)
{
    const int sat = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = ACQ_CAF_THREADS / 64;
    __shared__ float s_i[ACQ_CAF_MAX_BINS];
    __shared__ float s_q[ACQ_CAF_MAX_BINS];
    __shared__ float kv[NW];
    __shared__ unsigned kb[NW], ki[NW];
    __shared__ float cv[NW];
    __shared__ unsigned ci[NW];
    CafRowKey best = {-1.0f, 0xffffffffu, 0u};
    for (int b = tid; b < a.n_bins; b += ACQ_CAF_THREADS)
        {
            const size_t e0 = ((size_t)sat * a.n_bins + b) * a.n_blocks;
            CafMax m = {-1.0f, 0xffffffffu};
            for (int i = 0; i < a.n_blocks; i++)
                {
                    CafMax c = {a.blk_max_val[e0 + i], a.blk_max_idx[e0 + i]};
                    if (c.i != 0xffffffffu) m = caf_max(m, c);
                }
            const size_t e = (size_t)sat * a.n_bins + b;
            if (a.single_plane)
                {
                    // the grid row is the only plane: its maximum is the bin's CAF_I
                    a.caf_i[e] = m.i != 0xffffffffu ? m.v : 0.0f;
                    a.caf_q[e] = 0.0f;
                    a.choice[e] = 0;
                }
            if (m.i != 0xffffffffu) best = caf_row_max(best, CafRowKey{m.v / a.fnf4, (unsigned)b, m.i});
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            CafRowKey o;
            o.v = __shfl_down(best.v, off, 64);
            o.bin = __shfl_down(best.bin, off, 64);
            o.idx = __shfl_down(best.idx, off, 64);
            best = caf_row_max(best, o);
        }
    if (lane == 0)
        {
            kv[wave] = best.v;
            kb[wave] = best.bin;
            ki[wave] = best.idx;
        }
    __syncthreads();  // also: caf_i / caf_q written above by this workgroup are read below
    CafMax cbest = {-INFINITY, 0xffffffffu};
    if (a.caf_half > 0)
        {
            for (int b = tid; b < a.n_bins; b += ACQ_CAF_THREADS)
                {
                    s_i[b] = a.caf_i[(size_t)sat * a.n_bins + b];
                    s_q[b] = a.caf_q[(size_t)sat * a.n_bins + b];
                }
            __syncthreads();
            for (int d = tid; d < a.n_bins; d += ACQ_CAF_THREADS)
                {
                    const float c = acq_caf_at(s_i, a.both ? s_q : nullptr, a.n_bins, a.caf_half, d, a.arithmetic);
                    a.caf[(size_t)sat * a.n_bins + d] = c;
                    cbest = caf_max(cbest, CafMax{c, (unsigned)d});
                }
            cbest = caf_wave_max(cbest);
            if (lane == 0)
                {
                    cv[wave] = cbest.v;
                    ci[wave] = cbest.i;
                }
            __syncthreads();
        }
    if (tid != 0) return;
    for (int w = 1; w < NW; w++) best = caf_row_max(best, CafRowKey{kv[w], kb[w], ki[w]});
    gc_acq_result r = a.results[sat];
    const float power = *a.input_power;
    float mag = 0.0f;
    if (best.bin != 0xffffffffu && best.v > 0.0f)  // d_mag starts at 0 and moves with `d_mag < magt` (:635): nothing wins with 0 or NaN
        {
            mag = best.v;
            // the block tests every running maximum (:645); d_mag / P is monotone in d_mag, so testing the final one is the same
            const float stat = mag / power;
            if (!a.bit_transition || r.test_statistics < stat)
                {
                    r.test_statistics = stat;
                    r.indext = best.idx;
                    r.doppler_index = best.bin;
                    r.doppler_hz = -a.doppler_max + a.doppler_step * (int)best.bin;
                    r.acq_doppler_hz = (double)r.doppler_hz;
                    r.acq_delay_samples = (double)(best.idx % a.samples_per_code);  // integer remainder (:647)
                }
        }
    r.mag = mag;
    r.input_power = power;
    r.second_peak = 0.0f;
    r.second_peak_full_row = 0.0f;
    if (a.caf_half > 0)
        {
            for (int w = 1; w < NW; w++) cbest = caf_max(cbest, CafMax{cv[w], ci[w]});
            const unsigned d = cbest.i != 0xffffffffu ? cbest.i : 0u;  // NaN only: index 0, as a scan that starts there
            r.doppler_index = d;
            r.doppler_hz = -a.doppler_max + a.doppler_step * (int)d;
            r.acq_doppler_hz = (double)r.doppler_hz;
        }
    a.results[sat] = r;
}

hipError_t acq_caf_launch_select(hipStream_t st, const AcqCafSelectArgs& a, int n_sats)
{
    const int R = (1 + a.both) * a.hyp;
    if (n_sats <= 0 || a.n_bins <= 0 || a.n_blocks <= 0 || a.N <= 0 || R < 2 || R > 4) return hipErrorInvalidValue;
    dim3 grid((unsigned)a.n_blocks, (unsigned)(n_sats * a.n_bins));
    if (a.N % 4 == 0)
        hipLaunchKernelGGL(acq_caf_select_kernel<true>, grid, dim3(ACQ_CAF_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(acq_caf_select_kernel<false>, grid, dim3(ACQ_CAF_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t acq_caf_launch_decide(hipStream_t st, const AcqCafDecideArgs& a, int n_sats)
{
    if (n_sats <= 0 || a.samples_per_code == 0 || a.n_bins <= 0 || a.n_bins > ACQ_CAF_MAX_BINS) return hipErrorInvalidValue;
    if (a.caf_half > 0 && a.n_bins < 2 * a.caf_half + 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(acq_caf_decide_kernel, dim3(n_sats), dim3(ACQ_CAF_THREADS), 0, st, a);
    return hipGetLastError();
}
