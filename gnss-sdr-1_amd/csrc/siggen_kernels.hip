// siggen_kernels.hip -- the signal generator's kernel (gfx950): scenario samples t_first .. t_first + n_out - 1 into one contiguous
// piece of a ring and, for the piece's first n_mirror samples, behind the ring.
//
//   x[t] = sum_s amplitude_s b_s(t) w_s(t) + sigma (g_re(t) + j g_im(t))          float32, satellites in index order, noise last
//
// with b_s the sum of the satellite's components (table entry x gain x data symbol x secondary-code symbol, on the real or the
// imaginary axis) and w_s its carrier; gnsscorr.h states the model.  Every phase is a Q0.64 integer: a thread takes the closed form
// (siggen_phase.h) for the first sample of its run and adds integer increments for the rest -- the same integers, so which thread,
// tile, launch or piece of the ring a sample falls in cannot change its bits.  The float arithmetic of a sample is one function,
// sg_satellite / sg_noise, whatever the ring's format.
//
// A workgroup of 256 threads takes tiles of 1024 samples in turn.
//   GC_IQ_F32   thread i owns the 4 CONSECUTIVE samples 4 i .. 4 i + 3 of the tile and stores them as two 16-byte words.  Tiles are
//               laid out from the even ring position at or in front of the piece, so a piece that starts at an odd position has an
//               8-byte store in front (and one behind, when it ends at one); the mirror part, whose position has the parity of
//               the capacity, goes out as 8-byte stores.
//   GC_IQ_I16 / GC_IQ_I8   thread i owns samples i, i + 256, i + 512, i + 768 of the tile, the layout of the shared store epilogue
//               (cond_store_epilogue.h), which scales, clamps, rounds, counts the clipped components and packs the stores.
// The tables are read from HBM through L2 -- every workgroup reads the same few hundred KB -- or, when the launch's tables fit in
// GC_SIGGEN_LDS_FLOATS, from a copy each workgroup makes in LDS (SiggenJob::tables_in_lds; DESIGN.md has the measurement).  The
// satellite descriptors are read with a uniform index: scalar loads.
#include "siggen_kernels.h"
#include <algorithm>

extern __shared__ __attribute__((aligned(16))) float sg_lds_tables[];

template <bool LDS_TABLES>
static __device__ __forceinline__ float sg_table_read(const float* __restrict__ tables, const unsigned i)
{
    if constexpr (LDS_TABLES)
        return sg_lds_tables[i];
    else
        return tables[i];
}

// sine and cosine of x TURNS, |x| <= 1: the hardware's instructions take turns (valid to +-256), so no 2 pi is ever multiplied in.
// Measured against sincospif: the same parity maxima, a quarter less time at 8 and 32 satellites.
static __device__ __forceinline__ void sg_sincos_turns(const float x, float& sn, float& cs)
{
    sn = __builtin_amdgcn_sinf(x);
    cs = __builtin_amdgcn_cosf(x);
}

// gain x data symbol x secondary-code symbol of component c of satellite s in its code period k: the symbols are +-1, so the
// products are exact in any order
static __device__ __forceinline__ float sg_modulation(const SiggenJob& job, const SiggenComp& comp, const unsigned s, const unsigned c, const unsigned long long k)
{
    const unsigned long long kk = k + comp.period_offset;
    float m = comp.gain;
    if (comp.periods_per_symbol != 0) m *= sg_symbol(job.seed, kk / comp.periods_per_symbol, s, c);
    if (comp.secondary_len != 0) m *= (float)job.secondary[comp.secondary_off + (unsigned)(kk % comp.secondary_len)];
    return m;
}

// adds satellite s to the R samples t_run, t_run + STRIDE, ... of a thread
template <int R, unsigned STRIDE, bool LDS_TABLES>
static __device__ __forceinline__ void sg_satellite(const SiggenJob& job, const unsigned s, const unsigned long long t_run, float2 (&acc)[R])
{
    const SiggenSat& sat = job.sats[s];
    const unsigned long long inc_f = sat.code_step_q * STRIDE;
    const unsigned long long inc_k = STRIDE == 1 ? 0ull : sg_mulhi(sat.code_step_q, (unsigned long long)STRIDE);
    const unsigned long long carr_inc = sat.carr_step_q * STRIDE;
    SgCodePhase u = sg_code_phase(sat.code_phase0_q, sat.code_step_q, t_run);
    unsigned long long theta = sg_carrier_phase(sat.carr_phase0_q, sat.carr_step_q, t_run);
    unsigned long long k_cur = 0;
    float m[2] = {0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < R; r++)
        {
            if (r > 0)
                {
                    u = sg_code_advance(u, inc_k, inc_f);
                    // the step that carries the sample number itself past 2^64: U of the wrapped t is 2^64 step less, so the
                    // closed form's period count starts again, and with it the symbols (f and theta are residues: unchanged)
                    if (t_run + (unsigned long long)r * STRIDE < (unsigned long long)STRIDE) u.k -= sat.code_step_q;
                    theta += carr_inc;
                }
            if (r == 0 || u.k != k_cur)
                {
                    // a new code period: the symbols change here and nowhere else
                    k_cur = u.k;
                    m[0] = sg_modulation(job, sat.comp[0], s, 0u, k_cur);
                    if (sat.n_comp > 1) m[1] = sg_modulation(job, sat.comp[1], s, 1u, k_cur);
                }
            const unsigned e = sg_table_index(u.f, sat.table_len);
            float br = 0.0f, bi = 0.0f;
            {
                const float v = sg_table_read<LDS_TABLES>(job.tables, sat.comp[0].table_off + e) * m[0];
                if (sat.comp[0].axis) bi += v; else br += v;
            }
            if (sat.n_comp > 1)
                {
                    const float v = sg_table_read<LDS_TABLES>(job.tables, sat.comp[1].table_off + e) * m[1];
                    if (sat.comp[1].axis) bi += v; else br += v;
                }
            float sn, cs;
            sg_sincos_turns(0.5f * sg_half_turns(theta), sn, cs);
            const float px = br * cs - bi * sn;
            const float py = br * sn + bi * cs;
            acc[r].x += sat.amplitude * px;
            acc[r].y += sat.amplitude * py;
        }
}

// adds sigma (g_re + j g_im) of sample t: Box-Muller on the two 24-bit uniforms of the sample's Philox words
static __device__ __forceinline__ void sg_noise(const SiggenJob& job, const unsigned long long t, float2& acc)
{
    const SgPhilox w = sg_noise_words(job.seed, t);
    const float rad = sqrtf(-2.0f * logf(sg_uniform_open(w.x[0])));
    float sn, cs;
    sg_sincos_turns(sg_uniform(w.x[1]), sn, cs);
    acc.x += job.sigma * (rad * cs);
    acc.y += job.sigma * (rad * sn);
}

template <int OUT, bool LDS_TABLES>
__global__ __launch_bounds__(GC_SIGGEN_THREADS) void siggen_kernel(const SiggenJob job)
{
    constexpr int R = GC_SIGGEN_RUN, TH = GC_SIGGEN_THREADS, TILE = R * TH;
    constexpr unsigned STRIDE = OUT == GC_IQ_F32 ? 1u : (unsigned)TH;
    __shared__ float2 sg_stage[OUT == GC_IQ_I8 ? TILE / 4 : 1];  // the epilogue's cbyte stage: 2 bytes per sample of a tile
    const int tid = threadIdx.x;
    if constexpr (LDS_TABLES)
        {
            for (unsigned i = tid; i < job.n_table_floats; i += TH) sg_lds_tables[i] = job.tables[i];
            __syncthreads();
        }
    // tiles count from `shift` samples in front of the piece: the even ring position of the 16-byte stores
    const unsigned shift = OUT == GC_IQ_F32 ? (job.ring_pos & 1u) : 0u;
    const unsigned long long n_virtual = (unsigned long long)job.n_out + shift;
    const unsigned n_tiles = (unsigned)((n_virtual + TILE - 1) / TILE);
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
        {
            const unsigned long long v_tile = (unsigned long long)tile * TILE;
            // the thread's first sample, counted in the piece: -1 for the sample in front of an odd piece (computed, never stored)
            const long long j_run = (long long)(v_tile + (OUT == GC_IQ_F32 ? (unsigned)(tid * R) : (unsigned)tid)) - (long long)shift;
            const unsigned long long t_run = job.t_first + (unsigned long long)j_run;
            float2 acc[R];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = float2{0.0f, 0.0f};
            for (unsigned s = 0; s < job.n_sats; s++) sg_satellite<R, STRIDE, LDS_TABLES>(job, s, t_run, acc);
            if (job.sigma != 0.0f)
                {
#pragma unroll
                    for (int r = 0; r < R; r++) sg_noise(job, t_run + (unsigned long long)r * STRIDE, acc[r]);
                }
            if constexpr (OUT == GC_IQ_F32)
                {
                    float2* dst = static_cast<float2*>(job.out.dst);
                    float2* mirror_dst = static_cast<float2*>(job.out.mirror_dst);
#pragma unroll
                    for (int r = 0; r < R; r += 2)
                        {
                            const long long j0 = j_run + r, j1 = j0 + 1;
                            const bool ok0 = j0 >= 0 && j0 < (long long)job.n_out, ok1 = j1 < (long long)job.n_out;
                            if (ok0 && ok1)
                                *reinterpret_cast<float4*>(dst + j0) = float4{acc[r].x, acc[r].y, acc[r + 1].x, acc[r + 1].y};  // ring_pos + j0 is even
                            else if (ok0)
                                dst[j0] = acc[r];
                            else if (ok1)
                                dst[j1] = acc[r + 1];
                            if (ok0 && j0 < (long long)job.out.n_mirror) mirror_dst[j0] = acc[r];
                            if (ok1 && j1 < (long long)job.out.n_mirror) mirror_dst[j1] = acc[r + 1];
                        }
                }
            else
                {
                    const unsigned o0 = (unsigned)v_tile;
                    const int tn = (int)min((unsigned)TILE, job.n_out - o0);
                    // The epilogue's cbyte path takes the tile's mirror part as min(tn, n_mirror - o0) behind a test n_mirror > o0.  In
                    // this kernel's tile loop the compiled code kept the unsigned difference and lost the test, so a tile behind the
                    // mirror part stored tn samples past the ring.  Handing the epilogue max(n_mirror, o0) makes the difference
                    // itself 0 there: the same result with the test or without it.
                    CondStoreDst out = job.out;
                    out.n_mirror = max(job.out.n_mirror, o0);
                    cond_store_tile<OUT, R, TH>(sg_stage, acc, tn, o0, out);
                    __syncthreads();  // the epilogue's LDS is free again before the next tile writes it
                }
        }
}

template <int OUT>
static void siggen_launch_format(hipStream_t st, const SiggenJob& job, const dim3 grid)
{
    const dim3 block(GC_SIGGEN_THREADS);
    if (job.tables_in_lds)
        hipLaunchKernelGGL((siggen_kernel<OUT, true>), grid, block, sizeof(float) * (size_t)job.n_table_floats, st, job);
    else
        hipLaunchKernelGGL((siggen_kernel<OUT, false>), grid, block, 0, st, job);
}

hipError_t siggen_launch(int out_format, hipStream_t st, const SiggenJob& job, int n_groups)
{
    if (job.n_out == 0) return hipSuccess;
    const bool integer_out = out_format == GC_IQ_I16 || out_format == GC_IQ_I8;
    if (job.out.dst == nullptr || (job.out.n_mirror > 0 && job.out.mirror_dst == nullptr) || job.out.n_mirror > job.n_out || n_groups < 1 ||
        (job.n_sats > 0 && (job.sats == nullptr || job.tables == nullptr)) || job.n_sats > 32 || (integer_out && job.out.clipped == nullptr) ||
        (job.tables_in_lds && job.n_table_floats > GC_SIGGEN_LDS_FLOATS))
        return hipErrorInvalidValue;
    const unsigned tile = GC_SIGGEN_THREADS * GC_SIGGEN_RUN;
    const unsigned long long n_tiles = ((unsigned long long)job.n_out + 1ull + tile - 1) / tile;
    const dim3 grid((unsigned)std::min<unsigned long long>(n_tiles, (unsigned long long)n_groups));
    switch (out_format)
        {
        case GC_IQ_F32: siggen_launch_format<GC_IQ_F32>(st, job, grid); break;
        case GC_IQ_I16: siggen_launch_format<GC_IQ_I16>(st, job, grid); break;
        case GC_IQ_I8: siggen_launch_format<GC_IQ_I8>(st, job, grid); break;
        default: return hipErrorInvalidValue;
        }
    return hipGetLastError();
}
