// ring_notch_kernels.hip -- the notch filter ring stage's kernels (gfx950): the device image of the reference's Notch_Filter and
// Notch_Filter_Lite (src/algorithms/input_filter/gnuradio_blocks/notch_cc.cc, notch_lite_cc.cc).  Output m is source sample m,
// copied or filtered; the arithmetic is notch_decide.h's.  Separate launches chained on the output ring's copy stream; no
// workgroup waits for another.  For a batch of newly complete segments:
//
//   1. energies    E[s], one lane per segment, its L samples added in ascending order.
//   2. decisions   one workgroup walks the segments with the state in HBM.  While the floor is estimated, a segment at a time:
//                  the workgroup loads it into LDS, its lanes share the L bins of the direct DFT (each bin summed in sample
//                  order), and one lane per segment reduces the bins in bin order.  Otherwise a wave tests 64 segments at once
//                  against the constant floor, ballots, and resolves the ballot with bit operations (notch_wave_commit) up to
//                  the segment at which n is reset and an estimate begins.
//   3. composites  one lane per filtered segment: its coefficient (lite mode) and the composite map (A, B) of its L samples in
//                  sample order.
//   4. the walk    one wave carries last through the segments in order, last' = B + A last, 64 records per load; it leaves
//                  last in front of every filtered segment.
//
// and for every contiguous piece of the output ring:
//
//   5. copy        one lane per output: the samples of unfiltered segments, bits as they are.
//   6. filter      one lane per filtered segment: the recursion from the carried last, in sample order from the segment's first
//                  sample on; the lane stores the outputs that lie in the piece.  A segment that the ring's wrap cuts in two is
//                  walked once for each half, to the same bits.
//
// Everything a lane computes is a function of its segment's samples, x[sL - 1], the state in front of the batch and the records
// of earlier segments: nothing depends on where the batches and the pieces were cut.
#include "ring_notch_kernels.h"
#include <hip/hip_runtime.h>

// ring position of absolute sample n (one 64-bit modulo); the walkers then step and fold
static __device__ __forceinline__ unsigned notch_pos(unsigned long long n, unsigned cap) { return (unsigned)(n % cap); }
static __device__ __forceinline__ unsigned notch_fold(unsigned pos, unsigned cap) { return pos >= cap ? pos - cap : pos; }
static __device__ __forceinline__ NotchC notch_at(const void* src, unsigned pos)
{
    const float2 v = static_cast<const float2*>(src)[pos];
    return NotchC{v.x, v.y};
}
// record of segment i of a batch whose first segment has record rec0: i < records
static __device__ __forceinline__ unsigned notch_rec(unsigned rec0, unsigned i, unsigned records) { return notch_fold(rec0 + i, records); }

__global__ __launch_bounds__(GC_NOTCH_THREADS) void ring_notch_energy_kernel(const RingNotchJob job, const unsigned long long seg0, const unsigned rec0,
    const unsigned n_seg)
{
    const unsigned i = blockIdx.x * (unsigned)GC_NOTCH_THREADS + threadIdx.x;
    if (i >= n_seg) return;
    const unsigned L = job.params.length;
    unsigned pos = notch_pos((seg0 + i) * L, job.src_cap);
    float acc = 0.0f;
    for (unsigned k = 0; k < L; k++)
        {
            const NotchC x = notch_at(job.src, pos);
            acc += x.re * x.re + x.im * x.im;
            pos = notch_fold(pos + 1u, job.src_cap);
        }
    job.work.energies[notch_rec(rec0, i, job.work.records)] = acc;
}

__global__ __launch_bounds__(GC_NOTCH_THREADS) void ring_notch_decide_kernel(const RingNotchJob job, const unsigned long long seg0, const unsigned rec0,
    const unsigned n_seg)
{
    __shared__ NotchC seg[GC_NOTCH_MAX_LENGTH];
    __shared__ float pw[GC_NOTCH_MAX_LENGTH];
    __shared__ float db[GC_NOTCH_MAX_LENGTH];
    __shared__ float floors[GC_NOTCH_THREADS / 2];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const NotchParams p = job.params;
    const unsigned L = p.length;
    // lanes that share a segment of an estimate (the power of two at or above L, 256 at most) and segments taken at once:
    // per L <= 256 samples, or one segment of up to GC_NOTCH_MAX_LENGTH
    unsigned lanes_per = 1;
    while (lanes_per < L && lanes_per < (unsigned)GC_NOTCH_THREADS) lanes_per <<= 1;
    const unsigned per = (unsigned)GC_NOTCH_THREADS / lanes_per;
    NotchState st = *job.work.state;  // the same in every lane
    unsigned i = 0;
    while (i < n_seg)
        {
            if (notch_estimating(st, p))
                {
                    // active stays false inside an estimate, so its length is known here; the floors do not depend on the
                    // state, so `per` segments are taken at once, lanes_per lanes sharing the bins of each, and only the
                    // running mean goes one segment after the other
                    const unsigned run = min(p.segments_est - st.n, n_seg - i);
                    for (unsigned g = 0; g < run; g += per)
                        {
                            const unsigned ns = min(per, run - g);
                            const unsigned pos0 = notch_pos((seg0 + i + g) * L, job.src_cap);
                            for (unsigned k = tid; k < ns * L; k += GC_NOTCH_THREADS) seg[k] = notch_at(job.src, notch_fold(pos0 + k, job.src_cap));
                            __syncthreads();
                            const unsigned q = tid / lanes_per, k_first = tid % lanes_per;
                            if (q < ns)
                                for (unsigned k = k_first; k < L; k += lanes_per)
                                    {
                                        const float w = notch_bin(seg + q * L, job.work.twiddles, L, k);
                                        pw[q * L + k] = w;
                                        db[q * L + k] = notch_db(w);
                                    }
                            __syncthreads();
                            if (q < ns && k_first == 0) floors[q] = notch_floor(pw + q * L, db + q * L, L, p.noise_floor, p.dof);
                            __syncthreads();
                            for (unsigned k = 0; k < ns; k++) notch_estimate_step(st, floors[k]);
                            if (tid < ns) job.work.bits[notch_rec(rec0, i + g + tid, job.work.records)] = 0;
                            __syncthreads();  // the next segments overwrite the bins
                        }
                    i += run;
                }
            else
                {
                    // every wave of the workgroup does the same; the first one stores.  The energies of four chunks of 64 are
                    // loaded at once; the later ones are used while every chunk in front of them was committed whole
                    float e4[4];
#pragma unroll
                    for (unsigned q = 0; q < 4u; q++)
                        {
                            const unsigned at = i + 64u * q + lane;
                            e4[q] = at < n_seg ? job.work.energies[notch_rec(rec0, at, job.work.records)] : 0.0f;
                        }
#pragma unroll
                    for (unsigned q = 0; q < 4u; q++)
                        {
                            const unsigned cnt = min(64u, n_seg - i);
                            const unsigned long long over = __ballot(lane < cnt && notch_test(e4[q], st.noise, p.threshold));
                            unsigned done = 0, my_bits = 0, my_back = 0;
                            if (notch_wave_ready(st, p))
                                {
                                    unsigned long long filtered, starts;
                                    unsigned cn_in;
                                    done = notch_wave_commit(st, p, over, cnt, &filtered, &starts, &cn_in);
                                    if ((filtered >> lane) & 1ull)
                                        {
                                            my_bits = NOTCH_SEG_FILTERED | (((starts >> lane) & 1ull) ? NOTCH_SEG_START : 0u);
                                            if (p.mode == NOTCH_MODE_LITE)
                                                {
                                                    my_back = notch_lane_back(starts, cn_in, lane, p.segments_coeff);
                                                    if (my_back == 0u) my_bits |= NOTCH_SEG_COEFF;
                                                }
                                        }
                                }
                            else
                                // active below segments_est, or n about to wrap: one segment after the other
                                while (done < cnt && !notch_estimating(st, p))
                                    {
                                        unsigned back;
                                        const unsigned b = notch_steady_step(st, p, ((over >> done) & 1ull) != 0ull, &back);
                                        if (lane == done)
                                            {
                                                my_bits = b;
                                                my_back = back;
                                            }
                                        done++;
                                    }
                            if (tid < done)
                                {
                                    const unsigned r = notch_rec(rec0, i + tid, job.work.records);
                                    job.work.bits[r] = (unsigned char)my_bits;
                                    job.work.back[r] = my_back;
                                }
                            i += done;
                            if (done != 64u || i >= n_seg || notch_estimating(st, p)) break;
                        }
                }
        }
    if (tid == 0)
        {
            // last and z0 are the walk's
            NotchState* out = job.work.state;
            out->decided = st.decided;
            out->filtered = st.filtered;
            out->noise = st.noise;
            out->n = st.n;
            out->active = st.active;
            out->cn = st.cn;
        }
}

// lite: the coefficient computed from the samples of segment s
static __device__ __forceinline__ NotchC notch_segment_coeff(const RingNotchJob& job, unsigned long long s)
{
    const unsigned L = job.params.length, cap = job.src_cap;
    const unsigned pos = notch_pos(s * L, cap);
    return notch_lite_coeff(notch_at(job.src, pos), notch_at(job.src, notch_fold(pos + 1u, cap)), notch_at(job.src, notch_fold(pos + (L - 2u), cap)),
        notch_at(job.src, notch_fold(pos + (L - 1u), cap)));
}

__global__ __launch_bounds__(GC_NOTCH_THREADS) void ring_notch_composite_kernel(const RingNotchJob job, const unsigned long long seg0, const unsigned rec0,
    const unsigned n_seg)
{
    const unsigned i = blockIdx.x * (unsigned)GC_NOTCH_THREADS + threadIdx.x;
    if (i >= n_seg) return;
    const unsigned r = notch_rec(rec0, i, job.work.records);
    if (!(job.work.bits[r] & NOTCH_SEG_FILTERED)) return;
    const NotchParams p = job.params;
    const unsigned L = p.length, cap = job.src_cap;
    NotchC z0 = {0.0f, 0.0f};
    if (p.mode == NOTCH_MODE_LITE)
        {
            // the segment that computed the coefficient: this one, an earlier one of the batch, or one in front of the batch,
            // whose coefficient the walk of that batch left in the state
            const unsigned back = job.work.back[r];
            z0 = back <= i ? notch_segment_coeff(job, seg0 + (i - back)) : job.work.state->z0;
            job.work.z[r] = z0;
        }
    const unsigned long long n0 = (seg0 + i) * L;
    unsigned pos = notch_pos(n0, cap);
    NotchC xm1 = n0 == 0ull ? NotchC{0.0f, 0.0f} : notch_at(job.src, pos == 0u ? cap - 1u : pos - 1u);
    NotchC A = {1.0f, 0.0f}, B = {0.0f, 0.0f};
    for (unsigned k = 0; k < L; k++)
        {
            const NotchC x = notch_at(job.src, pos);
            NotchC a, b;
            notch_sample_maps(x, xm1, p.mode, z0, p.p, &a, &b);
            notch_compose(a, b, &A, &B);
            xm1 = x;
            pos = notch_fold(pos + 1u, cap);
        }
    job.work.A[r] = A;
    job.work.B[r] = B;
}

static __device__ __forceinline__ float notch_lane(float v, unsigned j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)j)); }

__global__ __launch_bounds__(64) void ring_notch_walk_kernel(const RingNotchJob job, const unsigned rec0, const unsigned n_seg)
{
    const unsigned lane = threadIdx.x;
    const bool lite = job.params.mode == NOTCH_MODE_LITE;
    NotchC last = job.work.state->last, z0 = job.work.state->z0;  // the same in every lane
    for (unsigned i = 0; i < n_seg; i += 64u)
        {
            const unsigned cnt = min(64u, n_seg - i);
            const unsigned r = notch_rec(rec0, min(i + lane, n_seg - 1u), job.work.records);
            const unsigned bits = lane < cnt ? job.work.bits[r] : 0u;
            NotchC A = {0.0f, 0.0f}, B = {0.0f, 0.0f}, z = {0.0f, 0.0f};
            if (bits & NOTCH_SEG_FILTERED)
                {
                    A = job.work.A[r];
                    B = job.work.B[r];
                    if (lite) z = job.work.z[r];
                }
            const unsigned long long filtered = __ballot((bits & NOTCH_SEG_FILTERED) != 0u), starts = __ballot((bits & NOTCH_SEG_START) != 0u);
            const unsigned r0 = notch_rec(rec0, i, job.work.records);
            // the filtered segments in order (a passing segment leaves last as it is); every lane computes the same last, and
            // every lane stores it -- the same value to the same place -- in front of the segment it is carried into (a store
            // from the first lane alone measured 20 % slower: it costs the loop two changes of the execution mask)
            for (unsigned long long left = filtered; left != 0ull; left &= left - 1ull)
                {
                    const unsigned j = (unsigned)__builtin_ctzll(left);
                    if ((starts >> j) & 1ull) last = NotchC{0.0f, 0.0f};
                    job.work.carry[notch_fold(r0 + j, job.work.records)] = last;
                    last = notch_carry(NotchC{notch_lane(A.re, j), notch_lane(A.im, j)}, NotchC{notch_lane(B.re, j), notch_lane(B.im, j)}, last);
                }
            if (lite && filtered != 0ull)
                {
                    const unsigned top = 63u - (unsigned)__builtin_clzll(filtered);
                    z0 = NotchC{notch_lane(z.re, top), notch_lane(z.im, top)};
                }
        }
    if (lane == 0)
        {
            job.work.state->last = last;
            job.work.state->z0 = z0;
        }
}

// one lane per output of the piece: outputs of unfiltered segments are the source's bits.  k0: where the piece's first output lies
// in its segment, pos_first: that sample's place in the source ring.
__global__ __launch_bounds__(GC_NOTCH_THREADS) void ring_notch_copy_kernel(const RingNotchJob job, const unsigned rec_first, const unsigned k0,
    const unsigned pos_first, const unsigned n_out, const CondStoreDst out)
{
    const unsigned j = blockIdx.x * (unsigned)GC_NOTCH_THREADS + threadIdx.x;
    if (j >= n_out) return;
    const unsigned i = (k0 + j) / job.params.length;  // segment of the piece
    if (job.work.bits[notch_rec(rec_first, i, job.work.records)] & NOTCH_SEG_FILTERED) return;
    // the piece's source samples are resident: n_out <= src_cap, so one fold
    const uint2 v = static_cast<const uint2*>(job.src)[notch_fold(pos_first + j, job.src_cap)];
    static_cast<uint2*>(out.dst)[j] = v;
    if (j < out.n_mirror) static_cast<uint2*>(out.mirror_dst)[j] = v;
}

// one lane per segment of the piece; seg_first: the segment of the piece's first output
__global__ __launch_bounds__(GC_NOTCH_THREADS) void ring_notch_filter_kernel(const RingNotchJob job, const unsigned long long seg_first, const unsigned rec_first,
    const unsigned k0, const unsigned n_seg, const unsigned n_out, const CondStoreDst out)
{
    const unsigned i = blockIdx.x * (unsigned)GC_NOTCH_THREADS + threadIdx.x;
    if (i >= n_seg) return;
    const unsigned r = notch_rec(rec_first, i, job.work.records);
    if (!(job.work.bits[r] & NOTCH_SEG_FILTERED)) return;
    const NotchParams p = job.params;
    const unsigned L = p.length, cap = job.src_cap;
    // sample k of the segment is output j = i L + k - k0 of the piece, for 0 <= j < n_out
    const unsigned long long first = (unsigned long long)i * L;  // + k - k0
    const unsigned k_lo = first >= k0 ? 0u : k0 - (unsigned)first;
    const unsigned long long room = (unsigned long long)n_out + k0 - first;  // > 0: the segment has an output in the piece
    const unsigned k_hi = room < L ? (unsigned)room : L;
    const NotchC z0 = p.mode == NOTCH_MODE_LITE ? job.work.z[r] : NotchC{0.0f, 0.0f};
    NotchC last = job.work.carry[r];
    const unsigned long long n0 = (seg_first + i) * L;
    unsigned pos = notch_pos(n0, cap);
    NotchC xm1 = n0 == 0ull ? NotchC{0.0f, 0.0f} : notch_at(job.src, pos == 0u ? cap - 1u : pos - 1u);
    for (unsigned k = 0; k < k_hi; k++)
        {
            const NotchC x = notch_at(job.src, pos);
            NotchC a, b;
            notch_sample_maps(x, xm1, p.mode, z0, p.p, &a, &b);
            last = notch_carry(a, b, last);
            if (k >= k_lo)
                {
                    const unsigned j = (unsigned)(first + k - k0);
                    const float2 y = float2{last.re, last.im};
                    static_cast<float2*>(out.dst)[j] = y;
                    if (j < out.n_mirror) static_cast<float2*>(out.mirror_dst)[j] = y;
                }
            xm1 = x;
            pos = notch_fold(pos + 1u, cap);
        }
}

static bool notch_job_ok(const RingNotchJob& job)
{
    const RingNotchWork& w = job.work;
    return job.src != nullptr && job.src_cap > 0 && job.params.length >= 2 && job.params.length <= GC_NOTCH_MAX_LENGTH && job.params.segments_coeff >= 1 &&
        w.records >= 2 && w.state && w.twiddles && w.energies && w.bits && w.back && w.z && w.A && w.B && w.carry;
}

hipError_t ring_notch_decide_launch(hipStream_t st, const RingNotchJob& job, unsigned long long seg0, unsigned n_seg)
{
    if (n_seg == 0) return hipSuccess;
    // the batch and the sample in front of it must not lap the source ring, nor the batch its records
    if (!notch_job_ok(job) || n_seg >= job.work.records || (unsigned long long)n_seg * job.params.length + 1ull > job.src_cap) return hipErrorInvalidValue;
    const unsigned rec0 = (unsigned)(seg0 % job.work.records);
    const dim3 grid((n_seg + GC_NOTCH_THREADS - 1) / GC_NOTCH_THREADS), block(GC_NOTCH_THREADS);
    hipLaunchKernelGGL(ring_notch_energy_kernel, grid, block, 0, st, job, seg0, rec0, n_seg);
    hipLaunchKernelGGL(ring_notch_decide_kernel, dim3(1), block, 0, st, job, seg0, rec0, n_seg);
    hipLaunchKernelGGL(ring_notch_composite_kernel, grid, block, 0, st, job, seg0, rec0, n_seg);
    hipLaunchKernelGGL(ring_notch_walk_kernel, dim3(1), dim3(64), 0, st, job, rec0, n_seg);
    return hipGetLastError();
}

hipError_t ring_notch_apply_launch(hipStream_t st, const RingNotchJob& job, unsigned long long idx, unsigned n_out, const CondStoreDst& out)
{
    if (n_out == 0) return hipSuccess;
    const unsigned L = job.params.length;
    if (!notch_job_ok(job) || out.dst == nullptr || (out.n_mirror > 0 && out.mirror_dst == nullptr) || out.n_mirror > n_out) return hipErrorInvalidValue;
    const unsigned long long seg_first = idx / L;
    const unsigned k0 = (unsigned)(idx - seg_first * L);
    const unsigned long long n_seg = ((unsigned long long)k0 + n_out + L - 1ull) / L;
    // from the first segment's first sample, less one, to the piece's last output: resident at once
    if (n_seg >= job.work.records || (unsigned long long)k0 + n_out + 1ull > job.src_cap) return hipErrorInvalidValue;
    const unsigned rec_first = (unsigned)(seg_first % job.work.records);
    const unsigned pos_first = (unsigned)(idx % job.src_cap);
    const dim3 block(GC_NOTCH_THREADS);
    hipLaunchKernelGGL(ring_notch_copy_kernel, dim3((n_out + GC_NOTCH_THREADS - 1) / GC_NOTCH_THREADS), block, 0, st, job, rec_first, k0, pos_first, n_out, out);
    hipLaunchKernelGGL(ring_notch_filter_kernel, dim3(((unsigned)n_seg + GC_NOTCH_THREADS - 1) / GC_NOTCH_THREADS), block, 0, st, job, seg_first, rec_first, k0,
        (unsigned)n_seg, n_out, out);
    return hipGetLastError();
}
