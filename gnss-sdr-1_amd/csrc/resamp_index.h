// resamp_index.h -- index arithmetic of the ring resampler (gc_ring_resampler.hip, ring_resamp_kernels.hip): which source sample an
// output is, how many outputs a source head completes, and the base of one launch.  Compiles without HIP
// (tests/resamp_index_selftest.cpp).  With M = 2^32:
//
//   RESAMP_DOWN      the reference's Direct_Resampler with fs_in > fs_out (direct_resampler_conditioner_cc.cc:96-110): its running
//                    32-bit phase wraps between source samples n - 1 and n exactly when floor(n step / M) grows, so
//                      step = floor(M fs_out / fs_in)      n_m = ceil(m M / step)      outputs(H) = floor((H - 1) step / M) + 1
//   RESAMP_UP        the same block with fs_in < fs_out (:111-125): the phase advances once per OUTPUT and the input pointer
//                    moves on each wrap, so
//                      step = floor(M fs_in / fs_out)      n_m = floor((m + 1) step / M)   outputs(H) = ceil(H M / step) - 1
//   RESAMP_IDENTITY  fs_in == fs_out: n_m = m, outputs(H) = H (the reference's cast of 2^32 to uint32 is undefined there)
//   RESAMP_POLY      INC = round(M fs_in / fs_out) (ties to even)    pos_m = m INC    n_m = pos_m >> 32
//                      p_m = (pos_m & (M - 1)) >> (32 - log2 P)        outputs(H) = ceil(H M / INC)
//
// outputs(0) = 0 everywhere.  Products m M and m INC pass 2^64 after 2^32 outputs and a ring's sample numbers are absolute, so the
// host splits the first output m0 of a launch with 128-bit arithmetic into (q0, r0), r0 < max(step, M), and the kernel adds
// offsets that fit in 64 bits because the source samples of one launch are resident, fewer than 2^31:
//
//   RESAMP_DOWN   m0 M         = q0 step + r0      n_{m0 + j} = q0 + ceil((r0 + j M) / step)
//   RESAMP_UP     (m0 + 1) step = q0 M + r0         n_{m0 + j} = q0 + ((r0 + j step) >> 32)
//   RESAMP_POLY   m0 INC       = q0 M + r0         n_{m0 + j} = q0 + ((r0 + j INC) >> 32),   p from the low 32 bits of r0 + j INC
#ifndef RESAMP_INDEX_H
#define RESAMP_INDEX_H
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define RESAMP_HD __host__ __device__
#else
#define RESAMP_HD
#endif

enum
{
    RESAMP_IDENTITY = 0,
    RESAMP_DOWN = 1,
    RESAMP_UP = 2,
    RESAMP_POLY = 3
};

struct ResampRatio
{
    int kind;       // RESAMP_*
    uint64_t step;  // step (< 2^32) of the direct kinds, INC of RESAMP_POLY; 0 for RESAMP_IDENTITY
};

// first output of a launch, split as the table above states
struct ResampBase
{
    uint64_t q0, r0;
};

typedef unsigned __int128 resamp_u128;
static const uint64_t RESAMP_M = 1ull << 32;

// the direct kinds: the reference's constructor (direct_resampler_conditioner_cc.cc:56-65), IEEE double then uint32
static inline ResampRatio resamp_direct_ratio(double fs_in, double fs_out)
{
    ResampRatio r = {RESAMP_IDENTITY, 0};
    if (fs_in == fs_out) return r;
    const double two_32 = 4294967296.0;
    if (fs_in > fs_out)
        {
            r.kind = RESAMP_DOWN;
            r.step = (uint64_t)(uint32_t)std::floor(two_32 * fs_out / fs_in);
        }
    else
        {
            r.kind = RESAMP_UP;
            r.step = (uint64_t)(uint32_t)std::floor(two_32 * fs_in / fs_out);
        }
    return r;
}

// the quotient in IEEE double, times 2^32 (exact), rounded to the nearest integer with ties to even
static inline ResampRatio resamp_poly_ratio(double fs_in, double fs_out)
{
    ResampRatio r = {RESAMP_POLY, 0};
    r.step = (uint64_t)std::nearbyint(fs_in / fs_out * 4294967296.0);
    return r;
}

// source sample n_m of output m, any m
static inline uint64_t resamp_source_index(const ResampRatio& r, uint64_t m)
{
    switch (r.kind)
        {
        case RESAMP_DOWN: return (uint64_t)((((resamp_u128)m << 32) + r.step - 1) / r.step);
        case RESAMP_UP: return (uint64_t)((((resamp_u128)m + 1) * r.step) >> 32);
        case RESAMP_POLY: return (uint64_t)(((resamp_u128)m * r.step) >> 32);
        default: return m;
        }
}

// filter phase p_m of output m (RESAMP_POLY), 0 <= p_m < 2^log2_phases
static inline uint32_t resamp_phase(const ResampRatio& r, int log2_phases, uint64_t m)
{
    const uint64_t frac = (uint64_t)((resamp_u128)m * r.step) & (RESAMP_M - 1);
    return (uint32_t)(frac >> (32 - log2_phases));
}

// outputs whose source sample lies below the source head H
static inline uint64_t resamp_available(const ResampRatio& r, uint64_t H)
{
    if (H == 0) return 0;
    switch (r.kind)
        {
        case RESAMP_DOWN: return (uint64_t)((((resamp_u128)H - 1) * r.step) >> 32) + 1;
        case RESAMP_UP: return (uint64_t)((((resamp_u128)H << 32) + r.step - 1) / r.step) - 1;
        case RESAMP_POLY: return (uint64_t)((((resamp_u128)H << 32) + r.step - 1) / r.step);
        default: return H;
        }
}

static inline ResampBase resamp_base(const ResampRatio& r, uint64_t m0)
{
    ResampBase b = {m0, 0};
    switch (r.kind)
        {
        case RESAMP_DOWN:
            {
                const resamp_u128 v = (resamp_u128)m0 << 32;
                b.q0 = (uint64_t)(v / r.step);
                b.r0 = (uint64_t)(v % r.step);
                break;
            }
        case RESAMP_UP:
            {
                const resamp_u128 v = ((resamp_u128)m0 + 1) * r.step;
                b.q0 = (uint64_t)(v >> 32);
                b.r0 = (uint64_t)v & (RESAMP_M - 1);
                break;
            }
        case RESAMP_POLY:
            {
                const resamp_u128 v = (resamp_u128)m0 * r.step;
                b.q0 = (uint64_t)(v >> 32);
                b.r0 = (uint64_t)v & (RESAMP_M - 1);
                break;
            }
        default: break;
        }
    return b;
}

// r0 + j * (M, step or INC): the position of output m0 + j behind q0; fits in 64 bits while the launch's source samples are
// fewer than 2^31 (resamp_offsets_fit)
static RESAMP_HD inline uint64_t resamp_offset_pos(int kind, uint64_t step, uint64_t r0, uint64_t j)
{
    return r0 + j * (kind == RESAMP_DOWN ? (1ull << 32) : step);
}

// n_{m0 + j}: what the kernels compute per lane
static RESAMP_HD inline uint64_t resamp_offset_index(int kind, uint64_t step, uint64_t q0, uint64_t r0, uint64_t j)
{
    switch (kind)
        {
        case RESAMP_DOWN: return q0 + (resamp_offset_pos(kind, step, r0, j) + step - 1) / step;
        case RESAMP_UP:
        case RESAMP_POLY: return q0 + (resamp_offset_pos(kind, step, r0, j) >> 32);
        default: return q0 + j;
        }
}

// p_{m0 + j} (RESAMP_POLY)
static RESAMP_HD inline uint32_t resamp_offset_phase(uint64_t step, int log2_phases, uint64_t r0, uint64_t j)
{
    return (uint32_t)(((r0 + j * step) & 0xffffffffull) >> (32 - log2_phases));
}

// true when the offsets of a launch of n_out outputs stay below 2^63
static inline bool resamp_offsets_fit(const ResampRatio& r, const ResampBase& b, uint64_t n_out)
{
    if (n_out == 0 || r.kind == RESAMP_IDENTITY) return true;
    const resamp_u128 last = (resamp_u128)b.r0 + (resamp_u128)(n_out - 1) * (r.kind == RESAMP_DOWN ? RESAMP_M : r.step) + r.step;
    return last < ((resamp_u128)1 << 63);
}

// oldest source sample an update that starts at output m0 reads: n_{m0}, less the filter's history in polyphase mode
static inline uint64_t resamp_floor(const ResampRatio& r, int taps, uint64_t m0)
{
    const uint64_t n = resamp_source_index(r, m0);
    if (r.kind != RESAMP_POLY) return n;
    return n >= (uint64_t)(taps - 1) ? n - (uint64_t)(taps - 1) : 0;
}

#endif
