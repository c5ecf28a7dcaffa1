// siggen_phase.h -- the signal generator's closed forms (gnsscorr.h, "Signal generator"): where a scenario sample stands in a
// satellite's code and carrier, and the counter-based random numbers of its noise and data symbols.  Everything here is exact
// integer arithmetic on Q0.64 fixed point, a function of the sample's ABSOLUTE number t alone; the kernel (siggen_kernels.hip),
// the host (gc_signal_generator.hip) and the host tests (tests/siggen_phase_selftest.cpp) compile this same text.
#ifndef SIGGEN_PHASE_H
#define SIGGEN_PHASE_H
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SG_HD __host__ __device__ __forceinline__
#else
#define SG_HD inline
#endif

// the upper 64 bits of a 64 x 64 bit product
static SG_HD uint64_t sg_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// U = k 2^64 + f: k code periods and the position f / 2^64 inside the period
struct SgCodePhase
{
    uint64_t k, f;
};

// U = phase0 + t step, all 128 bits of it
static SG_HD SgCodePhase sg_code_phase(uint64_t phase0, uint64_t step, uint64_t t)
{
    const uint64_t lo = t * step;
    SgCodePhase u;
    u.f = lo + phase0;
    u.k = sg_mulhi(t, step) + (u.f < lo ? 1u : 0u);
    return u;
}

// U + (inc_k 2^64 + inc_f): the step from one sample of a run to the next (inc = stride * step, 128 bits)
static SG_HD SgCodePhase sg_code_advance(SgCodePhase u, uint64_t inc_k, uint64_t inc_f)
{
    SgCodePhase v;
    v.f = u.f + inc_f;
    v.k = u.k + inc_k + (v.f < inc_f ? 1u : 0u);
    return v;
}

// e = floor(f table_len / 2^64) < table_len
static SG_HD uint32_t sg_table_index(uint64_t f, uint32_t table_len) { return (uint32_t)sg_mulhi(f, (uint64_t)table_len); }

// theta = (phase0 + t step) mod 2^64, in turns / 2^64
static SG_HD uint64_t sg_carrier_phase(uint64_t phase0, uint64_t step, uint64_t t) { return phase0 + t * step; }

// the carrier angle as float32 HALF turns in [-1, 1]: the signed upper 32 bits of theta, rounded once to float32, times 2^-31
// (exact).  exp(j pi h) is the carrier.
static SG_HD float sg_half_turns(uint64_t theta) { return (float)(int32_t)(uint32_t)(theta >> 32) * 4.656612873077393e-10f; }

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants)
struct SgPhilox
{
    uint32_t x[4];
};

static SG_HD SgPhilox sg_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int round = 0; round < 10; round++)
        {
            const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
            const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
            const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
            c1 = (uint32_t)p1;
            c3 = (uint32_t)p0;
            c0 = n0;
            c2 = n2;
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
    SgPhilox r;
    r.x[0] = c0;
    r.x[1] = c1;
    r.x[2] = c2;
    r.x[3] = c3;
    return r;
}

// the noise of sample t: counter (t_lo, t_hi, 0, 0), key (seed_lo, seed_hi)
static SG_HD SgPhilox sg_noise_words(uint64_t seed, uint64_t t)
{
    return sg_philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// u1 = ((x0 >> 8) + 1) 2^-24 in (0, 1], u2 = (x1 >> 8) 2^-24 in [0, 1): both exact in float32
static SG_HD float sg_uniform_open(uint32_t x0) { return (float)((x0 >> 8) + 1u) * 5.9604644775390625e-08f; }
static SG_HD float sg_uniform(uint32_t x1) { return (float)(x1 >> 8) * 5.9604644775390625e-08f; }

// data symbol j of component c (0, 1) of satellite s (0-based): counter (j_lo, j_hi, 2 s + c, 1); +1 when bit 0 of x0 is clear
static SG_HD float sg_symbol(uint64_t seed, uint64_t j, uint32_t s, uint32_t c)
{
    const SgPhilox r = sg_philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), 2u * s + c, 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (r.x[0] & 1u) ? -1.0f : 1.0f;
}

#endif
