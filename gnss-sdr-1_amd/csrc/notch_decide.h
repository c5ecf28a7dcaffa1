// notch_decide.h -- the notch filter ring stage for host and device: the noise floor of a segment, the state machine that decides a
// segment, the per-sample step of the filter, and the per-segment composite the device carries from segment to segment.
//
// The definition (include/gnsscorr.h) is the reference's notch_cc.cc / notch_lite_cc.cc, one segment of L samples after the other:
//
//   if n < segments_est and not active:  noise = (float(n) * noise + F[s]) / float(n + 1);   pass
//   else if E[s] / noise > threshold:    if not active: active = true; last = 0; (lite: cn = 0);   filter
//   else:                                if n > segments_reset: n = 0;   active = false;   pass
//   n = n + 1
//
// The filter is out[k] = b[k] + a[k] out[k - 1] with b = x[k] - z x[k - 1], a = p z: an affine map of the previous output with
// |a| = p < 1.  notch_sample_maps() is one sample of it; a segment's maps compose, in sample order, to one map (A, B)
// (notch_compose), which is all that the walk from segment to segment needs: last' = B + A last (notch_carry).  The outputs of a
// segment are then the sequential recursion from the last the walk carried INTO the segment.  Every one of these is a function of
// the segment's samples, x[sL - 1] and the carried value alone, so no bit depends on how the stream was cut into updates or pieces.
// The carried last is the composite's, not the segment's last output: the two differ by rounding.
//
// The decision is split the way the device runs it.  While the floor is estimated the segments are taken one at a time
// (notch_estimate_step with the floor F[s] of notch_bin + notch_floor).  Otherwise the floor is constant, the tests
// E[s] / noise > threshold of consecutive segments are independent (notch_test: a wave takes 64 at once and ballots them).
// notch_steady_step() is the definition's statement for one segment given its test; notch_wave_commit() resolves a whole ballot
// with bit operations -- flags, run starts, the lite coefficient schedule, and where n is reset -- as pulse blanking's
// blank_wave_commit does.  tests/notch_decide_selftest.cpp is the host image of the kernels' loops and holds the 64-wide form to
// the sequential one bit for bit.  Built with -ffp-contract=off like the rest of the library.
#ifndef NOTCH_DECIDE_H
#define NOTCH_DECIDE_H
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NOTCH_HD __host__ __device__
#else
#define NOTCH_HD
#endif

enum
{
    NOTCH_MODE_FULL = 0,  // a coefficient per sample (Notch_Filter)
    NOTCH_MODE_LITE = 1   // a coefficient per segments_coeff filtered segments (Notch_Filter_Lite)
};
enum
{
    NOTCH_FLOOR_REFERENCE = 0,  // mean of decibels over the kept bins, as the reference's block
    NOTCH_FLOOR_LINEAR = 1      // mean of powers over the same bins
};
// what a decided segment is, one byte per segment
enum
{
    NOTCH_SEG_FILTERED = 1,  // the segment is filtered
    NOTCH_SEG_START = 2,     // ... and starts a run: last = 0 in front of it
    NOTCH_SEG_COEFF = 4      // ... and (lite) computes a new coefficient from its own samples
};

struct NotchC
{
    float re, im;
};

// lives in HBM between launches (one block of 48 bytes).  The decide pass owns decided .. cn, the carry pass last and z0.
struct NotchState
{
    unsigned long long decided;   // segments decided so far
    unsigned long long filtered;  // of those, filtered
    float noise;                  // noise_pow_est
    unsigned n;                   // n_segments
    unsigned active;              // filter_state_, 0 / 1
    unsigned cn;                  // lite: n_segments_coeff
    NotchC last;                  // last_out
    NotchC z0;                    // lite: the coefficient in use
};

struct NotchParams
{
    float threshold;
    float p;    // p_c_factor
    float dof;  // float(2L)
    unsigned length;
    unsigned segments_est;
    unsigned segments_reset;
    unsigned segments_coeff;
    int mode;
    int noise_floor;
};

static NOTCH_HD inline NotchC notch_mul(NotchC a, NotchC b) { return NotchC{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
static NOTCH_HD inline NotchC notch_mul_conj(NotchC a, NotchC b) { return NotchC{a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}; }
static NOTCH_HD inline NotchC notch_add(NotchC a, NotchC b) { return NotchC{a.re + b.re, a.im + b.im}; }
static NOTCH_HD inline NotchC notch_sub(NotchC a, NotchC b) { return NotchC{a.re - b.re, a.im - b.im}; }

// ---- the noise floor of one segment ----

// entry j of the twiddle table of an L-point DFT: exp(-2 pi i j / L), rounded from double (host only: the device reads the table)
static inline NotchC notch_twiddle(unsigned j, unsigned L)
{
    const double a = -2.0 * 3.14159265358979323846 * (double)j / (double)L;
    return NotchC{(float)std::cos(a), (float)std::sin(a)};
}

// |X[k]|^2 of the segment x[0 .. L): X[k] = sum over i, ascending, of x[i] tw[(k i) mod L]
static NOTCH_HD inline float notch_bin(const NotchC* x, const NotchC* tw, unsigned L, unsigned k)
{
    NotchC acc = {0.0f, 0.0f};
    unsigned j = 0;  // (k i) mod L
    for (unsigned i = 0; i < L; i++)
        {
            acc = notch_add(acc, notch_mul(x[i], tw[j]));
            j += k;
            if (j >= L) j -= L;
        }
    return acc.re * acc.re + acc.im * acc.im;
}

static NOTCH_HD inline float notch_db(float power) { return 10.0f * log10f(power + 1e-20f); }

// F[s] from the L bin powers (pw) and their decibels (db), both summed in ascending bin order
static NOTCH_HD inline float notch_floor(const float* pw, const float* db, unsigned L, int noise_floor, float dof)
{
    float sum = 0.0f;
    for (unsigned k = 0; k < L; k++) sum += db[k];
    const float cut = sum / (float)L + 15.0f;
    float kept_db = 0.0f, kept_pw = 0.0f;
    unsigned kept = 0;
    for (unsigned k = 0; k < L; k++)
        if (db[k] <= cut)
            {
                kept_db += db[k];
                kept_pw += pw[k];
                kept++;
            }
    // the bin at or below the mean is kept: kept >= 1
    if (noise_floor == NOTCH_FLOOR_LINEAR) return kept_pw / (float)kept / dof;
    const float fl = kept_db / (float)kept;
    return (float)(pow(10.0, (double)fl / 10.0) / (double)dof);
}

// ---- the state machine ----

static NOTCH_HD inline bool notch_estimating(const NotchState& st, const NotchParams& p) { return st.n < p.segments_est && !st.active; }

// one segment while notch_estimating(): the running mean of the floors
static NOTCH_HD inline void notch_estimate_step(NotchState& st, float floor)
{
    st.noise = ((float)st.n * st.noise + floor) / (float)(st.n + 1u);
    st.n++;
    st.decided++;
}

// the test of a segment while not estimating; the floor does not change between such segments
static NOTCH_HD inline bool notch_test(float e, float noise, float threshold) { return e / noise > threshold; }

// One segment while not notch_estimating(), given its test: the NOTCH_SEG_* bits of the segment and, for a filtered segment in
// lite mode, how many segments back its coefficient was computed (cn in front of the segment: the filtered segments since then
// are consecutive).  Integer work alone.
static NOTCH_HD inline unsigned notch_steady_step(NotchState& st, const NotchParams& p, bool over, unsigned* back)
{
    unsigned bits = 0;
    *back = 0;
    if (over)
        {
            bits = NOTCH_SEG_FILTERED;
            if (!st.active)
                {
                    st.active = 1;
                    bits |= NOTCH_SEG_START;
                }
            if (p.mode == NOTCH_MODE_LITE)
                {
                    if (bits & NOTCH_SEG_START) st.cn = 0;
                    if (st.cn == 0) bits |= NOTCH_SEG_COEFF;
                    *back = st.cn;
                    st.cn = st.cn + 1u >= p.segments_coeff ? 0u : st.cn + 1u;  // (cn + 1) % segments_coeff: cn < segments_coeff
                }
            st.filtered++;
        }
    else
        {
            if (st.n > p.segments_reset) st.n = 0;
            st.active = 0;
        }
    st.n++;
    st.decided++;
    return bits;
}

// The same for `cnt` (1..64) consecutive segments at once, while n >= segments_est (no estimate can begin before n is reset) and
// n + 64 does not wrap: `over` holds their tests, lane i being n + i.  Commits the segments up to and including the first passing
// one at which the sequential loop resets n, and returns how many those are; *filtered and *starts are their NOTCH_SEG_FILTERED /
// NOTCH_SEG_START bits, *cn_in is cn in front of the first (notch_lane_back).  A run starts where a filtered segment follows a
// passing one (or, in lane 0, an inactive state).
static NOTCH_HD inline bool notch_wave_ready(const NotchState& st, const NotchParams& p) { return st.n >= p.segments_est && st.n <= 0xffffffffu - 64u; }
static NOTCH_HD inline unsigned notch_wave_commit(NotchState& st, const NotchParams& p, unsigned long long over, unsigned cnt, unsigned long long* filtered,
    unsigned long long* starts, unsigned* cn_in)
{
    const unsigned long long valid = cnt >= 64u ? ~0ull : ((1ull << cnt) - 1ull);
    over &= valid;
    // lanes with n + lane > segments_reset: lane >= k
    const unsigned long long k = st.n <= p.segments_reset ? (unsigned long long)p.segments_reset - st.n + 1ull : 0ull;
    const unsigned long long above = k >= 64ull ? 0ull : (~0ull << k);
    const unsigned long long resets = ~over & valid & above;
    const unsigned committed = resets != 0ull ? (unsigned)__builtin_ctzll(resets) + 1u : cnt;
    const unsigned long long done = committed >= 64u ? ~0ull : ((1ull << committed) - 1ull);
    const unsigned long long f = over & done;
    const unsigned long long s = f & ~((f << 1) | (st.active ? 1ull : 0ull));
    *filtered = f;
    *starts = s;
    *cn_in = st.cn;
    if (p.mode == NOTCH_MODE_LITE && f != 0ull)
        {
            // cn behind the newest filtered segment
            const unsigned top = 63u - (unsigned)__builtin_clzll(f);
            const unsigned long long below = s & (top >= 63u ? ~0ull : ((2ull << top) - 1ull));
            const unsigned long long pos = below != 0ull ? (unsigned long long)(top - (63u - (unsigned)__builtin_clzll(below))) : (unsigned long long)st.cn + top;
            st.cn = (unsigned)((pos + 1ull) % p.segments_coeff);
        }
    st.n = resets != 0ull ? 1u : st.n + cnt;  // a reset: n = 0, then n = n + 1
    st.active = (unsigned)((over >> (committed - 1u)) & 1ull);
    st.filtered += (unsigned long long)__builtin_popcountll(f);
    st.decided += committed;
    return committed;
}
// lite: cn in front of the filtered segment in lane `lane` of such a chunk -- the filtered segments since its run's start, or since
// the chunk's first segment where the run came in from before
static NOTCH_HD inline unsigned notch_lane_back(unsigned long long starts, unsigned cn_in, unsigned lane, unsigned segments_coeff)
{
    const unsigned long long below = starts & (lane >= 63u ? ~0ull : ((2ull << lane) - 1ull));
    const unsigned long long pos = below != 0ull ? (unsigned long long)(lane - (63u - (unsigned)__builtin_clzll(below))) : (unsigned long long)cn_in + lane;
    return (unsigned)(pos % segments_coeff);
}

// ---- the filter ----

// c / |c|, (1, 0) for c = 0: the reference's exp(j atan2(c.im, c.re)) without the trigonometry
static NOTCH_HD inline NotchC notch_unit(NotchC c)
{
    const float m = sqrtf(c.re * c.re + c.im * c.im);
    if (!(m > 0.0f)) return NotchC{1.0f, 0.0f};
    return NotchC{c.re / m, c.im / m};
}

// lite: the coefficient of a segment from its first two and its last two samples
static NOTCH_HD inline NotchC notch_lite_coeff(NotchC x0, NotchC x1, NotchC xl2, NotchC xl1)
{
    const NotchC c1 = notch_mul_conj(x1, x0), c2 = notch_mul_conj(xl1, xl2);
    const float th = (atan2f(c1.im, c1.re) + atan2f(c2.im, c2.re)) / 2.0f;
    return NotchC{cosf(th), sinf(th)};
}

// sample k: out[k] = b + a out[k - 1].  xm1 = x[k - 1] as it was before filtering; z0 is used in lite mode.
static NOTCH_HD inline void notch_sample_maps(NotchC x, NotchC xm1, int mode, NotchC z0, float p, NotchC* a, NotchC* b)
{
    const NotchC z = mode == NOTCH_MODE_FULL ? notch_unit(notch_mul_conj(x, xm1)) : z0;
    *b = notch_sub(x, notch_mul(z, xm1));
    *a = NotchC{p * z.re, p * z.im};
}

static NOTCH_HD inline NotchC notch_carry(NotchC a, NotchC b, NotchC last) { return notch_add(b, notch_mul(a, last)); }

// (A, B) followed by (a, b): the composite starts from the identity A = (1, 0), B = (0, 0)
static NOTCH_HD inline void notch_compose(NotchC a, NotchC b, NotchC* A, NotchC* B)
{
    *B = notch_carry(a, b, *B);  // b + a B
    *A = notch_mul(a, *A);
}

#endif
