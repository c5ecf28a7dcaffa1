// cond_blank_decide.h -- the decision stage of the conditioner's pulse blanking, for host and device.
//
// The definition (include/gnsscorr.h) is the reference's pulse_blanking_cc.cc, one segment after the other:
//
//   if n < segments_est and not last_filtered:  noise = (float(n) * noise + E / float(2L)) / float(n + 1);  pass
//   else if E / noise > threshold:              blank;  last_filtered = true
//   else:                                       pass;   last_filtered = false;  if n > segments_reset: n = 0
//   n = n + 1
//
// blank_seq_step() is that statement for statement.  While n >= segments_est the floor is constant and the tests of consecutive
// segments are independent, so a wave takes 64 segments at once: every lane evaluates blank_lane_flag(), the flags are balloted,
// and blank_wave_commit() finds how many of them stand -- up to and including the first PASSING lane whose n + lane exceeds
// segments_reset, where the sequential loop would have reset n and gone back to estimating.  tests/blank_decide_selftest.cpp
// holds the 64-wide form to the sequential loop bit for bit.  Built with -ffp-contract=off like the rest of the library.
#ifndef COND_BLANK_DECIDE_H
#define COND_BLANK_DECIDE_H
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BLANK_HD __host__ __device__
#else
#define BLANK_HD
#endif

// lives in HBM between launches (one block of 32 bytes)
struct BlankState
{
    unsigned long long decided;  // segments decided so far
    unsigned long long blanked;  // of those, zeroed
    float noise;                 // noise_power_estimation
    unsigned n;                  // n_segments
    unsigned last_filtered;      // 0 / 1
    unsigned pad;
};

struct BlankParams
{
    float threshold;
    float dof;  // float(2L); float(L) for real raw samples
    unsigned segments_est;
    unsigned segments_reset;
};

// one segment of the sequential loop; returns 1 when the segment is blanked
static BLANK_HD inline unsigned blank_seq_step(BlankState& st, const BlankParams& p, float e)
{
    unsigned flag = 0;
    if (st.n < p.segments_est && !st.last_filtered)
        st.noise = ((float)st.n * st.noise + e / p.dof) / (float)(st.n + 1u);
    else if (e / st.noise > p.threshold)
        {
            flag = 1;
            st.last_filtered = 1;
        }
    else
        {
            st.last_filtered = 0;
            if (st.n > p.segments_reset) st.n = 0;
        }
    st.n++;
    st.decided++;
    st.blanked += flag;
    return flag;
}

// steady mode (n >= segments_est): every lane's test
static BLANK_HD inline bool blank_lane_flag(float e, float noise, float threshold) { return e / noise > threshold; }

// steady mode: `flags` holds the tests of `cnt` (1..64) consecutive segments, lane i being n + i.  Commits the segments up to and
// including the first passing one at which the sequential loop resets n; returns how many were committed (the flags of the
// others are void: the floor changes before them).
static BLANK_HD inline unsigned blank_wave_commit(BlankState& st, const BlankParams& p, unsigned long long flags, unsigned cnt)
{
    const unsigned long long valid = cnt >= 64u ? ~0ull : ((1ull << cnt) - 1ull);
    flags &= valid;
    // lanes with n + lane > segments_reset: lane >= k
    const unsigned long long k = st.n <= p.segments_reset ? (unsigned long long)p.segments_reset - st.n + 1ull : 0ull;
    const unsigned long long over = k >= 64ull ? 0ull : (~0ull << k);
    const unsigned long long resets = ~flags & valid & over;
    unsigned committed = cnt;
    if (resets != 0ull)
        {
            committed = (unsigned)__builtin_ctzll(resets) + 1u;
            st.n = 1;  // n = 0, then n = n + 1
            st.last_filtered = 0;
        }
    else
        {
            st.n += cnt;
            st.last_filtered = (unsigned)((flags >> (cnt - 1u)) & 1ull);
        }
    const unsigned long long done = committed >= 64u ? ~0ull : ((1ull << committed) - 1ull);
    st.blanked += (unsigned long long)__builtin_popcountll(flags & done);
    st.decided += committed;
    return committed;
}

#endif
