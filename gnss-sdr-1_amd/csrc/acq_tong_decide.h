// acq_tong_decide.h -- the decision step of the Tong detector (pcps_tong_acquisition_cc.cc:393-415), for host and device.
//
// After every dwell the block compares the largest cell of its normalised, accumulated grid with a threshold that grows with the
// dwell count and walks an unsigned counter:
//
//   dwell_count = dwell_count + 1                                    (:316, in front of the dwell)
//   if stat > threshold * dwell_count:  tong_count++;  positive when tong_count == tong_max_val
//   else:                               tong_count--;  negative when tong_count == 0
//   if dwell_count >= tong_max_dwells:  negative                     (also over a positive reached in this same dwell)
//
// threshold * dwell_count is a float32 product of the float threshold and the uint32 count converted to float; a NaN statistic
// compares false and counts down.  acq_tong_step() is that statement for statement; acq_tong_decide_kernel runs it per satellite
// and tests/acq_tong_decide_selftest.cpp runs it on the CPU.  Built with -ffp-contract=off like the rest of the library.
#ifndef ACQ_TONG_DECIDE_H
#define ACQ_TONG_DECIDE_H
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TONG_HD __host__ __device__
#else
#define TONG_HD
#endif

enum
{
    ACQ_TONG_RUNNING = 0,
    ACQ_TONG_POSITIVE = 1,
    ACQ_TONG_NEGATIVE = 2
};

// lives in HBM between dwells, one per satellite; the layout of gc_acq_tong_status
struct AcqTongState
{
    int32_t state;
    uint32_t tong_count;
    uint32_t dwell_count;  // the dwell that decided, or the last dwell run
};

struct AcqTongParams
{
    float threshold;
    uint32_t init_val, max_val, max_dwells;
};

static TONG_HD inline void acq_tong_restart(AcqTongState& st, const AcqTongParams& p)
{
    st.state = ACQ_TONG_RUNNING;
    st.tong_count = p.init_val;
    st.dwell_count = 0;
}

// one dwell of a RUNNING satellite with test statistic `stat`; returns the new state
static TONG_HD inline int32_t acq_tong_step(AcqTongState& st, const AcqTongParams& p, float stat)
{
    st.dwell_count++;
    if (stat > p.threshold * (float)st.dwell_count)
        {
            st.tong_count++;
            if (st.tong_count == p.max_val) st.state = ACQ_TONG_POSITIVE;
        }
    else
        {
            st.tong_count--;
            if (st.tong_count == 0) st.state = ACQ_TONG_NEGATIVE;
        }
    if (st.dwell_count >= p.max_dwells) st.state = ACQ_TONG_NEGATIVE;
    return st.state;
}

#endif
