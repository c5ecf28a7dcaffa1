// acq_tong_decide_selftest.cpp -- the decision step shared by host and device (csrc/acq_tong_decide.h) on hand-made sequences of
// q_d = stat_d / d, the ones tests/test_tong_ref.py walks through the numpy restatement.  Stand-alone: its own main, no GPU, built with
// -fsanitize=address,undefined by tests/test_tong_abi.py.
#include "acq_tong_decide.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

struct Expect
{
    int32_t state;
    uint32_t tong_count, dwell_count;
};

static int failures = 0;

// runs q (in units of the threshold 1.0: stat_d = q_d * d) until the detector decides; compares the record after every dwell
static void run(const char* name, uint32_t init, uint32_t max_val, uint32_t max_dwells, const std::vector<float>& q, const std::vector<Expect>& want)
{
    AcqTongParams p;
    p.threshold = 1.0f;
    p.init_val = init;
    p.max_val = max_val;
    p.max_dwells = max_dwells;
    AcqTongState st;
    acq_tong_restart(st, p);
    size_t d = 0;
    for (; d < q.size() && st.state == ACQ_TONG_RUNNING; d++)
        {
            acq_tong_step(st, p, q[d] * (float)(d + 1));
            if (d >= want.size() || st.state != want[d].state || st.tong_count != want[d].tong_count || st.dwell_count != want[d].dwell_count)
                {
                    std::printf("FAIL %s dwell %zu: state %d count %u dwells %u\n", name, d + 1, st.state, st.tong_count, st.dwell_count);
                    failures++;
                    return;
                }
        }
    if (d != want.size())
        {
            std::printf("FAIL %s: decided after %zu dwells, expected %zu\n", name, d, want.size());
            failures++;
        }
}

int main()
{
    const int R = ACQ_TONG_RUNNING, P = ACQ_TONG_POSITIVE, N = ACQ_TONG_NEGATIVE;
    // the adapters' defaults (1, 2, 3): one hit is a positive, one miss a negative
    run("default hit", 1, 2, 3, {1.5f}, {{P, 2, 1}});
    run("default miss: init 1 goes negative on the first miss", 1, 2, 3, {0.5f}, {{N, 0, 1}});
    // up / down walks
    run("walk up", 2, 4, 8, {1.2f, 1.3f}, {{R, 3, 1}, {P, 4, 2}});
    run("walk down", 2, 4, 8, {0.9f, 0.8f}, {{R, 1, 1}, {N, 0, 2}});
    run("up down up up up", 2, 4, 8, {1.1f, 0.9f, 1.1f, 0.7f, 1.2f, 1.2f}, {{R, 3, 1}, {R, 2, 2}, {R, 3, 3}, {R, 2, 4}, {R, 3, 5}, {P, 4, 6}});
    run("non-monotone absent walk", 2, 4, 8, {1.32f, 0.68f, 0.49f, 0.41f}, {{R, 3, 1}, {R, 2, 2}, {R, 1, 3}, {N, 0, 4}});
    // the max-dwells override: alternating walk never reaches 0 or max, the last dwell is negative; a positive reached in the last dwell is overridden
    run("negative by max dwells", 2, 4, 4, {1.1f, 0.9f, 1.1f, 0.9f}, {{R, 3, 1}, {R, 2, 2}, {R, 3, 3}, {N, 2, 4}});
    run("positive overridden at max dwells", 2, 4, 2, {1.1f, 1.1f}, {{R, 3, 1}, {N, 4, 2}});
    run("max dwells 1", 1, 2, 1, {5.0f}, {{N, 2, 1}});
    run("max dwells 1, miss", 1, 2, 1, {0.1f}, {{N, 0, 1}});
    // equality is not a hit (strict >); NaN and a zero statistic count down; +inf threshold counts down whatever the statistic
    run("equal counts down", 2, 4, 8, {1.0f, 1.0f}, {{R, 1, 1}, {N, 0, 2}});
    run("NaN counts down", 2, 4, 8, {std::numeric_limits<float>::quiet_NaN(), 0.0f}, {{R, 1, 1}, {N, 0, 2}});
    {
        AcqTongParams p = {std::numeric_limits<float>::infinity(), 3, 5, 10};
        AcqTongState st;
        acq_tong_restart(st, p);
        int d = 0;
        while (st.state == ACQ_TONG_RUNNING) acq_tong_step(st, p, 1e30f), d++;
        if (d != 3 || st.state != N || st.tong_count != 0 || st.dwell_count != 3) std::printf("FAIL inf threshold\n"), failures++;
    }
    // the counter is a uint32 and the positive test an equality, like the block's: a large tong_max_val is reached exactly
    {
        AcqTongParams p = {1.0f, 4000000000u, 4000000002u, 100};
        AcqTongState st;
        acq_tong_restart(st, p);
        acq_tong_step(st, p, 2.0f);
        if (st.state != R || st.tong_count != 4000000001u) std::printf("FAIL uint32 counter (1)\n"), failures++;
        acq_tong_step(st, p, 3.0f);
        if (st.state != P || st.tong_count != 4000000002u || st.dwell_count != 2) std::printf("FAIL uint32 counter (2)\n"), failures++;
    }
    // threshold * dwell_count is a float32 product: 0.1f * 3 rounds to 0.3000000119, so 0.3f (0.3000000119) is NOT above it
    {
        AcqTongParams p = {0.1f, 5, 9, 100};
        AcqTongState st;
        acq_tong_restart(st, p);
        st.dwell_count = 2;
        acq_tong_step(st, p, 0.1f * 3.0f);
        if (st.tong_count != 4) std::printf("FAIL float32 product\n"), failures++;
    }
    if (failures) return 1;
    std::printf("tong decision step: all sequences as expected\n");
    return 0;
}
