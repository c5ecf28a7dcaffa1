// trk_loop_plan.h -- the closed-loop launch's decisions, as a pure host function: workgroup size and LDS code image from the
// engine's shape alone.  Compiles without HIP (tests/loop_plan_selftest.cpp prints the plan of any argument tuple;
// tests/test_loop_plan.py holds a table worked out by hand against it).
#ifndef TRK_LOOP_PLAN_H
#define TRK_LOOP_PLAN_H
#include <cstddef>

#ifdef __HIP__
#define TRK_LOOP_PLAN_HD __host__ __device__
#else
#define TRK_LOOP_PLAN_HD
#endif

// LDS header of a workgroup of `threads` threads: one (re, im) partial per wave and tap (GC_MAX_TAPS taps)
static constexpr TRK_LOOP_PLAN_HD int trk_hdr_floats(int threads) { return threads / 64 * 16; }

struct TrkLoopPlan
{
    int threads;           // per workgroup (= per channel)
    int lds_table_floats;  // the code image behind the header
    int resident;          // 1: the doubled image, loaded once per launch; 0: the per-period window
    size_t lds_bytes;      // dynamic LDS of the launch: header of `threads` + image
};

// started / code_len / track_pilot: per channel, read for a mixed engine only (its image is the largest need among its started
// channels -- longest code, pilot or not); a plain engine's image follows max_code_len and its pilot mode.  n_cus <= 0: 256.
static inline TrkLoopPlan trk_loop_plan(int n_channels, int n_cus, bool high_dyn, int forced_threads, bool mixed, const char* started, const int* code_len,
    const char* track_pilot, int max_code_len, bool pilot)
{
    if (n_cus <= 0) n_cus = 256;
    // LDS code image: the doubled resident one (2 L + 64 floats per replica, loaded once per launch) when it fits beside the
    // header, else the per-period window (L + 64).  With more channels than CUs several workgroups share a CU's 160 KB: the resident
    // image is then taken only while two workgroups still fit (<= 64 KiB each; Galileo E1 with the pilot's data component is 131 KB:
    // one workgroup per CU, which only costs nothing while every channel has a CU to itself)
    int resident_floats = (2 * max_code_len + 64) * (pilot ? 2 : 1);
    int window_floats = (max_code_len + 64) * (pilot ? 2 : 1);
    if (mixed)
        {
            resident_floats = window_floats = 0;
            for (int i = 0; i < n_channels; i++)
                if (started[i])
                    {
                        const int replicas = track_pilot[i] ? 2 : 1;
                        if ((2 * code_len[i] + 64) * replicas > resident_floats) resident_floats = (2 * code_len[i] + 64) * replicas;
                        if ((code_len[i] + 64) * replicas > window_floats) window_floats = (code_len[i] + 64) * replicas;
                    }
        }
    TrkLoopPlan p;
    const size_t resident_bytes = (size_t)(trk_hdr_floats(1024) + resident_floats) * sizeof(float);
    p.resident = !(resident_bytes > 150 * 1024 || (n_channels > n_cus && resident_bytes > 64 * 1024));
    p.lds_table_floats = p.resident ? resident_floats : window_floats;
    // few channels: more threads each, so that a channel's epoch is spread over a whole CU (measured, 256 channels x 64
    // epochs on 256 CUs: 0.89 / 0.65 / 0.69 ms with 256 / 512 / 1024 threads); high-dynamics kernels: always 256 (the per-sample
    // exact rotator keeps a workgroup busy)
    p.threads = high_dyn ? 256 : forced_threads ? forced_threads : (2 * n_channels <= n_cus ? 1024 : n_channels <= 2 * n_cus ? 512 : 256);
    p.lds_bytes = (size_t)(trk_hdr_floats(p.threads) + p.lds_table_floats) * sizeof(float);
    return p;
}

#endif
