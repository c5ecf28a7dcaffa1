// acq_plan_selftest.cpp -- the acquisition planner (gnss-sdr-1_amd/csrc/acq_plan.h) on the host: for every FFT size on the command
// line, one line `N N1 N2 radices perm_map` (radices joined by 'x'; perm_map 0 / 1: the store mapping of the forward column
// epilogues), or `N none` where acq_plan_make refuses the size.  The LDS limit is gc_acq_create's.  CPU only;
// tests/test_acq_plan.py compares the lines with tests/acq_plan_ref.py.
#define ACQ_PLAN_DEFINE
#include "acq_plan.h"
#include <cstdio>

int main(int argc, char** argv)
{
    const size_t lds_limit = 160 * 1024;
    for (int i = 1; i < argc; i++)
        {
            const int N = std::atoi(argv[i]);
            AcqFftPlan plan;
            if (!acq_plan_make(&plan, N, lds_limit))
                {
                    std::printf("%d none\n", N);
                    continue;
                }
            if (plan.N != N || plan.N1 * plan.N2 != N || acq_rows_lds_bytes(plan) > lds_limit) return 1;
            std::printf("%d %d %d ", N, plan.N1, plan.N2);
            for (int f = 0; f < plan.n_fac; f++) std::printf(f ? "x%d" : "%d", plan.fac[f]);
            if (plan.n_fac == 0) std::printf("1");
            std::printf(" %d\n", acq_cols_perm_map(plan.N1, ACQ_THREADS / plan.N1, plan.N2, acq_cols_blocks(plan)) ? 1 : 0);
        }
    return 0;
}
