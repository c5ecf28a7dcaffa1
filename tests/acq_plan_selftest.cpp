// acq_plan_selftest.cpp -- the acquisition planner (gnss-sdr-1_amd/csrc/acq_plan.h) on the host: for every FFT size on the command
// line, one line `N N1 N2 radices perm_map rows` (radices joined by 'x'; perm_map 0 / 1: the store mapping of the forward column
// epilogues; rows: the row kernel, `RxI,...,RxI/rpw` -- radix x butterflies per thread of every stage and the rows per workgroup --
// or `general`), or `N none` where acq_plan_make refuses the size.  `--range A B` takes every size from A to B, `--rpw-cap C` caps
// the rows per workgroup for the sizes behind it, `--n1` prints the column sizes and `--registry` the stage lists, one per line.
// The LDS limit is gc_acq_create's.  CPU only; tests/test_acq_plan.py compares the lines with tests/acq_plan_ref.py.
#define ACQ_PLAN_DEFINE
#include "acq_plan.h"
#include <cstdio>

static void print_stages(const int* radix, const int* iters, int n)
{
    for (int f = 0; f < n; f++) std::printf(f ? ",%dx%d" : "%dx%d", radix[f], iters[f]);
}

static bool print_plan(int N, int rpw_cap)
{
    const size_t lds_limit = 160 * 1024;
    AcqFftPlan plan;
    if (!acq_plan_make(&plan, N, lds_limit)) return std::printf("%d none\n", N) > 0;
    if (plan.N != N || plan.N1 * plan.N2 != N || acq_rows_lds_bytes(plan) > lds_limit) return false;
    std::printf("%d %d %d ", N, plan.N1, plan.N2);
    for (int f = 0; f < plan.n_fac; f++) std::printf(f ? "x%d" : "%d", plan.fac[f]);
    if (plan.n_fac == 0) std::printf("1");
    std::printf(" %d ", acq_cols_perm_map(plan.N1, ACQ_THREADS / plan.N1, plan.N2, acq_cols_blocks(plan)) ? 1 : 0);
    const AcqRowsPlan rows = acq_rows_plan_make(plan, rpw_cap);
    if (rows.entry < 0) return std::printf("general\n") > 0;
    print_stages(plan.fac, rows.iters, plan.n_fac);
    return std::printf("/%d\n", rows.rpw) > 0;
}

int main(int argc, char** argv)
{
    int rpw_cap = 0;
    for (int i = 1; i < argc; i++)
        {
            if (!std::strcmp(argv[i], "--n1"))
                {
#define PRINT_N1(K) std::printf("%d\n", K);
                    ACQ_N1_LIST(PRINT_N1)
                }
            else if (!std::strcmp(argv[i], "--registry"))
                for (const AcqRows2Stages& e : acq_rows2_stages)
                    {
                        int radix[4], iters[4], n = 0;
                        for (; n < 4 && e.ri[n]; n++) radix[n] = e.ri[n] / 16, iters[n] = e.ri[n] % 16;
                        print_stages(radix, iters, n);
                        std::printf("\n");
                    }
            else if (!std::strcmp(argv[i], "--rpw-cap") && i + 1 < argc)
                rpw_cap = std::atoi(argv[++i]);
            else if (!std::strcmp(argv[i], "--range") && i + 2 < argc)
                {
                    for (int N = std::atoi(argv[i + 1]); N <= std::atoi(argv[i + 2]); N++)
                        if (!print_plan(N, rpw_cap)) return 1;
                    i += 2;
                }
            else if (argv[i][0] == '-' || !print_plan(std::atoi(argv[i]), rpw_cap))
                return 1;
        }
    return 0;
}
