// acq_plan.h -- the host-side planner of the PCPS acquisition transforms, for host and device.
//
// An N-point FFT runs as N = N1 x N2 (acq_kernels.hip): acq_plan_make picks N1 among the instantiated column sizes and factor_rows
// the radices of the N2-point row FFT, from N alone.  Together with acq_cols_perm_map -- which of its two store mappings a forward
// column epilogue takes -- that decides which kernel instances a receiver's sampling rate runs.  The header compiles without HIP
// (tests/acq_plan_selftest.cpp prints the plan of any size; tests/test_acq_plan.py holds tests/acq_plan_ref.py to it and guards
// what the acquisition size matrix covers).  The planner's functions are DEFINED where ACQ_PLAN_DEFINE is set before the
// include -- acq_kernels.hip for the library, which exports them, and the self-test -- and declared everywhere else.
#ifndef ACQ_PLAN_H
#define ACQ_PLAN_H
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define ACQ_PLAN_HD __host__ __device__
#else
#define ACQ_PLAN_HD
struct float2
{
    float x, y;
};
static inline float2 make_float2(float x, float y)
{
    float2 v = {x, y};
    return v;
}
#endif

#define ACQ_MAX_FACTORS 12
#define ACQ_MAX_N1 64
#define ACQ_THREADS 256

// N-point FFT as N = N1 x N2: N2-point row FFTs in LDS, N1-point column DFTs in registers
struct AcqFftPlan
{
    int N, N1, N2;
    int n_fac;
    int fac[ACQ_MAX_FACTORS];  // radices of the N2-point row FFT, product = N2
    int tw_off[ACQ_MAX_FACTORS];  // offset of each stage's twiddle table inside the stage-twiddle array
    float2 w1[ACQ_MAX_N1];     // exp(-2*pi*j*k/N1), k < N1
};

bool acq_plan_make(AcqFftPlan* plan, int N, size_t lds_limit_bytes);
size_t acq_rows_lds_bytes(const AcqFftPlan& plan);
int acq_cols_blocks(const AcqFftPlan& plan);

// The second store mapping of the row-permuted (forward) column epilogues, acq_cols_body: where N2 is a multiple of N1 J
// (J = ACQ_THREADS / N1 column groups per block, pj here) and the blocks tile N2 exactly, a block takes columns N1 j + r instead of
// 256 consecutive ones
static ACQ_PLAN_HD inline bool acq_cols_perm_map(int n1, int pj, int N2, int n_xblk)
{
    return n1 > 1 && pj >= 4 && (N2 % (n1 * pj)) == 0 && n_xblk * (n1 * pj) == N2;
}

#ifdef ACQ_PLAN_DEFINE
static bool factor_rows(int N2, int* fac, int* n_fac)
{
    int n = N2, k = 0;
    const int pref[] = {16, 10, 8, 5, 4, 3, 2};
    while (n > 1)
        {
            int r = 0;
            for (int p : pref)
                if (n % p == 0)
                    {
                        r = p;
                        break;
                    }
            if (!r)
                {
                    // any other prime factor: the generic O(R^2) butterfly (slow for large R, but every length the
                    // LDS can hold is transformed -- the reference's FFTW takes any length)
                    for (int p = 7; (long)p * p <= n; p += 2)
                        if (n % p == 0)
                            {
                                r = p;
                                break;
                            }
                    if (!r) r = n;  // n itself is prime
                }
            if (!r || k >= ACQ_MAX_FACTORS) return false;
            fac[k++] = r;
            n /= r;
        }
    *n_fac = k;
    return true;
}

size_t acq_rows_lds_bytes(const AcqFftPlan& plan) { return (size_t)2 * plan.N2 * sizeof(float2); }

bool acq_plan_make(AcqFftPlan* plan, int N, size_t lds_limit_bytes)
{
    std::memset(plan, 0, sizeof *plan);
    if (N < 1) return false;
    // N1 candidates (register DFT sizes that are instantiated); prefer rows of ~1000-2000 points:
    // long enough to occupy a 256-thread workgroup, short enough for several workgroups per CU
    const int cands[] = {1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16, 20, 25, 32, 40, 50};  // 32-50: blocks of 256 k - 512 k samples
    int best = 0;
    long best_cost = -1;
    for (int n1 : cands)
        {
            if (N % n1) continue;
            int n2 = N / n1;
            if ((size_t)2 * n2 * sizeof(float2) > lds_limit_bytes) continue;
            int fac[ACQ_MAX_FACTORS], nf;
            if (!factor_rows(n2, fac, &nf)) continue;
            long cost = labs((long)n2 - 1024);
            if (best_cost < 0 || cost < best_cost)
                {
                    best_cost = cost;
                    best = n1;
                }
        }
    if (!best) return false;
    plan->N = N;
    plan->N1 = best;
    plan->N2 = N / best;
    factor_rows(plan->N2, plan->fac, &plan->n_fac);
    {
        // offsets of the per-stage twiddle tables [k-1][q] (sizes sum to N2 - 1)
        int n = plan->N2, off = 0;
        for (int f = 0; f < plan->n_fac; f++)
            {
                const int R = plan->fac[f], m = n / R;
                plan->tw_off[f] = off;
                off += (R - 1) * m;
                n = m;
            }
    }
    for (int k = 0; k < best; k++)
        {
            double a = -2.0 * M_PI * (double)k / (double)best;
            plan->w1[k] = make_float2((float)cos(a), (float)sin(a));
        }
    return true;
}

int acq_cols_blocks(const AcqFftPlan& plan) { return (plan.N2 + ACQ_THREADS - 1) / ACQ_THREADS; }
#endif  // ACQ_PLAN_DEFINE

#endif
