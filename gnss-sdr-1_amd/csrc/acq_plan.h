// acq_plan.h -- the host-side planner of the PCPS acquisition transforms, for host and device.
//
// An N-point FFT runs as N = N1 x N2 (acq_kernels.hip): acq_plan_make picks N1 among the instantiated column sizes and factor_rows
// the radices of the N2-point row FFT, from N alone.  Together with acq_cols_perm_map -- which of its two store mappings a forward
// column epilogue takes -- that decides which kernel instances a receiver's sampling rate runs.  The header compiles without HIP
// (tests/acq_plan_selftest.cpp prints the plan of any size; tests/test_acq_plan.py holds tests/acq_plan_ref.py to it and guards
// what the acquisition size matrix covers).  acq_rows_plan_make then picks the row kernel of a plan: an entry of ACQ_ROWS2_LIST,
// the stage lists acq_kernels.hip instantiates the packed row kernel for, or the general kernel.  The planner's functions are
// DEFINED where ACQ_PLAN_DEFINE is set before the include -- acq_kernels.hip for the library, which exports them, and the
// self-test -- and declared everywhere else.
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
// the column sizes N1 (register DFT sizes): acq_plan_make picks among them, acq_kernels.hip instantiates a column kernel for each
#define ACQ_N1_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8) X(9) X(10) X(12) X(15) X(16) X(20) X(25) X(32) X(40) X(50)

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

// The packed row kernel (acq_rows2_kernel) is instantiated per stage list: one ACQ_R2(radix, butterflies per thread) per stage, as
// acq_rows2_config derives them for the row lengths the planner picks for 1/2/4/8 ms blocks at 2 ... 25 Msps (and the power-of-two
// sizes).  A list that differs from what acq_rows2_config derives is never selected: its sizes run the general kernel.
#define ACQ_ROWS2_POINTS 20        // R * ITER: points a thread holds per stage
#define ACQ_ROWS2_LDS_BYTES 40000  // rows * N2 * 8 per workgroup: four workgroups per CU
#define ACQ_R2(r, i) ((r) * 16 + (i))
#define ACQ_ROWS2_LIST(X)                                                                                       \
    X(ACQ_R2(10, 2), ACQ_R2(10, 2), ACQ_R2(10, 2))                /* 1000: N = 2000 ... 25000 (planar pair kernel) */ \
    X(ACQ_R2(10, 1), ACQ_R2(10, 1), ACQ_R2(10, 1))                /* 1000, at most 2 rows per workgroup */             \
    X(ACQ_R2(16, 1), ACQ_R2(16, 1), ACQ_R2(4, 4))                 /* 1024 */                                           \
    X(ACQ_R2(10, 2), ACQ_R2(5, 4), ACQ_R2(5, 4), ACQ_R2(5, 4))    /* 1250: N = 2500, 6250, 12500 */                    \
    X(ACQ_R2(16, 1), ACQ_R2(16, 1), ACQ_R2(5, 4))                 /* 1280: N = 32000 */                                \
    X(ACQ_R2(16, 1), ACQ_R2(16, 1), ACQ_R2(8, 2))                 /* 2048 */                                           \
    X(ACQ_R2(16, 1), ACQ_R2(10, 2), ACQ_R2(10, 2))                /* 1600: N = 40000 */                                \
    X(ACQ_R2(16, 1), ACQ_R2(5, 4), ACQ_R2(5, 4), ACQ_R2(5, 4))    /* 2000: N = 50000 */                                \
    X(ACQ_R2(16, 1), ACQ_R2(16, 1), ACQ_R2(10, 1))                /* 2560: N = 64000 */                                \
    X(ACQ_R2(16, 1), ACQ_R2(16, 1), ACQ_R2(16, 1))                /* 4096 */                                           \
    X(ACQ_R2(16, 1), ACQ_R2(10, 2), ACQ_R2(5, 4), ACQ_R2(5, 4))   /* 4000: N = 100000 */                               \
    X(ACQ_R2(16, 1), ACQ_R2(10, 2), ACQ_R2(3, 4), ACQ_R2(2, 8))   /* 960: N = 24000 */                                 \
    X(ACQ_R2(16, 1), ACQ_R2(10, 2), ACQ_R2(10, 2), ACQ_R2(2, 8))  /* 3200: N = 80000 */
#define ACQ_ROWS2_PAIR_ENTRY 0  // the list that has planar pair kernels as well (acq_rows3_kernel)

// the row kernel of a plan: `entry` indexes ACQ_ROWS2_LIST, -1 is the general kernel (acq_rows_kernel: any radix, one row per
// workgroup); rows per workgroup and butterflies per thread of every stage where entry >= 0
struct AcqRowsPlan
{
    int entry, rpw;
    int iters[4];
};
AcqRowsPlan acq_rows_plan_make(const AcqFftPlan& plan, int rpw_cap /* tuning: most rows per workgroup, 0: no cap */);

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
#define ACQ_PLAN_ITEM(K) K,
    const int cands[] = {ACQ_N1_LIST(ACQ_PLAN_ITEM)};  // 32-50: blocks of 256 k - 512 k samples
#undef ACQ_PLAN_ITEM
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

struct AcqRows2Stages
{
    int ri[4];  // ACQ_R2 of every stage, then zeros
};
#define ACQ_PLAN_ITEM(...) {{__VA_ARGS__}},
static const AcqRows2Stages acq_rows2_stages[] = {ACQ_ROWS2_LIST(ACQ_PLAN_ITEM)};
#undef ACQ_PLAN_ITEM

// rows per workgroup and per-stage butterflies per thread for the packed kernel; false: use acq_rows_kernel
static bool acq_rows2_config(const AcqFftPlan& plan, int rpw_cap, int* rpw_out, int* iters)
{
    const int radices_ok[] = {2, 3, 4, 5, 8, 10, 16};
    for (int f = 0; f < plan.n_fac; f++)
        {
            bool ok = false;
            for (int r : radices_ok) ok = ok || (plan.fac[f] == r);
            if (!ok) return false;
        }
    if ((size_t)plan.N2 * sizeof(float2) > 64 * 1024) return false;
    int rpw = (int)(ACQ_ROWS2_LDS_BYTES / ((size_t)plan.N2 * sizeof(float2)));
    if (rpw < 1) rpw = 1;
    if (rpw > 16) rpw = 16;
    if (rpw_cap > 0 && rpw > rpw_cap) rpw = rpw_cap;
    for (; rpw >= 1; rpw--)
        {
            bool fits = true;
            for (int f = 0; f < plan.n_fac && fits; f++)
                {
                    const int R = plan.fac[f], nb = plan.N2 / R;
                    const int need = (rpw * nb + ACQ_THREADS - 1) / ACQ_THREADS;
                    int it = 1;
                    while (it < need) it *= 2;
                    if (it * R > ACQ_ROWS2_POINTS || it > 8) fits = false;
                    iters[f] = it;
                }
            if (fits)
                {
                    *rpw_out = rpw;
                    return true;
                }
        }
    return false;
}

AcqRowsPlan acq_rows_plan_make(const AcqFftPlan& plan, int rpw_cap)
{
    AcqRowsPlan rows = {-1, 0, {0, 0, 0, 0}};
    int rpw, iters[ACQ_MAX_FACTORS];
    if (plan.n_fac > 4 || !acq_rows2_config(plan, rpw_cap, &rpw, iters)) return rows;
    for (int e = 0; e < (int)(sizeof acq_rows2_stages / sizeof acq_rows2_stages[0]); e++)
        {
            bool same = true;
            for (int f = 0; f < 4 && same; f++) same = acq_rows2_stages[e].ri[f] == (f < plan.n_fac ? ACQ_R2(plan.fac[f], iters[f]) : 0);
            if (same) rows.entry = e;  // the last matching list
        }
    if (rows.entry < 0) return rows;  // a configuration no instance was built for
    rows.rpw = rpw;
    for (int f = 0; f < plan.n_fac; f++) rows.iters[f] = iters[f];
    return rows;
}
#endif  // ACQ_PLAN_DEFINE

#endif
