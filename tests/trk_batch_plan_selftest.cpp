// trk_batch_plan_selftest.cpp -- the open-loop tracking launches' plan (gnss-sdr-1_amd/csrc/trk_batch_plan.h) on the host.  Every
// argument is one launch:
//   forced_slices,lds_sizing,n_epochs,n_cus,format,small_window_ok,len,max_step,table_floats/COUNTxL,shift,shift,.../COUNTxL,shift,...
// -- behind each '/' COUNT channels with a code of L chips and these tap shifts (every group has the first group's tap count);
// format is the kernel's TRK_MODE_* number (0 plain, 2 high-dynamics, 3 complex chips, 4 16-bit) -- and prints `n_slices lds_floats`;
// or `l1:N,one_wg_max,partial_slices`, which prints the slice count of a level-1 call.  CPU only; tests/test_trk_batch_plan.py holds
// the expected lines.
// Built with -DTRK_SELFTEST_TRAITS (and the HIP headers on the include path, for trk_kernels.h) the argument `traits` prints what
// decides which instantiations of trk_multicorrelator_kernel a caller can reach: `max_taps GC_MAX_TAPS`, then one line per TRK_MODE_*,
// `mode iq_formats words_per_chip out_bytes` (iq_formats: bits 1 << gc_iq_format).  tests/open_loop_matrix_cases.py reads them.
#include "trk_batch_plan.h"
#ifdef TRK_SELFTEST_TRAITS
#include "trk_kernels.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Chan  // laid out like a channel descriptor: the plan walks one array
{
    int code_len;
    float shifts[8];
};

static std::vector<double> numbers(char* p, char** end)
{
    std::vector<double> v;
    while (*p && *p != '/')
        {
            v.push_back(std::strtod(p, &p));
            if (*p == ',' || *p == 'x') p++;
        }
    *end = p;
    return v;
}

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; a++)
        {
            char* p = argv[a];
#ifdef TRK_SELFTEST_TRAITS
            if (std::strcmp(p, "traits") == 0)
                {
                    std::printf("max_taps %d\n", GC_MAX_TAPS);
                    for (int m = TRK_MODE_PLAIN; m <= TRK_MODE_SC16; m++)
                        std::printf("%d %u %d %d\n", m, TRK_FORMAT_TRAITS[m].iq_formats, TRK_FORMAT_TRAITS[m].words_per_chip, TRK_FORMAT_TRAITS[m].out_bytes);
                    continue;
                }
#endif
            if (std::strncmp(p, "l1:", 3) == 0)
                {
                    const std::vector<double> v = numbers(p + 3, &p);
                    if (v.size() != 3) return 1;
                    std::printf("%d\n", trk_level1_slices((int)v[0], (int)v[1], (int)v[2]));
                    continue;
                }
            const std::vector<double> v = numbers(p, &p);
            if (v.size() != 9 || v[4] < 0 || v[4] > 4) return 1;
            std::vector<Chan> chans;
            size_t n_taps = 0;
            while (*p == '/')
                {
                    const std::vector<double> g = numbers(p + 1, &p);
                    if (g.size() < 3 || g.size() > 10 || g[0] < 1) return 1;
                    if (!n_taps) n_taps = g.size() - 2;
                    if (g.size() - 2 != n_taps) return 1;
                    Chan c = {(int)g[1], {}};
                    for (size_t t = 0; t < n_taps; t++) c.shifts[t] = (float)g[2 + t];
                    chans.insert(chans.end(), (size_t)g[0], c);
                }
            if (chans.empty()) return 1;
            const TrkBatchPlan plan = trk_batch_plan((int)v[0], v[1] != 0, (int)chans.size(), (int)v[2], (int)v[3], (int)v[4], v[5] != 0, (int)v[6], &chans[0].code_len,
                chans[0].shifts, (int)(sizeof(Chan) / 4), (int)n_taps, (float)v[7], (int)v[8]);
            std::printf("%d %d\n", plan.n_slices, plan.lds_floats);
        }
    return 0;
}
