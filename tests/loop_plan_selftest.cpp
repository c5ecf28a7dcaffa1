// loop_plan_selftest.cpp -- the closed loop's launch plan (gnss-sdr-1_amd/csrc/trk_loop_plan.h) on the host.  Every argument is one
// engine: `channels,cus,high_dyn,forced_threads,mixed,max_code_len,pilot` and then, for a mixed engine, one `length/pilot/started`
// per channel slot from slot 0 on (the remaining slots are empty and not started).  Prints one line per engine:
// `threads lds_table_floats resident lds_bytes`.  CPU only; tests/test_loop_plan.py holds the expected lines.
#include "trk_loop_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; a++)
        {
            std::vector<long> v;
            for (char* p = argv[a]; *p;)
                {
                    v.push_back(std::strtol(p, &p, 10));
                    if (*p) p++;  // ',' or '/'
                }
            if (v.size() < 7 || (v.size() - 7) % 3 != 0 || v[0] < 1 || (v.size() - 7) / 3 > (size_t)v[0]) return 1;
            const int n = (int)v[0];
            std::vector<int> code_len(n, 0);
            std::vector<char> track_pilot(n, 0), started(n, 0);
            for (size_t i = 0; 7 + 3 * i < v.size(); i++)
                {
                    code_len[i] = (int)v[7 + 3 * i];
                    track_pilot[i] = (char)v[8 + 3 * i];
                    started[i] = (char)v[9 + 3 * i];
                }
            const TrkLoopPlan p = trk_loop_plan(n, (int)v[1], v[2] != 0, (int)v[3], v[4] != 0, started.data(), code_len.data(), track_pilot.data(), (int)v[5], v[6] != 0);
            std::printf("%d %d %d %zu\n", p.threads, p.lds_table_floats, p.resident, p.lds_bytes);
        }
    return 0;
}
