// resamp_index_selftest -- prints what gnss-sdr-1_amd/csrc/resamp_index.h computes, for tests/test_resamp_index.py to compare with
// Python's exact integers and with an emulation of the reference's Direct_Resampler.  Host code only.
//
//   resamp_index_selftest direct|poly fs_in fs_out log2_phases taps request...
//
// First line: "ratio <kind> <step>".  Requests, each answered by lines that begin with its letter:
//   m:<first>:<count>   "m <m> <n_m> <p_m>"                         for count outputs from first
//   h:<H>               "h <H> <outputs available>"
//   b:<m0>:<count>      "b <m0> <q0> <r0> <fits>" and "j <j> <n> <p>"  for the launch base at m0 and its first count offsets
//   f:<m0>              "f <m0> <read-ticket floor>"
#include "resamp_index.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const bool poly = std::strcmp(argv[1], "poly") == 0;
    const double fs_in = std::atof(argv[2]), fs_out = std::atof(argv[3]);
    const int log2_phases = std::atoi(argv[4]), taps = std::atoi(argv[5]);
    const ResampRatio r = poly ? resamp_poly_ratio(fs_in, fs_out) : resamp_direct_ratio(fs_in, fs_out);
    std::printf("ratio %d %llu\n", r.kind, (unsigned long long)r.step);
    for (int a = 6; a < argc; a++)
        {
            const char kind = argv[a][0];
            char* p = argv[a] + 2;
            const unsigned long long v0 = std::strtoull(p, &p, 10);
            const unsigned long long v1 = *p == ':' ? std::strtoull(p + 1, &p, 10) : 0;
            if (kind == 'm')
                for (unsigned long long m = v0; m < v0 + v1; m++)
                    std::printf("m %llu %llu %u\n", m, (unsigned long long)resamp_source_index(r, m), poly ? resamp_phase(r, log2_phases, m) : 0u);
            else if (kind == 'h')
                std::printf("h %llu %llu\n", v0, (unsigned long long)resamp_available(r, v0));
            else if (kind == 'b')
                {
                    const ResampBase b = resamp_base(r, v0);
                    std::printf("b %llu %llu %llu %d\n", v0, (unsigned long long)b.q0, (unsigned long long)b.r0, (int)resamp_offsets_fit(r, b, v1));
                    for (unsigned long long j = 0; j < v1; j++)
                        std::printf("j %llu %llu %u\n", j, (unsigned long long)resamp_offset_index(r.kind, r.step, b.q0, b.r0, j),
                            poly ? resamp_offset_phase(r.step, log2_phases, b.r0, j) : 0u);
                }
            else if (kind == 'f')
                std::printf("f %llu %llu\n", v0, (unsigned long long)resamp_floor(r, taps, v0));
            else
                return 2;
        }
    return 0;
}
