// trk_window_plan_selftest.cpp -- the multicorrelator's window plan (gnss-sdr-1_amd/csrc/trk_window_plan.h) on the host, compiled
// with g++ (-ffp-contract=off, like the kernels).  Of what it exercises the kernels run the chip-index helpers and the whole-chunk
// range (trk_whole_first / trk_whole_end: lc0, lc1); the rest states trk_epoch's formulas (see the header).  CPU only;
// tests/test_trk_window_plan.py drives it.
//
//   sweep     every (N, a, n_slices, off, samples behind the window, plain buffer / ring) of the ranges below, chunk 512, against the
//             conditions the kernel relies on; prints `sweep ok <plans>` or the first plan that breaks one and exits with 1.
//   records   reads one record per line from the standard input,
//               n_taps hdr words lds_floats L first_elem align_pairs sample_offset n_iq ring_len N n_slices step rem rate shift...
//             (first_elem: the address of the window's first sample in elements) and prints what trk_epoch decides for it,
//               a n_chunks lc0 lc1 full c0:c1:path ...
//             full: one 0 / 1 per chunk (`-` for none); one c0:c1:path per slice, path as tests/open_loop_matrix_cases.py names it.
#include "trk_window_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static const int CHUNK = 512;
typedef TrkChunkPlan<CHUNK> Plan;

static int fail(const char* what, unsigned long long off, unsigned long long end, unsigned ring, int a, int N, int slice, int n_slices, int c)
{
    std::printf("%s: off %llu end %llu ring_len %u a %d N %d slice %d of %d chunk %d\n", what, off, end, ring, a, N, slice, n_slices, c);
    return 1;
}

static int sweep()
{
    const int OFFS[] = {0, 1, 5, 15, 16, 600};
    const int BEHIND[] = {0, 1, 511, 512, 513, 100000};  // samples of the buffer behind the window's last one
    unsigned long long plans = 0;
    // what depends on (N, a) alone: the chunks cover the window's samples once, a chunk is full when all its positions are samples
    for (int N = 0; N <= 1100; N++)
        for (int a = 0; a < 16; a++)
            {
                const Plan w = trk_chunk_plan<CHUNK>(a, 1u << 20, a, N, 0, 1);
                if (w.V != N + a || w.c0 != 0 || w.c1 != w.n_chunks) return fail("one slice is not the window", a, 1u << 20, 0, a, N, 0, 1, -1);
                for (int n = 0; n < N; n++)
                    {
                        int holders = 0;
                        for (int c = 0; c < w.n_chunks; c++) holders += (c * CHUNK <= n + a && n + a < (c + 1) * CHUNK);
                        if (holders != 1) return fail("a sample is not in exactly one chunk", a, 1u << 20, 0, a, N, 0, 1, n);
                    }
                for (int c = 0; c < w.n_chunks; c++)
                    {
                        bool all = true;
                        for (int v = c * CHUNK; v < (c + 1) * CHUNK; v++) all = all && v >= a && v < w.V;
                        if (all != w.chunk_is_full(c)) return fail("chunk_is_full", a, 1u << 20, 0, a, N, 0, 1, c);
                    }
            }
    for (int ring = 0; ring < 2; ring++)
        for (int off_in : OFFS)
            for (int behind : BEHIND)
                for (int N = 0; N <= 1100; N++)
                    {
                        const unsigned long long n_iq = (unsigned long long)off_in + N + behind;
                        const unsigned ring_len = ring ? (unsigned)n_iq : 0u;
                        if (ring && !ring_len) continue;  // (ring_len 0 says "a plain buffer")
                        // a ring's sample_offset is absolute: the stream has wrapped three times
                        const unsigned long long off = trk_window_off((unsigned long long)off_in + 3ull * ring_len, ring_len);
                        const unsigned long long end = trk_window_end(n_iq, ring_len);
                        if (end != n_iq || off != (unsigned long long)off_in % (ring ? ring_len : ~0u)) return fail("off / end", off, end, ring_len, 0, N, 0, 1, -1);
                        for (int a = 0; a < 16; a++)
                            for (int n_slices = 1; n_slices <= 4; n_slices++)
                                {
                                    int next = 0;
                                    for (int s = 0; s < n_slices; s++)
                                        {
                                            const Plan w = trk_chunk_plan<CHUNK>(off, end, a, N, s, n_slices);
                                            plans++;
                                            // the slices' [c0, c1) partition [0, n_chunks) in order (slices past the last chunk are empty)
                                            if (w.c0 < w.c1)
                                                {
                                                    if (w.c0 != next || w.c1 > w.n_chunks) return fail("slices do not partition the chunks", off, end, ring_len, a, N, s, n_slices, w.c0);
                                                    next = w.c1;
                                                }
                                            else if (next != w.n_chunks)
                                                return fail("an empty slice before the last chunk", off, end, ring_len, a, N, s, n_slices, w.c0);
                                            for (int c = w.c0; c < w.c1; c++)
                                                {
                                                    if (w.loadable(c, false) != w.chunk_is_full(c)) return fail("loadable without WHOLE is not chunk_is_full", off, end, ring_len, a, N, s, n_slices, c);
                                                    if (w.chunk_is_full(c) && !w.loadable(c, true)) return fail("a full chunk is not loadable", off, end, ring_len, a, N, s, n_slices, c);
                                                    // memory safety of the whole-chunk fetch of a ragged chunk: all of it lies in the buffer
                                                    if (w.loadable(c, true) && !w.chunk_is_full(c))
                                                        {
                                                            const long long first = (long long)off - a + (long long)c * CHUNK;
                                                            if (first < 0 || first + CHUNK > (long long)end) return fail("a loadable ragged chunk leaves the buffer", off, end, ring_len, a, N, s, n_slices, c);
                                                        }
                                                }
                                            // the slice's samples: inside the window (a slice without chunks runs no loop: only n_lo <= n_hi)
                                            const int nmax = N > 0 ? N - 1 : 0;
                                            for (int hdr = 0; hdr < 2; hdr++)
                                                {
                                                    const TrkSampleRange r = trk_sample_range(w, hdr != 0);
                                                    if (r.n_lo > r.n_hi) return fail("n_lo > n_hi", off, end, ring_len, a, N, s, n_slices, hdr);
                                                    if ((w.c0 < w.c1 || hdr) && (r.n_lo < 0 || r.n_hi > nmax)) return fail("sample range outside the window", off, end, ring_len, a, N, s, n_slices, hdr);
                                                }
                                        }
                                    if (next != trk_chunk_plan<CHUNK>(off, end, a, N, 0, 1).n_chunks) return fail("chunks left over", off, end, ring_len, a, N, -1, n_slices, next);
                                }
                    }
    std::printf("sweep ok %llu\n", plans);
    return 0;
}

static const char* PATH_NAMES[] = {"window", "window_mod", "resident", "resident_mod", "lds_table", "global_table"};

template <int NTAPS>
static void record(const std::vector<double>& v)
{
    const bool hdr = v[1] != 0;
    const int words = (int)v[2], lds_floats = (int)v[3], L = (int)v[4], align_pairs = (int)v[6], N = (int)v[10], n_slices = (int)v[11];
    const unsigned long long first_elem = (unsigned long long)v[5], sample_offset = (unsigned long long)v[7], n_iq = (unsigned long long)v[8];
    const unsigned ring_len = (unsigned)v[9];
    const float step = (float)v[12], rem = (float)v[13], rate = (float)v[14];
    float shifts[NTAPS];
    for (int t = 0; t < NTAPS; t++) shifts[t] = (float)v[15 + t];
    const int a = trk_window_lead(first_elem, align_pairs);
    const unsigned long long off = trk_window_off(sample_offset, ring_len), end = trk_window_end(n_iq, ring_len);
    const Plan w0 = trk_chunk_plan<CHUNK>(off, end, a, N, 0, n_slices);
    std::string full;
    for (int c = 0; c < w0.n_chunks; c++) full += w0.chunk_is_full(c) ? '1' : '0';
    std::printf("%d %d %d %d %s", a, w0.n_chunks, w0.lc0, w0.lc1, full.empty() ? "-" : full.c_str());
    for (int s = 0; s < n_slices; s++)
        {
            const Plan w = trk_chunk_plan<CHUNK>(off, end, a, N, s, n_slices);
            const TrkCodeSpan span = trk_code_span(hdr, false, step, rem, rate, shifts, trk_sample_range(w, hdr));
            const TrkTablePlan t = trk_table_plan(span.lo, span.hi, span.monotone, words, false, L, lds_floats, false, true);
            std::printf(" %d:%d:%s", w.c0, w.c1, w.c0 < w.c1 ? PATH_NAMES[t.path] : "none");
        }
    std::printf("\n");
}

static int records()
{
    char line[4096];
    while (std::fgets(line, sizeof line, stdin))
        {
            std::vector<double> v;
            for (char* p = line; *p && *p != '\n';)
                {
                    char* e;
                    const double x = std::strtod(p, &e);
                    if (e == p) return 1;
                    v.push_back(x);
                    p = e;
                    while (*p == ' ') p++;
                }
            if (v.size() < 16 || v[0] < 1 || v[0] > 8 || v.size() != 15 + (size_t)v[0] || v[11] < 1 || v[6] < 1) return 1;
            switch ((int)v[0])
                {
                case 1: record<1>(v); break;
                case 2: record<2>(v); break;
                case 3: record<3>(v); break;
                case 4: record<4>(v); break;
                case 5: record<5>(v); break;
                case 6: record<6>(v); break;
                case 7: record<7>(v); break;
                default: record<8>(v); break;
                }
        }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
    if (argc == 2 && std::strcmp(argv[1], "records") == 0) return records();
    return 1;
}
