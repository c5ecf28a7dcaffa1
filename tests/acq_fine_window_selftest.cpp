// acq_fine_window_selftest.cpp -- the rules of the fine Doppler stage shared by host and device (csrc/acq_fine_window.h) against
// hand-made values: the float32 frequency table, window runs (among them runs that cross from index Next - 1 to 0, one-bin and empty
// windows), the replica index map of both alignments, the 64-bit phase index and the argument checks.  Stand-alone: its own main, no
// GPU, built with -fsanitize=address,undefined by tests/test_fine_doppler_abi.py.
#include "acq_fine_window.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;

#define CHECK(cond)                                                   \
    do                                                                \
        {                                                             \
            if (!(cond))                                              \
                {                                                     \
                    std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
                    failures++;                                       \
                }                                                     \
        }                                                             \
    while (0)

static void window_is(int64_t fs, uint32_t next, double fc, double w, uint32_t want_lo, uint32_t want_count)
{
    uint32_t lo = 0, count = 0;
    fine_window(fs, next, fc, w, &lo, &count);
    if (count != want_count || (count && lo != want_lo))
        {
            std::printf("FAIL window fs %lld next %u fc %g w %g: (%u, %u), expected (%u, %u)\n", (long long)fs, next, fc, w, lo, count, want_lo, want_count);
            failures++;
        }
    // brute force over the whole table: the same members, and the run is contiguous
    std::vector<char> in(next, 0);
    uint32_t total = 0;
    for (uint32_t k = 0; k < next; k++)
        {
            in[k] = std::fabs((double)fine_freq(k, fs, next) - fc) < w;
            total += in[k];
        }
    if (total != count)
        {
            std::printf("FAIL window fs %lld next %u fc %g w %g: %u members by brute force, %u in the run\n", (long long)fs, next, fc, w, total, count);
            failures++;
        }
    for (uint32_t b = 0; b < count; b++)
        if (!in[(lo + b) % next])
            {
                std::printf("FAIL window fs %lld next %u fc %g: run entry %u is no member\n", (long long)fs, next, fc, b);
                failures++;
                break;
            }
}

static void map_is(uint32_t n, uint32_t s, int alignment, const std::vector<uint32_t>& want)
{
    for (uint32_t i = 0; i < n; i++)
        if (fine_replica_src(i, n, s, alignment) != want[i])
            {
                std::printf("FAIL map n %u s %u alignment %d at %u: %u, expected %u\n", n, s, alignment, i, fine_replica_src(i, n, s, alignment), want[i]);
                failures++;
                return;
            }
}

int main()
{
    // the table: 12.5 Hz bins at 4 Msps, 10 x 4000 x 8
    CHECK(fine_freq(0, 4000000, 320000) == 0.0f);
    CHECK(fine_freq(1, 4000000, 320000) == 12.5f);
    CHECK(fine_freq(159999, 4000000, 320000) == 1999987.5f);
    CHECK(fine_freq(160000, 4000000, 320000) == -2000000.0f);
    CHECK(fine_freq(319999, 4000000, 320000) == -12.5f);
    CHECK(fine_freq(3, 6625000, 530000) == 37.5f);
    // rounded once, from double: 1e6 / 3 Hz bins
    CHECK(fine_freq(1, 2000000, 6) == (float)(1000000.0 / 3.0));
    CHECK(fine_freq(5, 2000000, 6) == (float)(-1000000.0 / 3.0));

    // windows: (fs, Next, coarse, width) -> (first bin, bins)
    window_is(4000000, 320000, 0.0, 1000.0, 319921, 159);
    window_is(4000000, 320000, 500.0, 1000.0, 319961, 159);
    window_is(4000000, 320000, -500.0, 1000.0, 319881, 159);
    window_is(4000000, 320000, 2500.0, 1000.0, 121, 159);
    window_is(4000000, 320000, -4500.0, 1000.0, 319561, 159);
    window_is(4000000, 320000, 4500.0, 1000.0, 281, 159);
    window_is(4000000, 320000, 1000.0, 1000.0, 1, 159);          // 0 Hz is exactly 1 kHz away: outside
    window_is(4000000, 320000, 6.25, 1000.0, 319921, 160);        // half a bin up: one more member
    window_is(2000000, 2000, 0.0, 1000.0, 0, 1);                  // 1 kHz bins: 0 Hz alone
    window_is(2000000, 2000, 500.0, 1000.0, 0, 2);
    window_is(2000000, 2000, -500.0, 1000.0, 1999, 2);
    window_is(2000000, 2000, -4500.0, 1000.0, 1995, 2);
    window_is(2000000, 16000, 2500.0, 1000.0, 13, 15);            // 4 x 2000 x 2: 125 Hz bins
    window_is(2000000, 4000, 250.0, 100.0, 0, 0);                 // between two 500 Hz bins: empty
    window_is(2000000, 2000, 998000.0, 1000.0, 998, 1);           // just below Nyquist
    window_is(2000000, 2000, -998500.0, 1000.0, 1001, 2);
    window_is(16000000, 1u << 24, 0.0, 10.0, (1u << 24) - 10, 21);  // the largest table: bins of 0.95 Hz

    // the replica index map on N = 8
    map_is(8, 0, FINE_ALIGN_REFERENCE, {0, 1, 2, 3, 4, 5, 6, 7});
    map_is(8, 1, FINE_ALIGN_REFERENCE, {0, 1, 2, 3, 4, 5, 6, 7});  // std::rotate(r, r + 7, r + 7): nothing moves
    map_is(8, 2, FINE_ALIGN_REFERENCE, {6, 0, 1, 2, 3, 4, 5, 7});
    map_is(8, 3, FINE_ALIGN_REFERENCE, {5, 6, 0, 1, 2, 3, 4, 7});
    map_is(8, 7, FINE_ALIGN_REFERENCE, {1, 2, 3, 4, 5, 6, 0, 7});
    map_is(8, 0, FINE_ALIGN_EXACT, {0, 1, 2, 3, 4, 5, 6, 7});
    map_is(8, 1, FINE_ALIGN_EXACT, {7, 0, 1, 2, 3, 4, 5, 6});
    map_is(8, 3, FINE_ALIGN_EXACT, {5, 6, 7, 0, 1, 2, 3, 4});
    map_is(8, 7, FINE_ALIGN_EXACT, {1, 2, 3, 4, 5, 6, 7, 0});
    map_is(1, 0, FINE_ALIGN_REFERENCE, {0});
    map_is(1, 0, FINE_ALIGN_EXACT, {0});

    // the phase index, reduced in 64 bits
    CHECK(fine_phase_index(37, 1024, 160000) == 37888);
    CHECK(fine_phase_index(319999, 249999, 320000) == 70001);                // (-1)(-249999)
    CHECK(fine_phase_index((1u << 24) - 1, (1u << 24) - 1, 1u << 24) == 1);  // the product needs 48 bits
    CHECK(fine_phase_index(0, 12345, 320000) == 0);
    CHECK(fine_phase_index(160000, 3, 320000) == 160000);

    // argument checks
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(fine_sizes_ok(4000000, 320000) && fine_sizes_ok(1, 2) && fine_sizes_ok(16000000, 1u << 24));
    CHECK(!fine_sizes_ok(4000000, 6625) && !fine_sizes_ok(4000000, 0) && !fine_sizes_ok(0, 320000) && !fine_sizes_ok(4000000, (1u << 24) + 2));
    CHECK(fine_window_ok(4000000, 0.0, 1000.0) && fine_window_ok(4000000, -1998999.0, 1000.0));
    CHECK(!fine_window_ok(4000000, 1999000.0, 1000.0) && !fine_window_ok(4000000, -1999000.0, 1000.0));
    CHECK(!fine_window_ok(4000000, 0.0, 0.0) && !fine_window_ok(4000000, 0.0, -1.0) && !fine_window_ok(4000000, 0.0, inf) && !fine_window_ok(4000000, 0.0, nan));
    CHECK(!fine_window_ok(4000000, nan, 1000.0) && !fine_window_ok(4000000, inf, 1000.0) && !fine_window_ok(4000000, -inf, 1000.0));
    CHECK(fine_window_max_bins(4000000, 320000, 1000.0) >= 160);

    if (failures) return 1;
    std::printf("all windows, maps and phase indices as expected\n");
    return 0;
}
